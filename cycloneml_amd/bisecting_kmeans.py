"""BisectingKMeans (mllib/clustering/BisectingKMeans.scala,
BisectingKMeansModel.scala and ml/clustering/BisectingKMeans.scala, Spark 3.3)
over dense fp64 device rows, Euclidean measure, optional row weights.  The
kernels are csrc/bisecting_kmeans.hip (cyc_bkm_* in include/cyclone.h).

Node indices: ROOT = 1, left(i) = 2 i, right(i) = 2 i + 1.  A cluster's summary
over its rows is n, weightSum = sum w, sumSq = sum (norm norm) w and sum = sum w
x; center = sum * (1 / weightSum), cost = max(sumSq - weightSum |center|
|center|, 0), size = n.

Fit (fit_clusters).  Every row starts in ROOT.  Per level the divisible active
clusters (size >= minSize, cost > 2^-52 size; at most the `needed` largest) get
two children center -+ 1e-4 |center| noise, noise from java.util.Random(seed);
maxIter times every row of a divisible cluster picks the closer child on offer
by findClosest and the picked children are summarised (a child without rows
vanishes and its sibling is offered alone); one more pass moves the rows.  The
tree (build_tree) is a depth-first walk: a node is internal iff its left child
is among the clusters.

This project's own rules: divisible clusters are visited in ascending node
index (the order of the random draws; ties of size in the "largest" selection
go to the lower index), where Spark walks a Scala Map -- beyond four entries
that is the hash trie's order, so a fit that splits five or more clusters at
one level does not reproduce a Spark run's draws.  Rows with a non-finite norm
and weights that are not finite and positive are refused, naming the lowest
such row.  k >= 1, maxIter >= 0, minDivisibleClusterSize > 0.  maxIter = 0
takes no summaries, so nothing below the root is kept.  CSRRows and
distanceMeasure = "cosine" are refused.

The level loop takes its step as an object with check(), summarize(table, K,
centers, cnorm) -> (count, buf) and assign(table, K, centers, cnorm):
DeviceStep (the kernels; its buffers go through parallel.allreduce_ once per
inner iteration, so every rank calls fit and draws the same noise) and
NumpyStep (host rows) are interchangeable.  table is (numSlots x 3) int32
(leftNew, rightNew, keepNew) per current slot, new slots 0 .. K - 1 the
children; buf is [wsum (K) | sumSq (K) | sum (K x d)].
"""
from __future__ import annotations

import ctypes
import math

import numpy as np

from . import _native as N
from .ann import java_string_hash
from .kmeans_init import JavaRandom

ROOT = 1
LEVEL_LIMIT = math.log10(float(2 ** 63 - 1)) / math.log10(2.0)
EPSILON = 2.0 ** -52
DEFAULT_SEED = java_string_hash("org.apache.spark.ml.clustering.BisectingKMeans")
RULE_NORM, RULE_WEIGHT, RULE_SLOT = 1, 2, 3       # cyc_bkm_step_dev's badRule


def check_params(k, maxIter, minDivisibleClusterSize, distanceMeasure="euclidean"):
    if int(k) < 1:
        raise N.IllegalArgumentException(
            f"requirement failed: k must be at least 1 but got {k}.")
    if int(maxIter) < 0:
        raise N.IllegalArgumentException(
            f"requirement failed: maxIter must not be negative but got {maxIter}.")
    if not float(minDivisibleClusterSize) > 0.0:
        raise N.IllegalArgumentException(
            "requirement failed: minDivisibleClusterSize must be positive but got "
            f"{minDivisibleClusterSize}.")
    if distanceMeasure == "cosine":
        raise N.IllegalArgumentException(
            "BisectingKMeans runs the euclidean measure; the cosine measure is not provided")
    if distanceMeasure != "euclidean":
        raise N.IllegalArgumentException(
            f"distanceMeasure given invalid value {distanceMeasure}. Supported options: "
            "euclidean.")


def seq_norm(v) -> float:
    """Vectors.norm(v, 2): the sum of squares left to right, then sqrt."""
    s = 0.0
    for x in np.asarray(v, dtype=np.float64).tolist():
        s = s + x * x
    return math.sqrt(s)


def seq_sqdist(a, b) -> float:
    """Vectors.sqdist(a, b): the sum over j ascending of (a_j - b_j)^2."""
    s = 0.0
    for x, y in zip(np.asarray(a, dtype=np.float64).tolist(),
                    np.asarray(b, dtype=np.float64).tolist()):
        t = x - y
        s = s + t * t
    return s


def sums_length(K: int, d: int) -> int:
    return K * (2 + d)


class ClusterSummary:
    """size, center, norm and cost of one cluster."""

    def __init__(self, size, center, norm, cost):
        self.size, self.center, self.norm, self.cost = int(size), center, float(norm), float(cost)


def summaries(count, buf, K: int, d: int):
    """Per child 0 .. K - 1 its ClusterSummary, None for one without rows."""
    count = np.asarray(count, dtype=np.int64)
    buf = np.asarray(buf, dtype=np.float64)
    out = []
    for c in range(K):
        if count[c] <= 0:
            out.append(None)
            continue
        wsum, sumsq = float(buf[c]), float(buf[K + c])
        center = buf[2 * K + c * d:2 * K + (c + 1) * d] * (1.0 / wsum)   # BLAS.scal
        norm = seq_norm(center)
        out.append(ClusterSummary(count[c], center, norm, max(sumsq - wsum * norm * norm, 0.0)))
    return out


def _table(rows):
    return np.ascontiguousarray(np.asarray(rows, dtype=np.int32).reshape(-1, 3))


def fit_clusters(step, d: int, k: int = 4, maxIter: int = 20,
                 minDivisibleClusterSize: float = 1.0, seed: int = DEFAULT_SEED):
    """The level loop over `step`: {node index: ClusterSummary} of active ++
    inactive."""
    check_params(k, maxIter, minDivisibleClusterSize)
    step.check()
    zero = np.zeros((1, d), dtype=np.float64)
    count, buf = step.summarize(_table([[0, -1, -1]]), 1, zero, np.zeros(1))
    root = summaries(count, buf, 1, d)[0]
    if root is None:
        raise N.IllegalArgumentException("requirement failed: BisectingKMeans needs at least one row")
    slot_of = {ROOT: 0}          # the clusters that hold rows -> their slot (a fresh step: 0)
    active, inactive = {ROOT: root}, {}
    n = root.size
    minDiv = float(minDivisibleClusterSize)
    minSize = math.ceil(minDiv) if minDiv >= 1.0 else math.ceil(minDiv * n)
    random = JavaRandom(int(seed))
    needed, level = int(k) - 1, 1
    while active and needed > 0 and level < LEVEL_LIMIT:
        div = [i for i in sorted(active)
               if active[i].size >= minSize and active[i].cost > EPSILON * active[i].size]
        if len(div) > needed:
            div = sorted(sorted(div, key=lambda i: (-active[i].size, i))[:needed])
        if not div:
            inactive.update(active)
            active = {}
            break
        centers = {}
        for i in div:
            c = active[i]
            noise = np.array([random.next_double() for _ in range(d)], dtype=np.float64)
            lvl = 1e-4 * c.norm
            left = c.center + (-lvl) * noise        # axpy on a copy of the center
            right = c.center + lvl * noise
            centers[2 * i] = (left, seq_norm(left))
            centers[2 * i + 1] = (right, seq_norm(right))
        node_of = sorted(slot_of, key=slot_of.get)      # slot -> node
        last = None
        for _ in range(int(maxIter)):
            kids = sorted(centers)
            new = {c: j for j, c in enumerate(kids)}
            K = len(kids)
            table = _table([[new.get(2 * i, -1), new.get(2 * i + 1, -1), -1] if i in div
                            else [-1, -1, K] for i in node_of])
            C = np.stack([centers[c][0] for c in kids])
            cn = np.array([centers[c][1] for c in kids], dtype=np.float64)
            count, buf = step.summarize(table, K, C, cn)
            last = {c: s for c, s in zip(kids, summaries(count, buf, K, d)) if s is not None}
            centers = {c: (s.center, s.norm) for c, s in last.items()}
        # the rows move against the final centers
        kids = sorted(centers)
        new = {c: j for j, c in enumerate(kids)}
        K = len(kids)
        kept = [i for i in node_of if i not in div]
        keep = {i: K + j for j, i in enumerate(kept)}
        table = _table([[new.get(2 * i, -1), new.get(2 * i + 1, -1), -1] if i in div
                        else [-1, -1, keep[i]] for i in node_of])
        step.assign(table, K, np.stack([centers[c][0] for c in kids]),
                    np.array([centers[c][1] for c in kids], dtype=np.float64))
        slot_of = dict(new)
        slot_of.update(keep)
        inactive.update(active)
        active = last if last is not None else {}
        needed -= len(div)
        level += 1
    clusters = dict(inactive)
    clusters.update(active)
    return clusters


class ClusteringTreeNode:
    """One node of BisectingKMeansModel's tree: index (leaves 0, 1, ..,
    internal nodes -1, -2, .. in visiting order), size, center, norm, cost,
    height and children (left first)."""

    def __init__(self, index, size, center, norm, cost, height, children):
        self.index, self.size = int(index), int(size)
        self.center = np.ascontiguousarray(center, dtype=np.float64)
        self.norm, self.cost, self.height = float(norm), float(cost), float(height)
        self.children = list(children)

    @property
    def isLeaf(self):
        return not self.children

    def leafNodes(self):
        if self.isLeaf:
            return [self]
        return [leaf for c in self.children for leaf in c.leafNodes()]


def build_tree(clusters) -> ClusteringTreeNode:
    """buildTree over {node index: ClusterSummary}."""
    counters = [0, -1]      # the next leaf and internal index

    def build(raw):
        c = clusters[raw]
        if 2 * raw not in clusters:
            idx = counters[0]
            counters[0] += 1
            return ClusteringTreeNode(idx, c.size, c.center, c.norm, c.cost, 0.0, [])
        idx = counters[1]
        counters[1] -= 1
        kids = [i for i in (2 * raw, 2 * raw + 1) if i in clusters]
        height = max(math.sqrt(seq_sqdist(c.center, clusters[i].center)) for i in kids)
        return ClusteringTreeNode(idx, c.size, c.center, c.norm, c.cost, height,
                                  [build(i) for i in kids])

    return build(ROOT)


def flatten_tree(root):
    """(nodes, firstChild, numChildren, leafIndex) breadth first, so that a
    node's children are neighbours and follow it: cyc_bkm_predict_dev's form."""
    nodes, first, num, leaf = [root], [], [], []
    i = 0
    while i < len(nodes):
        nd = nodes[i]
        first.append(len(nodes) if nd.children else -1)
        num.append(len(nd.children))
        leaf.append(nd.index if nd.isLeaf else -1)
        nodes.extend(nd.children)
        i += 1
    return (nodes, np.array(first, dtype=np.int32), np.array(num, dtype=np.int32),
            np.array(leaf, dtype=np.int32))


class BKMPlan:
    """cyc_bkm_plan: the width of the rows and the device workspace
    (workspaceBytes 0: 256 MiB)."""

    def __init__(self, numFeatures: int, workspaceBytes: int = 0):
        if int(numFeatures) < 1:
            raise N.IllegalArgumentException(
                f"requirement failed: numFeatures must be positive but got {numFeatures}")
        self.numFeatures = int(numFeatures)
        self._lib = N.load()
        h = ctypes.c_void_p()
        N.check(self._lib.cyc_bkm_plan_create(self.numFeatures, int(workspaceBytes),
                                              ctypes.byref(h)))
        self.handle = h
        self.badRow, self.badRule = -1, 0
        self.tileRows = int(self._lib.cyc_bkm_tile_rows(h))
        self.panelCols = int(self._lib.cyc_bkm_panel_cols(h))
        self.chunkRows = int(self._lib.cyc_bkm_chunk_rows(h))
        self.chunksPerLaunch = int(self._lib.cyc_bkm_chunks_per_launch(h))
        self.maxChildren = int(self._lib.cyc_bkm_max_children(h))

    def close(self):
        if getattr(self, "handle", None):
            self._lib.cyc_bkm_plan_destroy(self.handle)
            self.handle = None

    __del__ = close

    def _rows(self, X):
        return check_rows(X, self.numFeatures, "plan")

    @staticmethod
    def _vector(v, n, dtype, what):
        import torch
        if not torch.is_tensor(v) or v.dtype != dtype or v.numel() != n or not v.is_contiguous():
            raise N.IllegalArgumentException(
                f"requirement failed: {what} must be {n} contiguous {dtype} values")

    def step(self, X, xnorm, weights, slot, table, centers, cnorm, newSlot, count=None, sums=None,
             check=False):
        """One assign step (and, with count and sums, the children's summary
        added into them).  X, xnorm, weights, slot, centers, cnorm, newSlot,
        count, sums: device tensors; table: host (numSlots x 3) int32.  badRow
        / badRule keep the lowest offending row and its rule when the call
        raises."""
        import torch
        n = self._rows(X)
        d = self.numFeatures
        table = _table(table)
        K = int(centers.shape[0])
        self._vector(xnorm, n, torch.float64, "xnorm")
        if weights is not None:
            self._vector(weights, n, torch.float64, "weights")
        if slot is not None:
            self._vector(slot, n, torch.int32, "slot")
        self._vector(newSlot, n, torch.int32, "newSlot")
        self._vector(centers, K * d, torch.float64, "centers")
        self._vector(cnorm, K, torch.float64, "cnorm")
        if (count is None) != (sums is None):
            raise N.IllegalArgumentException("requirement failed: count and sums: both or neither")
        if sums is not None:
            self._vector(count, K, torch.int64, "count")
            self._vector(sums, sums_length(K, d), torch.float64, "sums")
        row, rule = ctypes.c_int64(-1), ctypes.c_int32(0)
        try:
            with torch.cuda.device(X.device):
                N.check(self._lib.cyc_bkm_step_dev(
                    self.handle, N.ptr(X), N.ptr(xnorm), N.ptr(weights), n, N.ptr(slot),
                    int(table.shape[0]), table.ctypes.data, K, N.ptr(centers), N.ptr(cnorm),
                    N.ptr(newSlot), N.ptr(count), N.ptr(sums), int(bool(check)),
                    ctypes.byref(row), ctypes.byref(rule), N.stream_handle()))
        finally:
            self.badRow, self.badRule = int(row.value), int(rule.value)

    def predict(self, X, firstChild, numChildren, leafIndex, centers, cost=True):
        """(pred int32, cost fp64 or None) device tensors of the descent; the
        node arrays are host int32, centers a device (numNodes x d) tensor."""
        import torch
        n = self._rows(X)
        fc, nc, li = (np.ascontiguousarray(a, dtype=np.int32)
                      for a in (firstChild, numChildren, leafIndex))
        m = int(fc.size)
        if nc.size != m or li.size != m:
            raise N.IllegalArgumentException(
                "requirement failed: the node arrays must have one length")
        self._vector(centers, m * self.numFeatures, torch.float64, "centers")
        pred = torch.empty(n, dtype=torch.int32, device=X.device)
        cst = torch.empty(n, dtype=torch.float64, device=X.device) if cost else None
        with torch.cuda.device(X.device):
            N.check(self._lib.cyc_bkm_predict_dev(
                self.handle, N.ptr(X), n, m, fc.ctypes.data, nc.ctypes.data, li.ctypes.data,
                N.ptr(centers), N.ptr(pred), N.ptr(cst), N.stream_handle()))
        return pred, cst


def check_rows(X, numFeatures=None, what: str = "model") -> int:
    """The row count of dense fp64 rows (of this width); CSR rows are refused."""
    import torch
    from .linalg import CSRRows
    if isinstance(X, CSRRows):
        raise N.IllegalArgumentException(
            "BisectingKMeans takes dense rows; the CSR form is not provided")
    if not torch.is_tensor(X) or X.dtype != torch.float64 or X.dim() != 2 \
            or not X.is_contiguous():
        raise N.IllegalArgumentException(
            "requirement failed: rows must be a contiguous fp64 device tensor (n x d)")
    if numFeatures is not None and int(X.shape[1]) != numFeatures:
        raise N.IllegalArgumentException(
            f"requirement failed: the rows have {int(X.shape[1])} features but the {what} has "
            f"{numFeatures}")
    return int(X.shape[0])


class DeviceStep:
    """The step over device rows (this rank's shard): slots and norms live on
    the device, the summary comes back merged over the ranks."""

    def __init__(self, X, weights=None, workspaceBytes: int = 0, plan=None):
        import torch
        from .clustering import row_norms
        n = check_rows(X)
        self.X, self.weights = X, weights
        self.d = int(X.shape[1])
        self.plan = plan if plan is not None else BKMPlan(self.d, workspaceBytes)
        if weights is not None:
            BKMPlan._vector(weights, n, torch.float64, "weights")
        with torch.cuda.device(X.device):
            self.xnorm = row_norms(X)
        self.slot = None                     # every row in slot 0
        self.scratch = torch.empty(n, dtype=torch.int32, device=X.device)

    def _dev(self, a):
        import torch
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(self.X.device)

    def check(self):
        from . import parallel
        one = self._dev(np.zeros((1, self.d)))
        parallel.agree(lambda: self.plan.step(
            self.X, self.xnorm, self.weights, None, [[0, -1, -1]], one, one[0, :1].contiguous(),
            self.scratch, check=True))

    def summarize(self, table, K, centers, cnorm):
        import torch
        from . import parallel
        dev = self.X.device
        count = torch.zeros(K, dtype=torch.int64, device=dev)
        # [count (K, as fp64: exact below 2^53) | wsum | sumSq | sum]: one all-reduce
        both = torch.zeros(K + sums_length(K, self.d), dtype=torch.float64, device=dev)
        self.plan.step(self.X, self.xnorm, self.weights, self.slot, table, self._dev(centers),
                       self._dev(cnorm), self.scratch, count, both[K:])
        both[:K] = count.to(torch.float64)
        parallel.allreduce_(both)
        host = both.cpu().numpy()
        return host[:K].astype(np.int64), host[K:]

    def assign(self, table, K, centers, cnorm):
        import torch
        if self.slot is None:
            new = torch.empty_like(self.scratch)
            self.plan.step(self.X, self.xnorm, self.weights, None, table, self._dev(centers),
                           self._dev(cnorm), new)
            self.slot = new
        else:
            self.plan.step(self.X, self.xnorm, self.weights, self.slot, table,
                           self._dev(centers), self._dev(cnorm), self.slot)


class NumpyStep:
    """The step over host rows in numpy: the same picks as the kernels, the
    sums in plain row order."""

    def __init__(self, X, weights=None):
        self.X = np.ascontiguousarray(X, dtype=np.float64)
        n, self.d = self.X.shape
        self.weights = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
        s = np.zeros(n, dtype=np.float64)
        for j in range(self.d):
            s = s + self.X[:, j] * self.X[:, j]
        self.xnorm = np.sqrt(s)
        self.slot = np.zeros(n, dtype=np.int32)

    def check(self):
        bad = ~np.isfinite(self.xnorm)
        rule = np.where(bad, RULE_NORM, 0)
        if self.weights is not None:
            wbad = ~(np.isfinite(self.weights) & (self.weights > 0.0))
            rule = np.where(bad, rule, np.where(wbad, RULE_WEIGHT, 0))
        rows = np.nonzero(rule)[0]
        if not rows.size:
            return
        r = int(rows[0])
        if rule[r] == RULE_NORM:
            raise N.IllegalArgumentException(
                f"requirement failed: the norm of a row must be finite but got {self.xnorm[r]}. "
                f"(row {r})")
        raise N.IllegalArgumentException(
            f"requirement failed: illegal weight value: {self.weights[r]}. weight must be finite "
            f"and > 0.0. (row {r})")

    def _pick(self, table, K, centers, cnorm):
        table = _table(table)
        C = np.ascontiguousarray(centers, dtype=np.float64).reshape(K, self.d)
        cn = np.asarray(cnorm, dtype=np.float64)
        cl, cr, keep = (table[self.slot, q] for q in range(3))
        pick = np.where(cl >= 0, cl, np.where(cr >= 0, cr, keep)).astype(np.int32)
        two = np.nonzero((cl >= 0) & (cr >= 0))[0]
        if two.size:
            l, r, xn = cl[two], cr[two], self.xnorm[two]
            dl = np.zeros(two.size)
            dr = np.zeros(two.size)
            for j in range(self.d):
                x = self.X[two, j]
                a, b = C[l, j] - x, C[r, j] - x
                dl = dl + a * a
                dr = dr + b * b
            with np.errstate(invalid="ignore"):
                lb = cn[l] - xn
                first = (lb * lb < np.inf) & (dl < np.inf)
                best = np.where(first, dl, np.inf)
                lb = cn[r] - xn
                second = (lb * lb < best) & (dr < best)
            pick[two] = np.where(second, r, l)
        return pick

    def summarize(self, table, K, centers, cnorm):
        pick = self._pick(table, K, centers, cnorm)
        d = self.d
        count = np.zeros(K, dtype=np.int64)
        buf = np.zeros(sums_length(K, d), dtype=np.float64)
        for c in range(K):
            rows = np.nonzero(pick == c)[0]
            if not rows.size:
                continue
            w = np.ones(rows.size) if self.weights is None else self.weights[rows]
            xn = self.xnorm[rows]
            count[c] = rows.size
            buf[c] = np.cumsum(w)[-1]
            buf[K + c] = np.cumsum(xn * xn * w)[-1]
            buf[2 * K + c * d:2 * K + (c + 1) * d] = np.cumsum(w[:, None] * self.X[rows], axis=0)[-1]
        return count, buf

    def assign(self, table, K, centers, cnorm):
        self.slot = self._pick(table, K, centers, cnorm)


class BisectingKMeansSummary:
    def __init__(self, clusterSizes, k, numIter, trainingCost):
        self.clusterSizes = [int(s) for s in clusterSizes]
        self.k, self.numIter, self.trainingCost = int(k), int(numIter), float(trainingCost)


class BisectingKMeansModel:
    """The tree of a fit.  root: ClusteringTreeNode; clusterCenters: the leaf
    centers in leaf order (host, k x d); predict / computeCost run the descent
    on the device."""

    def __init__(self, root: ClusteringTreeNode, distanceMeasure: str = "euclidean",
                 summary=None):
        check_params(1, 0, 1.0, distanceMeasure)
        self.root = root
        self.distanceMeasure = distanceMeasure
        leaves = root.leafNodes()
        self.clusterCenters = np.stack([leaf.center for leaf in leaves])
        self.k = len(leaves)
        self.numFeatures = int(self.clusterCenters.shape[1])
        self.trainingCost = 0.0
        for leaf in leaves:
            self.trainingCost = self.trainingCost + leaf.cost
        self.summary = summary
        self._nodes, self._first, self._num, self._leaf = flatten_tree(root)
        self._plan, self._centers = None, {}

    @classmethod
    def from_arrays(cls, centers, firstChild, numChildren, sizes=None, costs=None,
                    distanceMeasure: str = "euclidean"):
        """A model from host arrays, node 0 the root, a node's children at
        firstChild, firstChild + 1 (flatten_tree's form).  Indices and heights
        are those of buildTree's walk."""
        centers = np.ascontiguousarray(centers, dtype=np.float64)
        m = centers.shape[0]
        fc = np.asarray(firstChild, dtype=np.int64)
        nc = np.asarray(numChildren, dtype=np.int64)
        if fc.shape != (m,) or nc.shape != (m,):
            raise N.IllegalArgumentException(
                "requirement failed: firstChild and numChildren need one entry per center")
        for i in range(m):
            if not 0 <= nc[i] <= 2 or (nc[i] > 0 and not (i < fc[i] and fc[i] + nc[i] <= m)):
                raise N.IllegalArgumentException(
                    f"requirement failed: node {i} must have 0, 1 or 2 children that follow it "
                    "and lie inside the tree")
        sizes = np.zeros(m, dtype=np.int64) if sizes is None else np.asarray(sizes)
        costs = np.zeros(m) if costs is None else np.asarray(costs, dtype=np.float64)
        counters = [0, -1]

        def build(i):
            kids = [int(fc[i]) + q for q in range(int(nc[i]))]
            if not kids:
                idx = counters[0]
                counters[0] += 1
                return ClusteringTreeNode(idx, sizes[i], centers[i], seq_norm(centers[i]),
                                          costs[i], 0.0, [])
            idx = counters[1]
            counters[1] -= 1
            height = max(math.sqrt(seq_sqdist(centers[i], centers[c])) for c in kids)
            return ClusteringTreeNode(idx, sizes[i], centers[i], seq_norm(centers[i]), costs[i],
                                      height, [build(c) for c in kids])

        return cls(build(0), distanceMeasure)

    def _device(self, X):
        import torch
        check_rows(X, self.numFeatures)
        if self._plan is None:
            self._plan = BKMPlan(self.numFeatures)
        key = str(X.device)
        if key not in self._centers:
            C = np.stack([nd.center for nd in self._nodes])
            self._centers[key] = torch.from_numpy(C).to(X.device)
        return self._centers[key]

    def predict_with_cost(self, X):
        """(leaf index int32, sqdist to the last node of the descent) on the
        device."""
        C = self._device(X)
        return self._plan.predict(X, self._first, self._num, self._leaf, C, cost=True)

    def predict(self, X):
        C = self._device(X)
        return self._plan.predict(X, self._first, self._num, self._leaf, C, cost=False)[0]

    def computeCost(self, X) -> float:
        return float(self.predict_with_cost(X)[1].sum().item())


class BisectingKMeans:
    """ml/clustering/BisectingKMeans.scala's estimator over dense fp64 device
    rows; with several ranks every rank calls fit on its shard."""

    def __init__(self, k: int = 4, maxIter: int = 20, seed: int = DEFAULT_SEED,
                 minDivisibleClusterSize: float = 1.0, distanceMeasure: str = "euclidean",
                 workspaceBytes: int = 0):
        check_params(k, maxIter, minDivisibleClusterSize, distanceMeasure)
        self.k, self.maxIter, self.seed = int(k), int(maxIter), int(seed)
        self.minDivisibleClusterSize = float(minDivisibleClusterSize)
        self.distanceMeasure = distanceMeasure
        self.workspaceBytes = int(workspaceBytes)

    def fit_step(self, step, d: int) -> BisectingKMeansModel:
        """The fit over any step object (DeviceStep, NumpyStep)."""
        clusters = fit_clusters(step, d, self.k, self.maxIter, self.minDivisibleClusterSize,
                                self.seed)
        root = build_tree(clusters)
        model = BisectingKMeansModel(root, self.distanceMeasure)
        model.summary = BisectingKMeansSummary([leaf.size for leaf in root.leafNodes()], self.k,
                                               self.maxIter, model.trainingCost)
        return model

    def fit(self, X, weights=None) -> BisectingKMeansModel:
        check_rows(X)
        return self.fit_step(DeviceStep(X, weights, self.workspaceBytes), int(X.shape[1]))
