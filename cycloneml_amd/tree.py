"""DecisionTreeClassifier / DecisionTreeRegressor (ml/tree/impl/RandomForest.scala,
DecisionTreeMetadata.scala, TreePoint.scala, mllib/tree/impurity/*,
ml/tree/Node.scala and ml/classification|regression/DecisionTree*.scala, Spark
3.3) over dense fp64 device rows, continuous features, optional row weights.
The kernels are csrc/decision_tree.hip (cyc_dt_* in include/cyclone.h).

Fit (grow).  The split candidates of every feature come from a sample of the
rows (find_splits); the rows are binned once into one byte per value (bin =
the number of thresholds strictly below the value); per level every node that
may still split gets its histogram feature x bin x stats over its rows, the
best split of every node is found on the host (best_splits) and the rows move
to the children.  Node indices: root 1, children 2 i and 2 i + 1.

The level loop takes its step as an object with check(), totals(),
sample(rows), bin(thresholds), histogram(nodeOf, K, B) and route(table): DeviceStep (the kernels; histograms go through
parallel.allreduce_ once per call, so every rank calls fit) and NumpyStep (host
rows) are interchangeable.  Every row has a slot, a compact id of its node; -1
is the skip slot of rows parked in leaves.  nodeOf names per slot its node 0 ..
K - 1 of one histogram call or -1; table is (numSlots x 4) int32 (feature,
splitBin, leftNew, rightNew) per slot, feature -1 for a slot whose rows park.

This project's own rules: the sample of find_splits is every row when the
sampling fraction min(max(maxBins^2, 10000) / n, 1) is 1 and otherwise
max(maxBins^2, 10000) rows drawn without replacement by
numpy.random.default_rng(seed) over the global row range (Spark's RDD.sample is
not restated).  Rows with a NaN feature, a label that is no class index (not
finite for the regressor) or a weight that is not finite and >= 0 are refused,
naming the lowest such row.  CSRRows and categorical features are refused.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _native as N

EPSILON = 2.0 ** -52
INVALID_GAIN = -np.finfo(np.float64).max          # -Double.MaxValue
MAX_SPLITS = 255
MAX_CLASSES = 1024
MAX_DEPTH = 30
MAX_NODES = 4096                                  # cyc_dt_max_nodes
MAX_FEATURES = 65535 * 16                         # cyc_dt_max_features
RULE_FEATURE, RULE_LABEL, RULE_WEIGHT = 1, 2, 3   # cyc_dt_check_dev's badRule
HIST_BYTES = 256 << 20                            # the histograms of one call (maxMemoryInMB)
IMPURITIES = {"gini": 0, "entropy": 1, "variance": 2}


def _require(cond, msg):
    if not cond:
        raise N.IllegalArgumentException("requirement failed: " + msg)


def check_params(maxDepth, maxBins, minInstancesPerNode, minWeightFractionPerNode, minInfoGain,
                 impurity, classifier, categoricalFeaturesInfo=None):
    _require(0 <= int(maxDepth) <= 30,
             f"DecisionTree currently only supports maxDepth in [0, 30], but was given maxDepth = {maxDepth}.")
    _require(2 <= int(maxBins) <= 256,
             f"DecisionTree takes maxBins in [2, 256] (a bin is a byte) but got {maxBins}.")
    _require(int(minInstancesPerNode) >= 1,
             f"minInstancesPerNode must be at least 1 but got {minInstancesPerNode}.")
    _require(0.0 <= float(minWeightFractionPerNode) < 0.5,
             f"minWeightFractionPerNode must be in [0, 0.5) but got {minWeightFractionPerNode}.")
    _require(float(minInfoGain) >= 0.0, f"minInfoGain must not be negative but got {minInfoGain}.")
    allowed = ("gini", "entropy") if classifier else ("variance",)
    if impurity not in allowed:
        raise N.IllegalArgumentException(
            f"impurity given invalid value {impurity}. Supported options: {', '.join(allowed)}.")
    if categoricalFeaturesInfo:
        raise N.IllegalArgumentException(
            "DecisionTree takes continuous features; categorical features are not provided")


def check_classes(numClasses, maxBins):
    _require(1 <= int(numClasses) <= MAX_CLASSES,
             f"DecisionTree supports 1 to {MAX_CLASSES} classes but got {numClasses}.")
    _require(int(numClasses) <= int(maxBins),
             f"DecisionTree requires maxBins (= {maxBins}) to be at least as large as the number "
             f"of classes (= {numClasses}).")


def num_stats(numClasses: int) -> int:
    return numClasses + 1 if numClasses else 4


# ---------------------------------------------------------------- split candidates
def sample_fraction(maxBins: int, numExamples: int) -> float:
    return min(max(maxBins * maxBins, 10000) / numExamples, 1.0)


def sample_rows(maxBins: int, numExamples: int, seed: int):
    """The global rows of find_splits' sample, ascending; None: every row."""
    if sample_fraction(maxBins, numExamples) >= 1.0:
        return None
    m = max(maxBins * maxBins, 10000)
    return np.sort(np.random.default_rng(int(seed)).choice(numExamples, size=m, replace=False))


def find_splits(values, weights, numSplits: int, weightedNumSamples: float):
    """findSplitsForContinuousFeature over one feature's sampled column."""
    v = np.asarray(values, dtype=np.float64)
    w = np.ones(v.size) if weights is None else np.asarray(weights, dtype=np.float64)
    nz = v != 0.0
    v, w = v[nz], w[nz]
    if not v.size:
        return np.zeros(0)
    partNum = float(np.cumsum(w)[-1])
    vals, inv = np.unique(v, return_inverse=True)
    counts = np.bincount(inv.ravel(), weights=w, minlength=vals.size)   # row order per value
    if weightedNumSamples - partNum > EPSILON * v.size * 100:
        at = int(np.searchsorted(vals, 0.0))
        vals = np.insert(vals, at, 0.0)
        counts = np.insert(counts, at, weightedNumSamples - partNum)
    possible = vals.size - 1
    if possible == 0:
        return np.zeros(0)
    if possible <= numSplits:
        return (vals[:-1] + vals[1:]) / 2.0
    stride = weightedNumSamples / (numSplits + 1)
    cur = np.cumsum(counts)                     # currentCount after index
    out = []
    target = stride
    cum = cur.tolist()
    for index in range(1, vals.size):
        prev, now = cum[index - 1], cum[index]
        if abs(prev - target) < abs(now - target):
            out.append((vals[index - 1] + vals[index]) / 2.0)
            target += stride
    return np.asarray(out, dtype=np.float64)


def all_splits(Xs, ws, maxBins: int, numExamples: int, weightedNumExamples: float):
    """The thresholds of every feature from the sample (Xs, ws)."""
    maxPossibleBins = min(int(maxBins), int(numExamples))
    numSplits = maxPossibleBins - 1
    W = sample_fraction(maxBins, numExamples) * weightedNumExamples
    return [find_splits(Xs[:, f], ws, numSplits, W) for f in range(Xs.shape[1])]


def pad_thresholds(thresholds):
    d = len(thresholds)
    thr = np.zeros((d, MAX_SPLITS), dtype=np.float64)
    cnt = np.zeros(d, dtype=np.int32)
    for f, t in enumerate(thresholds):
        _require(len(t) <= MAX_SPLITS, f"feature {f} has more than {MAX_SPLITS} splits")
        cnt[f] = len(t)
        thr[f, :len(t)] = t
    return thr, cnt


# ------------------------------------------------------------------ impurities
def stat_count(stats, numClasses: int):
    """The weighted count of statistics (.., S): the class weights summed in
    class order, or the variance's first entry."""
    if not numClasses:
        return stats[..., 0]
    s = np.zeros(stats.shape[:-1], dtype=np.float64)
    for c in range(numClasses):
        s = s + stats[..., c]
    return s


def calculate(stats, numClasses: int, impurity: str):
    """ImpurityCalculator.calculate() elementwise over statistics (.., S)."""
    stats = np.asarray(stats, dtype=np.float64)
    total = stat_count(stats, numClasses)
    with np.errstate(divide="ignore", invalid="ignore"):
        if impurity == "variance":
            s, ss = stats[..., 1], stats[..., 2]
            out = (ss - (s * s) / total) / total
        elif impurity == "gini":
            out = np.ones(total.shape, dtype=np.float64)
            for c in range(numClasses):
                f = stats[..., c] / total
                out = out - f * f
        else:
            out = np.zeros(total.shape, dtype=np.float64)
            ln2 = np.log(np.float64(2.0))
            for c in range(numClasses):
                n = stats[..., c]
                f = n / total
                term = f * (np.log(f) / ln2)
                out = np.where(n != 0.0, out - term, out)
    return np.where(total == 0.0, 0.0, out)


def predict_of(stats, numClasses: int) -> float:
    """ImpurityCalculator.predict of one node's statistics."""
    if numClasses:
        return float(np.argmax(stats[:numClasses]))       # the first largest
    return float(stats[1] / stats[0]) if stats[0] != 0.0 else 0.0


class BestSplits:
    """Per node of one histogram call: feature, split, gain (INVALID_GAIN: no
    valid split), the parent's statistics and impurity, the sides' statistics
    and impurities."""

    def __init__(self, feature, split, gain, parent, impurity, left, right, leftImp, rightImp):
        self.feature, self.split, self.gain = feature, split, gain
        self.parent, self.impurity = parent, impurity
        self.left, self.right, self.leftImp, self.rightImp = left, right, leftImp, rightImp


def best_splits(hist, numSplits, numClasses: int, impurity: str, minInstancesPerNode: int = 1,
                minWeightPerNode: float = 0.0, minInfoGain: float = 0.0,
                features=None) -> BestSplits:
    """binsToBestSplit over hist (K x d x B x S), features with numSplits[f]
    splits: the first maximum of the gain in (feature, split) order.  features
    (K x m, ascending per node; a forest's per-node subsets): hist is K x m x B x
    S over each node's own features, the parent's statistics come from the
    node's first listed feature with splits (its first feature when none has),
    and the feature returned is the listed one."""
    hist = np.asarray(hist, dtype=np.float64)
    K, d, B, S = hist.shape
    ns = np.asarray(numSplits, dtype=np.int64)
    if features is not None:
        features = np.asarray(features, dtype=np.int64).reshape(K, d)
        ns = ns[features]
    else:
        ns = np.broadcast_to(ns, (K, d))
    cum = np.cumsum(hist, axis=2)
    tot = np.take_along_axis(cum, np.minimum(ns, B - 1)[:, :, None, None], axis=2)[:, :, 0, :]
    nsp = max(B - 1, 1)
    left = cum[:, :, :nsp, :] if B > 1 else np.zeros((K, d, 1, S))
    right = tot[:, :, None, :] - left
    exists = np.arange(nsp)[None, None, :] < ns[:, :, None]         # (K, d, nsp)
    has = ns > 0
    f0 = np.argmax(has, axis=1)                                     # the first with splits
    k = np.arange(K)
    parent = np.where(has.any(axis=1)[:, None], left[k, f0, 0, :] + right[k, f0, 0, :],
                      np.cumsum(hist[:, 0], axis=1)[:, -1, :])
    imp = calculate(parent, numClasses, impurity)
    lc, rc = stat_count(left, numClasses), stat_count(right, numClasses)
    limp, rimp = calculate(left, numClasses, impurity), calculate(right, numClasses, impurity)
    total = lc + rc
    with np.errstate(divide="ignore", invalid="ignore"):
        gain = imp[:, None, None] - (lc / total) * limp - (rc / total) * rimp
    invalid = ((left[..., S - 1] < minInstancesPerNode) | (right[..., S - 1] < minInstancesPerNode)
               | (lc < minWeightPerNode) | (rc < minWeightPerNode))
    # this package's rule: a gain that is NaN (both sides without weight) is invalid too
    invalid = invalid | ~(gain >= minInfoGain)
    gain = np.where(invalid, INVALID_GAIN, gain)
    gain = np.where(exists, gain, -np.inf)
    flat = gain.reshape(K, d * nsp)
    at = np.argmax(flat, axis=1)                                   # the first maximum
    bf, bs = at // nsp, at % nsp
    g = flat[k, at]
    g = np.where(np.isfinite(g), g, INVALID_GAIN)
    return BestSplits(bf if features is None else features[k, bf], bs, g, parent, imp,
                      left[k, bf, bs], right[k, bf, bs], limp[k, bf, bs], rimp[k, bf, bs])


# ------------------------------------------------------------------------ tree
class Node:
    """A node of the fitted tree.  stats: the statistics (class weights and the
    raw count, or weight, sum, sum of squares and raw count); split: (feature,
    threshold) of an internal node; left / right: its children."""

    def __init__(self, stats, impurity, numClasses):
        self.stats = np.array(stats, dtype=np.float64)
        self.impurity = float(impurity)
        self.numClasses = numClasses
        self.prediction = predict_of(self.stats, numClasses)
        self.gain = 0.0
        self.split = None
        self.left = self.right = None

    @property
    def isLeaf(self):
        return self.left is None

    @property
    def impurityStats(self):
        return self.stats[:self.numClasses] if self.numClasses else self.stats[:3]

    @property
    def count(self):
        return float(stat_count(self.stats, self.numClasses))

    def leaf_copy(self):
        return Node(self.stats, self.impurity, self.numClasses)


def prune(node: Node) -> Node:
    """toNode(prune = true): an internal node whose children are leaves with
    one prediction becomes a leaf."""
    if node.isLeaf:
        return node
    node.left, node.right = prune(node.left), prune(node.right)
    if node.left.isLeaf and node.right.isLeaf and node.left.prediction == node.right.prediction:
        return node.leaf_copy()
    return node


def nodes_per_call(d: int, B: int, S: int, maxNodes: int = MAX_NODES) -> int:
    return int(min(maxNodes, max(1, HIST_BYTES // (8 * d * B * S))))


def grow(step, d: int, numClasses: int, impurity: str, maxDepth: int = 5, maxBins: int = 32,
         minInstancesPerNode: int = 1, minWeightFractionPerNode: float = 0.0,
         minInfoGain: float = 0.0, seed: int = 0, pruneTree: bool = True):
    """The level loop over `step`: (root Node, thresholds)."""
    check_params(maxDepth, maxBins, minInstancesPerNode, minWeightFractionPerNode, minInfoGain,
                 impurity, bool(numClasses))
    step.check()
    n, wsum = step.totals()
    _require(n > 0, "DecisionTree requires size of input RDD > 0, but was given by empty one.")
    thresholds = all_splits(*step.sample(sample_rows(maxBins, n, seed)), maxBins, n, wsum)
    numSplits = np.array([len(t) for t in thresholds], dtype=np.int64)
    B = int(numSplits.max()) + 1
    S = num_stats(numClasses)
    step.bin(thresholds)
    minWeight = float(minWeightFractionPerNode) * wsum
    per_call = nodes_per_call(d, B, S, getattr(step, "maxNodes", MAX_NODES))
    nodes = {}
    live = {1: 0}               # the nodes to split at this level -> their slot
    level = 0
    while live:
        order = sorted(live)
        numSlots = len(order)
        table = np.full((numSlots, 4), -1, dtype=np.int32)
        nxt = {}
        for g0 in range(0, len(order), per_call):
            group = order[g0:g0 + per_call]
            nodeOf = np.full(numSlots, -1, dtype=np.int32)
            for j, i in enumerate(group):
                nodeOf[live[i]] = j
            hist = step.histogram(nodeOf, len(group), B)
            best = best_splits(hist, numSplits, numClasses, impurity, minInstancesPerNode,
                               minWeight, minInfoGain)
            for j, i in enumerate(group):
                if i not in nodes:      # the root: its statistics are the first evaluation's
                    nodes[i] = Node(best.parent[j], best.impurity[j], numClasses)
                node = nodes[i]
                gain = float(best.gain[j])
                if gain <= 0.0 or level == maxDepth:
                    continue
                f, s = int(best.feature[j]), int(best.split[j])
                node.gain = gain
                node.split = (f, float(thresholds[f][s]))
                node.left = Node(best.left[j], best.leftImp[j], numClasses)
                node.right = Node(best.right[j], best.rightImp[j], numClasses)
                nodes[2 * i], nodes[2 * i + 1] = node.left, node.right
                new = []
                for child, idx in ((node.left, 2 * i), (node.right, 2 * i + 1)):
                    if level + 1 == maxDepth or abs(child.impurity) < EPSILON:
                        new.append(-1)
                    else:
                        nxt[idx] = len(nxt)
                        new.append(nxt[idx])
                table[live[i]] = (f, s, new[0], new[1])
        if nxt:
            step.route(table)
        live = nxt
        level += 1
    root = nodes[1]
    return (prune(root) if pruneTree else root), thresholds


# ----------------------------------------------------------------------- steps
class DTPlan:
    """cyc_dt_plan: the width of the rows, the number of classes (0: the
    variance statistics) and the device workspace (workspaceBytes 0: 256 MiB)."""

    def __init__(self, numFeatures: int, numClasses: int = 0, workspaceBytes: int = 0):
        _require(1 <= int(numFeatures) <= MAX_FEATURES,
                 f"DecisionTree supports 1 to {MAX_FEATURES} features but got {numFeatures}")
        self.numFeatures, self.numClasses = int(numFeatures), int(numClasses)
        self._lib = N.load()
        h = ctypes.c_void_p()
        N.check(self._lib.cyc_dt_plan_create(self.numFeatures, self.numClasses,
                                             int(workspaceBytes), ctypes.byref(h)))
        self.handle = h
        self.badRow, self.badRule = -1, 0
        self.numStats = int(self._lib.cyc_dt_num_stats(h))
        self.runRows = int(self._lib.cyc_dt_run_rows())
        self.maxNodes = int(self._lib.cyc_dt_max_nodes())

    def close(self):
        if getattr(self, "handle", None):
            self._lib.cyc_dt_plan_destroy(self.handle)
            self.handle = None

    __del__ = close

    def runs_per_launch(self, numBins: int) -> int:
        return int(self._lib.cyc_dt_runs_per_launch(self.handle, int(numBins)))

    def _rows(self, X):
        return check_rows(X, self.numFeatures, "plan")

    @staticmethod
    def _vector(v, n, dtype, what):
        import torch
        if not torch.is_tensor(v) or not v.is_cuda or v.dtype != dtype or v.numel() != n \
                or not v.is_contiguous():
            raise N.IllegalArgumentException(
                f"requirement failed: {what} must be {n} contiguous {dtype} values on the device")

    def check(self, X, y, weights=None):
        import torch
        n = self._rows(X)
        self._vector(y, n, torch.float64, "labels")
        if weights is not None:
            self._vector(weights, n, torch.float64, "weights")
        row, rule = ctypes.c_int64(-1), ctypes.c_int32(0)
        try:
            with torch.cuda.device(X.device):
                N.check(self._lib.cyc_dt_check_dev(self.handle, N.ptr(X), N.ptr(y), N.ptr(weights),
                                                   n, ctypes.byref(row), ctypes.byref(rule),
                                                   N.stream_handle()))
        finally:
            self.badRow, self.badRule = int(row.value), int(rule.value)

    def bin(self, X, thresholds):
        """The uint8 image (n x d) of X under per-feature thresholds (a list of
        ascending arrays)."""
        import torch
        n = self._rows(X)
        _require(len(thresholds) == self.numFeatures, "one threshold array per feature")
        thr, cnt = pad_thresholds(thresholds)
        image = torch.empty((n, self.numFeatures), dtype=torch.uint8, device=X.device)
        with torch.cuda.device(X.device):
            N.check(self._lib.cyc_dt_bin_dev(self.handle, N.ptr(X), n, thr.ctypes.data,
                                             cnt.ctypes.data, N.ptr(image), N.stream_handle()))
        return image

    def _image(self, image):
        import torch
        if not torch.is_tensor(image) or not image.is_cuda or image.dtype != torch.uint8 \
                or image.dim() != 2 or int(image.shape[1]) != self.numFeatures \
                or not image.is_contiguous():
            raise N.IllegalArgumentException(
                f"requirement failed: the image must be contiguous uint8 (n x {self.numFeatures}) "
                "on the device")
        return int(image.shape[0])

    def route(self, image, slot, table):
        import torch
        n = self._image(image)
        self._vector(slot, n, torch.int32, "slot")
        table = np.ascontiguousarray(np.asarray(table, dtype=np.int32).reshape(-1, 4))
        with torch.cuda.device(image.device):
            N.check(self._lib.cyc_dt_route_dev(self.handle, N.ptr(image), n, N.ptr(slot),
                                               int(table.shape[0]), table.ctypes.data,
                                               N.stream_handle()))

    def histogram(self, image, y, weights, slot, nodeOf, numNodes: int, numBins: int):
        """The device histogram (numNodes x d x numBins x numStats)."""
        import torch
        n = self._image(image)
        self._vector(y, n, torch.float64, "labels")
        if weights is not None:
            self._vector(weights, n, torch.float64, "weights")
        if slot is not None:
            self._vector(slot, n, torch.int32, "slot")
        nodeOf = np.ascontiguousarray(nodeOf, dtype=np.int32).ravel()
        hist = torch.empty((int(numNodes), self.numFeatures, int(numBins), self.numStats),
                           dtype=torch.float64, device=image.device)
        with torch.cuda.device(image.device):
            N.check(self._lib.cyc_dt_histogram_dev(
                self.handle, N.ptr(image), N.ptr(y), N.ptr(weights), n, N.ptr(slot),
                int(nodeOf.size), nodeOf.ctypes.data, int(numNodes), int(numBins), N.ptr(hist),
                N.stream_handle()))
        return hist

    def predict(self, X, feature, threshold, firstChild, leafIndex, leafPred, leafRaw=None,
                pred=True, raw=False, prob=False):
        """(leaf int32, pred, raw, prob) device tensors of the descent (None
        for what is not asked for); the tree arrays are host arrays."""
        import torch
        n = self._rows(X)
        ft, fc, li = (np.ascontiguousarray(a, dtype=np.int32) for a in (feature, firstChild, leafIndex))
        th = np.ascontiguousarray(threshold, dtype=np.float64)
        lp = np.ascontiguousarray(leafPred, dtype=np.float64)
        m, C = int(ft.size), self.numClasses
        _require(fc.size == m and li.size == m and th.size == m,
                 "the node arrays must have one length")
        lr = None
        if leafRaw is not None:
            lr = np.ascontiguousarray(leafRaw, dtype=np.float64)
            _require(lr.size == lp.size * C, "leafRaw must be numLeaves x numClasses")
        _require(not (raw or prob) or (lr is not None and C > 0), "raw and prob need leafRaw")
        dev = X.device
        leaf = torch.empty(n, dtype=torch.int32, device=dev)
        p = torch.empty(n, dtype=torch.float64, device=dev) if pred else None
        r = torch.empty((n, C), dtype=torch.float64, device=dev) if raw else None
        q = torch.empty((n, C), dtype=torch.float64, device=dev) if prob else None
        with torch.cuda.device(dev):
            N.check(self._lib.cyc_dt_predict_dev(
                self.handle, N.ptr(X), n, m, ft.ctypes.data, th.ctypes.data, fc.ctypes.data,
                li.ctypes.data, int(lp.size), lp.ctypes.data,
                None if lr is None else lr.ctypes.data, N.ptr(leaf), N.ptr(p), N.ptr(r), N.ptr(q),
                N.stream_handle()))
        return leaf, p, r, q


def check_rows(X, numFeatures=None, what: str = "model") -> int:
    """The row count of dense fp64 rows (of this width); CSR rows are refused."""
    import torch
    from .linalg import CSRRows
    if isinstance(X, CSRRows):
        raise N.IllegalArgumentException(
            "DecisionTree takes dense rows; the CSR form is not provided")
    if not torch.is_tensor(X) or not X.is_cuda or X.dtype != torch.float64 or X.dim() != 2 \
            or not X.is_contiguous():
        raise N.IllegalArgumentException(
            "requirement failed: rows must be a contiguous fp64 device tensor (n x d)")
    if numFeatures is not None and int(X.shape[1]) != numFeatures:
        raise N.IllegalArgumentException(
            f"requirement failed: the rows have {int(X.shape[1])} features but the {what} has "
            f"{numFeatures}")
    return int(X.shape[0])


class DeviceStep:
    """The step over device rows (this rank's shard): the image and the slots
    live on the device, a histogram comes back merged over the ranks."""

    def __init__(self, X, y, weights=None, numClasses: int = 0, workspaceBytes: int = 0,
                 plan=None, checked: bool = False):
        import torch
        n = check_rows(X)
        self.checked = checked          # the rows already passed the checks of check()
        self.X, self.y, self.weights = X, y, weights
        self.d = int(X.shape[1])
        self.plan = plan if plan is not None else DTPlan(self.d, numClasses, workspaceBytes)
        self.maxNodes = self.plan.maxNodes
        DTPlan._vector(y, n, torch.float64, "labels")
        if weights is not None:
            DTPlan._vector(weights, n, torch.float64, "weights")
        self.image = None
        self.slot = torch.zeros(n, dtype=torch.int32, device=X.device)

    def check(self):
        from . import parallel
        if self.checked:
            return
        parallel.agree(lambda: self.plan.check(self.X, self.y, self.weights))

    def totals(self):
        import torch
        from . import parallel
        n = int(self.X.shape[0])
        # the rank's weights summed in row order, as NumpyStep and the reference do (8 n
        # bytes to the host once per fit); with several ranks the ranks' sums are added
        ws = float(n) if self.weights is None or not n else \
            float(np.cumsum(self.weights.cpu().numpy())[-1])
        t = torch.tensor([float(n), ws], dtype=torch.float64, device=self.X.device)
        parallel.allreduce_(t)
        n_all, w_all = t.cpu().tolist()
        return int(n_all), float(w_all)

    def sample(self, rows):
        import torch
        from . import parallel
        n = int(self.X.shape[0])
        sizes = parallel.allgather_object(n)
        rank = parallel.world()[0]
        lo = self.rowOffset = int(sum(sizes[:rank]))     # this rank's first global row
        if rows is None:
            Xs = self.X.cpu().numpy()
            ws = None if self.weights is None else self.weights.cpu().numpy()
        else:
            mine = rows[(rows >= lo) & (rows < lo + n)] - lo
            idx = torch.from_numpy(np.ascontiguousarray(mine, dtype=np.int64)).to(self.X.device)
            Xs = self.X.index_select(0, idx).cpu().numpy()
            ws = None if self.weights is None else self.weights.index_select(0, idx).cpu().numpy()
        parts = parallel.allgather_object((Xs, ws))
        Xs = np.concatenate([p[0] for p in parts], axis=0)
        ws = None if self.weights is None else np.concatenate([p[1] for p in parts])
        return Xs, ws

    def bin(self, thresholds):
        self.image = self.plan.bin(self.X, thresholds)

    def histogram(self, nodeOf, K, B):
        from . import parallel
        hist = self.plan.histogram(self.image, self.y, self.weights, self.slot, nodeOf, K, B)
        parallel.allreduce_(hist.view(-1))
        return hist.cpu().numpy()

    def route(self, table):
        self.plan.route(self.image, self.slot, table)


class NumpyStep:
    """The step over host rows in numpy: the same bins and routes as the
    kernels, the sums in plain row order."""

    def __init__(self, X, y, weights=None, numClasses: int = 0):
        self.X = np.ascontiguousarray(X, dtype=np.float64)
        _require(self.X.ndim == 2, "rows must be n x d")
        n, self.d = self.X.shape
        self.y = np.ascontiguousarray(y, dtype=np.float64)
        self.weights = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
        self.numClasses = int(numClasses)
        self.image = None
        self.slot = np.zeros(n, dtype=np.int32)

    def check(self):
        C = self.numClasses
        y = self.y
        with np.errstate(invalid="ignore"):
            xbad = np.isnan(self.X).any(axis=1)
            if C:
                ybad = ~((y >= 0.0) & (y < C) & (np.floor(y) == y))
            else:
                ybad = ~np.isfinite(y)
            wbad = np.zeros(y.size, dtype=bool) if self.weights is None else \
                ~(np.isfinite(self.weights) & (self.weights >= 0.0))
        rule = np.where(xbad, RULE_FEATURE, np.where(ybad, RULE_LABEL,
                                                     np.where(wbad, RULE_WEIGHT, 0)))
        rows = np.nonzero(rule)[0]
        if not rows.size:
            return
        r = int(rows[0])
        if rule[r] == RULE_FEATURE:
            raise N.IllegalArgumentException(
                f"requirement failed: DecisionTree requires feature values that are not NaN. (row {r})")
        if rule[r] == RULE_LABEL:
            raise N.IllegalArgumentException(
                (f"requirement failed: Classification labels should be integers in [0 to {C - 1}]. "
                 f"Found {y[r]}. (row {r})") if C else
                f"requirement failed: Regression labels must be finite but got {y[r]}. (row {r})")
        raise N.IllegalArgumentException(
            f"requirement failed: illegal weight value: {self.weights[r]}. weight must be finite "
            f"and >= 0.0. (row {r})")

    def totals(self):
        n = int(self.X.shape[0])
        return n, (float(n) if self.weights is None or not n else float(np.cumsum(self.weights)[-1]))

    def sample(self, rows):
        if rows is None:
            return self.X, self.weights
        return self.X[rows], (None if self.weights is None else self.weights[rows])

    def bin(self, thresholds):
        n, d = self.X.shape
        self.image = np.zeros((n, d), dtype=np.uint8)
        for f, t in enumerate(thresholds):
            self.image[:, f] = np.searchsorted(np.asarray(t, dtype=np.float64), self.X[:, f], "left")

    def histogram(self, nodeOf, K, B):
        nodeOf = np.asarray(nodeOf, dtype=np.int64)
        C, d = self.numClasses, self.d
        S = num_stats(C)
        hist = np.zeros((K, d, B, S), dtype=np.float64)
        live = np.nonzero(self.slot >= 0)[0]
        node = nodeOf[self.slot[live]]
        live, node = live[node >= 0], node[node >= 0]
        w = np.ones(live.size) if self.weights is None else self.weights[live]
        y = self.y[live]
        if C:
            vals = [(y.astype(np.int64), w), (np.full(live.size, C), np.ones(live.size))]
        else:
            wy = w * y
            vals = [(np.full(live.size, s), v) for s, v in enumerate((w, wy, wy * y, np.ones(live.size)))]
        for f in range(d):
            b = self.image[live, f].astype(np.int64)
            for s, v in vals:
                np.add.at(hist, (node, f, b, s), v)      # unbuffered: row order
        return hist

    def route(self, table):
        table = np.asarray(table, dtype=np.int32).reshape(-1, 4)
        out = np.full(self.slot.size, -1, dtype=np.int32)
        ok = np.nonzero((self.slot >= 0) & (self.slot < table.shape[0]))[0]
        t = table[self.slot[ok]]
        split = t[:, 0] >= 0
        ok, t = ok[split], t[split]
        b = self.image[ok, t[:, 0]].astype(np.int32)
        out[ok] = np.where(b <= t[:, 1], t[:, 2], t[:, 3])
        self.slot = out


# ---------------------------------------------------------------------- models
def flatten_tree(root: Node):
    """(feature, threshold, firstChild, leafIndex, leaves) breadth first, so
    that a node's children are neighbours and follow it (cyc_dt_predict_dev's
    form); leaves in the order of a pre-order walk, which leafIndex counts."""
    leaves = []

    def walk(nd):
        if nd.isLeaf:
            leaves.append(nd)
        else:
            walk(nd.left)
            walk(nd.right)

    walk(root)
    index = {id(nd): i for i, nd in enumerate(leaves)}
    nodes, feature, threshold, first, leaf = [root], [], [], [], []
    i = 0
    while i < len(nodes):
        nd = nodes[i]
        if nd.isLeaf:
            feature.append(-1)
            threshold.append(0.0)
            first.append(-1)
            leaf.append(index[id(nd)])
        else:
            feature.append(nd.split[0])
            threshold.append(nd.split[1])
            first.append(len(nodes))
            leaf.append(-1)
            nodes.extend((nd.left, nd.right))
        i += 1
    return (np.array(feature, dtype=np.int32), np.array(threshold, dtype=np.float64),
            np.array(first, dtype=np.int32), np.array(leaf, dtype=np.int32), leaves)


class _TreeModel:
    """What the two models share: the tree, its flat form and the descent."""

    numClasses = 0

    def __init__(self, root: Node, numFeatures: int):
        self.rootNode = root
        self.numFeatures = int(numFeatures)
        (self._feature, self._threshold, self._first, self._leaf, leaves) = flatten_tree(root)
        self._leafPred = np.array([nd.prediction for nd in leaves], dtype=np.float64)
        self._leafRaw = (np.stack([nd.impurityStats for nd in leaves])
                         if self.numClasses else None)
        self.numNodes = int(self._feature.size)
        self._plan = None

    @property
    def depth(self) -> int:
        def h(nd):
            return 0 if nd.isLeaf else 1 + max(h(nd.left), h(nd.right))
        return h(self.rootNode)

    @property
    def featureImportances(self):
        imp = np.zeros(self.numFeatures, dtype=np.float64)

        def walk(nd):
            if nd.isLeaf:
                return
            imp[nd.split[0]] += nd.gain * nd.count
            walk(nd.left)
            walk(nd.right)

        walk(self.rootNode)
        total = float(np.cumsum(imp)[-1])
        return imp / total if total != 0.0 else imp

    def toDebugString(self) -> str:
        lines = [f"{type(self).__name__}: depth={self.depth}, numNodes={self.numNodes}"
                 + (f", numClasses={self.numClasses}" if self.numClasses else "")
                 + f", numFeatures={self.numFeatures}"]

        def walk(nd, indent):
            pre = " " * indent
            if nd.isLeaf:
                lines.append(f"{pre}Predict: {nd.prediction}")
                return
            f, t = nd.split
            lines.append(f"{pre}If (feature {f} <= {t})")
            walk(nd.left, indent + 1)
            lines.append(f"{pre}Else (feature {f} > {t})")
            walk(nd.right, indent + 1)

        walk(self.rootNode, 2)
        return "\n".join(lines) + "\n"

    @classmethod
    def from_arrays(cls, feature, threshold, firstChild, leafValues, numFeatures, **kw):
        """A model from host arrays, node 0 the root, the children of node i at
        firstChild[i], firstChild[i] + 1 (-1: a leaf).  leafValues has a row
        per NODE: the class weights (classifier) or the prediction (regressor)
        of a leaf.  No device is touched until the first predict."""
        ft = np.asarray(feature, dtype=np.int64)
        th = np.asarray(threshold, dtype=np.float64)
        fc = np.asarray(firstChild, dtype=np.int64)
        m = ft.size
        _require(th.size == m and fc.size == m and len(leafValues) == m,
                 "the node arrays must have one length")
        C = cls._classes_of(leafValues, kw)
        level = np.zeros(m, dtype=np.int64)
        for i in range(m):
            _require(fc[i] < 0 or (i < fc[i] and fc[i] + 2 <= m and 0 <= ft[i] < numFeatures),
                     f"node {i} must be a leaf or split a feature and have two children that "
                     "follow it and lie inside the tree")
            if fc[i] >= 0:
                level[fc[i]] = level[fc[i] + 1] = level[i] + 1
        # a fit never goes below maxDepth <= 30; it also bounds the walks over the tree
        _require(int(level.max()) <= MAX_DEPTH,
                 f"a tree of depth {int(level.max())} is deeper than {MAX_DEPTH}")
        # children follow their parents: the nodes from the last to the first
        nodes = [None] * m
        for i in range(m - 1, -1, -1):
            nd = cls._leaf_node(leafValues[i], C)
            if fc[i] >= 0:
                nd.split = (int(ft[i]), float(th[i]))
                nd.left, nd.right = nodes[fc[i]], nodes[fc[i] + 1]
            nodes[i] = nd
        return cls(nodes[0], numFeatures, **kw)

    def _device(self, X):
        check_rows(X, self.numFeatures)
        if self._plan is None:
            self._plan = DTPlan(self.numFeatures, self.numClasses)
        return self._plan

    def _run(self, X, **what):
        return self._device(X).predict(X, self._feature, self._threshold, self._first, self._leaf,
                                       self._leafPred, self._leafRaw, **what)

    def predict(self, X):
        return self._run(X)[1]

    def predictLeaf(self, X):
        return self._run(X, pred=False)[0]


class DecisionTreeClassificationModel(_TreeModel):
    def __init__(self, root: Node, numFeatures: int, numClasses: int):
        self.numClasses = int(numClasses)
        super().__init__(root, numFeatures)

    @staticmethod
    def _classes_of(leafValues, kw):
        kw.setdefault("numClasses", len(np.atleast_1d(leafValues[0])))
        return kw["numClasses"]

    @staticmethod
    def _leaf_node(value, C):
        stats = np.zeros(C + 1)
        stats[:C] = value
        return Node(stats, 0.0, C)

    def predictRaw(self, X):
        return self._run(X, pred=False, raw=True)[2]

    def predictProbability(self, X):
        return self._run(X, pred=False, prob=True)[3]


class DecisionTreeRegressionModel(_TreeModel):
    @staticmethod
    def _classes_of(leafValues, kw):
        return 0

    @staticmethod
    def _leaf_node(value, C):
        return Node([1.0, float(value), 0.0, 1.0], 0.0, 0)


class _TreeEstimator:
    classifier = False

    def __init__(self, maxDepth: int = 5, maxBins: int = 32, minInstancesPerNode: int = 1,
                 minWeightFractionPerNode: float = 0.0, minInfoGain: float = 0.0,
                 impurity: str = "gini", seed: int = 0, numClasses=None,
                 categoricalFeaturesInfo=None, workspaceBytes: int = 0):
        check_params(maxDepth, maxBins, minInstancesPerNode, minWeightFractionPerNode,
                     minInfoGain, impurity, self.classifier, categoricalFeaturesInfo)
        if numClasses is not None:
            check_classes(numClasses, maxBins)
        self.maxDepth, self.maxBins = int(maxDepth), int(maxBins)
        self.minInstancesPerNode = int(minInstancesPerNode)
        self.minWeightFractionPerNode = float(minWeightFractionPerNode)
        self.minInfoGain, self.impurity, self.seed = float(minInfoGain), impurity, int(seed)
        self.numClasses = None if numClasses is None else int(numClasses)
        self.workspaceBytes = int(workspaceBytes)

    def _grow(self, step, d, C):
        return grow(step, d, C, self.impurity, self.maxDepth, self.maxBins,
                    self.minInstancesPerNode, self.minWeightFractionPerNode, self.minInfoGain,
                    self.seed)


class DecisionTreeClassifier(_TreeEstimator):
    """ml/classification/DecisionTreeClassifier.scala's estimator over dense
    fp64 device rows; with several ranks every rank calls fit on its shard."""

    classifier = True

    def __init__(self, maxDepth: int = 5, maxBins: int = 32, minInstancesPerNode: int = 1,
                 minWeightFractionPerNode: float = 0.0, minInfoGain: float = 0.0,
                 impurity: str = "gini", seed: int = 0, numClasses=None,
                 categoricalFeaturesInfo=None, workspaceBytes: int = 0):
        super().__init__(maxDepth, maxBins, minInstancesPerNode, minWeightFractionPerNode,
                         minInfoGain, impurity, seed, numClasses, categoricalFeaturesInfo,
                         workspaceBytes)

    def classes(self, max_label) -> int:
        """numClasses, or the largest label + 1 (agreed over the ranks)."""
        if self.numClasses is not None:
            return self.numClasses
        m = max_label()
        _require(m == m and 0.0 <= m < MAX_CLASSES,
                 f"DecisionTree supports 1 to {MAX_CLASSES} classes but the largest label is {m}.")
        C = int(m) + 1
        check_classes(C, self.maxBins)
        return C

    def fit_step(self, step, d: int, numClasses: int) -> DecisionTreeClassificationModel:
        """The fit over any step object (DeviceStep, NumpyStep)."""
        root, _ = self._grow(step, d, numClasses)
        return DecisionTreeClassificationModel(root, d, numClasses)

    def fit(self, X, y, weights=None) -> DecisionTreeClassificationModel:
        import torch
        from . import parallel
        check_rows(X)
        DTPlan._vector(y, int(X.shape[0]), torch.float64, "labels")
        checked = False
        if self.numClasses is None:
            # the rows' checks come before the class count: a bad label is refused by its
            # row, and the largest label is then an integer below MAX_CLASSES
            wide = DTPlan(int(X.shape[1]), MAX_CLASSES)
            parallel.agree(lambda: wide.check(X, y, weights))
            wide.close()
            checked = True
        C = self.classes(lambda: parallel.max_over_ranks(
            float(y.max().item()) if y.numel() else 0.0, X.device))
        step = DeviceStep(X, y, weights, C, self.workspaceBytes, checked=checked)
        return self.fit_step(step, int(X.shape[1]), C)


class DecisionTreeRegressor(_TreeEstimator):
    """ml/regression/DecisionTreeRegressor.scala's estimator over dense fp64
    device rows; with several ranks every rank calls fit on its shard."""

    def __init__(self, maxDepth: int = 5, maxBins: int = 32, minInstancesPerNode: int = 1,
                 minWeightFractionPerNode: float = 0.0, minInfoGain: float = 0.0,
                 impurity: str = "variance", seed: int = 0, categoricalFeaturesInfo=None,
                 workspaceBytes: int = 0):
        super().__init__(maxDepth, maxBins, minInstancesPerNode, minWeightFractionPerNode,
                         minInfoGain, impurity, seed, None, categoricalFeaturesInfo,
                         workspaceBytes)

    def fit_step(self, step, d: int) -> DecisionTreeRegressionModel:
        root, _ = self._grow(step, d, 0)
        return DecisionTreeRegressionModel(root, d)

    def fit(self, X, y, weights=None) -> DecisionTreeRegressionModel:
        check_rows(X)
        return self.fit_step(DeviceStep(X, y, weights, 0, self.workspaceBytes), int(X.shape[1]))
