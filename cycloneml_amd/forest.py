"""RandomForestClassifier / RandomForestRegressor (ml/tree/impl/RandomForest.scala,
DecisionTreeMetadata.scala, BaggedPoint.scala, ml/tree/treeModels.scala and
ml/classification|regression/RandomForest*.scala, Spark 3.3) over dense fp64
device rows, continuous features, optional row weights.  The kernels are
csrc/random_forest.hip (cyc_rf_* in include/cyclone.h); the rows' checks, the
split candidates, the binned image, the impurities, the split search, pruning
and the trees themselves are tree.py's, unchanged.

Fit (grow_forest).  The rows are binned once; every tree t has a bag, an
integer numSamples[t][r] per row; the level loop is level-synchronous over ALL
trees: the live nodes of every tree at a level, in (tree, node) order, are cut
into calls of at most min(4096, HIST_BYTES // (8 m B S)) nodes, a call gives the
histogram node x subset feature x bin x stats of its nodes, best_splits picks
every node's split among its m features, and one route per level moves the rows
of all trees.  A row adds numSamples w to its label's statistic (numSamples w,
(numSamples w) y, ((numSamples w) y) y for the variance) and numSamples to the
raw count, which minInstancesPerNode tests; minWeightFractionPerNode multiplies
the un-bagged sum of the weights.  grow_forest is prepare_step (the rows'
checks, the totals, the thresholds and the image, once per fit) followed by
grow_prepared (the bag and the level loop); a boosted fit (gbt.py) prepares
once and grows a forest of one tree per iteration on the step's current labels.

The step object adds to tree.py's: bag(numTrees, table, seed), histogram(t0,
t1, slotStart, nodeOf, K, B, nodeFeat, m) over the trees [t0, t1) and
route(slotStart, table) over all trees.  Per-tree tables are concatenated:
tree t's slots are the entries slotStart[t] .. slotStart[t + 1].
ForestDeviceStep (the kernels; histograms go through parallel.allreduce_ once
per call, so every rank calls fit) and ForestNumpyStep (host rows) are
interchangeable.

This project's own rules (Spark's commons-math Poisson sampler and its
stack-ordered reservoir sampling are not restated, so a fit does not reproduce a
Spark run's forest).  One counter-based 64-bit mix supplies the randomness:

    mix(seed, stream, tree, index) = fin(fin(fin(seed + G) + G (2 tree + stream + 1))
                                         + G (index + 1))             (mod 2^64)

fin = splitmix64's finaliser, G = 0x9E3779B97F4A7C15.  Bag (stream 0): index is
the GLOBAL row, so the bag does not depend on the number of ranks; u = the top
53 bits, the count is the number of entries <= u of an ascending table of
floor(cdf_k 2^53): Poisson(subsamplingRate) with p_0 = exp(-rate), p_k = (p_(k-1)
rate) / k, the table ending with 2^53 once the cdf reaches 1 or stops growing;
Bernoulli(rate) has the one entry floor((1 - rate) 2^53).  Feature subsets
(stream 1): the subset of node i of tree t is a function of (seed, t, i) alone,
h = mix(seed, 1, t, i), a partial Fisher-Yates over 0 .. d - 1 whose step j = 0 ..
m - 1 swaps positions j and j + fin(h + G (j + 1)) mod (d - j), the first m
positions sorted ascending.  Call grouping, level order and workspace size
therefore cannot change a forest.
"""
from __future__ import annotations

import ctypes
import math
import re

import numpy as np

from . import _native as N
from . import tree as T
from .tree import (DecisionTreeClassificationModel, DecisionTreeClassifier,
                   DecisionTreeRegressionModel, DeviceStep, NumpyStep, _require)

MAX_TREES = 4096                                  # cyc_rf_max_trees
MAX_PAIRS = 2 ** 31 - 1                           # (tree1 - tree0) n of one histogram call
STREAM_BAG, STREAM_FEATURES = 0, 1
TWO53 = 1 << 53
_G = np.uint64(0x9E3779B97F4A7C15)
_M1 = np.uint64(0xBF58476D1CE4E5B9)
_M2 = np.uint64(0x94D049BB133111EB)
STRATEGIES = ("auto", "all", "onethird", "sqrt", "log2")


# ------------------------------------------------------------------ randomness
def _u64(x):
    if isinstance(x, np.ndarray):
        return x.astype(np.uint64)
    return np.array([int(x) % (1 << 64)], dtype=np.uint64)


def fin(z):
    """splitmix64's finaliser over a uint64 array."""
    with np.errstate(over="ignore"):
        z = z ^ (z >> np.uint64(30))
        z = z * _M1
        z = z ^ (z >> np.uint64(27))
        z = z * _M2
        return z ^ (z >> np.uint64(31))


def mix(seed, stream, tree, index):
    """The uint64 array mix(seed, stream, tree, index); the arguments are
    integers or integer arrays that broadcast."""
    with np.errstate(over="ignore"):
        h0 = fin(_u64(int(seed)) + _G)
        h1 = fin(h0 + _G * (np.uint64(2) * _u64(tree) + _u64(stream) + np.uint64(1)))
        return fin(h1 + _G * (_u64(index) + np.uint64(1)))


def poisson_table(rate: float):
    """floor(cdf_k 2^53), k = 0, 1, .., of Poisson(rate), ending with 2^53."""
    p = math.exp(-float(rate))
    cdf, k, out = p, 0, []
    while True:
        v = int(math.floor(min(cdf, 1.0) * TWO53))
        out.append(v)
        if v >= TWO53:
            break
        k += 1
        p = (p * float(rate)) / k
        nxt = cdf + p
        if nxt == cdf:
            out.append(TWO53)
            break
        cdf = nxt
    _require(len(out) <= 255, "the bag's counts must fit a byte")
    return np.array(out, dtype=np.uint64)


def bernoulli_table(rate: float):
    return np.array([int(math.floor((1.0 - float(rate)) * TWO53))], dtype=np.uint64)


def bag_table(bootstrap: bool, subsamplingRate: float):
    """The table of the bag's counts; None: every row once, no array kept."""
    if bootstrap:
        return poisson_table(subsamplingRate)
    if float(subsamplingRate) < 1.0:
        return bernoulli_table(subsamplingRate)
    return None


def bag_counts(seed: int, numTrees: int, n: int, table, rowOffset: int = 0):
    """numSamples (numTrees x n, uint8) of the rows rowOffset .. rowOffset + n."""
    table = np.asarray(table, dtype=np.uint64)
    rows = np.arange(int(rowOffset), int(rowOffset) + int(n), dtype=np.uint64)
    out = np.empty((int(numTrees), int(n)), dtype=np.uint8)
    for t in range(int(numTrees)):
        u = mix(seed, STREAM_BAG, t, rows) >> np.uint64(11)
        out[t] = np.searchsorted(table, u, side="right")        # the entries <= u
    return out


def feature_subset(seed: int, tree: int, node: int, d: int, m: int):
    """The m features of node `node` of tree `tree`, ascending."""
    if m >= d:
        return np.arange(d, dtype=np.int32)
    h = mix(seed, STREAM_FEATURES, tree, node)
    with np.errstate(over="ignore"):
        draws = fin(h + _G * np.arange(1, m + 1, dtype=np.uint64)).tolist()
    moved = {}                          # the positions of 0 .. d - 1 that no longer hold themselves
    out = []
    for j in range(m):
        k = j + draws[j] % (d - j)
        vj, vk = moved.get(j, j), moved.get(k, k)
        moved[j], moved[k] = vk, vj
        out.append(vk)
    return np.array(sorted(out), dtype=np.int32)


def num_features_per_node(featureSubsetStrategy, numTrees: int, d: int, classifier: bool) -> int:
    """DecisionTreeMetadata.buildMetadata's numFeaturesPerNode."""
    s = str(featureSubsetStrategy).lower()
    if s == "auto":
        s = "all" if int(numTrees) == 1 else ("sqrt" if classifier else "onethird")
    if s == "all":
        return int(d)
    if s == "sqrt":
        return int(math.ceil(math.sqrt(d)))
    if s == "log2":
        return max(1, int(math.ceil(math.log(d) / math.log(2))))
    if s == "onethird":
        return int(math.ceil(d / 3.0))
    if re.fullmatch(r"[+-]?\d+", s) and int(s) > 0:
        return min(int(s), int(d))
    try:
        f = float(s) if re.fullmatch(r"[+-]?(\d+\.?\d*|\.\d+)([eE][+-]?\d+)?", s) else math.nan
    except ValueError:
        f = math.nan
    if 0.0 < f <= 1.0:
        return int(math.ceil(f * d))
    raise N.IllegalArgumentException(
        f"Supported values: {', '.join(STRATEGIES)}, (0.0-1.0], [1-n]. The given value was "
        f"{featureSubsetStrategy}.")


def check_forest_params(numTrees, subsamplingRate):
    _require(1 <= int(numTrees) <= MAX_TREES,
             f"RandomForest takes numTrees in [1, {MAX_TREES}] but got {numTrees}.")
    _require(0.0 < float(subsamplingRate) <= 1.0,
             f"subsamplingRate must be in (0, 1] but got {subsamplingRate}.")


# ------------------------------------------------------------------ level loop
def forest_nodes_per_call(m: int, B: int, S: int, maxNodes: int = T.MAX_NODES) -> int:
    return int(min(maxNodes, T.MAX_NODES, max(1, T.HIST_BYTES // (8 * m * B * S))))


def grow_forest(step, d: int, numClasses: int, impurity: str, numTrees: int,
                numFeaturesPerNode: int, maxDepth: int = 5, maxBins: int = 32,
                minInstancesPerNode: int = 1, minWeightFractionPerNode: float = 0.0,
                minInfoGain: float = 0.0, bootstrap: bool = True, subsamplingRate: float = 1.0,
                seed: int = 0, pruneTree: bool = True, nodesPerCall=None):
    """The level loop over `step`: (the roots in tree order, thresholds)."""
    T.check_params(maxDepth, maxBins, minInstancesPerNode, minWeightFractionPerNode, minInfoGain,
                   impurity, bool(numClasses))
    check_forest_params(numTrees, subsamplingRate)
    m = int(numFeaturesPerNode)
    _require(1 <= m <= d, f"numFeaturesPerNode must be in [1, {d}] but got {m}")
    thresholds, _, wsum = prepare_step(step, maxBins, seed)
    roots = grow_prepared(step, d, numClasses, impurity, numTrees, m, thresholds, wsum, maxDepth,
                          minInstancesPerNode, minWeightFractionPerNode, minInfoGain, bootstrap,
                          subsamplingRate, seed, pruneTree, nodesPerCall)
    return roots, thresholds


def prepare_step(step, maxBins: int, seed: int):
    """What a fit does once with its rows: the rows' checks, the totals, the
    split candidates from the sample and the binned image.  (thresholds, n, the
    un-bagged sum of the weights)."""
    step.check()
    n, wsum = step.totals()
    _require(n > 0, "DecisionTree requires size of input RDD > 0, but was given by empty one.")
    thresholds = T.all_splits(*step.sample(T.sample_rows(maxBins, n, seed)), maxBins, n, wsum)
    step.bin(thresholds)
    return thresholds, n, wsum


def grow_prepared(step, d: int, numClasses: int, impurity: str, numTrees: int,
                  numFeaturesPerNode: int, thresholds, wsum: float, maxDepth: int = 5,
                  minInstancesPerNode: int = 1, minWeightFractionPerNode: float = 0.0,
                  minInfoGain: float = 0.0, bootstrap: bool = True, subsamplingRate: float = 1.0,
                  seed: int = 0, pruneTree: bool = True, nodesPerCall=None):
    """The bag and the level loop over a step that prepare_step has binned (a
    boosted fit grows many forests of one tree over one image, each on the
    step's current labels): the roots in tree order."""
    m, nt = int(numFeaturesPerNode), int(numTrees)
    numSplits = np.array([len(t) for t in thresholds], dtype=np.int64)
    B = int(numSplits.max()) + 1
    S = T.num_stats(numClasses)
    step.bag(nt, bag_table(bootstrap, subsamplingRate), seed)
    minWeight = float(minWeightFractionPerNode) * wsum
    per_call = int(nodesPerCall) if nodesPerCall else \
        forest_nodes_per_call(m, B, S, getattr(step, "maxNodes", T.MAX_NODES))
    nodes = [{} for _ in range(nt)]
    live = [{1: 0} for _ in range(nt)]      # per tree: the nodes to split at this level -> slot
    level = 0
    while any(live):
        slotStart = np.zeros(nt + 1, dtype=np.int32)
        slotStart[1:] = np.cumsum([len(lv) for lv in live])
        table = np.full((int(slotStart[nt]), 4), -1, dtype=np.int32)
        order = [(t, i) for t in range(nt) for i in sorted(live[t])]
        nxt = [{} for _ in range(nt)]
        for g0 in range(0, len(order), per_call):
            group = order[g0:g0 + per_call]
            t0, t1 = group[0][0], group[-1][0] + 1
            ss = (slotStart[t0:t1 + 1] - slotStart[t0]).astype(np.int32)
            nodeOf = np.full(int(ss[-1]), -1, dtype=np.int32)
            for j, (t, i) in enumerate(group):
                nodeOf[ss[t - t0] + live[t][i]] = j
            feats = None if m == d else \
                np.stack([feature_subset(seed, t, i, d, m) for t, i in group])
            hist = step.histogram(t0, t1, ss, nodeOf, len(group), B, feats, m)
            best = T.best_splits(hist, numSplits, numClasses, impurity, minInstancesPerNode,
                                 minWeight, minInfoGain, features=feats)
            for j, (t, i) in enumerate(group):
                if i not in nodes[t]:   # the root: its statistics are the first evaluation's
                    nodes[t][i] = T.Node(best.parent[j], best.impurity[j], numClasses)
                node = nodes[t][i]
                gain = float(best.gain[j])
                if gain <= 0.0 or level == maxDepth:
                    continue
                f, s = int(best.feature[j]), int(best.split[j])
                node.gain = gain
                node.split = (f, float(thresholds[f][s]))
                node.left = T.Node(best.left[j], best.leftImp[j], numClasses)
                node.right = T.Node(best.right[j], best.rightImp[j], numClasses)
                nodes[t][2 * i], nodes[t][2 * i + 1] = node.left, node.right
                new = []
                for child, idx in ((node.left, 2 * i), (node.right, 2 * i + 1)):
                    if level + 1 == maxDepth or abs(child.impurity) < T.EPSILON:
                        new.append(-1)
                    else:
                        nxt[t][idx] = len(nxt[t])
                        new.append(nxt[t][idx])
                table[slotStart[t] + live[t][i]] = (f, s, new[0], new[1])
        if any(nxt):
            step.route(slotStart, table)
        live = nxt
        level += 1
    roots = [nodes[t][1] for t in range(nt)]
    return [T.prune(r) if pruneTree else r for r in roots]


# ----------------------------------------------------------------------- steps
class RFPlan:
    """cyc_rf_plan: the width of the rows, the number of classes (0: the
    variance statistics) and the device workspace (workspaceBytes 0: 256 MiB)."""

    def __init__(self, numFeatures: int, numClasses: int = 0, workspaceBytes: int = 0):
        _require(1 <= int(numFeatures) <= T.MAX_FEATURES,
                 f"RandomForest supports 1 to {T.MAX_FEATURES} features but got {numFeatures}")
        self.numFeatures, self.numClasses = int(numFeatures), int(numClasses)
        self._lib = N.load()
        h = ctypes.c_void_p()
        N.check(self._lib.cyc_rf_plan_create(self.numFeatures, self.numClasses,
                                             int(workspaceBytes), ctypes.byref(h)))
        self.handle = h
        self.numStats = int(self._lib.cyc_rf_num_stats(h))
        self.runRows = int(self._lib.cyc_rf_run_rows())
        self.maxNodes = int(self._lib.cyc_rf_max_nodes())
        self.maxTrees = int(self._lib.cyc_rf_max_trees())
        self.maxPairs = MAX_PAIRS           # histogram() cuts a tree range above it

    def close(self):
        if getattr(self, "handle", None):
            self._lib.cyc_rf_plan_destroy(self.handle)
            self.handle = None

    __del__ = close

    def sub_runs(self, numSubset: int) -> int:
        return int(self._lib.cyc_rf_sub_runs(int(numSubset)))

    def runs_per_launch(self, numSubset: int, numBins: int) -> int:
        return int(self._lib.cyc_rf_runs_per_launch(self.handle, int(numSubset), int(numBins)))

    def _image(self, image):
        import torch
        if not torch.is_tensor(image) or not image.is_cuda or image.dtype != torch.uint8 \
                or image.dim() != 2 or int(image.shape[1]) != self.numFeatures \
                or not image.is_contiguous():
            raise N.IllegalArgumentException(
                f"requirement failed: the image must be contiguous uint8 (n x {self.numFeatures}) "
                "on the device")
        return int(image.shape[0])

    @staticmethod
    def _matrix(v, rows, n, dtype, what):
        import torch
        if not torch.is_tensor(v) or not v.is_cuda or v.dtype != dtype or v.dim() != 2 \
                or int(v.shape[1]) != n or int(v.shape[0]) < rows or not v.is_contiguous():
            raise N.IllegalArgumentException(
                f"requirement failed: {what} must be contiguous {dtype} (numTrees x {n}) on the "
                "device")

    def bag(self, n: int, numTrees: int, table, seed: int, rowOffset: int = 0, device="cuda"):
        """The device bag (numTrees x n uint8) of the rows rowOffset .. rowOffset + n."""
        import torch
        table = np.ascontiguousarray(table, dtype=np.uint64)
        out = torch.empty((int(numTrees), int(n)), dtype=torch.uint8, device=device)
        with torch.cuda.device(out.device):
            N.check(self._lib.cyc_rf_bag_dev(self.handle, int(n), int(numTrees), int(rowOffset),
                                             int(seed) % (1 << 64), table.ctypes.data,
                                             int(table.size), N.ptr(out), N.stream_handle()))
        return out

    def route(self, image, slot, slotStart, table):
        import torch
        n = self._image(image)
        slotStart = np.ascontiguousarray(slotStart, dtype=np.int32).ravel()
        nt = int(slotStart.size) - 1
        self._matrix(slot, nt, n, torch.int32, "slot")
        _require(int(slot.shape[0]) == nt, "one row of slots per tree")
        table = np.ascontiguousarray(np.asarray(table, dtype=np.int32).reshape(-1, 4))
        _require(nt >= 1 and int(table.shape[0]) == int(slotStart[-1]),
                 "the table must have slotStart's last entry many rows")
        with torch.cuda.device(image.device):
            N.check(self._lib.cyc_rf_route_dev(self.handle, N.ptr(image), n, nt, N.ptr(slot),
                                               slotStart.ctypes.data, table.ctypes.data,
                                               N.stream_handle()))

    def histogram_call(self, image, y, weights, bag, slot, t0, t1, slotStart, nodeOf, numNodes,
                       numSubset, nodeFeat, numBins):
        """One cyc_rf_histogram_dev call: (numNodes x numSubset x numBins x numStats)."""
        import torch
        n = self._image(image)
        T.DTPlan._vector(y, n, torch.float64, "labels")
        if weights is not None:
            T.DTPlan._vector(weights, n, torch.float64, "weights")
        t0, t1 = int(t0), int(t1)
        if bag is not None:
            self._matrix(bag, t1, n, torch.uint8, "bag")
        if slot is not None:
            self._matrix(slot, t1, n, torch.int32, "slot")
        slotStart = np.ascontiguousarray(slotStart, dtype=np.int32).ravel()
        nodeOf = np.ascontiguousarray(nodeOf, dtype=np.int32).ravel()
        _require(slotStart.size == t1 - t0 + 1 and slotStart.size >= 2
                 and nodeOf.size == int(slotStart[-1]),
                 "slotStart needs an entry per tree and one more, nodeOf its last entry many")
        K, m = int(numNodes), int(numSubset)
        nf = None
        if nodeFeat is not None:
            nf = np.ascontiguousarray(nodeFeat, dtype=np.int32)
            _require(nf.size == K * m, "nodeFeat must be numNodes x numSubset")
        hist = torch.empty((max(K, 0), max(m, 0), int(numBins), self.numStats),
                           dtype=torch.float64, device=image.device)
        with torch.cuda.device(image.device):
            N.check(self._lib.cyc_rf_histogram_dev(
                self.handle, N.ptr(image), N.ptr(y), N.ptr(weights), N.ptr(bag), n, N.ptr(slot),
                t0, t1, slotStart.ctypes.data, nodeOf.ctypes.data, K, m,
                None if nf is None else nf.ctypes.data, int(numBins), N.ptr(hist),
                N.stream_handle()))
        return hist

    def histogram(self, image, y, weights, bag, slot, t0, t1, slotStart, nodeOf, numNodes,
                  numSubset, nodeFeat, numBins):
        """The device histogram of the nodes of the trees [t0, t1); a range of
        more than maxPairs (tree, row) pairs is cut into calls by trees, each
        over its own nodes (a node's sums do not depend on the cut)."""
        import torch
        n = int(image.shape[0]) if torch.is_tensor(image) and image.dim() == 2 else 0
        span = max(1, self.maxPairs // max(n, 1))
        if int(t1) - int(t0) <= span:
            return self.histogram_call(image, y, weights, bag, slot, t0, t1, slotStart, nodeOf,
                                       numNodes, numSubset, nodeFeat, numBins)
        ss = np.asarray(slotStart, dtype=np.int64).ravel()
        nodeOf = np.asarray(nodeOf, dtype=np.int64).ravel()
        K, m = int(numNodes), int(numSubset)
        hist = torch.zeros((K, m, int(numBins), self.numStats), dtype=torch.float64,
                           device=image.device)
        for ta in range(int(t0), int(t1), span):
            tb = min(int(t1), ta + span)
            sub = nodeOf[ss[ta - t0]:ss[tb - t0]]
            ids = np.unique(sub[sub >= 0])
            if not ids.size:
                continue
            remap = np.full(K, -1, dtype=np.int64)
            remap[ids] = np.arange(ids.size)
            part = self.histogram_call(
                image, y, weights, bag, slot, ta, tb, ss[ta - t0:tb - t0 + 1] - ss[ta - t0],
                np.where(sub >= 0, remap[sub], -1), ids.size, m,
                None if nodeFeat is None else np.asarray(nodeFeat).reshape(K, m)[ids], numBins)
            hist[torch.from_numpy(ids).to(image.device)] = part
        return hist

    def predict(self, X, flat, leaf=False, raw=False, prob=False, pred=False):
        """(leaf n x numTrees int32, raw, prob, pred) device tensors of the
        descent through every tree (None for what is not asked for); flat: the
        host arrays of _ForestModel._flatten."""
        import torch
        n = T.check_rows(X, self.numFeatures, "plan")
        nodeStart, leafStart, ft, th, fc, li, lv = flat
        nt, C, dev = int(nodeStart.size) - 1, self.numClasses, X.device
        _require(not (raw or prob) or C > 0, "raw and prob need a classifier")
        lf = torch.empty((n, nt), dtype=torch.int32, device=dev) if leaf else None
        # a classifier's votes are added in the raw output
        r = torch.empty((n, C), dtype=torch.float64, device=dev) \
            if C and (raw or prob or pred) else None
        q = torch.empty((n, C), dtype=torch.float64, device=dev) if prob else None
        p = torch.empty(n, dtype=torch.float64, device=dev) if pred else None
        with torch.cuda.device(dev):
            N.check(self._lib.cyc_rf_predict_dev(
                self.handle, N.ptr(X), n, nt, nodeStart.ctypes.data, leafStart.ctypes.data,
                ft.ctypes.data, th.ctypes.data, fc.ctypes.data, li.ctypes.data, lv.ctypes.data,
                N.ptr(lf), N.ptr(r), N.ptr(q), N.ptr(p), N.stream_handle()))
        return lf, (r if raw else None), q, p


class ForestDeviceStep(DeviceStep):
    """The step over device rows (this rank's shard): the image, the bag and
    the slots of every tree live on the device, a histogram comes back merged
    over the ranks."""

    def __init__(self, X, y, weights=None, numClasses: int = 0, workspaceBytes: int = 0,
                 checked: bool = False):
        super().__init__(X, y, weights, numClasses, workspaceBytes, checked=checked)
        self.rf = RFPlan(self.d, numClasses, workspaceBytes)
        self.maxNodes = self.rf.maxNodes
        self.slot = self.bagCounts = self.rowOffset = None
        self.numTrees = 0

    def bag(self, numTrees: int, table, seed: int):
        import torch
        n = int(self.X.shape[0])
        # the rank's first global row is kept by sample(), from its allgather of the sizes
        _require(self.rowOffset is not None, "bag() follows sample(), which finds the row offset")
        self.numTrees = int(numTrees)
        self.slot = torch.zeros((self.numTrees, n), dtype=torch.int32, device=self.X.device)
        self.bagCounts = None if table is None else \
            self.rf.bag(n, numTrees, table, seed, self.rowOffset, self.X.device)

    def histogram(self, t0, t1, slotStart, nodeOf, K, B, nodeFeat, m):
        from . import parallel
        hist = self.rf.histogram(self.image, self.y, self.weights, self.bagCounts, self.slot, t0,
                                 t1, slotStart, nodeOf, K, m, nodeFeat, B)
        parallel.allreduce_(hist.view(-1))
        return hist.cpu().numpy()

    def route(self, slotStart, table):
        self.rf.route(self.image, self.slot, slotStart, table)


class ForestNumpyStep(NumpyStep):
    """The step over host rows in numpy (the rows rowOffset .. of the whole):
    the same bag, bins and routes as the kernels, the sums in plain row order."""

    def __init__(self, X, y, weights=None, numClasses: int = 0, rowOffset: int = 0):
        super().__init__(X, y, weights, numClasses)
        self.rowOffset = int(rowOffset)
        self.slot = self.bagCounts = None
        self.numTrees = 0

    def bag(self, numTrees: int, table, seed: int):
        n = int(self.X.shape[0])
        self.numTrees = int(numTrees)
        self.slot = np.zeros((self.numTrees, n), dtype=np.int32)
        self.bagCounts = None if table is None else \
            bag_counts(seed, numTrees, n, table, self.rowOffset)

    def histogram(self, t0, t1, slotStart, nodeOf, K, B, nodeFeat, m):
        nodeOf = np.asarray(nodeOf, dtype=np.int64)
        ss = np.asarray(slotStart, dtype=np.int64)
        C = self.numClasses
        S = T.num_stats(C)
        feats = np.broadcast_to(np.arange(self.d), (K, self.d)) if nodeFeat is None else \
            np.asarray(nodeFeat, dtype=np.int64).reshape(K, m)
        hist = np.zeros((K, m, B, S), dtype=np.float64)
        for t in range(t0, t1):
            slot = self.slot[t]
            rows = np.nonzero((slot >= 0) & (slot < ss[t - t0 + 1] - ss[t - t0]))[0]
            node = nodeOf[ss[t - t0] + slot[rows]]
            keep = node >= 0
            if self.bagCounts is not None:
                keep &= self.bagCounts[t, rows] > 0     # a row drawn 0 times is not loaded
            rows, node = rows[keep], node[keep]
            cnt = np.ones(rows.size) if self.bagCounts is None else \
                self.bagCounts[t, rows].astype(np.float64)
            iw = cnt * (np.ones(rows.size) if self.weights is None else self.weights[rows])
            y = self.y[rows]
            if C:
                vals = [(y.astype(np.int64), iw), (np.full(rows.size, C), cnt)]
            else:
                wy = iw * y
                vals = [(np.full(rows.size, s), v) for s, v in enumerate((iw, wy, wy * y, cnt))]
            for j in range(m):
                b = self.image[rows, feats[node, j]].astype(np.int64)
                for s, v in vals:
                    np.add.at(hist, (node, j, b, s), v)      # unbuffered: row order
        return hist

    def route(self, slotStart, table):
        table = np.asarray(table, dtype=np.int32).reshape(-1, 4)
        ss = np.asarray(slotStart, dtype=np.int64)
        out = np.full(self.slot.shape, -1, dtype=np.int32)
        for t in range(self.numTrees):
            slot = self.slot[t]
            ok = np.nonzero((slot >= 0) & (slot < ss[t + 1] - ss[t]))[0]
            e = table[ss[t] + slot[ok]]
            split = e[:, 0] >= 0
            ok, e = ok[split], e[split]
            b = self.image[ok, e[:, 0]].astype(np.int32)
            out[t, ok] = np.where(b <= e[:, 1], e[:, 2], e[:, 3])
        self.slot = out


# ---------------------------------------------------------------------- models
class _ForestModel:
    """What the two models share: the trees (each a DecisionTree*Model usable
    alone), their concatenated flat form and the descent through all of them."""

    numClasses = 0
    treeModel = None

    def __init__(self, trees, numFeatures: int):
        self.trees = list(trees)
        _require(1 <= len(self.trees) <= MAX_TREES,
                 f"a forest has 1 to {MAX_TREES} trees but got {len(self.trees)}")
        self.numFeatures = int(numFeatures)
        for t in self.trees:
            _require(isinstance(t, self.treeModel) and t.numFeatures == self.numFeatures
                     and t.numClasses == self.numClasses,
                     f"every tree must be a {self.treeModel.__name__} of this width and class "
                     "count")
        self.treeWeights = np.ones(len(self.trees), dtype=np.float64)
        self._flat = self._plan = None

    @classmethod
    def from_trees(cls, trees, numFeatures, *args):
        """A model from DecisionTree*Model trees, on the host: no device is
        touched until the first predict."""
        return cls(trees, numFeatures, *args)

    @property
    def getNumTrees(self) -> int:
        return len(self.trees)

    @property
    def totalNumNodes(self) -> int:
        return int(sum(t.numNodes for t in self.trees))

    @property
    def featureImportances(self):
        total = np.zeros(self.numFeatures, dtype=np.float64)
        for t in self.trees:
            total = total + t.featureImportances        # normalised per tree; in tree order
        s = float(np.cumsum(total)[-1])
        return total / s if s != 0.0 else total

    def toDebugString(self) -> str:
        lines = [f"{type(self).__name__}: numTrees={self.getNumTrees}"
                 + (f", numClasses={self.numClasses}" if self.numClasses else "")
                 + f", numFeatures={self.numFeatures}"]
        for i, t in enumerate(self.trees):
            lines.append(f"  Tree {i} (weight {self.treeWeights[i]}):")
            # the tree's own lines, two columns deeper
            lines.extend("  " + ln for ln in t.toDebugString().split("\n")[1:-1])
        return "\n".join(lines) + "\n"

    def _leaf_values(self, t):
        return t._leafPred.reshape(-1, 1)

    def _flatten(self):
        if self._flat is None:
            nodeStart = np.zeros(len(self.trees) + 1, dtype=np.int32)
            leafStart = np.zeros(len(self.trees) + 1, dtype=np.int32)
            nodeStart[1:] = np.cumsum([t.numNodes for t in self.trees])
            leafStart[1:] = np.cumsum([t._leafPred.size for t in self.trees])
            cat = lambda xs, dt: np.ascontiguousarray(np.concatenate(xs), dtype=dt)  # noqa: E731
            self._flat = (nodeStart, leafStart,
                          cat([t._feature for t in self.trees], np.int32),
                          cat([t._threshold for t in self.trees], np.float64),
                          cat([t._first for t in self.trees], np.int32),
                          cat([t._leaf for t in self.trees], np.int32),
                          cat([self._leaf_values(t) for t in self.trees], np.float64))
        return self._flat

    def _run(self, X, **what):
        T.check_rows(X, self.numFeatures)
        if self._plan is None:
            self._plan = RFPlan(self.numFeatures, self.numClasses)
        return self._plan.predict(X, self._flatten(), **what)

    def predict(self, X):
        return self._run(X, pred=True)[3]

    def predictLeaf(self, X):
        return self._run(X, leaf=True)[0]


def leaf_votes(counts):
    """counts / total per leaf (numLeaves x C), total the left-to-right sum of
    the leaf's class weights; a leaf without weight votes zeros."""
    counts = np.asarray(counts, dtype=np.float64)
    total = np.zeros(counts.shape[0], dtype=np.float64)
    for c in range(counts.shape[1]):
        total = total + counts[:, c]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(total[:, None] != 0.0, counts / total[:, None], 0.0)


class RandomForestClassificationModel(_ForestModel):
    treeModel = DecisionTreeClassificationModel

    def __init__(self, trees, numFeatures: int, numClasses: int):
        self.numClasses = int(numClasses)
        super().__init__(trees, numFeatures)

    def _leaf_values(self, t):
        return leaf_votes(t._leafRaw)

    def predictRaw(self, X):
        return self._run(X, raw=True)[1]

    def predictProbability(self, X):
        return self._run(X, prob=True)[2]


class RandomForestRegressionModel(_ForestModel):
    treeModel = DecisionTreeRegressionModel


# ------------------------------------------------------------------ estimators
class _ForestEstimator:
    classifier = False

    def __init__(self, numTrees, maxDepth, maxBins, minInstancesPerNode, minWeightFractionPerNode,
                 minInfoGain, impurity, featureSubsetStrategy, subsamplingRate, bootstrap, seed,
                 numClasses, categoricalFeaturesInfo, workspaceBytes):
        T.check_params(maxDepth, maxBins, minInstancesPerNode, minWeightFractionPerNode,
                       minInfoGain, impurity, self.classifier, categoricalFeaturesInfo)
        check_forest_params(numTrees, subsamplingRate)
        if numClasses is not None:
            T.check_classes(numClasses, maxBins)
        # the strategy's own refusals do not wait for the rows (d = 1 names every form)
        num_features_per_node(featureSubsetStrategy, numTrees, 1, self.classifier)
        self.numTrees, self.maxDepth, self.maxBins = int(numTrees), int(maxDepth), int(maxBins)
        self.minInstancesPerNode = int(minInstancesPerNode)
        self.minWeightFractionPerNode = float(minWeightFractionPerNode)
        self.minInfoGain, self.impurity, self.seed = float(minInfoGain), impurity, int(seed)
        self.featureSubsetStrategy = str(featureSubsetStrategy)
        self.subsamplingRate, self.bootstrap = float(subsamplingRate), bool(bootstrap)
        self.numClasses = None if numClasses is None else int(numClasses)
        self.workspaceBytes = int(workspaceBytes)

    def numFeaturesPerNode(self, d: int) -> int:
        return num_features_per_node(self.featureSubsetStrategy, self.numTrees, d, self.classifier)

    def _grow(self, step, d, C, nodesPerCall=None):
        return grow_forest(step, d, C, self.impurity, self.numTrees, self.numFeaturesPerNode(d),
                           self.maxDepth, self.maxBins, self.minInstancesPerNode,
                           self.minWeightFractionPerNode, self.minInfoGain, self.bootstrap,
                           self.subsamplingRate, self.seed, nodesPerCall=nodesPerCall)


class RandomForestClassifier(_ForestEstimator):
    """ml/classification/RandomForestClassifier.scala's estimator over dense
    fp64 device rows; with several ranks every rank calls fit on its shard."""

    classifier = True

    def __init__(self, numTrees: int = 20, maxDepth: int = 5, maxBins: int = 32,
                 minInstancesPerNode: int = 1, minWeightFractionPerNode: float = 0.0,
                 minInfoGain: float = 0.0, impurity: str = "gini",
                 featureSubsetStrategy: str = "auto", subsamplingRate: float = 1.0,
                 bootstrap: bool = True, seed: int = 0, numClasses=None, workspaceBytes: int = 0,
                 categoricalFeaturesInfo=None):
        super().__init__(numTrees, maxDepth, maxBins, minInstancesPerNode,
                         minWeightFractionPerNode, minInfoGain, impurity, featureSubsetStrategy,
                         subsamplingRate, bootstrap, seed, numClasses, categoricalFeaturesInfo,
                         workspaceBytes)

    def fit_step(self, step, d: int, numClasses: int, nodesPerCall=None):
        """The fit over any step object (ForestDeviceStep, ForestNumpyStep)."""
        roots, _ = self._grow(step, d, numClasses, nodesPerCall)
        return RandomForestClassificationModel(
            [DecisionTreeClassificationModel(r, d, numClasses) for r in roots], d, numClasses)

    def fit(self, X, y, weights=None) -> RandomForestClassificationModel:
        import torch
        from . import parallel
        T.check_rows(X)
        T.DTPlan._vector(y, int(X.shape[0]), torch.float64, "labels")
        checked = False
        if self.numClasses is None:
            # as DecisionTreeClassifier.fit: the rows' checks come before the class count
            wide = T.DTPlan(int(X.shape[1]), T.MAX_CLASSES)
            parallel.agree(lambda: wide.check(X, y, weights))
            wide.close()
            checked = True
        C = DecisionTreeClassifier(maxBins=self.maxBins, numClasses=self.numClasses).classes(
            lambda: parallel.max_over_ranks(float(y.max().item()) if y.numel() else 0.0, X.device))
        step = ForestDeviceStep(X, y, weights, C, self.workspaceBytes, checked=checked)
        return self.fit_step(step, int(X.shape[1]), C)


class RandomForestRegressor(_ForestEstimator):
    """ml/regression/RandomForestRegressor.scala's estimator over dense fp64
    device rows; with several ranks every rank calls fit on its shard."""

    def __init__(self, numTrees: int = 20, maxDepth: int = 5, maxBins: int = 32,
                 minInstancesPerNode: int = 1, minWeightFractionPerNode: float = 0.0,
                 minInfoGain: float = 0.0, impurity: str = "variance",
                 featureSubsetStrategy: str = "auto", subsamplingRate: float = 1.0,
                 bootstrap: bool = True, seed: int = 0, workspaceBytes: int = 0,
                 categoricalFeaturesInfo=None):
        super().__init__(numTrees, maxDepth, maxBins, minInstancesPerNode,
                         minWeightFractionPerNode, minInfoGain, impurity, featureSubsetStrategy,
                         subsamplingRate, bootstrap, seed, None, categoricalFeaturesInfo,
                         workspaceBytes)

    def fit_step(self, step, d: int, nodesPerCall=None):
        roots, _ = self._grow(step, d, 0, nodesPerCall)
        return RandomForestRegressionModel([DecisionTreeRegressionModel(r, d) for r in roots], d)

    def fit(self, X, y, weights=None) -> RandomForestRegressionModel:
        T.check_rows(X)
        return self.fit_step(ForestDeviceStep(X, y, weights, 0, self.workspaceBytes),
                             int(X.shape[1]))
