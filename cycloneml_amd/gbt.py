"""GBTClassifier / GBTRegressor (ml/tree/impl/GradientBoostedTrees.scala,
mllib/tree/loss/{LogLoss,SquaredError,AbsoluteError}.scala and
ml/{classification/GBTClassifier,regression/GBTRegressor}.scala, Spark 3.3) over
dense fp64 device rows, continuous features, optional row weights.  The kernels
are csrc/gbt.hip (cyc_gbt_* in include/cyclone.h); a tree is grown by forest.py's
level loop (a forest of one variance tree) over tree.py's binned image.

Fit (boost).  The rows are checked, sampled for the split candidates and binned
ONCE (forest.prepare_step).  Iteration m = 0 .. maxIter - 1 grows one tree with
seed + m (the bag: Bernoulli(subsamplingRate) without replacement below rate 1,
none otherwise; the subsets: feature_subset(seed + m, 0, node, d, m)) on the
step's current labels: tree 0 on the labels themselves (a classifier's 0 / 1
labels become -1 / +1) with weight 1.0, tree m > 0 on -gradient(pred, label) with
weight stepSize.  After every tree the step's update(tree, weight, loss) walks
the tree over the binned image for every row (Spark walks its binned points
there too), sets pred <- pred + leaf weight (the product rounded before the add,
pred from 0.0), the next residual, and returns (sum of w e, sum of w).  Losses,
F the prediction and y the label:

    squared   g = -2 (y - F)                 e = (y - F) (y - F)
    absolute  g = y - F < 0 ? 1 : -1         e = |y - F|
    logistic  g = -4 y / (1 + exp(2 y F))    e = 2 log1pExp(-2 y F)

Validation rows (fit's validation = (Xv, yv, wv | None), Spark's
validationIndicatorCol) are binned with the training thresholds and carried
through the same update without residuals; the weighted mean error sum w e / sum
w after tree 0 is the first best; after tree m boosting ends when best - current
< validationTol max(current, 0.01), else a smaller error becomes the best with
bestM = m + 1; the model keeps the first bestM trees.

The step objects add to forest.py's: set_labels(), update(flatTree, weight, loss)
and residual().  GBTDeviceStep (the kernels; the two sums go through one
parallel.allreduce_) and GBTNumpyStep (host rows) are interchangeable.

This package's own rules: the bag is forest.py's counter-based Bernoulli draw,
not Spark's, so a subsampled fit does not reproduce a Spark run.  Out of scope:
multiclass, categorical features, CSR rows, leafCol, save / load, thresholds,
transform.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np

from . import _native as N
from . import forest as RF
from . import tree as T
from .ann import java_string_hash
from .tree import DecisionTreeRegressionModel, _require

LOSSES = {"squared": 0, "absolute": 1, "logistic": 2}       # cyc_gbt_update_dev's codes
CLASSIFIER_SEED = java_string_hash("org.apache.spark.ml.classification.GBTClassifier")
REGRESSOR_SEED = java_string_hash("org.apache.spark.ml.regression.GBTRegressor")


# ---------------------------------------------------------------------- losses
def _exp(x: float) -> float:
    """java.lang.Math.exp: Infinity where the math module raises."""
    try:
        return math.exp(x)
    except OverflowError:
        return math.inf


def log1p_exp(x: float) -> float:
    """MLUtils.log1pExp."""
    return x + math.log1p(math.exp(-x)) if x > 0 else math.log1p(math.exp(x))


def neg_gradient_and_error(loss: str, pred, y):
    """(-gradient, error) of every row, host arrays; the logistic loss goes
    row by row through the scalar exp and log1p."""
    pred, y = np.asarray(pred, dtype=np.float64), np.asarray(y, dtype=np.float64)
    if loss == "logistic":
        g = np.array([-4.0 * b / (1.0 + _exp(2.0 * b * a)) for a, b in zip(pred, y)],
                     dtype=np.float64).reshape(y.shape)
        e = np.array([2.0 * log1p_exp(-(2.0 * b * a)) for a, b in zip(pred, y)],
                     dtype=np.float64).reshape(y.shape)
        return -g, e
    diff = y - pred
    if loss == "squared":
        return -(-2.0 * diff), diff * diff
    _require(loss == "absolute", f"unknown loss {loss}")
    return -np.where(diff < 0.0, 1.0, -1.0), np.abs(diff)


# ------------------------------------------------------------------ flat trees
class FlatTree:
    """One tree as host arrays in cyc_dt_predict_dev's breadth-first form, with
    the leaf's prediction per NODE and, given the fit's thresholds, the split of
    every internal node as a bin: the position of its threshold among its
    feature's (strictly ascending) thresholds."""

    def __init__(self, feature, threshold, firstChild, leafIndex, value, thresholds=None):
        self.feature = np.ascontiguousarray(feature, dtype=np.int32)
        self.threshold = np.ascontiguousarray(threshold, dtype=np.float64)
        self.firstChild = np.ascontiguousarray(firstChild, dtype=np.int32)
        self.leafIndex = np.ascontiguousarray(leafIndex, dtype=np.int32)
        self.value = np.ascontiguousarray(value, dtype=np.float64)
        self.splitBin = None
        if thresholds is not None:
            self.splitBin = np.full(self.feature.size, -1, dtype=np.int32)
            for i in np.nonzero(self.firstChild >= 0)[0]:
                t = np.asarray(thresholds[int(self.feature[i])], dtype=np.float64)
                s = int(np.searchsorted(t, self.threshold[i], "left"))
                _require(s < t.size and t[s] == self.threshold[i],
                         f"the threshold of node {i} is none of its feature's split candidates")
                self.splitBin[i] = s

    @property
    def numNodes(self) -> int:
        return int(self.feature.size)


def flat_tree(root, thresholds=None) -> FlatTree:
    """FlatTree of a fitted tree (tree.py's Node)."""
    ft, th, fc, li, leaves = T.flatten_tree(root)
    pred = np.array([nd.prediction for nd in leaves], dtype=np.float64)
    return FlatTree(ft, th, fc, li, np.where(li >= 0, pred[np.maximum(li, 0)], 0.0), thresholds)


def flat_model_tree(t) -> FlatTree:
    """FlatTree of a DecisionTreeRegressionModel (no bins: for fp64 rows)."""
    return FlatTree(t._feature, t._threshold, t._first, t._leaf,
                    np.where(t._leaf >= 0, t._leafPred[np.maximum(t._leaf, 0)], 0.0))


# ------------------------------------------------------------------------ plan
class GBTPlan:
    """cyc_gbt_plan: the width of the rows and the scratch of the two calls."""

    def __init__(self, numFeatures: int):
        _require(1 <= int(numFeatures) <= T.MAX_FEATURES,
                 f"GBT supports 1 to {T.MAX_FEATURES} features but got {numFeatures}")
        self.numFeatures = int(numFeatures)
        self._lib = N.load()
        h = ctypes.c_void_p()
        N.check(self._lib.cyc_gbt_plan_create(self.numFeatures, ctypes.byref(h)))
        self.handle = h
        self.ldsNodes = int(self._lib.cyc_gbt_lds_nodes())
        self.maxTrees = int(self._lib.cyc_gbt_max_trees())

    def close(self):
        if getattr(self, "handle", None):
            self._lib.cyc_gbt_plan_destroy(self.handle)
            self.handle = None

    __del__ = close

    def update(self, rows, flat: FlatTree, treeWeight: float, loss: str, y, weights, pred,
               resid=None, sums=None):
        """One cyc_gbt_update_dev call.  rows: the uint8 image (flat needs its
        bins) or fp64 rows; pred is updated in place, resid (None: not wanted) is
        set; returns sums (2 doubles on the device: sum of w e, sum of w)."""
        import torch
        _require(loss in LOSSES, f"unknown loss {loss}")
        _require(torch.is_tensor(rows) and rows.is_cuda and rows.dim() == 2
                 and int(rows.shape[1]) == self.numFeatures and rows.is_contiguous()
                 and rows.dtype in (torch.uint8, torch.float64),
                 f"rows must be a contiguous uint8 image or fp64 rows (n x {self.numFeatures}) on "
                 "the device")
        image = rows.dtype == torch.uint8
        _require(not image or flat.splitBin is not None, "the image needs a tree with split bins")
        n = int(rows.shape[0])
        T.DTPlan._vector(y, n, torch.float64, "labels")
        T.DTPlan._vector(pred, n, torch.float64, "pred")
        if weights is not None:
            T.DTPlan._vector(weights, n, torch.float64, "weights")
        if resid is not None:
            T.DTPlan._vector(resid, n, torch.float64, "resid")
        if sums is None:
            sums = torch.empty(2, dtype=torch.float64, device=rows.device)
        T.DTPlan._vector(sums, 2, torch.float64, "sums")
        with torch.cuda.device(rows.device):
            N.check(self._lib.cyc_gbt_update_dev(
                self.handle, N.ptr(rows) if image else None, None if image else N.ptr(rows), n,
                flat.numNodes, flat.feature.ctypes.data,
                flat.splitBin.ctypes.data if image else None,
                None if image else flat.threshold.ctypes.data, flat.firstChild.ctypes.data,
                flat.value.ctypes.data, float(treeWeight), LOSSES[loss], N.ptr(y), N.ptr(weights),
                N.ptr(pred), N.ptr(resid), N.ptr(sums), N.stream_handle()))
        return sums

    def predict(self, X, flats, treeWeights, classifier: bool, leaf=False, margin=False,
                raw=False, prob=False, pred=False):
        """(leaf n x numTrees int32, margin, raw n x 2, prob n x 2, pred) device
        tensors of the descent through the FlatTrees in order (None for what is
        not asked for)."""
        import torch
        n = T.check_rows(X, self.numFeatures, "plan")
        nt, dev = len(flats), X.device
        tw = np.ascontiguousarray(treeWeights, dtype=np.float64)
        _require(tw.size == nt and nt >= 1, "one weight per tree")
        _require(not (raw or prob) or classifier, "raw and prob need a classifier")
        nodeStart = np.zeros(nt + 1, dtype=np.int32)
        nodeStart[1:] = np.cumsum([f.numNodes for f in flats])
        cat = lambda name, dt: np.ascontiguousarray(          # noqa: E731
            np.concatenate([getattr(f, name) for f in flats]), dtype=dt)
        ft, fc, li = cat("feature", np.int32), cat("firstChild", np.int32), cat("leafIndex", np.int32)
        th, va = cat("threshold", np.float64), cat("value", np.float64)
        lf = torch.empty((n, nt), dtype=torch.int32, device=dev) if leaf else None
        mg = torch.empty(n, dtype=torch.float64, device=dev) if margin else None
        r = torch.empty((n, 2), dtype=torch.float64, device=dev) if raw else None
        q = torch.empty((n, 2), dtype=torch.float64, device=dev) if prob else None
        p = torch.empty(n, dtype=torch.float64, device=dev) if pred else None
        with torch.cuda.device(dev):
            N.check(self._lib.cyc_gbt_predict_dev(
                self.handle, N.ptr(X), n, nt, nodeStart.ctypes.data, ft.ctypes.data,
                th.ctypes.data, fc.ctypes.data, li.ctypes.data, va.ctypes.data, tw.ctypes.data,
                int(bool(classifier)), N.ptr(lf), N.ptr(mg), N.ptr(r), N.ptr(q), N.ptr(p),
                N.stream_handle()))
        return lf, mg, r, q, p


# ----------------------------------------------------------------------- steps
class GBTDeviceStep(RF.ForestDeviceStep):
    """The step over device rows (this rank's shard).  y is what the next tree
    is fitted to (the labels, then the residuals, written by the kernel); labels
    and pred stay on the device.  residuals=False: a validation step."""

    def __init__(self, X, y, weights=None, classifier: bool = False, workspaceBytes: int = 0,
                 residuals: bool = True):
        super().__init__(X, y, weights, 0, workspaceBytes)
        self.classifier, self.residuals = bool(classifier), bool(residuals)
        self.gbt = GBTPlan(self.d)
        self.labels = self.pred = self.sums = None

    def check(self):
        from . import parallel
        if not self.classifier:
            return super().check()
        two = T.DTPlan(self.d, 2)               # the labels are class indices 0, 1
        try:
            parallel.agree(lambda: two.check(self.X, self.y, self.weights))
        finally:
            two.close()

    def set_labels(self, labels=None):
        """The labels of the losses (None: the step's own, a classifier's as
        2 y - 1); pred starts from 0.0."""
        import torch
        if labels is None:
            labels = self.y * 2.0 - 1.0 if self.classifier else self.y
        self.labels = labels
        self.y = labels.clone()
        self.pred = torch.zeros_like(labels)
        self.sums = torch.empty(2, dtype=torch.float64, device=labels.device)

    def update(self, flat: FlatTree, weight: float, loss: str):
        from . import parallel
        rows = self.image if flat.splitBin is not None else self.X
        self.gbt.update(rows, flat, weight, loss, self.labels, self.weights, self.pred,
                        self.y if self.residuals else None, self.sums)
        parallel.allreduce_(self.sums)
        es, ws = self.sums.cpu().tolist()
        return float(es), float(ws)

    def residual(self):
        return self.y.cpu().numpy()


class GBTNumpyStep(RF.ForestNumpyStep):
    """The step over host rows in numpy: the same walk and losses as the
    kernel, the two sums in plain row order."""

    def __init__(self, X, y, weights=None, classifier: bool = False, rowOffset: int = 0,
                 residuals: bool = True):
        super().__init__(X, y, weights, 0, rowOffset)
        self.classifier, self.residuals = bool(classifier), bool(residuals)
        self.labels = self.pred = None

    def check(self):
        self.numClasses = 2 if self.classifier else 0   # the labels are class indices 0, 1
        try:
            super().check()
        finally:
            self.numClasses = 0

    def set_labels(self, labels=None):
        if labels is None:
            labels = self.y * 2.0 - 1.0 if self.classifier else self.y
        self.labels = np.array(labels, dtype=np.float64)
        self.y = self.labels.copy()
        self.pred = np.zeros_like(self.labels)

    def update(self, flat: FlatTree, weight: float, loss: str):
        n = self.labels.size
        node = np.zeros(n, dtype=np.int64)
        while True:
            rows = np.nonzero(flat.firstChild[node] >= 0)[0]
            if not rows.size:
                break
            at = node[rows]
            f = flat.feature[at]
            if flat.splitBin is not None:
                left = self.image[rows, f].astype(np.int64) <= flat.splitBin[at]
            else:
                left = self.X[rows, f] <= flat.threshold[at]
            node[rows] = flat.firstChild[at] + np.where(left, 0, 1)
        self.pred = self.pred + flat.value[node] * float(weight)
        resid, e = neg_gradient_and_error(loss, self.pred, self.labels)
        if self.residuals:
            self.y = resid
        w = np.ones(n) if self.weights is None else self.weights
        if not n:
            return 0.0, 0.0
        return float(np.cumsum(e * w)[-1]), float(np.cumsum(w)[-1])

    def residual(self):
        return self.y


# ------------------------------------------------------------------------ boost
def check_gbt_params(maxIter, stepSize, lossType, allowed, validationTol):
    _require(1 <= int(maxIter) <= RF.MAX_TREES,
             f"maxIter must be in [1, {RF.MAX_TREES}] but got {maxIter}.")
    _require(0.0 < float(stepSize) <= 1.0, f"stepSize must be in (0, 1] but got {stepSize}.")
    if lossType not in allowed:
        raise N.IllegalArgumentException(
            f"lossType given invalid value {lossType}. Supported options: {', '.join(allowed)}.")
    _require(float(validationTol) >= 0.0,
             f"validationTol must not be negative but got {validationTol}.")


def boost(step, d: int, loss: str, maxIter: int = 20, stepSize: float = 0.1, maxDepth: int = 5,
          maxBins: int = 32, minInstancesPerNode: int = 1, minWeightFractionPerNode: float = 0.0,
          minInfoGain: float = 0.0, subsamplingRate: float = 1.0,
          featureSubsetStrategy: str = "all", validationTol: float = 0.01, seed: int = 0,
          validation=None, nodesPerCall=None):
    """GradientBoostedTrees.boost over `step` (and a validation step): (the
    roots, their weights, thresholds)."""
    T.check_params(maxDepth, maxBins, minInstancesPerNode, minWeightFractionPerNode, minInfoGain,
                   "variance", False)
    RF.check_forest_params(1, subsamplingRate)
    check_gbt_params(maxIter, stepSize, loss, tuple(LOSSES), validationTol)
    m = RF.num_features_per_node(featureSubsetStrategy, 1, d, False)
    thresholds, _, wsum = RF.prepare_step(step, maxBins, seed)
    step.set_labels()
    if validation is not None:
        validation.check()
        validation.bin(thresholds)
        validation.set_labels()
    roots, weights = [], []
    best, bestM = None, 1
    for it in range(int(maxIter)):
        (root,) = RF.grow_prepared(step, d, 0, "variance", 1, m, thresholds, wsum, maxDepth,
                                   minInstancesPerNode, minWeightFractionPerNode, minInfoGain,
                                   False, subsamplingRate, int(seed) + it, True, nodesPerCall)
        weight = 1.0 if it == 0 else float(stepSize)
        roots.append(root)
        weights.append(weight)
        flat = flat_tree(root, thresholds)
        step.update(flat, weight, loss)
        if validation is None:
            continue
        es, ws = validation.update(flat, weight, loss)
        current = es / ws
        if it == 0:
            best = current
        elif best - current < float(validationTol) * max(current, 0.01):
            break
        elif current < best:
            best, bestM = current, it + 1
    if validation is not None:
        roots, weights = roots[:bestM], weights[:bestM]
    return roots, np.array(weights, dtype=np.float64), thresholds


# ---------------------------------------------------------------------- models
def tree_importance(root, numFeatures: int):
    """gain count per feature of one tree, NOT normalised."""
    imp = np.zeros(int(numFeatures), dtype=np.float64)

    def walk(nd):
        if nd.isLeaf:
            return
        imp[nd.split[0]] += nd.gain * nd.count
        walk(nd.left)
        walk(nd.right)

    walk(root)
    return imp


class _GBTModel(RF._ForestModel):
    """What the two models share: the trees (DecisionTreeRegressionModels),
    their weights and the descent of cyc_gbt_predict_dev."""

    treeModel = DecisionTreeRegressionModel
    classifier = False

    def __init__(self, trees, treeWeights, numFeatures: int, lossType: str):
        super().__init__(trees, numFeatures)
        self.treeWeights = np.array(treeWeights, dtype=np.float64).ravel()
        _require(self.treeWeights.size == len(self.trees), "one weight per tree")
        self.lossType = lossType

    @classmethod
    def from_trees(cls, trees, treeWeights, numFeatures, *args):
        """A model from DecisionTreeRegressionModel trees and their weights, on
        the host: no device is touched until the first predict."""
        return cls(trees, treeWeights, numFeatures, *args)

    @property
    def featureImportances(self):
        total = np.zeros(self.numFeatures, dtype=np.float64)
        for t in self.trees:
            total = total + tree_importance(t.rootNode, self.numFeatures)   # in tree order
        s = float(np.cumsum(total)[-1])
        return total / s if s != 0.0 else total

    def _flatten(self):
        if self._flat is None:
            self._flat = [flat_model_tree(t) for t in self.trees]
        return self._flat

    def _run(self, X, **what):
        T.check_rows(X, self.numFeatures)
        if self._plan is None:
            self._plan = GBTPlan(self.numFeatures)
        return self._plan.predict(X, self._flatten(), self.treeWeights, self.classifier, **what)

    def predict(self, X):
        return self._run(X, pred=True)[4]

    def evaluate_step(self, step, loss=None):
        """evaluateEachIteration over any step object holding the rows, the
        labels and the weights: the weighted mean error after each tree."""
        loss = self.lossType if loss is None else loss
        _require(loss in LOSSES, f"unknown loss {loss}")
        step.set_labels()
        out = []
        for flat, w in zip(self._flatten(), self.treeWeights):
            es, ws = step.update(flat, float(w), loss)
            out.append(es / ws)
        return out

    def evaluateEachIteration(self, X, y, weights=None, loss=None):
        T.check_rows(X, self.numFeatures)
        return self.evaluate_step(
            GBTDeviceStep(X, y, weights, self.classifier, residuals=False), loss)


class GBTRegressionModel(_GBTModel):
    def __init__(self, trees, treeWeights, numFeatures: int, lossType: str = "squared"):
        super().__init__(trees, treeWeights, numFeatures, lossType)


class GBTClassificationModel(_GBTModel):
    classifier = True

    def __init__(self, trees, treeWeights, numFeatures: int, lossType: str = "logistic"):
        super().__init__(trees, treeWeights, numFeatures, lossType)
        self.numClasses = 2         # the trees are regression trees (checked above as such)

    def margin(self, X):
        return self._run(X, margin=True)[1]

    def predictRaw(self, X):
        return self._run(X, raw=True)[2]

    def predictProbability(self, X):
        return self._run(X, prob=True)[3]


# ------------------------------------------------------------------ estimators
class _GBTEstimator:
    classifier = False
    losses = ()
    model = None

    def __init__(self, maxIter, stepSize, lossType, maxDepth, maxBins, minInstancesPerNode,
                 minWeightFractionPerNode, minInfoGain, subsamplingRate, featureSubsetStrategy,
                 validationTol, seed, workspaceBytes, categoricalFeaturesInfo):
        T.check_params(maxDepth, maxBins, minInstancesPerNode, minWeightFractionPerNode,
                       minInfoGain, "variance", False, categoricalFeaturesInfo)
        RF.check_forest_params(1, subsamplingRate)
        check_gbt_params(maxIter, stepSize, lossType, self.losses, validationTol)
        # the strategy's own refusals do not wait for the rows (d = 1 names every form)
        RF.num_features_per_node(featureSubsetStrategy, 1, 1, False)
        self.maxIter, self.stepSize, self.lossType = int(maxIter), float(stepSize), lossType
        self.maxDepth, self.maxBins = int(maxDepth), int(maxBins)
        self.minInstancesPerNode = int(minInstancesPerNode)
        self.minWeightFractionPerNode = float(minWeightFractionPerNode)
        self.minInfoGain, self.subsamplingRate = float(minInfoGain), float(subsamplingRate)
        self.featureSubsetStrategy = str(featureSubsetStrategy)
        self.validationTol, self.seed = float(validationTol), int(seed)
        self.workspaceBytes = int(workspaceBytes)

    def fit_step(self, step, d: int, validation=None, nodesPerCall=None):
        """The fit over any step object (GBTDeviceStep, GBTNumpyStep);
        validation: a step of the same kind over the validation rows."""
        roots, weights, _ = boost(
            step, d, self.lossType, self.maxIter, self.stepSize, self.maxDepth, self.maxBins,
            self.minInstancesPerNode, self.minWeightFractionPerNode, self.minInfoGain,
            self.subsamplingRate, self.featureSubsetStrategy, self.validationTol, self.seed,
            validation, nodesPerCall)
        return self.model([DecisionTreeRegressionModel(r, d) for r in roots], weights, d,
                          self.lossType)

    def fit(self, X, y, weights=None, validation=None):
        T.check_rows(X)
        d = int(X.shape[1])
        step = GBTDeviceStep(X, y, weights, self.classifier, self.workspaceBytes)
        vstep = None
        if validation is not None:
            Xv, yv, wv = validation
            T.check_rows(Xv, d, "training rows")
            vstep = GBTDeviceStep(Xv, yv, wv, self.classifier, self.workspaceBytes,
                                  residuals=False)
        return self.fit_step(step, d, vstep)


class GBTRegressor(_GBTEstimator):
    """ml/regression/GBTRegressor.scala's estimator over dense fp64 device
    rows; with several ranks every rank calls fit on its shard."""

    losses = ("squared", "absolute")
    model = GBTRegressionModel

    def __init__(self, maxIter: int = 20, stepSize: float = 0.1, lossType: str = "squared",
                 maxDepth: int = 5, maxBins: int = 32, minInstancesPerNode: int = 1,
                 minWeightFractionPerNode: float = 0.0, minInfoGain: float = 0.0,
                 subsamplingRate: float = 1.0, featureSubsetStrategy: str = "all",
                 validationTol: float = 0.01, seed: int = REGRESSOR_SEED, workspaceBytes: int = 0,
                 categoricalFeaturesInfo=None):
        super().__init__(maxIter, stepSize, lossType, maxDepth, maxBins, minInstancesPerNode,
                         minWeightFractionPerNode, minInfoGain, subsamplingRate,
                         featureSubsetStrategy, validationTol, seed, workspaceBytes,
                         categoricalFeaturesInfo)


class GBTClassifier(_GBTEstimator):
    """ml/classification/GBTClassifier.scala's estimator (binary labels 0 / 1)
    over dense fp64 device rows; with several ranks every rank calls fit on its
    shard."""

    classifier = True
    losses = ("logistic",)
    model = GBTClassificationModel

    def __init__(self, maxIter: int = 20, stepSize: float = 0.1, lossType: str = "logistic",
                 maxDepth: int = 5, maxBins: int = 32, minInstancesPerNode: int = 1,
                 minWeightFractionPerNode: float = 0.0, minInfoGain: float = 0.0,
                 subsamplingRate: float = 1.0, featureSubsetStrategy: str = "all",
                 validationTol: float = 0.01, seed: int = CLASSIFIER_SEED, workspaceBytes: int = 0,
                 categoricalFeaturesInfo=None):
        super().__init__(maxIter, stepSize, lossType, maxDepth, maxBins, minInstancesPerNode,
                         minWeightFractionPerNode, minInfoGain, subsamplingRate,
                         featureSubsetStrategy, validationTol, seed, workspaceBytes,
                         categoricalFeaturesInfo)
