"""GBT's host side (cycloneml_amd/gbt.py) without a device: the known answers
of pyspark's GBTClassifier / GBTRegressor doctests (derivable by hand), the
importances' rule, the GBTNumpyStep fit against the tree-by-tree restatement of
tests/gbt_restatement.py, validation stopping and the refusals.  A model's
margins are formed here by the restatement from the model's trees and weights;
the models' own predict runs on the device (tests/test_gbt_gpu.py).
"""
import math

import numpy as np
import pytest

import decision_tree_restatement as R
import gbt_restatement as G
from cycloneml_amd import _native as N
from cycloneml_amd import forest as RF
from cycloneml_amd import gbt as GB
from cycloneml_amd.ann import java_string_hash
from cycloneml_amd.gbt import (GBTClassificationModel, GBTClassifier, GBTNumpyStep,
                               GBTRegressionModel, GBTRegressor)
from cycloneml_amd.tree import DecisionTreeRegressionModel, Node

X2 = np.array([[1.0], [0.0]])
Y2 = np.array([1.0, 0.0])


def roots_of(model):
    return [t.rootNode for t in model.trees]


def margins_by_hand(iters):
    F = [1.0]
    for _ in range(iters - 1):
        F.append(F[-1] + 0.1 * 4.0 / (1.0 + math.exp(2.0 * F[-1])))
    return F


# ---------------------------------------------------------------- known answers
def test_classifier_doctest():
    est = GBTClassifier(maxIter=5, maxDepth=2, stepSize=0.1, seed=42)
    model = est.fit_step(GBTNumpyStep(X2, Y2, None, classifier=True), 1)
    assert isinstance(model, GBTClassificationModel) and model.numClasses == 2
    assert model.getNumTrees == 5 and model.numFeatures == 1
    assert [t.numNodes for t in model.trees] == [3] * 5 and model.totalNumNodes == 15
    assert model.treeWeights.tolist() == [1.0, 0.1, 0.1, 0.1, 0.1]
    assert model.featureImportances.tolist() == [1.0]
    F = margins_by_hand(5)
    roots, tw = roots_of(model), model.treeWeights
    for m in range(1, 6):
        up = G.margin(roots[:m], tw[:m], [1.0])
        down = G.margin(roots[:m], tw[:m], [0.0])
        assert abs(up - F[m - 1]) <= 1e-12 and abs(down + F[m - 1]) <= 1e-12, m
    raw, prob, pred = G.classify(G.margin(roots, tw, [0.0]))
    assert [round(v, 4) for v in raw] == [1.1697, -1.1697]
    assert [round(v, 4) for v in prob] == [0.9121, 0.0879]
    assert pred == 0.0 and G.classify(G.margin(roots, tw, [1.0]))[2] == 1.0
    # evaluateEachIteration on the single row x = -1, label 0
    errs = model.evaluate_step(GBTNumpyStep(np.array([[-1.0]]), np.array([0.0]), None,
                                            classifier=True, residuals=False))
    want = [2.0 * math.log1p(math.exp(-2.0 * f)) for f in F]
    assert np.allclose(errs, want, rtol=1e-12, atol=0.0)
    assert [round(v, 4) for v in errs[:2]] == [0.2539, 0.2321]
    assert all(a > b for a, b in zip(errs, errs[1:]))
    assert errs == G.evaluate_each_iteration(roots, tw, [[-1.0]], [0.0], None, "logistic", True)
    assert "GBTClassificationModel: numTrees=5, numClasses=2, numFeatures=1" in model.toDebugString()
    assert "Tree 1 (weight 0.1):" in model.toDebugString()


def test_regressor_doctest():
    est = GBTRegressor(maxIter=5, maxDepth=2, seed=42)
    model = est.fit_step(GBTNumpyStep(X2, Y2), 1)
    assert isinstance(model, GBTRegressionModel) and model.numClasses == 0
    assert [t.numNodes for t in model.trees] == [3, 1, 1, 1, 1]
    assert model.treeWeights.tolist() == [1.0, 0.1, 0.1, 0.1, 0.1]
    assert model.trees[0].rootNode.left.prediction == 0.0
    assert model.trees[0].rootNode.right.prediction == 1.0
    assert all(t.rootNode.prediction == 0.0 for t in model.trees[1:])
    assert model.featureImportances.tolist() == [1.0]
    assert G.margin(roots_of(model), model.treeWeights, [1.0]) == 1.0
    assert G.margin(roots_of(model), model.treeWeights, [0.0]) == 0.0
    assert model.evaluate_step(GBTNumpyStep(X2, Y2, residuals=False)) == [0.0] * 5
    assert model.evaluate_step(GBTNumpyStep(X2, Y2, residuals=False), "absolute") == [0.0] * 5


def stump(feature, gain, count):
    root = Node([count, 0.0, 0.0, count], 1.0, 0)
    root.gain, root.split = gain, (feature, 0.5)
    root.left = Node([count / 2, -count / 2, count / 2, count / 2], 0.0, 0)
    root.right = Node([count / 2, count / 2, count / 2, count / 2], 0.0, 0)
    return root


def test_importances_are_not_normalised_per_tree():
    trees = [DecisionTreeRegressionModel(stump(0, 1.0, 10.0), 2),
             DecisionTreeRegressionModel(stump(1, 1.0, 30.0), 2)]
    model = GBTRegressionModel.from_trees(trees, [1.0, 0.1], 2)
    assert model.featureImportances.tolist() == [0.25, 0.75]        # per tree: [0.5, 0.5]
    assert G.importances(roots_of(model), 2) == [0.25, 0.75]
    forest = RF.RandomForestRegressionModel(trees, 2)
    assert forest.featureImportances.tolist() == [0.5, 0.5]
    assert model.getNumTrees == 2 and model.totalNumNodes == 6 and model._plan is None
    with pytest.raises(N.IllegalArgumentException):
        GBTRegressionModel.from_trees(trees, [1.0], 2)


def test_default_seeds_and_params():
    assert GBTClassifier().seed == java_string_hash("org.apache.spark.ml.classification.GBTClassifier")
    assert GBTRegressor().seed == java_string_hash("org.apache.spark.ml.regression.GBTRegressor")
    est = GBTRegressor()
    assert (est.maxIter, est.stepSize, est.lossType, est.maxDepth, est.maxBins) == \
        (20, 0.1, "squared", 5, 32)
    assert (est.subsamplingRate, est.featureSubsetStrategy, est.validationTol) == (1.0, "all", 0.01)
    assert GBTClassifier().lossType == "logistic"


# -------------------------------------------------------------------- the losses
def test_losses_equal_restatement():
    rng = np.random.default_rng(3)
    pred = np.concatenate([rng.normal(size=40) * 3.0, [0.0, -0.0, 400.0, -400.0, 1.0]])
    for loss in ("squared", "absolute", "logistic"):
        y = rng.choice([-1.0, 1.0], size=pred.size) if loss == "logistic" else \
            np.concatenate([rng.normal(size=40), pred[40:]])
        resid, e = GB.neg_gradient_and_error(loss, pred, y)
        for i in range(pred.size):
            assert resid[i] == -G.gradient(loss, float(pred[i]), float(y[i])), (loss, i)
            assert e[i] == G.error(loss, float(pred[i]), float(y[i])), (loss, i)
    assert G.log1p_exp(800.0) == 800.0 and G.log1p_exp(-800.0) == 0.0
    assert GB.log1p_exp(0.5) == G.log1p_exp(0.5)


# ------------------------------------------------------ agreement with the restatement
def rows(n, d, seed, classifier):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, d))
    X[:, 0] = np.round(X[:, 0], 1)                      # ties among the values
    f = X[:, 0] + np.sin(2.0 * X[:, min(1, d - 1)]) - 0.5 * (X[:, d - 1] > 0.3)
    y = (f + 0.3 * rng.normal(size=n) > 0).astype(np.float64) if classifier else \
        f + 0.3 * rng.normal(size=n)
    w = rng.uniform(0.25, 4.0, size=n)
    return X, y, w


def same_fit(model, roots, weights):
    assert model.getNumTrees == len(roots) and model.treeWeights.tolist() == list(weights)
    for t, (a, b) in enumerate(zip(roots_of(model), roots)):
        assert R.same_tree(a, b), f"tree {t} differs from the restatement"
        assert np.array(G.leaf_values(a)).tobytes() == np.array(G.leaf_values(b)).tobytes()


CASES = [
    ("squared", False, dict(n=300, d=6, maxIter=4, maxDepth=3, stepSize=0.1)),
    ("absolute", False, dict(n=200, d=4, maxIter=3, maxDepth=3, stepSize=0.5)),
    ("logistic", True, dict(n=250, d=5, maxIter=4, maxDepth=2, stepSize=0.3)),
]


@pytest.mark.parametrize("loss,classifier,kw", CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize("variant", ["plain", "weights", "subsample", "sqrt"])
def test_numpy_step_fit_equals_restatement(loss, classifier, kw, variant):
    n, d = kw["n"], kw["d"]
    X, y, w = rows(n, d, 11, classifier)
    w = w if variant != "plain" else None
    rate = 0.5 if variant == "subsample" else 1.0
    strategy = "sqrt" if variant == "sqrt" else "all"
    m = RF.num_features_per_node(strategy, 1, d, False)
    Est = GBTClassifier if classifier else GBTRegressor
    est = Est(maxIter=kw["maxIter"], stepSize=kw["stepSize"], lossType=loss,
              maxDepth=kw["maxDepth"], subsamplingRate=rate, featureSubsetStrategy=strategy,
              seed=5)
    step = GBTNumpyStep(X, y, w, classifier=classifier)
    model = est.fit_step(step, d)
    roots, weights, thresholds, targets = G.fit_gbt(
        X.tolist(), y.tolist(), None if w is None else w.tolist(), loss, classifier,
        kw["maxIter"], kw["stepSize"], m, kw["maxDepth"], subsamplingRate=rate, seed=5)
    same_fit(model, roots, weights)
    assert model.getNumTrees == kw["maxIter"]
    # the step's last residual and prediction are the restatement's
    pred = [G.margin(roots, weights, x) for x in X.tolist()]
    assert step.pred.tolist() == pred
    labels = 2.0 * y - 1.0 if classifier else y
    assert step.residual().tolist() == [-G.gradient(loss, p, float(v)) for p, v in zip(pred, labels)]
    assert np.array(model.featureImportances).tolist() == G.importances(roots, d)
    errs = model.evaluate_step(GBTNumpyStep(X, y, w, classifier=classifier, residuals=False))
    assert errs == G.evaluate_each_iteration(roots, weights, X.tolist(), y.tolist(),
                                             None if w is None else w.tolist(), loss, classifier)


def test_binned_walk_uses_the_threshold_position():
    X, y, _ = rows(120, 3, 2, False)
    roots, _, thresholds, _ = G.fit_gbt(X.tolist(), y.tolist(), None, "squared", False, 1, 0.1, 3,
                                        maxDepth=4)
    step = GBTNumpyStep(X, y)
    est = GBTRegressor(maxIter=1, maxDepth=4, seed=0)
    model = est.fit_step(step, 3)
    flat = GB.flat_tree(model.trees[0].rootNode, thresholds)
    inner = np.nonzero(flat.firstChild >= 0)[0]
    assert inner.size and all(
        thresholds[flat.feature[i]][flat.splitBin[i]] == flat.threshold[i] for i in inner)
    assert np.all(flat.splitBin[flat.firstChild < 0] == -1)
    for r in range(120):
        binned = G.leaf_of_binned(roots[0], thresholds, step.image[r]).prediction
        assert binned == G.leaf_of(roots[0], X[r]).prediction
        assert G.flat_walk(flat.feature, flat.splitBin, flat.firstChild, flat.value,
                           step.image[r].astype(int))[0] == binned
    with pytest.raises(N.IllegalArgumentException, match="none of its feature's split candidates"):
        GB.flat_tree(model.trees[0].rootNode, [np.asarray(t) + 1e-3 for t in thresholds])


# ------------------------------------------------------------------- validation
def validation_rows():
    X, y, w = rows(260, 4, 21, False)
    return (X[:180], y[:180], w[:180]), (X[180:], y[180:], w[180:])


def test_validation_stops_at_iteration_two():
    (X, y, w), (Xv, yv, wv) = validation_rows()
    tol = 0.3
    kw = dict(maxIter=6, stepSize=0.5, maxDepth=2)
    roots, weights, _, targets = G.fit_gbt(
        X.tolist(), y.tolist(), w.tolist(), "squared", False, kw["maxIter"], kw["stepSize"], 4,
        kw["maxDepth"], seed=9, validation=(Xv.tolist(), yv.tolist(), wv.tolist()),
        validationTol=tol)
    # the case: trees 0, 1, 2 were grown, iteration 2 failed the rule, tree 1 was the best
    assert len(targets) == 3 and len(roots) == 2
    errs = G.evaluate_each_iteration(*G.fit_gbt(
        X.tolist(), y.tolist(), w.tolist(), "squared", False, 3, kw["stepSize"], 4,
        kw["maxDepth"], seed=9)[:2], Xv.tolist(), yv.tolist(), wv.tolist(), "squared", False)
    assert errs[0] - errs[1] >= tol * max(errs[1], 0.01)
    assert errs[1] - errs[2] < tol * max(errs[2], 0.01)
    est = GBTRegressor(validationTol=tol, seed=9, **kw)
    model = est.fit_step(GBTNumpyStep(X, y, w), 4,
                         validation=GBTNumpyStep(Xv, yv, wv, residuals=False))
    same_fit(model, roots, weights)
    assert model.getNumTrees == 2 and model.treeWeights.tolist() == [1.0, 0.5]
    # without validation every tree is kept
    assert est.fit_step(GBTNumpyStep(X, y, w), 4).getNumTrees == 6


def test_max_iter_one():
    (X, y, w), (Xv, yv, wv) = validation_rows()
    for validation in (None, GBTNumpyStep(Xv, yv, wv, residuals=False)):
        model = GBTRegressor(maxIter=1, maxDepth=3, seed=1).fit_step(
            GBTNumpyStep(X, y, w), 4, validation=validation)
        assert model.getNumTrees == 1 and model.treeWeights.tolist() == [1.0]
    yc = (y > 0).astype(np.float64)
    model = GBTClassifier(maxIter=1, maxDepth=3, seed=1).fit_step(
        GBTNumpyStep(X, yc, w, classifier=True), 4)
    assert model.getNumTrees == 1
    # tree 0 is fitted to 2 y - 1
    assert set(G.leaf_values(model.trees[0].rootNode)) <= {v for v in G.leaf_values(
        G.fit_gbt(X.tolist(), yc.tolist(), w.tolist(), "logistic", True, 1, 0.1, 4, 3, seed=1)[0][0])}


# --------------------------------------------------------------------- refusals
@pytest.mark.parametrize("kw,msg", [
    (dict(maxIter=0), "maxIter must be in"),
    (dict(maxIter=RF.MAX_TREES + 1), "maxIter must be in"),
    (dict(stepSize=0.0), r"stepSize must be in \(0, 1\]"),
    (dict(stepSize=1.5), r"stepSize must be in \(0, 1\]"),
    (dict(stepSize=-0.1), r"stepSize must be in \(0, 1\]"),
    (dict(lossType="huber"), "lossType given invalid value huber"),
    (dict(validationTol=-1e-3), "validationTol must not be negative"),
    (dict(maxDepth=31), "maxDepth"),
    (dict(maxBins=1), "maxBins"),
    (dict(minInstancesPerNode=0), "minInstancesPerNode"),
    (dict(minWeightFractionPerNode=0.5), "minWeightFractionPerNode"),
    (dict(minInfoGain=-1.0), "minInfoGain"),
    (dict(subsamplingRate=0.0), "subsamplingRate"),
    (dict(subsamplingRate=1.5), "subsamplingRate"),
    (dict(featureSubsetStrategy="most"), "Supported values"),
    (dict(categoricalFeaturesInfo={0: 3}), "categorical"),
])
def test_estimator_refusals(kw, msg):
    for Est in (GBTClassifier, GBTRegressor):
        with pytest.raises(N.IllegalArgumentException, match=msg):
            Est(**kw)


def test_loss_types_belong_to_their_estimator():
    with pytest.raises(N.IllegalArgumentException, match="Supported options: logistic"):
        GBTClassifier(lossType="squared")
    with pytest.raises(N.IllegalArgumentException, match="Supported options: squared, absolute"):
        GBTRegressor(lossType="logistic")
    GBTRegressor(lossType="absolute")


def test_row_refusals():
    X, y, w = rows(50, 3, 4, True)
    bad = y.copy()
    bad[17], bad[30] = 2.0, -1.0
    with pytest.raises(N.IllegalArgumentException, match=r"integers in \[0 to 1\]. Found 2.0. \(row 17\)"):
        GBTClassifier(maxIter=2).fit_step(GBTNumpyStep(X, bad, w, classifier=True), 3)
    half = y.copy()
    half[5] = 0.5
    with pytest.raises(N.IllegalArgumentException, match=r"\(row 5\)"):
        GBTClassifier(maxIter=2).fit_step(GBTNumpyStep(X, half, w, classifier=True), 3)
    # a regressor takes any finite label
    GBTRegressor(maxIter=2, maxDepth=1).fit_step(GBTNumpyStep(X, bad, w), 3)
    inf = y.copy()
    inf[9] = np.inf
    with pytest.raises(N.IllegalArgumentException, match=r"must be finite.*\(row 9\)"):
        GBTRegressor(maxIter=2).fit_step(GBTNumpyStep(X, inf, w), 3)
    Xn = X.copy()
    Xn[3, 1] = np.nan
    with pytest.raises(N.IllegalArgumentException, match=r"not NaN. \(row 3\)"):
        GBTRegressor(maxIter=2).fit_step(GBTNumpyStep(Xn, y, w), 3)
    wn = w.copy()
    wn[8] = -1.0
    with pytest.raises(N.IllegalArgumentException, match=r"illegal weight value.*\(row 8\)"):
        GBTClassifier(maxIter=2).fit_step(GBTNumpyStep(X, y, wn, classifier=True), 3)
    # the validation rows are checked as the training rows are
    with pytest.raises(N.IllegalArgumentException, match=r"\(row 17\)"):
        GBTClassifier(maxIter=2).fit_step(
            GBTNumpyStep(X, y, w, classifier=True), 3,
            validation=GBTNumpyStep(X, bad, w, classifier=True, residuals=False))
    with pytest.raises(N.IllegalArgumentException, match="size of input RDD > 0"):
        GBTRegressor(maxIter=2).fit_step(GBTNumpyStep(np.zeros((0, 3)), np.zeros(0)), 3)
