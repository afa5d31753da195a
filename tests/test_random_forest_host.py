"""RandomForest's host side (cycloneml_amd/forest.py) without a device: the
numFeaturesPerNode table, the bag generator and the feature subsets against the
pure-Python restatement of tests/random_forest_restatement.py, the identity of a
one-tree forest with DecisionTree*, a small forest over ForestNumpyStep against
the restatement's tree-by-tree fit, and the independence of a forest from the
nodes-per-call cap.
"""
import math

import numpy as np
import pytest

import decision_tree_restatement as R
import random_forest_restatement as F
from cycloneml_amd import _native as N
from cycloneml_amd import forest as RF
from cycloneml_amd.forest import (ForestNumpyStep, RandomForestClassificationModel,
                                  RandomForestClassifier, RandomForestRegressionModel,
                                  RandomForestRegressor)
from cycloneml_amd.tree import DecisionTreeClassifier, DecisionTreeRegressor, NumpyStep


# ------------------------------------------------------------ numFeaturesPerNode
def test_num_features_per_node_table():
    f = RF.num_features_per_node
    assert f("auto", 1, 100, True) == 100 and f("auto", 1, 100, False) == 100
    assert f("auto", 20, 100, True) == 10 and f("auto", 20, 100, False) == 34
    assert f("auto", 20, 101, True) == 11                   # ceil(sqrt(101))
    assert f("all", 20, 7, True) == 7
    assert f("sqrt", 1, 17, False) == 5
    assert f("log2", 3, 1, True) == 1 and f("log2", 3, 8, True) == 3 and f("log2", 3, 9, True) == 4
    assert f("onethird", 3, 10, True) == 4 and f("onethird", 3, 9, True) == 3
    assert f("1", 3, 10, True) == 1 and f("1.0", 3, 10, True) == 10
    assert f("7", 3, 10, True) == 7 and f("25", 3, 10, True) == 10
    assert f("0.25", 3, 10, True) == 3 and f("0.5", 3, 7, False) == 4
    assert f("SQRT", 3, 16, False) == 4
    for d1 in ("auto", "all", "sqrt", "log2", "onethird", "1", "3", "0.1", "1.0"):
        assert f(d1, 5, 1, True) == 1 and f(d1, 5, 1, False) == 1
    for bad in ("0", "-3", "0.0", "1.5", "-0.5", "half", "", "nan", "1e400", "2.0"):
        with pytest.raises(N.IllegalArgumentException):
            f(bad, 3, 10, True)


def test_estimator_refusals():
    for kw in (dict(numTrees=0), dict(numTrees=RF.MAX_TREES + 1), dict(subsamplingRate=0.0),
               dict(subsamplingRate=1.5), dict(subsamplingRate=-0.1),
               dict(featureSubsetStrategy="most"), dict(categoricalFeaturesInfo={0: 3}),
               dict(maxDepth=31), dict(impurity="variance")):
        with pytest.raises(N.IllegalArgumentException):
            RandomForestClassifier(**kw)
    with pytest.raises(N.IllegalArgumentException):
        RandomForestRegressor(impurity="gini")
    with pytest.raises(N.IllegalArgumentException):
        RandomForestRegressor(categoricalFeaturesInfo={1: 2})
    est = RandomForestClassifier()
    assert (est.numTrees, est.featureSubsetStrategy, est.subsamplingRate, est.bootstrap) == \
        (20, "auto", 1.0, True)
    assert est.numFeaturesPerNode(100) == 10 and RandomForestRegressor().numFeaturesPerNode(100) == 34


# ------------------------------------------------------------------------- bag
def test_mix_equals_restatement():
    rng = np.random.default_rng(0)
    idx = np.concatenate([np.arange(5), rng.integers(0, 2 ** 62, size=40)]).astype(np.uint64)
    for seed in (0, 1, -7, 2 ** 63 + 5):
        for stream in (0, 1):
            for tree in (0, 3, 4095):
                got = RF.mix(seed, stream, tree, idx)
                ref = [F.mix(seed % 2 ** 64, stream, tree, int(i)) for i in idx]
                assert got.dtype == np.uint64 and got.tolist() == ref


@pytest.mark.parametrize("rate", [1.0, 0.3, 0.01])
def test_poisson_table(rate):
    t = RF.poisson_table(rate)
    assert t.dtype == np.uint64 and t.tolist() == F.poisson_table(rate)
    assert np.all(t[1:] >= t[:-1]) and int(t[-1]) == 2 ** 53 and len(t) <= 255
    assert int(t[0]) == math.floor(math.exp(-rate) * 2 ** 53)
    assert int(t[1]) == math.floor((math.exp(-rate) + math.exp(-rate) * rate / 1) * 2 ** 53)


@pytest.mark.parametrize("rate", [1.0, 0.3])
def test_bag_bytes_and_mean(rate):
    table = RF.poisson_table(rate)
    small = RF.bag_counts(5, 3, 300, table, rowOffset=11)
    assert small.dtype == np.uint8 and small.shape == (3, 300)
    assert small.tobytes() == np.array(F.bag(5, 3, 300, table.tolist(), 11), dtype=np.uint8).tobytes()
    n, nt = 2 ** 14, 16                                     # n T = 2^18 draws
    big = RF.bag_counts(1, nt, n, table)
    # Poisson: mean = variance = rate, so the mean of N draws has deviation sqrt(rate / N)
    assert abs(float(big.mean()) - rate) <= 6.0 * math.sqrt(rate / (n * nt))
    assert RF.bag_counts(2, nt, n, table).tobytes() != big.tobytes()
    assert big[0].tobytes() != big[1].tobytes()


def test_bernoulli_bag():
    table = RF.bag_table(False, 0.3)
    assert table.tolist() == F.bernoulli_table(0.3) and len(table) == 1
    bag = RF.bag_counts(3, 4, 2 ** 14, table)
    assert set(np.unique(bag).tolist()) == {0, 1}
    assert bag.tobytes() == np.array(F.bag(3, 4, 2 ** 14, table.tolist()), dtype=np.uint8).tobytes()
    # Bernoulli: variance rate (1 - rate)
    assert abs(float(bag.mean()) - 0.3) <= 6.0 * math.sqrt(0.3 * 0.7 / bag.size)
    assert RF.bag_table(False, 1.0) is None
    assert RF.bag_table(True, 1.0).tolist() == F.poisson_table(1.0)


def test_bag_shards_concatenate():
    table = RF.poisson_table(0.7)
    whole = RF.bag_counts(9, 3, 1000, table)
    parts = [RF.bag_counts(9, 3, b - a, table, rowOffset=a) for a, b in ((0, 1), (1, 400), (400, 1000))]
    assert np.concatenate(parts, axis=1).tobytes() == whole.tobytes()


# ------------------------------------------------------------- feature subsets
def test_feature_subsets():
    d, m = 70, 9
    seen = {}
    for t in (0, 1, 7):
        for i in (1, 2, 3, 2 ** 30 + 5):
            s = RF.feature_subset(4, t, i, d, m)
            assert s.dtype == np.int32 and s.tolist() == F.feature_subset(4, t, i, d, m)
            assert len(set(s.tolist())) == m and np.all(s[1:] > s[:-1])
            assert 0 <= s[0] and s[-1] < d
            seen[(t, i)] = s.tolist()
    # any call order, the same subset
    for key in reversed(sorted(seen)):
        assert RF.feature_subset(4, *key, d, m).tolist() == seen[key]
    assert len({tuple(v) for v in seen.values()}) == len(seen)
    assert RF.feature_subset(5, 0, 1, d, m).tolist() != seen[(0, 1)]
    assert RF.feature_subset(4, 0, 1, d, d).tolist() == list(range(d))
    for mm in (1, 2, 69):
        assert RF.feature_subset(4, 2, 9, d, mm).tolist() == F.feature_subset(4, 2, 9, d, mm)
    # every feature is drawn by some node, the first and the last included
    drawn = set()
    for i in range(1, 200):
        drawn |= set(RF.feature_subset(0, 0, i, d, 3).tolist())
    assert drawn == set(range(d))
    assert RF.feature_subset(0, 0, 1, 1, 1).tolist() == [0]


# ---------------------------------------------------- identity with the one tree
same_node = F.same_node


@pytest.mark.parametrize("impurity,weighted", [("gini", True), ("entropy", False),
                                               ("variance", True)])
def test_one_tree_forest_is_the_decision_tree(impurity, weighted):
    X, ycls, yreg, w = R.exact_rows(700, 9, seed=4)
    rng = np.random.default_rng(1)
    X = X + rng.normal(size=X.shape) * 0.01          # real rows: the sums' order matters
    w = (w * rng.uniform(0.5, 1.5, size=w.size)) if weighted else None
    kw = dict(maxDepth=5, impurity=impurity, minInstancesPerNode=3)
    fkw = dict(numTrees=1, featureSubsetStrategy="all", bootstrap=False, subsamplingRate=1.0, **kw)
    if impurity == "variance":
        tree = DecisionTreeRegressor(**kw).fit_step(NumpyStep(X, yreg, w, 0), 9)
        forest = RandomForestRegressor(**fkw).fit_step(ForestNumpyStep(X, yreg, w, 0), 9)
    else:
        tree = DecisionTreeClassifier(numClasses=3, **kw).fit_step(NumpyStep(X, ycls, w, 3), 9, 3)
        forest = RandomForestClassifier(numClasses=3, **fkw).fit_step(
            ForestNumpyStep(X, ycls, w, 3), 9, 3)
    assert forest.getNumTrees == 1 and tree.numNodes >= 9
    assert forest.trees[0].toDebugString() == tree.toDebugString()
    assert same_node(forest.trees[0].rootNode, tree.rootNode)
    # the forest normalises the tree's normalised vector once more
    one = tree.featureImportances
    assert forest.featureImportances.tobytes() == (one / float(np.cumsum(one)[-1])).tobytes()
    assert forest.totalNumNodes == tree.numNodes
    # "auto" with one tree is "all" too
    auto = dict(fkw, featureSubsetStrategy="auto")
    est = RandomForestRegressor(**auto) if impurity == "variance" else \
        RandomForestClassifier(numClasses=3, **auto)
    assert est.numFeaturesPerNode(9) == 9


# ------------------------------------------------ a small forest, by the restatement
@pytest.fixture(scope="module")
def tiny():
    X, ycls, yreg, w = R.exact_rows(60, 6, seed=12)
    return X, ycls, yreg, w


CASES = [("gini", dict(bootstrap=True, subsamplingRate=1.0, featureSubsetStrategy="sqrt")),
         ("entropy", dict(bootstrap=False, subsamplingRate=0.6, featureSubsetStrategy="2")),
         ("gini", dict(bootstrap=False, subsamplingRate=1.0, featureSubsetStrategy="log2",
                       minInstancesPerNode=4)),
         ("variance", dict(bootstrap=True, subsamplingRate=0.8, featureSubsetStrategy="onethird")),
         ("variance", dict(bootstrap=True, subsamplingRate=1.0, featureSubsetStrategy="all",
                           minWeightFractionPerNode=0.05))]


@pytest.mark.parametrize("impurity,kw", CASES)
def test_three_tree_forest_equals_restatement(tiny, impurity, kw):
    X, ycls, yreg, w = tiny
    d, C = 6, (0 if impurity == "variance" else 3)
    y = yreg if impurity == "variance" else ycls
    kw = dict(kw, numTrees=3, maxDepth=4, impurity=impurity, seed=3)
    if C:
        est = RandomForestClassifier(numClasses=3, **kw)
        model = est.fit_step(ForestNumpyStep(X, y, w, C), d, C)
    else:
        est = RandomForestRegressor(**kw)
        model = est.fit_step(ForestNumpyStep(X, y, w, 0), d)
    m = est.numFeaturesPerNode(d)
    roots, _, counts = F.fit_forest(
        X.tolist(), y, w, C, impurity, 3, m, maxDepth=4,
        minInstancesPerNode=kw.get("minInstancesPerNode", 1),
        minWeightFractionPerNode=kw.get("minWeightFractionPerNode", 0.0),
        bootstrap=kw["bootstrap"], subsamplingRate=kw["subsamplingRate"], seed=3)
    assert model.getNumTrees == 3 and len(model.trees) == 3
    assert model.treeWeights.tolist() == [1.0, 1.0, 1.0] and model.numFeatures == d
    assert sum(t.numNodes for t in model.trees) == model.totalNumNodes > 3
    for t, root in zip(model.trees, roots):
        assert R.same_tree(t.rootNode, root)
    assert len({t.toDebugString() for t in model.trees}) > 1
    assert model.featureImportances.tobytes() == \
        np.array(F.importances(roots, d, C), dtype=np.float64).tobytes()
    assert abs(float(model.featureImportances.sum()) - 1.0) < 1e-12
    text = model.toDebugString()
    assert text.startswith(type(model).__name__ + ": numTrees=3")
    assert text.count("Tree ") == 3 and "  Tree 2 (weight 1.0):" in text
    # votes, mean and argmax on the host: the uploaded leaf values added in tree order
    nodeStart, leafStart, ft, th, fc, li, lv = model._flatten()
    for r in range(0, 60, 7):
        acc = np.zeros(max(C, 1))
        for t in range(3):
            _, leaf = R.descend(model.trees[t].rootNode, X[r])
            acc = acc + lv[leafStart[t] + leaf]
        if C:
            raw, prob, pred = F.votes(roots, X[r], C)
            assert acc.tobytes() == np.array(raw).tobytes()
            assert float(np.argmax(acc)) == pred
            s = float(np.cumsum(acc)[-1])
            assert (acc / s).tobytes() == np.array(prob).tobytes()
        else:
            assert np.float64(acc[0] / 3).tobytes() == np.float64(F.mean(roots, X[r])).tobytes()


def test_from_trees_on_the_host(tiny):
    X, ycls, yreg, w = tiny
    est = RandomForestClassifier(numTrees=2, maxDepth=2, numClasses=3, seed=1)
    model = est.fit_step(ForestNumpyStep(X, ycls, w, 3), 6, 3)
    again = RandomForestClassificationModel.from_trees(model.trees, 6, 3)
    assert again._plan is None and again.getNumTrees == 2
    assert again.toDebugString() == model.toDebugString()
    reg = RandomForestRegressor(numTrees=2, maxDepth=2, seed=1).fit_step(
        ForestNumpyStep(X, yreg, w, 0), 6)
    assert RandomForestRegressionModel.from_trees(reg.trees, 6)._plan is None
    for bad in ((reg.trees, 6, 3), ([], 6, 3), (model.trees, 5, 3), (model.trees, 6, 2)):
        with pytest.raises(N.IllegalArgumentException):
            RandomForestClassificationModel.from_trees(*bad)


# ------------------------------------------------------------ the nodes-per-call cap
@pytest.mark.parametrize("impurity", ["gini", "variance"])
def test_forest_does_not_depend_on_the_call_cap(impurity):
    X, ycls, yreg, w = R.exact_rows(400, 12, seed=6)
    rng = np.random.default_rng(2)
    w = w * rng.uniform(0.5, 1.5, size=w.size)              # real weights: order would show
    C = 0 if impurity == "variance" else 3
    y = yreg if impurity == "variance" else ycls
    kw = dict(numTrees=4, maxDepth=4, impurity=impurity, seed=8)
    est = RandomForestClassifier(numClasses=3, **kw) if C else RandomForestRegressor(**kw)
    args = (12, C) if C else (12,)
    ref = est.fit_step(ForestNumpyStep(X, y, w, C), *args)
    assert ref.totalNumNodes > 20
    for cap in (1, 3):
        got = est.fit_step(ForestNumpyStep(X, y, w, C), *args, nodesPerCall=cap)
        for a, b in zip(got.trees, ref.trees):
            assert same_node(a.rootNode, b.rootNode)
        assert got.featureImportances.tobytes() == ref.featureImportances.tobytes()
    # shards by rowOffset draw the bag of the whole: the step of the second half
    step = ForestNumpyStep(X[200:], y[200:], w[200:], C, rowOffset=200)
    step.bag(4, RF.poisson_table(1.0), 8)
    whole = ForestNumpyStep(X, y, w, C)
    whole.bag(4, RF.poisson_table(1.0), 8)
    assert step.bagCounts.tobytes() == whole.bagCounts[:, 200:].tobytes()
