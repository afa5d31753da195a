"""GBT on the device (csrc/gbt.hip) against the row-by-row restatement of
tests/gbt_restatement.py.

  update   image form: pred by bytes for every loss; resid by bytes for squared
           and absolute and within 1e-10 relative for logistic (the project's
           stated fp64 tolerance for exp-bearing losses and gradients: the
           device's exp is not the host's); sums by bytes on exact rows (integer
           labels, dyadic pred, weights in eighths, squared loss: every partial
           sum is exact in any order), otherwise within 1e-10 of the sum of |w e|.
           fp64-row form: the bytes of the image form on the same rows and tree.
  predict  leaf, margin and the regressor's pred by bytes, prob within 1e-10,
           raw = (-margin, margin) by bytes.  A margin starts from +0.0, so a
           leaf of -0.0 gives the margin +0.0 (0.0 + -0.0), as in the reference;
           both zeros predict class 0.
  fit      GBTDeviceStep against GBTNumpyStep: by bytes on an exact design,
           structure and 1e-10 leaves on real rows whose restatement fit is
           stable under a 1e-9 relative perturbation of every residual.
Every device call runs twice and the two results are compared by tobytes().
"""
import numpy as np
import pytest
import torch

import decision_tree_restatement as R
import gbt_restatement as G
import random_forest_restatement as F
from cycloneml_amd import gbt as GB
from cycloneml_amd.gbt import (FlatTree, GBTClassificationModel, GBTClassifier, GBTDeviceStep,
                               GBTNumpyStep, GBTPlan, GBTRegressionModel, GBTRegressor)
from cycloneml_amd.tree import DecisionTreeRegressionModel

pytestmark = pytest.mark.gpu

LOSS_NAMES = ("squared", "absolute", "logistic")
LDS_NODES = 2048          # cyc_gbt_lds_nodes, asserted below


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def twice(fn):
    a, b = fn(), fn()
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes(), "two calls differ"
    return a


# ------------------------------------------------------------------- the trees
def bfs_tree(numInternal, d, B, rng, pad=0):
    """A tree filled breadth first: the first numInternal nodes split, 2
    numInternal + 1 nodes, then `pad` leaves that no node points to."""
    m = 2 * numInternal + 1
    first = np.full(m + pad, -1, dtype=np.int32)
    first[:numInternal] = 1 + 2 * np.arange(numInternal)
    feature = np.where(first >= 0, rng.integers(0, d, size=m + pad), -1).astype(np.int32)
    split = np.where(first >= 0, rng.integers(0, max(B - 1, 1), size=m + pad), -1).astype(np.int32)
    return feature, split, first


def chain_tree(depth, d, B, rng):
    """Every right child splits again: 2 depth + 1 nodes, depth `depth`."""
    m = 2 * depth + 1
    first = np.full(m, -1, dtype=np.int32)
    first[0:2 * depth:2] = 1 + np.arange(0, 2 * depth, 2)
    feature = np.where(first >= 0, rng.integers(0, d, size=m), -1).astype(np.int32)
    # low bins: most rows go right, to the end of the chain
    split = np.where(first >= 0, rng.integers(0, max(min(B - 1, 2), 1), size=m), -1).astype(np.int32)
    return feature, split, first


SHAPES = {
    "leaf": lambda d, B, rng: bfs_tree(0, d, B, rng),
    "depth1": lambda d, B, rng: bfs_tree(1, d, B, rng),
    "depth5": lambda d, B, rng: bfs_tree(31, d, B, rng),
    "chain30": lambda d, B, rng: chain_tree(30, d, B, rng),
    "lds": lambda d, B, rng: bfs_tree((LDS_NODES - 1) // 2, d, B, rng, pad=1),      # 2048 nodes
    "lds+1": lambda d, B, rng: bfs_tree(LDS_NODES // 2, d, B, rng),                 # 2049 nodes
}


def values(first, rng, exact):
    v = rng.integers(-16, 17, size=first.size) / 8.0 if exact else rng.normal(size=first.size)
    return np.where(first < 0, v, 1e300)          # an internal node's value is never read


def reference(rows, feature, split, first, value, weight, loss, pred0, y, w):
    tree = [np.asarray(a).tolist() for a in (feature, split, first, value)]
    leaves = [G.flat_walk(*tree, row)[0] for row in np.asarray(rows).tolist()]
    pred, resid, errs, es, ws = G.update(leaves, weight, loss, pred0, y, w)
    absum = sum(abs(e * (1.0 if w is None else w[r])) for r, e in enumerate(errs))
    return np.array(pred), np.array(resid), es, ws, absum


def check_update(got, ref, loss, exact, what):
    pred, resid, sums = got
    rpred, rresid, es, ws, absum = ref
    assert pred.tobytes() == rpred.tobytes(), ("pred", what)
    if loss == "logistic":
        assert np.all(np.abs(resid - rresid) <= 1e-10 * np.abs(rresid)), ("resid", what)
    else:
        assert resid.tobytes() == rresid.tobytes(), ("resid", what)
    if exact:
        assert sums.tobytes() == np.array([es, ws]).tobytes(), ("sums", what)
    else:
        assert abs(sums[0] - es) <= 1e-10 * absum and abs(sums[1] - ws) <= 1e-10 * ws, \
            ("sums", what, sums, es, ws)


def run_update(plan, rows, flat, weight, loss, y, w, pred0, resid=True):
    def call():
        pred = dev(pred0)
        res = torch.full_like(pred, np.nan) if resid else None
        sums = plan.update(rows, flat, weight, loss, y, w, pred, res)
        return (pred.cpu().numpy(), res.cpu().numpy() if resid else np.zeros(0),
                sums.cpu().numpy())
    return twice(call)


SIZES = [(1, 1, True), (255, 3, False), (256, 64, True), (257, 257, False), (4097, 3, True),
         (4097, 257, False), (4097, 64, True), (257, 1, True)]


@pytest.mark.parametrize("shape", list(SHAPES))
def test_update_image(cuda, shape):
    rng = np.random.default_rng(sorted(SHAPES).index(shape))
    assert GBTPlan(1).ldsNodes == LDS_NODES
    for n, d, weighted in SIZES:
        B = 32
        feature, split, first = SHAPES[shape](d, B, rng)
        image = rng.integers(0, B, size=(n, d)).astype(np.uint8)
        plan = GBTPlan(d)
        for loss in LOSS_NAMES:
            exact = loss == "squared" and n % 2 == 1
            value = values(first, rng, exact)
            flat = FlatTree(feature, np.zeros(first.size), first, np.full(first.size, -1), value)
            flat.splitBin = split
            if exact:
                y = rng.integers(-9, 10, size=n).astype(np.float64)
                pred0 = rng.integers(-16, 17, size=n) / 8.0
                w = rng.integers(1, 17, size=n) / 8.0 if weighted else None
                weight = 0.5
            else:
                y = rng.choice([-1.0, 1.0], size=n) if loss == "logistic" else rng.normal(size=n) * 3
                pred0 = rng.normal(size=n)
                w = rng.uniform(0.25, 4.0, size=n) if weighted else None
                weight = 0.1
            got = run_update(plan, dev(image), flat, weight, loss, dev(y), dev(w), pred0)
            ref = reference(image.astype(int), feature, split, first, value, weight, loss, pred0,
                            y, w)
            check_update(got, ref, loss, exact, (shape, n, d, loss))
            # without resid nothing else changes
            bare = run_update(plan, dev(image), flat, weight, loss, dev(y), dev(w), pred0, False)
            assert bare[0].tobytes() == got[0].tobytes() and bare[2].tobytes() == got[2].tobytes()


def test_update_image_256_bins(cuda):
    """Bins reach 255 and a split bin 254: the byte compare is unsigned."""
    rng = np.random.default_rng(7)
    n, d = 513, 3
    image = rng.choice(np.array([0, 127, 128, 254, 255], dtype=np.uint8), size=(n, d))
    feature = np.array([1, 0, 2, -1, -1, -1, -1], dtype=np.int32)
    split = np.array([254, 127, 254, -1, -1, -1, -1], dtype=np.int32)
    first = np.array([1, 3, 5, -1, -1, -1, -1], dtype=np.int32)
    value = np.array([1e300, 1e300, 1e300, 1.0, 2.0, 3.0, 4.0])
    flat = FlatTree(feature, np.zeros(7), first, np.full(7, -1), value)
    flat.splitBin = split
    y, pred0 = rng.normal(size=n), np.zeros(n)
    got = run_update(GBTPlan(d), dev(image), flat, 1.0, "squared", dev(y), None, pred0)
    ref = reference(image.astype(int), feature, split, first, value, 1.0, "squared", pred0, y, None)
    check_update(got, ref, "squared", False, "256 bins")
    assert set(got[0].tolist()) == {1.0, 2.0, 3.0, 4.0}
    assert np.all(got[0][image[:, 1] == 255] >= 3.0) and np.all(got[0][image[:, 1] == 254] <= 2.0)


@pytest.mark.parametrize("shape", ["depth5", "lds+1"])
def test_update_rows_equal_image(cuda, shape):
    rng = np.random.default_rng(5)
    n, d, B = 1031, 5, 16
    thresholds = [np.sort(rng.choice(np.arange(-40, 41) / 8.0, size=B - 1, replace=False))
                  for _ in range(d)]
    X = rng.integers(-48, 49, size=(n, d)) / 8.0          # many rows exactly on a threshold
    X[::17, 0], X[5::23, 1], X[3::29, d - 1] = np.inf, -np.inf, np.inf
    image = np.stack([np.searchsorted(thresholds[f], X[:, f], "left") for f in range(d)],
                     axis=1).astype(np.uint8)
    feature, split, first = SHAPES[shape](d, B, rng)
    thr = np.array([thresholds[f][s] if f >= 0 else 0.0 for f, s in zip(feature, split)])
    on = sum(int(np.any(X[:, f] == t)) for f, t, c in zip(feature, thr, first) if c >= 0)
    assert on > 0, "no row sits on a threshold of the tree"
    plan = GBTPlan(d)
    for loss in LOSS_NAMES:
        value = values(first, rng, False)
        flat = FlatTree(feature, thr, first, np.full(first.size, -1), value)
        y = rng.choice([-1.0, 1.0], size=n) if loss == "logistic" else rng.normal(size=n)
        w, pred0 = rng.uniform(0.5, 2.0, size=n), rng.normal(size=n)
        byRows = run_update(plan, dev(X), flat, 0.3, loss, dev(y), dev(w), pred0)
        flat.splitBin = split
        byImage = run_update(plan, dev(image), flat, 0.3, loss, dev(y), dev(w), pred0)
        for a, b in zip(byRows, byImage):
            assert a.tobytes() == b.tobytes(), (shape, loss)
        ref = reference(X, feature, thr, first, value, 0.3, loss, pred0, y, w)
        check_update(byRows, ref, loss, False, (shape, loss, "rows"))


# --------------------------------------------------------------------- predict
def model_tree(numInternal, d, rng, leafValue=None):
    feature, _, first = bfs_tree(numInternal, d, 2, rng)
    thr = np.where(first >= 0, np.round(rng.normal(size=first.size), 1), 0.0)
    vals = rng.normal(size=first.size) if leafValue is None else np.full(first.size, leafValue)
    return DecisionTreeRegressionModel.from_arrays(feature, thr, first, list(vals), d)


def check_predict(model, X):
    Xd = dev(X)
    classifier = isinstance(model, GBTClassificationModel)

    def call():
        out = [model.predictLeaf(Xd), model.predict(Xd)]
        if classifier:
            out += [model.margin(Xd), model.predictRaw(Xd), model.predictProbability(Xd)]
        return tuple(o.cpu().numpy() for o in out)

    got = twice(call)
    roots = [t.rootNode for t in model.trees]
    mg = np.array([G.margin(roots, model.treeWeights, x) for x in X.tolist()])
    leaf = np.array([[R.descend(root, x)[1] for root in roots] for x in X.tolist()], dtype=np.int32)
    assert got[0].dtype == np.int32 and got[0].tobytes() == leaf.tobytes()
    for t, tree in enumerate(model.trees):
        assert got[0][:, t].tobytes() == tree.predictLeaf(Xd).cpu().numpy().tobytes(), t
    if not classifier:
        assert got[1].tobytes() == mg.tobytes()
        return got
    ref = [G.classify(v) for v in mg.tolist()]
    assert got[2].tobytes() == mg.tobytes()
    assert got[3].tobytes() == np.array([r[0] for r in ref]).tobytes()
    assert got[3].tobytes() == np.stack([-got[2], got[2]], axis=1).tobytes()
    assert np.all(np.abs(got[4] - np.array([r[1] for r in ref])) <= 1e-10)
    assert got[1].tobytes() == np.array([r[2] for r in ref]).tobytes()
    return got


@pytest.mark.parametrize("nt", [1, 2, 20])
def test_predict(cuda, nt):
    rng = np.random.default_rng(nt)
    d = 7
    X = np.round(rng.normal(size=(513, d)), 1)
    trees = [model_tree(int(rng.integers(0, 32)), d, rng) for _ in range(nt)]
    weights = [1.0] + [0.1] * (nt - 1)
    check_predict(GBTRegressionModel.from_trees(trees, weights, d), X)
    check_predict(GBTClassificationModel.from_trees(trees, weights, d), X[:257])


def test_predict_past_the_lds(cuda):
    """Two trees of 1023 nodes fill a tile, the third opens the next; a tree of
    2049 nodes is read from global memory; the sum stays in tree order."""
    rng = np.random.default_rng(9)
    d = 5
    X = np.round(rng.normal(size=(300, d)), 1)
    small = [model_tree(511, d, rng) for _ in range(3)]
    assert sum(t.numNodes for t in small[:2]) <= LDS_NODES < sum(t.numNodes for t in small)
    check_predict(GBTClassificationModel.from_trees(small, [1.0, 0.3, 0.3], d), X)
    big = model_tree(LDS_NODES // 2, d, rng)
    assert big.numNodes == LDS_NODES + 1
    mixed = [small[0], big, small[1], model_tree(3, d, rng), big]
    check_predict(GBTRegressionModel.from_trees(mixed, [1.0, 0.5, 0.25, 0.1, 0.1], d), X)


def test_predict_zero_margins(cuda):
    d = 2
    X = np.zeros((3, d))
    rng = np.random.default_rng(0)
    plus, minus = model_tree(0, d, rng, 1.0), model_tree(0, d, rng, -1.0)
    negzero = model_tree(0, d, rng, -0.0)
    got = check_predict(GBTClassificationModel.from_trees([plus, minus], [1.0, 1.0], d), X)
    assert got[2].tobytes() == np.zeros(3).tobytes() and got[1].tolist() == [0.0] * 3
    assert got[4].tolist() == [[0.5, 0.5]] * 3
    got = check_predict(GBTClassificationModel.from_trees([negzero], [1.0], d), X)
    assert got[2].tobytes() == np.zeros(3).tobytes()          # 0.0 + -0.0
    assert got[3].tobytes() == np.array([[-0.0, 0.0]] * 3).tobytes() and got[1].tolist() == [0.0] * 3
    got = check_predict(GBTClassificationModel.from_trees([plus], [0.1], d), X)
    assert got[1].tolist() == [1.0] * 3


# ------------------------------------------------------------------------- fits
def same_models(a, b):
    assert a.getNumTrees == b.getNumTrees and a.treeWeights.tobytes() == b.treeWeights.tobytes()
    for t, (x, y) in enumerate(zip(a.trees, b.trees)):
        assert F.same_node(x.rootNode, y.rootNode), f"tree {t} differs"


def test_fit_exact_design(cuda):
    rng = np.random.default_rng(1)
    signs = np.array([[a, b, c] for a in (-1, 1) for b in (-1, 1) for c in (-1, 1)], dtype=np.float64)
    X = np.concatenate([np.repeat(signs, 512, axis=0) * rng.integers(1, 9, size=(4096, 3)) / 4.0,
                        rng.integers(-8, 9, size=(4096, 2)) / 8.0], axis=1)
    X = np.ascontiguousarray(X[rng.permutation(4096)])
    y = 4.0 * (X[:, 0] > 0) + 2.0 * (X[:, 1] > 0) + 1.0 * (X[:, 2] > 0)
    est = GBTRegressor(maxIter=4, maxDepth=2, stepSize=0.5, seed=3)
    host = est.fit_step(GBTNumpyStep(X, y), 5)
    assert [t.numNodes for t in host.trees] == [7, 3, 1, 1]

    def fit():
        step = GBTDeviceStep(dev(X), dev(y))
        model = est.fit_step(step, 5)
        same_models(model, host)
        return (step.pred.cpu().numpy(), step.residual())

    pred, resid = twice(fit)
    assert pred.tobytes() == y.tobytes() and not resid.any()
    assert est.fit(dev(X), dev(y)).predict(dev(X)).cpu().numpy().tobytes() == y.tobytes()


def real_rows(seed, classifier, n=2000, d=8):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, d))
    f = X[:, 0] + np.sin(2.0 * X[:, 1]) - 0.5 * (X[:, 2] > 0.3) + 0.25 * X[:, 3] * X[:, 4]
    y = (f + 0.3 * rng.normal(size=n) > 0).astype(np.float64) if classifier else \
        f + 0.3 * rng.normal(size=n)
    return X, y, rng.uniform(0.5, 2.0, size=n)


REAL = {"squared": 0, "absolute": 0, "logistic": 0}       # the seeds of the stable inputs


@pytest.mark.parametrize("loss", LOSS_NAMES)
def test_fit_real_rows(cuda, loss):
    classifier = loss == "logistic"
    X, y, w = real_rows(REAL[loss], classifier)
    kw = dict(maxIter=5, maxDepth=3, stepSize=0.3)
    # the input's condition, on the CPU before any device call: a 1e-9 relative
    # perturbation of every residual leaves the restatement's structure alone
    args = (X.tolist(), y.tolist(), w.tolist(), loss, classifier, 5, 0.3, 8, 3)
    base = [G.structure(r) for r in G.fit_gbt(*args, seed=2)[0]]
    sign = np.random.default_rng(1).choice([-1.0, 1.0], size=(5, X.shape[0]))
    for flip in (1.0, -1.0):
        moved = G.fit_gbt(*args, seed=2, perturb=lambda it, res: [
            v * (1.0 + flip * s * 1e-9) for v, s in zip(res, sign[it])])[0]
        assert [G.structure(r) for r in moved] == base, "pick another seed: a near-tie"
    Est = GBTClassifier if classifier else GBTRegressor
    est = Est(lossType=loss, seed=2, **kw)
    host = est.fit_step(GBTNumpyStep(X, y, w, classifier=classifier), 8)
    assert [G.structure(t.rootNode) for t in host.trees] == base
    model = est.fit(dev(X), dev(y), dev(w))
    assert [G.structure(t.rootNode) for t in model.trees] == base
    for a, b in zip(model.trees, host.trees):
        va, vb = np.array(G.leaf_values(a.rootNode)), np.array(G.leaf_values(b.rootNode))
        assert np.all(np.abs(va - vb) <= np.maximum(1e-10 * np.abs(vb), 1e-12))
    roots = [t.rootNode for t in host.trees]
    want = np.array([G.margin(roots, host.treeWeights, x) for x in X.tolist()])
    got = (model.margin(dev(X)) if classifier else model.predict(dev(X))).cpu().numpy()
    assert np.all(np.abs(got - want) <= 1e-9)
    # evaluateEachIteration on the training rows: the host's within 1e-10
    errs = model.evaluateEachIteration(dev(X), dev(y), dev(w))
    ref = host.evaluate_step(GBTNumpyStep(X, y, w, classifier=classifier, residuals=False))
    assert len(errs) == 5 and np.allclose(errs, ref, rtol=1e-9, atol=0.0)


def test_fit_with_validation_stops_at_the_same_tree(cuda):
    rng = np.random.default_rng(21)
    X = rng.normal(size=(260, 4))
    X[:, 0] = np.round(X[:, 0], 1)
    y = X[:, 0] + np.sin(2.0 * X[:, 1]) - 0.5 * (X[:, 3] > 0.3) + 0.3 * rng.normal(size=260)
    w = rng.uniform(0.25, 4.0, size=260)
    tr, va = slice(0, 180), slice(180, 260)
    est = GBTRegressor(maxIter=6, stepSize=0.5, maxDepth=2, validationTol=0.3, seed=9)
    host = est.fit_step(GBTNumpyStep(X[tr], y[tr], w[tr]), 4,
                        validation=GBTNumpyStep(X[va], y[va], w[va], residuals=False))
    assert 1 <= host.getNumTrees < 6
    model = est.fit(dev(X[tr]), dev(y[tr]), dev(w[tr]),
                    validation=(dev(X[va]), dev(y[va]), dev(w[va])))
    assert model.getNumTrees == host.getNumTrees
    assert [G.structure(t.rootNode) for t in model.trees] == \
        [G.structure(t.rootNode) for t in host.trees]
