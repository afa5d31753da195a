"""DecisionTree on the device (csrc/decision_tree.hip) against the row-by-row
restatement of tests/decision_tree_restatement.py.

  bin        equals np.searchsorted(thresholds, x, "left") byte for byte
  histogram  exact rows (integer labels, weights in eighths) by bytes; real
             weights and labels within 1e-10 of the sum of the absolute terms
             of each entry (a sum of m terms in any order is within m 2^-53 of
             that sum; m < 2^15 here); nodes of one, two and three runs, with
             workspaces of one, two and three runs per launch
  route      equals the row-by-row rule; the threshold's own bin goes left
  predict    leaf, prediction, raw and probability equal the restatement's
             descent bit for bit
  fit        DeviceStep fits equal NumpyStep fits by bytes on exact rows
Every device call runs twice and the two results are compared by tobytes().
"""
import numpy as np
import pytest
import torch

import decision_tree_restatement as R
from cycloneml_amd import _native as N
from cycloneml_amd import tree as T
from cycloneml_amd.tree import (DecisionTreeClassificationModel, DecisionTreeClassifier,
                                DecisionTreeRegressionModel, DecisionTreeRegressor, DeviceStep,
                                DTPlan, NumpyStep)

pytestmark = pytest.mark.gpu


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def twice(fn):
    a, b = fn(), fn()
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes(), "two calls differ"
    return a


# ------------------------------------------------------------------------- bin
def bin_case(n, d, splits, seed):
    rng = np.random.default_rng(seed)
    thr = []
    for f in range(d):
        k = splits if f % 3 != 1 else min(splits, 5)
        t = np.sort(rng.choice(np.arange(-300, 300), size=k, replace=False) / 4.0)
        if k and f % 2 == 0:
            t[np.argmin(np.abs(t))] = 0.0           # a threshold at 0.0 for the -0.0 rows
            t = np.unique(t)
        thr.append(t)
    X = rng.normal(size=(n, d)) * 40.0
    for f in range(d):
        if len(thr[f]):
            on = rng.integers(0, n, size=max(1, n // 3))
            X[on, f] = rng.choice(thr[f], size=on.size)       # exactly on a threshold
    for r, v in zip(rng.integers(0, n, size=4), (np.inf, -np.inf, -0.0, 0.0)):
        X[r, rng.integers(0, d)] = v
    X[0, 0] = -0.0
    return X, thr


@pytest.mark.parametrize("d", [1, 3, 64, 65, 257])
def test_bin(cuda, d):
    plan = DTPlan(d, 2)
    for n in (1, 63, 64, 65, 257, 2049):
        for splits in (0, 1, 31, 255):
            X, thr = bin_case(n, d, splits, seed=n + splits)
            Xd = dev(X)
            (img,) = twice(lambda: (plan.bin(Xd, thr).cpu().numpy(),))
            ref = np.stack([np.searchsorted(thr[f], X[:, f], "left") for f in range(d)], axis=1)
            assert img.shape == (n, d) and np.array_equal(img, ref.astype(np.uint8)), (n, splits)


# ------------------------------------------------------------------- histogram
RUN = 4096
SLOT_NODE = np.array([0, -1, 1, 2], dtype=np.int32)      # slot 1 sits this call out


def hist_case(kind, n, d, C, B, seed):
    rng = np.random.default_rng(seed)
    image = rng.integers(0, B, size=(n, d)).astype(np.uint8)
    if kind == "exact":
        y = rng.integers(0, C, size=n) if C else rng.integers(-9, 10, size=n)
        w = rng.integers(1, 17, size=n) / 8.0
    else:
        y = rng.integers(0, C, size=n) if C else rng.normal(size=n) * 3.0
        w = rng.uniform(0.25, 4.0, size=n)
    y = y.astype(np.float64)
    slot = rng.choice(np.array([0, 0, 0, 2, 2, 1, -1], dtype=np.int32), size=n)
    if n > 4:
        slot[n // 2] = 3                                  # a node with one row
    poisoned = image.copy()
    poisoned[(slot == -1) | (slot == 1)] = 255            # never to be read into a sum
    return image, poisoned, y, w, slot


def reference_hist(image, y, w, slot, C, B):
    out, bar = [], []
    rows_img = image.tolist()
    for s in (0, 2, 3):
        rows = np.nonzero(slot == s)[0].tolist()
        out.append(R.histogram(rows_img, y, w, rows, C, B))
        bar.append(R.histogram(rows_img, y if C else np.abs(y), w, rows, C, B))
    return np.array(out), np.array(bar)


def run_hist(plan, poisoned, y, w, slot, nodeOf, K, B):
    args = dev(poisoned), dev(y), dev(w), dev(slot)
    return twice(lambda: (plan.histogram(*args, nodeOf, K, B).cpu().numpy(),))[0]


def check_hist(kind, n, d, C, B, weighted=True, seed=0):
    image, poisoned, y, w, slot = hist_case(kind, n, d, C, B, seed)
    w = w if weighted else None
    ref, bar = reference_hist(image, y, w, slot, C, B)
    got = run_hist(DTPlan(d, C), poisoned, y, w, slot, SLOT_NODE, 3, B)
    assert got.shape == ref.shape
    if kind == "exact":
        assert got.tobytes() == ref.tobytes()
    err = np.abs(got - ref)
    print(f"{kind} n={n} d={d} C={C} B={B}: worst error / bar = "
          f"{float(np.max(err / np.maximum(bar, 1e-300))):.3e}")
    assert np.all(err <= 1e-10 * bar)
    # a workspace of one run per launch, and the nodes one call at a time
    small = DTPlan(d, C, workspaceBytes=1)
    assert small.runs_per_launch(B) == 1
    assert run_hist(small, poisoned, y, w, slot, SLOT_NODE, 3, B).tobytes() == got.tobytes()
    for node in range(3):
        one = np.where(SLOT_NODE == node, 0, -1).astype(np.int32)
        part = run_hist(small, poisoned, y, w, slot, one, 1, B)
        assert part[0].tobytes() == got[node].tobytes()


@pytest.mark.parametrize("kind", ["exact", "real"])
@pytest.mark.parametrize("C", [2, 3, 17, 0])
def test_histogram_run_edges(cuda, C, kind):
    # three nodes, parked rows and a slot that sits out
    for n in (RUN - 1, RUN, RUN + 1, 2 * RUN + 1):
        check_hist(kind, n, 5, C, 32, seed=n + C)
    # every row in the one node: n itself around the run length
    for n in (RUN - 1, RUN, RUN + 1, 2 * RUN + 1):
        image, _, y, w, _ = hist_case(kind, n, 3, C, 4, seed=n)
        ref = np.array(R.histogram(image.tolist(), y, w, range(n), C, 4))
        bar = np.array(R.histogram(image.tolist(), y if C else np.abs(y), w, range(n), C, 4))
        one = np.zeros(1, dtype=np.int32)
        got = run_hist(DTPlan(3, C), image, y, w, None, one, 1, 4)[0]
        if kind == "exact":
            assert got.tobytes() == ref.tobytes()
        assert np.all(np.abs(got - ref) <= 1e-10 * bar)
        # one run per launch: the node's runs are folded over several launches
        small = DTPlan(3, C, workspaceBytes=1)
        assert small.runs_per_launch(4) == 1
        assert run_hist(small, image, y, w, None, one, 1, 4)[0].tobytes() == got.tobytes()


def ws_of(runs, d, C, B):
    return runs * 8 * T.num_stats(C) * B * d


@pytest.mark.parametrize("kind", ["exact", "real"])
@pytest.mark.parametrize("C", [3, 0])
def test_histogram_runs_across_launches(cuda, C, kind):
    """Nodes of 3 runs, of 2 runs and of a single row: with 2 runs per
    launch node 0's runs straddle the first launch boundary and node 1's the
    second; with 1 and 3 per launch the boundaries fall elsewhere.  Every
    grouping gives the default workspace's bytes."""
    n, d, B = 5 * RUN + 7, 3, 4
    rng = np.random.default_rng(C + 5)
    image = rng.integers(0, B, size=(n, d)).astype(np.uint8)
    _, _, y, w, _ = hist_case(kind, n, d, C, B, seed=C)
    slot = rng.choice(np.array([0, 0, 0, 0, 0, 2, 2, 2, 1, -1], dtype=np.int32), size=n)
    slot[n // 2] = 3
    sizes = [int(np.sum(slot == s)) for s in (0, 2, 3)]
    assert 2 * RUN < sizes[0] <= 3 * RUN and RUN < sizes[1] <= 2 * RUN and sizes[2] == 1
    poisoned = image.copy()
    poisoned[(slot == -1) | (slot == 1)] = 255
    ref, bar = reference_hist(image, y, w, slot, C, B)
    got = run_hist(DTPlan(d, C), poisoned, y, w, slot, SLOT_NODE, 3, B)
    if kind == "exact":
        assert got.tobytes() == ref.tobytes()
    err = np.abs(got - ref)
    print(f"{kind} n={n} C={C}: worst error / bar = "
          f"{float(np.max(err / np.maximum(bar, 1e-300))):.3e}")
    assert np.all(err <= 1e-10 * bar)
    for runs in (1, 2, 3):
        plan = DTPlan(d, C, workspaceBytes=ws_of(runs, d, C, B))
        assert plan.runs_per_launch(B) == runs
        assert run_hist(plan, poisoned, y, w, slot, SLOT_NODE, 3, B).tobytes() == got.tobytes()
        for node in range(3):
            one = np.where(SLOT_NODE == node, 0, -1).astype(np.int32)
            part = run_hist(plan, poisoned, y, w, slot, one, 1, B)
            assert part[0].tobytes() == got[node].tobytes()


@pytest.mark.parametrize("B", [2, 32, 256])
@pytest.mark.parametrize("C", [2, 17, 0])
def test_histogram_bins_and_passes(cuda, C, B):
    check_hist("exact", 700, 7, C, B, seed=B + C)
    check_hist("real", 700, 7, C, B, weighted=(B != 32), seed=B + C + 1)


@pytest.mark.parametrize("d", [1, 64, 65, 130])
def test_histogram_feature_panels(cuda, d):
    check_hist("exact", 300, d, 3, 8, seed=d)


# ----------------------------------------------------------------------- route
def test_route(cuda):
    rng = np.random.default_rng(1)
    n, d = 2049, 9
    image = rng.integers(0, 12, size=(n, d)).astype(np.uint8)
    slot = rng.choice(np.array([0, 1, 2, 3, -1, 7], dtype=np.int32), size=n)
    table = np.array([[4, 5, 0, 1], [-1, -1, -1, -1], [0, 0, -1, 2], [8, 10, 3, -1]],
                     dtype=np.int32)
    image[:40, 4] = 5                                     # the threshold's own bin
    ref = np.empty(n, dtype=np.int32)
    for r in range(n):
        s = int(slot[r])
        if not 0 <= s < 4 or table[s, 0] < 0:
            ref[r] = -1
        else:
            ref[r] = table[s, 2] if image[r, table[s, 0]] <= table[s, 1] else table[s, 3]
    plan = DTPlan(d, 2)
    imd = dev(image)

    def run():
        sd = dev(slot)
        plan.route(imd, sd, table)
        return (sd.cpu().numpy(),)
    (got,) = twice(run)
    assert np.array_equal(got, ref)
    at = np.nonzero((slot[:40] == 0))[0]
    assert at.size and np.all(got[at] == 0)
    ns = NumpyStep(np.zeros((n, d)), np.zeros(n), None, 2)
    ns.image, ns.slot = image, slot.copy()
    ns.route(table)
    assert np.array_equal(ns.slot, ref)


# --------------------------------------------------------------------- predict
def chain_model(depth, d, C, rng):
    """A chain: every internal node's left child is a leaf, down to `depth`."""
    m = 2 * depth + 1
    feature, thr, first = np.full(m, -1), np.zeros(m), np.full(m, -1)
    node = 0
    for lvl in range(depth):
        feature[node], thr[node], first[node] = rng.integers(0, d), float(lvl - depth // 2), 2 * lvl + 1
        node = 2 * lvl + 2
    values = rng.integers(0, 9, size=(m, C)) / 8.0 if C else rng.normal(size=m)
    if C:
        values[m - 1] = 0.0                               # a zero-sum leaf
    return feature, thr, first, values


@pytest.mark.parametrize("depth", [0, 1, 30])
def test_predict(cuda, depth):
    rng = np.random.default_rng(depth)
    n, d, C = 2049, 5, 3
    X = rng.integers(-16, 17, size=(n, d)).astype(np.float64)     # many rows on thresholds
    X[3, :] = np.inf
    X[4, :] = -np.inf
    X[5, :] = 100.0                                       # down the whole chain
    Xd = dev(X)
    feature, thr, first, values = chain_model(depth, d, C, rng)
    cm = DecisionTreeClassificationModel.from_arrays(feature, thr, first, values, d)
    rm = DecisionTreeRegressionModel.from_arrays(feature, thr, first, values[:, 0] * 3.0, d)
    assert cm.depth == depth and cm._plan is None
    leaf, pred, raw, prob = twice(lambda: tuple(
        t.cpu().numpy() for t in (cm.predictLeaf(Xd), cm.predict(Xd), cm.predictRaw(Xd),
                                  cm.predictProbability(Xd))))
    rleaf, rpred = twice(lambda: (rm.predictLeaf(Xd).cpu().numpy(), rm.predict(Xd).cpu().numpy()))
    for r in range(n):
        nd, li = R.descend(cm.rootNode, X[r])
        assert leaf[r] == li and rleaf[r] == li
        assert pred[r] == nd.prediction
        assert raw[r].tobytes() == nd.impurityStats.tobytes()
        assert prob[r].tobytes() == np.array(R.probability(nd.impurityStats.tolist())).tobytes()
        assert np.float64(rpred[r]).tobytes() == np.float64(R.descend(rm.rootNode, X[r])[0].prediction).tobytes()
    if depth == 30:
        assert leaf[5] == 30 and np.all(raw[5] == 0.0) and np.all(prob[5] == 0.0)
        assert set(leaf.tolist()) >= {0, 30}


# ----------------------------------------------------------------------- check
def test_check_names_the_lowest_row(cuda):
    X, ycls, yreg, w = R.exact_rows(2049, 7, seed=3)
    X[100, 2] = np.inf                                    # legal
    plan = DTPlan(7, 3)
    plan.check(dev(X), dev(ycls), dev(w))
    plan.check(dev(X), dev(ycls), None)

    def refused(plan, X, y, w, row, rule):
        with pytest.raises(N.IllegalArgumentException, match=rf"row {row}\)"):
            plan.check(dev(X), dev(y), dev(w))
        assert (plan.badRow, plan.badRule) == (row, rule)
        with pytest.raises(N.IllegalArgumentException, match=rf"row {row}\)"):
            NumpyStep(X, y, w, plan.numClasses).check()

    bad = X.copy()
    bad[1500, 6] = bad[700, 0] = np.nan
    refused(plan, bad, ycls, w, 700, T.RULE_FEATURE)
    for v in (3.0, -1.0, 0.5, np.nan, 1e300):
        yb = ycls.copy()
        yb[2048] = yb[1234] = v
        refused(plan, X, yb, w, 1234, T.RULE_LABEL)
    for v in (-0.125, np.inf, np.nan):
        wb = w.copy()
        wb[2000] = wb[64] = v
        refused(plan, X, ycls, wb, 64, T.RULE_WEIGHT)
    reg = DTPlan(7, 0)
    reg.check(dev(X), dev(yreg), dev(w))
    yb = yreg.copy()
    yb[9] = -np.inf
    refused(reg, X, yb, w, 9, T.RULE_LABEL)


# ------------------------------------------------------------------------- fit
FITS = [("gini", True, {}), ("gini", False, {"minInstancesPerNode": 9}),
        ("entropy", True, {"minInfoGain": 0.01}), ("entropy", False, {}),
        ("variance", True, {"minInstancesPerNode": 4}), ("variance", False, {"minInfoGain": 0.05})]


@pytest.fixture(scope="module")
def exact_fit_rows():
    return R.exact_rows(2049, 17, seed=21)


@pytest.mark.parametrize("impurity,weighted,extra", FITS)
def test_device_fit_equals_numpy_fit(cuda, exact_fit_rows, impurity, weighted, extra):
    X, ycls, yreg, w = exact_fit_rows
    C = 0 if impurity == "variance" else 3
    y = yreg if impurity == "variance" else ycls
    w = w if weighted else None
    kw = dict(maxDepth=6, impurity=impurity, **extra)
    est = DecisionTreeClassifier(numClasses=3, **kw) if C else DecisionTreeRegressor(**kw)

    def same(a, b):
        if a.isLeaf != b.isLeaf or a.stats.tobytes() != b.stats.tobytes() \
                or a.prediction != b.prediction or a.impurity != b.impurity:
            return False
        return a.isLeaf or (a.split == b.split and a.gain == b.gain
                            and same(a.left, b.left) and same(a.right, b.right))

    host = est.fit_step(NumpyStep(X, y, w, C), 17, *([3] if C else []))
    fits = [est.fit(dev(X), dev(y), dev(w)) for _ in range(2)]
    # a workspace of one run per launch: the same tree
    fits.append(est.fit_step(DeviceStep(dev(X), dev(y), dev(w), C, workspaceBytes=1), 17,
                             *([3] if C else [])))
    assert host.depth >= 3 and host.numNodes >= 9
    for m in fits:
        assert same(m.rootNode, host.rootNode)
        assert m.featureImportances.tobytes() == host.featureImportances.tobytes()
    # the model's own predictions on its training rows
    Xd = dev(X)
    pred, leaf = fits[0].predict(Xd).cpu().numpy(), fits[0].predictLeaf(Xd).cpu().numpy()
    for r in range(0, 2049, 41):
        nd, li = R.descend(host.rootNode, X[r])
        assert pred[r] == nd.prediction and leaf[r] == li


def test_fit_names_the_bad_row_before_counting_classes(cuda):
    X, ycls, _, w = R.exact_rows(257, 5, seed=2)
    est = DecisionTreeClassifier()                         # numClasses from the labels
    for v in (np.nan, -1.0, 1e300, 2.5):
        yb = ycls.copy()
        yb[200] = yb[77] = v
        with pytest.raises(N.IllegalArgumentException, match=r"row 77\)"):
            est.fit(dev(X), dev(yb), dev(w))
    wb = w.copy()
    wb[31] = np.nan
    with pytest.raises(N.IllegalArgumentException, match=r"row 31\)"):
        est.fit(dev(X), dev(ycls), dev(wb))
    with pytest.raises(N.IllegalArgumentException, match="device"):
        est.fit(torch.from_numpy(X), torch.from_numpy(ycls))
    assert est.fit(dev(X), dev(ycls), dev(w)).numClasses == 3


def test_device_fit_on_real_rows(cuda):
    rng = np.random.default_rng(8)
    n, d = 2049, 17
    X = rng.normal(size=(n, d))
    y = ((X[:, 2] + 0.5 * X[:, 11] > 0.2) ^ (rng.random(n) < 0.05)).astype(np.float64)
    w = rng.uniform(0.25, 4.0, size=n)
    est = DecisionTreeClassifier(maxDepth=4, minInfoGain=1e-3)
    host = est.fit_step(NumpyStep(X, y, w, 2), d, 2)
    m = est.fit(dev(X), dev(y), dev(w))
    assert m.numClasses == 2 and m.numNodes == host.numNodes >= 5
    assert np.array_equal(m._feature, host._feature) and np.array_equal(m._first, host._first)
    assert m._threshold.tobytes() == host._threshold.tobytes()
    # a leaf's class weights are sums of positive weights: their own sum of absolute terms
    assert np.all(np.abs(m._leafRaw - host._leafRaw) <= 1e-10 * host._leafRaw)
    yr = X[:, 2] * 2.0 + rng.normal(size=n) * 0.1
    reg = DecisionTreeRegressor(maxDepth=4, minInfoGain=1e-3)
    hr = reg.fit_step(NumpyStep(X, yr, w, 0), d)
    mr = reg.fit(dev(X), dev(yr), dev(w))
    assert np.array_equal(mr._feature, hr._feature)
    # sum / count with either within 1e-10 of its absolute terms: the error of the
    # quotient is below 1e-10 (mean |y| + |prediction|), and mean |y| <= max |y|
    assert np.all(np.abs(mr._leafPred - hr._leafPred)
                  <= 1e-10 * (np.max(np.abs(yr)) + np.abs(hr._leafPred)))
