"""RandomForest on the device (csrc/random_forest.hip) against the row-by-row
restatement of tests/random_forest_restatement.py.

  bag        equals forest.bag_counts (numpy) byte for byte
  histogram  exact rows (integer labels, weights in eighths, counts from the
             bag) by bytes; real weights and labels within 1e-10 of the sum of the
             absolute terms of each entry (a sum of m terms in any order is within
             m 2^-53 of that sum; m < 2^15 here); image bytes of rows that no tree
             may read (parked, sitting out, drawn 0 times) are poisoned with 255.
             What the poison can show is limited: the kernel never indexes with
             a byte >= B, so below 256 bins a poisoned row gathered by mistake
             adds nothing, and at 256 bins a row drawn 0 times adds +0.0 and a
             count of 0.  So a parked or sitting-out row gathered by mistake is
             caught in the cases with 256 bins only (it lands in bin 255, which
             the reference leaves empty for it); that a row drawn 0 times is not
             LOADED is the key kernel's rule (key K) and is not observable in
             any sum, so no test here asserts it
  route      equals the row-by-row rule for every tree
  predict    leaf matrix, raw, probability, argmax and mean equal the
             restatement's bit for bit
  fit        ForestDeviceStep fits equal ForestNumpyStep fits by bytes on exact rows
Every device call runs twice and the two results are compared by tobytes().
"""
import numpy as np
import pytest
import torch

import decision_tree_restatement as R
import random_forest_restatement as F
from cycloneml_amd import _native as N
from cycloneml_amd import forest as RF
from cycloneml_amd.forest import (ForestDeviceStep, ForestNumpyStep, RandomForestClassificationModel,
                                  RandomForestClassifier, RandomForestRegressionModel,
                                  RandomForestRegressor, RFPlan)
from cycloneml_amd.tree import (DecisionTreeClassificationModel, DecisionTreeClassifier,
                                DecisionTreeRegressionModel, DTPlan)

pytestmark = pytest.mark.gpu


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def twice(fn):
    a, b = fn(), fn()
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes(), "two calls differ"
    return a


# ------------------------------------------------------------------------- bag
@pytest.mark.parametrize("nt", [1, 3])
def test_bag(cuda, nt):
    plan = RFPlan(4, 2)
    for table in (RF.poisson_table(1.0), RF.poisson_table(0.3), RF.bernoulli_table(0.3)):
        for n in (1, 255, 256, 257, 4097):
            off = 1_000_003 + n
            (got,) = twice(lambda: (plan.bag(n, nt, table, 17, off).cpu().numpy(),))
            ref = RF.bag_counts(17, nt, n, table, off)
            assert got.shape == (nt, n) and got.tobytes() == ref.tobytes(), (n, len(table))
    # a rank's shard is the whole's piece
    whole = plan.bag(600, nt, RF.poisson_table(1.0), 2, 0).cpu().numpy()
    part = plan.bag(200, nt, RF.poisson_table(1.0), 2, 400).cpu().numpy()
    assert part.tobytes() == whole[:, 400:].tobytes()


# ------------------------------------------------------------------- histogram
def labels_weights(kind, n, C, rng):
    if kind == "exact":
        y = rng.integers(0, C, size=n) if C else rng.integers(-9, 10, size=n)
        w = rng.integers(1, 17, size=n) / 8.0
    else:
        y = rng.integers(0, C, size=n) if C else rng.normal(size=n) * 3.0
        w = rng.uniform(0.25, 4.0, size=n)
    return y.astype(np.float64), w


def subsets(K, d, m, rng):
    """K sorted subsets of m features; node 0's holds feature 0 and (m > 1) d - 1,
    node 1's holds d - 1."""
    out = np.stack([np.sort(rng.choice(d, size=m, replace=False)) for _ in range(K)])
    first = [0, d - 1] if m > 1 else [0]
    rest = rng.choice(np.arange(1, d - 1), size=m - len(first), replace=False) if d > 2 else []
    out[0] = np.sort(np.concatenate([first, rest]).astype(np.int64))
    if K > 1 and d - 1 not in out[1]:
        out[1, -1] = d - 1
    return out.astype(np.int32)


class Case:
    """nt trees of 4 slots each: slot 0 -> node 3 t, slot 1 sits out, slot 2 ->
    node 3 t + 1, slot 3 (a single pair) -> node 3 t + 2."""

    def __init__(self, kind, n, d, m, C, B, nt=3, weighted=True, bagged=True, seed=0):
        rng = np.random.default_rng(seed)
        self.n, self.d, self.m, self.C, self.B, self.nt = n, d, m, C, B, nt
        self.image = rng.integers(0, B, size=(n, d)).astype(np.uint8)
        self.y, w = labels_weights(kind, n, C, rng)
        self.w = w if weighted else None
        self.bag = RF.bag_counts(seed, nt, n, RF.poisson_table(1.0)) if bagged else None
        self.slot = rng.choice(np.array([0, 0, 0, 2, 2, 1, -1], dtype=np.int32), size=(nt, n))
        if n >= 40:
            self.slot[:, 0::10] = -1                       # parked in every tree
            self.slot[:, 1::10] = 1                        # sitting out in every tree
            if bagged:
                self.bag[:, 2::10] = 0                     # drawn 0 times by every tree
        for t in range(nt):
            ok = np.nonzero((self.slot[t] == 0) & (self.bag[t] > 0 if bagged else True))[0]
            if ok.size:
                self.slot[t, ok[ok.size // 2]] = 3
        self.K = 3 * nt
        self.slotStart = 4 * np.arange(nt + 1, dtype=np.int32)
        self.nodeOf = np.concatenate([[3 * t, -1, 3 * t + 1, 3 * t + 2] for t in range(nt)]).astype(np.int32)
        self.feats = None if m == d and seed % 2 else subsets(self.K, d, m, rng)
        unread = np.ones(n, dtype=bool)
        for t in range(nt):
            live = (self.slot[t] != -1) & (self.slot[t] != 1)
            if bagged:
                live &= self.bag[t] > 0
            unread &= ~live
        self.poisoned = self.image.copy()
        self.poisoned[unread] = 255                        # never to be read into a sum
        self.unread = int(unread.sum())

    def rows_of(self, node):
        t, s = node // 3, (0, 2, 3)[node % 3]
        return t, np.nonzero(self.slot[t] == s)[0].tolist()

    def reference(self):
        img = self.image.tolist()
        out, bar = [], []
        for k in range(self.K):
            t, rows = self.rows_of(k)
            feats = list(range(self.d)) if self.feats is None else self.feats[k].tolist()
            cnt = None if self.bag is None else self.bag[t]
            out.append(F.histogram(img, self.y, self.w, cnt, rows, feats, self.C, self.B))
            bar.append(F.histogram(img, self.y if self.C else np.abs(self.y), self.w, cnt, rows,
                                   feats, self.C, self.B))
        return np.array(out), np.array(bar)

    def device(self):
        return dict(image=dev(self.poisoned), y=dev(self.y), weights=dev(self.w),
                    bag=dev(self.bag), slot=dev(self.slot))

    def run(self, plan, args, t0=0, t1=None, slotStart=None, nodeOf=None, K=None, feats="all",
            call=None):
        t1 = self.nt if t1 is None else t1
        fn = call or plan.histogram
        return twice(lambda: (fn(
            args["image"], args["y"], args["weights"], args["bag"], args["slot"], t0, t1,
            self.slotStart if slotStart is None else slotStart,
            self.nodeOf if nodeOf is None else nodeOf, self.K if K is None else K, self.m,
            self.feats if isinstance(feats, str) else feats, self.B).cpu().numpy(),))[0]


def check_hist(kind, n, d, m, C, B, **kw):
    case = Case(kind, n, d, m, C, B, **kw)
    ref, bar = case.reference()
    args = case.device()
    got = case.run(RFPlan(d, C), args)
    assert got.shape == ref.shape == (case.K, m, B, (C + 1 if C else 4))
    if kind == "exact":
        assert got.tobytes() == ref.tobytes()
    err = np.abs(got - ref)
    print(f"{kind} n={n} d={d} m={m} C={C} B={B}: unread rows {case.unread}, worst error / bar = "
          f"{float(np.max(err / np.maximum(bar, 1e-300))):.3e}")
    assert np.all(err <= 1e-10 * bar)
    if case.bag is not None:
        assert np.array_equal(got[..., -1], ref[..., -1])       # the raw counts are integers
    # a workspace of one run per launch, the nodes one call at a time, the tree range cut
    small = RFPlan(d, C, workspaceBytes=1)
    assert small.runs_per_launch(m, B) == 1
    assert case.run(small, args).tobytes() == got.tobytes()
    for node in range(case.K):
        one = np.where(case.nodeOf == node, 0, -1).astype(np.int32)
        part = case.run(small, args, nodeOf=one, K=1,
                        feats=None if case.feats is None else case.feats[node:node + 1])
        assert part[0].tobytes() == got[node].tobytes()
    if case.nt > 1:
        cut = RFPlan(d, C)
        cut.maxPairs = n                                    # one tree per call
        assert case.run(cut, args).tobytes() == got.tobytes()
        # the trees [1, nt) alone, as their own call with their own nodes 0 ..
        tail = case.run(cut, args, t0=1, slotStart=case.slotStart[1:] - 4,
                        nodeOf=np.where(case.nodeOf[4:] >= 0, case.nodeOf[4:] - 3, -1),
                        K=case.K - 3, feats=None if case.feats is None else case.feats[3:],
                        call=cut.histogram_call)
        assert tail.tobytes() == got[3:].tobytes()
    return case, got


@pytest.mark.parametrize("kind", ["exact", "real"])
@pytest.mark.parametrize("C", [2, 17, 0])
def test_histogram_classes_and_windows(cuda, C, kind):
    # S B below (C = 2: 96) and above (C = 17: 576, C = 0 at 64 bins: 256) the window of 128
    check_hist(kind, 700, 9, 4, C, 64 if C == 0 else 32, seed=C)
    check_hist(kind, 300, 9, 4, C, 2, weighted=False, seed=C + 1)
    check_hist(kind, 300, 5, 5, C, 256, seed=C + 2)


@pytest.mark.parametrize("m", [1, 2, 16, 63, 64, 65])
def test_histogram_subset_widths(cuda, m):
    case, _ = check_hist("exact", 500, 70, m, 3, 8, seed=2 * m)
    assert 0 in case.feats[0] and (m == 1 or 69 in case.feats[0]) and 69 in case.feats[1]
    check_hist("real", 500, 70, m, 0, 8, seed=2 * m)


@pytest.mark.parametrize("kind", ["exact", "real"])
def test_histogram_all_features_and_no_bag(cuda, kind):
    for d, seed in ((5, 1), (70, 3)):
        case, _ = check_hist(kind, 400, d, d, 3, 8, seed=seed)      # nodeFeat = null
        assert case.feats is None
        check_hist(kind, 400, d, d, 0, 8, seed=seed + 1)            # every feature, listed
        check_hist(kind, 400, d, min(d, 3), 3, 8, bagged=False, seed=seed)
        check_hist(kind, 400, d, d, 2, 8, nt=1, seed=seed)


def pairs_case(kind, pairs, d, m, C, B, seed):
    """Two trees: tree 0's node holds every row it drew, tree 1's node exactly
    `pairs` pairs."""
    rng = np.random.default_rng(seed)
    n = 2 * pairs + 64
    image = rng.integers(0, B, size=(n, d)).astype(np.uint8)
    y, w = labels_weights(kind, n, C, rng)
    bag = RF.bag_counts(seed, 2, n, RF.poisson_table(1.0))
    drawn = np.nonzero(bag[1] > 0)[0]
    assert drawn.size >= pairs
    slot = np.zeros((2, n), dtype=np.int32)
    slot[1] = -1
    slot[1, drawn[:pairs]] = 0
    feats = subsets(2, d, m, rng)
    poisoned = image.copy()
    poisoned[(bag[0] == 0) & (slot[1] < 0)] = 255
    img = image.tolist()
    rows = [list(range(n)), drawn[:pairs].tolist()]
    ref = np.array([F.histogram(img, y, w, bag[t], rows[t], feats[t].tolist(), C, B)
                    for t in range(2)])
    bar = np.array([F.histogram(img, y if C else np.abs(y), w, bag[t], rows[t], feats[t].tolist(),
                                C, B) for t in range(2)])
    assert ref[1, 0, :, -1].sum() == bag[1, drawn[:pairs]].sum()
    args = [dev(a) for a in (poisoned, y, w, bag, slot)]
    ss, nodeOf = np.array([0, 1, 2], dtype=np.int32), np.array([0, 1], dtype=np.int32)

    def run(plan):
        return twice(lambda: (plan.histogram(*args, 0, 2, ss, nodeOf, 2, m, feats, B).cpu().numpy(),))[0]
    got = run(RFPlan(d, C))
    if kind == "exact":
        assert got.tobytes() == ref.tobytes()
    assert np.all(np.abs(got - ref) <= 1e-10 * bar)
    small = RFPlan(d, C, workspaceBytes=1)
    assert small.runs_per_launch(m, B) == 1
    assert run(small).tobytes() == got.tobytes()


@pytest.mark.parametrize("kind", ["exact", "real"])
def test_histogram_run_and_sub_run_edges(cuda, kind):
    plan = RFPlan(5, 3)
    RUN = plan.runRows                                     # the run length the plan reports
    # m features x floor(64 / m) sub-runs of ceil(RUN / sub-runs) pairs up to 64 features
    for m in (1, 2, 3, 5, 10, 16, 21, 22, 32, 33, 63, 64, 65, 200):
        assert plan.sub_runs(m) == max(1, 64 // m)
    for pairs in (RUN - 1, RUN, RUN + 1, 2 * RUN + 1):
        pairs_case(kind, pairs, 5, 3, 3, 4, seed=pairs)
    Q = plan.sub_runs(3)                                   # m = 3: 21 sub-runs, 1 lane idle
    sub = -(-RUN // Q)
    assert Q * 3 < 64 and (Q - 1) * sub < RUN <= Q * sub   # the last sub-run is shorter
    for pairs in (1, sub - 1, sub, sub + 1, 2 * sub + 1, (Q - 1) * sub, (Q - 1) * sub + 1):
        pairs_case(kind, pairs, 5, 3, 0, 4, seed=pairs)
    Q = plan.sub_runs(5)                                   # m = 5: 12 sub-runs, 4 lanes idle
    sub = -(-RUN // Q)
    for pairs in (sub, sub + 1, (Q - 1) * sub + 1):
        pairs_case(kind, pairs, 7, 5, 2, 4, seed=pairs)
    sub = RUN // plan.sub_runs(16)                         # m = 16: 4 sub-runs, no lane idle
    for pairs in (sub - 1, sub, sub + 1):
        pairs_case(kind, pairs, 20, 16, 2, 4, seed=pairs)
    pairs_case(kind, RUN + 1, 40, 33, 2, 4, seed=33)       # m = 33: one sub-run, 31 lanes idle


@pytest.mark.parametrize("kind", ["exact", "real"])
@pytest.mark.parametrize("C", [3, 0])
def test_histogram_equals_the_tree_kernel(cuda, C, kind):
    """bag = null and every feature: cyc_dt_histogram_dev's bytes on the same
    slots.  d = 70 is one run chain per node in both kernels (a panel of 64
    lanes, no sub-runs), so real data agree by bytes too; at d = 5 the sub-runs
    are another order, and only exact data do."""
    RUN = RFPlan(5, C).runRows
    for d, n in ((70, 2 * RUN + 1), (5, RUN + 1)):
        if d == 5 and kind == "real":
            continue
        rng = np.random.default_rng(d + C)
        image = rng.integers(0, 8, size=(n, d)).astype(np.uint8)
        y, w = labels_weights(kind, n, C, rng)
        slot = rng.choice(np.array([0, 0, 0, 2, 1, -1], dtype=np.int32), size=n)
        nodeOf = np.array([0, -1, 1], dtype=np.int32)
        args = dev(image), dev(y), dev(w)
        ref = DTPlan(d, C).histogram(*args, dev(slot), nodeOf, 2, 8).cpu().numpy()
        got = twice(lambda: (RFPlan(d, C).histogram(
            *args, None, dev(slot.reshape(1, n)), 0, 1, np.array([0, 3], dtype=np.int32), nodeOf,
            2, d, None, 8).cpu().numpy(),))[0]
        assert got.tobytes() == ref.tobytes()


# ----------------------------------------------------------------------- route
def test_route(cuda):
    rng = np.random.default_rng(1)
    n, d, nt = 2049, 9, 3
    image = rng.integers(0, 12, size=(n, d)).astype(np.uint8)
    slot = rng.choice(np.array([0, 1, 2, 3, -1, 7], dtype=np.int32), size=(nt, n))
    tables = [np.array([[4, 5, 0, 1], [-1, -1, -1, -1], [0, 0, -1, 2], [8, 10, 3, -1]]),
              np.zeros((0, 4)),                            # a tree with nothing left to split
              np.array([[4, 5, 1, 0], [2, 3, 2, 3]])]
    slotStart = np.array([0, 4, 4, 6], dtype=np.int32)
    table = np.concatenate(tables).astype(np.int32)
    image[:40, 4] = 5                                     # the threshold's own bin
    ref = np.empty((nt, n), dtype=np.int32)
    for t in range(nt):
        tb = tables[t]
        for r in range(n):
            s = int(slot[t, r])
            if not 0 <= s < len(tb) or tb[s, 0] < 0:
                ref[t, r] = -1
            else:
                ref[t, r] = tb[s, 2] if image[r, int(tb[s, 0])] <= tb[s, 1] else tb[s, 3]
    plan = RFPlan(d, 2)
    imd = dev(image)

    def run():
        sd = dev(slot)
        plan.route(imd, sd, slotStart, table)
        return (sd.cpu().numpy(),)
    (got,) = twice(run)
    assert np.array_equal(got, ref)
    at = np.nonzero(slot[0, :40] == 0)[0]
    assert at.size and np.all(got[0, at] == 0) and np.all(got[1] == -1)
    assert np.all(got[2, np.nonzero(slot[2, :40] == 0)[0]] == 1)
    ns = ForestNumpyStep(np.zeros((n, d)), np.zeros(n), None, 2)
    ns.bag(nt, None, 0)
    ns.image, ns.slot = image, slot.copy()
    ns.route(slotStart, table)
    assert np.array_equal(ns.slot, ref)


# --------------------------------------------------------------------- predict
def chain_tree(depth, d, C, rng):
    """A chain: every internal node's left child is a leaf, down to `depth`."""
    m = 2 * depth + 1
    feature, thr, first = np.full(m, -1), np.zeros(m), np.full(m, -1)
    node = 0
    for lvl in range(depth):
        feature[node], thr[node], first[node] = rng.integers(0, d), float(lvl - depth // 2), 2 * lvl + 1
        node = 2 * lvl + 2
    values = rng.integers(0, 9, size=(m, max(C, 1))) / 8.0
    return feature, thr, first, values


@pytest.mark.parametrize("C", [2, 17])
def test_predict(cuda, C):
    rng = np.random.default_rng(C)
    n, d = 1031, 5
    X = rng.integers(-8, 9, size=(n, d)).astype(np.float64)       # many rows on thresholds
    X[3, :], X[4, :], X[5, :] = np.inf, -np.inf, 100.0
    Xd = dev(X)
    ctrees, rtrees = [], []
    for depth in (3, 0, 9, 1, 30):                       # unequal depths, a one-node tree
        feature, thr, first, values = chain_tree(depth, d, C, rng)
        if depth in (3, 30):
            values[-1] = 0.0                              # the deepest leaf has total 0
        ctrees.append(DecisionTreeClassificationModel.from_arrays(feature, thr, first, values, d,
                                                                  numClasses=C))
        rtrees.append(DecisionTreeRegressionModel.from_arrays(
            feature, thr, first, values[:, 0] * 3.0 - 1.0, d))
    cm = RandomForestClassificationModel.from_trees(ctrees, d, C)
    rm = RandomForestRegressionModel.from_trees(rtrees, d)
    assert cm._plan is None and rm._plan is None and cm.getNumTrees == 5
    assert cm.totalNumNodes == sum(2 * k + 1 for k in (3, 0, 9, 1, 30))
    leaf, raw, prob, pred = twice(lambda: tuple(
        t.cpu().numpy() for t in (cm.predictLeaf(Xd), cm.predictRaw(Xd), cm.predictProbability(Xd),
                                  cm.predict(Xd))))
    rleaf, rpred = twice(lambda: (rm.predictLeaf(Xd).cpu().numpy(), rm.predict(Xd).cpu().numpy()))
    assert leaf.shape == (n, 5) and leaf.dtype == np.int32 and raw.shape == prob.shape == (n, C)
    croots, rroots = [t.rootNode for t in ctrees], [t.rootNode for t in rtrees]
    for r in range(n):
        want = [R.descend(root, X[r])[1] for root in croots]
        assert leaf[r].tolist() == want and rleaf[r].tolist() == want
        wraw, wprob, wpred = F.votes(croots, X[r], C)
        assert raw[r].tobytes() == np.array(wraw).tobytes()
        assert prob[r].tobytes() == np.array(wprob).tobytes()
        assert pred[r] == wpred
        assert np.float64(rpred[r]).tobytes() == np.float64(F.mean(rroots, X[r])).tobytes()
    assert leaf[5, 4] == 30 and leaf[5, 0] == 3           # down the whole chains, to the empty leaves
    # a forest of empty leaves only: raw 0, probability left as it is
    empty = DecisionTreeClassificationModel.from_arrays([-1], [0.0], [-1], np.zeros((1, C)), d,
                                                        numClasses=C)
    em = RandomForestClassificationModel.from_trees([empty, empty], d, C)
    assert np.all(em.predictProbability(Xd).cpu().numpy() == 0.0)
    assert np.all(em.predict(Xd).cpu().numpy() == 0.0)


# ------------------------------------------------------------------------- fit
same_node = F.same_node


@pytest.fixture(scope="module")
def exact_fit_rows(cuda):
    # n = 2 RUN + 1, the run length from a plan; computed once, shared and left unchanged
    return R.exact_rows(2 * RFPlan(20, 0).runRows + 1, 20, seed=21)


@pytest.mark.parametrize("impurity", ["gini", "variance"])
def test_device_fit_equals_numpy_fit(cuda, exact_fit_rows, impurity):
    X, ycls, yreg, w = exact_fit_rows
    n, d = X.shape
    C = 0 if impurity == "variance" else 3
    y = yreg if impurity == "variance" else ycls
    kw = dict(numTrees=5, featureSubsetStrategy="sqrt", maxDepth=4, impurity=impurity, seed=5)
    est = RandomForestClassifier(numClasses=3, **kw) if C else RandomForestRegressor(**kw)
    extra = (C,) if C else ()
    assert est.numFeaturesPerNode(d) == 5
    host = est.fit_step(ForestNumpyStep(X, y, w, C), d, *extra)
    fits = [est.fit(dev(X), dev(y), dev(w)) for _ in range(2)]
    # a workspace of one run per launch and one node per call: the same forest
    fits.append(est.fit_step(ForestDeviceStep(dev(X), dev(y), dev(w), C, workspaceBytes=1), d,
                             *extra, nodesPerCall=1))
    assert host.totalNumNodes >= 5 * 9
    for m in fits:
        assert m.getNumTrees == 5
        for a, b in zip(m.trees, host.trees):
            assert same_node(a.rootNode, b.rootNode)
        assert m.featureImportances.tobytes() == host.featureImportances.tobytes()
    # the model's own predictions on some training rows
    Xd = dev(X)
    pred, leaf = fits[0].predict(Xd).cpu().numpy(), fits[0].predictLeaf(Xd).cpu().numpy()
    roots = [t.rootNode for t in host.trees]
    for r in range(0, n, 173):
        assert leaf[r].tolist() == [R.descend(root, X[r])[1] for root in roots]
        want = F.votes(roots, X[r], C)[2] if C else F.mean(roots, X[r])
        assert np.float64(pred[r]).tobytes() == np.float64(want).tobytes()


@pytest.mark.parametrize("impurity", ["entropy", "variance"])
def test_one_tree_forest_is_the_device_tree(cuda, impurity):
    X, ycls, yreg, w = R.exact_rows(2049, 17, seed=9)
    kw = dict(maxDepth=5, impurity=impurity, minInstancesPerNode=2)
    fkw = dict(numTrees=1, featureSubsetStrategy="all", bootstrap=False, subsamplingRate=1.0, **kw)
    if impurity == "variance":
        from cycloneml_amd.tree import DecisionTreeRegressor
        tree = DecisionTreeRegressor(**kw).fit(dev(X), dev(yreg), dev(w))
        forest = RandomForestRegressor(**fkw).fit(dev(X), dev(yreg), dev(w))
    else:
        tree = DecisionTreeClassifier(**kw).fit(dev(X), dev(ycls), dev(w))
        forest = RandomForestClassifier(**fkw).fit(dev(X), dev(ycls), dev(w))
        assert forest.numClasses == tree.numClasses == 3
    assert tree.numNodes >= 9 and forest.trees[0].toDebugString() == tree.toDebugString()
    assert same_node(forest.trees[0].rootNode, tree.rootNode)


# -------------------------------------------------------------------- refusals
def test_refusals_before_any_launch(cuda):
    from cycloneml_amd.linalg import CSRRows
    csr = CSRRows.__new__(CSRRows)
    y = dev(np.zeros(4))
    for est in (RandomForestClassifier(), RandomForestRegressor()):
        with pytest.raises(N.IllegalArgumentException, match="CSR"):
            est.fit(csr, y)
    model = RandomForestRegressionModel.from_trees(
        [DecisionTreeRegressionModel.from_arrays([-1], [0.0], [-1], [1.0], 3)], 3)
    with pytest.raises(N.IllegalArgumentException, match="CSR"):
        model.predict(csr)
    n, d = 64, 6
    plan = RFPlan(d, 2)
    image, yv = dev(np.zeros((n, d), dtype=np.uint8)), dev(np.zeros(n))
    slot = dev(np.zeros((2, n), dtype=np.int32))
    ss, nodeOf = np.array([0, 1, 2], dtype=np.int32), np.array([0, 1], dtype=np.int32)

    def call(t0=0, t1=2, ss=ss, nodeOf=nodeOf, K=2, m=2, feats=((0, 5), (1, 2)), image=image,
             yv=yv, slot=slot):
        return plan.histogram_call(image, yv, None, None, slot, t0, t1, ss, nodeOf, K, m,
                                   None if feats is None else np.array(feats), 4)
    assert call().shape == (2, 2, 4, 3)
    for feats in (((0, 6), (1, 2)), ((0, 5), (-1, 2))):
        with pytest.raises(N.IllegalArgumentException, match="nodeFeat"):
            call(feats=feats)
    with pytest.raises(N.IllegalArgumentException, match="nodeFeat"):
        call(feats=None)                                  # null lists need m = d
    with pytest.raises(N.IllegalArgumentException, match="4096 nodes"):
        call(K=4097, feats=None, m=d)
    with pytest.raises(N.IllegalArgumentException, match="two trees"):
        call(nodeOf=np.array([0, 0], dtype=np.int32))
    with pytest.raises(N.IllegalArgumentException, match="node of slot"):
        call(nodeOf=np.array([0, 2], dtype=np.int32))
    # (t1 - t0) n above int32: refused by its arithmetic, whatever the arrays hold
    lib = N.load()
    rc = lib.cyc_rf_histogram_dev(plan.handle, N.ptr(image), N.ptr(yv), None, None, 2 ** 30,
                                  N.ptr(slot), 0, 2, ss.ctypes.data, nodeOf.ctypes.data, 2, d,
                                  None, 4, N.ptr(yv), None)
    assert rc == N.CYC_ERR_INVALID_ARG and b"2147483647" in lib.cyc_last_error()
    with pytest.raises(N.IllegalArgumentException):
        plan.bag(8, 0, RF.poisson_table(1.0), 0)
    with pytest.raises(N.IllegalArgumentException, match="ascending"):
        plan.bag(8, 1, np.array([5, 3], dtype=np.uint64), 0)
    with pytest.raises(N.IllegalArgumentException, match="slot entry 1"):
        plan.route(image, slot, ss, np.array([[0, 0, -1, -1], [d, 0, -1, -1]], dtype=np.int32))
