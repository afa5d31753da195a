"""BisectingKMeans on the device (csrc/bisecting_kmeans.hip) against the
row-by-row restatement of tests/bisecting_kmeans_restatement.py.

  step     newSlot equals the restatement's findClosest pick for every row and
           count is equal; on exact rows (integers below 2^20, weights in
           eighths) sum and wsum are equal by bytes; sumSq, and everything on
           real rows, within 1e-10 of the sum of the absolute terms (rounding
           is below n 2^-53 of that sum)
  predict  leaf index and cost equal the restatement's descent bit for bit
  fit      exact rows: centers and sizes by bytes, costs within 1e-10 relative
Every device call runs twice and the two results are compared by tobytes().
"""
import numpy as np
import pytest
import torch

import bisecting_kmeans_restatement as R
import oracle
from cycloneml_amd import _native as N
from cycloneml_amd import bisecting_kmeans as bk
from cycloneml_amd.bisecting_kmeans import BisectingKMeans, BisectingKMeansModel, BKMPlan

pytestmark = pytest.mark.gpu

DIMS = [1, 3, 4, 17, 64, 65, 256, 257]
ROWS = [1, 63, 64, 65, 255, 256, 257, 1000, 2049]


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def twice(fn):
    a, b = fn(), fn()
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes(), "two calls differ"
    return a


def rows_of(kind, n, d, seed):
    if kind == "exact":
        return R.exact_rows(n, d, seed=seed)
    rng = np.random.default_rng(seed)
    return rng.normal(size=(n, d)) * 3.0 + rng.integers(0, 4, size=(n, 1)), \
        rng.uniform(0.25, 4.0, size=n)


def mixed_case(kind, n, d, seed):
    """Slots 0 and 3 divide (children 0, 1 and 3, 4), 1 and 4 are parked
    between them, 2 has only a right child (2), 5 only a left one (5).  Slot
    0's children are base -+ delta: its rows put at base are equidistant (exact
    rows) and go left; a row put on the left child itself has distance 0, so
    the bound skips the right child."""
    X, w = rows_of(kind, n, d, seed)
    rng = np.random.default_rng(seed + 1)
    slot = (np.arange(n) % 6).astype(np.int32)
    K = 6
    table = np.array([[0, 1, -1], [-1, -1, K + 1], [-1, 2, -1], [3, 4, -1], [-1, -1, K],
                      [5, -1, -1]], dtype=np.int32)
    C = X[rng.integers(0, n, size=K)] + (rng.integers(-8, 9, size=(K, d)) if kind == "exact"
                                         else rng.normal(size=(K, d)))
    base = X[0].copy()
    delta = rng.integers(1, 9, size=d).astype(np.float64)
    C[0], C[1] = base - delta, base + delta
    zero = np.nonzero(slot == 0)[0]
    for q, r in enumerate(zero[:8]):
        X[r] = base if q % 2 == 0 else C[0]
    return X, w, slot, table, np.ascontiguousarray(C)


def one_slot_case(kind, n, d, seed):
    X, w = rows_of(kind, n, d, seed)
    rng = np.random.default_rng(seed + 2)
    C = X[rng.integers(0, n, size=2)] + (rng.integers(-8, 9, size=(2, d)) if kind == "exact"
                                         else rng.normal(size=(2, d)))
    return X, w, None, np.array([[0, 1, -1]], dtype=np.int32), np.ascontiguousarray(C)


def run_step(plan, X, w, slot, table, C, norms, cn):
    n, d, K = X.shape[0], X.shape[1], C.shape[0]
    Xd, wd, sd, Cd, nd, cnd = dev(X), dev(w), dev(slot), dev(C), dev(norms), dev(cn)

    def run():
        new = torch.full((n,), -7, dtype=torch.int32, device="cuda:0")
        count = torch.zeros(K, dtype=torch.int64, device="cuda:0")
        sums = torch.zeros(bk.sums_length(K, d), dtype=torch.float64, device="cuda:0")
        plan.step(Xd, nd, wd, sd, table, Cd, cnd, new, count, sums)
        return new.cpu().numpy(), count.cpu().numpy(), sums.cpu().numpy()
    return twice(run)


def check_step(plan, kind, case):
    X, w, slot, table, C = case
    n, d = X.shape
    K = C.shape[0]
    norms, cn = oracle.row_norms(X), oracle.row_norms(C)
    new, count, sums = run_step(plan, X, w, slot, table, C, norms, cn)
    ref = R.step(X, norms, np.zeros(n, dtype=np.int32) if slot is None else slot, table, C, cn)
    assert np.array_equal(new, ref)
    rcount, rbuf, bar = R.step_summary(X, norms, w, ref, K)
    assert np.array_equal(count, rcount)
    if kind == "exact":
        assert sums[:K].tobytes() == rbuf[:K].tobytes()
        assert sums[2 * K:].tobytes() == rbuf[2 * K:].tobytes()
    err = np.abs(sums - rbuf)
    print(f"{kind} n={n} d={d} K={K}: worst error / bar = "
          f"{float(np.max(err / np.maximum(bar, 1e-300))):.3e}")
    assert np.all(err <= 1e-10 * bar)
    return new, ref


@pytest.mark.parametrize("kind", ["exact", "real"])
@pytest.mark.parametrize("d", DIMS)
def test_step_conformance(cuda, d, kind):
    plan = BKMPlan(d)
    for n in ROWS:
        new, _ = check_step(plan, kind, mixed_case(kind, n, d, seed=n + d))
        check_step(plan, kind, one_slot_case(kind, n, d, seed=n + d))
        if kind == "exact" and n >= 63:
            X, w, slot, table, C = mixed_case(kind, n, d, seed=n + d)
            zero = np.nonzero(slot == 0)[0][:8]
            assert np.all(new[zero] == 0)      # the ties and the skipped bound: left


def test_step_without_summary_and_in_place(cuda):
    X, w, slot, table, C = mixed_case("real", 1000, 17, seed=5)
    norms, cn = oracle.row_norms(X), oracle.row_norms(C)
    plan = BKMPlan(17)
    ref = R.step(X, norms, slot, table, C, cn)

    def run():
        s = dev(slot)
        plan.step(dev(X), dev(norms), dev(w), s, table, dev(C), dev(cn), s)
        return (s.cpu().numpy(),)
    assert np.array_equal(twice(run)[0], ref)


@pytest.mark.parametrize("kind", ["exact", "real"])
def test_small_workspace_same_bytes(cuda, kind):
    n, d = 2049, 65
    X, w, slot, table, C = mixed_case(kind, n, d, seed=3)
    norms, cn = oracle.row_norms(X), oracle.row_norms(C)
    big, small = BKMPlan(d), BKMPlan(d, workspaceBytes=1)
    assert small.chunksPerLaunch == 1 and big.chunksPerLaunch > n
    a = run_step(big, X, w, slot, table, C, norms, cn)
    b = run_step(small, X, w, slot, table, C, norms, cn)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


def test_plan_constants_and_refusals(cuda):
    plan = BKMPlan(5)
    assert (plan.tileRows, plan.panelCols, plan.chunkRows) == (256, 16, 256)
    assert plan.chunksPerLaunch == (256 << 20) // (8 * 7)
    X, w, slot, table, C = mixed_case("exact", 64, 5, seed=1)
    norms, cn = oracle.row_norms(X), oracle.row_norms(C)
    new = torch.empty(64, dtype=torch.int32, device="cuda:0")
    for bad in ([[0, 9, -1]], [[-1, -1, -1]], [[0, 1, 2]]):
        with pytest.raises(N.IllegalArgumentException):
            plan.step(dev(X), dev(norms), None, None, bad, dev(C), dev(cn), new)
    # a slot outside the table is never an index: the call names the row
    slot[40] = 6
    slot[50] = -1
    with pytest.raises(N.IllegalArgumentException, match=r"\(row 40\)"):
        plan.step(dev(X), dev(norms), None, dev(slot), table, dev(C), dev(cn), new)
    assert (plan.badRow, plan.badRule) == (40, bk.RULE_SLOT)


TREES = {
    "leaf": ([-1], [0]),
    "depth1": ([1, -1, -1], [2, 0, 0]),
    # unbalanced, one-child nodes at 2, 6 and 10: 0 > 2 > 3 > 5 > 6 > 8 > 10 > 11
    "deep": ([1, -1, 3, 4, -1, 6, 8, -1, 9, -1, 11, -1], [2, 0, 1, 2, 0, 2, 1, 0, 2, 0, 1, 0]),
}


def flat_leaf_index(first, num):
    """Leaf indices in build_tree's depth-first order."""
    leaf, nxt = [-1] * len(num), [0]

    def visit(i):
        if num[i] == 0:
            leaf[i] = nxt[0]
            nxt[0] += 1
        for q in range(num[i]):
            visit(first[i] + q)
    visit(0)
    return leaf


@pytest.mark.parametrize("d", [1, 17, 256, 257])
@pytest.mark.parametrize("tree", sorted(TREES))
def test_predict_equals_descent(cuda, tree, d):
    first, num = TREES[tree]
    rng = np.random.default_rng(d + len(num))
    n = 777
    centers = rng.normal(size=(len(num), d)) * 2.0
    X = centers[rng.integers(0, len(num), size=n)] + rng.normal(size=(n, d))
    X[:5] = centers[0]
    if tree == "depth1":
        centers[2] = centers[1]            # a tie at the root goes to the first child
    root = R.tree_from_arrays(centers, first, num)
    ref = [R.predict(root, X[r]) for r in range(n)]
    plan = BKMPlan(d)
    Xd, Cd = dev(X), dev(centers)

    def run():
        p, c = plan.predict(Xd, first, num, flat_leaf_index(first, num), Cd)
        return p.cpu().numpy(), c.cpu().numpy()
    pred, cost = twice(run)
    assert np.array_equal(pred, np.array([p for p, _ in ref], dtype=np.int32))
    assert cost.tobytes() == np.array([c for _, c in ref]).tobytes()
    model = BisectingKMeansModel.from_arrays(centers, first, num)
    assert np.array_equal(model.predict(Xd).cpu().numpy(), pred)
    total = 0.0
    for _, c in ref:
        total = total + c
    assert abs(model.computeCost(Xd) - total) <= 1e-10 * total


def test_predict_refuses_a_bad_tree(cuda):
    plan = BKMPlan(3)
    X, C = dev(np.zeros((4, 3))), dev(np.zeros((3, 3)))
    for first, num, leaf in (([0, -1, -1], [2, 0, 0], [-1, 0, 1]),     # a child that is its parent
                             ([2, -1, -1], [2, 0, 0], [-1, 0, 1]),     # a child past the end
                             ([1, -1, -1], [3, 0, 0], [-1, 0, 1]),     # three children
                             ([1, -1, -1], [2, 0, 0], [-1, -1, 1])):   # a leaf without an index
        with pytest.raises(N.IllegalArgumentException):
            plan.predict(X, first, num, leaf, C)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("k", [2, 4, 7])
def test_fit_exact_rows(cuda, k, weighted):
    X, w = R.exact_rows(700, 5, seed=k, weighted=weighted)
    clusters, assign = R.fit(X, w, k, 20, 1.0, 11)
    root = R.build_tree(clusters)

    def run():
        m = BisectingKMeans(k=k, seed=11).fit(dev(X), dev(w))
        nodes = list(R.walk(m.root))
        return (m.clusterCenters, np.array([nd.size for nd in nodes]),
                np.array([nd.index for nd in nodes]), np.array([nd.cost for nd in nodes]),
                np.stack([nd.center for nd in nodes]), m.predict(dev(X)).cpu().numpy())
    centers, sizes, index, costs, allc, pred = twice(run)
    ref = list(R.walk(root))
    assert centers.tobytes() == np.stack([leaf.center for leaf in R.leaves(root)]).tobytes()
    assert allc.tobytes() == np.stack([nd.center for nd in ref]).tobytes()
    assert sizes.tolist() == [nd.size for nd in ref]
    assert index.tolist() == [nd.index for nd in ref]
    for got, nd in zip(costs, ref):
        print(f"k={k} node {nd.index}: cost {got!r} against {nd.cost!r}")
        assert abs(got - nd.cost) <= 1e-10 * nd.cost
    assert np.array_equal(pred, np.array([R.predict(root, x)[0] for x in X], dtype=np.int32))


def test_fit_finds_the_blobs(cuda):
    sizes = [150, 90, 200, 120]
    X, lab = R.real_rows(sizes, 8, seed=6)
    m = BisectingKMeans(k=4, seed=1).fit(dev(X))
    assert sorted(m.summary.clusterSizes) == sorted(sizes)
    pred = m.predict(dev(X)).cpu().numpy()
    for b in range(4):
        assert len(set(pred[lab == b].tolist())) == 1
    assert m.summary.trainingCost == m.trainingCost > 0.0


def test_fit_names_the_lowest_bad_row_and_weight(cuda):
    X, w = R.exact_rows(600, 4)
    bad = X.copy()
    bad[411, 1] = np.inf
    bad[300, 3] = np.nan
    with pytest.raises(N.IllegalArgumentException, match=r"\(row 300\)"):
        BisectingKMeans(k=2).fit(dev(bad), dev(w))
    for v in (0.0, -1.0, np.inf, np.nan):
        wb = w.copy()
        wb[512] = v
        wb[257] = v
        with pytest.raises(N.IllegalArgumentException, match=r"weight.*\(row 257\)"):
            BisectingKMeans(k=2).fit(dev(X), dev(wb))
    with pytest.raises(N.IllegalArgumentException):
        BisectingKMeans().fit(dev(X.astype(np.float32)))
