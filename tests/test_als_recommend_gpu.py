"""ALS top-N on the device (csrc/als_recommend.hip) against the numpy
restatement of tests/als_recommend_restatement.py.

Every comparison is exact: np.array_equal on the ids, tobytes() on the scores
(the padding and a NaN score are the canonical NaN on both sides).  Every
device call runs twice and the two results are compared by bytes.  The edge
shapes come from the library's own queries: T the source tile, Dt the
destination tile of a rank, the split count and span of a shape, the cap on
num and the greatest num whose lists stay in LDS.
"""
import functools

import numpy as np
import pytest

import als_recommend_restatement as R
from cycloneml_amd import _native as N
from cycloneml_amd.recommendation import ALS, ALSModel, ALSPlan

pytestmark = pytest.mark.gpu

RANKS = [1, 3, 10, 15, 16, 17, 32, 33, 64]
T = ALSPlan(10).recommend_src_tile()
CAP = ALSPlan(10).recommend_max_num()
LDS_NUM = ALSPlan(10).recommend_lds_num()
NUM = 10


def dev():
    import torch
    return torch.device("cuda:0")


def to_dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.array(a)).to(dev())


def first_ndst_with_splits(m, want):
    plan = ALSPlan(10)
    n = 1
    while plan.recommend_splits(m, n) < want:
        n += 1
    return n


@functools.lru_cache(maxsize=None)
def factors(n, rank, seed):
    a = np.random.default_rng(seed).standard_normal((n, rank)).astype(np.float32)
    a.setflags(write=False)
    return a


def device_twice(rank, S, sp, D, dp, num, srcIds=None):
    plan = ALSPlan(rank)
    args = (to_dev(S), to_dev(sp), to_dev(D), to_dev(dp), num, to_dev(srcIds))
    a = [t.cpu().numpy() for t in plan.recommend(*args)]
    b = [t.cpu().numpy() for t in plan.recommend(*args)]
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), "two calls differ"
    assert a[0].dtype == np.int32 and a[1].dtype == np.float32
    return a


def check(rank, S, sp, D, dp, num, srcIds=None):
    ids, scores = device_twice(rank, S, sp, D, dp, num, srcIds)
    want_ids, want_scores = R.recommend(S, sp, D, dp, num, srcIds)
    assert ids.shape == want_ids.shape
    assert np.array_equal(ids, want_ids)
    assert scores.tobytes() == want_scores.tobytes()
    return ids, scores


def masks(ns, nd, seed):
    rng = np.random.default_rng(seed)
    sp = (rng.random(ns) < 0.9).astype(np.uint8)
    dp = (rng.random(nd) < 0.8).astype(np.uint8)
    return sp, dp


@pytest.mark.parametrize("rank", RANKS)
def test_rank_edges(cuda, rank):
    """70 x 300: two splits, and more than one tile in the first at every rank."""
    m, ndst = 70, 300
    plan = ALSPlan(rank)
    assert plan.recommend_splits(m, ndst) == 2
    assert plan.recommend_dst_tile() < plan.recommend_span(m, ndst)
    sp, dp = masks(m, ndst, rank)
    check(rank, factors(m, rank, 1), sp, factors(ndst, rank, 2), dp, NUM)


@pytest.mark.parametrize("rank", [10, 17])
@pytest.mark.parametrize("m", [1, T - 1, T, T + 1, 2 * T + 1])
def test_source_row_edges(cuda, rank, m):
    ndst = 150
    sp, dp = masks(m, ndst, m)
    sp[[0, m - 1]] = 1
    check(rank, factors(m, rank, 3), sp, factors(ndst, rank, 4), dp, NUM)


def ndst_edges(m):
    dt = ALSPlan(10).recommend_dst_tile()
    two, three = first_ndst_with_splits(m, 2), first_ndst_with_splits(m, 3)
    return sorted({1, NUM - 1, NUM, NUM + 1, dt - 1, dt, dt + 1, two - 1, two, two + 1,
                   three - 1, three, three + 1})


@pytest.mark.parametrize("m", [1, T + 1])
def test_destination_edges(cuda, m):
    rank = 10
    plan = ALSPlan(rank)
    edges = ndst_edges(m)
    assert plan.recommend_splits(m, edges[-1]) == 3 and plan.recommend_splits(m, edges[-4]) == 2
    for ndst in edges:
        check(rank, factors(m, rank, 5), None, factors(ndst, rank, 6 + ndst), None, NUM)


@pytest.mark.parametrize("num", [1, NUM, LDS_NUM, LDS_NUM + 1, CAP])
def test_num_values(cuda, num):
    rank, m, ndst = 10, T + 3, 600
    sp, dp = masks(m, ndst, num)
    check(rank, factors(m, rank, 7), sp, factors(ndst, rank, 8), dp, num)


@pytest.mark.parametrize("num", [NUM, LDS_NUM + 1, CAP])
def test_num_above_the_destinations(cuda, num):
    rank, m, ndst = 10, 5, 7
    dp = np.array([1, 1, 0, 1, 1, 1, 1], dtype=np.uint8)
    ids, scores = check(rank, factors(m, rank, 9), None, factors(ndst, rank, 10), dp, num)
    assert np.all(ids[:, 6:] == -1) and np.all(ids[:, :6] >= 0) and np.isnan(scores[:, 6:]).all()


@pytest.mark.parametrize("rank", [3, 10, 64])
def test_scores_are_predicts_bits(cuda, rank):
    nu, ni = 90, 310
    U, V = factors(nu, rank, 11), factors(ni, rank, 12)
    up, vp = masks(nu, ni, 13)
    model = ALSModel(rank, to_dev(U), to_dev(V), to_dev(up), to_dev(vp))
    for forUsers in (True, False):
        rec = model.recommendForAllUsers if forUsers else model.recommendForAllItems
        src, ids, scores = rec(7)
        src2, ids2, scores2 = rec(7, blockSize=17)
        for a, b in ((src, src2), (ids, ids2), (scores, scores2)):
            assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
        pairs_src = src.view(-1, 1).expand(-1, ids.shape[1]).contiguous().view(-1)
        pairs_dst = ids.contiguous().view(-1)
        users, items = (pairs_src, pairs_dst) if forUsers else (pairs_dst, pairs_src)
        p = model.predict(users, items).cpu().numpy()
        assert not np.isnan(p).any()
        assert p.tobytes() == scores.cpu().numpy().tobytes()
        assert np.array_equal(src.cpu().numpy(), np.nonzero(up if forUsers else vp)[0])


def test_ties_small_integer_factors(cuda):
    """Factors k / 8 with k in -2 .. 2: a handful of distinct scores, so nearly
    every position of every list is decided by the id."""
    rank, m, ndst = 3, T + 5, 700
    rng = np.random.default_rng(14)
    S = (rng.integers(-2, 3, (m, rank)) / 8.0).astype(np.float32)
    D = (rng.integers(-2, 3, (ndst, rank)) / 8.0).astype(np.float32)
    sp, dp = masks(m, ndst, 15)
    ids, scores = check(rank, S, sp, D, dp, NUM)
    assert len(np.unique(scores[sp != 0])) < 30


def test_ties_across_tile_and_split_boundaries(cuda):
    """The best destination row copied to both sides of the first tile
    boundary and of the first split boundary: the lower id leads every time."""
    rank, m = 10, 9
    plan = ALSPlan(rank)
    ndst = first_ndst_with_splits(m, 3)
    dt, span = plan.recommend_dst_tile(), plan.recommend_span(m, ndst)
    assert dt < span < ndst
    D = np.array(factors(ndst, rank, 16)) * np.float32(0.01)
    S = np.array(factors(m, rank, 17))
    big = S[0] * np.float32(4.0)                  # row 0 scores it far above the rest
    where = [dt - 1, dt, span - 1, span, ndst - 1]
    D[where] = big
    ids, scores = check(rank, S, None, D, None, NUM)
    assert ids[0, :5].tolist() == where and len(set(scores[0, :5].tolist())) == 1


def test_all_zero_factors(cuda):
    rank, m, ndst = 10, 3, 600
    dp = np.ones(ndst, dtype=np.uint8)
    dp[[0, 2, 5]] = 0
    ids, scores = check(rank, np.zeros((m, rank), np.float32), None,
                        np.zeros((ndst, rank), np.float32), dp, NUM)
    assert ids[0].tolist() == [1, 3, 4, 6, 7, 8, 9, 10, 11, 12]
    assert np.all(scores.view(np.uint32) == 0)       # +0.0, never -0.0


@pytest.mark.parametrize("num", [NUM, LDS_NUM + 4])
@pytest.mark.parametrize("ascending", [True, False])
def test_insert_path(cuda, ascending, num):
    """Scores that rise with the id: every destination enters every list.
    Falling: none does after the first num of a split."""
    rank, m, ndst = 3, 70, 600
    S = np.zeros((m, rank), dtype=np.float32)
    S[:, 0] = 1.0 + (np.arange(m) % 3)
    D = np.zeros((ndst, rank), dtype=np.float32)
    D[:, 0] = 0.5 * (np.arange(ndst) if ascending else np.arange(ndst)[::-1])
    ids, _ = check(rank, S, None, D, None, num)
    want = np.arange(ndst)[::-1][:num] if ascending else np.arange(num)
    assert ids[0].tolist() == want.tolist()


def test_presence(cuda):
    rank, m, ndst = 10, T + 9, 300
    S, D = factors(m, rank, 18), factors(ndst, rank, 19)
    rng = np.random.default_rng(20)
    sp = (rng.random(m) < 0.5).astype(np.uint8)
    dp = (rng.random(ndst) < 0.5).astype(np.uint8)
    ids, _ = check(rank, S, sp, D, dp, NUM)                 # scattered
    assert np.all(ids[sp == 0] == -1) and np.all(dp[ids[sp != 0]] == 1)
    few = np.zeros(ndst, dtype=np.uint8)
    few[[3, 150, 151, 299]] = 1                             # fewer than num, in both splits
    ids, _ = check(rank, S, sp, D, few, NUM)
    assert np.all(np.sort(ids[sp != 0][:, :4], axis=1) == [3, 150, 151, 299])
    ids, scores = check(rank, S, sp, D, np.zeros(ndst, dtype=np.uint8), NUM)     # none
    assert np.all(ids == -1) and np.isnan(scores).all()
    check(rank, S, None, D, dp, NUM)                        # a NULL mask on either side
    check(rank, S, sp, D, None, NUM)
    check(rank, S, None, D, None, NUM)


def test_subset_at_c_level(cuda):
    """srcIds unordered, with repeats, negative and past-the-end ids: those rows
    are -1 / NaN and every other row is the full call's row of that id."""
    rank, ns, ndst = 10, 40, 300
    S, D = factors(ns, rank, 21), factors(ndst, rank, 22)
    sp, dp = masks(ns, ndst, 23)
    sp[[4, 6]] = [0, 1]
    full_ids, full_scores = check(rank, S, sp, D, dp, NUM)
    src = np.array([17, 6, -1, 6, ns, 0, 4, 39, -2 ** 31, 2 ** 31 - 1, 17], dtype=np.int32)
    ids, scores = check(rank, S, sp, D, dp, NUM, src)
    for r, u in enumerate(src):
        if 0 <= u < ns:
            assert np.array_equal(ids[r], full_ids[u])
            assert scores[r].tobytes() == full_scores[u].tobytes()
        else:
            assert np.all(ids[r] == -1) and np.isnan(scores[r]).all()
    assert np.all(ids[6] == -1)                            # id 4 is absent
    # an empty request is an empty answer
    ids, scores = device_twice(rank, S, sp, D, dp, NUM, np.zeros(0, dtype=np.int32))
    assert ids.shape == (0, NUM) and scores.shape == (0, NUM)


def test_subset_in_python(cuda):
    rank, nu, ni = 10, 50, 80
    U, V = np.array(factors(nu, rank, 24)), np.array(factors(ni, rank, 25))
    up, vp = masks(nu, ni, 26)
    up[[3, 7, 20]] = [1, 0, 1]
    vp[[5, 9]] = [1, 0]
    vp[30:] = 0                                            # 2 <= present items < 30
    model = ALSModel(rank, U, V, up, vp)                   # host arrays: uploaded by the call
    want_ids, want_scores = R.recommend(U, up, V, vp, 40)
    keep = min(40, int(vp.sum()))
    src, ids, scores = model.recommendForUserSubset([20, 3, 7, 3, -5, nu, 20], 40)
    assert src.cpu().numpy().tolist() == [3, 20] and src.dtype.is_floating_point is False
    assert ids.shape == (2, keep) and scores.shape == (2, keep)
    assert np.array_equal(ids.cpu().numpy(), want_ids[[3, 20], :keep])
    assert scores.cpu().numpy().tobytes() == want_scores[[3, 20], :keep].tobytes()
    assert not np.isnan(scores.cpu().numpy()).any()
    want_ids, want_scores = R.recommend(V, vp, U, up, 3)
    src, ids, scores = model.recommendForItemSubset(to_dev(np.array([9, 5, 5])), 3)
    assert src.cpu().numpy().tolist() == [5]
    assert np.array_equal(ids.cpu().numpy(), want_ids[[5]])
    assert scores.cpu().numpy().tobytes() == want_scores[[5]].tobytes()
    src, ids, scores = model.recommendForItemSubset([9, ni + 3], 3)
    assert src.numel() == 0 and ids.shape == (0, 3) and scores.shape == (0, 3)


def test_refusals(cuda):
    import torch
    rank = 10
    S, D = to_dev(factors(6, rank, 27)), to_dev(factors(9, rank, 28))
    plan = ALSPlan(rank)
    for num in (0, CAP + 1):
        with pytest.raises(N.IllegalArgumentException,
                           match="requirement failed: the number of recommendations"):
            plan.recommend(S, None, D, None, num)
    with pytest.raises(N.IllegalArgumentException, match="the destination mask must be 9"):
        plan.recommend(S, None, D, torch.ones(8, dtype=torch.uint8, device=dev()), 3)
    with pytest.raises(N.IllegalArgumentException, match="srcIds must be"):
        plan.recommend(S, None, D, None, 3, torch.zeros(2, dtype=torch.int64, device=dev()))
    lib = N.load()
    ids = torch.full((6, 3), 77, dtype=torch.int32, device=dev())
    scores = torch.full((6, 3), 77.0, dtype=torch.float32, device=dev())
    need = plan.recommend_workspace(6, 9, 3)
    ws = torch.empty(need // 8, dtype=torch.int64, device=dev())

    def call(rank=rank, num=3, nbytes=need):
        return lib.cyc_als_recommend_dev(N.ptr(S), None, 6, None, 6, N.ptr(D), None, 9, rank, num,
                                         N.ptr(ids), N.ptr(scores), N.ptr(ws), nbytes,
                                         N.stream_handle())
    for kw, match in [(dict(rank=0), "ALS supports rank 1 to 64 but got 0"),
                      (dict(rank=65), "ALS supports rank 1 to 64 but got 65"),
                      (dict(num=0), "recommendations must be in .* but got 0"),
                      (dict(num=CAP + 1), f"recommendations must be in .* but got {CAP + 1}"),
                      (dict(nbytes=need - 8), f"the workspace must hold {need} bytes")]:
        with pytest.raises(N.IllegalArgumentException, match="requirement failed: .*" + match):
            N.check(call(**kw))
    torch.cuda.synchronize()
    assert torch.all(ids == 77) and torch.all(scores == 77.0)      # nothing was launched
    N.check(call())
    assert torch.all(ids >= 0)


def test_small_fit(cuda):
    """60 x 45 ids, rank 5 (user 13 and item 7 have no ratings): both
    directions against the restatement applied to the model's own factors."""
    rng = np.random.default_rng(2024)
    nu, ni, n, rank = 60, 45, 1200, 5
    users = rng.integers(0, nu, n).astype(np.int32)
    items = rng.integers(0, ni, n).astype(np.int32)
    users[users == 13] = 14
    items[items == 7] = 8
    ratings = rng.uniform(0.5, 5.0, n).astype(np.float32)
    model = ALS(rank=rank, maxIter=3, regParam=0.1, seed=1).fit(to_dev(users), to_dev(items),
                                                               to_dev(ratings))
    U, V = model.userFactors.cpu().numpy(), model.itemFactors.cpu().numpy()
    up, vp = model.userPresent.cpu().numpy(), model.itemPresent.cpu().numpy()
    assert not up[13] and not vp[7]
    for rec, (S, sp, D, dp) in ((model.recommendForAllUsers, (U, up, V, vp)),
                                (model.recommendForAllItems, (V, vp, U, up))):
        a, b = rec(NUM), rec(NUM)
        for x, y in zip(a, b):
            assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
        src, ids, scores = (t.cpu().numpy() for t in a)
        want_ids, want_scores = R.recommend(S, sp, D, dp, NUM)
        present = np.nonzero(sp)[0]
        assert np.array_equal(src, present) and src.dtype == np.int32
        assert np.array_equal(ids, want_ids[present])
        assert scores.tobytes() == want_scores[present].tobytes()
        assert np.all(ids >= 0) and np.all(dp[ids] == 1)
