"""ALS top-N, host side (no device): the numpy restatement against hand-worked
cases, the Python argument checks, the subset reduction and the shape queries
of csrc/als_recommend.hip (pure functions of the library)."""
import numpy as np
import pytest

import als_recommend_restatement as R
import als_restatement as A
from cycloneml_amd import _native as N
from cycloneml_amd import recommendation as rec
from cycloneml_amd.recommendation import ALSModel, ALSPlan


def bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


def test_scores_are_the_sdot_chain():
    # 1 + 2^-24 rounds back to 1 twice, then - 1: the chain gives 0, any other
    # order or a fused multiply-add does not
    S = np.array([[1.0, 2.0 ** -24, 2.0 ** -24, -1.0], [0.1, 0.2, 0.3, 0.4]], dtype=np.float32)
    D = np.array([[1.0, 1.0, 1.0, 1.0], [0.7, -0.3, 0.9, 1.1]], dtype=np.float32)
    sc = R.scores(S, D)
    assert sc.dtype == np.float32 and sc[0, 0] == 0.0
    for u in range(2):
        for j in range(2):
            assert bits(sc[u, j]) == bits(A.sdot(S[u], D[j]))


def test_float_compare_order_by_hand():
    inf = np.float32(np.inf)
    neg_nan = np.array([0xffc00001], dtype=np.uint32).view(np.float32)[0]
    xs = np.array([-inf, -1.0, -0.0, 0.0, 1e-45, 1.0, inf, np.nan], dtype=np.float32)
    r = R.float_compare_rank(xs).astype(np.int64)
    assert np.all(np.diff(r) > 0)                     # strictly increasing, -0.0 < +0.0
    assert R.float_compare_rank([neg_nan])[0] == r[-1]    # every NaN is the one NaN


def test_top_ties_nan_absent_and_padding_by_hand():
    #            id 0    1    2    3     4     5    6
    sc = np.array([2.0, 5.0, 2.0, np.nan, -0.0, 0.0, 5.0], dtype=np.float32)
    present = np.array([1, 1, 1, 1, 1, 1, 0], dtype=np.uint8)      # id 6 absent
    ids, out = R.top(sc, present, 4)
    assert ids.tolist() == [3, 1, 0, 2]               # NaN first, then 5, then the tie by id
    assert np.isnan(out[0]) and out[1:].tolist() == [5.0, 2.0, 2.0]
    ids, out = R.top(sc, present, 8)                  # num above the candidate count
    assert ids.tolist() == [3, 1, 0, 2, 5, 4, -1, -1]  # +0.0 before -0.0
    assert bits(out[4]) == 0 and bits(out[5]) == 0x80000000
    assert bits(out[0]) == 0x7fc00000 and np.all(bits(out[6:]) == 0x7fc00000)
    ids, out = R.top(sc, np.zeros(7, dtype=np.uint8), 3)
    assert ids.tolist() == [-1, -1, -1] and np.isnan(out).all()


def test_recommend_rows_by_hand():
    S = np.array([[1.0, 0.0], [0.0, 1.0], [1.0, 1.0]], dtype=np.float32)
    D = np.array([[3.0, 1.0], [2.0, 2.0], [1.0, 3.0], [9.0, 9.0]], dtype=np.float32)
    sp = np.array([1, 0, 1], dtype=np.uint8)
    dp = np.array([1, 1, 1, 0], dtype=np.uint8)
    ids, out = R.recommend(S, sp, D, dp, 2)
    assert ids.tolist() == [[0, 1], [-1, -1], [0, 1]]      # row 2: 4, 4, 4 -> ids 0, 1
    assert out[0].tolist() == [3.0, 2.0] and np.isnan(out[1]).all()
    assert out[2].tolist() == [4.0, 4.0]
    # a subset: unordered, a repeat, a negative and a past-the-end id
    ids2, out2 = R.recommend(S, sp, D, dp, 2, srcIds=[2, -1, 0, 2, 3, 1])
    assert ids2.tolist() == [[0, 1], [-1, -1], [0, 1], [0, 1], [-1, -1], [-1, -1]]
    assert out2[3].tobytes() == out[2].tobytes()
    # masks given as None: everything present
    ids3, _ = R.recommend(S, None, D, None, 1)
    assert ids3.tolist() == [[3], [3], [3]]


def test_subset_ids_are_distinct_known_present_ascending():
    import torch
    present = np.array([1, 0, 1, 1, 0, 1], dtype=np.uint8)
    got = rec.subset_ids([5, 2, 2, -1, 9, 1, 0, 5, 6], present)
    assert got.dtype == torch.int32 and got.tolist() == [0, 2, 5]
    got = rec.subset_ids(torch.tensor([3, 3, 4], dtype=torch.int64), torch.from_numpy(present))
    assert got.tolist() == [3]
    assert rec.subset_ids([], present).tolist() == []
    assert rec.subset_ids(np.arange(6), present).tolist() == [0, 2, 3, 5]
    with pytest.raises(N.IllegalArgumentException, match="integers"):
        rec.subset_ids([0.5], present)


@pytest.mark.parametrize("num", [0, -3, rec.MAX_RECOMMEND + 1])
def test_model_refuses_num_before_any_device_work(num):
    m = ALSModel(2, np.zeros((4, 2), dtype=np.float32), np.zeros((3, 2), dtype=np.float32))
    for call in (lambda: m.recommendForAllUsers(num), lambda: m.recommendForAllItems(num),
                 lambda: m.recommendForUserSubset([0], num),
                 lambda: m.recommendForItemSubset([0], num)):
        with pytest.raises(N.IllegalArgumentException,
                           match="requirement failed: the number of recommendations"):
            call()


def test_model_refuses_block_size():
    m = ALSModel(2, np.zeros((4, 2), dtype=np.float32), np.zeros((3, 2), dtype=np.float32))
    with pytest.raises(N.IllegalArgumentException, match="blockSize"):
        m.recommendForAllUsers(3, blockSize=0)


def test_shape_queries():
    lib = N.load()
    plan = ALSPlan(10)
    T = plan.recommend_src_tile()
    assert T == lib.cyc_als_recommend_src_tile() and T >= 64
    assert plan.recommend_max_num() == rec.MAX_RECOMMEND >= 100
    assert 1 <= plan.recommend_lds_num() < plan.recommend_max_num()
    for rank in (1, 3, 10, 15, 16, 17, 32, 33, 64):
        dt = ALSPlan(rank).recommend_dst_tile()
        assert dt >= 4 and dt % 4 == 0
    assert lib.cyc_als_recommend_dst_tile(0) == 0 and lib.cyc_als_recommend_dst_tile(65) == 0
    # the splits cover the destinations, a fixed function of the shape alone
    for m, ndst in [(1, 0), (1, 1), (1, 257), (T + 1, 1000), (138493, 26744), (26744, 138493),
                    (5000000, 300)]:
        s, span = plan.recommend_splits(m, ndst), plan.recommend_span(m, ndst)
        assert s >= 1 and span >= 1 and s * span >= ndst and (s - 1) * span < max(ndst, 1)
        assert s == plan.recommend_splits(m, ndst)
        tiles = max(1, -(-m // T))
        assert plan.recommend_workspace(m, ndst, 10) == 8 * tiles * s * 10 * T
    assert plan.recommend_splits(138493, 26744) > 1       # neither side fills the CUs alone
    assert plan.recommend_splits(5000000, 300) == 1
    assert plan.recommend_workspace(1, 10, 0) == 0 == plan.recommend_workspace(1, 10, 129)


def test_c_refusals_come_before_any_device_work():
    """Null pointers throughout: a refusal that came after a launch would fault."""
    lib = N.load()

    def call(rank=10, num=10, m=4, ndst=7, ws=None, nsrc=4):
        if ws is None:
            ws = lib.cyc_als_recommend_workspace(m, ndst, rank, num)
        return lib.cyc_als_recommend_dev(None, None, nsrc, None, m, None, None, ndst, rank, num,
                                         None, None, None, ws, None)
    for kw, match in [(dict(rank=0), "ALS supports rank 1 to 64 but got 0"),
                      (dict(rank=65), "ALS supports rank 1 to 64 but got 65"),
                      (dict(num=0), r"recommendations must be in \[1, 128\] but got 0"),
                      (dict(num=129), r"recommendations must be in \[1, 128\] but got 129"),
                      (dict(ws=8), "the workspace must hold"),
                      (dict(m=5), "must not pass the 4 source rows")]:
        with pytest.raises(N.IllegalArgumentException, match="requirement failed: .*" + match):
            N.check(call(**kw))
