"""ALS, host side (no device): the numpy restatement against hand-written
normal equations, the refusals, the initial factors and the model's save /
load in Spark's layout."""
import numpy as np
import pytest

import als_restatement as R
from cycloneml_amd import _native as N
from cycloneml_amd import persist
from cycloneml_amd import recommendation as rec
from cycloneml_amd.recommendation import ALS, ALSModel, ALSPlan

# rank 2, 2 x 2: user 0 rated items 0 and 1, user 1 rated items 0 and 1
Y2 = np.array([[0.6, 0.8], [1.0, -0.5]], dtype=np.float32)
ROWPTR = np.array([0, 2, 4], dtype=np.int64)
COLIDX = np.array([0, 1, 0, 1], dtype=np.int32)


def test_restatement_explicit_by_hand():
    vals = np.array([4.0, -1.0, 0.0, 2.5], dtype=np.float32)
    lam = 0.1
    out = R.half_step(ROWPTR, COLIDX, vals, Y2, lam)
    y0, y1 = Y2[0].astype(np.float64), Y2[1].astype(np.float64)
    for u, (r0, r1) in enumerate([(4.0, -1.0), (0.0, 2.5)]):
        A = np.outer(y0, y0) + np.outer(y1, y1) + lam * 2 * np.eye(2)
        b = r0 * y0 + r1 * y1
        np.testing.assert_allclose(out["A"][u], A, rtol=1e-15)
        np.testing.assert_allclose(out["x64"][u], np.linalg.solve(A, b), rtol=1e-13)
        assert np.array_equal(out["X"][u], out["x64"][u].astype(np.float32))
    assert out["present"].all() and not out["singular"]


def test_restatement_implicit_by_hand():
    # a negative and a zero rating: confidence from |r|, preference 0
    vals = np.array([2.0, -3.0, 0.0, 1.5], dtype=np.float32)
    lam, alpha = 0.1, 0.5
    out = R.half_step(ROWPTR, COLIDX, vals, Y2, lam, True, alpha)
    y0, y1 = Y2[0].astype(np.float64), Y2[1].astype(np.float64)
    YtY = np.outer(y0, y0) + np.outer(y1, y1)
    np.testing.assert_allclose(R.unpack(R.yty(Y2), 2), YtY, rtol=1e-15)
    # user 0: c = (1, 1.5), b = (1 + 1, 0), one positive rating
    A0 = YtY + 1.0 * np.outer(y0, y0) + 1.5 * np.outer(y1, y1) + lam * 1 * np.eye(2)
    b0 = 2.0 * y0
    # user 1: c = (0, 0.75), b = (0, 1.75), one positive rating
    A1 = YtY + 0.75 * np.outer(y1, y1) + lam * 1 * np.eye(2)
    b1 = 1.75 * y1
    for u, (A, b) in enumerate([(A0, b0), (A1, b1)]):
        np.testing.assert_allclose(out["A"][u], A, rtol=1e-15)
        np.testing.assert_allclose(out["x64"][u], np.linalg.solve(A, b), rtol=1e-13)


def test_restatement_empty_and_singular_rows():
    rowptr = np.array([0, 0, 1, 4], dtype=np.int64)
    colidx = np.array([0, 0, 1, 2], dtype=np.int32)
    vals = np.ones(4, dtype=np.float32)
    Y = np.eye(3, dtype=np.float32)
    out = R.half_step(rowptr, colidx, vals, Y, 0.0)
    assert list(out["present"]) == [False, True, True]
    assert out["singular"] == [1]              # one rating, rank 3, no ridge
    assert not out["X"][0].any() and not out["X"][1].any()
    np.testing.assert_allclose(out["x64"][2], [1.0, 1.0, 1.0])


def test_restatement_sdot_is_left_to_right_fp32():
    a = np.array([1.0, 2.0 ** -24, 2.0 ** -24, -1.0], dtype=np.float32)
    b = np.ones(4, dtype=np.float32)
    assert R.sdot(a, b) == np.float32(0.0)     # 1 + 2^-24 rounds back to 1, twice
    assert R.sdot(a[::-1].copy(), b) != np.float32(0.0)


@pytest.mark.parametrize("kwargs,match", [
    (dict(nonnegative=True), "nonnegative"),
    (dict(rank=0), "rank 1 to 64"),
    (dict(rank=65), "rank 1 to 64"),
    (dict(regParam=-0.1), "regParam"),
    (dict(alpha=-1.0), "alpha"),
    (dict(coldStartStrategy="zero"), "coldStartStrategy"),
])
def test_constructor_refusals(kwargs, match):
    with pytest.raises(N.IllegalArgumentException, match=match):
        ALS(**kwargs)


def test_plan_refuses_rank_and_exports_segment():
    for rank in (0, 65):
        with pytest.raises(N.IllegalArgumentException, match="requirement failed: ALS supports"):
            ALSPlan(rank)
    assert ALSPlan.segment == rec.SEGMENT == N.load().cyc_als_segment()


def test_fit_input_refusals():
    import torch
    u = torch.tensor([0, 1, 2], dtype=torch.int32)
    i = torch.tensor([0, 1, 0], dtype=torch.int32)
    r = torch.tensor([1.0, 2.0, 3.0], dtype=torch.float32)
    with pytest.raises(N.IllegalArgumentException, match="one length"):
        ALS().fit(u, i[:2], r)
    with pytest.raises(N.IllegalArgumentException, match="one length"):
        ALS().fit(u, i, r[:1])
    with pytest.raises(N.IllegalArgumentException, match="non-negative ids"):
        ALS().fit(torch.tensor([0, -1, 2], dtype=torch.int32), i, r)
    with pytest.raises(N.IllegalArgumentException, match="non-negative ids"):
        ALS().fit(u, torch.tensor([0, 1, -5], dtype=torch.int32), r)
    with pytest.raises(N.IllegalArgumentException, match="below numUsers"):
        ALS().fit(u, i, r, numUsers=2)
    with pytest.raises(N.IllegalArgumentException, match="int32"):
        ALS().fit(u.to(torch.int64), i, r)
    with pytest.raises(N.IllegalArgumentException, match="No ratings"):
        ALS().fit(u[:0], i[:0], r[:0])
    assert ALS.check_ratings(u, i, r) == (3, 2)
    assert ALS.check_ratings(u, i, r, 10, 7) == (10, 7)


def test_initial_factors():
    present = np.ones(50, dtype=bool)
    present[[3, 17, 49]] = False
    for rank in (1, 10, 64):
        a = rec.init_factors(present, rank, 42)
        assert a.dtype == np.float32 and a.shape == (50, rank)
        nrm = np.sqrt((a.astype(np.float64) ** 2).sum(axis=1))
        assert np.all(np.abs(nrm[present] - 1.0) <= 4 * rank * 2.0 ** -24)
        assert not a[~present].any()
        assert a.tobytes() == rec.init_factors(present, rank, 42).tobytes()
        assert a.tobytes() != rec.init_factors(present, rank, 43).tobytes()


def test_model_save_load_round_trip(tmp_path):
    rng = np.random.default_rng(5)
    U = rng.standard_normal((7, 3)).astype(np.float32)
    V = rng.standard_normal((5, 3)).astype(np.float32)
    up = np.array([1, 1, 0, 1, 1, 0, 1], dtype=np.uint8)
    vp = np.array([1, 0, 1, 1, 1], dtype=np.uint8)
    U[up == 0] = 0.0
    V[vp == 0] = 0.0
    path = str(tmp_path / "als")
    ALSModel(3, U, V, up, vp, "drop").save(path)
    meta = persist.read_metadata(path)
    assert meta["class"] == "org.apache.spark.ml.recommendation.ALSModel"
    assert meta["rank"] == 3
    rows = persist._read_parquet_rows(str(tmp_path / "als" / "userFactors"))
    assert [r["id"] for r in rows] == [0, 1, 3, 4, 6]     # present ids only
    assert set(rows[0]) == {"id", "features"}
    m = ALSModel.load(path)
    assert m.rank == 3 and m.coldStartStrategy == "drop"
    assert m.userFactors.dtype == np.float32
    assert m.userFactors.tobytes() == U.tobytes() and m.itemFactors.tobytes() == V.tobytes()
    assert np.array_equal(m.userPresent, up) and np.array_equal(m.itemPresent, vp)
    with pytest.raises(IOError):
        ALSModel(3, U, V, up, vp).save(path)


def test_model_refuses_mismatched_factors():
    with pytest.raises(N.IllegalArgumentException):
        ALSModel(3, np.zeros((4, 2), dtype=np.float32), np.zeros((4, 3), dtype=np.float32))
    with pytest.raises(N.IllegalArgumentException, match="coldStartStrategy"):
        ALSModel(2, np.zeros((4, 2), dtype=np.float32), np.zeros((4, 2), dtype=np.float32),
                 coldStartStrategy="keep")
