"""The row half of the require(norm1 >= 0.0 && norm2 >= 0.0) check kept with
the row image (include/cyclone.h, cyc_kmeans_rows_create): the first
accumulate call with a given (xnorm pointer, n) checks the rows' norms, later
calls on the image check the centers alone and raise what the first raised.
One image against a fresh image per call (whose first call always checks)."""
import numpy as np
import pytest

gpu = pytest.mark.gpu

N, D, K = 300, 8, 3
PREFIX = "requirement failed: Both norms should be greater or equal to 0.0, found "


def _data():
    rng = np.random.default_rng(11)
    X = rng.normal(size=(N, D)) * 2.0
    Cs = [X[:K] + 0.25 * t for t in range(5)]       # moving centers
    return X, Cs


def _call(plan, rows, Xd, xn, C, cuda):
    import torch
    from cycloneml_amd.clustering import row_norms
    k, d = C.shape
    Cd = torch.from_numpy(np.ascontiguousarray(C)).to(cuda)
    buf = torch.zeros(k * d + k + 1, dtype=torch.float64, device=cuda)
    plan.accumulate(Xd, xn, None, Cd, row_norms(Cd), buf[:k * d], buf[k * d:k * d + k],
                    buf[k * d + k:], rows=rows)
    torch.cuda.synchronize()
    return buf.cpu().numpy()


def _message(plan, rows, Xd, xn, C, cuda):
    from cycloneml_amd import _native as N_
    with pytest.raises(N_.IllegalArgumentException) as e:
        _call(plan, rows, Xd, xn, C, cuda)
    return str(e.value)


@gpu
def test_cached_verdict_same_results(cuda):
    """Five calls with moving centers on one image: sums, weights and cost
    bit-equal to the same calls each on a new image."""
    import torch
    from cycloneml_amd.clustering import KMeansPlan, row_norms
    X, Cs = _data()
    Xd = torch.from_numpy(X).to(cuda)
    xn = row_norms(Xd)
    plan = KMeansPlan(D, K, N)
    rows = plan.rows(Xd)
    kept = [_call(plan, rows, Xd, xn, C, cuda) for C in Cs]
    fresh = [_call(plan, plan.rows(Xd), Xd, xn, C, cuda) for C in Cs]
    for t, (a, b) in enumerate(zip(kept, fresh)):
        assert a.tobytes() == b.tobytes(), f"call {t}"
        assert a[K * D:K * D + K].sum() == N


@gpu
@pytest.mark.parametrize("row", [0, 137, N - 1])
def test_nan_row_raises_on_every_call(cuda, row):
    """A NaN norm at the first, an interior and the last row: the reference's
    message on the first call and, from the image's verdict, on the third,
    the same string."""
    import torch
    from cycloneml_amd.clustering import KMeansPlan, row_norms
    X, Cs = _data()
    X = X.copy()
    X[row, 3] = np.nan
    Xd = torch.from_numpy(X).to(cuda)
    xn = row_norms(Xd)
    plan = KMeansPlan(D, K, N)
    rows = plan.rows(Xd)
    msgs = [_message(plan, rows, Xd, xn, C, cuda) for C in Cs[:3]]
    c0 = [float(np.sqrt(np.sum(C[0] * C[0]))) for C in Cs[:3]]
    for m, nrm in zip(msgs, c0):
        assert m.startswith(PREFIX + "norm1=") and m.endswith(", norm2=NaN"), m
        assert float(m[len(PREFIX) + 6:m.index(", norm2=")]) == pytest.approx(nrm, rel=1e-15)
    # the same centers again: the first call's string from the stored verdict
    assert _message(plan, rows, Xd, xn, Cs[0], cuda) == msgs[0]
    assert _message(plan, plan.rows(Xd), Xd, xn, Cs[2], cuda) == msgs[2]


@gpu
def test_nan_center_with_cached_rows(cuda):
    """Clean rows, a NaN center on the third call: the centers' half still
    runs when the rows' verdict is cached, and the next call is clean."""
    import torch
    from cycloneml_amd.clustering import KMeansPlan, row_norms
    X, Cs = _data()
    Xd = torch.from_numpy(X).to(cuda)
    xn = row_norms(Xd)
    plan = KMeansPlan(D, K, N)
    rows = plan.rows(Xd)
    _call(plan, rows, Xd, xn, Cs[0], cuda)
    _call(plan, rows, Xd, xn, Cs[1], cuda)
    for bad, side in ((0, "norm1=NaN"), (2, "norm2=NaN")):
        Cb = Cs[2].copy()
        Cb[bad, 1] = np.nan
        msg = _message(plan, rows, Xd, xn, Cb, cuda)
        assert msg.startswith(PREFIX) and side in msg and msg.count("NaN") == 1, msg
        assert msg == _message(plan, plan.rows(Xd), Xd, xn, Cb, cuda)
    ok = _call(plan, rows, Xd, xn, Cs[3], cuda)
    assert ok.tobytes() == _call(plan, plan.rows(Xd), Xd, xn, Cs[3], cuda).tobytes()


@gpu
def test_other_norm_buffer_is_checked(cuda):
    """Norms at another address are checked afresh: a second xnorm buffer
    with a NaN raises after clean calls with the first, and the first buffer
    is clean again afterwards."""
    import torch
    from cycloneml_amd.clustering import KMeansPlan, row_norms
    X, Cs = _data()
    Xd = torch.from_numpy(X).to(cuda)
    xn = row_norms(Xd)
    xn2 = xn.clone()
    xn2[5] = float("nan")
    assert xn2.data_ptr() != xn.data_ptr()
    plan = KMeansPlan(D, K, N)
    rows = plan.rows(Xd)
    first = _call(plan, rows, Xd, xn, Cs[0], cuda)
    _call(plan, rows, Xd, xn, Cs[1], cuda)
    msg = _message(plan, rows, Xd, xn2, Cs[1], cuda)
    assert msg.startswith(PREFIX) and msg.endswith(", norm2=NaN"), msg
    assert msg == _message(plan, rows, Xd, xn2, Cs[1], cuda)
    assert _call(plan, rows, Xd, xn, Cs[0], cuda).tobytes() == first.tobytes()


@gpu
def test_k1_messages(cuda):
    """k = 1 (no statistics) with the image's own norms (xnorm None): a NaN
    row names center 0's norm; a NaN center names row 0's norm, recomputed on
    the host from the row (require_check's Xrow0 branch) on the first call
    and on the third.  The strings are the ones the call raised before the
    verdict was kept with the image."""
    import torch
    from cycloneml_amd.clustering import KMeansPlan
    X, _ = _data()
    X = X.copy()
    X[0] = [3.0, 4.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]            # |x0| = 5
    C = np.array([[1.0, 2.0, 2.0, 0.0, 0.0, 0.0, 0.0, 0.0]])   # |c0| = 3
    Cn = np.full((1, D), np.nan)
    Xd = torch.from_numpy(X).to(cuda)
    plan = KMeansPlan(D, 1, N)
    rows = plan.rows(Xd)
    msgs = [_message(plan, rows, Xd, None, Cn, cuda) for _ in range(3)]
    assert msgs == [PREFIX + "norm1=NaN, norm2=5.0"] * 3
    Xb = X.copy()
    Xb[7, 2] = np.nan
    Xbd = torch.from_numpy(Xb).to(cuda)
    rows = plan.rows(Xbd)
    msgs = [_message(plan, rows, Xbd, None, C, cuda) for _ in range(3)]
    assert msgs == [PREFIX + "norm1=3.0, norm2=NaN"] * 3
    msgs = [_message(plan, rows, Xbd, None, Cn, cuda) for _ in range(2)]
    assert msgs == [PREFIX + "norm1=NaN, norm2=5.0"] * 2
