"""GPU conformance: RowMatrix.tallSkinnyQR (csrc/tsqr.hip) against
Rnp = the sign-normalised numpy.linalg.qr(X, mode="r"), compared in
numpy.longdouble on the host.

Bar per entry: |R - Rnp|_ij <= 1e-10 ||X[:, j]||_2 (the project's fp64 bar),
exact zeros below the diagonal, diagonal >= 0.  The kernel works on tiles of T
rows (cyc_tsqr_tile_rows), panels of cyc_tsqr_panel_cols columns and runs of
cyc_tsqr_run_rows rows; the shapes sit at those edges.

The ill-conditioned case (cond 1e6) is the one a Cholesky of the Gramian
fails: on the CPU numpy.linalg.cholesky(X^T X)^T gives o = 9.6e-06 and e =
4.3e-12 against bounds of 1.4e-08 and 1.4e-14, both missed by over two orders
(numpy's own Householder R: o = 1.5e-11, e = 0)."""
import numpy as np
import pytest
import torch

from cycloneml_amd import _native as N
from cycloneml_amd.linalg import RowMatrix, TSQRPlan, normalize_r_signs
from cycloneml_amd.regression import SingularMatrixException

pytestmark = pytest.mark.gpu

LD = np.longdouble
EPS = np.finfo(np.float64).eps
RUN = N.load().cyc_tsqr_run_rows()
PANEL = N.load().cyc_tsqr_panel_cols()


def T(n):
    return N.load().cyc_tsqr_tile_rows(n)


def spectrum(m, n, s, seed=0):
    """X = U diag(s) V^T, U (m x k) and V (n x k) orthonormal, k = min(m, n)."""
    rng = np.random.default_rng(seed + 7 * m + n)
    k = min(m, n)
    U, _ = np.linalg.qr(rng.normal(size=(m, k)))
    V, _ = np.linalg.qr(rng.normal(size=(n, k)))
    return (U * np.asarray(s)[:k]) @ V.T


def device_r(cuda, X, **kw):
    return RowMatrix(torch.from_numpy(X).to(cuda)).tallSkinnyQR(**kw).R


def check_r(R, X):
    Rnp = normalize_r_signs(np.linalg.qr(X, mode="r"))
    assert R.shape == Rnp.shape == (min(X.shape), X.shape[1])
    assert np.array_equal(np.tril(R, -1), np.zeros_like(R))
    assert (np.diagonal(R) >= 0).all()
    excess = np.abs(R.astype(LD) - Rnp) - LD(1e-10) * np.linalg.norm(X, axis=0)
    assert excess.max() <= 0, excess.max()


SHAPES = [(m, n) for n in (1, 15, PANEL, PANEL + 1, 33, 80)
          for m in (T(n) - 1, T(n), T(n) + 1, RUN - 1, RUN + 1, 2 * RUN + 3)]
SHAPES += [(RUN + 1, 272), (3 * T(1024) + 1, 1024), (5, 17)]


@pytest.mark.parametrize("m,n", SHAPES)
def test_r_matches_householder_reference(cuda, m, n):
    assert T(272) < T(256) == 64
    X = spectrum(m, n, np.linspace(10.0, 1.0, n))
    check_r(device_r(cuda, X), X)


def q_of(X, R):
    """Q = X inv(R) in longdouble, column by column."""
    Q = np.zeros(X.shape, dtype=LD)
    R = R.astype(LD)
    for j in range(R.shape[0]):
        Q[:, j] = (X[:, j] - Q[:, :j] @ R[:j, j]) / R[j, j]
    return Q


def quality(X, R):
    """(o, e): max |Q^T Q - I| of Q = X inv(R), and max_i |sigma_i(R) -
    sigma_i(X)| / sigma_1."""
    Q = q_of(X, R)
    sx = np.linalg.svd(X, compute_uv=False)
    return (float(np.abs(Q.T @ Q - np.eye(R.shape[0])).max()),
            float(np.abs(np.linalg.svd(R, compute_uv=False) - sx).max() / sx[0]))


def ill_conditioned():
    n, kappa = 48, 1e6
    return spectrum(RUN + 17, n, np.logspace(0.0, -np.log10(kappa), n)), kappa


def quality_bounds(X, kappa):
    o, e = quality(X, normalize_r_signs(np.linalg.qr(X, mode="r")))
    return max(8 * o, 64 * EPS * kappa), max(8 * e, 64 * EPS), (o, e)


def test_ill_conditioned_keeps_householder_accuracy(cuda):
    X, kappa = ill_conditioned()
    obound, ebound, ref = quality_bounds(X, kappa)
    o, e = quality(X, device_r(cuda, X))
    print(f"device (o, e) = ({o:.3e}, {e:.3e}); numpy (o, e) = ({ref[0]:.3e}, {ref[1]:.3e})")
    assert o <= obound and e <= ebound, (o, obound, e, ebound)


def test_degenerate_columns(cuda):
    n, m = 17, 2 * T(17) + 3
    X = spectrum(m, n, np.linspace(10.0, 1.0, n))
    X[:, 5] = 0.0
    X[:, 9] = X[:, 2]
    A = RowMatrix(torch.from_numpy(X).to(cuda))
    R = A.tallSkinnyQR().R
    fro = np.linalg.norm(X)
    assert np.isfinite(R).all()
    Xl, Rl = X.astype(LD), R.astype(LD)
    assert np.abs(Rl.T @ Rl - Xl.T @ Xl).max() <= 1e-10 * fro ** 2
    assert R[5, 5] == 0.0 and R[9, 9] <= 1e-10 * fro
    with pytest.raises(SingularMatrixException):
        A.tallSkinnyQR(computeQ=True)


def test_same_bytes_on_every_call_and_for_every_workspace(cuda):
    n, m = 33, 2 * RUN + 3
    X = spectrum(m, n, np.linspace(10.0, 1.0, n))
    first = device_r(cuda, X)
    assert first.tobytes() == device_r(cuda, X).tobytes()
    small = TSQRPlan(n, TSQRPlan.minWorkspaceBytes(n))      # one run per launch
    assert first.tobytes() == device_r(cuda, X, plan=small).tobytes()
    with pytest.raises(N.IllegalArgumentException):
        TSQRPlan(n, TSQRPlan.minWorkspaceBytes(n) - 1)


def test_compute_q(cuda):
    n, m = 33, RUN + 1
    X = spectrum(m, n, np.linspace(10.0, 1.0, n))
    Q, R = RowMatrix(torch.from_numpy(X).to(cuda)).tallSkinnyQR(computeQ=True)
    Qh = Q.rows.cpu().numpy().astype(LD)
    assert (np.abs(Qh @ R - X) <= 1e-10 * (np.abs(Qh) @ np.abs(R))).all()
    assert np.abs(Qh.T @ Qh - np.eye(n)).max() <= 1e-10


def _two_rank_r(rank, world):
    m, n, cut = RUN + 782, 33, RUN + 5          # unequal shards: RUN + 5 rows and 777
    X = spectrum(m, n, np.linspace(10.0, 1.0, n))
    shard = X[:cut] if rank == 0 else X[cut:]
    return RowMatrix(torch.from_numpy(shard.copy()).to("cuda:0"), nRows=m).tallSkinnyQR().R


def test_two_ranks_hold_the_same_bytes(cuda):
    from test_comm_gpu import _run
    out = _run(_two_rank_r)
    assert isinstance(out[0], np.ndarray) and isinstance(out[1], np.ndarray), out
    assert out[0].tobytes() == out[1].tobytes()
    check_r(out[0], spectrum(RUN + 782, 33, np.linspace(10.0, 1.0, 33)))
