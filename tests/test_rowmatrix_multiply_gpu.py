"""GPU conformance: RowMatrix.multiply (cyc_rowmatrix_multiply_dev /
_csr_dev), computeSVD's U and PCAModel.transform against a numpy restatement
of the reference loop (RowMatrix.scala:400-423: Y[i, l] = dot of row i with
column l of B, fp64).

Bar per entry: |got - ref| <= 1e-10 (|X| |B|)[i, l] -- the project's 1e-10
taken against the sum of absolute products, so that cancellation cannot fake
a failure (both sides round below n 2^-53 of that sum).  Non-finite values
are compared position by position.

The dense kernel works on 16 x 16 MFMA tiles, 16-index chunks of the
contraction, 256-row workgroups and panels of PANEL = 64 columns of B; the
shapes sit at those edges."""
import numpy as np
import pytest

from test_rowmatrix_svd_host import CASES, columns_close_up_to_sign

pytestmark = pytest.mark.gpu

PANEL = 64      # columns of B per pass over the rows (rowmatrix_multiply.hip)
NROWS = (1, 15, 17, 63, 65, 257, 1000)
NK = [(1, 1), (3, 2), (4, 16), (5, 17), (16, 15), (17, 64), (130, 65), (1024, 8), (1025, 129),
      (257, 200),
      # just below, at and above the panel width, and the same past two panels
      (40, PANEL - 1), (40, PANEL), (40, PANEL + 1), (33, 2 * PANEL + 1)]


def ref_multiply(X, B):
    """The reference loop: one fp64 dot per output element."""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([(X * B[:, l]).sum(axis=1) for l in range(B.shape[1])], axis=1)


def reference(X, B):
    """(the reference loop's product, the bound per entry)."""
    with np.errstate(invalid="ignore"):
        return ref_multiply(X, B), 1e-10 * (np.abs(X) @ np.abs(B))


def check(got, X, B, what="", ref=None):
    ref, bound = ref if ref is not None else reference(X, B)
    assert got.shape == ref.shape, what
    fin = np.isfinite(ref)
    assert np.array_equal(np.isfinite(got), fin), what
    assert np.array_equal(got[~fin], ref[~fin], equal_nan=True), what
    with np.errstate(invalid="ignore"):
        excess = (np.abs(got - ref) - bound)[fin]
    assert excess.size == 0 or excess.max() <= 0.0, (what, excess.max())


def dev(a, cuda):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def csr_of(X, mask, cuda):
    """CSRRows of the entries of X where mask (stored zeros included)."""
    from cycloneml_amd.linalg import CSRRows
    rowptr = np.concatenate([[0], np.cumsum(mask.sum(axis=1))]).astype(np.int64)
    cols = np.nonzero(mask)[1].astype(np.int32)
    return CSRRows(dev(rowptr, cuda), dev(cols, cuda), dev(X[mask].astype(np.float64), cuda),
                   X.shape[1])


def data(nrows, n, k, seed=0):
    rng = np.random.default_rng(1000 * n + k + seed)
    return rng.normal(size=(nrows, n)), rng.normal(size=(n, k))


@pytest.mark.parametrize("n,k", NK)
def test_dense_matches_reference_loop(cuda, n, k):
    from cycloneml_amd.linalg import RowMatrix
    X, B = data(max(NROWS), n, k)
    Xd = dev(X, cuda)
    ref, bound = reference(X, B)          # rows are independent: one reference, sliced
    for nrows in NROWS:
        Y = RowMatrix(Xd[:nrows]).multiply(B).rows
        assert tuple(Y.shape) == (nrows, k)
        check(Y.cpu().numpy(), X[:nrows], B, f"nrows={nrows}", (ref[:nrows], bound[:nrows]))


@pytest.mark.parametrize("n,k", NK)
def test_csr_matches_dense_on_densified_rows(cuda, n, k):
    from cycloneml_amd.linalg import RowMatrix
    X, B = data(max(NROWS), n, k, seed=1)
    rng = np.random.default_rng(n + k)
    mask = rng.random(X.shape) < 0.3
    Xz = np.where(mask, X, 0.0)
    Xd = dev(Xz, cuda)
    ref, bound = reference(Xz, B)
    for nrows in (1, 17, 65, 1000):
        got = RowMatrix(csr_of(Xz[:nrows], mask[:nrows], cuda)).multiply(B).rows.cpu().numpy()
        check(got, Xz[:nrows], B, f"csr nrows={nrows}", (ref[:nrows], bound[:nrows]))
        dense = RowMatrix(Xd[:nrows]).multiply(B).rows.cpu().numpy()
        assert (np.abs(got - dense) <= bound[:nrows]).all()


@pytest.mark.parametrize("k", [3, 16, 40, 70, 300])
def test_csr_patterns(cuda, k):
    """No entries at all; empty first, middle and last rows; one full row;
    rows whose stored values are all zero."""
    from cycloneml_amd.linalg import RowMatrix
    n = 37
    X, B = data(70, n, k, seed=2)
    mask = np.random.default_rng(k).random(X.shape) < 0.2
    mask[[0, 33, 34, 69]] = False         # empty first, middle and last rows
    mask[5] = True                        # one full row
    mask[7, :9] = True                    # stored zeros only
    X[7] = 0.0
    Xz = np.where(mask, X, 0.0)
    got = RowMatrix(csr_of(Xz, mask, cuda)).multiply(B).rows.cpu().numpy()
    check(got, Xz, B)
    assert (got[[0, 33, 34, 69, 7]] == 0.0).all()
    none = np.zeros_like(mask)
    got = RowMatrix(csr_of(Xz, none, cuda)).multiply(B).rows.cpu().numpy()
    assert got.shape == (70, k) and (got == 0.0).all()


@pytest.mark.parametrize("sparse", [False, True])
def test_nonfinite_values_stay_in_their_row_and_column(cuda, sparse):
    """A NaN and an Inf in one row of X (sharing a 16-row tile with finite
    rows), an Inf in one column of B (sharing a 16-column tile with finite
    columns): only the reference's outputs are non-finite."""
    from cycloneml_amd.linalg import RowMatrix
    X, B = data(40, 20, 20, seed=3)

    def run(X, B):
        rows = csr_of(X, np.ones(X.shape, dtype=bool), cuda) if sparse else dev(X, cuda)
        return RowMatrix(rows).multiply(B).rows.cpu().numpy()

    Xn = X.copy()
    Xn[5, 3], Xn[5, 7] = np.nan, np.inf
    got = run(Xn, B)
    check(got, Xn, B, "row")
    assert not np.isfinite(got[5]).any() and np.isfinite(np.delete(got, 5, axis=0)).all()
    Bn = B.copy()
    Bn[2, 9] = np.inf
    got = run(X, Bn)
    check(got, X, Bn, "column")
    assert np.isinf(got[:, 9]).all() and np.isfinite(np.delete(got, 9, axis=1)).all()
    got = run(Xn, Bn)
    check(got, Xn, Bn, "both")
    fin = np.isfinite(got)
    assert not fin[5].any() and not fin[:, 9].any()
    assert np.delete(np.delete(fin, 5, axis=0), 9, axis=1).all()


def test_two_calls_give_the_same_bits(cuda):
    import torch
    from cycloneml_amd.linalg import RowMatrix
    X, B = data(1000, 257, 200, seed=4)
    mat = RowMatrix(dev(X, cuda))
    assert torch.equal(mat.multiply(B).rows, mat.multiply(B).rows)
    mask = np.random.default_rng(4).random(X.shape) < 0.3
    smat = RowMatrix(csr_of(X, mask, cuda))
    assert torch.equal(smat.multiply(B).rows, smat.multiply(B).rows)


def test_slices_streams_and_no_rows(cuda):
    import torch
    from cycloneml_amd import _native as N
    from cycloneml_amd.linalg import CSRRows, RowMatrix
    X, B = data(300, 33, 20, seed=5)
    Xd, Bd = dev(X, cuda), dev(B, cuda)
    # a slice that starts off the 16-row tile; B as a device tensor
    check(RowMatrix(Xd[5:300]).multiply(Bd).rows.cpu().numpy(), X[5:300], B, "slice")
    # CSR rows of a slice: rowptr keeps its base
    mask = np.random.default_rng(5).random(X.shape) < 0.4
    Xz = np.where(mask, X, 0.0)
    full = csr_of(Xz, mask, cuda)
    part = CSRRows(full.rowptr[5:301], full.colidx, full.values, 33)
    check(RowMatrix(part).multiply(Bd).rows.cpu().numpy(), Xz[5:300], B, "csr slice")
    # a stream of the caller's
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=cuda)
    with torch.cuda.stream(s):
        Y = RowMatrix(Xd).multiply(Bd).rows
        Ys = RowMatrix(full).multiply(Bd, stream=s).rows
    s.synchronize()
    check(Y.cpu().numpy(), X, B, "stream")
    check(Ys.cpu().numpy(), Xz, B, "csr stream")
    # no rows: OK without a launch
    Y0 = RowMatrix(Xd[:0], 0, 33).multiply(B).rows
    assert tuple(Y0.shape) == (0, 20)
    lib = N.load()
    assert lib.cyc_rowmatrix_multiply_dev(None, 0, 33, N.ptr(Bd), 20, None, None) == N.CYC_OK
    empty = CSRRows(full.rowptr[:1], full.colidx, full.values, 33)
    assert tuple(RowMatrix(empty).multiply(B).rows.shape) == (0, 20)


def test_argument_checks(cuda):
    from cycloneml_amd import _native as N
    X, B = data(4, 3, 2)
    Xd, Bd = dev(X, cuda), dev(B, cuda)
    lib = N.load()
    p = N.ptr(Xd)
    # n k past the JVM array bound of DenseMatrix
    rc = lib.cyc_rowmatrix_multiply_dev(p, 1, 65536, p, 32768, p, None)
    assert rc == N.CYC_ERR_INVALID_ARG
    assert b"65536 x 32768 dense matrix is too large to allocate" in lib.cyc_last_error()
    rc = lib.cyc_rowmatrix_multiply_csr_dev(p, p, p, 1, 65536, p, 32768, p, None)
    assert rc == N.CYC_ERR_INVALID_ARG
    for bad in ((-1, 3, 2), (4, 0, 2), (4, 3, 0)):
        assert lib.cyc_rowmatrix_multiply_dev(p, bad[0], bad[1], N.ptr(Bd), bad[2], p,
                                              None) == N.CYC_ERR_INVALID_ARG


def test_multiply_returns_a_row_matrix(cuda):
    from cycloneml_amd._native import IllegalArgumentException
    from cycloneml_amd.linalg import RowMatrix
    X, B = data(500, 40, 7, seed=6)
    mat = RowMatrix(dev(X, cuda))
    out = mat.multiply(B)
    assert isinstance(out, RowMatrix)
    assert out.numRows() == 500 and out.numCols() == 7
    Y = ref_multiply(X, B)
    np.testing.assert_allclose(out.computeGramianMatrix(), Y.T @ Y, rtol=1e-10, atol=1e-10)
    with pytest.raises(IllegalArgumentException) as e:
        mat.multiply(np.zeros((41, 2)))
    assert str(e.value) == "Dimension mismatch: 40 vs 41"


def _svd_case(X, rows, k):
    from cycloneml_amd.linalg import RowMatrix
    u_ref, s_ref, vt_ref = np.linalg.svd(X, full_matrices=False)
    res = RowMatrix(rows).computeSVD(k, computeU=True)
    assert res.s.shape == (k,) and res.V.shape == (X.shape[1], k)
    assert np.abs(res.s - s_ref[:k]).max() <= 1e-10
    columns_close_up_to_sign(res.V, vt_ref[:k].T, 1e-10)
    assert res.U.numCols() == k
    U = res.U.rows.cpu().numpy()
    columns_close_up_to_sign(U, u_ref[:, :k], 1e-10)
    # the rank-k product; X itself at k = n
    target = X if k == X.shape[1] else (u_ref[:, :k] * s_ref[:k]) @ vt_ref[:k]
    assert np.abs((U * res.s) @ res.V.T - target).max() <= 1e-10 * s_ref[0]


@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("name", list(CASES))
def test_compute_svd_with_u(cuda, name, sparse):
    X = CASES[name]()
    rows = csr_of(X, np.ones(X.shape, dtype=bool), cuda) if sparse else dev(X, cuda)
    ks = (1, 2, 3) if name == "suite4x3" else (X.shape[1],)
    for k in ks:
        _svd_case(X, rows, k)


def test_compute_svd_without_u(cuda):
    from cycloneml_amd.linalg import RowMatrix
    X = CASES["300x6"]()
    res = RowMatrix(dev(X, cuda)).computeSVD(3)
    assert res.U is None and res.s.shape == (3,)


@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("k", [1, 3])
def test_pca_fit_transform(cuda, k, sparse):
    from cycloneml_amd import PCA
    from cycloneml_amd.linalg import RowMatrix
    X = np.random.default_rng(64).normal(size=(1000, 64)) * np.linspace(3.0, 0.5, 64) + 0.25
    rows = (lambda: csr_of(X, np.ones(X.shape, dtype=bool), cuda)) if sparse \
        else (lambda: dev(X, cuda))
    model = PCA(k).fit(rows())
    assert model.pc.shape == (64, k)
    pc_ref, ev_ref = RowMatrix(rows()).computePrincipalComponentsAndExplainedVariance(k)
    np.testing.assert_allclose(model.explainedVariance, ev_ref, rtol=1e-12)
    T = model.transform(rows())
    assert T.is_cuda and tuple(T.shape) == (1000, k)
    check(T.cpu().numpy(), X, model.pc, "transform")
    check(model.transform(RowMatrix(rows())).cpu().numpy(), X, model.pc, "transform RowMatrix")
    assert len(model._pc_dev) == 1            # pc uploaded once per device
