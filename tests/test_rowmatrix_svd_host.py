"""RowMatrix.computeSVD's host part (linalg.svd_from_gramian: the reference's
local-LAPACK branch as a function of the Gramian) against np.linalg.svd of
the rows, and the argument checks of computeSVD, multiply and PCA that fail
before any device call.  No GPU.  Bar: the project's 1e-10 (numpy's own
Gramian route stays below 2e-14 on these inputs)."""
import json
import os
import warnings

import numpy as np
import pytest

from cycloneml_amd import PCA, PCAModel
from cycloneml_amd._native import IllegalArgumentException
from cycloneml_amd.linalg import RowMatrix, SingularValueDecomposition, svd_from_gramian

GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden",
                                   "reference_known_answers.json")))


def spectrum_matrix(m, p, seed=0):
    """X = U0 diag(linspace(10, 1, p)) V0^T with orthonormal U0 (m x p), V0."""
    rng = np.random.default_rng(seed + m + p)
    U0, _ = np.linalg.qr(rng.normal(size=(m, p)))
    V0, _ = np.linalg.qr(rng.normal(size=(p, p)))
    return U0 @ np.diag(np.linspace(10.0, 1.0, p)) @ V0.T


def columns_close_up_to_sign(A, B, tol):
    assert A.shape == B.shape
    for j in range(A.shape[1]):
        d = min(np.abs(A[:, j] - B[:, j]).max(), np.abs(A[:, j] + B[:, j]).max())
        assert d <= tol, (j, d)


CASES = {
    "suite4x3": lambda: np.array(GOLD["rowmatrix_gram"]["rows"], dtype=np.float64),
    "300x6": lambda: spectrum_matrix(300, 6),
    "1000x40": lambda: spectrum_matrix(1000, 40),
}


@pytest.mark.parametrize("name", list(CASES))
def test_svd_from_gramian_matches_numpy_svd(name):
    X = CASES[name]()
    n = X.shape[1]
    _, s_ref, vt_ref = np.linalg.svd(X, full_matrices=False)
    for k in sorted({1, max(1, n // 2), n}):
        with warnings.catch_warnings():
            warnings.simplefilter("error")          # full rank: no cut, no warning
            s, V = svd_from_gramian(X.T @ X, k)
        assert s.shape == (k,) and V.shape == (n, k)
        err = np.abs(s - s_ref[:k]).max()
        print(f"{name} k={k}: max|s - ref| = {err:.3e}")
        assert err <= 1e-10
        columns_close_up_to_sign(V, vt_ref[:k].T, 1e-10)


def test_rcond_cut_on_low_rank_input():
    """X = A C of rank 2 (integer factors): with rCond = 1e-6, above the
    Gramian route's noise floor of about 1e-8 sigma_0, k = 5 keeps sk = 2."""
    rng = np.random.default_rng(7)
    A = rng.integers(-5, 6, size=(40, 2)).astype(np.float64)
    C = rng.integers(-5, 6, size=(2, 6)).astype(np.float64)
    X = A @ C
    assert np.linalg.matrix_rank(X) == 2
    with pytest.warns(RuntimeWarning, match="Requested 5 singular values but only found 2 "
                                            "nonzeros."):
        s, V = svd_from_gramian(X.T @ X, 5, rCond=1e-6)
    assert s.shape == (2,) and V.shape == (6, 2)
    _, s_ref, vt_ref = np.linalg.svd(X, full_matrices=False)
    assert np.abs(s - s_ref[:2]).max() <= 1e-10 * s_ref[0]
    columns_close_up_to_sign(V, vt_ref[:2].T, 1e-10)


@pytest.mark.parametrize("k", [0, -1, 4])
def test_svd_requires_k_in_range(k):
    X = CASES["suite4x3"]()
    msg = f"Requested k singular values but got k={k} and numCols=3."
    with pytest.raises(IllegalArgumentException) as e:
        svd_from_gramian(X.T @ X, k)
    assert str(e.value) == msg
    import torch
    with pytest.raises(IllegalArgumentException) as e:
        RowMatrix(torch.from_numpy(X)).computeSVD(k)          # before any device call
    assert str(e.value) == msg


def test_svd_result_type():
    r = SingularValueDecomposition(None, np.ones(1), np.ones((3, 1)))
    assert r.U is None and r.s.shape == (1,) and r.V.shape == (3, 1)


def test_multiply_dimension_mismatch_message():
    import torch
    mat = RowMatrix(torch.zeros((4, 3), dtype=torch.float64))
    with pytest.raises(IllegalArgumentException) as e:
        mat.multiply(np.zeros((5, 2)))
    assert str(e.value) == "Dimension mismatch: 3 vs 5"


def test_pca_validation():
    import torch
    with pytest.raises(IllegalArgumentException):
        PCA(0)
    with pytest.raises(IllegalArgumentException) as e:
        PCA(4).fit(torch.zeros((10, 3), dtype=torch.float64))
    assert str(e.value) == "source vector size 3 must be no less than k=4"
    m = PCAModel(np.eye(3)[:, :2], np.array([0.6, 0.3]))
    assert m.k == 2 and m.pc.shape == (3, 2)
