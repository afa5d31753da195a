"""RowMatrix.tallSkinnyQR: what is decided before any device call.  No GPU."""
import numpy as np
import pytest
import torch

from cycloneml_amd._native import IllegalArgumentException
from cycloneml_amd.linalg import CSRRows, QRDecomposition, RowMatrix, normalize_r_signs


def _csr():
    return CSRRows(torch.tensor([0, 1, 2]), torch.tensor([0, 1], dtype=torch.int32),
                   torch.ones(2, dtype=torch.float64), 3)


@pytest.mark.parametrize("rows,computeQ", [
    (_csr, False),
    (lambda: torch.zeros((2, 1025), dtype=torch.float64), False),
    (lambda: torch.zeros((8, 64), dtype=torch.float64).t(), False),     # not contiguous
    (lambda: torch.zeros((5, 17), dtype=torch.float64), True),          # m < n
], ids=["csr", "n1025", "noncontiguous", "computeQ_wide"])
def test_refusals(rows, computeQ):
    with pytest.raises(IllegalArgumentException):
        RowMatrix(rows()).tallSkinnyQR(computeQ)


def test_decomposition_fields():
    assert QRDecomposition._fields == ("Q", "R")


def test_sign_normalisation():
    R = np.array([[-1.0, 2.0, -3.0], [0.0, 4.0, 5.0], [0.0, 0.0, -6.0]])
    want = np.array([[1.0, -2.0, 3.0], [0.0, 4.0, 5.0], [0.0, 0.0, 6.0]])
    assert np.array_equal(normalize_r_signs(R), want)
    assert np.array_equal(normalize_r_signs(R[:2]), want[:2])      # m < n: 2 x 3
    assert R[0, 0] == -1.0                                          # a copy
