"""PCA on MI355X: host-side mirror of mllib/feature/PCA.scala (and the
ml/feature/PCA.scala estimator over it).

fit runs RowMatrix.computePrincipalComponentsAndExplainedVariance (the
covariance on the device, its eigensolve on the host); PCAModel.transform
projects device-resident rows onto the components with RowMatrix.multiply, the
fp64-MFMA product of libcyclone, so the projected rows stay in HBM for the
next stage.
"""
from __future__ import annotations

import numpy as np

from . import _native as N
from .linalg import RowMatrix


def _as_row_matrix(rows) -> RowMatrix:
    return rows if isinstance(rows, RowMatrix) else RowMatrix(rows)


class PCA:
    """mllib/feature/PCA.scala:33-82: PCA(k).fit(rows) -> PCAModel."""

    def __init__(self, k: int):
        if not k > 0:
            raise N.IllegalArgumentException(
                f"Number of principal components must be positive but got {k}")
        self.k = int(k)

    def fit(self, rows) -> "PCAModel":
        """rows: a dense fp64 device tensor, CSRRows or a RowMatrix (this
        rank's shard; the covariance is merged over ranks)."""
        mat = _as_row_matrix(rows)
        numFeatures = mat.numCols()
        if not self.k <= numFeatures:
            raise N.IllegalArgumentException(
                f"source vector size {numFeatures} must be no less than k={self.k}")
        pc, explainedVariance = mat.computePrincipalComponentsAndExplainedVariance(self.k)
        return PCAModel(pc, explainedVariance)


class PCAModel:
    """mllib/feature/PCA.scala:92-131: pc is numFeatures x k (numpy),
    explainedVariance the k leading shares of the variance."""

    def __init__(self, pc, explainedVariance):
        self.pc = np.ascontiguousarray(pc, dtype=np.float64)
        self.explainedVariance = np.asarray(explainedVariance, dtype=np.float64)
        self.k = int(self.pc.shape[1])
        self._pc_dev = {}      # device -> pc as a device tensor, uploaded once

    def _pc_on(self, device):
        import torch
        t = self._pc_dev.get(device)
        if t is None:
            t = self._pc_dev[device] = torch.from_numpy(self.pc).to(device)
        return t

    def transform(self, rows):
        """The nrows x k device tensor rows . pc (pc.transpose.multiply(vector)
        per row, PCA.scala:118-130) for a dense tensor, CSRRows or a
        RowMatrix.  Rows are not centred, as in the reference."""
        mat = _as_row_matrix(rows)
        device = mat.rows.device
        return mat.multiply(self._pc_on(device)).rows

