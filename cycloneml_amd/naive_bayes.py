"""NaiveBayes (ml/classification/NaiveBayes.scala, Spark 3.3): the fit over
dense fp64 device rows.  The kernels are csrc/naive_bayes.hip (cyc_nb_* in
include/cyclone.h); the estimator and the model are in classification.py.

Aggregate.  One pass adds, per class c, into one fp64 buffer [W (C) | S (C x d,
row-major) | Q (C x d, gaussian only)]: W_c = sum of w_i, S_c[j] = sum of w_i
x_ij, Q_c[j] = sum of w_i (x_ij x_ij) over the rows of label c.  Buffers of
shards and ranks merge by addition (parallel.allreduce_).

M step (host, sums over j left to right), lam = smoothing, D = sum_c W_c:
  multinomial  pi_c = log(W_c + lam) - log(D + C lam),
               theta_cj = log(S_cj + lam) - log(sum_j S_cj + d lam)
  complement   pi as above; T_j = sum_c S_cj (c ascending), K_cj = T_j - S_cj,
               theta_cj = -(log(K_cj + lam) - log(sum_j K_cj + d lam))
  bernoulli    pi as above; theta_cj = log(S_cj + lam) - log(W_c + 2 lam)
  gaussian     pi_c = log W_c - log D, theta_cj = S_cj / W_c,
               eps = 1e-9 max_j(sum_c Q_cj / D - (sum_c S_cj)^2 / D / D),
               sigma_cj = eps + Q_cj / W_c - theta_cj^2
Spark forms Q as the square of a square root of the same sum; the plain sum
here is within an ulp of it.

This project's own rules: every class 0 .. C - 1 needs W_c > 0 (Spark's groupBy
would silently renumber the classes); C is 1 to 1024; the fit takes dense rows
only (there is no CSR aggregate); the model holds pi, theta and sigma on the
host and has no device predictions yet; `thresholds` is not offered.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _native as N

MODEL_TYPES = ("multinomial", "complement", "bernoulli", "gaussian")
MAX_NUM_CLASSES = 1024
RULE_LABEL, RULE_WEIGHT, RULE_VALUE = 1, 2, 3     # cyc_nb_aggregate_dev's badRule


def check_model_type(modelType: str) -> int:
    if modelType not in MODEL_TYPES:
        raise N.IllegalArgumentException(
            f"NaiveBayes was created with an unknown modelType: {modelType}. Supported options: "
            + ", ".join(MODEL_TYPES) + ".")
    return MODEL_TYPES.index(modelType)


def check_shape(numClasses, numFeatures=None):
    if not 1 <= int(numClasses) <= MAX_NUM_CLASSES:
        raise N.IllegalArgumentException(
            f"requirement failed: NaiveBayes supports 1 to {MAX_NUM_CLASSES} classes but got "
            f"{numClasses}")
    if numFeatures is not None and int(numFeatures) < 1:
        raise N.IllegalArgumentException(
            f"requirement failed: numFeatures must be positive but got {numFeatures}")


def sums_length(C: int, d: int, modelType: str = "multinomial") -> int:
    return C + C * d * (2 if modelType == "gaussian" else 1)


def split_sums(sums, C: int, d: int, modelType: str = "multinomial"):
    """(W (C), S (C x d), Q (C x d) or None) views of a host sums buffer."""
    sums = np.asarray(sums, dtype=np.float64)
    if sums.shape != (sums_length(C, d, modelType),):
        raise N.IllegalArgumentException(
            f"requirement failed: a sums buffer for numClasses = {C}, numFeatures = {d}, "
            f"{modelType} has {sums_length(C, d, modelType)} values but got {sums.size}")
    S = sums[C:C + C * d].reshape(C, d)
    Q = sums[C + C * d:].reshape(C, d) if modelType == "gaussian" else None
    return sums[:C], S, Q


def _rowsum(A):
    """Per row, the sum over j left to right."""
    out = np.zeros(A.shape[0], dtype=np.float64)
    for j in range(A.shape[1]):
        out = out + A[:, j]
    return out


def _colsum(A):
    """Per column, the sum over c ascending."""
    out = np.zeros(A.shape[1], dtype=np.float64)
    for c in range(A.shape[0]):
        out = out + A[c]
    return out


def m_step(sums, C: int, d: int, modelType: str = "multinomial", smoothing: float = 1.0):
    """(pi (C), theta (C x d), sigma (C x d; 0 x 0 unless gaussian)) from a
    merged buffer."""
    check_model_type(modelType)
    if not smoothing >= 0:
        raise N.IllegalArgumentException(f"smoothing given invalid value {smoothing}.")
    W, S, Q = split_sums(sums, C, d, modelType)
    empty = np.nonzero(~(W > 0))[0]
    if empty.size:
        raise N.IllegalArgumentException(
            f"requirement failed: class {int(empty[0])} has no weight; every class 0 .. "
            f"{C - 1} needs training rows of positive weight")
    lam = float(smoothing)
    D = 0.0
    for c in range(C):
        D = D + W[c]
    sigma = np.zeros((0, 0), dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        if modelType == "gaussian":
            pi = np.log(W) - np.log(D)
            theta = S / W[:, None]
            tS, tQ = _colsum(S), _colsum(Q)
            eps = 1e-9 * np.max(tQ / D - tS * tS / D / D)
            sigma = eps + Q / W[:, None] - theta * theta
            return pi, theta, sigma
        pi = np.log(W + lam) - np.log(D + C * lam)
        if modelType == "multinomial":
            theta = np.log(S + lam) - np.log(_rowsum(S) + d * lam)[:, None]
        elif modelType == "complement":
            K = _colsum(S)[None, :] - S
            theta = -(np.log(K + lam) - np.log(_rowsum(K) + d * lam)[:, None])
        else:
            theta = np.log(S + lam) - np.log(W + 2.0 * lam)[:, None]
    return pi, theta, sigma


class NBPlan:
    """cyc_nb_plan: classes, features, model type and the device workspace
    (workspaceBytes 0: 256 MiB)."""

    def __init__(self, numClasses: int, numFeatures: int, modelType: str = "multinomial",
                 workspaceBytes: int = 0):
        self.typeCode = check_model_type(modelType)
        check_shape(numClasses, numFeatures)
        self.numClasses, self.numFeatures = int(numClasses), int(numFeatures)
        self.modelType = modelType
        self.sumsLength = sums_length(self.numClasses, self.numFeatures, modelType)
        self._lib = N.load()
        h = ctypes.c_void_p()
        N.check(self._lib.cyc_nb_plan_create(self.numClasses, self.numFeatures, self.typeCode,
                                             int(workspaceBytes), ctypes.byref(h)))
        self.handle = h
        self.badRow, self.badRule = -1, 0
        self.colTile = int(self._lib.cyc_nb_col_tile(h))
        self.rowsPerRun = int(self._lib.cyc_nb_rows_per_run(h))
        self.classesPerPass = int(self._lib.cyc_nb_classes_per_pass(h))

    def close(self):
        if getattr(self, "handle", None):
            self._lib.cyc_nb_plan_destroy(self.handle)
            self.handle = None

    __del__ = close

    def _rows(self, X):
        """The row count of dense rows of this plan's width."""
        import torch
        if not torch.is_tensor(X) or X.dtype != torch.float64 or X.dim() != 2 \
                or not X.is_contiguous():
            raise N.IllegalArgumentException(
                "requirement failed: rows must be a contiguous fp64 device tensor (n x "
                f"{self.numFeatures})")
        if int(X.shape[1]) != self.numFeatures:
            raise N.IllegalArgumentException(
                f"requirement failed: the rows have {int(X.shape[1])} features but the plan has "
                f"{self.numFeatures}")
        return int(X.shape[0])

    @staticmethod
    def _vector(v, n, what):
        import torch
        if not torch.is_tensor(v) or v.dtype != torch.float64 or v.numel() != n \
                or not v.is_contiguous():
            raise N.IllegalArgumentException(
                f"requirement failed: {what} must be {n} contiguous fp64 values")

    def accumulate(self, X, y, weights, sums):
        """sums += the aggregate of this shard (dense rows; all device fp64).
        badRow / badRule keep the lowest offending row and its rule when the
        call raises."""
        n = self._rows(X)
        self._vector(y, n, "labels")
        if weights is not None:
            self._vector(weights, n, "weights")
        self._vector(sums, self.sumsLength, "sums")
        row, rule = ctypes.c_int64(-1), ctypes.c_int32(0)
        try:
            N.check(self._lib.cyc_nb_aggregate_dev(
                self.handle, N.ptr(X), n, N.ptr(y), N.ptr(weights), N.ptr(sums),
                ctypes.byref(row), ctypes.byref(rule), N.stream_handle()))
        finally:
            self.badRow, self.badRule = int(row.value), int(rule.value)
