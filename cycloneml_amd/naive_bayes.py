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
host; `thresholds` is not offered.

Scoring (csrc/naive_bayes_score.hip, cyc_nbmodel_* in include/cyclone.h).
score_operands turns the model into b (C), M (C x d) and, gaussian, V and ls on
the host; NBScorer holds their device image and scores dense fp64 device rows:
  multinomial  raw_c = pi_c + sum_j x_j theta_cj
  complement   t_c = sum_j x_j theta_cj, raw_c = t_c - (max t + log sum_c
               exp(t_c - max))
  bernoulli    raw_c = (pi_c + sum_j L_cj) + sum_j x_j (theta_cj - L_cj),
               L = log1p(-exp theta)
  gaussian     raw_c = pi_c - (sum_j (x_j - theta_cj)^2 / sigma_cj + sum_j log
               sigma_cj) / 2
probability = exp(raw - max) / sum_c exp(raw_c - max); predict = the first
index of the largest raw.  In the linear forms a term with x_j == 0 is skipped
(the reference's sparse dot), so 0 times a -inf of theta (smoothing = 0) adds
nothing; Spark's dense gemv gives NaN there.  CSR rows are not scored.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _native as N

MODEL_TYPES = ("multinomial", "complement", "bernoulli", "gaussian")
MAX_NUM_CLASSES = 1024
RULE_LABEL, RULE_WEIGHT, RULE_VALUE = 1, 2, 3     # cyc_nb_aggregate_dev's badRule
SCORERS = ("auto", "product", "plain")            # cyc_nbmodel_create's scorer


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


def score_operands(pi, theta, sigma, modelType: str = "multinomial"):
    """(b (C), M (C x d), V (C x d or None), ls (C or None), finite) in numpy
    fp64, sums over j left to right: the operands of csrc/naive_bayes_score.hip.
    b is pi (zeros for complement, pi + sum_j L_cj for bernoulli, L =
    log1p(-exp theta)), M is theta (theta - L for bernoulli); gaussian adds V =
    sigma and ls_c = sum_j log sigma_cj.  finite: no inf or NaN in M."""
    check_model_type(modelType)
    pi = np.ascontiguousarray(pi, dtype=np.float64)
    theta = np.ascontiguousarray(theta, dtype=np.float64)
    C = pi.size
    V = ls = None
    with np.errstate(all="ignore"):
        if modelType == "gaussian":
            V = np.ascontiguousarray(sigma, dtype=np.float64)
            ls = np.zeros(C)
            for j in range(V.shape[1]):
                ls = ls + np.log(V[:, j])
            b, M = pi, theta
        elif modelType == "bernoulli":
            L = np.log1p(-np.exp(theta))
            b = pi + _rowsum(L)
            M = theta - L
        elif modelType == "complement":
            b, M = np.zeros(C), theta
        else:
            b, M = pi, theta
    return b, M, V, ls, bool(np.isfinite(M).all())


def check_rows(X, numFeatures: int, what: str = "model") -> int:
    """The row count of dense fp64 rows of this width; CSR rows are refused."""
    import torch
    from .linalg import CSRRows
    if isinstance(X, CSRRows):
        raise N.IllegalArgumentException(
            "NaiveBayesModel scores dense rows; the CSR form is not provided")
    if not torch.is_tensor(X) or X.dtype != torch.float64 or X.dim() != 2 \
            or not X.is_contiguous():
        raise N.IllegalArgumentException(
            "requirement failed: rows must be a contiguous fp64 device tensor (n x "
            f"{numFeatures})")
    if int(X.shape[1]) != numFeatures:
        raise N.IllegalArgumentException(
            f"requirement failed: the rows have {int(X.shape[1])} features but the {what} has "
            f"{numFeatures}")
    return int(X.shape[0])


class NBScorer:
    """cyc_nbmodel: the device image of one model's scoring operands
    (score_operands) and the workspace (workspaceBytes 0: 256 MiB).  scorer:
    "auto" (the MFMA product for a linear form with a finite M, else the plain
    kernel), "product" or "plain".  path is the one chosen."""

    def __init__(self, pi, theta, sigma=None, modelType: str = "multinomial", device=None,
                 workspaceBytes: int = 0, scorer: str = "auto"):
        import torch
        self.typeCode = check_model_type(modelType)
        if scorer not in SCORERS:
            raise N.IllegalArgumentException(
                f"scorer given invalid value {scorer}. Supported options: " + ", ".join(SCORERS)
                + ".")
        b, M, V, ls, self.finite = score_operands(pi, theta, sigma, modelType)
        check_shape(b.size, M.shape[1])
        self.numClasses, self.numFeatures = int(b.size), int(M.shape[1])
        self.modelType = modelType
        if scorer == "product" and (modelType == "gaussian" or not self.finite):
            raise N.IllegalArgumentException(
                "requirement failed: the product scorer serves the linear forms with a finite "
                "model matrix; this model takes the plain scorer")
        self._lib = N.load()
        self.device = torch.device("cuda:0" if device is None else device)
        with torch.cuda.device(self.device):
            dv = [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(self.device)
                  for a in (b, M, V, ls)]
            h = ctypes.c_void_p()
            N.check(self._lib.cyc_nbmodel_create(
                self.numClasses, self.numFeatures, self.typeCode, int(workspaceBytes),
                N.ptr(dv[0]), N.ptr(dv[1]), N.ptr(dv[2]), N.ptr(dv[3]), SCORERS.index(scorer),
                N.stream_handle(), ctypes.byref(h)))
        self.handle = h
        self.badRow = -1
        self.path = SCORERS[int(self._lib.cyc_nbmodel_path(h))]
        self.chunkRows = int(self._lib.cyc_nbmodel_chunk_rows(h))

    def close(self):
        if getattr(self, "handle", None):
            self._lib.cyc_nbmodel_destroy(self.handle)
            self.handle = None

    __del__ = close

    def score(self, X, raw=False, prob=False, pred=False):
        """(raw (n x C), prob (n x C), pred (n, fp64)) device tensors, None
        where not asked for.  badRow keeps the lowest offending row when the
        call raises."""
        import torch
        n = check_rows(X, self.numFeatures, "scorer")
        if not (raw or prob or pred):
            raise N.IllegalArgumentException(
                "requirement failed: one of raw, prob and pred must be asked for")
        C = self.numClasses
        out = [torch.empty((n, C), dtype=torch.float64, device=X.device) if raw else None,
               torch.empty((n, C), dtype=torch.float64, device=X.device) if prob else None,
               torch.empty(n, dtype=torch.float64, device=X.device) if pred else None]
        self.badRow = -1
        if n == 0:
            return tuple(out)
        row = ctypes.c_int64(-1)
        try:
            with torch.cuda.device(X.device):
                N.check(self._lib.cyc_nbmodel_score_dev(
                    self.handle, N.ptr(X), n, N.ptr(out[0]), N.ptr(out[1]), N.ptr(out[2]),
                    ctypes.byref(row), N.stream_handle()))
        finally:
            self.badRow = int(row.value)
        return tuple(out)
