"""The evaluate pass of a fitted linear model and the summary built on it:
LinearRegressionSummary / LinearRegressionTrainingSummary of
ml/regression/LinearRegression.scala over libcyclone's k_linreg_rows
(csrc/linreg.hip): one read of the rows gives the predictions and the ten
sums and extrema every metric below is a function of.
"""
from __future__ import annotations

import math

import numpy as np

from . import _native as N
from . import parallel

# the slots of a stats call (include/cyclone.h, cyc_linreg_stats_dev)
W, WY, WYY, SSTOT, WE, SSERR, WABS, SSREG, RMIN, RMAX = range(10)


def _torch():
    import torch
    return torch


# ---- the Student-t tail -----------------------------------------------------------
def _log_beta_half(a: float) -> float:
    """log B(a, 1/2).  lgamma(a) - lgamma(a + 1/2) cancels badly for large a,
    so from a = 40 on it comes from the asymptotic series of the ratio
    (-log a / 2 + 1/(8a) - 1/(192 a^3) + 1/(640 a^5) - 17/(14336 a^7)), whose
    first omitted term is below 1e-17 there."""
    if a < 40.0:
        return math.lgamma(a) + 0.5 * math.log(math.pi) - math.lgamma(a + 0.5)
    a2 = a * a
    ratio = -0.5 * math.log(a) + (1.0 / 8.0 - (1.0 / 192.0 - (1.0 / 640.0 - 17.0 / (14336.0 * a2))
                                               / a2) / a2) / a
    return 0.5 * math.log(math.pi) + ratio


def _beta_cf(a: float, b: float, x: float) -> float:
    """The continued fraction of the incomplete beta function by the modified
    Lentz method; converges for x < (a + 1) / (a + b + 2) in O(sqrt(max(a, b)))
    terms, stopped when a term changes the product by less than 1e-16."""
    tiny = 1e-300
    qab, qap, qam = a + b, a + 1.0, a - 1.0
    c = 1.0
    d = 1.0 - qab * x / qap
    d = 1.0 / (d if abs(d) > tiny else tiny)
    h = d
    for m in range(1, 100000):
        m2 = 2 * m
        aa = m * (b - m) * x / ((qam + m2) * (a + m2))
        d = 1.0 + aa * d
        d = 1.0 / (d if abs(d) > tiny else tiny)
        c = 1.0 + aa / c
        c = c if abs(c) > tiny else tiny
        h *= d * c
        aa = -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2))
        d = 1.0 + aa * d
        d = 1.0 / (d if abs(d) > tiny else tiny)
        c = 1.0 + aa / c
        c = c if abs(c) > tiny else tiny
        delta = d * c
        h *= delta
        if abs(delta - 1.0) < 1e-16:
            return h
    raise ArithmeticError("incomplete beta: the continued fraction did not converge")


def student_t_two_sided(t: float, df: float) -> float:
    """P(|T| > |t|) for Student's t with df degrees of freedom:
    I_x(df / 2, 1 / 2) at x = df / (df + t^2), the regularized incomplete beta
    function by its continued fraction (on whichever side of the symmetry
    I_x(a, b) = 1 - I_{1-x}(b, a) it converges)."""
    if not df > 0.0:
        return math.nan
    if math.isnan(t):
        return math.nan
    t2 = t * t
    if t2 == 0.0:
        return 1.0
    if math.isinf(t2):
        return 0.0
    a, b = 0.5 * df, 0.5
    x, xc = df / (df + t2), t2 / (df + t2)           # x and 1 - x, each formed directly
    lnx, lnxc = -math.log1p(t2 / df), -math.log1p(df / t2)
    lbeta = _log_beta_half(a)
    front = math.exp(a * lnx + b * lnxc - lbeta)      # x^a (1-x)^b / B(a, b)
    # for many degrees of freedom the direct fraction loses digits next to the
    # switch-over point (its first denominator, 1 - (a + b) x / (a + 1), is a
    # difference of two numbers next to 1), so the complement's fraction, which
    # still converges there, is used as long as the tail is not tiny
    direct = x < (a + 1.0) / (a + b + 2.0) and not (a > 40.0 and t2 < 10.0)
    if direct:
        return min(1.0, front * _beta_cf(a, b, x) / a)
    return max(0.0, 1.0 - front * _beta_cf(b, a, xc) / b)


# ---- the device pass ----------------------------------------------------------------
def _rows_args(X):
    from .linalg import CSRRows
    if isinstance(X, CSRRows):
        return True, X.n, X.numCols
    return False, int(X.shape[0]), int(X.shape[1])


def linreg_predict(X, coef_dev, intercept: float, stream=None):
    """x_r . coef + intercept for every row of X (fp64 device tensor n x F, or
    linalg.CSRRows): a device vector."""
    torch = _torch()
    sparse, n, F = _rows_args(X)
    if int(coef_dev.shape[0]) != F:
        raise N.IllegalArgumentException(
            f"requirement failed: expected {int(coef_dev.shape[0])} features but got {F}")
    out = torch.empty(n, dtype=torch.float64, device=coef_dev.device)
    lib, s = N.load(), N.stream_handle(stream)
    if sparse:
        N.check(lib.cyc_linreg_predict_csr_dev(N.ptr(X.rowptr), N.ptr(X.colidx), N.ptr(X.values),
                                               n, F, N.ptr(coef_dev), float(intercept),
                                               N.ptr(out), s))
    else:
        N.check(lib.cyc_linreg_predict_dev(N.ptr(X.contiguous()), n, F, N.ptr(coef_dev),
                                           float(intercept), N.ptr(out), s))
    return out


def linreg_stats(X, y, w, coef_dev, intercept: float, center: float, want_pred=False,
                 stream=None):
    """(out, pred): the ten device doubles of cyc_linreg_stats_dev over this
    rank's rows, and the predictions if want_pred (else None)."""
    torch = _torch()
    sparse, n, F = _rows_args(X)
    if int(coef_dev.shape[0]) != F:
        raise N.IllegalArgumentException(
            f"requirement failed: expected {int(coef_dev.shape[0])} features but got {F}")
    if int(y.shape[0]) != n or (w is not None and int(w.shape[0]) != n):
        raise N.IllegalArgumentException("requirement failed: labels and weights of one per row")
    out = torch.empty(10, dtype=torch.float64, device=coef_dev.device)
    pred = torch.empty(n, dtype=torch.float64, device=coef_dev.device) if want_pred else None
    lib, s = N.load(), N.stream_handle(stream)
    if sparse:
        N.check(lib.cyc_linreg_stats_csr_dev(N.ptr(X.rowptr), N.ptr(X.colidx), N.ptr(X.values),
                                             n, F, N.ptr(y), N.ptr(w), N.ptr(coef_dev),
                                             float(intercept), float(center), N.ptr(out),
                                             N.ptr(pred), s))
    else:
        N.check(lib.cyc_linreg_stats_dev(N.ptr(X.contiguous()), n, F, N.ptr(y), N.ptr(w),
                                         N.ptr(coef_dev), float(intercept), float(center),
                                         N.ptr(out), N.ptr(pred), s))
    return out, pred


def _merge_over_ranks(out, n):
    """The ten outputs and the row count over ranks: the eight sums (and the
    count) by one all-reduce, the extrema by one max all-reduce of
    (-min, max)."""
    torch = _torch()
    d = parallel._dist()
    if d is None or d.get_world_size() == 1:
        return out.cpu().numpy(), n
    sums = torch.cat([out[:8], torch.tensor([float(n)], dtype=torch.float64, device=out.device)])
    parallel.allreduce_(sums)
    ext = torch.stack([-out[RMIN], out[RMAX]])
    comm = parallel.communicator()
    if comm is not None and ext.is_cuda:
        comm.allreduce_max_(ext)
    else:
        d.all_reduce(ext, op=d.ReduceOp.MAX)
    s, e = sums.cpu().numpy(), ext.cpu().numpy()
    return np.concatenate([s[:8], [-e[0], e[1]]]), int(s[8])


class LinearRegressionSummary:
    """The metrics of a linear model over a set of rows (X, y, weights), from
    one device pass (linreg_stats), run on first access.

    With p_r the prediction, e_r = y_r - p_r, W = sum w, ybar = sum w y / W,
    SSerr = sum w e^2, SStot = sum w (y - ybar)^2, SSy = sum w y^2,
    SSreg = sum w (p - ybar)^2, n = numInstances (rows, over ranks), p the
    number of features and k = 1 if the model fits an intercept, else 0:

      meanSquaredError      SSerr / W
      rootMeanSquaredError  sqrt(SSerr / W)
      meanAbsoluteError     sum w |e| / W
      explainedVariance     SSreg / W
      r2                    1 - SSerr / SStot with an intercept, else 1 - SSerr / SSy
      r2adj                 1 - (1 - r2) (n - k) / (n - p - k)
      degreesOfFreedom      n - p - k
      devianceResiduals     [min, max] of sqrt(w) e over the rows with w > 0
      residuals             device vector y - predictions
      predictions           device vector

    These definitions hold for every weighting.  The reference computes
    explainedVariance and the mean errors through its own weighted summarizer
    and may differ from them for non-unit weights; where it does, the table
    above is what this class returns.

    coefficientStandardErrors, tValues and pValues (coefficients first, the
    intercept last) exist only for a model of the normal-equation fit with
    regParam == 0, which carries diagInvAtWA:
    se = sqrt(diagInvAtWA SSerr / degreesOfFreedom), t = estimate / se, p the
    two-sided Student-t tail with degreesOfFreedom.  Any other model raises
    NotImplementedError, as the reference does."""

    def __init__(self, model, X, y, weights=None, center=None):
        self._model = model
        self._X, self._y, self._w = X, y, weights
        self._center = center
        self._s = None
        self._pred = None
        self._n = None

    # -- the pass -----------------------------------------------------------------
    def _stats(self):
        if self._s is None:
            torch = _torch()
            m, y, w = self._model, self._y, self._w
            if w is not None and bool((w < 0).any().item()):
                raise N.IllegalArgumentException(
                    "requirement failed: instance weights have to be >= 0.0")
            center = self._center
            if center is None:
                # ybar from (y, w) alone, over ranks
                sw = torch.stack([(y * w).sum() if w is not None else y.sum(),
                                  w.sum() if w is not None else
                                  torch.tensor(float(y.shape[0]), dtype=torch.float64,
                                               device=y.device)])
                parallel.allreduce_(sw)
                sw = sw.cpu().numpy()
                center = float(sw[0] / sw[1]) if sw[1] > 0 else 0.0
            out, pred = linreg_stats(self._X, y, w, m._coefficients_on(y.device), m.intercept,
                                     center, want_pred=True)
            self._s, self._n = _merge_over_ranks(out, int(y.shape[0]))
            self._pred = pred
        return self._s

    @property
    def predictions(self):
        self._stats()
        return self._pred

    @property
    def residuals(self):
        return self._y - self.predictions

    @property
    def numInstances(self) -> int:
        self._stats()
        return self._n

    @property
    def weightSum(self) -> float:
        return float(self._stats()[W])

    @property
    def meanSquaredError(self) -> float:
        s = self._stats()
        return float(s[SSERR] / s[W])

    @property
    def rootMeanSquaredError(self) -> float:
        return math.sqrt(self.meanSquaredError)

    @property
    def meanAbsoluteError(self) -> float:
        s = self._stats()
        return float(s[WABS] / s[W])

    @property
    def explainedVariance(self) -> float:
        s = self._stats()
        return float(s[SSREG] / s[W])

    @property
    def r2(self) -> float:
        s = self._stats()
        den = s[SSTOT] if self._model.fitIntercept else s[WYY]
        return float(1.0 - s[SSERR] / den)

    @property
    def degreesOfFreedom(self) -> int:
        k = 1 if self._model.fitIntercept else 0
        return self.numInstances - self._model.numFeatures - k

    @property
    def r2adj(self) -> float:
        k = 1 if self._model.fitIntercept else 0
        n = self.numInstances
        return 1.0 - (1.0 - self.r2) * (n - k) / (n - self._model.numFeatures - k)

    @property
    def devianceResiduals(self):
        s = self._stats()
        return [float(s[RMIN]), float(s[RMAX])]

    # -- inference on the coefficients --------------------------------------------------
    def _estimates(self):
        m = self._model
        k = m.numFeatures + (1 if m.fitIntercept else 0)
        if not getattr(m, "_inference", False) or m.diagInvAtWA.shape[0] != k:
            raise NotImplementedError(
                "No Std. Error of coefficients available for this LinearRegressionModel")
        est = np.append(m.coefficients, m.intercept) if m.fitIntercept else m.coefficients
        return est

    @property
    def coefficientStandardErrors(self):
        self._estimates()
        s = self._stats()
        rss = s[SSERR] / self.degreesOfFreedom
        return np.sqrt(self._model.diagInvAtWA * rss)

    @property
    def tValues(self):
        est = self._estimates()
        return est / self.coefficientStandardErrors

    @property
    def pValues(self):
        df = float(self.degreesOfFreedom)
        return np.array([student_t_two_sided(float(t), df) for t in self.tValues])


class LinearRegressionTrainingSummary(LinearRegressionSummary):
    """The summary of the training rows: the fit's own label mean is the
    centre, so it costs one pass and no reduction of its own."""

    def __init__(self, model, X, y, weights, yMean, objectiveHistory):
        super().__init__(model, X, y, weights, center=yMean)
        self.objectiveHistory = np.asarray(objectiveHistory, dtype=np.float64)

    @property
    def totalIterations(self) -> int:
        return max(0, int(self.objectiveHistory.shape[0]) - 1)
