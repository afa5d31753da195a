"""GeneralizedLinearRegression by iteratively reweighted least squares: the
host side of ml/regression/GeneralizedLinearRegression.scala and
ml/optim/IterativelyReweightedLeastSquares.scala.

One IRLS iteration is a per-row pass that turns the current model into a
working label z and a working weight w' (libcyclone's k_glm_rows,
cyc_glm_reweight_dev) followed by the WeightedLeastSquares fit of
(X, z, w') that regression.py already has: the weighted fp64 MFMA syrk, the
all-reduce of its packed moments and the host solve.  The training summary's
sums (deviance, Pearson chi-square, log-likelihood) are one more pass
(k_glm_stats) whose six results merge over ranks by one all-reduce.

The reference's sources are not vendored; the semantics are restated and
pinned by the numpy restatement in tests/test_glm_host.py.
"""
from __future__ import annotations

import ctypes
import math
from statistics import NormalDist
from typing import Callable, Optional

import numpy as np

from . import _native as N
from . import parallel
from .regression import (MAX_NUM_FEATURES, WeightedLeastSquares, WeightedLeastSquaresModel,
                         WLSPlan)

EPSILON = 1e-16        # GeneralizedLinearRegression.epsilon
DELTA = 0.1            # Poisson / Tweedie delta

# the C ABI's codes (include/cyclone.h, CYC_GLM_*)
FAMILY_CODES = {"gaussian": 0, "binomial": 1, "poisson": 2, "gamma": 3, "tweedie": 4}
LINK_CODES = {"identity": 0, "log": 1, "inverse": 2, "logit": 3, "probit": 4, "cloglog": 5,
              "sqrt": 6, "power": 7}
# supported links per family, the default first
SUPPORTED_LINKS = {
    "gaussian": ("identity", "log", "inverse"),
    "binomial": ("logit", "probit", "cloglog"),
    "poisson": ("log", "identity", "sqrt"),
    "gamma": ("inverse", "identity", "log"),
}
_POWER_LINKS = {0.0: "log", 1.0: "identity", -1.0: "inverse", 0.5: "sqrt"}
_POWER_FAMILIES = {0.0: "gaussian", 1.0: "poisson", 2.0: "gamma"}
# sums of the stats pass
S_W, S_WY, S_DEVIANCE, S_PEARSON, S_LOGLIK, S_LOGW = range(6)


def _torch():
    import torch
    return torch


def _require(cond, msg):
    if not cond:
        raise N.IllegalArgumentException("requirement failed: " + msg)


class FamilyAndLink:
    """The family and link objects of a parameter set (Family.fromParams,
    Link.fromParams): `family` and `link` are the resolved names (tweedie
    with variancePower 0 / 1 / 2 is gaussian / poisson / gamma; linkPower
    0 / 1 / -1 / 0.5 is log / identity / inverse / sqrt)."""

    def __init__(self, family: str, link: Optional[str], variancePower: float,
                 linkPower: Optional[float]):
        family = str(family).lower()
        _require(family in FAMILY_CODES,
                 f"family must be one of {', '.join(FAMILY_CODES)} but got {family}")
        self.paramFamily = family
        if family == "tweedie":
            _require(link is None, "When family is tweedie, use param linkPower to specify "
                                   "link function; param link must not be set.")
            vp = float(variancePower)
            _require(vp == 0.0 or vp >= 1.0,
                     f"variancePower must be 0.0 or in [1, inf) but got {vp}")
            lp = 1.0 - vp if linkPower is None else float(linkPower)
            _require(lp == lp, "linkPower must not be NaN")
            self.family = _POWER_FAMILIES.get(vp, "tweedie")
            self.link = _POWER_LINKS.get(lp, "power")
            self.variancePower, self.linkPower = vp, lp
            self.codes = (FAMILY_CODES["tweedie"], LINK_CODES["power"])
        else:
            _require(linkPower is None, "param linkPower is for the tweedie family; use param "
                                        f"link with family {family}")
            link = SUPPORTED_LINKS[family][0] if link is None else str(link).lower()
            _require(link in SUPPORTED_LINKS[family],
                     f"Generalized Linear Regression with {family} family does not support "
                     f"{link} link function.")
            self.family, self.link = family, link
            self.variancePower, self.linkPower = 0.0, 0.0
            self.codes = (FAMILY_CODES[family], LINK_CODES[link])

    # -- one value on the host (predict of one vector, the null model) ------------
    def link_fn(self, mu: float) -> float:
        k, lp = self.link, self.linkPower
        if k == "identity":
            return mu
        if k == "log":
            return math.log(mu)
        if k == "inverse":
            return 1.0 / mu
        if k == "logit":
            return math.log(mu / (1.0 - mu))
        if k == "probit":
            return NormalDist().inv_cdf(mu)
        if k == "cloglog":
            return math.log(-math.log(1.0 - mu))
        if k == "sqrt":
            return math.sqrt(mu)
        return math.pow(mu, lp)

    def unlink(self, eta: float) -> float:
        k, lp = self.link, self.linkPower
        try:
            if k == "identity":
                return eta
            if k == "log":
                return math.exp(eta)
            if k == "inverse":
                return 1.0 / eta
            if k == "logit":
                return 1.0 / (1.0 + math.exp(-eta))
            if k == "probit":
                return NormalDist().cdf(eta)
            if k == "cloglog":
                return 1.0 - math.exp(-math.exp(eta))
            if k == "sqrt":
                return eta * eta
            return math.pow(eta, 1.0 / lp)
        except OverflowError:
            # math.exp past the double range: the reference's +Infinity
            if k == "logit":
                return 0.0
            if k == "cloglog":
                return 1.0
            return math.inf

    def project(self, mu: float) -> float:
        if self.family == "gaussian":
            return mu
        if self.family == "binomial":
            return EPSILON if mu < EPSILON else (1.0 - EPSILON if mu > 1.0 - EPSILON else mu)
        return EPSILON if mu < EPSILON else (1.7976931348623157e308 if math.isinf(mu) else mu)

    # -- elementwise on device vectors (the summary's residuals) -------------------
    def variance_t(self, mu):
        if self.family == "binomial":
            return mu * (1.0 - mu)
        if self.family == "poisson":
            return mu
        if self.family == "gamma":
            return mu * mu
        if self.family == "tweedie":
            return mu ** self.variancePower
        return _torch().ones_like(mu)

    def deriv_t(self, mu):
        torch = _torch()
        k, lp = self.link, self.linkPower
        if k == "identity":
            return torch.ones_like(mu)
        if k == "log":
            return 1.0 / mu
        if k == "inverse":
            return -1.0 / (mu * mu)
        if k == "logit":
            return 1.0 / (mu * (1.0 - mu))
        if k == "probit":
            x = torch.special.ndtri(mu)
            return 1.0 / (torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi))
        if k == "cloglog":
            return 1.0 / ((mu - 1.0) * torch.log(1.0 - mu))
        if k == "sqrt":
            return 1.0 / (2.0 * torch.sqrt(mu))
        return lp * mu ** (lp - 1.0)

    def deviance_t(self, y, mu, w):
        torch = _torch()
        f, vp = self.family, self.variancePower
        if f == "binomial":
            return 2.0 * w * (torch.xlogy(y, y / mu) + torch.xlogy(1.0 - y, (1.0 - y) / (1.0 - mu)))
        if f == "poisson":
            return 2.0 * w * (torch.xlogy(y, y / mu) - (y - mu))
        if f == "gamma":
            return -2.0 * w * (torch.log(y / mu) - (y - mu) / mu)
        if f == "tweedie":
            def yp(a, p):
                return torch.log(a / mu) if p == 0.0 else (a ** p - mu ** p) / p
            y1 = torch.clamp(y, min=DELTA) if 1.0 <= vp < 2.0 else y
            return 2.0 * w * (y * yp(y1, 1.0 - vp) - yp(y, 2.0 - vp))
        return w * (y - mu) * (y - mu)


def _rows_info(X):
    """(sparse, n, numFeatures) of device rows (fp64 tensor or CSRRows)."""
    from .linalg import CSRRows
    if isinstance(X, CSRRows):
        return True, X.n, X.numCols
    return False, int(X.shape[0]), int(X.shape[1])


class GLMPlan:
    """The per-row passes of one family and link over rows of width
    numFeatures (C ABI cyc_glm_*)."""

    def __init__(self, fl: FamilyAndLink, numFeatures: int):
        self._lib = N.load()
        h = ctypes.c_void_p()
        N.check(self._lib.cyc_glm_plan_create(fl.codes[0], fl.codes[1], fl.variancePower,
                                              fl.linkPower, int(numFeatures), ctypes.byref(h)))
        self.handle = h
        self.numFeatures = int(numFeatures)

    def close(self):
        if self.handle:
            self._lib.cyc_glm_plan_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _call(self, name, X, *rest):
        sparse, n, k = _rows_info(X)
        _require(k == self.numFeatures, f"expected {self.numFeatures} features but got {k}")
        if sparse:
            fn = getattr(self._lib, f"cyc_glm_{name}_csr_dev")
            rows = (N.ptr(X.rowptr), N.ptr(X.colidx), N.ptr(X.values))
        else:
            fn = getattr(self._lib, f"cyc_glm_{name}_dev")
            rows = (N.ptr(X),)
        N.check(fn(self.handle, *rows, n, *rest))

    def reweight(self, X, y, w, offset, coef, intercept, z, wOut, init=False, stream=None):
        """(z, wOut) of the rows: FamilyAndLink.initialize (init) or
        reweightFunc at (coef, intercept); coef None is a model without
        features.  Raises IllegalArgumentException on a label outside the
        family's domain."""
        self._call("reweight", X, N.ptr(y), N.ptr(w), N.ptr(offset), N.ptr(coef), float(intercept),
                   int(bool(init)), N.ptr(z), N.ptr(wOut), N.stream_handle(stream))

    def mean(self, X, offset, coef, intercept, out, linkPrediction=False, stream=None):
        self._call("mean", X, N.ptr(offset), N.ptr(coef), float(intercept),
                   int(bool(linkPrediction)), N.ptr(out), N.stream_handle(stream))

    def stats(self, X, y, w, offset, coef, intercept, sums, project=True, dispersion=1.0,
              stream=None):
        """sums (6 device doubles): sum w, sum w y, deviance, Pearson
        chi-square, log-likelihood, sum log w of this shard's rows."""
        self._call("stats", X, N.ptr(y), N.ptr(w), N.ptr(offset), N.ptr(coef), float(intercept),
                   int(bool(project)), float(dispersion), N.ptr(sums), N.stream_handle(stream))


class IterativelyReweightedLeastSquaresModel:
    def __init__(self, coefficients, intercept, diagInvAtWA, numIterations):
        self.coefficients = np.asarray(coefficients, dtype=np.float64)
        self.intercept = float(intercept)
        self.diagInvAtWA = np.asarray(diagInvAtWA, dtype=np.float64)
        self.numIterations = int(numIterations)


class IterativelyReweightedLeastSquares:
    """IterativelyReweightedLeastSquares(initialModel, reweightFunc,
    fitIntercept, regParam, maxIter, tol).  reweight(model) returns the
    device vectors (z, w') of the rows at that model."""

    def __init__(self, initialModel: WeightedLeastSquaresModel, reweight: Callable,
                 fitIntercept: bool, regParam: float, maxIter: int, tol: float):
        self.initialModel = initialModel
        self.reweight = reweight
        self.fitIntercept = bool(fitIntercept)
        self.regParam = float(regParam)
        self.maxIter = int(maxIter)
        self.tol = float(tol)

    def fit(self, X, plan: Optional[WLSPlan] = None) -> IterativelyReweightedLeastSquaresModel:
        wls = WeightedLeastSquares(self.fitIntercept, self.regParam, 0.0,
                                   standardizeFeatures=False, standardizeLabel=False)
        it, converged, model = 0, False, self.initialModel
        while it < self.maxIter and not converged:
            old = model
            z, w = self.reweight(old)
            model = wls.fit(X, z, w, plan=plan)
            maxTol = max(float(np.abs(old.coefficients - model.coefficients).max(initial=0.0)),
                         abs(old.intercept - model.intercept))
            converged = maxTol < self.tol
            it += 1
        return IterativelyReweightedLeastSquaresModel(model.coefficients, model.intercept,
                                                      model.diagInvAtWA, it)


class GeneralizedLinearRegression:
    """GeneralizedLinearRegression estimator over device-resident rows
    (solver "irls", up to 4096 features)."""

    def __init__(self, family: str = "gaussian", link: Optional[str] = None,
                 variancePower: float = 0.0, linkPower: Optional[float] = None,
                 fitIntercept: bool = True, maxIter: int = 25, tol: float = 1e-6,
                 regParam: float = 0.0, solver: str = "irls"):
        self.familyAndLink = FamilyAndLink(family, link, variancePower, linkPower)
        _require(regParam >= 0.0, f"regParam cannot be negative: {regParam}")
        _require(maxIter > 0, f"maxIter must be a positive integer: {maxIter}")
        _require(tol >= 0.0, f"tol must be >= 0, but was set to {tol}")
        if solver != "irls":
            raise N.IllegalArgumentException(
                f"GeneralizedLinearRegression: unsupported solver {solver}")
        self.family, self.link = self.familyAndLink.paramFamily, link
        self.variancePower, self.linkPower = float(variancePower), linkPower
        self.fitIntercept = bool(fitIntercept)
        self.maxIter, self.tol, self.regParam = int(maxIter), float(tol), float(regParam)
        self.solver = solver

    def fit(self, X, y, weights=None, offset=None) -> "GeneralizedLinearRegressionModel":
        """X: this rank's device rows (fp64 tensor n x k, or linalg.CSRRows);
        y, weights, offset: device fp64 vectors (None: weights 1, offset 0)."""
        torch = _torch()
        fl = self.familyAndLink
        _, n, k = _rows_info(X)
        _require(k <= MAX_NUM_FEATURES,
                 f"Currently, GeneralizedLinearRegression only supports number of features <= "
                 f"{MAX_NUM_FEATURES}. Found {k} in the input dataset.")
        first = WeightedLeastSquares(self.fitIntercept, self.regParam, 0.0,
                                     standardizeFeatures=True, standardizeLabel=True)
        plan = GLMPlan(fl, k)
        if fl.family == "gaussian" and fl.link == "identity":
            m = first.fit(X, y if offset is None else y - offset, weights)
            fitted = IterativelyReweightedLeastSquaresModel(m.coefficients, m.intercept,
                                                            m.diagInvAtWA, 0)
        else:
            z = torch.empty(n, dtype=torch.float64, device=X.device)
            wz = torch.empty(n, dtype=torch.float64, device=X.device)
            wls = WLSPlan(k)
            try:
                plan.reweight(X, y, weights, offset, None, 0.0, z, wz, init=True)
                initial = first.fit(X, z, wz, plan=wls)

                def reweight(model):
                    coef = torch.from_numpy(model.coefficients).to(X.device)
                    plan.reweight(X, y, weights, offset, coef, model.intercept, z, wz)
                    return z, wz

                fitted = IterativelyReweightedLeastSquares(
                    initial, reweight, self.fitIntercept, self.regParam, self.maxIter,
                    self.tol).fit(X, plan=wls)
            finally:
                wls.close()
        model = GeneralizedLinearRegressionModel(fitted.coefficients, fitted.intercept, fl,
                                                 plan=plan)
        model.summary = GeneralizedLinearRegressionTrainingSummary(
            model, X, y, weights, offset, self, fitted.diagInvAtWA, fitted.numIterations)
        return model


class GeneralizedLinearRegressionModel:
    """coefficients, intercept and the training summary of a fitted
    GeneralizedLinearRegression."""

    def __init__(self, coefficients, intercept: float, familyAndLink: FamilyAndLink,
                 plan: Optional[GLMPlan] = None):
        self.coefficients = np.asarray(coefficients, dtype=np.float64)
        self.intercept = float(intercept)
        self.familyAndLink = familyAndLink
        self.summary = None
        self._plan = plan
        self._coef_dev = None

    @property
    def numFeatures(self) -> int:
        return int(self.coefficients.shape[0])

    def _device_coef(self, device):
        if self._coef_dev is None or self._coef_dev.device != device:
            self._coef_dev = _torch().from_numpy(self.coefficients).to(device)
        return self._coef_dev

    def _predict(self, X, offset, linkPrediction):
        from .linalg import CSRRows
        torch = _torch()
        fl = self.familyAndLink
        if isinstance(X, (torch.Tensor, CSRRows)):
            _, n, k = _rows_info(X)
            _require(k == self.numFeatures,
                     f"expected {self.numFeatures} features but got {k}")
            if self._plan is None:
                self._plan = GLMPlan(fl, self.numFeatures)
            out = torch.empty(n, dtype=torch.float64, device=X.device)
            self._plan.mean(X, offset, self._device_coef(X.device), self.intercept, out,
                            linkPrediction=linkPrediction)
            return out
        v = np.asarray(X, dtype=np.float64)
        eta = float(np.dot(v, self.coefficients) + self.intercept) + (
            0.0 if offset is None else float(offset))
        return eta if linkPrediction else fl.project(fl.unlink(eta))

    def predict(self, X, offset=None):
        """The fitted mean project(unlink(eta)), eta = dot(features,
        coefficients) + intercept + offset: for device rows (fp64 tensor
        n x numFeatures, or CSRRows) a device vector; for one host vector a
        float."""
        return self._predict(X, offset, False)

    def predictLink(self, X, offset=None):
        """The linear predictor eta of the same rows."""
        return self._predict(X, offset, True)


class GeneralizedLinearRegressionTrainingSummary:
    """GeneralizedLinearRegressionTrainingSummary over the training rows
    (kept by reference).  The sums are computed on first use; under
    torch.distributed every rank has to ask for the same fields, since each
    is an all-reduce."""

    RESIDUALS = ("deviance", "pearson", "working", "response")

    def __init__(self, model, X, y, weights, offset, estimator, diagInvAtWA, numIterations):
        self._model, self._X, self._y, self._w, self._off = model, X, y, weights, offset
        self._fl = model.familyAndLink
        self._fitIntercept = estimator.fitIntercept
        self._maxIter, self._tol = estimator.maxIter, estimator.tol
        self._diagInvAtWA = np.asarray(diagInvAtWA, dtype=np.float64)
        self.numIterations = int(numIterations)
        self._cache = {}

    # -- the stats pass, merged over ranks ------------------------------------------
    def _sums(self, coef, intercept, project=True, dispersion=1.0):
        """The six sums at a model, and the row count, over all ranks."""
        torch = _torch()
        X = self._X
        _, n, _ = _rows_info(X)
        buf = torch.zeros(7, dtype=torch.float64, device=X.device)
        self._model._plan.stats(X, self._y, self._w, self._off, coef, intercept, buf[:6],
                                project=project, dispersion=dispersion)
        buf[6] = n
        parallel.allreduce_(buf)
        return buf.cpu().numpy()

    def _fitted_sums(self):
        if "fitted" not in self._cache:
            m = self._model
            self._cache["fitted"] = self._sums(m._device_coef(self._X.device), m.intercept)
        return self._cache["fitted"]

    def _cached(self, key, fn):
        if key not in self._cache:
            self._cache[key] = fn()
        return self._cache[key]

    @property
    def numInstances(self) -> int:
        return int(self._fitted_sums()[6])

    @property
    def rank(self) -> int:
        return self._model.numFeatures + (1 if self._fitIntercept else 0)

    @property
    def degreesOfFreedom(self) -> int:
        return self.numInstances - self.rank

    @property
    def residualDegreeOfFreedom(self) -> int:
        return self.degreesOfFreedom

    @property
    def residualDegreeOfFreedomNull(self) -> int:
        return self.numInstances - (1 if self._fitIntercept else 0)

    @property
    def deviance(self) -> float:
        return float(self._fitted_sums()[S_DEVIANCE])

    @property
    def pearsonChiSquare(self) -> float:
        return float(self._fitted_sums()[S_PEARSON])

    def _null_intercept(self) -> float:
        fl = self._fl
        if not self._fitIntercept:
            return 0.0
        s = self._fitted_sums()
        if self._off is None:
            return fl.link_fn(s[S_WY] / s[S_W])
        return self._intercept_only_fit()

    def _intercept_only_fit(self) -> float:
        """The intercept of the model without features, fitted with the
        offset: the same IRLS with b = sum w' z / sum w' as its WLS fit."""
        torch = _torch()
        fl, X, y, off = self._fl, self._X, self._y, self._off
        _, n, _ = _rows_info(X)

        def mean(z, w):
            t = torch.stack([(w * z).sum(), w.sum()])
            parallel.allreduce_(t)
            t = t.cpu().numpy()
            _require(t[1] > 0.0, "Sum of weights cannot be zero.")
            return float(t[0] / t[1])

        if fl.family == "gaussian" and fl.link == "identity":
            w = torch.ones_like(y) if self._w is None else self._w
            return mean(y - off, w)
        plan = self._model._plan
        z = torch.empty(n, dtype=torch.float64, device=X.device)
        wz = torch.empty(n, dtype=torch.float64, device=X.device)
        plan.reweight(X, y, self._w, off, None, 0.0, z, wz, init=True)
        b = mean(z, wz)
        it, converged = 0, False
        while it < self._maxIter and not converged:
            plan.reweight(X, y, self._w, off, None, b, z, wz)
            old, b = b, mean(z, wz)
            converged = abs(old - b) < self._tol
            it += 1
        return b

    @property
    def nullDeviance(self) -> float:
        return self._cached("nullDeviance", lambda: float(
            self._sums(None, self._null_intercept(), project=False)[S_DEVIANCE]))

    @property
    def dispersion(self) -> float:
        if self._fl.family in ("binomial", "poisson"):
            return 1.0
        return self.pearsonChiSquare / self.degreesOfFreedom

    @property
    def aic(self) -> float:
        f = self._fl.family
        s = self._fitted_sums()
        if f == "tweedie":
            raise NotImplementedError("No AIC available for the tweedie family")
        if f == "gaussian":
            n = self.numInstances
            fam = n * (math.log(self.deviance / n * 2.0 * math.pi) + 1.0) + 2.0 - s[S_LOGW]
        elif f == "gamma":
            # Gamma.aic's own dispersion: deviance / weightSum
            m = self._model
            disp = self.deviance / s[S_W]
            ll = self._cached("gammaLoglik", lambda: float(self._sums(
                m._device_coef(self._X.device), m.intercept, dispersion=disp)[S_LOGLIK]))
            fam = -2.0 * ll + 2.0
        else:
            fam = -2.0 * s[S_LOGLIK]
        return float(fam + 2 * self.rank)

    @property
    def coefficientStandardErrors(self) -> np.ndarray:
        """sqrt(diagInvAtWA * dispersion), the intercept's last."""
        d = self._diagInvAtWA
        if d.shape == (1,) and d[0] == 0.0:
            raise NotImplementedError(
                "No Std. Error of coefficients available for this "
                "GeneralizedLinearRegressionModel")
        return np.sqrt(d * self.dispersion)

    @property
    def tValues(self) -> np.ndarray:
        m = self._model
        est = np.append(m.coefficients, m.intercept) if self._fitIntercept else m.coefficients
        return est / self.coefficientStandardErrors

    @property
    def pValues(self) -> np.ndarray:
        from scipy import special
        t = np.abs(self.tValues)
        if self._fl.paramFamily in ("binomial", "poisson"):
            return 2.0 * special.ndtr(-t)
        return 2.0 * special.stdtr(float(self.degreesOfFreedom), -t)

    def residuals(self, residualsType: str = "deviance"):
        """Device vector of this rank's residuals: deviance, pearson, working
        or response."""
        torch = _torch()
        if residualsType not in self.RESIDUALS:
            raise NotImplementedError(f"The residuals type {residualsType} is not supported by "
                                      "Generalized Linear Regression.")
        fl, y = self._fl, self._y
        mu = self._cached("mu", lambda: self._model.predict(self._X, self._off))
        w = torch.ones_like(y) if self._w is None else self._w
        r = y - mu
        if residualsType == "response":
            return r
        if residualsType == "working":
            return r * fl.deriv_t(mu)
        if residualsType == "pearson":
            return r / torch.sqrt(fl.variance_t(mu)) * torch.sqrt(w)
        return torch.sign(r) * torch.sqrt(torch.clamp(fl.deviance_t(y, mu, w), min=0.0))
