"""CPU: GeneralizedLinearRegression's parameter checks, and the numpy
restatement of its IRLS fit and training summary that tests/test_glm_gpu.py
uses as the reference.

The restatement (class Ref, fit_ref, summary_ref) follows
ml/regression/GeneralizedLinearRegression.scala and
ml/optim/IterativelyReweightedLeastSquares.scala: eta by a longdouble dot,
float64 after that, the weighted moments of every WLS fit in
numpy.longdouble, and WeightedLeastSquares.solve for the solve.  Here it is
checked against scikit-learn's Poisson, Gamma and logistic fits (1e-6
absolute: the margin covers L-BFGS's stopping point, not IRLS) and its
deviance and AIC against closed forms written with scipy.special.gammaln.
"""
import functools
import math

import numpy as np
import pytest
from scipy import special

from cycloneml_amd import GeneralizedLinearRegression, WeightedLeastSquares
from cycloneml_amd._native import IllegalArgumentException

EPS, DELTA = 1e-16, 0.1
PAIRS = [("gaussian", "identity"), ("gaussian", "log"), ("gaussian", "inverse"),
         ("binomial", "logit"), ("binomial", "probit"), ("binomial", "cloglog"),
         ("poisson", "log"), ("poisson", "identity"), ("poisson", "sqrt"),
         ("gamma", "inverse"), ("gamma", "identity"), ("gamma", "log")]
# (centre, scale) of eta per link: mu stays clear of every project clamp,
# binomial mu in [0.02, 0.98], positive families' mu in [0.05, 50], eta > 0.1
# for inverse, sqrt and power links (a standardized predictor stays within
# +-4.5 at these sizes)
ETA_RANGE = {"identity": (2.0, 0.4), "log": (0.5, 0.5), "inverse": (1.0, 0.2),
             "logit": (0.0, 0.8), "probit": (0.0, 0.45), "cloglog": (-0.8, 0.5),
             "sqrt": (1.6, 0.3), "power": (1.0, 0.2)}


class Ref:
    """Family and link of a parameter set, on numpy arrays."""

    def __init__(self, family, link=None, variancePower=0.0, linkPower=None):
        self.paramFamily = family
        self.vp, self.lp = 0.0, 0.0
        if family == "tweedie":
            self.vp = float(variancePower)
            self.lp = 1.0 - self.vp if linkPower is None else float(linkPower)
            family = {0.0: "gaussian", 1.0: "poisson", 2.0: "gamma"}.get(self.vp, "tweedie")
            link = {0.0: "log", 1.0: "identity", -1.0: "inverse", 0.5: "sqrt"}.get(self.lp, "power")
        elif link is None:
            link = {"gaussian": "identity", "binomial": "logit", "poisson": "log",
                    "gamma": "inverse"}[family]
        self.family, self.link = family, link

    def kwargs(self):
        """The estimator's parameters of this pair."""
        if self.paramFamily == "tweedie":
            return {"family": "tweedie", "variancePower": self.vp, "linkPower": self.lp}
        return {"family": self.family, "link": self.link}

    # families
    def variance(self, mu):
        return {"gaussian": lambda: np.ones_like(mu), "binomial": lambda: mu * (1.0 - mu),
                "poisson": lambda: mu, "gamma": lambda: mu * mu,
                "tweedie": lambda: mu ** self.vp}[self.family]()

    def initialize(self, y, w):
        if self.family == "binomial":
            return (w * y + 0.5) / (w + 1.0)
        if self.family == "poisson":
            return np.maximum(y, DELTA)
        if self.family == "tweedie":
            return np.where(y == 0.0, DELTA, y)
        return y.copy()

    def project(self, mu):
        if self.family == "gaussian":
            return mu
        if self.family == "binomial":
            return np.where(mu < EPS, EPS, np.where(mu > 1.0 - EPS, 1.0 - EPS, mu))
        return np.where(mu < EPS, EPS, np.where(np.isinf(mu), np.finfo(np.float64).max, mu))

    def deviance(self, y, mu, w):
        with np.errstate(divide="ignore", invalid="ignore"):
            def ylogy(a, b):
                return np.where(a == 0.0, 0.0, a * np.log(np.where(a == 0.0, 1.0, a) / b))
            if self.family == "binomial":
                return 2.0 * w * (ylogy(y, mu) + ylogy(1.0 - y, 1.0 - mu))
            if self.family == "poisson":
                return 2.0 * w * (ylogy(y, mu) - (y - mu))
            if self.family == "gamma":
                return -2.0 * w * (np.log(y / mu) - (y - mu) / mu)
            if self.family == "tweedie":
                def yp(a, p):
                    return np.log(a / mu) if p == 0.0 else (a ** p - mu ** p) / p
                y1 = np.maximum(y, DELTA) if 1.0 <= self.vp < 2.0 else y
                return 2.0 * w * (y * yp(y1, 1.0 - self.vp) - yp(y, 2.0 - self.vp))
            return w * (y - mu) * (y - mu)

    def loglik(self, y, mu, w, dispersion=1.0):
        if self.family == "binomial":
            n, k = np.floor(w + 0.5), np.floor(y * w + 0.5)
            ll = (special.gammaln(n + 1.0) - special.gammaln(k + 1.0)
                  - special.gammaln(n - k + 1.0) + k * np.log(mu) + (n - k) * np.log(1.0 - mu))
            return np.where(n == 0.0, 0.0, ll)
        if self.family == "poisson":
            k = np.trunc(y)
            return w * (k * np.log(mu) - mu - special.gammaln(k + 1.0))
        if self.family == "gamma":
            a, s = 1.0 / dispersion, mu * dispersion
            return w * ((a - 1.0) * np.log(y) - y / s - special.gammaln(a) - a * np.log(s))
        return np.zeros_like(mu)

    # links
    def linkf(self, mu):
        return {"identity": lambda: mu, "log": lambda: np.log(mu), "inverse": lambda: 1.0 / mu,
                "logit": lambda: np.log(mu / (1.0 - mu)), "probit": lambda: special.ndtri(mu),
                "cloglog": lambda: np.log(-np.log(1.0 - mu)), "sqrt": lambda: np.sqrt(mu),
                "power": lambda: mu ** self.lp}[self.link]()

    def deriv(self, mu):
        return {"identity": lambda: np.ones_like(mu), "log": lambda: 1.0 / mu,
                "inverse": lambda: -1.0 / (mu * mu), "logit": lambda: 1.0 / (mu * (1.0 - mu)),
                "probit": lambda: 1.0 / (np.exp(-0.5 * special.ndtri(mu) ** 2)
                                         / math.sqrt(2.0 * math.pi)),
                "cloglog": lambda: 1.0 / ((mu - 1.0) * np.log(1.0 - mu)),
                "sqrt": lambda: 1.0 / (2.0 * np.sqrt(mu)),
                "power": lambda: self.lp * mu ** (self.lp - 1.0)}[self.link]()

    def unlink(self, eta):
        with np.errstate(over="ignore", divide="ignore"):
            return {"identity": lambda: eta, "log": lambda: np.exp(eta),
                    "inverse": lambda: 1.0 / eta, "logit": lambda: 1.0 / (1.0 + np.exp(-eta)),
                    "probit": lambda: special.ndtr(eta),
                    "cloglog": lambda: 1.0 - np.exp(-np.exp(eta)), "sqrt": lambda: eta * eta,
                    "power": lambda: eta ** (1.0 / self.lp)}[self.link]()

    # the passes
    def eta(self, X, coef, intercept, off):
        dot = 0.0 if coef is None else (
            X.astype(np.longdouble) @ np.asarray(coef, dtype=np.longdouble)).astype(np.float64)
        return dot + intercept + off

    def init_pass(self, y, w, off):
        return self.linkf(self.initialize(y, w)) - off, w.copy()

    def step_pass(self, X, y, w, off, coef, intercept):
        eta = self.eta(X, coef, intercept, off)
        mu = self.project(self.unlink(eta))
        g = self.deriv(mu)
        z = eta - off + (y - mu) * g
        wz = w / (g * g * self.variance(mu))
        dead = w == 0.0
        return np.where(dead, 0.0, z), np.where(dead, 0.0, wz), mu

    def stats(self, X, y, w, off, coef, intercept, project=True, dispersion=1.0):
        """(the six sums, sum |term| of each)."""
        mu = self.unlink(self.eta(X, coef, intercept, off))
        if project:
            mu = self.project(mu)
        with np.errstate(divide="ignore"):
            terms = [w, w * y, self.deviance(y, mu, w), w * (y - mu) ** 2 / self.variance(mu),
                     self.loglik(y, mu, w, dispersion), np.log(w)]
        return (np.array([math.fsum(t) for t in terms]),
                np.array([math.fsum(np.abs(t)) for t in terms]))


def moments_ld(X, y, w):
    Z = np.column_stack([X, y, np.ones(len(y))]).astype(np.longdouble)
    return ((Z * w.astype(np.longdouble)[:, None]).T @ Z).astype(np.float64)


def pack(M):
    j, i = np.tril_indices(M.shape[0])
    return np.ascontiguousarray(M[i, j])


def system(M, k, fitIntercept, regParam, standardized):
    """The k x k system WeightedLeastSquares.solve factors for the
    coefficients from full moments M (the intercept row eliminated): its
    condition number scales the fits' tolerance, as in tests/test_wls_gpu.py.
    standardized: the first fit (features and label standardized); the IRLS
    fits are not, which leaves regParam / aStd^2 on the diagonal."""
    ws = M[k + 1, k + 1]
    aBar, bBar = M[:k, k + 1] / ws, M[k, k + 1] / ws
    aStd = np.sqrt(np.diag(M[:k, :k]) / ws - aBar ** 2)
    bStd = np.sqrt(M[k, k] / ws - bBar ** 2)
    lam = regParam / bStd * np.ones(k) if standardized else regParam / aStd ** 2
    S = M[:k, :k] / ws / np.outer(aStd, aStd) + np.diag(lam)
    if fitIntercept:
        S = S - np.outer(aBar / aStd, aBar / aStd)
    return S


def fit_ref(ref, X, y, w, off, fitIntercept=True, regParam=0.0, maxIter=25, tol=1e-6):
    """GeneralizedLinearRegression.fit restated: dict with coefficients,
    intercept, diagInvAtWA, numIterations and cond, the condition number of
    the last WLS fit's system."""
    n, k = X.shape
    first = WeightedLeastSquares(fitIntercept, regParam, 0.0, True, True)
    if ref.family == "gaussian" and ref.link == "identity":
        M = moments_ld(X, y - off, w)
        m = first.solve(pack(M), k, count=n)
        return {"coefficients": m.coefficients, "intercept": m.intercept,
                "diagInvAtWA": m.diagInvAtWA, "numIterations": 0,
                "cond": np.linalg.cond(system(M, k, fitIntercept, regParam, True))}
    z, wz = ref.init_pass(y, w, off)
    M = moments_ld(X, z, wz)
    model = first.solve(pack(M), k, count=n)
    wls = WeightedLeastSquares(fitIntercept, regParam, 0.0, False, False)
    it, converged = 0, False
    while it < maxIter and not converged:
        old = model
        z, wz, _ = ref.step_pass(X, y, w, off, old.coefficients, old.intercept)
        M = moments_ld(X, z, wz)
        model = wls.solve(pack(M), k, count=n)
        maxTol = max(np.abs(old.coefficients - model.coefficients).max(),
                     abs(old.intercept - model.intercept))
        converged = maxTol < tol
        it += 1
    return {"coefficients": model.coefficients, "intercept": model.intercept,
            "diagInvAtWA": model.diagInvAtWA, "numIterations": it,
            "cond": np.linalg.cond(system(M, k, fitIntercept, regParam, False))}


def null_intercept_ref(ref, y, w, off, hasOffset, fitIntercept, maxIter, tol):
    if not fitIntercept:
        return 0.0
    if not hasOffset:
        return float(ref.linkf(np.array(np.sum(w * y) / np.sum(w))))
    if ref.family == "gaussian" and ref.link == "identity":
        return float(np.sum(w * (y - off)) / np.sum(w))
    z, wz = ref.init_pass(y, w, off)
    b = float(np.sum(wz * z) / np.sum(wz))
    it, converged = 0, False
    while it < maxIter and not converged:
        z, wz, _ = ref.step_pass(None, y, w, off, None, b)
        old, b = b, float(np.sum(wz * z) / np.sum(wz))
        converged = abs(old - b) < tol
        it += 1
    return b


def summary_ref(ref, X, y, w, off, fit, fitIntercept, hasOffset=True, maxIter=25, tol=1e-6):
    """The training summary of a fit_ref result."""
    n, k = X.shape
    coef, b = fit["coefficients"], fit["intercept"]
    s, _ = ref.stats(X, y, w, off, coef, b)
    rank = k + int(fitIntercept)
    dof = n - rank
    out = {"numInstances": n, "rank": rank, "degreesOfFreedom": dof,
           "residualDegreeOfFreedomNull": n - int(fitIntercept), "deviance": s[2]}
    b0 = null_intercept_ref(ref, y, w, off, hasOffset, fitIntercept, maxIter, tol)
    out["nullDeviance"] = ref.stats(X, y, w, off, None, b0, project=False)[0][2]
    out["dispersion"] = 1.0 if ref.family in ("binomial", "poisson") else s[3] / dof
    if ref.family == "gaussian":
        out["aic"] = n * (math.log(s[2] / n * 2.0 * math.pi) + 1.0) + 2.0 - s[5] + 2 * rank
    elif ref.family == "gamma":
        ll = ref.stats(X, y, w, off, coef, b, dispersion=s[2] / s[0])[0][4]
        out["aic"] = -2.0 * ll + 2.0 + 2 * rank
    elif ref.family != "tweedie":
        out["aic"] = -2.0 * s[4] + 2 * rank
    d = fit["diagInvAtWA"]
    if not (d.shape == (1,) and d[0] == 0.0):
        se = np.sqrt(d * out["dispersion"])
        t = (np.append(coef, b) if fitIntercept else coef) / se
        out["coefficientStandardErrors"], out["tValues"] = se, t
        if ref.paramFamily in ("binomial", "poisson"):
            out["pValues"] = 2.0 * special.ndtr(-np.abs(t))
        else:
            out["pValues"] = 2.0 * special.stdtr(float(dof), -np.abs(t))
    return out


@functools.lru_cache(maxsize=None)
def case(n, p, family, link=None, variancePower=0.0, integerWeights=False, density=None,
         linkPower=None):
    """Seeded rows for a pair: X, w, offset, the coefficients and intercept
    that put eta = X coef + intercept + offset in the link's ETA_RANGE, the
    reference's mu there and labels drawn around it.  density: that share of
    nonzeros, with row 7 empty and row 11 fully dense.  Read-only, shared."""
    ref = Ref(family, link, variancePower, linkPower)
    rng = np.random.default_rng(1000 * p + n)
    X = rng.normal(size=(n, p)) * rng.uniform(0.5, 2, size=p) + rng.uniform(-1, 1, size=p)
    if density is not None:
        keep = rng.uniform(size=(n, p)) < density
        keep[7], keep[11] = False, True
        X = np.where(keep, X, 0.0)
    w = rng.integers(1, 5, size=n).astype(np.float64) if integerWeights else rng.uniform(0.5, 2, size=n)
    off = rng.uniform(-0.05, 0.05, size=n)
    direction = rng.normal(size=p)
    raw = X @ direction
    centre, scale = ETA_RANGE[ref.link]
    sd = raw.std() if n > 1 and raw.std() > 0 else 1.0
    beta = direction * (scale / sd)
    intercept = centre - raw.mean() * scale / sd
    eta = ref.eta(X, beta, intercept, off)
    mu = ref.project(ref.unlink(eta))
    if ref.family == "binomial":
        y = (rng.binomial(w.astype(int), mu) / w) if integerWeights else rng.binomial(1, mu).astype(float)
    elif ref.family == "poisson":
        y = rng.poisson(mu).astype(np.float64)
    elif ref.family == "gamma":
        y = rng.gamma(2.0, mu / 2.0)
    elif ref.family == "tweedie":
        y = np.where(rng.uniform(size=n) < 0.3, 0.0, rng.gamma(2.0, mu / 2.0))
        if ref.vp >= 2.0:
            y = np.maximum(y, 0.01)
    else:
        y = mu + 0.3 * rng.normal(size=n)
    c = {"X": X, "y": y, "w": w, "off": off, "coef": beta, "intercept": float(intercept),
         "eta": eta, "mu": mu}
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    c["ref"] = ref
    return c


# ---------------------------------------------------------------- parameters
@pytest.mark.parametrize("kw,msg", [
    ({"family": "gaussian", "link": "logit"},
     "requirement failed: Generalized Linear Regression with gaussian family does not support "
     "logit link function."),
    ({"family": "binomial", "link": "log"},
     "requirement failed: Generalized Linear Regression with binomial family does not support "
     "log link function."),
    ({"family": "poisson", "link": "inverse"},
     "requirement failed: Generalized Linear Regression with poisson family does not support "
     "inverse link function."),
    ({"family": "gamma", "link": "sqrt"},
     "requirement failed: Generalized Linear Regression with gamma family does not support "
     "sqrt link function."),
    ({"family": "tweedie", "link": "log"},
     "requirement failed: When family is tweedie, use param linkPower to specify link function; "
     "param link must not be set."),
    ({"family": "tweedie", "variancePower": 0.5},
     "requirement failed: variancePower must be 0.0 or in [1, inf) but got 0.5"),
    ({"regParam": -0.1}, "requirement failed: regParam cannot be negative: -0.1"),
    ({"maxIter": 0}, "requirement failed: maxIter must be a positive integer: 0"),
    ({"solver": "x"}, "GeneralizedLinearRegression: unsupported solver x"),
])
def test_parameter_errors(kw, msg):
    with pytest.raises(IllegalArgumentException) as e:
        GeneralizedLinearRegression(**kw)
    assert str(e.value) == msg


def test_every_legal_pair_and_the_defaults_construct():
    for family, link in PAIRS:
        assert GeneralizedLinearRegression(family=family, link=link).familyAndLink.link == link
    for family, link in [("gaussian", "identity"), ("binomial", "logit"), ("poisson", "log"),
                         ("gamma", "inverse")]:
        assert GeneralizedLinearRegression(family=family).familyAndLink.link == link
    fl = GeneralizedLinearRegression(family="tweedie", variancePower=1.5).familyAndLink
    assert (fl.family, fl.link, fl.linkPower) == ("tweedie", "power", -0.5)
    for vp, family in [(0.0, "gaussian"), (1.0, "poisson"), (2.0, "gamma")]:
        fl = GeneralizedLinearRegression(family="tweedie", variancePower=vp,
                                         linkPower=0.0).familyAndLink
        assert (fl.family, fl.link) == (family, "log")


def test_host_link_functions_match_the_restatement():
    """FamilyAndLink's one-value link, unlink and project (predict of one
    vector, the null model's intercept) against the restatement's arrays."""
    for family, link in PAIRS + [("tweedie", None)]:
        ref = Ref(family, link, 1.5)
        fl = GeneralizedLinearRegression(**ref.kwargs()).familyAndLink
        centre, scale = ETA_RANGE[ref.link]
        for eta in (centre - 2 * scale, centre, centre + 2 * scale):
            mu = float(ref.unlink(np.array(eta)))
            assert fl.unlink(eta) == pytest.approx(mu, rel=1e-13)
            assert fl.link_fn(mu) == pytest.approx(float(ref.linkf(np.array(mu))), rel=1e-12,
                                                   abs=1e-13)
        for mu in (-1.0, 0.0, 0.5, 1.0, 2.0, math.inf):
            assert fl.project(mu) == float(ref.project(np.array(mu)))
    fl = GeneralizedLinearRegression(family="binomial").familyAndLink
    assert fl.project(fl.unlink(-800.0)) == EPS and fl.project(fl.unlink(800.0)) == 1.0 - EPS
    fl = GeneralizedLinearRegression(family="poisson").familyAndLink
    assert fl.project(fl.unlink(800.0)) == np.finfo(np.float64).max


# ------------------------------------------------- restatement vs scikit-learn
@pytest.mark.parametrize("which", ["poisson", "gamma", "binomial"])
def test_restatement_against_scikit_learn(which):
    lm = pytest.importorskip("sklearn.linear_model")
    link = {"poisson": "log", "gamma": "log", "binomial": "logit"}[which]
    c = case(300, 7, which, link)
    X, y, w = c["X"], c["y"], c["w"]
    fit = fit_ref(c["ref"], X, y, w, np.zeros(300), maxIter=100, tol=1e-12)
    if which == "binomial":
        sk = lm.LogisticRegression(penalty=None, tol=1e-12, max_iter=10000).fit(X, y, sample_weight=w)
        coef, b = sk.coef_[0], sk.intercept_[0]
    else:
        cls = lm.PoissonRegressor if which == "poisson" else lm.GammaRegressor
        sk = cls(alpha=0, tol=1e-12, max_iter=10000).fit(X, y, sample_weight=w)
        coef, b = sk.coef_, sk.intercept_
    err = max(np.abs(coef - fit["coefficients"]).max(), abs(b - fit["intercept"]))
    print(f"{which}: IRLS iterations {fit['numIterations']}, max |d| vs scikit-learn {err:.3g}")
    assert fit["numIterations"] < 100
    assert err <= 1e-6


# ------------------------------------------------------------ summary formulas
def _fit_and_summary(family, link, vp=0.0, integerWeights=False):
    c = case(300, 7, family, link, vp, integerWeights)
    fit = fit_ref(c["ref"], c["X"], c["y"], c["w"], c["off"])
    s = summary_ref(c["ref"], c["X"], c["y"], c["w"], c["off"], fit, True)
    mu = c["ref"].project(c["ref"].unlink(c["ref"].eta(c["X"], fit["coefficients"],
                                                      fit["intercept"], c["off"])))
    return c, s, mu


def test_poisson_deviance_and_aic_closed_forms():
    c, s, mu = _fit_and_summary("poisson", "log")
    y, w = c["y"], c["w"]

    def ll(m):
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.sum(w * (np.where(y == 0, 0.0, y * np.log(m)) - m - special.gammaln(y + 1)))
    assert s["deviance"] == pytest.approx(2 * (ll(np.where(y == 0, 1e-300, y)) - ll(mu)), rel=1e-11)
    assert s["aic"] == pytest.approx(-2 * ll(mu) + 2 * 8, rel=1e-12)
    assert s["dispersion"] == 1.0


def test_binomial_deviance_and_aic_closed_forms():
    c, s, mu = _fit_and_summary("binomial", "logit", integerWeights=True)
    n = c["w"]
    k = np.rint(c["y"] * n)

    def ll(m):
        with np.errstate(divide="ignore", invalid="ignore"):
            a = np.where(k == 0, 0.0, k * np.log(m)) + np.where(k == n, 0.0, (n - k) * np.log1p(-m))
        return np.sum(special.gammaln(n + 1) - special.gammaln(k + 1) - special.gammaln(n - k + 1) + a)
    assert s["deviance"] == pytest.approx(2 * (ll(k / n) - ll(mu)), rel=1e-11)
    assert s["aic"] == pytest.approx(-2 * ll(mu) + 2 * 8, rel=1e-12)


def test_gamma_deviance_and_aic_closed_forms():
    c, s, mu = _fit_and_summary("gamma", "log")
    y, w = c["y"], c["w"]
    disp = s["deviance"] / w.sum()        # Gamma.aic's dispersion: deviance / weightSum

    def ll(m):
        a = 1.0 / disp
        return np.sum(w * (a * np.log(a * y / m) - a * y / m - np.log(y) - special.gammaln(a)))
    assert s["deviance"] == pytest.approx(2 * disp * (ll(y) - ll(mu)), rel=1e-10)
    assert s["aic"] == pytest.approx(-2 * ll(mu) + 2 + 2 * 8, rel=1e-11)
    pearson = np.sum(w * (y - mu) ** 2 / mu ** 2)
    assert s["dispersion"] == pytest.approx(pearson / (300 - 8), rel=1e-12)


def test_gaussian_deviance_and_aic_closed_forms():
    c, s, mu = _fit_and_summary("gaussian", "log")
    y, w = c["y"], c["w"]
    rss = np.sum(w * (y - mu) ** 2)
    sigma2 = rss / 300
    # the weighted normal log-likelihood at the ML variance; + 1 parameter for it
    ll = np.sum(0.5 * np.log(w) - 0.5 * math.log(2 * math.pi * sigma2) - w * (y - mu) ** 2 / (2 * sigma2))
    assert s["deviance"] == pytest.approx(rss, rel=1e-12)
    assert s["aic"] == pytest.approx(-2 * ll + 2 * (8 + 1), rel=1e-12)


def test_tweedie_deviance_meets_poisson_and_gamma_at_the_ends():
    """variancePower -> 1 is the Poisson deviance (zero labels included: the
    first term is y * yp(max(y, delta), ...), which vanishes there) and
    variancePower -> 2 the Gamma deviance; no AIC for tweedie."""
    c = case(300, 7, "tweedie", None, 1.5)
    y, w, mu = c["y"], c["w"], c["mu"]
    assert (y == 0).sum() > 30
    # labels in (0, delta) are lifted to delta inside the first term: not Poisson's
    at = (y == 0) | (y >= DELTA)
    near1 = Ref("tweedie", variancePower=1.0 + 1e-7).deviance(y[at], mu[at], w[at])
    np.testing.assert_allclose(near1, Ref("poisson").deviance(y[at], mu[at], w[at]), rtol=1e-5,
                               atol=1e-6)
    pos = y > 0
    near2 = Ref("tweedie", variancePower=2.0 + 1e-7).deviance(y[pos], mu[pos], w[pos])
    np.testing.assert_allclose(near2, Ref("gamma").deviance(y[pos], mu[pos], w[pos]), rtol=1e-5,
                               atol=1e-6)
    fit = fit_ref(c["ref"], c["X"], y, w, c["off"])
    assert "aic" not in summary_ref(c["ref"], c["X"], y, w, c["off"], fit, True)
