"""GPU: GeneralizedLinearRegression's device passes (k_glm_rows, k_glm_init,
k_glm_stats through cyc_glm_*) against the numpy restatement of
tests/test_glm_host.py, and its fit, predictions and training summary end to
end.

Bars.  Reweight and INIT: |dz| <= 1e-10 max(1, |z|), |dw'| <= 1e-10 w' with
the inputs kept where no project clamp acts (asserted on the reference
first): the dot's rounding, p eps sum |x_j b_j| (about 1e-12 at p = 4096),
leaves two orders of margin.  Stats: 1e-10 of sum |term| per sum, and two
calls bitwise equal.  Fits: 2e-10 cond max|coef| with cond, the condition
number of the last iteration's reference system, asserted <= 1e3 (the
end-to-end bar of tests/test_wls_gpu.py).

Dense shapes: besides the edges of the 64-row batch and of more than one
block, every width at which the launch geometry changes: 8 | 9, 16 | 17 and
32 | 33 (8, 16, 32 or 64 lanes per row, so 8, 4, 2 or 1 rows of a wave in
flight) and 64 | 65 (one or more features per lane).
"""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_glm_host as H  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (40, 1), (300, 7), (300, 8), (300, 9), (300, 16), (300, 17), (300, 32),
          (300, 33), (2600, 63), (2600, 64), (2600, 65), (4099, 130), (4099, 257), (70, 4096)]
# (family, link, variancePower): run at every shape / only at (300, 7)
EVERYWHERE = [("poisson", "log", 0.0), ("binomial", "logit", 0.0), ("binomial", "probit", 0.0),
              ("gamma", "inverse", 0.0), ("tweedie", None, 1.5)]
ALL_PAIRS = [(f, l, 0.0) for f, l in H.PAIRS] + [("tweedie", None, 1.5)]
REWEIGHT_CASES = [(n, p) + fl for n, p in SHAPES for fl in EVERYWHERE] + [
    (300, 7) + fl for fl in ALL_PAIRS if fl not in EVERYWHERE]
FAMILIES = [("gaussian", "identity", 0.0), ("binomial", "logit", 0.0), ("poisson", "log", 0.0),
            ("gamma", "inverse", 0.0), ("tweedie", None, 1.5)]


def _dev(a, cuda):
    import torch
    if a is None:
        return None
    return torch.from_numpy(np.array(a, dtype=np.float64, order="C")).to(cuda)


def _csr(X, cuda):
    import torch
    from cycloneml_amd.linalg import CSRRows
    nz = X != 0.0
    rowptr = np.concatenate([[0], np.cumsum(nz.sum(1))]).astype(np.int64)
    colidx = np.nonzero(nz)[1].astype(np.int32)
    return CSRRows(torch.from_numpy(rowptr).to(cuda), torch.from_numpy(colidx).to(cuda),
                   _dev(X[nz], cuda), X.shape[1])


def _plan(ref, p):
    from cycloneml_amd.glm import FamilyAndLink, GLMPlan
    kw = ref.kwargs()
    return GLMPlan(FamilyAndLink(kw["family"], kw.get("link"), kw.get("variancePower", 0.0),
                                 kw.get("linkPower")), p)


def _assert_in_range(ref, eta, mu):
    if ref.family == "binomial":
        assert mu.min() >= 0.02 and mu.max() <= 0.98, (mu.min(), mu.max())
    elif ref.family != "gaussian":
        assert mu.min() >= 0.05 and mu.max() <= 50.0, (mu.min(), mu.max())
    if ref.link in ("inverse", "sqrt", "power"):
        assert eta.min() > 0.1, eta.min()


def _assert_zw(z, wz, zr, wr, what):
    rz = float((np.abs(z - zr) / np.maximum(1.0, np.abs(zr))).max())
    rw = float((np.abs(wz - wr) / wr).max()) if (wr != 0).all() else float(
        (np.abs(wz - wr) / np.where(wr == 0, 1.0, wr)).max())
    print(f"{what}: worst |dz| / max(1, |z|) = {rz:.3g}, worst |dw'| / w' = {rw:.3g} (bar 1e-10)")
    assert np.isfinite(z).all() and np.isfinite(wz).all(), what
    assert rz <= 1e-10 and rw <= 1e-10, what


def _device_reweight(cuda, plan, rows, y, w, off, coef, intercept, init=False):
    import torch
    n = len(y)
    z = torch.full((n,), np.nan, dtype=torch.float64, device=cuda)
    wz = torch.full((n,), np.nan, dtype=torch.float64, device=cuda)
    plan.reweight(rows, _dev(y, cuda), _dev(w, cuda), _dev(off, cuda), _dev(coef, cuda),
                  intercept, z, wz, init=init)
    return z.cpu().numpy(), wz.cpu().numpy()


def _check_variants(cuda, c, rows, what):
    """The three input variants of a STEP pass: w and offset, no w, no offset."""
    ref, X, y = c["ref"], c["X"], c["y"]
    n, p = X.shape
    plan = _plan(ref, p)
    out = {}
    for name, w, off in (("both", c["w"], c["off"]), ("w null", None, c["off"]),
                         ("offset null", c["w"], None)):
        wr = np.ones(n) if w is None else w
        offr = np.zeros(n) if off is None else off
        zr, wzr, mu = ref.step_pass(X, y, wr, offr, c["coef"], c["intercept"])
        _assert_in_range(ref, ref.eta(X, c["coef"], c["intercept"], offr), mu)
        z, wz = _device_reweight(cuda, plan, rows, y, w, off, c["coef"], c["intercept"])
        _assert_zw(z, wz, zr, wzr, f"{what} {ref.family}/{ref.link} {n} x {p}, {name}")
        out[name] = (z, wz)
    plan.close()
    return out


@pytest.mark.parametrize("n,p,family,link,vp", REWEIGHT_CASES)
def test_reweight_dense(cuda, n, p, family, link, vp):
    c = H.case(n, p, family, link, vp)
    _check_variants(cuda, c, _dev(c["X"], cuda), "dense")


@pytest.mark.parametrize("family,link,vp", EVERYWHERE)
def test_reweight_csr(cuda, family, link, vp):
    """(4099, 130) at 10 % density, row 7 empty and row 11 fully dense,
    against the restatement and against the dense path on the densified
    rows."""
    c = H.case(4099, 130, family, link, vp, density=0.10)
    X = c["X"]
    assert (X[7] == 0).all() and (X[11] != 0).all()
    assert 0.08 < (X != 0).mean() < 0.12
    sparse = _check_variants(cuda, c, _csr(X, cuda), "CSR")
    dense = _check_variants(cuda, c, _dev(X, cuda), "densified")
    for name in sparse:
        _assert_zw(*sparse[name], *dense[name], f"CSR vs dense, {name}")


def test_zero_weight_rows_are_not_read(cuda):
    """Rows of weight 0 hold NaN and Inf features: z = 0 and w' = 0 there,
    dense and CSR, and the fit is finite: that of the other rows."""
    from cycloneml_amd import GeneralizedLinearRegression
    c = H.case(300, 7, "poisson", "log")
    ref = c["ref"]
    X, w = c["X"].copy(), c["w"].copy()
    dead = np.zeros(300, dtype=bool)
    dead[[0, 5, 17, 63, 64, 150, 299]] = True
    w[dead] = 0.0
    X[dead] = np.nan
    X[dead, ::2] = np.inf
    plan = _plan(ref, 7)
    live = ~dead
    zr, wzr, _ = ref.step_pass(c["X"], c["y"], w, c["off"], c["coef"], c["intercept"])
    for rows, what in ((_dev(X, cuda), "dense"), (_csr(X, cuda), "CSR")):
        z, wz = _device_reweight(cuda, plan, rows, c["y"], w, c["off"], c["coef"], c["intercept"])
        assert (z[dead] == 0.0).all() and (wz[dead] == 0.0).all(), what
        _assert_zw(z[live], wz[live], zr[live], wzr[live], f"zero-weight rows, {what}")
    plan.close()
    m = GeneralizedLinearRegression(family="poisson", maxIter=8, tol=0.0).fit(
        _dev(X, cuda), _dev(c["y"], cuda), _dev(w, cuda), _dev(c["off"], cuda))
    want = H.fit_ref(ref, c["X"][live], c["y"][live], w[live], c["off"][live], maxIter=8, tol=0.0)
    got = np.append(m.coefficients, m.intercept)
    assert np.isfinite(got).all()
    tol = 2e-10 * want["cond"] * np.abs(want["coefficients"]).max()
    assert np.abs(got - np.append(want["coefficients"], want["intercept"])).max() <= tol
    assert np.isfinite(m.summary.deviance)


@pytest.mark.parametrize("family,link,vp", FAMILIES)
@pytest.mark.parametrize("n,p", [(300, 7), (4099, 130)])
def test_init_pass(cuda, n, p, family, link, vp):
    c = H.case(n, p, family, link, vp)
    ref = c["ref"]
    plan = _plan(ref, p)
    X = _dev(c["X"], cuda)
    for w, off in ((c["w"], c["off"]), (None, c["off"]), (c["w"], None)):
        zr, wzr = ref.init_pass(c["y"], np.ones(n) if w is None else w,
                                np.zeros(n) if off is None else off)
        z, wz = _device_reweight(cuda, plan, X, c["y"], w, off, None, 0.0, init=True)
        _assert_zw(z, wz, zr, wzr, f"INIT {family} {n} x {p}")
        assert np.array_equal(wz, wzr)
    plan.close()


@pytest.mark.parametrize("family,link,vp,bad", [("poisson", "log", 0.0, -1.0),
                                                ("gamma", "inverse", 0.0, 0.0),
                                                ("binomial", "logit", 0.0, 1.5),
                                                ("tweedie", None, 1.5, -1.0),
                                                ("tweedie", None, 2.5, 0.0)])
def test_label_outside_the_domain_raises(cuda, family, link, vp, bad):
    from cycloneml_amd import GeneralizedLinearRegression
    from cycloneml_amd._native import IllegalArgumentException
    c = H.case(300, 7, family, link, vp)
    ref = c["ref"]
    y = c["y"].copy()
    y[123] = bad
    plan = _plan(ref, 7)
    X = _dev(c["X"], cuda)
    for init in (True, False):
        with pytest.raises(IllegalArgumentException, match="requirement failed: The response"):
            _device_reweight(cuda, plan, X, y, c["w"], c["off"], c["coef"], c["intercept"], init)
    plan.close()
    with pytest.raises(IllegalArgumentException, match="requirement failed: The response"):
        GeneralizedLinearRegression(**ref.kwargs()).fit(X, _dev(y, cuda))


def test_illegal_pairs_fail_at_plan_creation(cuda):
    import ctypes
    from cycloneml_amd import _native as N
    lib = N.load()
    h = ctypes.c_void_p()
    for args in ((0, 3, 0.0, 0.0, 7), (1, 1, 0.0, 0.0, 7), (4, 1, 1.5, 0.0, 7),
                 (4, 7, 0.5, 0.0, 7), (2, 1, 0.0, 0.0, 0), (2, 1, 0.0, 0.0, 4097)):
        assert lib.cyc_glm_plan_create(*args, ctypes.byref(h)) == N.CYC_ERR_INVALID_ARG, args
        assert lib.cyc_last_error().startswith(b"requirement failed:")
    assert lib.cyc_glm_plan_create(2, 1, 0.0, 0.0, 4096, ctypes.byref(h)) == N.CYC_OK
    # nrows == 0 is a no-op
    assert lib.cyc_glm_reweight_dev(h, None, 0, None, None, None, None, 0.0, 0, None, None,
                                    None) == N.CYC_OK
    assert lib.cyc_glm_plan_destroy(h) == N.CYC_OK


@pytest.mark.parametrize("family", ["binomial", "poisson"])
def test_predict_clamps(cuda, family):
    """eta = +-800: unlink leaves the double range and project puts the mean
    back, exactly as the numpy expression does."""
    from cycloneml_amd.glm import FamilyAndLink, GeneralizedLinearRegressionModel
    ref = H.Ref(family)
    X = np.zeros((4, 3))
    X[:, 0] = [800.0, -800.0, 0.0, 1.0]
    coef = np.array([1.0, 0.0, 0.0])
    m = GeneralizedLinearRegressionModel(coef, 0.0, FamilyAndLink(family, None, 0.0, None))
    want = ref.project(ref.unlink(X @ coef))
    got = m.predict(_dev(X, cuda)).cpu().numpy()
    assert np.array_equal(got[:2], want[:2]), (got, want)
    np.testing.assert_allclose(got[2:], want[2:], rtol=1e-14)
    lo, hi = (H.EPS, 1.0 - H.EPS) if family == "binomial" else (H.EPS, np.finfo(np.float64).max)
    assert got[0] == hi and got[1] == lo
    assert np.array_equal(m.predictLink(_dev(X, cuda)).cpu().numpy(), X @ coef)
    assert np.array_equal(m.predict(_csr(X, cuda)).cpu().numpy(), got)
    for i in range(4):
        assert m.predict(X[i]) == pytest.approx(want[i], rel=1e-14)


@pytest.mark.parametrize("family,link,vp", FAMILIES)
@pytest.mark.parametrize("n,p", [(300, 7), (4099, 130)])
def test_stats_pass(cuda, n, p, family, link, vp):
    import torch
    dense = H.case(n, p, family, link, vp)
    sparse = H.case(n, p, family, link, vp, density=0.10) if n > 7 else dense
    for c, what in ((dense, "dense"), (sparse, "CSR")):
        ref = c["ref"]
        plan = _plan(ref, p)
        rows = _dev(c["X"], cuda) if what == "dense" else _csr(c["X"], cuda)
        y, w, off = (_dev(c[k], cuda) for k in ("y", "w", "off"))
        for coef, b, project, disp in ((c["coef"], c["intercept"], True, 0.7),
                                       (c["coef"], c["intercept"], False, 1.0),
                                       (None, H.ETA_RANGE[ref.link][0], False, 1.0)):
            want, scale = ref.stats(c["X"], c["y"], c["w"], c["off"], coef, b, project, disp)
            got = []
            for _ in range(2):
                s = torch.full((6,), np.nan, dtype=torch.float64, device=cuda)
                plan.stats(rows, y, w, off, _dev(coef, cuda), b, s, project=project,
                           dispersion=disp)
                got.append(s.cpu().numpy())
            assert np.array_equal(got[0], got[1]), f"{what}: two calls differ"
            ratio = np.abs(got[0] - want) / np.where(scale == 0, 1.0, scale)
            print(f"stats {family} {n} x {p} {what}: worst |d| / sum |term| = {ratio.max():.3g}")
            assert (ratio <= 1e-10).all(), (got[0], want)
        plan.close()


# ------------------------------------------------------------------------ fits
# (family, link, variancePower, linkPower).  tweedie(1.5) is fitted with the
# log link (linkPower 0): under its default power link, -0.5, mu = eta^-2 and
# a fit without an intercept has eta near 0 on these rows (reference system's
# cond 3e12, against the 1e3 the bar is stated for), and with one the IRLS
# from the initial model does not settle on the 30 % of zero labels (cond
# 6e11).  The default link is covered by the reweight tests at every shape.
FIT_COMBOS = {"poisson+offset": ("poisson", "log", 0.0, None),
              "binomial": ("binomial", "logit", 0.0, None),
              "gamma/log": ("gamma", "log", 0.0, None),
              "tweedie": ("tweedie", None, 1.5, 0.0),
              "gaussian": ("gaussian", "identity", 0.0, None)}


@functools.lru_cache(maxsize=None)
def _fit_case(n, p, combo, fitIntercept, regParam, maxIter=8, tol=0.0):
    """(case, offset or None, the restatement's fit): computed once, shared
    by the fit and summary tests."""
    family, link, vp, lp = FIT_COMBOS[combo]
    c = H.case(n, p, family, link, vp, linkPower=lp)
    off = c["off"] if combo in ("poisson+offset", "gaussian") else None
    fit = H.fit_ref(c["ref"], c["X"], c["y"], c["w"], np.zeros(n) if off is None else off,
                    fitIntercept, regParam, maxIter, tol)
    return c, off, fit


def _device_fit(cuda, c, off, fitIntercept, regParam, **kw):
    from cycloneml_amd import GeneralizedLinearRegression
    est = GeneralizedLinearRegression(fitIntercept=fitIntercept, regParam=regParam,
                                      **c["ref"].kwargs(), **kw)
    return est.fit(_dev(c["X"], cuda), _dev(c["y"], cuda), _dev(c["w"], cuda), _dev(off, cuda))


@pytest.mark.parametrize("regParam", [0.0, 0.3])
@pytest.mark.parametrize("fitIntercept", [False, True])
@pytest.mark.parametrize("combo", list(FIT_COMBOS))
@pytest.mark.parametrize("n,p", [(2600, 63), (4099, 130)])
def test_fit_against_the_restatement(cuda, n, p, combo, fitIntercept, regParam):
    c, off, ref = _fit_case(n, p, combo, fitIntercept, regParam)
    assert ref["cond"] <= 1e3, ref["cond"]
    m = _device_fit(cuda, c, off, fitIntercept, regParam, maxIter=8, tol=0.0)
    want = np.append(ref["coefficients"], ref["intercept"])
    got = np.append(m.coefficients, m.intercept)
    tol = 2e-10 * ref["cond"] * np.abs(want).max()
    print(f"{combo} {n} x {p} intercept {fitIntercept} reg {regParam}: cond {ref['cond']:.3g}, "
          f"max |dx| {np.abs(got - want).max():.3g}, tol {tol:.3g}")
    assert np.abs(got - want).max() <= tol
    assert m.numFeatures == p
    assert m.summary.numIterations == ref["numIterations"] == (0 if combo == "gaussian" else 8)
    if not fitIntercept:
        assert m.intercept == 0.0
    # the fitted mean and the linear predictor of the training rows
    R = c["ref"]
    offr = np.zeros(n) if off is None else off
    eta = R.eta(c["X"], m.coefficients, m.intercept, offr)
    Xd, offd = _dev(c["X"], cuda), _dev(off, cuda)
    np.testing.assert_allclose(m.predictLink(Xd, offd).cpu().numpy(), eta, rtol=1e-11, atol=1e-11)
    np.testing.assert_allclose(m.predict(Xd, offd).cpu().numpy(), R.project(R.unlink(eta)),
                               rtol=1e-10)


def test_fit_converges_before_max_iter(cuda):
    c, off, ref = _fit_case(2600, 63, "poisson+offset", True, 0.0, 25, 1e-6)
    m = _device_fit(cuda, c, off, True, 0.0)
    assert m.summary.numIterations == ref["numIterations"] < 25
    assert np.abs(m.coefficients - ref["coefficients"]).max() <= 2e-10 * ref["cond"] * np.abs(
        ref["coefficients"]).max()


def test_csr_fit_matches_dense(cuda):
    from cycloneml_amd import GeneralizedLinearRegression
    c = H.case(4099, 130, "poisson", "log", density=0.10)
    est = GeneralizedLinearRegression(family="poisson", maxIter=8, tol=0.0)
    y, w, off = (_dev(c[k], cuda) for k in ("y", "w", "off"))
    a = est.fit(_csr(c["X"], cuda), y, w, off)
    b = est.fit(_dev(c["X"], cuda), y, w, off)
    np.testing.assert_allclose(np.append(a.coefficients, a.intercept),
                               np.append(b.coefficients, b.intercept), rtol=0, atol=1e-10)
    assert a.summary.deviance == pytest.approx(b.summary.deviance, rel=1e-12)


# --------------------------------------------------------------------- summary
@pytest.mark.parametrize("combo", list(FIT_COMBOS))
def test_summary(cuda, combo):
    from scipy import special  # noqa: F401  (pValues' lazy import has to succeed)
    n, p = 2600, 63
    c, off, fit = _fit_case(n, p, combo, True, 0.0, 25, 1e-6)
    R = c["ref"]
    offr = np.zeros(n) if off is None else off
    want = H.summary_ref(R, c["X"], c["y"], c["w"], offr, fit, True, hasOffset=off is not None)
    m = _device_fit(cuda, c, off, True, 0.0)
    s = m.summary
    for k in ("numInstances", "rank", "degreesOfFreedom", "residualDegreeOfFreedomNull"):
        assert getattr(s, k) == want[k], k
    for k in ("deviance", "nullDeviance", "dispersion"):
        print(f"{combo} {k}: {getattr(s, k)!r} vs {want[k]!r}")
        assert getattr(s, k) == pytest.approx(want[k], rel=1e-9), k
    if combo == "tweedie":
        with pytest.raises(NotImplementedError, match="No AIC available for the tweedie family"):
            s.aic
    else:
        assert s.aic == pytest.approx(want["aic"], rel=1e-9)
    for k in ("coefficientStandardErrors", "tValues", "pValues"):
        assert getattr(s, k).shape == (p + 1,)
        np.testing.assert_allclose(getattr(s, k), want[k], rtol=1e-8, atol=0, err_msg=k)
    # residuals, elementwise on the fitted mean
    y, w = c["y"], c["w"]
    mu = R.project(R.unlink(R.eta(c["X"], m.coefficients, m.intercept, offr)))
    r = y - mu
    ref_res = {"response": r, "working": r * R.deriv(mu),
               "pearson": r / np.sqrt(R.variance(mu)) * np.sqrt(w),
               "deviance": np.sign(r) * np.sqrt(np.maximum(R.deviance(y, mu, w), 0.0))}
    for kind, ref in ref_res.items():
        np.testing.assert_allclose(s.residuals(kind).cpu().numpy(), ref, rtol=1e-7,
                                   atol=1e-9 * np.abs(ref).max(), err_msg=kind)


@pytest.mark.parametrize("fitIntercept,hasOffset", [(False, True), (True, False), (True, True)])
@pytest.mark.parametrize("combo", ["poisson+offset", "gamma/log", "gaussian"])
def test_null_deviance_three_intercepts(cuda, combo, fitIntercept, hasOffset):
    """b0 = 0 without an intercept, link(sum w y / sum w) with one and no
    offset, the intercept-only IRLS fit with both."""
    n, p = 300, 7
    c = H.case(n, p, *FIT_COMBOS[combo][:3])
    off = c["off"] * 10 if hasOffset else None
    offr = np.zeros(n) if off is None else off
    fit = H.fit_ref(c["ref"], c["X"], c["y"], c["w"], offr, fitIntercept)
    want = H.summary_ref(c["ref"], c["X"], c["y"], c["w"], offr, fit, fitIntercept, hasOffset)
    s = _device_fit(cuda, c, off, fitIntercept, 0.0).summary
    assert s.nullDeviance == pytest.approx(want["nullDeviance"], rel=1e-9)
    assert s.deviance == pytest.approx(want["deviance"], rel=1e-9)
    assert s.residualDegreeOfFreedomNull == n - int(fitIntercept)


@pytest.mark.parametrize("standardization", [False, True])
@pytest.mark.parametrize("fitIntercept", [False, True])
def test_gaussian_identity_is_the_linear_regression(cuda, fitIntercept, standardization):
    """The 4-row WeightedLeastSquaresSuite instances: gaussian / identity is
    LinearRegression(solver="normal")'s fit."""
    from cycloneml_amd import GeneralizedLinearRegression, LinearRegression
    A = np.array([[0.0, 5.0], [1.0, 7.0], [2.0, 11.0], [3.0, 13.0]])
    b = np.array([17.0, 19.0, 23.0, 29.0])
    w = np.array([1.0, 2.0, 3.0, 4.0])
    lr = LinearRegression(fitIntercept=fitIntercept, standardization=standardization,
                          solver="normal").fit(_dev(A, cuda), _dev(b, cuda), _dev(w, cuda))
    m = GeneralizedLinearRegression(fitIntercept=fitIntercept).fit(
        _dev(A, cuda), _dev(b, cuda), _dev(w, cuda))
    np.testing.assert_allclose(np.append(m.coefficients, m.intercept),
                               np.append(lr.coefficients, lr.intercept), rtol=0, atol=1e-12)
    assert m.summary.numIterations == 0
    want = (0.0, -3.727121, 3.009983) if not fitIntercept else (18.08, 6.08, -0.60)
    np.testing.assert_allclose([m.intercept, *m.coefficients], want, rtol=0, atol=1e-4)
