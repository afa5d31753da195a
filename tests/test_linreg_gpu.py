"""GPU: the evaluate pass of linear models (k_linreg_rows through
cyc_linreg_*) against the numpy restatement of tests/test_linreg_host.py,
LinearRegression's quasi-Newton fits over the device aggregators, and the
summary end to end.

Bars.  Stats: each sum within 1e-10 sum |term| of ref_stats (the dot's
rounding, p eps sum |x_j b_j|, leaves two orders of margin at p = 4096), the
extrema within 1e-10 max(1, |value|), pred within 1e-10 max(1, |p|), two
calls bitwise equal.  Fits: the bars measured in the host file.

Dense shapes: the edges of the 64-row batch and of more than one block, and
every width at which the launch geometry changes: 8 | 9, 16 | 17, 32 | 33
(lanes per row) and 64 | 65 (features per lane).  The coefficients leave LDS
for global memory above 8192 features: 8192 | 8193 dense, and the wide CSR
case.
"""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_linreg_host as H  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (40, 1), (300, 7), (300, 8), (300, 9), (300, 16), (300, 17), (300, 32),
          (300, 33), (2600, 63), (2600, 64), (2600, 65), (4099, 130), (4099, 257), (70, 4096),
          (70, 8192), (70, 8193)]
CSR_SHAPES = [(300, 7), (2600, 65), (4099, 257)]


def _dev(a, cuda, dtype=np.float64):
    import torch
    if a is None:
        return None
    return torch.from_numpy(np.array(a, dtype=dtype, order="C")).to(cuda)


def _csr_of(rowptr, colidx, vals, p, cuda):
    from cycloneml_amd.linalg import CSRRows
    return CSRRows(_dev(rowptr, cuda, np.int64), _dev(colidx, cuda, np.int32), _dev(vals, cuda), p)


def _csr(X, cuda):
    nz = X != 0.0
    rowptr = np.concatenate([[0], np.cumsum(nz.sum(1))])
    return _csr_of(rowptr, np.nonzero(nz)[1], X[nz], X.shape[1], cuda)


def _sum_ratio(o, ref, mags):
    """Worst |dsum| / sum |term| over the eight sums; a sum whose terms are all
    0 (one row at the centre) has to be 0 itself."""
    d = np.abs(o[:8] - ref[:8])
    assert (d[mags == 0.0] == 0.0).all()
    return float((d[mags > 0.0] / mags[mags > 0.0]).max())


@functools.lru_cache(maxsize=None)
def case(n, p, sparse=False):
    """Rows, labels, weights (a tenth of them 0 in the third variant), a model
    and a centre; CSR cases have about 30 % zeros."""
    rng = np.random.default_rng(100 * n + p + sparse)
    X = rng.normal(size=(n, p)) * 10.0 ** rng.uniform(-1.0, 1.0, p)
    if sparse:
        X[rng.random((n, p)) < 0.3] = 0.0
    coef = rng.normal(size=p) / (np.abs(X).max(0) + 1.0) / np.sqrt(p)
    b0 = 0.7
    y = X @ coef + b0 + 0.5 * rng.normal(size=n) + 2.0
    w = rng.uniform(0.25, 3.0, n)
    wz = w.copy()
    wz[rng.random(n) < 0.1] = 0.0
    if n > 1:
        wz[0], wz[n - 1] = 0.0, 1.5
    for a in (X, y, w, wz, coef):
        a.setflags(write=False)
    return {"X": X, "y": y, "w": w, "wz": wz, "coef": coef, "b0": b0, "center": float(y.mean())}


def _check_stats(cuda, rows_of, X, y, coef, b0, center, variants, what):
    """Every weight variant: the ten outputs and pred against ref_stats, a
    second call bitwise equal, and the call without pred the same ten."""
    from cycloneml_amd.regression_summary import linreg_predict, linreg_stats
    cd, yd = _dev(coef, cuda), _dev(y, cuda)
    for name, w in variants:
        Xv = X
        if name == "zeros":
            Xv = X.copy()
            Xv[w == 0.0] = np.nan          # a row of weight 0 reaches no output
        rows = rows_of(Xv)
        ref, mags, pref = H.ref_stats(X, y, w, coef, b0, center)
        out, pred = linreg_stats(rows, yd, _dev(w, cuda), cd, b0, center, want_pred=True)
        out2, pred2 = linreg_stats(rows, yd, _dev(w, cuda), cd, b0, center, want_pred=True)
        out3, none = linreg_stats(rows, yd, _dev(w, cuda), cd, b0, center)
        o, pr = out.cpu().numpy(), pred.cpu().numpy()
        assert none is None
        assert np.array_equal(o, out2.cpu().numpy()) and np.array_equal(o, out3.cpu().numpy())
        assert np.array_equal(pr, pred2.cpu().numpy(), equal_nan=True)
        assert np.isfinite(o).all(), (what, name, o)
        live = np.ones(len(y), bool) if w is None else w != 0.0
        rs = _sum_ratio(o, ref, mags)
        re = float((np.abs(o[8:] - ref[8:]) / np.maximum(1.0, np.abs(ref[8:]))).max())
        rp = float((np.abs(pr[live] - pref[live]) / np.maximum(1.0, np.abs(pref[live]))).max())
        print(f"{what}, {name}: worst |dsum| / sum|term| = {rs:.3g}, extrema {re:.3g}, "
              f"pred {rp:.3g} (bar 1e-10)")
        assert np.isfinite(pr[live]).all()
        assert rs <= 1e-10 and re <= 1e-10 and rp <= 1e-10, (what, name)
        if name != "zeros":
            pp = linreg_predict(rows, cd, b0).cpu().numpy()
            assert np.array_equal(pp, pr), "predict and the stats pass's pred differ"


@pytest.mark.parametrize("n,p", SHAPES)
def test_stats_and_predict_dense(cuda, n, p):
    c = case(n, p)
    _check_stats(cuda, lambda X: _dev(X, cuda), c["X"], c["y"], c["coef"], c["b0"], c["center"],
                 (("w", c["w"]), ("w null", None), ("zeros", c["wz"])), f"dense {n} x {p}")


@pytest.mark.parametrize("n,p", CSR_SHAPES)
def test_stats_and_predict_csr(cuda, n, p):
    c = case(n, p, True)
    _check_stats(cuda, lambda X: _csr(X, cuda), c["X"], c["y"],
                 c["coef"], c["b0"], c["center"],
                 (("w", c["w"]), ("w null", None), ("zeros", c["wz"])), f"csr {n} x {p}")


def _wide(n, p, nnz, seed):
    rng = np.random.default_rng(seed)
    colidx = np.sort(np.stack([rng.choice(p, nnz, replace=False) for _ in range(n)]), axis=1)
    vals = rng.normal(size=(n, nnz))
    rowptr = np.arange(n + 1) * nnz
    return rowptr, colidx.ravel(), vals


def _wide_dot(colidx, vals, coef, n, nnz):
    g = np.asarray(coef, np.longdouble)[colidx.reshape(n, nnz)]
    return np.asarray((vals.astype(np.longdouble) * g).sum(1), dtype=np.float64)


def test_stats_csr_beyond_lds(cuda):
    """600 x 200000, 8 nonzeros per row: the coefficients do not fit LDS and
    are gathered from global memory."""
    from cycloneml_amd.regression_summary import linreg_predict, linreg_stats
    n, p, nnz = 600, 200000, 8
    rowptr, colidx, vals = _wide(n, p, nnz, 5)
    rng = np.random.default_rng(6)
    coef, b0 = rng.normal(size=p), -0.3
    w = rng.uniform(0.25, 3.0, n)
    w[::7] = 0.0
    pref = _wide_dot(colidx, vals, coef, n, nnz) + b0
    y = pref + rng.normal(size=n)
    # the dense restatement over the columns in use only
    used = np.unique(colidx)
    Xs = np.zeros((n, used.size))
    Xs[np.repeat(np.arange(n), nnz), np.searchsorted(used, colidx)] = vals.ravel()
    ref, mags, _ = H.ref_stats(Xs, y, w, coef[used], b0, 0.25)
    vz = vals.copy()
    vz[w == 0.0] = np.nan
    rows = _csr_of(rowptr, colidx, vz.ravel(), p, cuda)
    cd = _dev(coef, cuda)
    out, pred = linreg_stats(rows, _dev(y, cuda), _dev(w, cuda), cd, b0, 0.25, want_pred=True)
    out2, _ = linreg_stats(rows, _dev(y, cuda), _dev(w, cuda), cd, b0, 0.25, want_pred=True)
    o, pr = out.cpu().numpy(), pred.cpu().numpy()
    live = w != 0.0
    rs = _sum_ratio(o, ref, mags)
    re = float((np.abs(o[8:] - ref[8:]) / np.maximum(1.0, np.abs(ref[8:]))).max())
    rp = float((np.abs(pr[live] - pref[live]) / np.maximum(1.0, np.abs(pref[live]))).max())
    print(f"csr 600 x 200000: worst |dsum| / sum|term| = {rs:.3g}, extrema {re:.3g}, pred "
          f"{rp:.3g} (bar 1e-10)")
    assert np.isfinite(o).all() and np.array_equal(o, out2.cpu().numpy())
    assert rs <= 1e-10 and re <= 1e-10 and rp <= 1e-10
    clean = _csr_of(rowptr, colidx, vals.ravel(), p, cuda)
    pp = linreg_predict(clean, cd, b0).cpu().numpy()
    assert float((np.abs(pp - pref) / np.maximum(1.0, np.abs(pref))).max()) <= 1e-10


# ---- fits --------------------------------------------------------------------------------
def _fit(cuda, X, y, w, rows=None, **kw):
    from cycloneml_amd import LinearRegression
    lr = LinearRegression(maxIter=H.MAX_ITER, tol=H.TOL, **kw)
    return lr, lr.fit(_dev(X, cuda) if rows is None else rows, _dev(y, cuda), _dev(w, cuda))


def test_fit_lbfgs_dense_and_csr(cuda):
    """solver = "l-bfgs" at 2600 x 17, dense and CSR of the same rows, against
    WeightedLeastSquares at the host file's bar."""
    X, y, w, _ = H.data(2600, 17)
    for reg in (0.0, 0.1):
        ref = H.wls_reference(X, y, w, reg, True, True)
        scale = np.abs(ref.coefficients).max()
        for name, rows in (("dense", None), ("csr", _csr(X, cuda))):
            _, m = _fit(cuda, X, y, w, rows, regParam=reg, solver="l-bfgs")
            d = float(np.abs(m.coefficients - ref.coefficients).max() / scale)
            di = abs(m.intercept - ref.intercept) / max(1.0, abs(ref.intercept))
            print(f"device l-bfgs {name} reg={reg}: |dcoef| / max|coef| = {d:.3g}, |dintercept| "
                  f"= {di:.3g} (bar {H.BAR_L2:.3g}), {len(m.objectiveHistory)} states")
            assert d <= H.BAR_L2 and di <= H.BAR_L2
            assert m.diagInvAtWA.shape == (1,) and m.diagInvAtWA[0] == 0.0
            assert m.summary.totalIterations == len(m.objectiveHistory) - 1


def test_fit_auto_wide_csr(cuda):
    """solver = "auto" above 4096 features is the quasi-Newton path: 600 x
    4100 CSR, 8 nonzeros per row, regParam = 0.1; the oracle objective's
    gradient at the solution within the host file's elastic-net bar (the same
    objective with alpha = 0)."""
    from cycloneml_amd import LinearRegression
    n, p, nnz = 600, 4100, 8
    rowptr, colidx, vals = _wide(n, p, nnz, 11)
    rng = np.random.default_rng(12)
    beta = rng.normal(size=p)
    y = _wide_dot(colidx, vals, beta, n, nnz) + 0.1 * rng.normal(size=n)
    w = rng.uniform(0.5, 2.0, n)
    lr = LinearRegression(maxIter=H.MAX_ITER, tol=H.TOL, regParam=0.1, solver="auto")
    m = lr.fit(_csr_of(rowptr, colidx, vals.ravel(), p, cuda), _dev(y, cuda), _dev(w, cuda))
    assert m.diagInvAtWA.shape == (1,) and m.diagInvAtWA[0] == 0.0, "the normal path ran"
    assert lr.lastCost.evaluations >= len(m.objectiveHistory) > 1
    X = np.zeros((n, p))
    X[np.repeat(np.arange(n), nnz), colidx] = vals.ravel()
    v, _ = H.enet_violation(X, y, w, lr, m)
    print(f"device auto 600 x 4100 csr: worst |gradient| = {v:.3g} (bar {H.BAR_ENET:.3g}), "
          f"{len(m.objectiveHistory)} states, {lr.lastCost.evaluations} passes")
    assert v <= H.BAR_ENET


def test_fit_huber_dense(cuda):
    X, y, w, _ = H.data(2600, 17, outliers=True)
    for reg in (0.0, 0.1):
        lr, m = _fit(cuda, X, y, w, regParam=reg, loss="huber", epsilon=1.35)
        g = H.huber_gradient(X, y, w, lr, m)
        _, href = H.fit_host(X, y, w, regParam=reg, loss="huber", epsilon=1.35)
        d = float(np.abs(m.coefficients - href.coefficients).max() /
                  np.abs(href.coefficients).max())
        print(f"device huber reg={reg}: |gradient|_inf = {g:.3g} (bar {H.BAR_HUBER:.3g}), scale "
              f"{m.scale:.6g} (host {href.scale:.6g}), |dcoef| / max|coef| vs host = {d:.3g}")
        assert g <= H.BAR_HUBER and m.scale > 0.0


def test_fit_auto_narrow_is_the_normal_path(cuda):
    from cycloneml_amd import LinearRegression, WeightedLeastSquares
    X, y, w, _ = H.data(300, 7)
    Xd, yd, wd = _dev(X, cuda), _dev(y, cuda), _dev(w, cuda)
    m = LinearRegression(regParam=0.1).fit(Xd, yd, wd)
    ref = WeightedLeastSquares(True, 0.1, 0.0, standardizeFeatures=True, standardizeLabel=True,
                               solverType="auto", maxIter=100, tol=1e-6).fit(Xd, yd, wd)
    assert np.array_equal(m.coefficients, ref.coefficients) and m.intercept == ref.intercept
    assert np.array_equal(m.diagInvAtWA, ref.diagInvAtWA)


# ---- summary -----------------------------------------------------------------------------
FIELDS = ("meanSquaredError", "rootMeanSquaredError", "meanAbsoluteError", "explainedVariance",
          "r2", "r2adj")


def _check_summary(s, X, y, w, m, fitIntercept, what):
    n, p = X.shape
    ybar = float(np.sum(w * y) / np.sum(w))
    ref, _, pref = H.ref_stats(X, y, w, m.coefficients, m.intercept, ybar)
    want = H.ref_metrics(ref, n, p, fitIntercept)
    worst = max(abs(getattr(s, f) - want[f]) / abs(want[f]) for f in FIELDS)
    dr = s.devianceResiduals
    worst = max(worst, *(abs(a - b) / abs(b) for a, b in zip(dr, want["devianceResiduals"])))
    print(f"{what}: worst relative difference of a summary field = {worst:.3g} (bar 1e-10)")
    assert worst <= 1e-10
    assert s.degreesOfFreedom == want["degreesOfFreedom"] and s.numInstances == n
    pr = s.predictions.cpu().numpy()
    assert float((np.abs(pr - pref) / np.maximum(1.0, np.abs(pref))).max()) <= 1e-10
    assert np.array_equal(s.residuals.cpu().numpy(), y - pr)


@pytest.mark.parametrize("icpt", [True, False])
def test_summary_and_evaluate(cuda, icpt):
    X, y, w, _ = H.data(2600, 17)
    lr, m = _fit(cuda, X, y, w, solver="l-bfgs", fitIntercept=icpt)
    assert m.hasSummary and m._summary is None, "built on first access"
    _check_summary(m.summary, X, y, w, m, icpt, f"training summary, intercept {icpt}")
    _check_summary(m.evaluate(_dev(X, cuda), _dev(y, cuda), _dev(w, cuda)), X, y, w, m, icpt,
                   f"evaluate, intercept {icpt}")
    _check_summary(m.evaluate(_csr(X, cuda), _dev(y, cuda), _dev(w, cuda)), X, y, w, m, icpt,
                   f"evaluate csr, intercept {icpt}")
    with pytest.raises(NotImplementedError, match="No Std. Error"):
        m.summary.coefficientStandardErrors
    with pytest.raises(NotImplementedError, match="No Std. Error"):
        m.summary.pValues


def test_standard_errors_of_the_normal_fit(cuda):
    from scipy import stats
    X, y, w, _ = H.data(300, 7)
    _, m = _fit(cuda, X, y, w, solver="normal")
    n, p = X.shape
    # the reference on standardized columns (its conditioning is the fit's)
    A = np.column_stack([X, np.ones(n)])
    G = (A * w[:, None]).T @ A
    sd = np.sqrt(np.diag(G))
    cond = np.linalg.cond(G / np.outer(sd, sd))
    assert cond <= 1e3, cond
    Ginv = np.linalg.inv(G / np.outer(sd, sd)) / np.outer(sd, sd)
    est = np.append(m.coefficients, m.intercept)
    e = y - (X @ m.coefficients + m.intercept)
    df = n - p - 1
    se = np.sqrt(np.diag(Ginv) * np.sum(w * e * e) / df)
    t = est / se
    pv = 2.0 * stats.t.sf(np.abs(t), df)
    s = m.summary
    bar = 1e-8 * cond
    worst = max(float((np.abs(s.coefficientStandardErrors - se) / se).max()),
                float((np.abs(s.tValues - t) / np.abs(t)).max()),
                float((np.abs(s.pValues - pv) / np.maximum(pv, 1e-300)).max()))
    print(f"standard errors, t and p values: worst relative difference {worst:.3g} "
          f"(bar {bar:.3g}, cond {cond:.3g})")
    assert worst <= bar
    _, reg = _fit(cuda, X, y, w, solver="normal", regParam=0.1)
    with pytest.raises(NotImplementedError, match="No Std. Error"):
        reg.summary.tValues


def test_predict_csr_equals_dense(cuda):
    X, y, w, _ = H.data(2600, 17)
    Xs = X.copy()
    Xs[np.random.default_rng(3).random(X.shape) < 0.3] = 0.0
    _, m = _fit(cuda, Xs, y, w, solver="normal")
    a = m.predict(_csr(Xs, cuda)).cpu().numpy()
    b = m.predict(_dev(Xs, cuda)).cpu().numpy()
    assert float((np.abs(a - b) / np.maximum(1.0, np.abs(b))).max()) <= 1e-10
    with pytest.raises(ValueError, match="expected 17 features"):
        m.predict(_csr(Xs[:, :5], cuda))
