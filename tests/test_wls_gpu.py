"""GPU: the weighted augmented syrk (k_wls_tiles, cyc_wls_accumulate_dev) per
entry against numpy.longdouble moments, its weight handling, the CSR path,
and LinearRegression's normal-equation fit end to end.

Bars.  Moments: |dU_ij| <= 1e-10 sqrt(U_ii U_jj) for every entry (the
project's entrywise bar, tests/test_gramian_gpu.py).  Where two device
results of the same rows are compared (two calls against one, CSR against
dense) the bar is 1e-12 in the same per-entry unit sqrt(U_ii U_jj): the
generator's columns are signed, so single entries cancel to far below their
columns' scale, and a bound relative to the entry itself would measure that
cancellation, not the kernel (n eps = 4.6e-13 at n = 4099 bounds the
difference of two summation orders in this unit).
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (40, 1), (300, 7), (2600, 126), (2600, 127), (4099, 130), (4099, 257)]


def _dev(a, cuda):
    import torch
    return torch.from_numpy(np.array(a, dtype=np.float64, order="C")).to(cuda)


def _moments_ld(X, y, w):
    Z = np.column_stack([X, y, np.ones(len(y))]).astype(np.longdouble)
    return ((Z * w.astype(np.longdouble)[:, None]).T @ Z).astype(np.float64)


@functools.lru_cache(maxsize=None)
def _case(n, p):
    rng = np.random.default_rng(7 + p)
    X = rng.normal(size=(n, p)) * rng.uniform(0.5, 2, size=p) + rng.uniform(-1, 1, size=p)
    w = rng.uniform(0.5, 2, size=n)
    y = X @ rng.normal(size=p) + 0.1 * rng.normal(size=n)
    ref = {"X": X, "y": y, "w": w, "Mw": _moments_ld(X, y, w),
           "M1": _moments_ld(X, y, np.ones(n))}
    for a in ref.values():
        a.setflags(write=False)
    return ref


def _device_moments(cuda, X, y, w, parts=1, plan=None):
    """The packed U of the rows, accumulated in `parts` successive calls;
    returns (full symmetric matrix, split counts of the calls)."""
    import torch
    from cycloneml_amd.regression import WLSPlan, packed_to_full
    p = X.shape[1]
    own = plan is None
    plan = WLSPlan(p) if own else plan
    U = torch.zeros(plan.packedSize, dtype=torch.float64, device=cuda)
    Xd, yd = _dev(X, cuda), _dev(y, cuda)
    wd = None if w is None else _dev(w, cuda)
    edges = np.linspace(0, X.shape[0], parts + 1).astype(int)
    splits = []
    for a, b in zip(edges[:-1], edges[1:]):
        plan.accumulate(Xd[a:b], yd[a:b], None if wd is None else wd[a:b], U)
        splits.append(plan.last_splits())
    if own:
        plan.close()
    return packed_to_full(U.cpu().numpy(), p + 2), splits


def _assert_entrywise(got, ref, tol, what=""):
    d = np.sqrt(np.clip(np.diag(ref), 0.0, None))
    lim = tol * np.outer(d, d)
    err = np.abs(got - ref)
    worst = float((err / np.maximum(lim / tol, 1e-300)).max())
    print(f"{what}: worst |dU_ij| / sqrt(U_ii U_jj) = {worst:.3g} (bar {tol:g})")
    assert np.all(np.isfinite(got)), what
    assert not (err > lim).any(), f"{what}: {int((err > lim).sum())} entries off, worst {worst:.3g}"


@pytest.mark.parametrize("n,p", SHAPES)
def test_moments_entrywise(cuda, n, p):
    c = _case(n, p)
    got, splits = _device_moments(cuda, c["X"], c["y"], c["w"])
    _assert_entrywise(got, c["Mw"], 1e-10, f"weighted {n} x {p}")
    got1, _ = _device_moments(cuda, c["X"], c["y"], None)
    _assert_entrywise(got1, c["M1"], 1e-10, f"unit weights {n} x {p}")
    assert got1[p + 1, p + 1] == float(n)      # wSum of unit weights: the row count
    if n >= 2600:
        # more than one row split, the last one ragged (rows per split are a
        # multiple of the 16-row chunk; n is not)
        assert splits[0] >= 2 and n % 16 != 0, splits


@pytest.mark.parametrize("n,p", [(2600, 127), (4099, 130)])
def test_two_calls_accumulate_into_one(cuda, n, p):
    c = _case(n, p)
    whole, _ = _device_moments(cuda, c["X"], c["y"], c["w"])
    halves, _ = _device_moments(cuda, c["X"], c["y"], c["w"], parts=2)
    _assert_entrywise(halves, whole, 1e-12, f"two calls {n} x {p}")


def test_zero_rows_leave_moments_unchanged(cuda):
    import torch
    from cycloneml_amd.regression import WeightedLeastSquares, WLSPlan
    from cycloneml_amd._native import IllegalArgumentException
    plan = WLSPlan(3)
    U = torch.arange(plan.packedSize, dtype=torch.float64, device=cuda)
    e = torch.zeros((0, 3), dtype=torch.float64, device=cuda)
    plan.accumulate(e, e[:, 0], None, U)
    assert torch.equal(U, torch.arange(plan.packedSize, dtype=torch.float64, device=cuda))
    plan.close()
    with pytest.raises(IllegalArgumentException, match="Training dataset is empty."):
        WeightedLeastSquares(True, 0.0).fit(e, e[:, 0].contiguous())


@pytest.mark.parametrize("n,p", [(300, 7), (2600, 126)])
def test_zero_weight_rows_contribute_nothing(cuda, n, p):
    """Rows of weight 0 hold NaN and Inf features and labels: U is finite and
    is the moments of the other rows."""
    c = _case(n, p)
    X, y, w = c["X"].copy(), c["y"].copy(), c["w"].copy()
    dead = np.zeros(n, dtype=bool)
    dead[[0, 5, 17, n // 2, n - 1]] = True
    dead[40:60:3] = True
    w[dead] = 0.0
    X[dead] = np.nan
    X[dead, ::2] = np.inf
    y[dead] = -np.inf
    y[5] = np.nan
    got, _ = _device_moments(cuda, X, y, w)
    ref = _moments_ld(X[~dead], y[~dead], w[~dead])
    _assert_entrywise(got, ref, 1e-10, f"zero-weight rows {n} x {p}")


@pytest.mark.parametrize("bad", [-1.0, -1e-300, float("nan")])
def test_negative_weight_raises(cuda, bad):
    from cycloneml_amd._native import IllegalArgumentException
    from cycloneml_amd.regression import LinearRegression
    c = _case(300, 7)
    w = c["w"].copy()
    w[123] = bad
    with pytest.raises(IllegalArgumentException) as e:
        _device_moments(cuda, c["X"], c["y"], w)
    assert str(e.value).startswith("requirement failed: Negative weight")
    with pytest.raises(IllegalArgumentException, match="requirement failed: Negative weight"):
        LinearRegression().fit(_dev(c["X"], cuda), _dev(c["y"], cuda), _dev(w, cuda))


def test_more_than_4096_features_fails_at_plan_creation(cuda):
    from cycloneml_amd._native import IllegalArgumentException
    from cycloneml_amd.regression import WLSPlan
    with pytest.raises(IllegalArgumentException) as e:
        WLSPlan(4097)
    assert str(e.value) == ("requirement failed: In order to take the normal equation approach "
                            "efficiently, we set the max number of features to 4096 but got 4097.")
    WLSPlan(4096).close()


def test_csr_rows_match_dense(cuda):
    """(4099, 130) at 10 % density through CSRRows against the dense path on
    the densified rows.  The two sum in the same order: bitwise equality was
    seen on an MI355X (the assertion stays at the 1e-12 bar)."""
    import torch
    from cycloneml_amd.linalg import CSRRows
    from cycloneml_amd.regression import WLSPlan, packed_to_full
    n, p = 4099, 130
    c = _case(n, p)
    rng = np.random.default_rng(99)
    X = np.where(rng.uniform(size=(n, p)) < 0.10, c["X"], 0.0)
    X[7] = 0.0                                   # an empty row
    nz = X != 0.0
    rowptr = np.concatenate([[0], np.cumsum(nz.sum(1))]).astype(np.int64)
    colidx = np.nonzero(nz)[1].astype(np.int32)
    rows = CSRRows(torch.from_numpy(rowptr).to(cuda), torch.from_numpy(colidx).to(cuda),
                   _dev(X[nz], cuda), p)
    plan = WLSPlan(p)
    U = torch.zeros(plan.packedSize, dtype=torch.float64, device=cuda)
    plan.accumulate_csr(rows, _dev(c["y"], cuda), _dev(c["w"], cuda), U)
    plan.close()
    sparse = packed_to_full(U.cpu().numpy(), p + 2)
    dense, _ = _device_moments(cuda, X, c["y"], c["w"])
    print("CSR vs dense bitwise equal:", bool(np.array_equal(sparse, dense)))
    _assert_entrywise(sparse, dense, 1e-12, "CSR vs dense")
    _assert_entrywise(sparse, _moments_ld(X, c["y"], c["w"]), 1e-10, "CSR vs longdouble")


def _pack(M):
    n = M.shape[0]
    j, i = np.tril_indices(n)
    return np.ascontiguousarray(M[i, j])


def _standardized_system(M, k, fitIntercept, regParam):
    """The k x k system LinearRegression's defaults solve for the
    coefficients (features and label standardized), from full reference
    moments.  With an intercept it is the system left once the intercept
    row [aBar, 1.0] is eliminated: the (regularized) correlation matrix,
    whose condition number is the smaller one, so the tighter tolerance."""
    ws = M[k + 1, k + 1]
    aBar, bBar = M[:k, k + 1] / ws, M[k, k + 1] / ws
    aStd = np.sqrt(np.diag(M[:k, :k]) / ws - aBar ** 2)
    bStd = np.sqrt(M[k, k] / ws - bBar ** 2)
    S = M[:k, :k] / ws / np.outer(aStd, aStd) + regParam / bStd * np.eye(k)
    if fitIntercept:
        a = aBar / aStd
        S = S - np.outer(a, a)
    return S


@pytest.mark.parametrize("regParam", [0.0, 0.3])
@pytest.mark.parametrize("fitIntercept", [False, True])
@pytest.mark.parametrize("n,p", [(2600, 127), (4099, 130)])
def test_linear_regression_end_to_end(cuda, n, p, fitIntercept, regParam):
    """LinearRegression().fit on the device against WeightedLeastSquares.solve
    on the longdouble moments (no kernel in the reference)."""
    from cycloneml_amd import LinearRegression, WeightedLeastSquares
    c = _case(n, p)
    cond = np.linalg.cond(_standardized_system(c["Mw"], p, fitIntercept, regParam))
    assert cond <= 1e3, cond
    ref = WeightedLeastSquares(fitIntercept, regParam).solve(_pack(c["Mw"]), p)
    Xd = _dev(c["X"], cuda)
    model = LinearRegression(fitIntercept=fitIntercept, regParam=regParam).fit(
        Xd, _dev(c["y"], cuda), _dev(c["w"], cuda))
    assert model.numFeatures == p and model.scale == 1.0
    want = np.append(ref.coefficients, ref.intercept)
    got = np.append(model.coefficients, model.intercept)
    tol = 2e-10 * cond * np.abs(want).max()
    print(f"{n} x {p} intercept {fitIntercept} reg {regParam}: cond {cond:.3g}, "
          f"max |dx| {np.abs(got - want).max():.3g}, tol {tol:.3g}")
    assert np.abs(got - want).max() <= tol
    if not fitIntercept:
        assert model.intercept == 0.0
    pred = model.predict(Xd).cpu().numpy()
    # 1e-12 relative, in units of the largest label for predictions that
    # cancel to near zero (a dot product's rounding does not shrink with them)
    np.testing.assert_allclose(pred, c["X"] @ model.coefficients + model.intercept, rtol=1e-12,
                               atol=1e-12 * np.abs(c["y"]).max())
    assert model.predict(c["X"][3]) == pytest.approx(pred[3], rel=1e-12)


@pytest.mark.parametrize("standardization", [False, True])
@pytest.mark.parametrize("fitIntercept,expected", [(False, (0.0, -3.727121, 3.009983)),
                                                   (True, (18.08, 6.08, -0.60))])
def test_suite_instances_through_the_device_fit(cuda, fitIntercept, expected, standardization):
    from cycloneml_amd import LinearRegression
    A = np.array([[0.0, 5.0], [1.0, 7.0], [2.0, 11.0], [3.0, 13.0]])
    b = np.array([17.0, 19.0, 23.0, 29.0])
    w = np.array([1.0, 2.0, 3.0, 4.0])
    for solver in ("auto", "normal"):
        m = LinearRegression(fitIntercept=fitIntercept, standardization=standardization,
                             solver=solver).fit(_dev(A, cuda), _dev(b, cuda), _dev(w, cuda))
        np.testing.assert_allclose([m.intercept, *m.coefficients], expected, rtol=0, atol=1e-4)
