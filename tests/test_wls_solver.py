"""WeightedLeastSquares.solve on packed moments (host, no GPU): the
WeightedLeastSquaresSuite instances' known answers, ridge against a closed
form written here, the singular system's quasi-Newton fallback, L1, and the
validation messages."""
import ctypes
import itertools

import numpy as np
import pytest

from cycloneml_amd import _native as N
from cycloneml_amd.regression import (LinearRegression, SingularMatrixException,
                                      WeightedLeastSquares, packed_to_full)

# WeightedLeastSquaresSuite: instances (w, a, b)
A = np.array([[0.0, 5.0], [1.0, 7.0], [2.0, 11.0], [3.0, 13.0]])
B = np.array([17.0, 19.0, 23.0, 29.0])
W = np.array([1.0, 2.0, 3.0, 4.0])


def pack(M):
    n = M.shape[0]
    return np.array([M[i, j] for j in range(n) for i in range(j + 1)], dtype=np.float64)


def moments(a, b, w):
    Z = np.column_stack([a, b, np.ones(len(b))])
    return pack((Z * w[:, None]).T @ Z)


U_AB = moments(A, B, W)
U_CONST = moments(A, np.full(4, 17.0), W)


def test_packed_layout_of_the_suite_instances():
    full = np.array([[50, 236, 524, 20], [236, 1162, 2618, 104], [524, 2618, 5962, 240],
                     [20, 104, 240, 10]], dtype=np.float64)
    assert np.array_equal(packed_to_full(U_AB, 4), full)
    assert np.array_equal(U_AB, pack(full))
    # aaSum, abSum, bbSum, aSum, bSum, wSum where the kernel's layout puts them
    M = packed_to_full(U_AB, 4)
    assert np.array_equal(M[:2, 2], (A * (W * B)[:, None]).sum(0))
    assert M[2, 2] == (W * B * B).sum() and M[2, 3] == (W * B).sum() and M[3, 3] == W.sum()
    assert np.array_equal(M[:2, 3], (A * W[:, None]).sum(0))


@pytest.mark.parametrize("solver", ["auto", "cholesky", "quasi-newton"])
@pytest.mark.parametrize("standardize", [False, True])
@pytest.mark.parametrize("fitIntercept,expected", [(False, (0.0, -3.727121, 3.009983)),
                                                   (True, (18.08, 6.08, -0.60))])
def test_known_answers(fitIntercept, expected, standardize, solver):
    m = WeightedLeastSquares(fitIntercept, 0.0, standardizeFeatures=standardize,
                             standardizeLabel=standardize, solverType=solver).solve(U_AB, 2)
    got = np.array([m.intercept, *m.coefficients])
    print(fitIntercept, standardize, solver, got)
    np.testing.assert_allclose(got, expected, rtol=0, atol=1e-4)
    if solver == "quasi-newton":
        assert np.array_equal(m.diagInvAtWA, [0.0]) and len(m.objectiveHistory) >= 2
    else:
        assert m.diagInvAtWA.shape == (3 if fitIntercept else 2,)
        assert np.array_equal(m.objectiveHistory, [0.0])


@pytest.mark.parametrize("solver", ["auto", "cholesky", "quasi-newton"])
@pytest.mark.parametrize("standardize", [False, True])
def test_constant_label_without_intercept(standardize, solver):
    m = WeightedLeastSquares(False, 0.0, standardizeFeatures=standardize,
                             standardizeLabel=True, solverType=solver).solve(U_CONST, 2)
    got = np.array([m.intercept, *m.coefficients])
    print(standardize, solver, got)
    np.testing.assert_allclose(got, (0.0, -9.221298, 3.394343), rtol=0, atol=1e-4)


@pytest.mark.parametrize("solver", ["auto", "cholesky", "quasi-newton"])
@pytest.mark.parametrize("regParam", [0.0, 0.1])
def test_constant_label_with_intercept(regParam, solver):
    m = WeightedLeastSquares(True, regParam, solverType=solver).solve(U_CONST, 2)
    assert m.intercept == 17.0
    assert np.array_equal(m.coefficients, [0.0, 0.0])
    assert np.array_equal(m.diagInvAtWA, [0.0])
    assert np.array_equal(m.objectiveHistory, [0.0])


def test_constant_label_regularized_standardized_label_raises():
    with pytest.raises(N.IllegalArgumentException) as e:
        WeightedLeastSquares(False, 0.1, standardizeLabel=True).solve(U_CONST, 2)
    assert "The standard deviation of the label is zero. Model cannot be regularized when " \
           "labels are standardized." in str(e.value)
    # the label not standardized: the fit goes on with bStd = |bBar|
    m = WeightedLeastSquares(False, 0.1, standardizeLabel=False).solve(U_CONST, 2)
    assert np.all(np.isfinite(m.coefficients)) and m.intercept == 0.0


def _ridge_closed_form(a, b, w, fitIntercept, regParam, stdFeatures, stdLabel):
    """The standardized system of the issue, written out from the rows (not
    from packed moments) and solved by numpy.linalg.solve."""
    ws = w.sum()
    aBar = (w[:, None] * a).sum(0) / ws
    bBar = (w * b).sum() / ws
    aaBar = (a * w[:, None]).T @ a / ws
    abBar = (a * (w * b)[:, None]).sum(0) / ws
    bbBar = (w * b * b).sum() / ws
    aStd = np.sqrt(np.maximum(np.diag(aaBar) - aBar ** 2, 0))
    bStd = np.sqrt(max(bbBar - bBar ** 2, 0))
    k = a.shape[1]
    S = aaBar / np.outer(aStd, aStd)
    for j in range(k):
        lam = regParam / bStd
        if not stdFeatures:
            lam /= aStd[j] ** 2
        if not stdLabel:
            lam *= bStd
        S[j, j] += lam
    rhs = abBar / (aStd * bStd)
    if fitIntercept:
        S = np.block([[S, (aBar / aStd)[:, None]], [(aBar / aStd)[None, :], np.ones((1, 1))]])
        rhs = np.append(rhs, bBar / bStd)
    x = np.linalg.solve(S, rhs)
    coef = x[:k] * bStd / aStd
    return np.array([x[k] * bStd if fitIntercept else 0.0, *coef])


@pytest.mark.parametrize("fitIntercept", [False, True])
@pytest.mark.parametrize("stdFeatures,stdLabel", list(itertools.product([False, True], repeat=2)))
@pytest.mark.parametrize("regParam", [0.1, 1.0])
def test_ridge_against_closed_form(regParam, stdFeatures, stdLabel, fitIntercept):
    ref = _ridge_closed_form(A, B, W, fitIntercept, regParam, stdFeatures, stdLabel)
    for solver in ("auto", "cholesky"):
        m = WeightedLeastSquares(fitIntercept, regParam, 0.0, stdFeatures, stdLabel,
                                 solver).solve(U_AB, 2)
        got = np.array([m.intercept, *m.coefficients])
        np.testing.assert_allclose(got, ref, rtol=1e-10, atol=0)
        assert np.all(m.diagInvAtWA > 0)


def test_diag_inv_atwa_is_the_inverse_normal_matrix_diagonal():
    """regParam = 0 with an intercept: diagInvAtWA = diag((Z^T W Z)^-1) for
    Z = [A, 1] (the covariance of the estimates up to sigma^2)."""
    m = WeightedLeastSquares(True, 0.0, solverType="cholesky").solve(U_AB, 2)
    Z = np.column_stack([A, np.ones(4)])
    ref = np.diag(np.linalg.inv((Z * W[:, None]).T @ Z))
    np.testing.assert_allclose(m.diagInvAtWA, ref, rtol=1e-9)


def test_singular_system():
    """A constant third column with an intercept: Cholesky fails, "auto"
    falls back to the quasi-Newton solver.  The constant column's coefficient
    is exactly 0; the others agree with the two-column Cholesky answer
    within 10 sqrt(tol cond) relative (breeze's LBFGS stops on the relative
    improvement of the objective, which on a quadratic bounds the iterate's
    error by sqrt(tol cond)); cond is that of the standardized two-column
    system.  Observed: cond 3969, bound 6.3e-5, largest relative gap 1.6e-7."""
    A3 = np.column_stack([A, np.ones(4)])
    U3 = moments(A3, B, W)
    with pytest.raises(SingularMatrixException):
        WeightedLeastSquares(True, 0.0, solverType="cholesky").solve(U3, 3)
    tol = 1e-14
    m = WeightedLeastSquares(True, 0.0, solverType="auto", maxIter=1000, tol=tol).solve(U3, 3)
    assert m.coefficients[2] == 0.0
    assert np.array_equal(m.diagInvAtWA, [0.0])
    ref = WeightedLeastSquares(True, 0.0, solverType="cholesky").solve(U_AB, 2)
    # the standardized two-column system with its intercept row
    ws = W.sum()
    aBar = (W[:, None] * A).sum(0) / ws
    aaBar = (A * W[:, None]).T @ A / ws
    aStd = np.sqrt(np.diag(aaBar) - aBar ** 2)
    S = np.block([[aaBar / np.outer(aStd, aStd), (aBar / aStd)[:, None]],
                  [(aBar / aStd)[None, :], np.ones((1, 1))]])
    cond = np.linalg.cond(S)
    bound = 10 * np.sqrt(tol * cond)
    got = np.array([m.intercept, m.coefficients[0], m.coefficients[1]])
    want = np.array([ref.intercept, *ref.coefficients])
    gap = np.abs(got - want) / np.abs(want)
    print(f"cond {cond:.4g} bound {bound:.3g} gaps {gap}")
    assert np.all(gap <= bound), (gap, bound)


@pytest.mark.parametrize("solver", ["auto", "quasi-newton"])
@pytest.mark.parametrize("stdFeatures", [False, True])
def test_l1_large_enough_zeroes_every_coefficient(stdFeatures, solver):
    ws = W.sum()
    aBar = (W[:, None] * A).sum(0) / ws
    bBar = (W * B).sum() / ws
    aStd = np.sqrt(np.diag((A * W[:, None]).T @ A / ws) - aBar ** 2)
    bStd = np.sqrt((W * B * B).sum() / ws - bBar ** 2)
    abBar = (A * (W * B)[:, None]).sum(0) / ws / (aStd * bStd)
    regParam = 10 * np.max(np.abs(abBar))
    m = WeightedLeastSquares(True, regParam, 1.0, stdFeatures, True, solver).solve(U_AB, 2)
    assert np.array_equal(m.coefficients, [0.0, 0.0])
    assert abs(m.intercept - bBar) <= 1e-12
    assert np.array_equal(m.diagInvAtWA, [0.0])


def test_elastic_net_takes_the_quasi_newton_solver_under_auto():
    """elasticNetParam and regParam both nonzero: OWLQN (an objective
    history, no inverse), with a solution between ridge's and zero."""
    m = WeightedLeastSquares(True, 0.5, 0.5, solverType="auto").solve(U_AB, 2)
    assert np.array_equal(m.diagInvAtWA, [0.0]) and len(m.objectiveHistory) >= 2
    assert np.all(np.diff(m.objectiveHistory) <= 1e-12)
    ridge = WeightedLeastSquares(True, 0.0, solverType="cholesky").solve(U_AB, 2)
    assert np.linalg.norm(m.coefficients, 1) < np.linalg.norm(ridge.coefficients, 1)


def test_validation_messages():
    wls = WeightedLeastSquares(True, 0.0)
    with pytest.raises(N.IllegalArgumentException) as e:
        wls.solve(moments(A, B, np.zeros(4)), 2)
    assert str(e.value) == "requirement failed: Sum of weights cannot be zero."
    with pytest.raises(N.IllegalArgumentException) as e:
        wls.solve(np.zeros(10), 2, count=0)
    assert str(e.value) == "requirement failed: Training dataset is empty."
    with pytest.raises(N.IllegalArgumentException):
        wls.solve(np.zeros(9), 2)      # not a packed triangle of order 4
    with pytest.raises(N.IllegalArgumentException):
        WeightedLeastSquares(True, -1.0)
    with pytest.raises(N.IllegalArgumentException):
        WeightedLeastSquares(True, 0.0, solverType="normal")


def test_plan_refuses_more_than_4096_features():
    """WeightedLeastSquares.MAX_NUM_FEATURES, checked before any device use."""
    h = ctypes.c_void_p()
    rc = N.load().cyc_wls_plan_create(4097, ctypes.byref(h))
    assert rc == N.CYC_ERR_INVALID_ARG
    with pytest.raises(N.IllegalArgumentException) as e:
        N.check(rc)
    assert str(e.value) == ("requirement failed: In order to take the normal equation approach "
                            "efficiently, we set the max number of features to 4096 but got 4097.")


def test_linear_regression_paths_not_built():
    import cycloneml_amd
    assert cycloneml_amd.LinearRegression is LinearRegression
    X = np.zeros((4, 2))
    with pytest.raises(NotImplementedError, match="HuberBlockAggregator"):
        LinearRegression(loss="huber").fit(X, B)
    with pytest.raises(NotImplementedError, match="LeastSquaresBlockAggregator"):
        LinearRegression(solver="l-bfgs").fit(X, B)
    with pytest.raises(NotImplementedError, match="LeastSquaresBlockAggregator"):
        LinearRegression(solver="auto").fit(np.zeros((1, 4097)), B[:1])


def test_model_predicts_one_host_vector():
    from cycloneml_amd.regression import LinearRegressionModel
    m = LinearRegressionModel([6.08, -0.60], 18.08)
    assert m.numFeatures == 2 and m.scale == 1.0
    assert m.predict([1.0, 7.0]) == pytest.approx(18.08 + 6.08 - 4.2, rel=1e-15)
