"""LinearRegression by the normal equations: the host side of
ml/optim/WeightedLeastSquares.scala and of the `Auto | Normal` branch of
ml/regression/LinearRegression.scala.

The reference's fit is one treeAggregate whose seqOp
(WeightedLeastSquares.Aggregator.add) accumulates aaSum, abSum, aSum, bSum,
bbSum and wSum per instance, then a small solve on the driver.  Here the
aggregate is one weighted fp64 MFMA syrk over the augmented rows
z = [a, b, 1.0] (libcyclone's k_wls_tiles, cyc_wls_accumulate_dev): the
packed upper triangle U of sum_r w_r z_r z_r^T holds every field.  With
torch.distributed initialised each rank runs it on its shard and one
all-reduce of U is the combOp.  `WeightedLeastSquares.solve` is the driver
side on the packed moments, in numpy: standardization, the L2 diagonal, the
Cholesky solve with its inverse's diagonal, and the quasi-Newton solver
(cycloneml_amd.optimize's LBFGS / OWLQN) for L1 and for singular systems.

The reference's sources are not vendored; the semantics are restated and
pinned by the WeightedLeastSquaresSuite known answers in tests/.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np

from . import _native as N
from . import optimize, parallel

MAX_NUM_FEATURES = 4096


class SingularMatrixException(ArithmeticError):
    """CholeskyDecomposition.solve on a matrix that is not positive definite
    (org.apache.spark.ml.optim.SingularMatrixException)."""


def _torch():
    import torch
    return torch


def packed_to_full(U: np.ndarray, n: int) -> np.ndarray:
    """The symmetric n x n matrix of a packed upper triangle
    (U[j(j+1)/2 + i], i <= j)."""
    U = np.asarray(U, dtype=np.float64)
    if U.shape != (n * (n + 1) // 2,):
        raise N.IllegalArgumentException(
            f"requirement failed: packed triangle of order {n} has {n * (n + 1) // 2} "
            f"entries but got {U.shape}")
    M = np.empty((n, n), dtype=np.float64)
    # the lower triangle in row-major order (j, i) walks the packed upper one
    j, i = np.tril_indices(n)
    M[i, j] = U
    M[j, i] = U
    return M


class WLSPlan:
    """The weighted augmented syrk of width numFeatures + 2 (C ABI
    cyc_wls_*): U += sum_r w_r z_r z_r^T over a shard's rows."""

    def __init__(self, numFeatures: int):
        self._lib = N.load()
        h = ctypes.c_void_p()
        N.check(self._lib.cyc_wls_plan_create(int(numFeatures), ctypes.byref(h)))
        self.handle = h
        self.numFeatures = int(numFeatures)

    @property
    def packedSize(self) -> int:
        q = self.numFeatures + 2
        return q * (q + 1) // 2

    def close(self):
        if self.handle:
            self._lib.cyc_wls_plan_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def accumulate(self, X, y, w, U, stream=None):
        """Dense rows X (n x numFeatures, row-major), labels y, weights w
        (None: all 1).  Raises IllegalArgumentException on a negative weight."""
        N.check(self._lib.cyc_wls_accumulate_dev(
            self.handle, N.ptr(X), int(X.shape[0]), N.ptr(y), N.ptr(w), N.ptr(U),
            N.stream_handle(stream)))

    def accumulate_csr(self, rows, y, w, U, stream=None):
        N.check(self._lib.cyc_wls_accumulate_csr_dev(
            self.handle, N.ptr(rows.rowptr), N.ptr(rows.colidx), N.ptr(rows.values), rows.n,
            N.ptr(y), N.ptr(w), N.ptr(U), N.stream_handle(stream)))

    def last_splits(self) -> int:
        """Row splits of the last syrk launch (its split-K slabs)."""
        s = ctypes.c_int64()
        N.check(self._lib.cyc_wls_last_splits(self.handle, ctypes.byref(s)))
        return s.value


class WeightedLeastSquaresModel:
    def __init__(self, coefficients, intercept, diagInvAtWA, objectiveHistory):
        self.coefficients = np.asarray(coefficients, dtype=np.float64)
        self.intercept = float(intercept)
        self.diagInvAtWA = np.asarray(diagInvAtWA, dtype=np.float64)
        self.objectiveHistory = np.asarray(objectiveHistory, dtype=np.float64)

    def predict(self, features) -> float:
        return float(np.dot(self.coefficients, np.asarray(features, dtype=np.float64))
                     + self.intercept)


def _safe_div(num, den):
    """num / den, 0 where den is 0 (the reference's `if (std != 0.0)`)."""
    den = np.asarray(den, dtype=np.float64)
    ok = den != 0.0
    return np.where(ok, num / np.where(ok, den, 1.0), 0.0)


class WeightedLeastSquares:
    """WeightedLeastSquares(fitIntercept, regParam, elasticNetParam,
    standardizeFeatures, standardizeLabel, solverType, maxIter, tol)."""

    SOLVERS = ("auto", "cholesky", "quasi-newton")

    def __init__(self, fitIntercept: bool, regParam: float, elasticNetParam: float = 0.0,
                 standardizeFeatures: bool = True, standardizeLabel: bool = True,
                 solverType: str = "auto", maxIter: int = 100, tol: float = 1e-6):
        if not regParam >= 0.0:
            raise N.IllegalArgumentException(
                f"requirement failed: regParam cannot be negative: {regParam}")
        if not 0.0 <= elasticNetParam <= 1.0:
            raise N.IllegalArgumentException(
                f"requirement failed: elasticNetParam must be in [0, 1]: {elasticNetParam}")
        if not maxIter > 0:
            raise N.IllegalArgumentException(
                f"requirement failed: maxIter must be a positive integer: {maxIter}")
        if not tol >= 0.0:
            raise N.IllegalArgumentException(
                f"requirement failed: tol must be >= 0, but was set to {tol}")
        if solverType not in self.SOLVERS:
            raise N.IllegalArgumentException(f"Unsupported solver type: {solverType}")
        self.fitIntercept = bool(fitIntercept)
        self.regParam = float(regParam)
        self.elasticNetParam = float(elasticNetParam)
        self.standardizeFeatures = bool(standardizeFeatures)
        self.standardizeLabel = bool(standardizeLabel)
        self.solverType = solverType
        self.maxIter = int(maxIter)
        self.tol = float(tol)

    # -- the aggregate: one weighted syrk per shard, one all-reduce ---------------
    def moments(self, X, y, w=None, plan: Optional[WLSPlan] = None):
        """(U, count): the packed moments of this fit's rows, merged over
        ranks, on the device; count is the number of rows over ranks.  plan:
        a caller's WLSPlan of these rows' width, kept open (a fit repeated
        over the same rows, as IRLS does, holds one)."""
        from .linalg import CSRRows
        torch = _torch()
        sparse = isinstance(X, CSRRows)
        k = X.numCols if sparse else int(X.shape[1])
        n = X.n if sparse else int(X.shape[0])
        own = plan is None
        if own:
            plan = WLSPlan(k)
        try:
            # the last slot carries the row count through the same all-reduce
            buf = torch.zeros(plan.packedSize + 1, dtype=torch.float64, device=X.device)
            U = buf[:plan.packedSize]
            if sparse:
                plan.accumulate_csr(X, y, w, U)
            else:
                plan.accumulate(X, y, w, U)
            buf[plan.packedSize] = n
            parallel.allreduce_(buf)       # treeAggregate combOp: merge by addition
        finally:
            if own:
                plan.close()
        return U, int(buf[plan.packedSize].item())

    def fit(self, X, y, w=None, plan: Optional[WLSPlan] = None) -> WeightedLeastSquaresModel:
        """X: this rank's device rows (fp64 tensor n x k, or linalg.CSRRows);
        y, w: device fp64 vectors (w None: unit weights)."""
        from .linalg import CSRRows
        k = X.numCols if isinstance(X, CSRRows) else int(X.shape[1])
        U, count = self.moments(X, y, w, plan)
        return self.solve(U.cpu().numpy(), k, count=count)

    # -- the driver side ----------------------------------------------------------
    def solve(self, U, numFeatures: int, count: Optional[int] = None) -> WeightedLeastSquaresModel:
        """The model from the packed moments U of order numFeatures + 2
        (host).  count: the number of instances when known (0: the empty
        training set's error)."""
        k = int(numFeatures)
        if count is not None and count <= 0:
            raise N.IllegalArgumentException("requirement failed: Training dataset is empty.")
        M = packed_to_full(U, k + 2)
        wSum = M[k + 1, k + 1]
        if not wSum > 0.0:
            raise N.IllegalArgumentException("requirement failed: Sum of weights cannot be zero.")
        aBar = M[:k, k + 1] / wSum
        rawBBar = M[k, k + 1] / wSum
        aaBar = M[:k, :k] / wSum
        abBar = M[:k, k] / wSum
        rawBbBar = M[k, k] / wSum
        aStd = np.sqrt(np.maximum(np.diag(aaBar) - aBar * aBar, 0.0))
        rawBStd = float(np.sqrt(max(rawBbBar - rawBBar * rawBBar, 0.0)))
        bStd = abs(rawBBar) if rawBStd == 0.0 else rawBStd

        if rawBStd == 0.0:
            if self.fitIntercept or rawBBar == 0.0:
                # a constant label: zero coefficients, the label as the intercept
                return WeightedLeastSquaresModel(np.zeros(k), rawBBar, [0.0], [0.0])
            if self.regParam > 0.0 and self.standardizeLabel:
                raise N.IllegalArgumentException(
                    "requirement failed: The standard deviation of the label is zero. Model "
                    "cannot be regularized when labels are standardized.")

        # the standardized space
        bBar = rawBBar / bStd
        bbBar = rawBbBar / (bStd * bStd)
        aBar = _safe_div(aBar, aStd)
        abBar = _safe_div(abBar, aStd * bStd)
        aaBar = _safe_div(aaBar, np.outer(aStd, aStd))

        effReg = self.regParam / bStd
        effL1 = self.elasticNetParam * effReg
        effL2 = (1.0 - self.elasticNetParam) * effReg
        lam = np.full(k, effL2)
        if not self.standardizeFeatures:
            lam = _safe_div(lam, aStd * aStd)
        if not self.standardizeLabel:
            lam = lam * bStd
        aaBar = aaBar.copy()
        aaBar[np.diag_indices(k)] += lam

        # getAtA / getAtB: with an intercept one more row and column [aBar, 1.0]
        if self.fitIntercept:
            aa = np.empty((k + 1, k + 1))
            aa[:k, :k] = aaBar
            aa[:k, k] = aa[k, :k] = aBar
            aa[k, k] = 1.0
            ab = np.append(abBar, bBar)
        else:
            aa, ab = aaBar, abBar

        def l1fun(index):
            if self.fitIntercept and index == k:
                return 0.0
            if self.standardizeFeatures:
                return effL1
            return effL1 / aStd[index] if aStd[index] != 0.0 else 0.0

        quasi = self.solverType == "quasi-newton" or (
            self.solverType == "auto" and self.elasticNetParam != 0.0 and self.regParam != 0.0)
        if quasi:
            x, aaInvDiag, history = self._quasi_newton(
                bBar, bbBar, ab, aa, aBar, l1fun if effL1 != 0.0 else None)
        else:
            try:
                x, aaInvDiag, history = self._cholesky(ab, aa)
            except SingularMatrixException:
                if self.solverType != "auto":
                    raise
                # Cholesky failed on a singular system: the quasi-Newton
                # solver, without L1, finds a solution of it
                x, aaInvDiag, history = self._quasi_newton(bBar, bbBar, ab, aa, aBar, None)

        intercept = x[k] * bStd if self.fitIntercept else 0.0
        coef = x[:k] * _safe_div(bStd, aStd)
        if aaInvDiag is None:
            diag = np.array([0.0])
        else:
            mult = aStd * aStd
            if self.fitIntercept:
                mult = np.append(mult, 1.0)
            with np.errstate(divide="ignore", invalid="ignore"):
                diag = aaInvDiag / (wSum * mult)
        return WeightedLeastSquaresModel(coef, intercept, diag,
                                         [0.0] if history is None else history)

    @staticmethod
    def _cholesky(ab, aa):
        """CholeskySolver: dppsv, then dpptri for the inverse's diagonal."""
        try:
            L = np.linalg.cholesky(aa)
        except np.linalg.LinAlgError:
            raise SingularMatrixException(
                "A is not positive definite. Is A derived from a singular matrix (e.g. "
                "collinear column values)?") from None
        if not np.all(np.isfinite(L)) or np.any(np.diag(L) <= 0.0):
            raise SingularMatrixException(
                "A is not positive definite. Is A derived from a singular matrix (e.g. "
                "collinear column values)?")
        n = aa.shape[0]
        z = np.linalg.solve(L, np.column_stack([ab, np.eye(n)]))   # L^-1 [ab, I]
        x = np.linalg.solve(L.T, z[:, 0])
        Linv = z[:, 1:]
        aaInvDiag = np.einsum("ij,ij->j", Linv, Linv)              # diag(L^-T L^-1)
        return x, aaInvDiag, None

    def _quasi_newton(self, bBar, bbBar, ab, aa, aBar, l1fun):
        """QuasiNewtonSolver on NormalEquationCostFun."""
        k = aBar.shape[0]
        fitIntercept = self.fitIntercept
        x0 = np.zeros(k + 1 if fitIntercept else k)
        if fitIntercept:
            x0[k] = bBar

        def cost(x):
            if fitIntercept:
                # the intercept in closed form, written into the iterate as the
                # reference does (the vector handed in is the optimizer's own)
                x[k] = bBar - float(np.dot(x[:k], aBar))
            aax = aa @ x
            loss = 0.5 * bbBar - float(np.dot(ab, x)) + 0.5 * float(np.dot(x, aax))
            return loss, aax - ab

        if l1fun is not None:
            opt = optimize.OWLQN(self.maxIter, 10, l1fun, self.tol)
        else:
            opt = optimize.LBFGS(self.maxIter, 10, self.tol)
        history = []
        state = None
        for state in opt.iterations(cost, x0):
            history.append(state.adjustedValue)
        return state.x.copy(), None, history


class LinearRegressionModel:
    """coefficients, intercept and scale (1.0 for squaredError) of a fitted
    LinearRegression."""

    def __init__(self, coefficients, intercept: float, scale: float = 1.0,
                 objectiveHistory=(0.0,), diagInvAtWA=(0.0,)):
        self.coefficients = np.asarray(coefficients, dtype=np.float64)
        self.intercept = float(intercept)
        self.scale = float(scale)
        self.objectiveHistory = np.asarray(objectiveHistory, dtype=np.float64)
        self.diagInvAtWA = np.asarray(diagInvAtWA, dtype=np.float64)
        self._coef_dev = None

    @property
    def numFeatures(self) -> int:
        return int(self.coefficients.shape[0])

    def predict(self, X):
        """dot(features, coefficients) + intercept: for device rows (fp64
        tensor n x numFeatures) a device vector of n predictions; for one
        host vector a float."""
        torch = _torch()
        if isinstance(X, torch.Tensor):
            if self._coef_dev is None or self._coef_dev.device != X.device:
                self._coef_dev = torch.from_numpy(self.coefficients).to(X.device)
            if X.shape[-1] != self.numFeatures:
                raise N.IllegalArgumentException(
                    f"requirement failed: expected {self.numFeatures} features but got "
                    f"{X.shape[-1]}")
            return X @ self._coef_dev + self.intercept
        v = np.asarray(X, dtype=np.float64)
        return float(np.dot(v, self.coefficients) + self.intercept)


class LinearRegression:
    """LinearRegression estimator over device-resident rows.  solver "normal"
    (and "auto" up to 4096 features) is the WeightedLeastSquares fit."""

    def __init__(self, maxIter: int = 100, regParam: float = 0.0, elasticNetParam: float = 0.0,
                 tol: float = 1e-6, fitIntercept: bool = True, standardization: bool = True,
                 solver: str = "auto", loss: str = "squaredError"):
        if solver not in ("auto", "normal", "l-bfgs"):
            raise N.IllegalArgumentException(f"LinearRegression: unsupported solver {solver}")
        if loss not in ("squaredError", "huber"):
            raise N.IllegalArgumentException(f"LinearRegression: unsupported loss {loss}")
        self.maxIter = int(maxIter)
        self.regParam = float(regParam)
        self.elasticNetParam = float(elasticNetParam)
        self.tol = float(tol)
        self.fitIntercept = bool(fitIntercept)
        self.standardization = bool(standardization)
        self.solver = solver
        self.loss = loss

    def fit(self, X, y, weights=None) -> LinearRegressionModel:
        from .linalg import CSRRows
        numFeatures = X.numCols if isinstance(X, CSRRows) else int(X.shape[1])
        if self.loss == "huber":
            raise NotImplementedError(
                "LinearRegression(loss='huber') is not implemented: it is the l-bfgs loop over "
                "the device HuberBlockAggregator (optim.HuberBlockAggregator)")
        if self.solver == "normal" or (self.solver == "auto" and numFeatures <= MAX_NUM_FEATURES):
            wls = WeightedLeastSquares(self.fitIntercept, self.regParam, self.elasticNetParam,
                                       standardizeFeatures=self.standardization,
                                       standardizeLabel=True, solverType="auto",
                                       maxIter=self.maxIter, tol=self.tol)
            m = wls.fit(X, y, weights)
            return LinearRegressionModel(m.coefficients, m.intercept, 1.0, m.objectiveHistory,
                                         m.diagInvAtWA)
        raise NotImplementedError(
            f"LinearRegression(solver='{self.solver}') with {numFeatures} features is not "
            "implemented: it is the l-bfgs loop over the device LeastSquaresBlockAggregator "
            "(optim.LeastSquaresBlockAggregator); only the normal-equation fit (solver "
            f"'normal', or 'auto' up to {MAX_NUM_FEATURES} features) is")
