"""LinearRegression by the normal equations: the host side of
ml/optim/WeightedLeastSquares.scala and of the `Auto | Normal` branch of
ml/regression/LinearRegression.scala.

The reference's fit is one treeAggregate whose seqOp
(WeightedLeastSquares.Aggregator.add) accumulates aaSum, abSum, aSum, bSum,
bbSum and wSum per instance, then a small solve on the driver.  Here the
aggregate is one weighted fp64 MFMA syrk over the augmented rows
z = [a, b, 1.0] (libcyclone's k_wls_tiles in wls.hip, cyc_wls_accumulate_dev): the
packed upper triangle U of sum_r w_r z_r z_r^T holds every field.  With
torch.distributed initialised each rank runs it on its shard and one
all-reduce of U is the combOp.  `WeightedLeastSquares.solve` is the driver
side on the packed moments, in numpy: standardization, the L2 diagonal, the
Cholesky solve with its inverse's diagonal, and the quasi-Newton solver
(cycloneml_amd.optimize's LBFGS / OWLQN) for L1 and for singular systems.

Every other LinearRegression fit (solver "l-bfgs", "auto" above 4096
features, loss "huber") is the reference's quasi-Newton branch:
`LinearRegression.train_from_summary` drives LBFGS / OWLQN / LBFGSB over a
cost callable, which on the device is `BlockCost`: one
LeastSquaresBlockAggregator / HuberBlockAggregator add over the shard plus
its all-reduce per evaluation.  Predictions over CSR rows and the model's
summary come from libcyclone's evaluate pass (regression_summary.py).

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
                 objectiveHistory=(0.0,), diagInvAtWA=(0.0,), fitIntercept: bool = True):
        self.coefficients = np.asarray(coefficients, dtype=np.float64)
        self.intercept = float(intercept)
        self.scale = float(scale)
        self.objectiveHistory = np.asarray(objectiveHistory, dtype=np.float64)
        self.diagInvAtWA = np.asarray(diagInvAtWA, dtype=np.float64)
        self.fitIntercept = bool(fitIntercept)
        self._coef_dev = None
        self._inference = False    # diagInvAtWA of an unregularized normal-equation fit
        self._training = None      # (X, y, weights, yMean) of the fit, for `summary`
        self._summary = None

    @property
    def numFeatures(self) -> int:
        return int(self.coefficients.shape[0])

    def _coefficients_on(self, device):
        torch = _torch()
        if self._coef_dev is None or self._coef_dev.device != device:
            self._coef_dev = torch.from_numpy(self.coefficients).to(device)
        return self._coef_dev

    @property
    def hasSummary(self) -> bool:
        return self._training is not None

    @property
    def summary(self):
        """LinearRegressionTrainingSummary of the rows this model was fitted
        on, built on first access: one stats pass, none inside fit."""
        if self._training is None:
            raise RuntimeError("No training summary available for this LinearRegressionModel")
        if self._summary is None:
            from .regression_summary import LinearRegressionTrainingSummary
            X, y, w, yMean = self._training
            self._summary = LinearRegressionTrainingSummary(self, X, y, w, yMean,
                                                            self.objectiveHistory)
        return self._summary

    def evaluate(self, X, y, weights=None):
        """LinearRegressionSummary of this model on (X, y, weights): X an fp64
        device tensor n x numFeatures or linalg.CSRRows."""
        from .regression_summary import LinearRegressionSummary
        return LinearRegressionSummary(self, X, y, weights)

    def predict(self, X):
        """dot(features, coefficients) + intercept: for device rows (fp64
        tensor n x numFeatures, or linalg.CSRRows) a device vector of n
        predictions; for one host vector a float."""
        from .linalg import CSRRows
        torch = _torch()
        if isinstance(X, CSRRows):
            from .regression_summary import linreg_predict
            if X.numCols != self.numFeatures:
                raise N.IllegalArgumentException(
                    f"requirement failed: expected {self.numFeatures} features but got "
                    f"{X.numCols}")
            return linreg_predict(X, self._coefficients_on(X.device), self.intercept)
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


class _L2:
    """L2Regularization over the first nreg parameters: 0.5 regParam sum c_j^2;
    with std given (standardization = false) c_j^2 / std_j^2, 0 where std_j
    is 0 (classification._L2 restated for one coefficient set)."""

    def __init__(self, regParam, nreg, std=None):
        self.regParam, self.nreg = float(regParam), int(nreg)
        self.mult = np.ones(nreg) if std is None else _safe_div(1.0, np.asarray(std) ** 2)

    def calculate(self, x):
        t = x[:self.nreg] * self.mult
        g = np.zeros_like(x)
        g[:self.nreg] = self.regParam * t
        return 0.5 * self.regParam * float(np.dot(x[:self.nreg], t)), g


class BlockCost:
    """RDDLossFunction.calculate over one device shard for the parameters of
    the STANDARDIZED problem, without the regularization term: the rows stay
    as they are, the parameters go in multiplied by `scale` (inverseStd for
    the linear terms, 1 for intercept and sigma slots) and the gradient comes
    back multiplied by it.  One evaluation is one aggregator add over the
    block plus the aggregator's all-reduce.  make_aggregator(raw parameters)
    returns a fresh optim.DifferentiableLossAggregator (least squares and
    Huber here; hinge and AFT take the same shape)."""

    def __init__(self, block, make_aggregator, scale):
        self.block = block
        self.make_aggregator = make_aggregator
        self.scale = np.asarray(scale, dtype=np.float64)
        self.evaluations = 0

    def __call__(self, x):
        agg = self.make_aggregator(x * self.scale)
        agg.add(self.block)
        agg.allreduce()
        self.evaluations += 1
        return agg.loss, agg.gradient * self.scale


class LinearRegression:
    """LinearRegression estimator over device-resident rows.

    loss "squaredError" with solver "normal", or "auto" up to 4096 features:
    the WeightedLeastSquares fit (one weighted syrk, a host solve).
    loss "squaredError" otherwise: LBFGS / OWLQN over the device
    LeastSquaresBlockAggregator on standardized features and label.
    loss "huber": LBFGSB over the device HuberBlockAggregator, parameters
    [coefficients, intercept, sigma], L2 only."""

    def __init__(self, maxIter: int = 100, regParam: float = 0.0, elasticNetParam: float = 0.0,
                 tol: float = 1e-6, fitIntercept: bool = True, standardization: bool = True,
                 solver: str = "auto", loss: str = "squaredError", epsilon: float = 1.35):
        if solver not in ("auto", "normal", "l-bfgs"):
            raise N.IllegalArgumentException(f"LinearRegression: unsupported solver {solver}")
        if loss not in ("squaredError", "huber"):
            raise N.IllegalArgumentException(f"LinearRegression: unsupported loss {loss}")
        if not epsilon > 1.0:
            raise N.IllegalArgumentException(
                f"LinearRegression: epsilon given invalid value {epsilon}, must be > 1.0")
        if loss == "huber" and elasticNetParam != 0.0:
            raise N.IllegalArgumentException(
                "requirement failed: LinearRegression with huber loss only supports L2 "
                f"regularization, but got elasticNetParam = {elasticNetParam}.")
        if loss == "huber" and solver == "normal":
            raise N.IllegalArgumentException(
                "requirement failed: LinearRegression with huber loss doesn't support normal "
                "solver, please change solver to auto or l-bfgs.")
        self.epsilon = float(epsilon)
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
        if self.loss == "squaredError" and (
                self.solver == "normal" or
                (self.solver == "auto" and numFeatures <= MAX_NUM_FEATURES)):
            wls = WeightedLeastSquares(self.fitIntercept, self.regParam, self.elasticNetParam,
                                       standardizeFeatures=self.standardization,
                                       standardizeLabel=True, solverType="auto",
                                       maxIter=self.maxIter, tol=self.tol)
            m = wls.fit(X, y, weights)
            model = LinearRegressionModel(m.coefficients, m.intercept, 1.0, m.objectiveHistory,
                                          m.diagInvAtWA, self.fitIntercept)
            # standard errors need the unregularized inverse
            model._inference = self.regParam == 0.0
            model._training = (X, y, weights, None)
            return model
        return self._fit_quasi_newton(X, y, weights, numFeatures)

    def _fit_quasi_newton(self, X, y, weights, numFeatures):
        """The summaries (features: the device summarizer; label: a one-column
        one), then train_from_summary over the device aggregators."""
        from . import optim
        from .linalg import CSRRows
        from .stat import SummarizerBuffer
        if not isinstance(X, CSRRows) and not _torch().is_tensor(X):
            # outside fit's contract (device rows); there is no host data pass
            aggregator = "HuberBlockAggregator" if self.loss == "huber" \
                else "LeastSquaresBlockAggregator"
            raise NotImplementedError(
                f"LinearRegression(loss='{self.loss}', solver='{self.solver}') with "
                f"{numFeatures} features over host rows ({type(X).__name__}) is not "
                f"implemented: the fit runs over the device {aggregator} "
                f"(optim.{aggregator}), which takes an fp64 device tensor or linalg.CSRRows")
        device = y.device
        if isinstance(X, CSRRows):
            block = optim.DeviceInstanceBlock(y, weights, rowptr=X.rowptr, colidx=X.colidx,
                                              values=X.values, numFeatures=numFeatures)
        else:
            block = optim.DeviceInstanceBlock(y, weights, X=X.contiguous())
        feat = SummarizerBuffer.of_block(block).allgather_merge()
        lab = SummarizerBuffer.of_dense(y.reshape(-1, 1), weights).allgather_merge()
        if feat.count <= 0:
            raise N.IllegalArgumentException("requirement failed: Training dataset is empty.")
        if not feat.weightSum > 0.0:
            raise N.IllegalArgumentException("requirement failed: Sum of weights cannot be zero.")
        if block.is_sparse:
            # the layout the binary aggregators run on, once per fit
            block.prepare(layout="tiles")

        def make_cost(loss, fitIntercept, inverseStd, featuresMean, labelStd, labelMean, epsilon):
            # raw rows: the aggregator sees unit inverseStd and the unscaled mean
            ones = np.ones(numFeatures)
            mean = np.asarray(featuresMean, dtype=np.float64) if fitIntercept else None
            if loss == "huber":
                scale = np.ones(numFeatures + (2 if fitIntercept else 1))
                scale[:numFeatures] = inverseStd
                make = lambda raw: optim.HuberBlockAggregator(  # noqa: E731
                    ones, mean, fitIntercept, epsilon, raw, device=device)
            else:
                scale = inverseStd
                make = lambda raw: optim.LeastSquaresBlockAggregator(  # noqa: E731
                    ones, mean, fitIntercept, labelStd, labelMean, raw, device=device)
            # kept as lastCost: its evaluations count the data passes
            self.lastCost = BlockCost(block, make, scale)
            return self.lastCost

        yMean, yStd = float(lab.mean[0]), float(lab.std[0])
        model = self.train_from_summary(numFeatures, feat.mean, feat.std, yMean, yStd,
                                        feat.weightSum, make_cost)
        model._training = (X, y, weights, yMean)
        return model

    def train_from_summary(self, numFeatures: int, featuresMean, featuresStd, yMean: float,
                           yStd: float, weightSum: float, make_cost) -> LinearRegressionModel:
        """The driver logic of the quasi-Newton fits once the summaries exist.
        make_cost(loss, fitIntercept, inverseStd, featuresMean, labelStd,
        labelMean, epsilon) returns a function: parameters of the SCALED
        problem -> (loss, gradient) without the regularization term, i.e. one
        pass of LeastSquaresBlockAggregator (labelStd, labelMean given, epsilon
        None) or HuberBlockAggregator (epsilon given) over the standardized
        rows."""
        F = int(numFeatures)
        featuresMean = np.asarray(featuresMean, dtype=np.float64)
        featuresStd = np.asarray(featuresStd, dtype=np.float64)
        yMean, yStd = float(yMean), float(yStd)
        if not weightSum > 0.0:
            raise N.IllegalArgumentException("requirement failed: Sum of weights cannot be zero.")
        if not self.regParam >= 0.0:
            raise N.IllegalArgumentException(
                f"requirement failed: regParam cannot be negative: {self.regParam}")
        if not 0.0 <= self.elasticNetParam <= 1.0:
            raise N.IllegalArgumentException(
                "requirement failed: elasticNetParam must be in [0, 1]: "
                f"{self.elasticNetParam}")
        inverseStd = _safe_div(1.0, featuresStd)
        stdOf = None if self.standardization else featuresStd
        if self.loss == "huber":
            return self._train_huber(F, featuresMean, inverseStd, stdOf, make_cost)

        if yStd == 0.0:
            if self.fitIntercept or yMean == 0.0:
                # a constant label: zero coefficients, the label as the intercept
                return LinearRegressionModel(np.zeros(F), yMean, 1.0, [0.0],
                                             fitIntercept=self.fitIntercept)
            if self.regParam != 0.0:
                raise N.IllegalArgumentException(
                    "requirement failed: The standard deviation of the label is zero. Model "
                    "cannot be regularized.")
            yStd = abs(yMean)
        effReg = self.regParam / yStd
        effL1 = self.elasticNetParam * effReg
        effL2 = (1.0 - self.elasticNetParam) * effReg
        cost = make_cost("squaredError", self.fitIntercept, inverseStd, featuresMean, yStd, yMean,
                         None)
        regularization = _L2(effL2, F, stdOf) if effL2 != 0.0 else None
        if effL1 != 0.0:
            l1 = np.full(F, effL1) if self.standardization else _safe_div(effL1, featuresStd)
            optimizer = optimize.OWLQN(self.maxIter, 10, l1, self.tol)
        else:
            optimizer = optimize.LBFGS(self.maxIter, 10, self.tol)
        state, history = self._minimize(optimizer, cost, regularization, np.zeros(F))
        coef = state.x * inverseStd * yStd
        intercept = yMean - float(np.dot(coef, featuresMean)) if self.fitIntercept else 0.0
        return LinearRegressionModel(coef, intercept, 1.0, history,
                                     fitIntercept=self.fitIntercept)

    def _train_huber(self, F, featuresMean, inverseStd, stdOf, make_cost):
        fitIntercept = self.fitIntercept
        dim = F + (2 if fitIntercept else 1)
        cost = make_cost("huber", fitIntercept, inverseStd, featuresMean, None, None,
                         self.epsilon)
        regularization = _L2(self.regParam, F, stdOf) if self.regParam != 0.0 else None
        lower = np.full(dim, -np.inf)
        lower[dim - 1] = np.finfo(np.float64).tiny      # sigma > 0
        optimizer = optimize.LBFGSB(lower, np.full(dim, np.inf), self.maxIter, 10, self.tol)
        x0 = np.zeros(dim)
        x0[dim - 1] = 1.0
        # the aggregator centres whenever it fits an intercept: its intercept
        # slot is the intercept of the centred rows (0 . scaledMean at x0)
        state, history = self._minimize(optimizer, cost, regularization, x0)
        sol = state.x
        coef = sol[:F] * inverseStd
        intercept = 0.0
        if fitIntercept:
            intercept = sol[F] - float(np.dot(coef, featuresMean))
        return LinearRegressionModel(coef, intercept, float(sol[dim - 1]), history,
                                     fitIntercept=fitIntercept)

    def _minimize(self, optimizer, cost, regularization, x0):
        def fn(x):
            loss, grad = cost(x)
            if regularization is not None:
                rl, rg = regularization.calculate(x)
                loss, grad = loss + rl, grad + rg
            return loss, grad

        history, state, last = [], None, None
        for state in optimizer.iterations(fn, x0):
            if state is not last:          # LBFGSB yields a failed state twice
                history.append(state.adjustedValue)
            last = state
        if state is None:
            raise RuntimeError(f"{type(optimizer).__name__} failed.")
        self.lastState = state
        return state, history
