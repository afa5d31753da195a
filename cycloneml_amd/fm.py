"""FMRegressor / FMClassifier (ml/regression/FMRegressor.scala, ml/classification/
FMClassifier.scala and mllib/optimization/GradientDescent.scala, Spark 3.3) over
device rows: dense fp64 (csrc/fm.hip, cyc_fm_* in include/cyclone.h, up to
65 535 features) or CSR (linalg.CSRRows, or FMSparseRows prepared from them
once; csrc/fm_csr.hip, cyc_fmcsr_*, any number of features, a stored zero
contributes nothing).  The caller chooses the layout; every rank of one fit
uses the same one.

Coefficients: one flat fp64 vector [V (d x k row-major) | w (d, fitLinear) | b
(1, fitIntercept)].  Per row, i and f ascending, every product rounded before its
add: raw = b + sum_i w_i x_i (x_i == 0 skipped), then per factor s_f = sum_i
V[i,f] x_i, q_f = sum_i (V[i,f] x_i)^2, raw += 0.5 (s_f s_f - q_f).

    squared   prediction raw      loss (raw - y)^2                m = 2 (raw - y)
    logistic  p = 1/(1+exp(-raw)) loss y > 0 ? log1pExp(-raw)     m = p - y
                                              : log1pExp(raw)

Row gradient: gb = 1, gw_i = x_i, gV[i,f] = x_i s_f - V[i,f] x_i x_i.  One
evaluation returns G = sum m (row gradient), L = sum loss, cnt = rows taken.

Fit (GradientDescent.runMiniBatchSGD): regVal = updater(w, 0, 0, 1, regParam)'s;
for i = 1 .. maxIter while not converged, evaluate batch i; when cnt > 0:
history += L / cnt + regVal, (w, regVal) = updater(w, G / cnt, stepSize, i,
regParam); from the second update on the fit has converged when ||prev - cur|| <
tol max(||cur||, 1).  Updaters, each elementwise op rounded once:

    gd     eta = stepSize / sqrt(i); w <- w (1 - eta regParam); w <- w + (-eta) g
    adamW  m <- m b1 + (1 - b1) g; v <- v b2 + (1 - b2) (g g); b1T <- b1T b1;
           b2T <- b2T b2; w <- w - ((stepSize mHat) / (sqrt(vHat) + eps) + regParam w)
           with mHat = m / (1 - b1T), vHat = v / (1 - b2T); only when stepSize > 0

and regVal = 0.5 regParam ||w||^2.  The step objects FMDeviceStep (the kernels;
[G | L | cnt] goes through one parallel.allreduce_ per iteration, the updaters run
as device tensor ops) and FMNumpyStep (the literal per-row loop on host rows) are
interchangeable: evaluate(coef, i) -> (G, L, cnt).

This package's own rules: below miniBatchFraction 1 global row r is in batch i iff
the top 53 bits of forest.mix(42 + i, 0, 0, r) are >= forest.bernoulli_table(
fraction)[0] (Spark's RDD.sample is not restated; fraction 1 reproduces Spark);
the initial factors are java.util.Random(seed).nextGaussian() initStd with
StrictMath.log / sqrt taken as math.log / math.sqrt.  Out of scope: a weight
column, Spark's own mini-batch draws, thresholds, transform, factorSize above
64, an automatic choice between the dense and the CSR layout, a sparse gradient
or allreduce, a CSR FMNumpyStep.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np

from . import _native as N
from . import forest as RF
from .ann import java_string_hash
from .gbt import log1p_exp
from .kmeans_init import JavaRandom
from .tree import _require

LOSSES = {"squared": 0, "logistic": 1}          # cyc_fm_plan_create's codes
SOLVERS = ("gd", "adamW")
MAX_FACTORS = 64
REGRESSOR_SEED = java_string_hash("org.apache.spark.ml.regression.FMRegressor")
CLASSIFIER_SEED = java_string_hash("org.apache.spark.ml.classification.FMClassifier")
BETA1, BETA2, EPSILON = 0.9, 0.999, 1e-8


def coef_len(d: int, k: int, fitIntercept: bool, fitLinear: bool) -> int:
    return d * k + (d if fitLinear else 0) + (1 if fitIntercept else 0)


def split_coef(coef, d: int, k: int, fitIntercept: bool, fitLinear: bool):
    """(intercept, linear (d; zeros without fitLinear), factors (d x k)) of
    host coefficients."""
    coef = np.asarray(coef, dtype=np.float64)
    _require(coef.size == coef_len(d, k, fitIntercept, fitLinear),
             f"the coefficients must hold {coef_len(d, k, fitIntercept, fitLinear)} values but "
             f"hold {coef.size}")
    V = coef[:d * k].reshape(d, k).copy()
    w = coef[d * k:d * k + d].copy() if fitLinear else np.zeros(d)
    b = float(coef[-1]) if fitIntercept else 0.0
    return b, w, V


def check_fm_params(factorSize, regParam, miniBatchFraction, initStd, maxIter, stepSize, tol,
                    solver):
    _require(1 <= int(factorSize) <= MAX_FACTORS,
             f"factorSize must be in [1, {MAX_FACTORS}] but got {factorSize}.")
    _require(0.0 < float(miniBatchFraction) <= 1.0,
             f"miniBatchFraction must be in (0, 1] but got {miniBatchFraction}.")
    _require(float(stepSize) > 0.0, f"stepSize must be positive but got {stepSize}.")
    _require(float(regParam) >= 0.0, f"regParam must not be negative but got {regParam}.")
    _require(float(tol) >= 0.0, f"tol must not be negative but got {tol}.")
    _require(float(initStd) >= 0.0, f"initStd must not be negative but got {initStd}.")
    _require(int(maxIter) >= 0, f"maxIter must not be negative but got {maxIter}.")
    if solver not in SOLVERS:
        raise N.IllegalArgumentException(
            f"solver given invalid value {solver}. Supported options: {', '.join(SOLVERS)}.")


def init_coef(d: int, k: int, fitIntercept: bool, fitLinear: bool, initStd: float, seed: int):
    rnd = JavaRandom(seed)
    coef = np.zeros(coef_len(d, k, fitIntercept, fitLinear))
    for e in range(d * k):
        coef[e] = rnd.next_gaussian() * float(initStd)
    return coef


def batch_rows(i: int, fraction: float, n: int, rowOffset: int = 0):
    """The mask of the rows rowOffset .. rowOffset + n taken by batch i."""
    if float(fraction) >= 1.0:
        return np.ones(n, dtype=bool)
    rows = np.arange(int(rowOffset), int(rowOffset) + n, dtype=np.uint64)
    u = RF.mix(42 + int(i), 0, 0, rows) >> np.uint64(11)
    return u >= RF.bernoulli_table(fraction)[0]


# ------------------------------------------------------------------------ rows
class FMSparseRows:
    """cyc_fmcsr_rows: a CSRRows shard prepared once for the CSR kernels (the
    index check, the column-major copy and its segment table).  It keeps the
    shard's arrays alive; a slice whose rowptr[0] > 0 is rebased here."""

    def __init__(self, csr):
        import torch
        from .linalg import CSRRows
        _require(isinstance(csr, CSRRows), "FMSparseRows takes CSRRows")
        rowptr, colidx, values = csr.rowptr, csr.colidx, csr.values
        _require(rowptr.is_cuda and rowptr.dtype == torch.int64 and colidx.dtype == torch.int32
                 and values.dtype == torch.float64 and colidx.numel() == values.numel(),
                 "CSR rows are int64 rowptr, int32 colidx and fp64 values on the device")
        self.n, self.d, self.device = csr.n, csr.numCols, csr.device
        base = int(rowptr[0]) if self.n > 0 else 0
        if base:
            rowptr = rowptr - base
        self._arrays = (rowptr.contiguous(), colidx.contiguous(), values.contiguous())
        self._lib = N.load()
        self.segmentEntries = int(self._lib.cyc_fmcsr_segment_entries())
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            N.check(self._lib.cyc_fmcsr_rows_create(*(N.ptr(t) for t in self._arrays), self.n,
                                                    self.d, N.stream_handle(), ctypes.byref(h)))
        self.handle = h

    def close(self):
        if getattr(self, "handle", None):
            self._lib.cyc_fmcsr_rows_destroy(self.handle)
            self.handle = None

    __del__ = close


def as_rows(X):
    """Dense rows and FMSparseRows as they are; CSRRows prepared."""
    from .linalg import CSRRows
    return FMSparseRows(X) if isinstance(X, CSRRows) else X


# ------------------------------------------------------------------------ plan
class FMPlan:
    """cyc_fm_plan: the shape, the flags, the loss and the scratch of the calls."""

    def __init__(self, numFeatures: int, factorSize: int, fitIntercept: bool = True,
                 fitLinear: bool = True, loss: str = "squared", workspaceBytes: int = 0):
        _require(loss in LOSSES, f"unknown loss {loss}")
        self.d, self.k = int(numFeatures), int(factorSize)
        self.fitIntercept, self.fitLinear, self.loss = bool(fitIntercept), bool(fitLinear), loss
        self.coefLen = coef_len(self.d, self.k, self.fitIntercept, self.fitLinear)
        self._lib = N.load()
        h = ctypes.c_void_p()
        N.check(self._lib.cyc_fm_plan_create(self.d, self.k, int(self.fitIntercept),
                                             int(self.fitLinear), LOSSES[loss],
                                             int(workspaceBytes), ctypes.byref(h)))
        self.handle = h
        self.runRows = int(self._lib.cyc_fm_run_rows())
        self.tileRows = int(self._lib.cyc_fm_tile_rows())
        self.fusedFeatures = int(self._lib.cyc_fm_fused_features(self.k))

    def close(self):
        if getattr(self, "handle", None):
            self._lib.cyc_fm_plan_destroy(self.handle)
            self.handle = None

    __del__ = close

    def _rows(self, X) -> int:
        import torch
        if isinstance(X, FMSparseRows):
            _require(X.d == self.d,
                     f"the rows have {X.d} features but the plan has {self.d}")
            return X.n
        _require(torch.is_tensor(X) and X.is_cuda and X.dtype == torch.float64 and X.dim() == 2
                 and X.is_contiguous(), "rows must be a contiguous fp64 device tensor (n x d)")
        _require(int(X.shape[1]) == self.d,
                 f"the rows have {int(X.shape[1])} features but the plan has {self.d}")
        return int(X.shape[0])

    @staticmethod
    def _vector(t, size, what):
        import torch
        _require(torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float64
                 and t.is_contiguous() and t.numel() == size,
                 f"{what} must be a contiguous fp64 device tensor of {size} values")

    def evaluate(self, X, y, coef, out=None, iter: int = 1, fraction: float = 1.0,
                 rowOffset: int = 0):
        """out (device, coefLen + 2) = [G | L | cnt] of batch `iter` of this
        shard, whose first row is global row rowOffset."""
        import torch
        X = as_rows(X)
        n = self._rows(X)
        self._vector(y, n, "labels")
        self._vector(coef, self.coefLen, "coef")
        if out is None:
            out = torch.empty(self.coefLen + 2, dtype=torch.float64, device=X.device)
        self._vector(out, self.coefLen + 2, "out")
        with torch.cuda.device(X.device):
            if isinstance(X, FMSparseRows):
                N.check(self._lib.cyc_fmcsr_evaluate_dev(
                    self.handle, X.handle, N.ptr(y), N.ptr(coef), int(iter), float(fraction),
                    int(rowOffset), N.ptr(out), N.stream_handle()))
                return out
            N.check(self._lib.cyc_fm_evaluate_dev(self.handle, N.ptr(X), N.ptr(y), n, N.ptr(coef),
                                                  int(iter), float(fraction), int(rowOffset),
                                                  N.ptr(out), N.stream_handle()))
        return out

    def predict(self, X, coef, margin=False, raw=False, prob=False, pred=False):
        """(margin n, raw n x 2, prob n x 2, pred n) device tensors (None for
        what is not asked for)."""
        import torch
        X = as_rows(X)
        n = self._rows(X)
        self._vector(coef, self.coefLen, "coef")
        new = lambda want, *shape: (torch.empty(shape, dtype=torch.float64, device=X.device)
                                    if want else None)          # noqa: E731
        mg, r, q, p = new(margin, n), new(raw, n, 2), new(prob, n, 2), new(pred, n)
        with torch.cuda.device(X.device):
            if isinstance(X, FMSparseRows):
                N.check(self._lib.cyc_fmcsr_predict_dev(
                    self.handle, X.handle, N.ptr(coef), N.ptr(mg), N.ptr(r), N.ptr(q), N.ptr(p),
                    N.stream_handle()))
                return mg, r, q, p
            N.check(self._lib.cyc_fm_predict_dev(self.handle, N.ptr(X), n, N.ptr(coef), N.ptr(mg),
                                                 N.ptr(r), N.ptr(q), N.ptr(p), N.stream_handle()))
        return mg, r, q, p


# ----------------------------------------------------------------------- steps
class FMNumpyStep:
    """The step over host rows: the literal per-row loop, rows in order."""

    def __init__(self, X, y, factorSize: int, loss: str = "squared", fitIntercept: bool = True,
                 fitLinear: bool = True, fraction: float = 1.0, rowOffset: int = 0):
        self.X = np.ascontiguousarray(X, dtype=np.float64)
        self.y = np.ascontiguousarray(y, dtype=np.float64)
        _require(self.X.ndim == 2 and self.y.shape == (self.X.shape[0],),
                 "rows (n x d) and one label per row")
        _require(loss in LOSSES, f"unknown loss {loss}")
        self.d, self.k, self.loss = int(self.X.shape[1]), int(factorSize), loss
        self.fitIntercept, self.fitLinear = bool(fitIntercept), bool(fitLinear)
        self.fraction, self.rowOffset = float(fraction), int(rowOffset)
        if loss == "logistic":
            bad = np.nonzero((self.y != 0.0) & (self.y != 1.0))[0]
            _require(bad.size == 0, "Classification labels should be 0 or 1 but row "
                     f"{self.rowOffset + int(bad[0]) if bad.size else 0} has another label")

    # the array operations fit_step needs beside + - * /
    def from_host(self, a):
        return np.array(a, dtype=np.float64)

    def to_host(self, a):
        return np.array(a, dtype=np.float64)

    sqrt = staticmethod(np.sqrt)

    @staticmethod
    def norm(a) -> float:
        return math.sqrt(float(np.cumsum(a * a)[-1])) if a.size else 0.0

    def row(self, x, yv, b, w, V):
        """(raw, loss, m, s) of one row."""
        nz = np.nonzero(x)[0]
        raw = b
        if self.fitLinear:
            for i in nz:
                raw += w[i] * x[i]
        s, q = np.zeros(self.k), np.zeros(self.k)
        for i in nz:
            t = V[i] * x[i]
            s += t
            q += t * t
        for f in range(self.k):
            raw += 0.5 * (s[f] * s[f] - q[f])
        if self.loss == "squared":
            return raw, (raw - yv) * (raw - yv), 2.0 * (raw - yv), s
        p = 1.0 / (1.0 + math.exp(-raw))
        return raw, (log1p_exp(-raw) if yv > 0 else log1p_exp(raw)), p - yv, s

    def evaluate(self, coef, i: int):
        d, k = self.d, self.k
        b, w, V = split_coef(coef, d, k, self.fitIntercept, self.fitLinear)
        gV, gw, gb, L, cnt = np.zeros((d, k)), np.zeros(d), 0.0, 0.0, 0.0
        take = batch_rows(i, self.fraction, self.X.shape[0], self.rowOffset)
        for r in np.nonzero(take)[0]:
            x = self.X[r]
            _, loss, m, s = self.row(x, self.y[r], b, w, V)
            for j in np.nonzero(x)[0]:
                gV[j] += m * (x[j] * s - (V[j] * x[j]) * x[j])
                gw[j] += m * x[j]
            gb += m
            L += loss
            cnt += 1.0
        G = np.concatenate([gV.ravel()] + ([gw] if self.fitLinear else [])
                           + ([np.array([gb])] if self.fitIntercept else []))
        return G, float(L), float(cnt)


class FMDeviceStep:
    """The step over device rows (this rank's shard): the kernels, then one
    allreduce of [G | L | cnt]; rowOffset from an allgather of the shard sizes,
    so a batch does not depend on the number of ranks."""

    def __init__(self, X, y, factorSize: int, loss: str = "squared", fitIntercept: bool = True,
                 fitLinear: bool = True, fraction: float = 1.0, workspaceBytes: int = 0):
        import torch
        from . import parallel
        X = as_rows(X)                  # a CSR shard is prepared here, once
        sparse = isinstance(X, FMSparseRows)
        _require(sparse or (torch.is_tensor(X) and X.dim() == 2),
                 "rows must be a device tensor (n x d), CSRRows or FMSparseRows")
        n, d = (X.n, X.d) if sparse else (int(v) for v in X.shape)
        self.X, self.y, self.fraction = X, y, float(fraction)
        self.plan = FMPlan(d, factorSize, fitIntercept, fitLinear, loss, workspaceBytes)
        self.d, self.k = self.plan.d, self.plan.k
        sizes = parallel.allgather_object(n)
        self.rowOffset = int(sum(sizes[:parallel.world()[0]])) if len(sizes) > 1 else 0
        self.out = torch.empty(self.plan.coefLen + 2, dtype=torch.float64, device=X.device)

    def from_host(self, a):
        import torch
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(self.X.device)

    def to_host(self, a):
        return a.cpu().numpy()

    @staticmethod
    def sqrt(a):
        return a.sqrt()

    @staticmethod
    def norm(a) -> float:
        import torch
        return float(torch.linalg.vector_norm(a))

    def evaluate(self, coef, i: int):
        from . import parallel
        err = None
        try:
            self.plan.evaluate(self.X, self.y, coef, self.out, i, self.fraction, self.rowOffset)
        except N.IllegalArgumentException as e:
            err = e
        parallel.agree(lambda: _reraise(err))
        parallel.allreduce_(self.out)
        L, cnt = self.out[-2:].cpu().tolist()
        return self.out[:-2], float(L), float(cnt)


def _reraise(err):
    if err is not None:
        raise err


# ------------------------------------------------------------------------- fit
def _updater(solver: str, step, regParam: float):
    """updater(w, g, stepSize, iter) -> (w, regVal) with its own state."""
    reg = float(regParam)
    state = {"m": None, "v": None, "b1T": 1.0, "b2T": 1.0}

    def reg_val(w):
        nrm = step.norm(w)
        return 0.5 * reg * nrm * nrm

    def gd(w, g, stepSize, it):
        eta = float(stepSize) / math.sqrt(it)
        w = w * (1.0 - eta * reg)
        w = w + (-eta) * g
        return w, reg_val(w)

    def adamw(w, g, stepSize, it):
        if stepSize > 0:
            if state["m"] is None:
                state["m"], state["v"] = w * 0.0, w * 0.0
            state["m"] = state["m"] * BETA1 + (1.0 - BETA1) * g
            state["v"] = state["v"] * BETA2 + (1.0 - BETA2) * (g * g)
            state["b1T"] *= BETA1
            state["b2T"] *= BETA2
            mHat = state["m"] / (1.0 - state["b1T"])
            vHat = state["v"] / (1.0 - state["b2T"])
            w = w - ((float(stepSize) * mHat) / (step.sqrt(vHat) + EPSILON) + reg * w)
        return w, reg_val(w)

    return gd if solver == "gd" else adamw


def fit_step(step, d: int, factorSize: int = 8, fitIntercept: bool = True, fitLinear: bool = True,
             regParam: float = 0.0, initStd: float = 0.01, maxIter: int = 100,
             stepSize: float = 1.0, tol: float = 1e-6, solver: str = "adamW", seed: int = 0,
             miniBatchFraction: float = 1.0, initialCoef=None):
    """GradientDescent.runMiniBatchSGD over `step`: (coefficients on the host,
    the objective history)."""
    check_fm_params(factorSize, regParam, miniBatchFraction, initStd, maxIter, stepSize, tol,
                    solver)
    k = int(factorSize)
    host = init_coef(d, k, fitIntercept, fitLinear, initStd, seed) if initialCoef is None \
        else np.array(initialCoef, dtype=np.float64)
    _require(host.size == coef_len(d, k, fitIntercept, fitLinear), "initialCoef has another size")
    w = step.from_host(host)
    update = _updater(solver, step, regParam)
    _, regVal = update(w, w * 0.0, 0.0, 1)
    history, prev, converged, i = [], None, False, 1
    while not converged and i <= int(maxIter):
        G, L, cnt = step.evaluate(w, i)
        if cnt > 0:
            history.append(L / cnt + regVal)
            had = prev is not None
            prev = w
            w, regVal = update(w, G / cnt, float(stepSize), i)
            if had:
                converged = step.norm(prev - w) < float(tol) * max(step.norm(w), 1.0)
        i += 1
    return step.to_host(w), history


# ---------------------------------------------------------------------- models
class FMTrainingSummary:
    def __init__(self, objectiveHistory):
        self.objectiveHistory = [float(v) for v in objectiveHistory]
        self.totalIterations = len(self.objectiveHistory)


class _FMModel:
    """intercept, linear (d) and factors (d x k) on the host; nothing touches a
    device before the first predict."""
    LOSS = "squared"

    def __init__(self, intercept, linear, factors):
        self.factors = np.array(factors, dtype=np.float64)
        _require(self.factors.ndim == 2, "factors must be a d x k matrix")
        self.linear = np.array(linear, dtype=np.float64).ravel()
        _require(self.linear.size == self.factors.shape[0], "one linear coefficient per feature")
        self.intercept = float(intercept)
        self.numFeatures, self.factorSize = (int(v) for v in self.factors.shape)
        self.summary = None
        self._plan = self._coef = None

    def _forward(self, X, **want):
        import torch
        if self._plan is None:
            self._plan = FMPlan(self.numFeatures, self.factorSize, True, True, self.LOSS)
        X = as_rows(X)
        self._plan._rows(X)
        if self._coef is None or self._coef.device != X.device:
            flat = np.concatenate([self.factors.ravel(), self.linear, [self.intercept]])
            self._coef = torch.from_numpy(flat).to(X.device)
        return self._plan.predict(X, self._coef, **want)


class FMRegressionModel(_FMModel):
    def predict(self, X):
        return self._forward(X, pred=True)[3]


class FMClassificationModel(_FMModel):
    LOSS = "logistic"
    numClasses = 2

    def predictRaw(self, X):
        return self._forward(X, raw=True)[1]

    def predictProbability(self, X):
        return self._forward(X, prob=True)[2]

    def predict(self, X):
        return self._forward(X, pred=True)[3]


# ------------------------------------------------------------------ estimators
class _FMEstimator:
    LOSS, MODEL, SEED = "squared", FMRegressionModel, REGRESSOR_SEED

    def __init__(self, factorSize: int = 8, fitIntercept: bool = True, fitLinear: bool = True,
                 regParam: float = 0.0, miniBatchFraction: float = 1.0, initStd: float = 0.01,
                 maxIter: int = 100, stepSize: float = 1.0, tol: float = 1e-6,
                 solver: str = "adamW", seed=None, workspaceBytes: int = 0):
        check_fm_params(factorSize, regParam, miniBatchFraction, initStd, maxIter, stepSize, tol,
                        solver)
        self.factorSize, self.fitIntercept, self.fitLinear = int(factorSize), bool(fitIntercept), \
            bool(fitLinear)
        self.regParam, self.miniBatchFraction = float(regParam), float(miniBatchFraction)
        self.initStd, self.maxIter, self.stepSize = float(initStd), int(maxIter), float(stepSize)
        self.tol, self.solver = float(tol), solver
        self.seed = self.SEED if seed is None else int(seed)
        self.workspaceBytes = int(workspaceBytes)

    def fit(self, X, y):
        """Every rank calls fit with its shard."""
        step = FMDeviceStep(X, y, self.factorSize, self.LOSS, self.fitIntercept, self.fitLinear,
                            self.miniBatchFraction, self.workspaceBytes)
        coef, history = fit_step(step, step.d, self.factorSize, self.fitIntercept, self.fitLinear,
                                 self.regParam, self.initStd, self.maxIter, self.stepSize,
                                 self.tol, self.solver, self.seed, self.miniBatchFraction)
        b, w, V = split_coef(coef, step.d, self.factorSize, self.fitIntercept, self.fitLinear)
        model = self.MODEL(b, w, V)
        model.summary = FMTrainingSummary(history)
        return model


class FMRegressor(_FMEstimator):
    pass


class FMClassifier(_FMEstimator):
    LOSS, MODEL, SEED = "logistic", FMClassificationModel, CLASSIFIER_SEED
