"""GaussianMixture (ml/clustering/GaussianMixture.scala) over dense fp64 device
rows, and MultivariateGaussian (ml/stat/distribution/MultivariateGaussian
.scala).  The kernels are csrc/gmm.hip (cyc_gmm_* in include/cyclone.h).

Gaussian constants (host, one eigh per component): (lam, U) = eigh(cov), tol =
EPSILON max(lam) d; rootSigmaInv A = diag(pinv) U^T with pinv_i = sqrt(1 /
lam_i) where lam_i > tol and 0 elsewhere; u = -0.5 (d log 2 pi + sum of log
lam_i over lam_i > tol); logpdf(x) = u - 0.5 |A (x - mean)|^2.

EM step.  Row i of weight om_i: p_ij = EPSILON + w_j pdf_j(x_i), s_i = sum_j
p_ij, r_ij = om_i p_ij / s_i, ll += om_i log s_i.  The device adds into one
sums buffer [ll | W (k) | M (k x d) | S (k x d(d+1)/2)]: W_j = sum_i r_ij, M_j =
sum_i r_ij x_i, S_j the packed upper triangle (column-major, S_j[b(b+1)/2 + a],
a <= b) of sum_i r_ij x_i x_i^T.  Buffers of shards and ranks merge by addition
(parallel.allreduce_, the treeAggregate merge).  The M step runs on the host:
mu_j = M_j / W_j, S_j <- (S_j - W_j mu_j mu_j^T) / W_j (spr(-W_j, mu_j, S_j),
then scal(1 / W_j, S_j)), w_j = W_j / sum_j W_j.

The initial model without initialModel has the shape of the reference's
initRandom (5 sampled rows per component: their mean, their per-feature
variance as a diagonal covariance, weights 1 / k), but the 5 k rows are drawn
with replacement by numpy.random.default_rng(seed) over the global row range.
Spark's Poisson takeSample(withReplacement = true) is NOT restated (kmeans_init
.take_sample_indices covers only the sampler without replacement), so a fit
without initialModel does not reproduce a Spark run's draws.

CSR rows and save / load are not provided.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np

from . import _native as N
from . import parallel

EPSILON = 2.0 ** -52          # ml.impl.Utils.EPSILON
MAX_NUM_FEATURES = 1024
NUM_SAMPLES = 5               # rows per component of the random initial model
DOUBLE_MAX = 1.7976931348623157e308


def check_shape(k, numFeatures=None):
    if int(k) < 1:
        raise N.IllegalArgumentException(f"requirement failed: k must be positive but got {k}")
    if numFeatures is not None:
        if int(numFeatures) < 1:
            raise N.IllegalArgumentException(
                f"requirement failed: numFeatures must be positive but got {numFeatures}")
        if int(numFeatures) > MAX_NUM_FEATURES:
            raise N.IllegalArgumentException(
                f"requirement failed: GaussianMixture supports up to {MAX_NUM_FEATURES} "
                f"features but got {numFeatures}")


def sums_length(k: int, d: int) -> int:
    return 1 + k + k * d + k * (d * (d + 1) // 2)


def split_sums(sums, k: int, d: int):
    """(ll, W (k), M (k x d), S (k x d(d+1)/2)) views of a host sums buffer."""
    sums = np.asarray(sums, dtype=np.float64)
    if sums.shape != (sums_length(k, d),):
        raise N.IllegalArgumentException(
            f"requirement failed: a sums buffer for k = {k}, numFeatures = {d} has "
            f"{sums_length(k, d)} values but got {sums.size}")
    tri = d * (d + 1) // 2
    o = 1 + k
    return (float(sums[0]), sums[1:o], sums[o:o + k * d].reshape(k, d),
            sums[o + k * d:].reshape(k, tri))


def unpack_upper(tri: np.ndarray, d: int) -> np.ndarray:
    """The full symmetric d x d matrix of a packed upper triangle."""
    full = np.empty((d, d), dtype=np.float64)
    a, b = np.triu_indices(d)          # a <= b, row-major over (a, b)
    full[a, b] = tri[b * (b + 1) // 2 + a]
    full[b, a] = full[a, b]
    return full


def m_step(sums, k: int, d: int):
    """(weights (k), means (k x d), covs (k x d x d)) from a merged buffer."""
    _, W, M, S = split_sums(sums, k, d)
    a, b = np.triu_indices(d)
    pos = b * (b + 1) // 2 + a
    means = np.empty((k, d), dtype=np.float64)
    covs = np.empty((k, d, d), dtype=np.float64)
    for j in range(k):
        mu = M[j] / W[j]
        tri = S[j].copy()
        tri[pos] += mu[a] * (-W[j] * mu[b])      # spr(-W_j, mu_j, S_j): x_a (alpha x_b)
        tri *= 1.0 / W[j]                        # scal(1 / W_j, S_j)
        means[j] = mu
        covs[j] = unpack_upper(tri, d)
    return W / W.sum(), means, covs


class MultivariateGaussian:
    """ml.stat.distribution.MultivariateGaussian: mean (d), cov (d x d,
    symmetric; singular covariances are served by the pseudo-inverse)."""

    def __init__(self, mean, cov):
        self.mean = np.array(mean, dtype=np.float64).ravel()
        d = self.mean.size
        self.cov = np.array(cov, dtype=np.float64).reshape(d, d)
        lam, U = np.linalg.eigh(self.cov)
        tol = EPSILON * lam.max() * d
        keep = lam > tol
        if not keep.any():
            raise N.IllegalArgumentException("Covariance matrix has no non-zero singular values")
        self.logPseudoDet = float(np.log(lam[keep]).sum())
        pinv = np.zeros(d, dtype=np.float64)
        pinv[keep] = np.sqrt(1.0 / lam[keep])
        self.rootSigmaInv = np.ascontiguousarray(pinv[:, None] * U.T)
        self.u = -0.5 * (d * math.log(2.0 * math.pi) + self.logPseudoDet)

    def logpdf(self, x) -> float:
        x = np.asarray(x, dtype=np.float64).ravel()
        if x.size != self.mean.size:
            raise N.IllegalArgumentException(
                f"requirement failed: the vector has {x.size} features but the Gaussian has "
                f"{self.mean.size}")
        v = self.rootSigmaInv @ (x - self.mean)
        return self.u - 0.5 * float(v @ v)

    def pdf(self, x) -> float:
        return math.exp(self.logpdf(x))


def model_constants(weights, gaussians) -> np.ndarray:
    """[weights (k) | means (k d) | rootSigmaInv (k d d, row-major) | u (k)],
    the host image of cyc_gmm_set_model_dev's arguments."""
    return np.concatenate([np.asarray(weights, dtype=np.float64).ravel()] +
                          [g.mean for g in gaussians] +
                          [g.rootSigmaInv.ravel() for g in gaussians] +
                          [np.array([g.u for g in gaussians], dtype=np.float64)])


class GMMPlan:
    """cyc_gmm_plan: k, the feature count and the device workspace of one
    mixture (chunkRows 0: the r workspace of chunkRows k doubles sized to 1
    GiB)."""

    def __init__(self, k: int, numFeatures: int, chunkRows: int = 0):
        check_shape(k, numFeatures)
        self.k = int(k)
        self.numFeatures = int(numFeatures)
        self.sumsLength = sums_length(self.k, self.numFeatures)
        self._lib = N.load()
        h = ctypes.c_void_p()
        N.check(self._lib.cyc_gmm_plan_create(self.k, self.numFeatures, int(chunkRows),
                                              ctypes.byref(h)))
        self.handle = h
        self._model = None

    def close(self):
        if getattr(self, "handle", None):
            self._lib.cyc_gmm_plan_destroy(self.handle)
            self.handle = None

    __del__ = close

    def _rows(self, X):
        import torch
        if isinstance(X, _csr_type()):
            raise N.IllegalArgumentException(
                "GaussianMixture takes dense rows; CSR rows are not supported")
        if not torch.is_tensor(X) or X.dtype != torch.float64 or X.dim() != 2 \
                or not X.is_contiguous():
            raise N.IllegalArgumentException(
                "requirement failed: rows must be a contiguous fp64 device tensor (n x "
                f"{self.numFeatures})")
        if int(X.shape[1]) != self.numFeatures:
            raise N.IllegalArgumentException(
                f"requirement failed: the rows have {int(X.shape[1])} features but the mixture "
                f"has {self.numFeatures}")
        return int(X.shape[0])

    def _sums(self, sums):
        import torch
        if not torch.is_tensor(sums) or sums.dtype != torch.float64 \
                or sums.numel() != self.sumsLength or not sums.is_contiguous():
            raise N.IllegalArgumentException(
                f"requirement failed: sums must be {self.sumsLength} contiguous fp64 values")

    def set_model(self, weights, gaussians, device):
        """Upload the constants of (weights, gaussians) (one host buffer up)."""
        import torch
        k, d = self.k, self.numFeatures
        if len(gaussians) != k or np.asarray(weights).size != k:
            raise N.IllegalArgumentException(
                f"requirement failed: the mixture has {k} components")
        for g in gaussians:
            if g.mean.size != d:
                raise N.IllegalArgumentException(
                    f"requirement failed: a Gaussian of {g.mean.size} features in a mixture of "
                    f"{d}")
        m = torch.from_numpy(model_constants(weights, gaussians)).to(device)
        self.set_model_dev(m)

    def set_model_dev(self, m):
        """m: the device image of model_constants (k + k d + k d^2 + k)."""
        k, d = self.k, self.numFeatures
        if m.numel() != 2 * k + k * d + k * d * d:
            raise N.IllegalArgumentException("requirement failed: model image of the wrong length")
        o1, o2, o3 = k, k + k * d, k + k * d + k * d * d
        N.check(self._lib.cyc_gmm_set_model_dev(
            self.handle, N.ptr(m[:o1]), N.ptr(m[o1:o2]), N.ptr(m[o2:o3]), N.ptr(m[o3:]),
            N.stream_handle()))
        self._model = m        # alive until the stream has consumed it

    def accumulate(self, X, weights, sums):
        """sums += the E step and aggregate of this shard (all device fp64)."""
        import torch
        n = self._rows(X)
        self._sums(sums)
        if weights is not None and (not torch.is_tensor(weights) or weights.dtype != torch.float64
                                    or weights.numel() != n or not weights.is_contiguous()):
            raise N.IllegalArgumentException(
                f"requirement failed: weights must be {n} contiguous fp64 values")
        N.check(self._lib.cyc_gmm_accumulate_dev(self.handle, N.ptr(X), n, N.ptr(weights),
                                                 N.ptr(sums), N.stream_handle()))

    def mstep(self, X, R, sums):
        """sums[1:] += the aggregate of X under the responsibilities R (n x k)."""
        import torch
        n = self._rows(X)
        self._sums(sums)
        if not torch.is_tensor(R) or R.dtype != torch.float64 or R.numel() != n * self.k \
                or not R.is_contiguous():
            raise N.IllegalArgumentException(
                f"requirement failed: R must be {n} x {self.k} contiguous fp64 values")
        N.check(self._lib.cyc_gmm_mstep_dev(self.handle, N.ptr(X), n, N.ptr(R), N.ptr(sums),
                                            N.stream_handle()))

    def predict(self, X, prob: bool = False, label: bool = False, logpdf: bool = False):
        """(prob (n x k), label (n int32), logpdf (n x k)) device tensors of
        the requested outputs (else None)."""
        import torch
        n = self._rows(X)
        p = torch.empty((n, self.k), dtype=torch.float64, device=X.device) if prob else None
        y = torch.empty(n, dtype=torch.int32, device=X.device) if label else None
        lp = torch.empty((n, self.k), dtype=torch.float64, device=X.device) if logpdf else None
        N.check(self._lib.cyc_gmm_predict_dev(self.handle, N.ptr(X), n, N.ptr(p), N.ptr(y),
                                              N.ptr(lp), N.stream_handle()))
        return p, y, lp

    def logpdf(self, X):
        """u_j - 0.5 q_ij of every row and component (n x k, device)."""
        return self.predict(X, logpdf=True)[2]


def _csr_type():
    from .linalg import CSRRows
    return CSRRows


def init_sample_indices(total: int, k: int, seed: int) -> np.ndarray:
    """The 5 k global row indices (with replacement) of the random initial
    model; component j takes draws 5 j .. 5 j + 4."""
    if total < 1:
        raise N.IllegalArgumentException("requirement failed: the training set is empty")
    return np.random.default_rng(int(seed)).integers(0, total, size=NUM_SAMPLES * int(k))


def init_from_samples(samples: np.ndarray, k: int):
    """(weights, means, covs) from the 5 k sampled rows (5 k x d, host)."""
    samples = np.asarray(samples, dtype=np.float64)
    d = samples.shape[1]
    means = np.empty((k, d), dtype=np.float64)
    covs = np.zeros((k, d, d), dtype=np.float64)
    for j in range(k):
        s = samples[NUM_SAMPLES * j:NUM_SAMPLES * (j + 1)]
        mu = s.sum(axis=0) / NUM_SAMPLES
        means[j] = mu
        covs[j][np.diag_indices(d)] = (s * s).sum(axis=0) / NUM_SAMPLES - mu * mu
    return np.full(k, 1.0 / k), means, covs


class GaussianMixtureSummary:
    def __init__(self, logLikelihood, numIter, clusterSizes, objectiveHistory):
        self.logLikelihood = float(logLikelihood)
        self.numIter = int(numIter)
        self.clusterSizes = np.asarray(clusterSizes, dtype=np.int64)
        self.objectiveHistory = np.asarray(objectiveHistory, dtype=np.float64)


class GaussianMixtureModel:
    """weights (k) and gaussians (MultivariateGaussian); predictions run the
    device E step over fp64 device rows and stay on the device."""

    def __init__(self, weights, gaussians, summary=None):
        self.weights = np.array(weights, dtype=np.float64).ravel()
        self.gaussians = list(gaussians)
        if len(self.gaussians) != self.weights.size or not self.gaussians:
            raise N.IllegalArgumentException(
                "requirement failed: one weight per Gaussian, at least one Gaussian")
        self.summary = summary
        self._plan = None
        self._device = None

    @property
    def k(self) -> int:
        return self.weights.size

    @property
    def numFeatures(self) -> int:
        return self.gaussians[0].mean.size

    def _ready(self, X):
        import torch
        if isinstance(X, _csr_type()):
            raise N.IllegalArgumentException(
                "GaussianMixture takes dense rows; CSR rows are not supported")
        if self._plan is None:
            self._plan = GMMPlan(self.k, self.numFeatures)
        if torch.is_tensor(X) and self._device != X.device:
            self._plan._rows(X)
            self._plan.set_model(self.weights, self.gaussians, X.device)
            self._device = X.device
        return self._plan

    def predictProbability(self, X):
        """p_ij / s_i at unit row weight (n x k row-major, device)."""
        return self._ready(X).predict(X, prob=True)[0]

    def predict(self, X):
        """argmax of the probabilities as int32 (the lowest index on ties),
        device."""
        return self._ready(X).predict(X, label=True)[1]


class GaussianMixture:
    """GaussianMixture.train: EM over the device E step + aggregate, the M
    step on the host.  Per iteration the host traffic is the sums buffer down
    and the new constants up.  initialModel = (weights (k), means (k x d),
    covs (k x d x d)); without it see the module docstring."""

    def __init__(self, k: int = 2, maxIter: int = 100, tol: float = 0.01, seed: int = 0,
                 initialModel=None, chunkRows: int = 0):
        check_shape(k)
        if int(maxIter) < 0:
            raise N.IllegalArgumentException(f"maxIter given invalid value {maxIter}")
        if not tol >= 0:
            raise N.IllegalArgumentException(f"tol given invalid value {tol}")
        self.k = int(k)
        self.maxIter = int(maxIter)
        self.tol = float(tol)
        self.seed = int(seed)
        self.chunkRows = int(chunkRows)
        self.initialModel = None
        if initialModel is not None:
            w, mu, cov = initialModel
            w = np.array(w, dtype=np.float64).ravel()
            mu = np.array(mu, dtype=np.float64).reshape(self.k, -1)
            cov = np.array(cov, dtype=np.float64).reshape(self.k, mu.shape[1], mu.shape[1])
            if w.size != self.k:
                raise N.IllegalArgumentException(
                    f"requirement failed: initialModel has {w.size} weights but k = {self.k}")
            self.initialModel = (w, mu, cov)

    def _initial(self, X):
        if self.initialModel is not None:
            return self.initialModel
        import torch
        n, d = int(X.shape[0]), int(X.shape[1])
        counts = parallel.allgather_object(n)
        rank, _ = parallel.world()
        lo = int(sum(counts[:rank]))
        idx = parallel.agree(lambda: init_sample_indices(int(sum(counts)), self.k, self.seed))
        samples = np.zeros((idx.size, d), dtype=np.float64)
        mine = np.nonzero((idx >= lo) & (idx < lo + n))[0]
        if mine.size:
            sel = torch.from_numpy(idx[mine] - lo).to(X.device)
            samples[mine] = X.index_select(0, sel).cpu().numpy()
        if len(counts) > 1:
            t = torch.from_numpy(samples).to(X.device)
            parallel.allreduce_(t.view(-1))     # every draw has one owner
            samples = t.cpu().numpy()
        return init_from_samples(samples, self.k)

    def fit(self, X, weights=None) -> GaussianMixtureModel:
        """X: this rank's dense fp64 device rows (n x d); weights: its row
        weights (device, optional).  With several ranks every rank calls fit."""
        import torch
        if isinstance(X, _csr_type()):
            raise N.IllegalArgumentException(
                "GaussianMixture takes dense rows; CSR rows are not supported")
        if not torch.is_tensor(X) or X.dim() != 2:
            raise N.IllegalArgumentException(
                "requirement failed: rows must be an fp64 device tensor (n x numFeatures)")
        d = int(X.shape[1])
        check_shape(self.k, d)
        if self.initialModel is not None and self.initialModel[1].shape[1] != d:
            raise N.IllegalArgumentException(
                f"requirement failed: the rows have {d} features but initialModel has "
                f"{self.initialModel[1].shape[1]}")
        X = X.to(torch.float64).contiguous()
        if weights is not None:
            weights = torch.as_tensor(weights, device=X.device).to(torch.float64).contiguous()
        k = self.k
        w, means, covs = self._initial(X)
        gaussians = [MultivariateGaussian(means[j], covs[j]) for j in range(k)]
        plan = GMMPlan(k, d, self.chunkRows)
        try:
            sums = torch.empty(plan.sumsLength, dtype=torch.float64, device=X.device)
            ll, llPrev, it, history = -DOUBLE_MAX, 0.0, 0, []
            while it < self.maxIter and abs(ll - llPrev) > self.tol:
                plan.set_model(w, gaussians, X.device)
                sums.zero_()
                parallel.agree(lambda: plan.accumulate(X, weights, sums))
                parallel.allreduce_(sums)          # the treeAggregate merge
                host = sums.cpu().numpy()
                w, means, covs = m_step(host, k, d)
                gaussians = [MultivariateGaussian(means[j], covs[j]) for j in range(k)]
                llPrev, ll = ll, float(host[0])
                history.append(ll)
                it += 1
            plan.set_model(w, gaussians, X.device)
            sizes = torch.bincount(plan.predict(X, label=True)[1].to(torch.int64),
                                   minlength=k).to(torch.float64)
            parallel.allreduce_(sizes)
            sizes = sizes.cpu().numpy()
        finally:
            plan.close()
        summary = GaussianMixtureSummary(ll, it, sizes, history)
        return GaussianMixtureModel(w, gaussians, summary)
