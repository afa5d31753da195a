"""LDA by online variational Bayes (mllib/clustering/LDAOptimizer.scala's
OnlineLDAOptimizer and LDAModel.scala's LocalLDAModel, Spark 3.3) over device
CSR documents of term counts (linalg.CSRRows; csrc/lda.hip, cyc_lda_* in
include/cyclone.h, 1 <= k <= cyc_lda_max_topics).

psi is digamma, E(v)_t = psi(v_t) - psi(sum v), B = exp(E(lambda))^T with E taken
per topic row of lambda (k x V).  Per document with a non-zero count, ids / cts
its words and counts, from gamma = gamma0_d:

    e = exp(E(gamma));  phi = B[ids] e + 1e-100
    repeat:  last = gamma;  gamma = e o (B[ids]^T (cts / phi)) + alpha
             e = exp(E(gamma));  phi = B[ids] e + 1e-100;  it += 1
    until not (sum|gamma - last| / k > 1e-3) or it == maxInner

Spark's loop has no cap; here maxInner (default 100, at least 1) bounds it, so
that no input can keep a wave spinning.  A stored zero contributes nothing; a
document without a non-zero count, or of weight 0, is not run: gamma row of
zeros, it = 0, not counted.  One E step returns [stat | logphat | nonEmpty]:
stat[t, v] = B[v, t] sum_d w_d e_dt cts_dv / phi_dv (d ascending), logphat_t =
sum_d w_d E(gamma_d)_t, nonEmpty = sum_d w_d.

fit_online, iteration i = 1 .. maxIter, rho = (tau0 + i)^-kappa: draw the batch,
E step, lambda <- (1 - rho) lambda + rho (stat corpusSize / ceil(fraction
corpusSize) + eta); with optimizeDocConcentration the Newton step of
updateAlpha on the host: N = nonEmpty, g = N (logphat / N - E(alpha)), c = N
psi'(sum alpha), q = -N psi'(alpha), b = sum(g / q) / (1 / c + sum(1 / q)), d =
-(g - b) / q, alpha += rho d only if every component stays positive.  A batch
without a non-empty document changes nothing.  The step objects (LDADeviceStep
here, a host restatement in the tests) are interchangeable: estep(lambda, alpha,
gamma0, weights) -> the host buffer [stat | logphat | nonEmpty], merged over
ranks by one parallel.allreduce_.

Bound (LocalLDAModel.logLikelihoodBound): the corpus part on the device from
each document's final gamma (cyc_lda_bound_dev), the topics part sum((eta -
lambda) o E(lambda)) + sum(lgamma(lambda) - lgamma(eta)) + sum_t(lgamma(eta V) -
lgamma(sum_v lambda_tv)) on the host.

This package's own draws: lambda0 is numpy.random.default_rng(seed).gamma(100,
1 / 100, (k, V)); rank r's batches come from default_rng([seed, r]): first the
weights, Poisson(fraction) with replacement (the default) or Bernoulli without,
then gamma0 = gamma(100, 1 / 100, (n, k)).  A document drawn m times runs once at
weight m (in Spark the copies get different starts).  Spark's breeze draws are
not restated, so a fit does not reproduce a Spark run's numbers.  Out of scope:
the EM optimizer, DistributedLDAModel, save / load.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np

from . import _native as N
from .tree import _require

GAMMA_SHAPE = 100.0


def _dev(a, device, dtype=np.float64):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(device)


class LDADocs:
    """cyc_lda_docs: a CSRRows shard of term counts prepared once (the index and
    count checks, the column copy with its segment table, the length order).
    It keeps the shard's arrays alive; a slice whose rowptr[0] > 0 is rebased."""

    def __init__(self, csr):
        import torch
        from .linalg import CSRRows
        _require(isinstance(csr, CSRRows), "LDADocs takes CSRRows")
        rowptr, colidx, values = csr.rowptr, csr.colidx, csr.values
        _require(rowptr.is_cuda and rowptr.dtype == torch.int64 and colidx.dtype == torch.int32
                 and values.dtype == torch.float64 and colidx.numel() == values.numel(),
                 "CSR rows are int64 rowptr, int32 colidx and fp64 values on the device")
        self.n, self.vocabSize, self.device = csr.n, csr.numCols, csr.device
        base = int(rowptr[0]) if self.n > 0 else 0
        if base:
            rowptr = rowptr - base
        self._arrays = (rowptr.contiguous(), colidx.contiguous(), values.contiguous())
        self.tokens = float(values.sum())
        self._lib = N.load()
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            N.check(self._lib.cyc_lda_docs_create(*(N.ptr(t) for t in self._arrays), self.n,
                                                  self.vocabSize, N.stream_handle(),
                                                  ctypes.byref(h)))
        self.handle = h

    def close(self):
        if getattr(self, "handle", None):
            self._lib.cyc_lda_docs_destroy(self.handle)
            self.handle = None

    __del__ = close


def as_docs(X):
    return X if isinstance(X, LDADocs) else LDADocs(X)


class LDAPlan:
    """cyc_lda_plan: k, the vocabulary, the prepared topics and the scratch."""

    def __init__(self, k: int, vocabSize: int):
        self.k, self.vocabSize = int(k), int(vocabSize)
        self._lib = N.load()
        h = ctypes.c_void_p()
        N.check(self._lib.cyc_lda_plan_create(self.k, self.vocabSize, ctypes.byref(h)))
        self.handle = h
        self.topicStride = int(self._lib.cyc_lda_topic_stride(self.k))
        self.slabWords = int(self._lib.cyc_lda_slab_bytes()) // (8 * self.topicStride)

    def close(self):
        if getattr(self, "handle", None):
            self._lib.cyc_lda_plan_destroy(self.handle)
            self.handle = None

    __del__ = close

    @staticmethod
    def _tensor(t, size, what, dtype=None):
        import torch
        _require(torch.is_tensor(t) and t.is_cuda and t.dtype == (dtype or torch.float64)
                 and t.is_contiguous() and t.numel() == size,
                 f"{what} must be a contiguous device tensor of {size} values")

    def set_topics(self, lam):
        """lambda (k x vocabSize, device)."""
        import torch
        self._tensor(lam, self.k * self.vocabSize, "lambda")
        with torch.cuda.device(lam.device):
            N.check(self._lib.cyc_lda_set_topics_dev(self.handle, N.ptr(lam), N.stream_handle()))
        return self

    def _inputs(self, docs, alpha, gamma0, weights):
        _require(isinstance(docs, LDADocs), "documents must be LDADocs")
        self._tensor(alpha, self.k, "alpha")
        self._tensor(gamma0, docs.n * self.k, "gamma0")
        if weights is not None:
            self._tensor(weights, docs.n, "weights")

    def infer(self, docs, alpha, gamma0, weights=None, maxInner: int = 100):
        """(gamma (n x k), the sweeps taken (n, int32))."""
        import torch
        self._inputs(docs, alpha, gamma0, weights)
        gamma = torch.empty((docs.n, self.k), dtype=torch.float64, device=docs.device)
        iters = torch.empty(docs.n, dtype=torch.int32, device=docs.device)
        with torch.cuda.device(docs.device):
            N.check(self._lib.cyc_lda_infer_dev(self.handle, docs.handle, N.ptr(alpha),
                                                N.ptr(gamma0), N.ptr(weights), int(maxInner),
                                                N.ptr(gamma), N.ptr(iters), N.stream_handle()))
        return gamma, iters

    def estep(self, docs, alpha, gamma0, weights=None, maxInner: int = 100, out=None,
              gamma=None, iters=None):
        """out (device, k vocabSize + k + 1) = [stat | logphat | nonEmpty]."""
        import torch
        self._inputs(docs, alpha, gamma0, weights)
        size = self.k * self.vocabSize + self.k + 1
        if out is None:
            out = torch.empty(size, dtype=torch.float64, device=docs.device)
        self._tensor(out, size, "out")
        if gamma is not None:
            self._tensor(gamma, docs.n * self.k, "gamma")
        if iters is not None:
            self._tensor(iters, docs.n, "iters", torch.int32)
        with torch.cuda.device(docs.device):
            N.check(self._lib.cyc_lda_estep_dev(self.handle, docs.handle, N.ptr(alpha),
                                                N.ptr(gamma0), N.ptr(weights), int(maxInner),
                                                N.ptr(gamma), N.ptr(iters), N.ptr(out),
                                                N.stream_handle()))
        return out

    def bound(self, docs, alpha, gamma, weights=None):
        """The corpus part of the bound (device, 1 value) from infer's gamma."""
        import torch
        self._inputs(docs, alpha, gamma, weights)
        out = torch.empty(1, dtype=torch.float64, device=docs.device)
        with torch.cuda.device(docs.device):
            N.check(self._lib.cyc_lda_bound_dev(self.handle, docs.handle, N.ptr(alpha),
                                                N.ptr(gamma), N.ptr(weights), N.ptr(out),
                                                N.stream_handle()))
        return out


def digamma(x):
    """The kernels' psi over a device fp64 tensor."""
    import torch
    x = x.contiguous()
    out = torch.empty_like(x)
    with torch.cuda.device(x.device):
        N.check(N.load().cyc_lda_digamma_dev(N.ptr(x), x.numel(), N.ptr(out), N.stream_handle()))
    return out


class LDADeviceStep:
    """The E step over this rank's shard: the kernels, then one allreduce."""

    def __init__(self, X, k: int, maxInner: int = 100):
        self.docs = as_docs(X)
        self.n = self.docs.n
        self.maxInner = int(maxInner)
        self.plan = LDAPlan(k, self.docs.vocabSize)

    def estep(self, lam, alpha, gamma0, weights):
        from . import parallel
        dev = self.docs.device
        self.plan.set_topics(_dev(lam, dev))
        out = self.plan.estep(self.docs, _dev(alpha, dev), _dev(gamma0, dev),
                              None if weights is None else _dev(weights, dev), self.maxInner)
        parallel.allreduce_(out)
        return out.cpu().numpy()


def dirichlet_expectation(v):
    from scipy.special import psi
    return psi(v) - psi(np.sum(v))


def update_alpha(alpha, logphat, nonEmpty: float, rho: float):
    """OnlineLDAOptimizer.updateAlpha; logphat is the batch's sum."""
    from scipy.special import polygamma
    n = float(nonEmpty)
    g = n * (logphat / n - dirichlet_expectation(alpha))
    c = n * polygamma(1, np.sum(alpha))
    q = -n * polygamma(1, alpha)
    b = np.sum(g / q) / (1.0 / c + np.sum(1.0 / q))
    d = -(g - b) / q
    return alpha + rho * d if np.all(rho * d + alpha > 0) else alpha


def fit_online(step, vocabSize: int, k: int = 10, maxIter: int = 20, seed: int = 0,
               docConcentration=None, topicConcentration=None, learningOffset: float = 1024.0,
               learningDecay: float = 0.51, subsamplingRate: float = 0.05,
               optimizeDocConcentration: bool = True, sampleWithReplacement: bool = True):
    """OnlineLDAOptimizer's loop over `step`: (lambda (k x V), alpha (k)) on the host."""
    from . import parallel
    k, V, n = int(k), int(vocabSize), int(step.n)
    _require(k >= 1, f"k must be at least 1 but got {k}")
    _require(0.0 < float(subsamplingRate) <= 1.0,
             f"subsamplingRate must be in (0, 1] but got {subsamplingRate}")
    _require(float(learningOffset) > 0 and float(learningDecay) > 0,
             "learningOffset and learningDecay must be positive")
    alpha = np.full(k, 1.0 / k) if docConcentration is None else \
        np.broadcast_to(np.asarray(docConcentration, dtype=np.float64), (k,)).copy()
    eta = 1.0 / k if topicConcentration is None else float(topicConcentration)
    _require(np.all(alpha > 0) and eta > 0, "the concentrations must be positive")
    rank = parallel.world()[0]
    corpusSize = int(sum(parallel.allgather_object(n)))
    batchSize = math.ceil(float(subsamplingRate) * corpusSize)
    lam = np.random.default_rng(seed).gamma(GAMMA_SHAPE, 1.0 / GAMMA_SHAPE, (k, V))
    rng = np.random.default_rng([seed, rank])
    for i in range(1, int(maxIter) + 1):
        weights = rng.poisson(subsamplingRate, n).astype(np.float64) if sampleWithReplacement \
            else (rng.random(n) < subsamplingRate).astype(np.float64)
        gamma0 = rng.gamma(GAMMA_SHAPE, 1.0 / GAMMA_SHAPE, (n, k))
        out = step.estep(lam, alpha, gamma0, weights)
        stat, logphat, nonEmpty = out[:k * V].reshape(k, V), out[k * V:k * V + k], float(out[-1])
        if nonEmpty == 0:
            continue
        rho = (float(learningOffset) + i) ** -float(learningDecay)
        lam = (1.0 - rho) * lam + rho * (stat * (corpusSize / batchSize) + eta)
        if optimizeDocConcentration:
            alpha = update_alpha(alpha, logphat, nonEmpty, rho)
    return lam, alpha


class LocalLDAModel:
    def __init__(self, topics, docConcentration, topicConcentration: float, seed: int = 0,
                 maxInner: int = 100):
        self.topics = np.ascontiguousarray(topics, dtype=np.float64)        # V x k = lambda^T
        self.vocabSize, self.k = self.topics.shape
        self.docConcentration = np.asarray(docConcentration, dtype=np.float64)
        self.topicConcentration = float(topicConcentration)
        self.seed, self.maxInner = int(seed), int(maxInner)
        self._plans = {}

    def topicsMatrix(self):
        return self.topics

    @property
    def estimatedDocConcentration(self):
        return self.docConcentration

    def describeTopics(self, maxTermsPerTopic: int = 10):
        """Per topic (term indices, term weights), weights descending."""
        out = []
        for t in range(self.k):
            topic = self.topics[:, t] / np.sum(np.abs(self.topics[:, t]))
            terms = np.argsort(-topic, kind="stable")[:int(maxTermsPerTopic)]
            out.append((terms, topic[terms]))
        return out

    def _infer(self, X):
        docs = as_docs(X)
        _require(docs.vocabSize == self.vocabSize,
                 f"the documents have a vocabulary of {docs.vocabSize} but the model has "
                 f"{self.vocabSize}")
        plan = self._plans.get(docs.device)
        if plan is None:
            plan = LDAPlan(self.k, self.vocabSize).set_topics(
                _dev(self.topics.T, docs.device))
            self._plans[docs.device] = plan
        gamma0 = np.random.default_rng(self.seed).gamma(GAMMA_SHAPE, 1.0 / GAMMA_SHAPE,
                                                        (docs.n, self.k))
        alpha = _dev(self.docConcentration, docs.device)
        gamma, _ = plan.infer(docs, alpha, _dev(gamma0, docs.device), None, self.maxInner)
        return plan, docs, alpha, gamma

    def transform(self, X):
        """topicDistribution per document (device, n x k): gamma normalised,
        zeros for an empty document."""
        gamma = self._infer(X)[3]
        total = gamma.sum(1, keepdim=True)
        return gamma / total.masked_fill(total == 0, 1.0)

    topicDistribution = transform

    def logLikelihood(self, X) -> float:
        from scipy.special import gammaln
        plan, docs, alpha, gamma = self._infer(X)
        lam, eta = self.topics.T, self.topicConcentration
        Elam = np.stack([dirichlet_expectation(row) for row in lam])
        topicsPart = (np.sum((eta - lam) * Elam) + np.sum(gammaln(lam) - gammaln(eta))
                      + np.sum(gammaln(eta * self.vocabSize) - gammaln(lam.sum(1))))
        return float(plan.bound(docs, alpha, gamma)) + float(topicsPart)

    def logPerplexity(self, X) -> float:
        docs = as_docs(X)
        return -self.logLikelihood(docs) / docs.tokens


class LDA:
    def __init__(self, k: int = 10, maxIter: int = 20, seed: int = 0, docConcentration=None,
                 topicConcentration=None, learningOffset: float = 1024.0,
                 learningDecay: float = 0.51, subsamplingRate: float = 0.05,
                 optimizeDocConcentration: bool = True, optimizer: str = "online"):
        if optimizer != "online":
            raise N.IllegalArgumentException(
                f"optimizer given invalid value {optimizer}. Supported options: online "
                "(the em optimizer is not built).")
        kmax = int(N.load().cyc_lda_max_topics())
        _require(1 <= int(k) <= kmax, f"k must be in [1, {kmax}] but got {k}")
        _require(int(maxIter) >= 0, f"maxIter must not be negative but got {maxIter}")
        self.k, self.maxIter, self.seed = int(k), int(maxIter), int(seed)
        self.params = dict(docConcentration=docConcentration,
                           topicConcentration=topicConcentration, learningOffset=learningOffset,
                           learningDecay=learningDecay, subsamplingRate=subsamplingRate,
                           optimizeDocConcentration=optimizeDocConcentration)

    def fit(self, X) -> LocalLDAModel:
        """X: this rank's CSRRows (or LDADocs) of term counts."""
        step = LDADeviceStep(X, self.k)
        lam, alpha = fit_online(step, step.docs.vocabSize, self.k, self.maxIter, self.seed,
                                **self.params)
        eta = self.params["topicConcentration"]
        return LocalLDAModel(lam.T, alpha, 1.0 / self.k if eta is None else eta, self.seed)
