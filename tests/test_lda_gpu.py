"""LDA's E step, bound, model and online fit on the device (csrc/lda.hip) against
the numpy.longdouble restatement: every lane layout of the topics, document
lengths at the wave's chunk and at the LDS tier's boundary, word lengths at the
segment, document counts at the run, weights 0 / 1 / 2, stored zeros, both sweep
caps.  Every device call runs twice and must give the same bytes; sweep counts
are compared exactly on inputs whose reference stays clear of the threshold.

Measured on an MI355X, maximum over all cases here: gamma relative deviation
5.223e-13 (k = 8 over the eight lengths); asserted at 100 x that, rounded up to a
power of ten, 1e-10 (never looser than 1e-8); stat, logphat and the bound at the
same factor of their sums of absolute terms."""
import functools

import mpmath
import numpy as np
import pytest
import torch

import lda_restatement as R
from cycloneml_amd import _native as N
from cycloneml_amd import lda as L
from cycloneml_amd.linalg import CSRRows

pytestmark = pytest.mark.gpu
BOUND = 1e-10
FIT_BOUND = 1e-12
LENS = (0, 1, 63, 0, 64, 65, 129, 0)      # an empty document first, inside and last
EPS = 2.0 ** -52


def dev(a, cuda, dtype=np.float64):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(cuda)


def rows(csr, V, cuda):
    return CSRRows(dev(csr[0], cuda, np.int64), dev(csr[1], cuda, np.int32), dev(csr[2], cuda), V)


def corpus(n, V, lens, cols, rng):
    """Host CSR: document d stores lens[d % len(lens)] words, word c of every
    (c, length) in cols is then reset to the last `length` documents; counts
    in 1 .. 5, one stored entry in twenty a stored zero."""
    mask = np.zeros((n, V), dtype=bool)
    for d in range(n):
        mask[d, rng.choice(V, lens[d % len(lens)], replace=False)] = True
    for c, length in cols:
        mask[:, c] = False
        mask[n - length:, c] = True
    cts = rng.integers(1, 6, int(mask.sum())) * (rng.random(int(mask.sum())) >= 0.05)
    rowptr = np.concatenate([[0], np.cumsum(mask.sum(1))])
    return rowptr, np.nonzero(mask)[1].astype(np.int32), cts.astype(np.float64)


@functools.lru_cache(maxsize=None)
def case(k, V=500, lens=LENS, n=None, cols=(), peaked=False, maxInner=100):
    rng = np.random.default_rng(3)
    n = n or len(lens)
    csr = corpus(n, V, lens, cols, rng)
    # peaked: a topic's mass on a few words; the floor keeps exp(E(lambda)) >= 1e-46, inside
    # fp64's normal range (the reference's longdouble reaches 1e-4932, the device does not)
    lam = rng.gamma(0.1, 1.0, (k, V)) + 1e-2 if peaked else rng.gamma(100.0, 0.01, (k, V))
    alpha, gamma0 = rng.uniform(0.01, 1.0, k), rng.gamma(100.0, 0.01, (n, k))
    weights = rng.integers(0, 3, n).astype(np.float64)
    ref = R.estep(*csr, lam, alpha, gamma0, weights, maxInner)
    changes = np.array(ref["changes"], dtype=np.float64)
    assert np.all(np.abs(changes / 1e-3 - 1.0) > 1e-6)      # clear of the threshold
    return csr, lam, alpha, gamma0, weights, maxInner, ref


def check(cuda, c):
    csr, lam, alpha, gamma0, weights, maxInner, ref = c
    k, V = lam.shape
    n = len(csr[0]) - 1
    docs = L.LDADocs(rows(csr, V, cuda))
    plan = L.LDAPlan(k, V).set_topics(dev(lam, cuda))
    args = (docs, dev(alpha, cuda), dev(gamma0, cuda), dev(weights, cuda), maxInner)
    calls = []
    for _ in range(2):
        gd = torch.empty((n, k), dtype=torch.float64, device=cuda)
        it = torch.empty(n, dtype=torch.int32, device=cuda)
        out = plan.estep(*args, gamma=gd, iters=it)
        part = plan.bound(docs, args[1], gd, args[3])
        calls.append([t.cpu().numpy() for t in (out, gd, it, part, *plan.infer(*args))])
    assert all(a.tobytes() == b.tobytes() for a, b in zip(*calls))
    out, gamma, iters, part, gamma2, iters2 = calls[0]
    assert gamma.tobytes() == gamma2.tobytes() and iters.tobytes() == iters2.tobytes()
    assert np.array_equal(iters, ref["iters"]) and not gamma[iters == 0].any()
    want = ref["gamma"]
    deviation = float(np.max(np.abs(gamma - want) / np.where(want == 0, 1, want)))
    print(f"lda gamma deviation k={k} n={n} V={V}: {deviation:.3e}")
    assert deviation <= BOUND
    stat = out[:k * V].reshape(k, V)
    assert np.all(np.abs(stat - ref["stat"]) <= BOUND * ref["stat"])    # positive terms
    assert np.all(np.abs(out[k * V:-1] - ref["logphat"]) <= BOUND * ref["logphatAbs"])
    assert out[-1] == ref["nonEmpty"]
    total, bar = R.bound(*csr, lam, alpha, gamma, weights)
    assert abs(part[0] - total) <= BOUND * bar


def test_digamma(cuda):
    """|error| <= 16 ulps of the largest term: 1 / x, the harmonic terms (< 3)
    and log(x + 10), each rounded once."""
    x = np.concatenate([np.logspace(-3, 6, 4000), [1.4616321449683623, 9.999999, 10.0]])
    got = L.digamma(dev(x, cuda)).cpu().numpy()
    mpmath.mp.dps = 30
    want = np.array([float(mpmath.digamma(mpmath.mpf(float(v)))) for v in x])
    assert np.all(np.abs(got - want) <= 16 * EPS * (1 / x + 3 + np.log(x + 10)))
    assert np.all(np.abs(R.digamma(x).astype(np.float64) - want) <= 2 * EPS * np.abs(want) + 1e-17)


@pytest.mark.parametrize("k", [1, 2, 3, 8, 9, 63, 64, 65, 100, 256])
def test_lane_layouts_and_document_lengths(cuda, k):
    assert N.load().cyc_lda_max_topics() == 256
    check(cuda, case(k))


@pytest.mark.parametrize("k, peaked, maxInner", [(9, False, 1), (100, True, 1), (3, True, 100),
                                                 (64, True, 100), (256, True, 100)])
def test_peaked_topics_and_the_sweep_cap(cuda, k, peaked, maxInner):
    check(cuda, case(k, peaked=peaked, maxInner=maxInner))


@pytest.mark.parametrize("k, peaked", [(8, True), (100, False), (256, True)])
def test_document_lengths_at_the_lds_tier(cuda, k, peaked):
    words = N.load().cyc_lda_slab_bytes() // (8 * N.load().cyc_lda_topic_stride(k))
    assert L.LDAPlan(k, 8).slabWords == words
    check(cuda, case(k, V=2 * words + 7, lens=(words, words + 1, 5, words - 1), peaked=peaked))


@pytest.mark.parametrize("k", [3, 65])
def test_word_lengths_at_the_segment(cuda, k):
    seg = int(N.load().cyc_lda_segment_entries())
    lengths = (0, 1, seg - 1, seg, seg + 1, 2 * seg + 3)
    c = case(k, V=40, lens=(3,), n=2 * seg + 3, cols=tuple(enumerate(lengths)))
    assert tuple(np.bincount(c[0][1], minlength=40)[:6]) == lengths
    check(cuda, c)


@pytest.mark.parametrize("n, V, k", [(1, 50, 8), (63, 50, 8), (65, 50, 8), (1025, 50, 8),
                                     (33, 65537, 2)])
def test_document_counts_and_a_wide_vocabulary(cuda, n, V, k):
    assert N.load().cyc_lda_run_docs() == 1024
    check(cuda, case(k, V=V, lens=(6,), n=n))


def test_transform_and_log_perplexity(cuda):
    csr, lam, alpha, _, _, _, _ = case(8)
    rng = np.random.default_rng(4)
    csr = corpus(40, 500, (0, 7, 30), (), rng)
    model = L.LocalLDAModel(lam.T, alpha, 0.3, seed=5)
    gamma0 = np.random.default_rng(5).gamma(100.0, 0.01, (40, 8))
    ref = R.estep(*csr, lam, alpha, gamma0)
    total = ref["gamma"].sum(1, keepdims=True)
    want = ref["gamma"] / np.where(total == 0, 1, total)
    got = model.transform(rows(csr, 500, cuda)).cpu().numpy()
    assert np.all(np.abs(got - want) <= BOUND * want) and not got[::3].any()
    part, bar = R.bound(*csr, lam, alpha, ref["gamma"])
    lamL, eta = lam.astype(R.LD), R.LD(0.3)
    terms = np.concatenate([((eta - lamL) * R.topics(lam)[1].T).ravel(), R.lgamma(lamL.ravel()),
                            -R.lgamma(np.full(lam.size, eta)), R.lgamma(np.full(8, eta * 500)),
                            -R.lgamma(lamL.sum(1))])
    tokens = csr[2].sum()
    perplexity = model.logPerplexity(rows(csr, 500, cuda))
    assert abs(perplexity + float(part + terms.sum()) / tokens) \
        <= BOUND * float(bar + np.abs(terms).sum()) / tokens


def test_refusals(cuda):
    csr = list(corpus(4, 20, (3,), (), np.random.default_rng(0)))
    csr[2][1] = -1.0
    with pytest.raises(N.IllegalArgumentException, match="requirement failed: term counts"):
        L.LDADocs(rows(csr, 20, cuda))
    for k in (0, 257):
        with pytest.raises(N.IllegalArgumentException, match=f"got {k}"):
            L.LDAPlan(k, 20)
        with pytest.raises(N.IllegalArgumentException, match=f"got {k}"):
            L.LDA(k=k)
    with pytest.raises(N.IllegalArgumentException, match="em"):
        L.LDA(optimizer="em")


def test_whole_fit_on_the_device_step(cuda):
    """max|dlambda| / max|lambda| against the restatement's step through the same
    fit_online.  Measured on an MI355X: 7.905e-15; asserted at 100 x that, rounded up to a
    power of ten; alpha at gamma's bound."""
    csr = corpus(300, 400, (0, 5, 20, 40), (), np.random.default_rng(2))
    kw = dict(k=3, maxIter=5, seed=1, subsamplingRate=0.5)
    host = R.Step(*csr)
    want, wantAlpha = L.fit_online(host, 400, **kw)
    assert np.all(np.abs(np.array(host.changes, dtype=np.float64) / 1e-3 - 1.0) > 1e-6)
    got, alpha = L.fit_online(L.LDADeviceStep(rows(csr, 400, cuda), 3), 400, **kw)
    deviation = float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
    print(f"lda fit deviation: {deviation:.3e}")
    assert deviation <= FIT_BOUND and np.all(np.abs(alpha - wantAlpha) <= BOUND * wantAlpha)
    assert not np.array_equal(alpha, np.full(3, 1.0 / 3))
    model = L.LDA(**kw).fit(rows(csr, 400, cuda))
    assert model.topicsMatrix().tobytes() == got.T.tobytes()
    assert [len(t) for t, _ in model.describeTopics(4)] == [4, 4, 4]


def test_header_symbols():
    syms = {s for s in N.header_symbols() if s.startswith("cyc_lda_")}
    assert syms == {"cyc_lda_" + s for s in (
        "max_topics", "slab_bytes", "segment_entries", "run_docs", "topic_stride", "docs_create",
        "docs_destroy", "plan_create", "plan_destroy", "set_topics_dev", "infer_dev", "estep_dev",
        "bound_dev", "digamma_dev")}
    assert all(hasattr(N.load(), s) and s in N.SIGNATURES for s in syms)
