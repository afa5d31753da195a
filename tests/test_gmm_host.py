"""GaussianMixture, host side (no device): MultivariateGaussian and the numpy
restatement against the reference suites' known answers, the M-step
arithmetic, the sums-buffer layout, the refusals and the initial model."""
import ctypes
import math

import numpy as np
import pytest

import gmm_restatement as R
from cycloneml_amd import _native as N
from cycloneml_amd import gmm
from cycloneml_amd.clustering import GaussianMixture, MultivariateGaussian

# MultivariateGaussianSuite: (cov, x, pdf), mean 0
PDFS = [
    ([[1.0]], [0.0], 0.39894), ([[1.0]], [1.5], 0.12952),
    ([[4.0]], [0.0], 0.19947), ([[4.0]], [1.5], 0.15057),
    (np.eye(2), [0.0, 0.0], 0.159155), (np.eye(2), [1.0, 1.0], 0.05855),
    ([[4.0, -1.0], [-1.0, 2.0]], [0.0, 0.0], 0.060155),
    ([[4.0, -1.0], [-1.0, 2.0]], [1.0, 1.0], 0.033971),
    ([[1.0, 1.0], [1.0, 1.0]], [0.0, 0.0], 0.11254),
    ([[1.0, 1.0], [1.0, 1.0]], [1.0, 1.0], 0.068259),
]

# GaussianMixtureSuite's univariate data
UNI = np.array([-5.1971, -2.5359, -3.8220, -5.2211, -5.0602, 4.7118, 6.8989, 3.4592, 4.6322,
                5.7048, 4.6567, 5.5026, 4.5605, 5.2043, 6.2734]).reshape(-1, 1)
UNI_INIT = ([0.5, 0.5], [[-1.0], [1.0]], [[[1.0]], [[1.0]]])


@pytest.mark.parametrize("cov,x,want", PDFS)
def test_multivariate_gaussian_known_answers(cov, x, want):
    g = MultivariateGaussian(np.zeros(len(x)), cov)
    assert abs(g.pdf(x) - want) <= 1e-5
    assert abs(math.exp(g.logpdf(x)) - want) <= 1e-5
    A, u = R.consts(np.zeros(len(x)), cov)
    assert abs(math.exp(R.logpdf(x, np.zeros(len(x)), A, u)) - want) <= 1e-5
    assert g.u == u and np.array_equal(g.rootSigmaInv, A)


def test_restatement_univariate_known_answer():
    w, mu, cov, ll, it, hist = R.fit(UNI, None, UNI_INIT)
    assert it == 3 and len(hist) == 3
    np.testing.assert_allclose(w, [1 / 3, 2 / 3], atol=1e-3)
    np.testing.assert_allclose(mu.ravel(), [-4.3673, 5.1604], atol=1e-3)
    np.testing.assert_allclose(cov.ravel(), [1.1098, 0.86644], atol=1e-3)
    assert abs(ll - -30.3754783) <= 1e-6


def test_no_nonzero_singular_values():
    with pytest.raises(N.IllegalArgumentException, match="no non-zero singular values"):
        MultivariateGaussian([0.0, 0.0], np.zeros((2, 2)))


def test_singular_covariance_has_a_zero_row():
    g = MultivariateGaussian([0.0, 0.0], [[1.0, 1.0], [1.0, 1.0]])
    assert np.count_nonzero(np.abs(g.rootSigmaInv).sum(axis=1)) == 1


def test_sums_layout_and_length():
    assert gmm.sums_length(3, 4) == 1 + 3 + 12 + 30
    k, d = 2, 3
    buf = np.arange(gmm.sums_length(k, d), dtype=np.float64)
    ll, W, M, S = gmm.split_sums(buf, k, d)
    assert ll == 0.0
    assert W.tolist() == [1.0, 2.0]
    assert M.tolist() == [[3.0, 4.0, 5.0], [6.0, 7.0, 8.0]]
    assert S.shape == (2, 6) and S[0, 0] == 9.0 and S[1, 5] == 20.0
    # packed upper, column-major: entry (a, b), a <= b, at b(b+1)/2 + a
    full = gmm.unpack_upper(np.array([11.0, 12.0, 22.0, 13.0, 23.0, 33.0]), 3)
    assert full.tolist() == [[11.0, 12.0, 13.0], [12.0, 22.0, 23.0], [13.0, 23.0, 33.0]]
    with pytest.raises(N.IllegalArgumentException):
        gmm.split_sums(buf[:-1], k, d)


def test_m_step_on_a_hand_made_buffer():
    # component 0: rows (1, 2) and (3, 6), r = 1 and 3; component 1: row (2, 0), r = 2
    k, d = 2, 2
    W = np.array([4.0, 2.0])
    M = np.array([[1.0 + 9.0, 2.0 + 18.0], [4.0, 0.0]])
    S = np.array([[1.0 + 27.0, 2.0 + 54.0, 4.0 + 108.0], [8.0, 0.0, 0.0]])
    buf = np.concatenate([[-7.0], W, M.ravel(), S.ravel()])
    w, mu, cov = gmm.m_step(buf, k, d)
    assert w.tolist() == [4.0 / 6.0, 2.0 / 6.0]
    assert mu.tolist() == [[2.5, 5.0], [2.0, 0.0]]
    # cov_0 = S / W - mu mu^T = [[7 - 6.25, 14 - 12.5], [., 28 - 25]]
    assert cov[0].tolist() == [[0.75, 1.5], [1.5, 3.0]]
    assert cov[1].tolist() == [[0.0, 0.0], [0.0, 0.0]]
    w2, mu2, cov2 = R.mstep(buf, k, d)
    assert np.array_equal(w, w2) and np.array_equal(mu, mu2) and np.array_equal(cov, cov2)


def test_m_step_matches_restatement_bits():
    rng = np.random.default_rng(5)
    X = rng.normal(size=(40, 3)) + 2.0
    sums, _, _ = R.em_step(X, None, [0.3, 0.7], X[:2], np.stack([np.eye(3)] * 2))
    a = gmm.m_step(sums, 2, 3)
    b = R.mstep(sums, 2, 3)
    for u, v in zip(a, b):
        assert np.array_equal(u, v)


def test_refusals():
    import torch
    from cycloneml_amd.linalg import CSRRows
    with pytest.raises(N.IllegalArgumentException, match="k must be positive"):
        GaussianMixture(k=0)
    with pytest.raises(N.IllegalArgumentException, match="k must be positive"):
        gmm.GMMPlan(0, 3)
    csr = CSRRows.__new__(CSRRows)      # fit looks at the type alone
    with pytest.raises(N.IllegalArgumentException, match="CSR rows are not supported"):
        GaussianMixture(k=2).fit(csr)
    with pytest.raises(N.IllegalArgumentException, match="up to 1024 features"):
        GaussianMixture(k=2).fit(torch.zeros((4, 1025), dtype=torch.float64))
    with pytest.raises(N.IllegalArgumentException, match="up to 1024 features"):
        gmm.GMMPlan(2, 1025)
    # a row of the wrong width
    with pytest.raises(N.IllegalArgumentException, match="features"):
        GaussianMixture(k=2, initialModel=UNI_INIT).fit(torch.zeros((4, 3), dtype=torch.float64))
    with pytest.raises(N.IllegalArgumentException):
        MultivariateGaussian([0.0, 0.0], np.eye(2)).logpdf([1.0, 2.0, 3.0])


def test_c_abi_refusals():
    lib = N.load()
    h = ctypes.c_void_p()
    assert lib.cyc_gmm_plan_create(0, 3, 0, ctypes.byref(h)) == N.CYC_ERR_INVALID_ARG
    assert b"requirement failed" in lib.cyc_last_error()
    assert lib.cyc_gmm_plan_create(2, 1025, 0, ctypes.byref(h)) == N.CYC_ERR_INVALID_ARG
    assert b"1024" in lib.cyc_last_error()
    assert lib.cyc_gmm_plan_create(2, 0, 0, ctypes.byref(h)) == N.CYC_ERR_INVALID_ARG
    assert lib.cyc_gmm_plan_create(2, 3, -1, ctypes.byref(h)) == N.CYC_ERR_INVALID_ARG


def test_initial_model_is_deterministic_for_a_seed():
    idx = gmm.init_sample_indices(1000, 3, 7)
    assert idx.shape == (15,) and idx.min() >= 0 and idx.max() < 1000
    assert np.array_equal(idx, gmm.init_sample_indices(1000, 3, 7))
    assert np.array_equal(idx, np.random.default_rng(7).integers(0, 1000, size=15))
    assert not np.array_equal(idx, gmm.init_sample_indices(1000, 3, 8))
    rng = np.random.default_rng(0)
    X = rng.normal(size=(1000, 4))
    w, mu, cov = gmm.init_from_samples(X[idx], 3)
    assert w.tolist() == [1 / 3] * 3
    for j in range(3):
        s = X[idx[5 * j:5 * j + 5]]
        np.testing.assert_allclose(mu[j], s.mean(axis=0), rtol=1e-14)
        np.testing.assert_allclose(np.diag(cov[j]), (s * s).sum(axis=0) / 5 - mu[j] ** 2,
                                   rtol=1e-12, atol=1e-15)
        assert np.count_nonzero(cov[j] - np.diag(np.diag(cov[j]))) == 0
    with pytest.raises(N.IllegalArgumentException):
        gmm.init_sample_indices(0, 3, 7)


def test_model_constants_image():
    gs = [MultivariateGaussian([1.0, 2.0], np.eye(2)), MultivariateGaussian([3.0, 4.0], np.eye(2))]
    m = gmm.model_constants([0.25, 0.75], gs)
    assert m.size == 2 + 4 + 8 + 2
    assert m[:6].tolist() == [0.25, 0.75, 1.0, 2.0, 3.0, 4.0]
    assert np.array_equal(m[6:10].reshape(2, 2), gs[0].rootSigmaInv)
    assert m[-2:].tolist() == [gs[0].u, gs[1].u]
