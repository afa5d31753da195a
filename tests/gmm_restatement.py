"""Plain numpy restatement of ml.clustering.GaussianMixture (Spark 3.3) and of
ml.stat.distribution.MultivariateGaussian, row by row in the reference's
order, with the absolute-product bounds the device tests scale their bars by.

It reproduces the reference suites' known answers (tests/test_gmm_host.py):
MultivariateGaussianSuite's pdf table and GaussianMixtureSuite's univariate
fit (3 iterations to weights (1/3, 2/3), means (-4.36726, 5.16044), variances
(1.109806, 0.866446), logLikelihood -30.3754783).
"""
import math

import numpy as np

EPSILON = 2.0 ** -52
DOUBLE_MAX = 1.7976931348623157e308


def consts(mean, cov):
    """(rootSigmaInv A (d x d), u) of one Gaussian."""
    mean = np.asarray(mean, dtype=np.float64).ravel()
    d = mean.size
    cov = np.asarray(cov, dtype=np.float64).reshape(d, d)
    lam, U = np.linalg.eigh(cov)
    tol = EPSILON * lam.max() * d
    if not (lam > tol).any():
        raise ValueError("Covariance matrix has no non-zero singular values")
    log_pseudo_det = 0.0
    pinv = np.zeros(d)
    for i in range(d):
        if lam[i] > tol:
            log_pseudo_det += math.log(lam[i])
            pinv[i] = math.sqrt(1.0 / lam[i])
    A = pinv[:, None] * U.T
    return A, -0.5 * (d * math.log(2.0 * math.pi) + log_pseudo_det)


def logpdf(x, mean, A, u):
    v = A @ (np.asarray(x, dtype=np.float64) - mean)
    return u - 0.5 * float(v @ v)


def estep(X, omega, weights, means, As, us):
    """One E step over the rows in order.  Returns a dict: logpdf (n x k), B
    (n x k, the sum of absolute products behind q_ij), p (n x k), s (n), prob
    (n x k, p / s), R (n x k, omega prob), ll and llTerms (n, omega log s)."""
    X = np.asarray(X, dtype=np.float64)
    n, d = X.shape
    k = len(weights)
    omega = np.ones(n) if omega is None else np.asarray(omega, dtype=np.float64)
    lp = np.empty((n, k))
    B = np.empty((n, k))
    p = np.empty((n, k))
    s = np.empty(n)
    prob = np.empty((n, k))
    R = np.zeros((n, k))
    terms = np.zeros(n)
    ll = 0.0
    absA = [np.abs(A) for A in As]
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(n):
            si = 0.0
            for j in range(k):
                delta = X[i] - means[j]
                v = As[j] @ delta
                lp[i, j] = us[j] - 0.5 * float(v @ v)
                b = absA[j] @ np.abs(delta)
                B[i, j] = float(b @ b)
                p[i, j] = EPSILON + weights[j] * math.exp(lp[i, j]) \
                    if not math.isnan(lp[i, j]) else math.nan
                si += p[i, j]
            s[i] = si
            prob[i] = p[i] / si
            if omega[i] > 0.0:
                terms[i] = omega[i] * math.log(si)
                ll += terms[i]
                R[i] = omega[i] * prob[i]
    return dict(logpdf=lp, B=B, p=p, s=s, prob=prob, R=R, ll=ll, llTerms=terms, omega=omega)


def tri_index(d):
    """(a, b, pos): the entries a <= b of a packed upper triangle, pos = b(b+1)/2 + a."""
    a, b = np.triu_indices(d)
    return a, b, b * (b + 1) // 2 + a


def aggregate(X, R):
    """(W (k), M (k x d), S (k x d(d+1)/2)) over the rows in order, and the
    same sums over absolute values (Wb, Mb, Sb).  Rows whose R are all zero
    are skipped, whatever their features hold."""
    X = np.asarray(X, dtype=np.float64)
    n, d = X.shape
    k = R.shape[1]
    a, b, pos = tri_index(d)
    tri = d * (d + 1) // 2
    W, M, S = np.zeros(k), np.zeros((k, d)), np.zeros((k, tri))
    Wb, Mb, Sb = np.zeros(k), np.zeros((k, d)), np.zeros((k, tri))
    for i in range(n):
        r = R[i]
        if not r.any():
            continue
        x = X[i]
        xx = np.empty(tri)
        xx[pos] = x[a] * x[b]
        W += r
        M += r[:, None] * x[None, :]
        S += r[:, None] * xx[None, :]
        ar, ax, axx = np.abs(r), np.abs(x), np.abs(xx)
        Wb += ar
        Mb += ar[:, None] * ax[None, :]
        Sb += ar[:, None] * axx[None, :]
    return (W, M, S), (Wb, Mb, Sb)


def pack(ll, W, M, S):
    return np.concatenate([[ll], W, M.ravel(), S.ravel()])


def mstep(sums, k, d):
    """(weights, means (k x d), covs (k x d x d)) from [ll | W | M | S]."""
    tri = d * (d + 1) // 2
    W = sums[1:1 + k]
    M = sums[1 + k:1 + k + k * d].reshape(k, d)
    S = sums[1 + k + k * d:].reshape(k, tri)
    means = np.empty((k, d))
    covs = np.empty((k, d, d))
    for j in range(k):
        mu = M[j] / W[j]
        U = S[j].copy()
        for bb in range(d):                      # spr(-W_j, mu, U)
            temp = -W[j] * mu[bb]
            for aa in range(bb + 1):
                U[bb * (bb + 1) // 2 + aa] += mu[aa] * temp
        U *= 1.0 / W[j]                          # scal(1 / W_j, U)
        for bb in range(d):
            for aa in range(bb + 1):
                covs[j, aa, bb] = covs[j, bb, aa] = U[bb * (bb + 1) // 2 + aa]
        means[j] = mu
    return W / W.sum(), means, covs


def em_step(X, omega, weights, means, covs):
    """(sums buffer, E-step dict, bounds) of one pass from a model."""
    k = len(weights)
    cs = [consts(means[j], covs[j]) for j in range(k)]
    e = estep(X, omega, weights, means, [c[0] for c in cs], [c[1] for c in cs])
    (W, M, S), bounds = aggregate(X, e["R"])
    return pack(e["ll"], W, M, S), e, bounds


def fit(X, omega, init, maxIter=100, tol=0.01):
    """The reference's loop.  Returns (weights, means, covs, ll, numIter, history)."""
    X = np.asarray(X, dtype=np.float64)
    d = X.shape[1]
    weights, means, covs = (np.array(v, dtype=np.float64) for v in init)
    k = weights.size
    means = means.reshape(k, d)
    covs = covs.reshape(k, d, d)
    ll, ll_prev, it, history = -DOUBLE_MAX, 0.0, 0, []
    while it < maxIter and abs(ll - ll_prev) > tol:
        sums, _, _ = em_step(X, omega, weights, means, covs)
        weights, means, covs = mstep(sums, k, d)
        ll_prev, ll = ll, float(sums[0])
        history.append(ll)
        it += 1
    return weights, means, covs, ll, it, history


def r_bar(e, rel=1e-10):
    """The responsibility bar at unit weight: rel r_ij (2 + B_ij + sum_l r_il B_il)."""
    rb = (e["prob"] * e["B"]).sum(axis=1, keepdims=True)
    return rel * e["prob"] * (2.0 + e["B"] + rb)


def sums_bars(X, e, bounds, rel=1e-10, with_estep=True):
    """The bars of a sums buffer, laid out like the buffer: the aggregate's
    rel sum_i r_ij |x_ia x_ib| (and |x_ia|, 1 for M, W), plus, with_estep,
    sum_i (bar of r_ij) |x_ia x_ib| and the ll bar."""
    Wb, Mb, Sb = bounds
    bar = pack(0.0, rel * Wb, rel * Mb, rel * Sb)
    if with_estep:
        with np.errstate(invalid="ignore"):
            dR = np.where(e["omega"][:, None] > 0.0, e["omega"][:, None] * r_bar(e, rel), 0.0)
            rb = np.where(e["omega"] > 0.0, (e["prob"] * e["B"]).sum(axis=1), 0.0)
        _, extra = aggregate(X, dR)
        bar += pack(rel * float((e["omega"] * (1.0 + rb)).sum()), *extra)
    return bar
