"""NaiveBayes restated in plain numpy (Spark 3.3 ml.classification.NaiveBayes):
the aggregate walks the rows in order, the M steps and raw forms walk classes
and features in order.  Nothing here uses cycloneml_amd.naive_bayes.

Also the input generators and the case list of test_naive_bayes_host.py and
test_naive_bayes_gpu.py.  The raw forms, the probability, the argmax and their
error magnitudes restate the model's predictions, which the package does not
run on the device yet.
"""
import functools

import numpy as np

TYPES = ("multinomial", "complement", "bernoulli", "gaussian")


# -- aggregate -------------------------------------------------------------------

def aggregate(X, y, w, C, modelType):
    """(W, S, Q or None) and the absolute sums (aS, aQ) behind S and Q."""
    n, d = X.shape
    gauss = modelType == "gaussian"
    W = np.zeros(C)
    S = np.zeros((C, d))
    Q = np.zeros((C, d)) if gauss else None
    aS = np.zeros((C, d))
    aQ = np.zeros((C, d)) if gauss else None
    for i in range(n):
        c = int(y[i])
        wi = 1.0 if w is None else w[i]
        W[c] += wi
        S[c] += wi * X[i]
        aS[c] += np.abs(wi * X[i])
        if gauss:
            Q[c] += wi * (X[i] * X[i])
            aQ[c] += np.abs(wi) * (X[i] * X[i])
    return W, S, Q, aS, aQ


def sums_buffer(W, S, Q):
    return np.concatenate([W, S.ravel()] + ([Q.ravel()] if Q is not None else []))


# -- M step ------------------------------------------------------------------------

def m_step(W, S, Q, modelType, lam=1.0):
    C, d = S.shape
    D = 0.0
    for c in range(C):
        D = D + W[c]
    pi = np.zeros(C)
    theta = np.zeros((C, d))
    sigma = np.zeros((0, 0))
    if modelType == "gaussian":
        sigma = np.zeros((C, d))
        best = -np.inf
        for j in range(d):
            ts, tq = 0.0, 0.0
            for c in range(C):
                ts = ts + S[c, j]
                tq = tq + Q[c, j]
            best = max(best, tq / D - ts * ts / D / D)
        eps = 1e-9 * best
        for c in range(C):
            pi[c] = np.log(W[c]) - np.log(D)
            for j in range(d):
                theta[c, j] = S[c, j] / W[c]
                sigma[c, j] = eps + Q[c, j] / W[c] - theta[c, j] * theta[c, j]
        return pi, theta, sigma
    for c in range(C):
        pi[c] = np.log(W[c] + lam) - np.log(D + C * lam)
    if modelType == "multinomial":
        for c in range(C):
            t = 0.0
            for j in range(d):
                t = t + S[c, j]
            lt = np.log(t + d * lam)
            for j in range(d):
                theta[c, j] = np.log(S[c, j] + lam) - lt
    elif modelType == "complement":
        T = np.zeros(d)
        for j in range(d):
            for c in range(C):
                T[j] = T[j] + S[c, j]
        for c in range(C):
            t = 0.0
            for j in range(d):
                t = t + (T[j] - S[c, j])
            lt = np.log(t + d * lam)
            for j in range(d):
                theta[c, j] = -(np.log((T[j] - S[c, j]) + lam) - lt)
    elif modelType == "bernoulli":
        for c in range(C):
            lw = np.log(W[c] + 2.0 * lam)
            for j in range(d):
                theta[c, j] = np.log(S[c, j] + lam) - lw
    else:
        raise ValueError(modelType)
    return pi, theta, sigma


# -- predictions -------------------------------------------------------------------

def raw(X, pi, theta, sigma, modelType):
    """(raw (n x C), B (n x C)): B is the error magnitude of the linear part,
    |b_c| + sum_j |x_j M_cj| (gaussian: |pi_c| + |sum log sigma| / 2 + sum_j
    (x_j - theta_cj)^2 / sigma_cj); complement's raw is normalized after it
    (bars adds that step's share)."""
    n, d = X.shape
    C = pi.size
    with np.errstate(all="ignore"):
        if modelType == "gaussian":
            ls = np.zeros(C)
            for j in range(d):
                ls = ls + np.log(sigma[:, j])
            q = np.zeros((n, C))
            for j in range(d):
                df = X[:, j, None] - theta[None, :, j]
                q = q + df * df / sigma[None, :, j]
            return pi[None, :] - (q + ls[None, :]) / 2.0, np.abs(pi)[None, :] + \
                np.abs(ls)[None, :] / 2.0 + q
        if modelType == "bernoulli":
            L = np.log1p(-np.exp(theta))
            b = pi.copy()
            s = np.zeros(C)
            for j in range(d):
                s = s + L[:, j]
            b = pi + s
            M = theta - L
        elif modelType == "complement":
            b, M = np.zeros(C), theta
        else:
            b, M = pi, theta
        t = np.zeros((n, C))
        B = np.zeros((n, C))
        for j in range(d):
            # absent (zero) entries are skipped: the reference's sparse dot
            xj = X[:, j, None]
            term = np.where(xj != 0.0, xj * M[None, :, j], 0.0)
            t = t + term
            B = B + np.abs(term)
        t = b[None, :] + t
        B = np.abs(b)[None, :] + B
        if modelType == "complement":
            m = t.max(axis=1, keepdims=True)
            s = np.zeros((n, 1))
            for c in range(C):
                s = s + np.exp(t[:, c:c + 1] - m)
            t = t - (m + np.log(s))
    return t, B


def probability(r):
    with np.errstate(all="ignore"):
        e = np.exp(r - r.max(axis=1, keepdims=True))
        s = np.zeros((r.shape[0], 1))
        for c in range(r.shape[1]):
            s = s + e[:, c:c + 1]
        return e / s


def predict(r):
    """DenseVector.argmax: the first index of the largest value."""
    out = np.zeros(r.shape[0], dtype=np.int32)
    for i in range(r.shape[0]):
        best, bi = r[i, 0], 0
        for c in range(1, r.shape[1]):
            if r[i, c] > best:
                best, bi = r[i, c], c
        out[i] = bi
    return out


def bars(r, B, modelType):
    """(raw bar, prob bar) per entry, as multiples of 1e-10."""
    p = probability(r)
    mix = (p * B).sum(axis=1, keepdims=True)
    rb = B + (1.0 + mix if modelType == "complement" else 0.0)
    return 1e-10 * rb, 1e-10 * p * (2.0 + B + mix)


def duplicates(pi, theta, sigma, modelType):
    """Classes whose model row repeats an earlier class bit for bit (complement
    at d = 1 has theta = 0 throughout): both sides run the same arithmetic on
    the same operands for such a pair, so its raw values are equal exactly and
    the tie goes to the lowest index -- a constructed tie, not a close call."""
    key = [theta] + ([] if modelType == "complement" else [pi[:, None]]) + \
        ([sigma] if modelType == "gaussian" else [])
    key = np.concatenate(key, axis=1)
    return np.array([any(key[c].tobytes() == key[e].tobytes() for e in range(c))
                     for c in range(pi.size)])


def ambiguous(r, rawBar, dup=None):
    """Rows whose two best raw values are closer than the sum of their bars
    (classes marked in dup left out)."""
    if dup is not None and dup.any():
        r, rawBar = r[:, ~dup], rawBar[:, ~dup]
    n, C = r.shape
    if C == 1:
        return np.zeros(n, dtype=bool)
    order = np.argsort(-r, axis=1, kind="stable")
    i = np.arange(n)
    a, b = order[:, 0], order[:, 1]
    return (r[i, a] - r[i, b]) <= rawBar[i, a] + rawBar[i, b]


# -- generators ----------------------------------------------------------------------

def frozen(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)
    return arrays


def labels(rng, n, C):
    """Every class present when n >= C (class i for row i < C), else 0..n-1."""
    y = rng.integers(0, C, size=n).astype(np.float64)
    m = min(n, C)
    y[:m] = np.arange(m)
    return y


def weights8(rng, n, y, C):
    """Multiples of 1/8 in [0, 4] with exact zeros; the first row of a class
    keeps a positive weight."""
    w = rng.integers(0, 33, size=n) / 8.0
    w[rng.random(n) < 0.1] = 0.0
    m = min(n, C)
    w[:m] = np.maximum(w[:m], 0.125)
    return w


@functools.lru_cache(maxsize=None)
def exact_rows(modelType, d, C, n, seed=0):
    """Integer features below 2^20 (0/1 for bernoulli, signed for gaussian),
    labels, weights8: every sum is exact in any order."""
    rng = np.random.default_rng(1009 * d + 31 * C + n + seed)
    y = labels(rng, n, C)
    if modelType == "bernoulli":
        X = (rng.random((n, d)) < 0.4).astype(np.float64)
    elif modelType == "gaussian":
        X = rng.integers(-1000, 1000, size=(n, d)).astype(np.float64)
    else:
        X = rng.integers(0, 1 << 20, size=(n, d)).astype(np.float64)
        X[rng.random((n, d)) < 0.3] = 0.0
    return frozen(X, y, weights8(rng, n, y, C))


@functools.lru_cache(maxsize=None)
def real_rows(modelType, d, C, n, seed=0):
    """Rows whose class shows: counts around a class profile (multinomial,
    complement), 0/1 draws from a class profile (bernoulli), blobs (gaussian);
    real weights in (0, 2) with exact zeros."""
    rng = np.random.default_rng(7919 * d + 101 * C + n + seed)
    y = labels(rng, n, C)
    yi = y.astype(np.int64)
    if modelType == "gaussian":
        centres = rng.normal(size=(C, d)) * 4.0
        X = centres[yi] + rng.normal(size=(n, d))
    elif modelType == "bernoulli":
        prof = rng.random((C, d)) * 0.8 + 0.1
        X = (rng.random((n, d)) < prof[yi]).astype(np.float64)
    else:
        prof = rng.random((C, d)) ** 3 * 6.0
        X = rng.poisson(prof[yi]).astype(np.float64) * (0.5 + rng.random((n, d)))
        X[rng.random((n, d)) < 0.2] = 0.0
        # no all-zero row: its raw values would tie exactly (complement has no
        # pi) on the restatement's side already
        empty = np.nonzero(~X.any(axis=1))[0]
        X[empty, empty % d] = 1.5 + rng.random(empty.size)
    w = rng.random(n) * 2.0
    w[rng.random(n) < 0.1] = 0.0
    m = min(n, C)
    w[:m] = np.maximum(w[:m], 0.25)
    return frozen(X, y, w)


@functools.lru_cache(maxsize=None)
def model_of(modelType, d, C, n, seed=0):
    """The restatement's own fit of real_rows (lam = 1); of at least 4 C rows,
    so that every class has weight when fewer rows are scored."""
    X, y, w = real_rows(modelType, d, C, max(n, 4 * C), seed)
    W, S, Q, _, _ = aggregate(X, y, w, C, modelType)
    return frozen(*m_step(W, S, Q, modelType, 1.0))


# -- cases -----------------------------------------------------------------------------

DS = [1, 3, 15, 16, 17, 64, 65, 130, 257]
CS = [1, 2, 3, 16, 17, 33]
ROWS = [1, 63, 64, 65, 255, 256, 257, 1000]
# the plan's constants (asserted against the device's queries in the GPU test):
# columns per lane group (of d + 1), rows per run, classes per pass
COL_TILES = (16, 32, 64, 128, 256)
ROWS_PER_RUN = 1024
CLASSES_PER_PASS = {"multinomial": 16, "complement": 16, "bernoulli": 16, "gaussian": 8}


def shape_cases():
    """(d, C, rows): every (d, C) at 257 rows, every row count at (17, 3), the
    shapes on both sides of each constant: d + 1 around every column tile, C
    around classes per pass (8 and 16), rows around rows per run."""
    cases = [(d, C, 257) for d in DS for C in CS]
    cases += [(17, 3, n) for n in ROWS if n != 257]
    cases += [(d, 3, 65) for d in (14, 30, 31, 32, 62, 63, 126, 127, 128, 254, 255, 256)]
    cases += [(17, C, 257) for C in (8, 9, 15)]
    cases += [(3, 2, n) for n in (1023, 1024, 1025, 2049)]
    # more runs than a workgroup holds (d + 1 > 128: one run per workgroup, so
    # 2049 rows are workgroups 0, 1, 2 along x), with one and two column blocks
    cases += [(130, 3, 2049), (257, 3, 2049)]
    return cases


@functools.lru_cache(maxsize=None)
def scored(modelType, d, C, n, seed=0):
    """(raw, B, rawBar, probBar, prob, pred, ambiguous) of real_rows under
    model_of."""
    X, _, _ = real_rows(modelType, d, C, n, seed)
    pi, theta, sigma = model_of(modelType, d, C, n, seed)
    r, B = raw(X, pi, theta, sigma, modelType)
    rb, pb = bars(r, B, modelType)
    return frozen(r, B, rb, pb, probability(r), predict(r),
                  ambiguous(r, rb, duplicates(pi, theta, sigma, modelType)))


# (d, C, rows, workspaceBytes): the run fold in groups of 1 (a run's partial is
# C (d + 1) doubles, doubled for gaussian, so 3000 rows are 3 runs in 3
# launches)
SMALL_WS_AGG = (17, 3, 3000, 3 * 18 * 8)
