"""The factorization machine's evaluation, updaters and fit as plain per-row,
per-element loops (the semantics cycloneml_amd/fm.py documents), and the
absolute-value sums the GPU tests' bars are made of."""
import math

import numpy as np

from cycloneml_amd import forest
from cycloneml_amd.kmeans_init import JavaRandom


def log1p_exp(x):
    return x + math.log1p(math.exp(-x)) if x > 0 else math.log1p(math.exp(x))


def split(coef, d, k, fitIntercept, fitLinear):
    V = [[float(coef[i * k + f]) for f in range(k)] for i in range(d)]
    w = [float(coef[d * k + i]) if fitLinear else 0.0 for i in range(d)]
    b = float(coef[-1]) if fitIntercept else 0.0
    return b, w, V


def taken(i, fraction, row):
    if fraction >= 1.0:
        return True
    u = int(np.asarray(forest.mix(42 + i, 0, 0, row)).ravel()[0]) >> 11
    return u >= int(forest.bernoulli_table(fraction)[0])


def evaluate(X, y, coef, k, loss, fitIntercept=True, fitLinear=True, i=1, fraction=1.0,
             rowOffset=0, order=None, bars=False):
    """(G, L, cnt), rows in `order` (default ascending); with bars also (raw,
    rawAbs per row, GAbs, LAbs): the sums of absolute values of every term."""
    n, d = X.shape
    b, w, V = split(coef, d, k, fitIntercept, fitLinear)
    gV = [[0.0] * k for _ in range(d)]
    gw, gb, L, cnt = [0.0] * d, 0.0, 0.0, 0.0
    aV = [[0.0] * k for _ in range(d)]
    aw, ab, aL = [0.0] * d, 0.0, 0.0
    raws, rawAbs = np.zeros(n), np.zeros(n)
    carry = 2.0 if loss == "squared" else 0.25          # |dm / draw|
    for r in (range(n) if order is None else order):
        if not taken(i, fraction, rowOffset + r):
            continue
        x = [float(v) for v in X[r]]
        nz = [j for j in range(d) if x[j] != 0.0]
        raw, ra = b, abs(b)
        if fitLinear:
            for j in nz:
                raw += w[j] * x[j]
                ra += abs(w[j] * x[j])
        s, sa = [0.0] * k, [0.0] * k
        for f in range(k):
            q = 0.0
            for j in nz:
                t = V[j][f] * x[j]
                s[f] += t
                q += t * t
                sa[f] += abs(t)
            raw += 0.5 * (s[f] * s[f] - q)
            ra += 0.5 * (sa[f] * sa[f] + q)
        yv = float(y[r])
        if loss == "squared":
            l, m = (raw - yv) * (raw - yv), 2.0 * (raw - yv)
        else:
            p = 1.0 / (1.0 + math.exp(-raw))
            l, m = (log1p_exp(-raw) if yv > 0 else log1p_exp(raw)), p - yv
        raws[r], rawAbs[r] = raw, ra
        ma = abs(m) + carry * ra                        # m and the bar it carries from raw
        for j in nz:
            for f in range(k):
                gV[j][f] += m * (x[j] * s[f] - (V[j][f] * x[j]) * x[j])
                aV[j][f] += ma * (abs(x[j]) * sa[f] + abs(V[j][f]) * x[j] * x[j])
            gw[j] += m * x[j]
            aw[j] += ma * abs(x[j])
        gb += m
        ab += ma
        L += l
        aL += abs(l) + (abs(m) if loss == "squared" else 1.0) * ra
        cnt += 1.0
    flat = lambda M, v, s: np.array([e for row in M for e in row] + (v if fitLinear else [])
                                    + ([s] if fitIntercept else []))       # noqa: E731
    G = flat(gV, gw, gb)
    if bars:
        return G, L, cnt, raws, rawAbs, flat(aV, aw, ab), aL
    return G, L, cnt


def norm(w):
    s = 0.0
    for v in w:
        s += v * v
    return math.sqrt(s)


class Updater:
    def __init__(self, solver, regParam, size):
        self.solver, self.reg = solver, regParam
        self.m, self.v, self.b1T, self.b2T = [0.0] * size, [0.0] * size, 1.0, 1.0

    def __call__(self, w, g, stepSize, it):
        w = list(w)
        if self.solver == "gd":
            eta = stepSize / math.sqrt(it)
            for e in range(len(w)):
                w[e] = w[e] * (1.0 - eta * self.reg)
                w[e] = w[e] + (-eta) * g[e]
        elif stepSize > 0:
            self.b1T *= 0.9
            self.b2T *= 0.999
            for e in range(len(w)):
                self.m[e] = self.m[e] * 0.9 + (1.0 - 0.9) * g[e]
                self.v[e] = self.v[e] * 0.999 + (1.0 - 0.999) * (g[e] * g[e])
                mHat = self.m[e] / (1.0 - self.b1T)
                vHat = self.v[e] / (1.0 - self.b2T)
                w[e] = w[e] - ((stepSize * mHat) / (math.sqrt(vHat) + 1e-8) + self.reg * w[e])
        nrm = norm(w)
        return w, 0.5 * self.reg * nrm * nrm


def init_coef(d, k, fitIntercept, fitLinear, initStd, seed):
    rnd = JavaRandom(seed)
    return [rnd.next_gaussian() * initStd for _ in range(d * k)] \
        + [0.0] * ((d if fitLinear else 0) + (1 if fitIntercept else 0))


def fit(X, y, k, loss, solver, fitIntercept=True, fitLinear=True, regParam=0.0, initStd=0.01,
        maxIter=100, stepSize=1.0, tol=1e-6, seed=0, fraction=1.0):
    d = X.shape[1]
    w = init_coef(d, k, fitIntercept, fitLinear, initStd, seed)
    upd = Updater(solver, regParam, len(w))
    _, regVal = upd(w, [0.0] * len(w), 0.0, 1)
    history, prev, converged, i = [], None, False, 1
    while not converged and i <= maxIter:
        G, L, cnt = evaluate(X, y, w, k, loss, fitIntercept, fitLinear, i, fraction)
        if cnt > 0:
            history.append(L / cnt + regVal)
            had, prev = prev is not None, w
            w, regVal = upd(w, [g / cnt for g in G], stepSize, i)
            if had:
                diff = norm([a - c for a, c in zip(prev, w)])
                converged = diff < tol * max(norm(w), 1.0)
        i += 1
    return np.array(w), history


def real_rows(n, d, seed, classifier=False):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, d)) * (rng.random((n, d)) < 0.7)
    y = (rng.random(n) < 0.5).astype(np.float64) if classifier else rng.normal(size=n)
    return X, y


def exact_rows(n, d, k, seed, fitIntercept=True, fitLinear=True):
    """Integer x in [-2, 2] (at most 6 non-zeros a row), coefficients and labels
    in quarters: every sum of the squared-loss evaluation is exact in any order,
    asserted by evaluating the rows forward and in reverse."""
    rng = np.random.default_rng(seed)
    X = np.zeros((n, d))
    for r in range(n):
        cols = rng.choice(d, size=min(d, 6), replace=False)
        X[r, cols] = rng.integers(-2, 3, size=cols.size)
    size = d * k + (d if fitLinear else 0) + (1 if fitIntercept else 0)
    coef = rng.integers(-2, 3, size=size) / 4.0
    y = rng.integers(-4, 5, size=n) / 4.0
    ref = evaluate(X, y, coef, k, "squared", fitIntercept, fitLinear)
    rev = evaluate(X, y, coef, k, "squared", fitIntercept, fitLinear, order=range(n - 1, -1, -1))
    assert ref[0].tobytes() == rev[0].tobytes() and ref[1:] == rev[1:]
    return X, y, coef, ref
