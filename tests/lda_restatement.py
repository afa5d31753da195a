"""The LDA E step, bound and online fit step of cycloneml_amd/lda.py's docstring
restated in numpy.longdouble over host CSR documents (rowptr, ids, cts), with
its own digamma and lgamma, and the sums of absolute terms the tests' bars use."""
import numpy as np

LD = np.longdouble
# B_2n / (2 n), n = 1 .. 8, and B_2n / (2 n (2 n - 1))
PSI_C = [LD(1) / 12, -LD(1) / 120, LD(1) / 252, -LD(1) / 240, LD(1) / 132, -LD(691) / 32760,
         LD(1) / 12, -LD(3617) / 8160]
LG_C = [LD(1) / 12, -LD(1) / 360, LD(1) / 1260, -LD(1) / 1680, LD(1) / 1188, -LD(691) / 360360,
        LD(1) / 156, -LD(3617) / 122400]


def _shift(x):
    """x moved up to y = x + m >= 20 by whole steps: (y, the steps x + i for i <
    m with ones elsewhere, their mask)."""
    x = np.atleast_1d(np.asarray(x, dtype=LD))
    m = np.maximum(0, np.ceil(20 - x)).astype(np.int64)
    i = np.arange(int(m.max(initial=0)))
    on = i < m[..., None]
    return x + m, np.where(on, x[..., None] + i, 1), on


def digamma(x):
    y, steps, on = _shift(x)
    y2 = 1 / (y * y)
    series = sum(c * y2 ** (n + 1) for n, c in enumerate(PSI_C))
    return np.log(y) - 1 / (2 * y) - series - np.where(on, 1 / steps, 0).sum(-1)


def lgamma(x):
    y, steps, _ = _shift(x)
    s = np.log(steps).sum(-1)
    series = sum(c / y ** (2 * n + 1) for n, c in enumerate(LG_C))
    return (y - LD(0.5)) * np.log(y) - y + np.log(8 * np.arctan(LD(1))) / 2 + series - s


def expect(v):
    return digamma(v) - digamma(v.sum())


def topics(lam):
    """(B, E(lambda)), both V x k."""
    Elam = np.stack([expect(row) for row in np.asarray(lam, dtype=LD)]).T
    return np.exp(Elam), Elam


def infer_doc(Bd, cts, alpha, g0, maxInner):
    """(gamma, e, phi, sweeps, each sweep's mean change)."""
    k = alpha.size
    gamma = g0.copy()
    e = np.exp(expect(gamma))
    phi = Bd @ e + LD(1e-100)
    changes = []
    while True:
        last = gamma
        gamma = e * (Bd.T @ (cts / phi)) + alpha
        e = np.exp(expect(gamma))
        phi = Bd @ e + LD(1e-100)
        changes.append(np.abs(gamma - last).sum() / k)
        if not changes[-1] > 1e-3 or len(changes) == maxInner:
            return gamma, e, phi, len(changes), changes


def estep(rowptr, ids, cts, lam, alpha, gamma0, weights=None, maxInner=100):
    """dict of gamma, iters, changes, stat, logphat (with its sum of absolute
    terms logphatAbs; stat's terms are all positive) and nonEmpty."""
    lam, alpha = np.asarray(lam, dtype=LD), np.asarray(alpha, dtype=LD)
    k, V = lam.shape
    n = len(rowptr) - 1
    B, _ = topics(lam)
    w = np.ones(n) if weights is None else np.asarray(weights)
    out = dict(gamma=np.zeros((n, k), dtype=LD), iters=np.zeros(n, dtype=np.int32), changes=[],
               logphat=np.zeros(k, dtype=LD), logphatAbs=np.zeros(k, dtype=LD), nonEmpty=0.0)
    acc = np.zeros((V, k), dtype=LD)
    for d in range(n):
        sl = slice(rowptr[d], rowptr[d + 1])
        keep = cts[sl] != 0
        if w[d] == 0 or not keep.any():
            continue
        di, dc = ids[sl][keep], cts[sl][keep].astype(LD)
        gamma, e, phi, it, changes = infer_doc(B[di], dc, alpha, gamma0[d].astype(LD), maxInner)
        out["gamma"][d], out["iters"][d] = gamma, it
        out["changes"] += changes
        acc[di] += LD(w[d]) * np.outer(dc / phi, e)
        out["logphat"] += LD(w[d]) * expect(gamma)
        out["logphatAbs"] += LD(w[d]) * np.abs(expect(gamma))
        out["nonEmpty"] += float(w[d])
    out["stat"] = (B * acc).T
    return out


def bound(rowptr, ids, cts, lam, alpha, gamma, weights=None):
    """(corpusPart, its sum of absolute terms)."""
    alpha = np.asarray(alpha, dtype=LD)
    _, Elam = topics(lam)
    w = np.ones(len(rowptr) - 1) if weights is None else np.asarray(weights)
    total, bar = LD(0), LD(0)
    for d in range(len(rowptr) - 1):
        sl = slice(rowptr[d], rowptr[d + 1])
        if w[d] == 0 or not (cts[sl] != 0).any():
            continue
        g = np.asarray(gamma[d], dtype=LD)
        Eg = expect(g)
        z = Eg + Elam[ids[sl]]
        m = z.max(1)
        terms = np.concatenate([cts[sl] * (m + np.log(np.exp(z - m[:, None]).sum(1))),
                                (alpha - g) * Eg, lgamma(g), -lgamma(alpha),
                                lgamma(alpha.sum()), -lgamma(g.sum())])
        total += LD(w[d]) * terms.sum()
        bar += LD(w[d]) * np.abs(terms).sum()
    return total, bar


class Step:
    """fit_online's step over host documents."""

    def __init__(self, rowptr, ids, cts, maxInner=100):
        self.csr, self.n, self.maxInner = (rowptr, ids, cts), len(rowptr) - 1, maxInner
        self.changes = []

    def estep(self, lam, alpha, gamma0, weights):
        r = estep(*self.csr, lam, alpha, gamma0, weights, self.maxInner)
        self.changes += r["changes"]
        return np.concatenate([r["stat"].ravel(), r["logphat"], [r["nonEmpty"]]]).astype(
            np.float64)
