"""Conformance tests of the device Silhouette (csrc/silhouette.hip through
cyc_kmeans_silhouette_stats_dev / _score_dev) at its chunk, column-loop, row
block, cluster tile, quarter, slice and total-fold edges.

The kernels run unfused fp64 in a fixed order, so every device bar here is
bit equality (NaN equal by position) against a numpy restatement that folds
in the device's order:

  statistics (stats_restate): a cluster's rows in row order cut into runs of
    256 (kChunkRows); a run summed from 0.0, term w * x (cosine: x * (1 /
    norm) first); the runs folded in order from 0.0; the result added to the
    incoming buffer.  A cluster without rows is not written.
  score (score_restate): per row the dot over j = 0 .. d - 1 from 0.0, the
    distance as the kernel writes it, the own / other split, Set.min as a
    reduceLeft keeping x when x <= y over the present clusters in cluster-id
    order, the coefficient, s * w; a 64-row block sums s w and w in row order
    (rows past n add 0.0); k_silh_total gives thread t the blocks [t per,
    (t + 1) per), per = ceil(blocks / 256), folds the 256 partials with a
    tree and adds the result to out.

test_host_cases pins the restatement to oracle.silhouette: bit for bit where
every cluster fits one run and the rows one block; otherwise the statistics
entry by entry within 2 m u sum|t| (both are folds of the same m correctly
rounded terms t, each within (m - 1) u sum|t| of the exact sum to first
order, Higham 4.2, as sum_bounds.check_entries derives; u = 2^-53), and the
score within the bound score_bound() derives the same way.  It also asserts
that every case reaches the edge it is named for.

The issue's edges that arithmetic does not reach:
  * a distance of -0.0: the squared Euclidean distance is (|x|^2 + psi / W)
    - 2 dot / W with |x|^2 = norm * norm >= +0.0, and a sum or difference of
    doubles is -0.0 only when both operands are (x - x is +0.0), likewise the
    cosine 1.0 - dot / W.  So two tied distances always carry the same bits,
    and the order of the fold shows only through NaN (x <= NaN is false, so
    the fold forgets everything before its last NaN).  The tie cases
    therefore pair equal finite distances, and pair NaNs, in one quarter,
    across quarters and across tiles.
"""
import functools

import numpy as np
import pytest

import oracle
from sum_bounds import U

gpu = pytest.mark.gpu
CHUNK = 256      # kChunkRows
SR = 64          # rows per workgroup of k_silh_score
SC = 64          # clusters per tile
MEASURES = (False, True)


def quiet():
    return np.errstate(all="ignore")


def mname(cosine):
    return "cosine" if cosine else "euclidean"


# -------------------------------------------------------------- restatement
def split(stats, k, d):
    return (stats[:k * d].reshape(k, d), stats[k * d:k * d + k], stats[k * d + k:k * d + 2 * k],
            stats[k * d + 2 * k:])


def stats_restate(X, xn, pred, w, k, cosine, prior=None):
    n, d = X.shape
    out = np.zeros(k * d + 3 * k) if prior is None else prior.copy()
    fs, psi, W, cnt = split(out, k, d)
    wt = np.ones(n) if w is None else w
    with quiet():
        for c in range(k):
            rows = np.flatnonzero(pred == c)
            if rows.size == 0:
                continue
            s, sw, sq = np.zeros(d), 0.0, 0.0
            for a in range(0, rows.size, CHUNK):
                ps, pw, pq = np.zeros(d), np.float64(0.0), np.float64(0.0)
                for r in rows[a:a + CHUNK]:
                    x = X[r] * (np.float64(1.0) / xn[r]) if cosine else X[r]
                    ps = ps + wt[r] * x
                    pw = pw + wt[r]
                    if not cosine:
                        pq = pq + (xn[r] * xn[r]) * wt[r]
                s, sw, sq = s + ps, sw + pw, sq + pq
            fs[c] = fs[c] + s
            psi[c] = psi[c] + sq
            W[c] = W[c] + sw
            cnt[c] = cnt[c] + float(rows.size)
    return out


def total_fold(parts):
    """k_silh_total over one column of block partials."""
    blocks = len(parts)
    per = (blocks + 255) // 256
    a = np.zeros(256)
    for t in range(256):
        s = np.float64(0.0)
        for i in range(t * per, min(blocks, (t + 1) * per)):
            s = s + parts[i]
        a[t] = s
    step = 128
    while step > 0:
        a[:step] = a[:step] + a[step:2 * step]
        step >>= 1
    return a[0], per


def score_restate(X, xn, pred, w, k, stats, cosine, prior=(0.0, 0.0)):
    """(out[2], per-row s w, per-row detail dict)."""
    n, d = X.shape
    fs, psi, W, cnt = split(np.asarray(stats, np.float64), k, d)
    wt = np.ones(n) if w is None else np.asarray(w, np.float64)
    with quiet():
        V = X * (1.0 / xn)[:, None] if cosine else X
        acc = np.zeros((n, k))
        for j in range(d):
            acc = acc + V[:, j, None] * fs[None, :, j]
        if cosine:
            dist = 1.0 - acc / W[None, :]
        else:
            dist = ((xn * xn)[:, None] + (psi / W)[None, :]) - (2.0 * acc) / W[None, :]
        nb, hb, cur = np.zeros(n), np.zeros(n, bool), np.zeros(n)
        who = np.full(n, -1)
        for c in range(k):
            if not cnt[c] > 0.0:
                continue
            own = pred == c
            cur = np.where(own, dist[:, c], cur)
            take = ~own & ~(hb & (nb <= dist[:, c]))
            nb = np.where(take, dist[:, c], nb)
            who = np.where(take, c, who)
            hb = hb | ~own
        Wo = W[pred]
        cd = (cur * Wo) / (Wo - wt)
        s = np.where(cd < nb, 1.0 - cd / nb, np.where(cd > nb, nb / cd - 1.0, 0.0))
        s = np.where(Wo == wt, 0.0, s)
        sw = s * wt
        blocks = (n + SR - 1) // SR
        S = np.zeros(blocks * SR)
        Wt = np.zeros(blocks * SR)
        S[:n], Wt[:n] = sw, wt
        S, Wt = S.reshape(blocks, SR), Wt.reshape(blocks, SR)
        pa, pb = np.zeros(blocks), np.zeros(blocks)
        for i in range(SR):
            pa, pb = pa + S[:, i], pb + Wt[:, i]
        ta, per = total_fold(pa)
        tb, _ = total_fold(pb)
        out = np.array([prior[0] + ta, prior[1] + tb])
    return out, sw, dict(dist=dist, nb=nb, who=who, cd=cd, cur=cur, s=s, per=per, blocks=blocks)


def same_bits(a, b):
    """Equal as int64 words, a NaN matching any NaN at the same position."""
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    na, nb_ = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb_) and \
        np.array_equal(a[~na].view(np.int64), b[~nb_].view(np.int64))


def first_diff(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    bad = np.flatnonzero(~((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))))
    return [(int(i), float(a[i]), float(b[i])) for i in bad[:5]]


# ------------------------------------------------------------ stats cases
SIZES = (0, 1, 255, 256, 257, 513)
D_STATS = (1, 255, 256, 257)
WEIGHTS = ("none", "positive", "zeros")


@functools.lru_cache(maxsize=None)
def stats_case(d, weights, cosine):
    """k = 7: clusters of 0, 1, 255, 256, 257 and 513 rows interleaved in a
    random row order, and cluster 6 with 5 rows that all weigh 0 under
    "zeros" (which also zeroes one row in sixteen elsewhere)."""
    rng = np.random.default_rng(100 * d + len(weights) + cosine)
    pred = np.repeat(np.arange(7), SIZES + (5,)).astype(np.int32)
    pred = pred[rng.permutation(len(pred))]
    n = len(pred)
    X = rng.normal(size=(n, d)) + pred[:, None]
    w = None
    if weights != "none":
        w = rng.uniform(0.25, 3.0, n)
        if weights == "zeros":
            w[rng.random(n) < 1 / 16] = 0.0
            w[pred == 6] = 0.0
    return X, oracle.row_norms(X), pred, w, 7


@functools.lru_cache(maxsize=None)
def one_cluster_case(cosine):
    rng = np.random.default_rng(11 + cosine)
    X = rng.normal(size=(300, 3))
    return X, oracle.row_norms(X), np.zeros(300, np.int32), rng.uniform(0.5, 2.0, 300), 1


@functools.lru_cache(maxsize=None)
def zero_row_case():
    """Cosine with an all-zero row in cluster 1: its norm is 0, 1 / norm is
    Inf and 0 * Inf is NaN in that cluster's feature sum; the row's own
    coefficient and everybody's distance to cluster 1 follow."""
    rng = np.random.default_rng(12)
    X = rng.normal(size=(70, 3))
    pred = (np.arange(70) % 3).astype(np.int32)
    X[4] = 0.0
    return X, oracle.row_norms(X), pred, None, 3


# ------------------------------------------------------------ score cases
@functools.lru_cache(maxsize=None)
def population_stats(k, d, cosine, absent=()):
    """Statistics of a random population of 5 rows per present cluster with
    weights in (1, 2) (so no W is 0 or 1), around centers 6 apart."""
    rng = np.random.default_rng(1000 * k + 10 * d + cosine)
    C = rng.normal(size=(k, d)) * 6.0
    present = np.array([c for c in range(k) if c not in absent])
    pred = np.repeat(present, 5).astype(np.int32)
    X = C[pred] + rng.normal(size=(len(pred), d))
    st = stats_restate(X, oracle.row_norms(X), pred, rng.uniform(1.0, 2.0, len(pred)), k, cosine)
    return C, st, present


@functools.lru_cache(maxsize=None)
def shape_case(n, d, k, cosine, weighted=True):
    """n random rows scored against population_stats(k, d); for k > 4 every
    fifth cluster is absent (empty clusters interleaved with present ones);
    every eighth row weighs 0."""
    absent = tuple(range(2, k, 5)) if k > 4 else ()
    C, st, present = population_stats(k, d, cosine, absent)
    rng = np.random.default_rng(n + 7 * d + 13 * k + cosine)
    pred = present[rng.integers(0, len(present), size=n)].astype(np.int32)
    X = C[pred] + rng.normal(size=(n, d)) * 2.0
    w = None
    if weighted:
        w = rng.uniform(0.25, 3.0, n)
        w[::8] = 0.0
    return X, oracle.row_norms(X), pred, w, k, st


N_ROWS = (1, 63, 64, 65, 129)
BLOCKS = (255, 256, 257, 513)
D_SCORE = (1, 15, 16, 17, 33)
K_SCORE = (2, 15, 16, 17, 63, 64, 65, 129)

K_DIRECT = 192       # three cluster tiles


def direct_case(cosine, k, own, t, absent=(), W=None, w=1.0):
    """One row x = [1.0] whose distance to cluster c is exactly t[c]: with
    W = 2, cosine dist = 1 - fs / W with fs = (1 - t) W, Euclidean dist =
    (1 + psi / W) - 2 fs / W with fs = 1 and psi = 2 t; t defaults to
    8 + (c % 7) / 8, all dyadic, so every operation is exact.  A NaN t puts
    NaN in fs / psi.  W overrides some weight sums afterwards (the sums stay
    as built for W = 2)."""
    tt = 8.0 + (np.arange(k) % 7) / 8.0
    for c, v in t.items():
        tt[c] = v
    Wv = np.full(k, 2.0)
    cnt = np.array([0.0 if c in absent else 5.0 for c in range(k)])
    fs = (1.0 - tt) * Wv if cosine else np.ones(k)
    psi = np.zeros(k) if cosine else 2.0 * tt
    for c, v in (W or {}).items():
        Wv[c] = v
    st = np.concatenate([fs, psi, Wv, cnt])
    X = np.ones((1, 1))
    return X, np.ones(1), np.array([own], np.int32), np.array([w]), k, st


# name -> (k, own, t, extra kwargs, what the restatement must show)
NAN = float("nan")
DIRECT = {
    # ties of equal finite distances; the lower id is kept
    "tie in one quarter": (K_DIRECT, 40, {40: 0.125, 3: 0.5, 5: 0.5}, {},
                           dict(who=3, nb=0.5, branch="lt")),
    "tie across quarters": (K_DIRECT, 40, {40: 0.125, 3: 0.5, 20: 0.5}, {},
                            dict(who=3, nb=0.5, branch="lt")),
    "tie across tiles": (K_DIRECT, 40, {40: 0.125, 20: 0.5, 70: 0.5}, {},
                         dict(who=20, nb=0.5, branch="lt")),
    # cd = cur W / (W - w) = 2 cur
    "cd == nb": (K_DIRECT, 40, {40: 0.25, 7: 0.5}, {}, dict(who=7, nb=0.5, branch="eq")),
    "cd > nb": (K_DIRECT, 40, {40: 1.0, 7: 0.5}, {}, dict(who=7, nb=0.5, branch="gt")),
    # the own cluster in every quarter of a tile, the nearest in the last
    "own in quarter 0": (K_DIRECT, 3, {3: 0.125, 60: 0.5}, {}, dict(who=60, branch="lt")),
    "own in quarter 1": (K_DIRECT, 19, {19: 0.125, 60: 0.5}, {}, dict(who=60, branch="lt")),
    "own in quarter 2": (K_DIRECT, 35, {35: 0.125, 60: 0.5}, {}, dict(who=60, branch="lt")),
    "own in quarter 3": (K_DIRECT, 51, {51: 0.125, 5: 0.5}, {}, dict(who=5, branch="lt")),
    # own and nearest in different tiles, both ways
    "own in tile 1, nearest in tile 0": (K_DIRECT, 70, {70: 0.125, 5: 0.5}, {},
                                         dict(who=5, branch="lt")),
    "own in tile 2, nearest in tile 0": (K_DIRECT, 140, {140: 0.125, 5: 0.5}, {},
                                         dict(who=5, branch="lt")),
    "own in tile 0, nearest in tile 1": (K_DIRECT, 5, {5: 0.125, 70: 0.5}, {},
                                         dict(who=70, branch="lt")),
    "own in tile 0, nearest in tile 2": (K_DIRECT, 5, {5: 0.125, 140: 0.5}, {},
                                         dict(who=140, branch="lt")),
    # NaN: the fold forgets what came before its last NaN (0.25 at id 1 / 3)
    "NaN in one quarter": (K_DIRECT, 40, {40: 0.125, 1: 0.25, 3: NAN, 5: 0.5}, {},
                           dict(who=5, nb=0.5, branch="lt")),
    "NaN across quarters": (K_DIRECT, 40, {40: 0.125, 3: 0.25, 20: NAN, 50: 0.5}, {},
                            dict(who=50, nb=0.5, branch="lt")),
    "NaN across tiles": (K_DIRECT, 40, {40: 0.125, 3: 0.25, 70: NAN, 100: 0.5}, {},
                         dict(who=100, nb=0.5, branch="lt")),
    "NaN pair across tiles": (K_DIRECT, 40, {40: 0.125, 3: NAN, 30: 0.25, 70: NAN, 100: 0.5}, {},
                              dict(who=100, nb=0.5, branch="lt")),
    "NaN at the last cluster": (65, 40, {40: 0.125, 3: 0.25, 64: NAN}, {},
                                dict(who=64, nb=NAN, branch="eq")),
    # Set.min never sees an absent cluster, however near its stale entries
    "absent clusters nearest": (K_DIRECT, 40, {40: 0.125, 3: 0.0, 70: 0.0, 100: 0.5},
                                dict(absent=(3, 70) + tuple(range(1, K_DIRECT, 2))),
                                dict(who=100, nb=0.5, branch="lt")),
    # single-element clusters: W[own] == w
    "W[own] == w": (K_DIRECT, 40, {40: 0.125, 7: 0.5}, dict(W={40: 1.0}), dict(branch="single")),
    "W[own] == w == 0": (K_DIRECT, 40, {40: 0.125, 7: 0.5}, dict(W={40: 0.0}, w=0.0),
                         dict(branch="single")),
    # a cluster with rows but weight 0: a division by zero
    "W[c] == 0": (K_DIRECT, 40, {40: 0.125, 7: 0.5, 9: -0.5}, dict(W={9: 0.0}),
                  dict(who=9, nb=-np.inf, zero_w=9)),
}


@functools.lru_cache(maxsize=None)
def isolation_case(cosine):
    """64 rows (one block) against population_stats(5, 4)."""
    return shape_case(64, 4, 5, cosine, weighted=False)


# ------------------------------------------------------------- host checks
def score_bound(sw, w, score):
    """|num / den| of two folds of the same n terms each: num and den are
    each within n u sum|t| of their exact sums for either order (the module
    docstring), so they differ by at most 2 n u sum|t|; the quotient moves by
    (dnum + |score| dden) / den to first order, and its own rounding, in
    both, adds 2 u |score|."""
    n = len(sw)
    dnum = 2 * n * U * np.abs(sw).sum()
    dden = 2 * n * U * np.abs(w).sum()
    return (dnum + abs(score) * dden) / np.abs(w).sum() + 2 * U * abs(score)


def _pin_small(cosine, weighted):
    """One run per cluster, one block of rows: bit for bit."""
    rng = np.random.default_rng(50 + cosine + 2 * weighted)
    n, d, k = 60, 5, 4
    pred = rng.integers(0, 3, size=n).astype(np.int32)        # cluster 3 empty
    X = rng.normal(size=(n, d)) + 3.0 * pred[:, None]
    w = rng.uniform(0.25, 3.0, n) if weighted else None
    if weighted:
        w[5] = 0.0
    xn = oracle.row_norms(X)
    s_ref, st_ref = oracle.silhouette(X, pred, k, w, cosine=cosine)
    st = stats_restate(X, xn, pred, w, k, cosine)
    assert same_bits(st, st_ref), first_diff(st, st_ref)
    out, _, _ = score_restate(X, xn, pred, w, k, st, cosine)
    assert out[0] / out[1] == s_ref


def _pin_large(cosine):
    """Clusters of several runs, several blocks: within the derived bounds."""
    X, xn, pred, w, k = stats_case(17 if cosine else 1, "positive", cosine)
    n, d = X.shape
    s_ref, st_ref = oracle.silhouette(X, pred, k, w, cosine=cosine)
    st = stats_restate(X, xn, pred, w, k, cosine)
    V = X / xn[:, None] if cosine else X
    for c in range(k):
        rows = pred == c
        m = int(rows.sum())
        mag = np.abs(w[rows, None] * V[rows]).sum(axis=0)
        # cosine: x * (1 / norm) against the oracle's (1 / norm) * x is the
        # same product; the terms are bit-identical
        assert (np.abs(split(st, k, d)[0][c] - split(st_ref, k, d)[0][c]) <= 2 * m * U * mag).all()
        for f in (1, 2):
            tm = (xn[rows] ** 2 * w[rows]) if f == 1 else w[rows]
            assert abs(split(st, k, d)[f][c] - split(st_ref, k, d)[f][c]) <= 2 * m * U * tm.sum()
    assert np.array_equal(split(st, k, d)[3], split(st_ref, k, d)[3])
    # the score's summation order alone: rows of one block per cluster run
    X, xn, pred, w, k, _ = shape_case(129, 4, 3, cosine)
    s_ref, st_ref = oracle.silhouette(X, pred, k, w, cosine=cosine)
    st = stats_restate(X, xn, pred, w, k, cosine)
    assert same_bits(st, st_ref)
    out, sw, _ = score_restate(X, xn, pred, w, k, st, cosine)
    assert abs(out[0] / out[1] - s_ref) <= score_bound(sw, w, s_ref)


def check_direct(name, cosine):
    k, own, t, kw, want = DIRECT[name]
    X, xn, pred, w, k, st = direct_case(cosine, k, own, t, **kw)
    out, sw, det = score_restate(X, xn, pred, w, k, st, cosine)
    dist = det["dist"][0]
    cnt = split(st, k, 1)[3]
    for c, v in t.items():
        if c in kw.get("absent", ()) or split(st, k, 1)[2][c] != 2.0:
            continue
        assert dist[c] == v or (np.isnan(v) and np.isnan(dist[c])), (name, c, dist[c])
    branch = want.get("branch")
    if branch == "single":
        assert split(st, k, 1)[2][own] == w[0] and sw[0] == 0.0
        return
    if "who" in want:
        assert det["who"][0] == want["who"], (name, det["who"][0])
    if "nb" in want:
        assert same_bits(det["nb"][0], want["nb"]), (name, det["nb"][0])
    cd, nb = det["cd"][0], det["nb"][0]
    if branch == "lt":
        assert cd < nb and det["s"][0] == 1.0 - cd / nb
    elif branch == "gt":
        assert cd > nb and det["s"][0] == nb / cd - 1.0
    elif branch == "eq":
        assert not cd < nb and not cd > nb and det["s"][0] == 0.0
        assert cd == nb or np.isnan(nb)
    if "zero_w" in want:
        c = want["zero_w"]
        assert cnt[c] > 0 and split(st, k, 1)[2][c] == 0.0 and not np.isfinite(dist[c])
        assert not np.isfinite(out[0])
    if name.startswith("tie"):
        ids = [c for c, v in t.items() if v == 0.5]
        assert len(ids) == 2 and dist[ids[0]] == dist[ids[1]] == nb and det["who"][0] == min(ids)
    if name.startswith("NaN"):
        # the forgotten 0.25 sits before the last NaN and is below the result
        last = max(c for c, v in t.items() if np.isnan(v))
        assert any(v == 0.25 and c < last for c, v in t.items())
    if "absent" in kw:
        assert all(not cnt[c] > 0 and dist[c] == 0.0 for c in (3, 70))


def test_host_cases():
    for cosine in MEASURES:
        for weighted in (False, True):
            _pin_small(cosine, weighted)
        _pin_large(cosine)
        # statistics: cluster sizes, weights
        for d in D_STATS:
            for weights in WEIGHTS:
                X, xn, pred, w, k = stats_case(d, weights, cosine)
                assert X.shape[1] == d
                assert tuple(np.bincount(pred, minlength=7)[:6]) == SIZES
                if weights == "zeros":
                    assert (w == 0).sum() > 5 and not w[pred == 6].any()
                    st = stats_restate(X, xn, pred, w, k, cosine)
                    assert split(st, k, d)[2][6] == 0.0 and split(st, k, d)[3][6] == 5.0
        assert one_cluster_case(cosine)[4] == 1
        # score shapes
        for n in N_ROWS:
            assert shape_case(n, 4, 3, cosine)[0].shape == (n, 4)
        for b in BLOCKS:
            X, xn, pred, w, k, st = shape_case(b * SR - 5, 2, 2, cosine)
            _, _, det = score_restate(X, xn, pred, w, k, st, cosine)
            assert det["blocks"] == b and det["per"] == (1 if b <= 256 else 2 if b <= 512 else 3)
        for k in K_SCORE:
            X, xn, pred, w, k_, st = shape_case(70, 3, k, cosine)
            cnt = split(st, k, 3)[3]
            assert k_ == k and (cnt > 0).sum() >= 2
            if k > 4:       # empty clusters interleaved
                assert not cnt[2] > 0 and cnt[1] > 0 and cnt[3] > 0
            _, _, det = score_restate(X, xn, pred, w, k, st, cosine)
            assert {"lt", "gt"} <= {"lt" if a < b else "gt" for a, b in zip(det["cd"], det["nb"])
                                    } or k < 15
        for name in DIRECT:
            check_direct(name, cosine)
        # per-row isolation: the one-hot weight reads the row's coefficient
        X, xn, pred, _, k, st = isolation_case(cosine)
        _, _, full = score_restate(X, xn, pred, None, k, st, cosine)
        Wv = split(st, k, 4)[2][np.unique(pred)]
        assert not np.isin(Wv, (0.0, 1.0)).any()
        for r in (0, 17, 63):
            w = np.zeros(64)
            w[r] = 1.0
            out, _, det = score_restate(X, xn, pred, w, k, st, cosine)
            assert out[1] == 1.0 and out[0] == det["s"][r] and np.isfinite(out[0])
            assert det["nb"][r] == full["nb"][r]
    # 257 blocks: per == 2
    assert total_fold(np.ones(257))[1] == 2
    X, xn, pred, w, k = zero_row_case()
    assert xn[4] == 0.0
    st = stats_restate(X, xn, pred, w, k, True)
    assert np.isnan(split(st, k, 3)[0][1]).all() and not np.isnan(split(st, k, 3)[0][0]).any()
    out, sw, det = score_restate(X, xn, pred, w, k, st, True)
    assert np.isnan(det["dist"][:, 1]).all() and np.isnan(det["dist"][4]).all()


# ------------------------------------------------------------------- device
def _dev(cuda, *arrs):
    import torch
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
            for a in arrs]


def _plan(k, d, n, cosine):
    from cycloneml_amd.clustering import KMeansPlan
    return KMeansPlan(d, k, max(n, 1), distanceMeasure="cosine" if cosine else "euclidean")


def dev_stats(cuda, X, xn, pred, w, k, cosine, prior=None, calls=1):
    import torch
    from cycloneml_amd import _native as N
    n, d = X.shape
    Xd, xnd, pd, wd = _dev(cuda, X, xn, pred, w)
    st = torch.zeros(k * d + 3 * k, dtype=torch.float64, device=cuda) if prior is None \
        else _dev(cuda, prior)[0]
    plan = _plan(k, d, n, cosine)
    try:
        for _ in range(calls):
            N.check(N.load().cyc_kmeans_silhouette_stats_dev(
                plan.handle, N.ptr(Xd), N.ptr(xnd), n, N.ptr(pd), N.ptr(wd), N.ptr(st), None))
        torch.cuda.synchronize()
        return st.cpu().numpy()
    finally:
        plan.close()


def dev_score(cuda, X, xn, pred, w, k, st, cosine, prior=(0.0, 0.0), plan=None, xnd=None):
    import torch
    from cycloneml_amd import _native as N
    n, d = X.shape
    Xd, pd, wd, std, out = _dev(cuda, X, pred, w, st, np.array(prior, np.float64))
    if xnd is None and xn is not None:
        xnd = _dev(cuda, xn)[0]
    mine = plan is None
    plan = plan or _plan(k, d, n, cosine)
    try:
        N.check(N.load().cyc_kmeans_silhouette_score_dev(
            plan.handle, N.ptr(Xd), N.ptr(xnd), n, N.ptr(pd), N.ptr(wd), N.ptr(std), N.ptr(out),
            None))
        torch.cuda.synchronize()
        return out.cpu().numpy()
    finally:
        if mine:
            plan.close()


def check_score(cuda, case, cosine, what, prior=(0.0, 0.0)):
    X, xn, pred, w, k, st = case
    ref, _, _ = score_restate(X, xn, pred, w, k, st, cosine, prior)
    got = dev_score(cuda, X, xn, pred, w, k, st, cosine, prior)
    print(what, mname(cosine), "device", got, "restatement", ref)
    assert same_bits(got, ref), (what, mname(cosine), got, ref)


@gpu
@pytest.mark.parametrize("cosine", MEASURES, ids=mname)
@pytest.mark.parametrize("weights", WEIGHTS)
@pytest.mark.parametrize("d", D_STATS)
def test_stats_cluster_sizes(cuda, d, weights, cosine):
    X, xn, pred, w, k = stats_case(d, weights, cosine)
    ref = stats_restate(X, xn, pred, w, k, cosine)
    got = dev_stats(cuda, X, xn, pred, w, k, cosine)
    assert same_bits(got, ref), first_diff(got, ref)


@gpu
@pytest.mark.parametrize("cosine", MEASURES, ids=mname)
def test_stats_two_calls_into_one_buffer(cuda, cosine):
    """The fold adds to what the buffer holds: a random prior, two calls."""
    X, xn, pred, w, k = stats_case(257, "zeros", cosine)
    prior = np.random.default_rng(3).normal(size=k * 257 + 3 * k)
    ref = stats_restate(X, xn, pred, w, k, cosine,
                        stats_restate(X, xn, pred, w, k, cosine, prior))
    got = dev_stats(cuda, X, xn, pred, w, k, cosine, prior, calls=2)
    assert same_bits(got, ref), first_diff(got, ref)
    untouched = np.r_[0:257, 7 * 257, 7 * 257 + 7, 7 * 257 + 14]      # cluster 0 has no rows
    assert same_bits(got[untouched], prior[untouched])


@gpu
@pytest.mark.parametrize("cosine", MEASURES, ids=mname)
def test_stats_one_cluster(cuda, cosine):
    X, xn, pred, w, k = one_cluster_case(cosine)
    ref = stats_restate(X, xn, pred, w, k, cosine)
    got = dev_stats(cuda, X, xn, pred, w, k, cosine)
    assert same_bits(got, ref), first_diff(got, ref)


@gpu
def test_cosine_zero_row(cuda):
    X, xn, pred, w, k = zero_row_case()
    ref = stats_restate(X, xn, pred, w, k, True)
    got = dev_stats(cuda, X, xn, pred, w, k, True)
    assert same_bits(got, ref), first_diff(got, ref)
    check_score(cuda, (X, xn, pred, w, k, ref), True, "zero row")


@gpu
@pytest.mark.parametrize("cosine", MEASURES, ids=mname)
def test_norms_computed_by_the_call(cuda, cosine):
    """xnorm = None equals the call that is given cyc_row_norms_dev's output."""
    from cycloneml_amd.clustering import row_norms
    X, _, pred, w, k = stats_case(17, "positive", cosine)
    xnd = row_norms(_dev(cuda, X)[0])
    xn = xnd.cpu().numpy()
    a = dev_stats(cuda, X, None, pred, w, k, cosine)
    b = dev_stats(cuda, X, xn, pred, w, k, cosine)
    assert same_bits(a, b), first_diff(a, b)
    assert same_bits(b, stats_restate(X, xn, pred, w, k, cosine))
    X, _, pred, w, k, st = shape_case(129, 4, 3, cosine)
    xn = row_norms(_dev(cuda, X)[0]).cpu().numpy()
    a = dev_score(cuda, X, None, pred, w, k, st, cosine)
    b = dev_score(cuda, X, xn, pred, w, k, st, cosine)
    assert same_bits(a, b), (a, b)


@gpu
@pytest.mark.parametrize("cosine", MEASURES, ids=mname)
@pytest.mark.parametrize("n", N_ROWS)
def test_score_rows(cuda, n, cosine):
    check_score(cuda, shape_case(n, 4, 3, cosine), cosine, f"n={n}")
    check_score(cuda, shape_case(n, 4, 3, cosine, weighted=False), cosine, f"n={n} unweighted",
                prior=(0.375, 2.5))


@gpu
@pytest.mark.parametrize("cosine", MEASURES, ids=mname)
@pytest.mark.parametrize("blocks", BLOCKS)
def test_score_block_counts(cuda, blocks, cosine):
    check_score(cuda, shape_case(blocks * SR - 5, 2, 2, cosine), cosine, f"blocks={blocks}")


@gpu
@pytest.mark.parametrize("cosine", MEASURES, ids=mname)
@pytest.mark.parametrize("d", D_SCORE)
def test_score_slices(cuda, d, cosine):
    check_score(cuda, shape_case(70, d, 5, cosine), cosine, f"d={d}")


@gpu
@pytest.mark.parametrize("cosine", MEASURES, ids=mname)
@pytest.mark.parametrize("k", K_SCORE)
def test_score_cluster_tiles(cuda, k, cosine):
    check_score(cuda, shape_case(70, 3, k, cosine), cosine, f"k={k}")


@gpu
@pytest.mark.parametrize("cosine", MEASURES, ids=mname)
@pytest.mark.parametrize("name", list(DIRECT))
def test_score_placement_ties_and_branches(cuda, name, cosine):
    k, own, t, kw, _ = DIRECT[name]
    check_score(cuda, direct_case(cosine, k, own, t, **kw), cosine, name)


@gpu
@pytest.mark.parametrize("cosine", MEASURES, ids=mname)
def test_score_every_row_alone(cuda, cosine):
    """The same 64 rows scored once per position r with weight 1 on row r and
    0 elsewhere: out[0] is row r's coefficient, out[1] is 1."""
    X, xn, pred, _, k, st = isolation_case(cosine)
    xnd = _dev(cuda, xn)[0]
    plan = _plan(k, 4, 64, cosine)
    try:
        bad = []
        for r in range(64):
            w = np.zeros(64)
            w[r] = 1.0
            ref, _, _ = score_restate(X, xn, pred, w, k, st, cosine)
            got = dev_score(cuda, X, xn, pred, w, k, st, cosine, plan=plan, xnd=xnd)
            if not same_bits(got, ref):
                bad.append((r, got.tolist(), ref.tolist()))
        assert not bad, bad[:4]
    finally:
        plan.close()


@gpu
@pytest.mark.parametrize("cosine", MEASURES, ids=mname)
def test_error_paths(cuda, cosine):
    from cycloneml_amd import _native as N
    X, xn, pred, w, k, st = shape_case(65, 4, 3, cosine)
    w = np.ones(65)

    def both(match, exc, pred=pred, w=w, st=st):
        with pytest.raises(exc, match=match):
            dev_score(cuda, X, xn, pred, w, k, st, cosine)
        if exc is N.IllegalArgumentException:
            with pytest.raises(exc, match=match):
                dev_stats(cuda, X, xn, pred, w, k, cosine)

    bad = pred.copy()
    bad[64] = k
    both(r"requirement failed: predictions must lie in \[0, k\) for k = 3",
         N.IllegalArgumentException, pred=bad)
    bad = pred.copy()
    bad[0] = -1
    both(r"requirement failed: predictions must lie in \[0, k\) for k = 3",
         N.IllegalArgumentException, pred=bad)
    # the lowest offending row is the one reported
    bw = w.copy()
    bw[[9, 64]] = [np.nan, -1.0]
    both(r"requirement failed: illegal weight value: NaN\. weight must be >= 0\.0\.",
         N.IllegalArgumentException, w=bw)
    bw[[9, 64]] = [-1.0, np.nan]
    both(r"requirement failed: illegal weight value: -1\.0\. weight must be >= 0\.0\.",
         N.IllegalArgumentException, w=bw)
    one = st.copy()
    split(one, k, 4)[3][1:] = 0.0
    both("assertion failed: Number of clusters must be greater than one.",
         N.JavaAssertionError, st=one)
