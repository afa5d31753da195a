"""Conformance tests of KMeans with the cosine measure (KMeansPlan(...,
"cosine"): stats / assign / point_cost / accumulate / update and the CSR
entry points) at the tile, wave, chunk and norm edges of kmeans_cos.hip and
the cos_* glue of kmeans.hip, at the smallest shapes that reach them.

Bars (all derived, none measured):
  * packed statistics, diagonal included: array_equal(equal_nan=True) against
    oracle.cos_stats (k_cos_stats_pairs runs the reference's sequential ddot
    and the same divisions and sqrt; the diagonal is a minimum, which has no
    rounding);
  * assignments and per-row costs, every row: array_equal against
    oracle.cos_kmeans_partition (with statistics) and oracle.cos_point_costs
    (without), the _sparse forms for CSR (the kernels restate the reference
    loop's operation order: kmeans_cos.hip, the comment above
    k_cos_assign_exact);
  * wsum with unit weights: bit-exact (counts are exact integers);
  * sums, weighted wsum and the cost sum: entry by entry within the bound
    that check_entries (sum_bounds.py) derives from that entry's terms alone,
    m * 2**-53 * sum|t|.  The terms (terms() below) are built as
    k_cos_chunk_sums builds them: sums fold (w_r / |x_r|) * x_rj with the
    rows of coefficient 0 dropped (netlib daxpy returns on a zero a), the
    cost sum folds cost_r * w_r;
  * update after accumulate: centers, cnorm and the convergence flag
    bit-exact, NaN positions included, against oracle.cos_update_centers fed
    the device's own sums and weights (both run the same sequential
    recurrence);
  * a second identical call on a fresh plan: every output bit-equal (compared
    as int64 words where an output holds NaN).

Every case is built on the host by a cached function that also asserts, on
the reference alone, that its inputs reach the edge it is about (replay()
restates the reference loop with a trace of its visits, and is itself held
to oracle.cos_find_closest_stats); host_cases() lists them and
test_host_cases walks them without a device.

Edges of the issue's list that arithmetic does not reach, with what is
pinned in their place:
  * a NaN statistic needs 1 - dot / |ci| / |cj| > 2.  For c and -c (or
    -2^m c) the dot is the very sum the norms are the root of, and the three
    roundings of sum / sqrt(sum) / sqrt(sum) do not carry the quotient to
    1 + 2^-51 in magnitude, which is what the subtraction needs to leave 2.0
    (3000 seeds per width gave none).  The pair used is c and -3c with the
    coordinates of c rounded to 50 bits, so that -3c is exact and the pair is
    exactly antipodal as real vectors while its three sums round apart;
    seeds are searched until the oracle gives the NaN.  At d = 1 the
    search finds none in 4000 seeds, and the d = 1 pair pins what the
    oracle gives instead;
  * a negative statistic likewise needs a scaled copy (3c, 1.7c, 0.3c): an
    exact duplicate gives 0.0 at most;
  * at d = 1 there are two directions only, so nine cluster sizes cannot be
    told apart: the d = 1 sums case has k = 2 with 513 and 257 rows; the
    nine sizes are at d = 255, 256 and 257;
  * statistics that prune every later center need k >= 3 (one pair's
    statistic is the diagonal of both, so the visit of center 1 is never
    pruned without an early return at center 0).
"""
import functools

import numpy as np
import pytest

import oracle
from sum_bounds import U, check_entries
import test_kmeans_sparse_conformance as S

gpu = pytest.mark.gpu
ASSERT_TEXT = "assertion failed: Cosine distance is not defined for zero-length"


# --------------------------------------------------------------------- host
def iut(i, j):
    i, j = min(i, j), max(i, j)
    return j * (j + 1) // 2 + i


def cdist(c, cn, x, xn):
    """distance(center, point) = 1 - ddot / |c| / |x| (DistanceMeasure.scala:453-456)."""
    dot = oracle.lib().orc_ddot(oracle._p(np.ascontiguousarray(c)),
                                oracle._p(np.ascontiguousarray(x)), len(x))
    return 1.0 - dot / float(cn) / float(xn)


def replay(C, cn, st, x, xn):
    """CosineDistanceMeasure.findClosest with statistics (:421-447) with a
    trace: per center 'skip' (pruned), 'visit', 'best' (a new best) or
    'return' (the early return); the result equals the oracle's."""
    k = C.shape[0]
    best, bi = cdist(C[0], cn[0], x, xn), 0
    trace = ["best"]
    done = best < st[0]
    if done:
        trace[0] = "return"
    for i in range(1, k):
        if done:
            break
        if not st[iut(i, bi)] < best:
            trace.append("skip")
            continue
        dd = cdist(C[i], cn[i], x, xn)
        if dd < st[iut(i, i)]:
            best, bi, done = dd, i, True
            trace.append("return")
        elif dd < best:
            best, bi = dd, i
            trace.append("best")
        else:
            trace.append("visit")
    assert (bi, best) == oracle.cos_find_closest_stats(C, cn, st, x, xn)
    return bi, best, trace


class Ref:
    """The oracle's cosine Lloyd call for (X, C): findClosest with the
    statistics (a, c, sums, wsum, cost) and without (na, nc).  cn: the given
    center norms (the computed ones by default); stats_cn: the norms the
    statistics are built from (plan.stats computes its own; accumulate uses
    the given ones)."""

    def __init__(self, X, C, w=None, cn=None, stats_cn=None):
        self.xn = oracle.row_norms(X)
        self.cn = oracle.row_norms(C) if cn is None else cn
        self.stats = oracle.cos_stats(C, self.cn if stats_cn is None else stats_cn)
        self.a, self.c, self.sums, self.wsum, self.cost = oracle.cos_kmeans_partition(
            X, self.xn, w, C, self.cn, self.stats)
        self.na, self.nc, _ = oracle.cos_point_costs(X, self.xn, C, self.cn)


def terms(X, w, ref):
    """The terms the device folds into (sums, wsum, cost sum), as (entry
    index, term) arrays; see the module docstring."""
    n, d = X.shape
    a64 = ref.a.astype(np.int64)
    wr = np.ones(n) if w is None else np.asarray(w, np.float64)
    coef = wr / ref.xn
    keep = coef != 0.0
    keys = (a64[keep, None] * d + np.arange(d)[None, :]).ravel()
    t = (coef[keep, None] * X[keep]).ravel()
    return (keys, t), (a64, wr), (np.zeros(n, np.int64), ref.c * wr)


# ---- statistics
K_STATS = (1, 2, 16, 17, 31, 32, 33, 63, 64, 65, 97)
D_STATS = (1, 2, 31, 32, 33, 65)
STATS_CONTENT = ((33, 33), (65, 31), (17, 65), (97, 32))


@functools.lru_cache(maxsize=None)
def stats_case(k, d):
    """Random centers of mixed magnitude."""
    rng = np.random.default_rng(1000 * k + d)
    C = rng.normal(size=(k, d)) * rng.uniform(0.1, 10.0, size=(k, 1))
    st = oracle.cos_stats(C, oracle.row_norms(C))
    if k == 1:
        assert st.shape == (1,) and np.isnan(st[0])
    else:
        for i in range(k):
            row = [st[iut(i, j)] for j in range(k) if j != i]
            assert st[iut(i, i)] == np.nanmin(row)
    return C, st


@functools.lru_cache(maxsize=None)
def antipode(d):
    """c with 50-bit coordinates (-3c is exact) for which the oracle's
    statistic of (c, -3c) is NaN; d = 1 has none (module docstring)."""
    for seed in range(4000):
        rng = np.random.default_rng(seed)
        m, e = np.frexp(rng.normal(size=d) * rng.uniform(0.5, 4.0))
        c = np.ldexp(np.round(np.ldexp(m, 50)), e - 50)
        C = np.vstack([c, -3.0 * c])
        assert np.array_equal(C[1] / -3.0, c)
        st = oracle.cos_stats(C, oracle.row_norms(C))
        if np.isnan(st[1]):
            return c, True
    assert d == 1, f"no NaN statistic at d = {d}"
    return c, False


@functools.lru_cache(maxsize=None)
def stats_pair_case(d):
    """k = 2 with the antipodal pair: both diagonal entries +Infinity
    (`if (s < diag)` never keeps a NaN); at d = 1 no NaN, whatever the
    oracle gives."""
    c, nan = antipode(d)
    C = np.vstack([c, -3.0 * c])
    st = oracle.cos_stats(C, oracle.row_norms(C))
    if nan:
        assert np.isposinf(st[0]) and np.isnan(st[1]) and np.isposinf(st[2])
    return C, st


@functools.lru_cache(maxsize=None)
def stats_content_case(k, d):
    """Random centers, then: center k - 1 an exact duplicate of center 0;
    centers 2, 3, 4 the copies 3.0, 1.7 and 0.3 times center 1; center 6 the
    antipode -3 x center 5 (50-bit coordinates).  Seeds are searched until the
    oracle gives a negative statistic; then the minimum is negative and lies
    on the diagonal (as well as off it), and a NaN lies off the diagonal,
    and no diagonal entry is NaN."""
    c5, nan = antipode(d)
    assert nan
    for seed in range(4000):
        rng = np.random.default_rng(7 * k + d + 10000 * seed)
        C = rng.normal(size=(k, d)) * rng.uniform(0.1, 10.0, size=(k, 1))
        C[k - 1] = C[0]
        C[2], C[3], C[4] = 3.0 * C[1], 1.7 * C[1], 0.3 * C[1]
        C[5], C[6] = c5, -3.0 * c5
        st = oracle.cos_stats(C, oracle.row_norms(C))
        if np.nanmin(st) < 0:
            break
    else:
        raise AssertionError("no negative statistic")
    diag = np.array([st[iut(i, i)] for i in range(k)])
    assert np.nanmin(st) < 0 and np.min(diag) == np.nanmin(st)
    assert np.isnan(st[iut(5, 6)]) and not np.isnan(diag).any()
    return C, st


# ---- the reference loop
K_LOOP = (1, 2, 64, 65, 66, 128, 129, 130)
D_LOOP = (3, 4, 5, 33)


def _plane(rng, d):
    """Two orthonormal directions of R^d (a random plane)."""
    Q, _ = np.linalg.qr(rng.normal(size=(d, 2)))
    return Q[:, 0], Q[:, 1]


def _at(theta, e0, e1, scale):
    theta = np.atleast_1d(np.asarray(theta, np.float64))
    return (np.cos(theta)[:, None] * e0 + np.sin(theta)[:, None] * e1) * \
        np.broadcast_to(scale, theta.shape)[:, None]


@functools.lru_cache(maxsize=None)
def fan_case(k, d):
    """Centers in a plane at angles (k - i) * delta, i = 0 .. k - 1, with the
    statistic of neighbours 1 - cos(delta / 2).  Rows, by replay():
      * 'climb', at angle 0: every center 1 .. k - 1 is a new best (for
        k >= 65 a new best at each of the 64 lanes of a group) and no visit
        returns early;
      * 'ret m', 0.1 delta inside center m, for m in {0, 1, 64, 65, k - 1}
        below k: new bests up to m - 1, then `dd < s(m, m)` returns at m: at
        center 0, the first lane, the last lane, the first lane of the second
        group;
      * eight rows at random angles of the plane and eight random rows."""
    rng = np.random.default_rng(100 * k + d)
    e0, e1 = _plane(rng, d)
    delta = min(0.05, 1.3 / k)
    ang = (k - np.arange(k)) * delta
    C = _at(ang, e0, e1, rng.uniform(0.5, 4.0, k))
    ms = sorted({m for m in (0, 1, 64, 65, k - 1) if m < k}) if k > 1 else []
    th = [0.0] + [ang[m] - 0.1 * delta for m in ms] + rng.uniform(-3.0, 3.0, 8).tolist()
    X = np.vstack([_at(th, e0, e1, rng.uniform(0.5, 20.0, len(th))), rng.normal(size=(8, d))])
    ref = Ref(X, C)
    if k > 1:
        a, _, tr = replay(C, ref.cn, ref.stats, X[0], ref.xn[0])
        assert a == k - 1 == ref.a[0] and tr == ["best"] * k
        for q, m in enumerate(ms):
            a, _, tr = replay(C, ref.cn, ref.stats, X[1 + q], ref.xn[1 + q])
            assert a == m == ref.a[1 + q] and tr == ["best"] * m + ["return"], (m, tr)
            assert ref.na[1 + q] == m
    for r in range(len(X)):
        replay(C, ref.cn, ref.stats, X[r], ref.xn[r])
    return X, C, ref


@functools.lru_cache(maxsize=None)
def prune_case(k, d):
    """k >= 3: centers 0 and 1 at angles 0 and 0.02, the others from 0.5 on,
    delta2 apart; for k >= 4 center k - 1 is 2.0 x center 2 (an exact tie:
    the scaling is exact in the dot and in the norm).  Rows, by replay():
      * at 0.06, 0.07, 0.08: center 1 becomes the best without a return and
        the statistics prune every later center;
      * 0.3 delta2 past center 2 (k >= 4): center 2 becomes the best, center
        k - 1 is visited with a bit-equal distance and the lower index stays,
        with and without statistics.
    k = 2: centers c and 2c; every row ties and goes to center 0."""
    rng = np.random.default_rng(200 * k + d)
    e0, e1 = _plane(rng, d)
    if k == 2:
        C = _at([0.3], e0, e1, rng.uniform(0.5, 4.0))
        C = np.vstack([C, 2.0 * C])
        X = _at(rng.uniform(-3.0, 3.0, 12), e0, e1, rng.uniform(0.5, 20.0, 12))
        ref = Ref(X, C)
        for r in range(len(X)):
            assert cdist(C[0], ref.cn[0], X[r], ref.xn[r]) == cdist(C[1], ref.cn[1], X[r], ref.xn[r])
        assert not ref.a.any() and not ref.na.any()
        return X, C, ref
    delta2 = min(0.02, 2.0 / k)
    ang = np.concatenate([[0.0, 0.02], 0.5 + np.arange(k - 2) * delta2])
    C = _at(ang, e0, e1, rng.uniform(0.5, 4.0, k))
    th = [0.06, 0.07, 0.08]
    if k >= 4:
        C[k - 1] = 2.0 * C[2]
        th += [0.5 + 0.3 * delta2] * 3
    X = _at(th, e0, e1, rng.uniform(0.5, 20.0, len(th)))
    ref = Ref(X, C)
    for r in range(3):
        a, _, tr = replay(C, ref.cn, ref.stats, X[r], ref.xn[r])
        assert a == 1 and tr == ["best", "best"] + ["skip"] * (k - 2), tr
    for r in range(3, len(X)):
        a, best, tr = replay(C, ref.cn, ref.stats, X[r], ref.xn[r])
        assert a == 2 and tr[2] == "best" and tr[k - 1] == "visit", tr
        assert cdist(C[k - 1], ref.cn[k - 1], X[r], ref.xn[r]) == best
        assert ref.na[r] == 2 and ref.nc[r] == best
    return X, C, ref


@functools.lru_cache(maxsize=None)
def line_case(k):
    """d = 1: every center and row is one of two directions, so every
    distance is 0 or 2 to a rounding; the lowest index of a direction wins
    unless a rounding says otherwise, which the oracle decides."""
    rng = np.random.default_rng(300 + k)
    C = rng.normal(size=(k, 1)) * rng.uniform(0.1, 10.0, size=(k, 1))
    if k >= 2:
        C[1] = -abs(C[1])
        C[0] = abs(C[0])
    X = rng.normal(size=(40, 1)) * 3.0
    ref = Ref(X, C)
    assert k == 1 or (np.unique(ref.a).size >= 2 and np.unique(ref.na).size >= 2)
    return X, C, ref


N_STRIDE = 16385


@functools.lru_cache(maxsize=None)
def stride_case():
    """n = 16385, d = 3, k = 3: min((n + 3) / 4, 4096) workgroups of four
    waves, one wave per row, so row 16384 is the second trip of wave 0."""
    rng = np.random.default_rng(16385)
    X, C = rng.normal(size=(N_STRIDE, 3)), rng.normal(size=(3, 3))
    assert (N_STRIDE + 3) // 4 > 4096 and N_STRIDE > 4096 * 4
    return X, C, Ref(X, C)


# ---- row cost
N_COST = (1, 255, 256, 257, 513)
D_COST = (1, 15, 16, 17, 31, 32, 33, 48)


@functools.lru_cache(maxsize=None)
def cost_case(n, d):
    """Random rows, k = 5 random centers (d = 1: one of each sign first)."""
    rng = np.random.default_rng(50 * n + d)
    X, C = rng.normal(size=(n, d)) * 2.0, rng.normal(size=(5, d))
    if d == 1:
        C[0], C[1] = 0.8, -1.3
    return X, C, Ref(X, C), rng.uniform(0.1, 2.0, n)


# ---- the screen on unit directions
SCREEN_SHAPES = ((63, 15), (64, 16), (65, 17), (255, 33), (256, 15), (257, 16), (512, 17),
                 (513, 33), (64, 33), (256, 17))
N_SCREEN = 600
SCALED_TILE = range(32, 48)


@functools.lru_cache(maxsize=None)
def screen_case(d, k):
    """k random directions as centers (about a right angle apart), rows 0.15
    rad around them with a tenth reversed, magnitudes 0.5 .. 20; rows 32 ..
    47 (one 16-row tile of the image) scaled by 1e-100, 1 and 1e100 in turn;
    24 hard rows spread from row 0 to row n - 1, in turn a center itself,
    the bisector of two centers and that bisector one ulp up and down in
    coordinate 0.  A bisector's two distances are within 2 (d + 8) roundings
    of each other (two d-term dots, the divisions, the unit vectors) and are the row's two smallest, far inside the screen's margin
    (2^-20 of the squared norms, kmeans_cos.hip's header), so the screen must
    leave it to the reference loop.  A row around its center has its
    runner-up farther by 0.05 at least, five orders above that margin; a
    reversed row's two nearest are two of the other centers, a random gap
    apart: those within 1e-3 (three orders above the margin) are counted
    with the hard rows, and together they stay below n / 10, half of the
    20 % the device test allows."""
    n = N_SCREEN
    rng = np.random.default_rng(100 * d + k)
    dirs = rng.normal(size=(k, d))
    C = dirs * rng.uniform(0.5, 3.0, size=(k, 1))
    lab = rng.integers(0, k, n)
    X = (dirs[lab] + 0.15 * rng.normal(size=(n, d))) * rng.uniform(0.5, 20.0, size=(n, 1))
    X[rng.random(n) < 0.1] *= -1.0
    unit = dirs / np.linalg.norm(dirs, axis=1)[:, None]
    hpos = np.unique(np.linspace(0, n - 1, 24).round().astype(np.int64))
    kinds = {"center": [], "tie": []}
    for q, r in enumerate(hpos.tolist()):
        a, b = (q // 4) % k, (q // 4 + 1) % k
        if q % 4 == 0:
            X[r] = C[a] * 2.5
            kinds["center"].append((r, a))
        else:
            X[r] = (unit[a] + unit[b]) * 7.0
            if q % 4 >= 2:
                X[r, 0] = np.nextafter(X[r, 0], np.inf if q % 4 == 2 else -np.inf)
            kinds["tie"].append((r, a, b))
    for r in SCALED_TILE:
        X[r] *= (1e-100, 1.0, 1e100)[r % 3]
    ref = Ref(X, C)
    assert hpos[0] == 0 and hpos[-1] == n - 1 and np.isfinite(ref.xn).all() and (ref.xn > 0).all()
    cosd = 1.0 - (X / ref.xn[:, None]) @ unit.T
    srt = np.sort(cosd, axis=1)
    hard = {r for r, *_ in kinds["tie"]}
    for r, a in kinds["center"]:
        assert ref.a[r] == a and abs(ref.c[r]) <= 4 * U * d
    for r, a, b in kinds["tie"]:
        da, db = cdist(C[a], ref.cn[a], X[r], ref.xn[r]), cdist(C[b], ref.cn[b], X[r], ref.xn[r])
        assert abs(da - db) <= 2 * (d + 8) * U and set(np.argsort(cosd[r])[:2].tolist()) == {a, b}
        assert ref.a[r] in (a, b)
    soft = np.array([r for r in range(n) if r not in hard])
    gap = srt[soft, 1] - srt[soft, 0]
    assert (gap[srt[soft, 0] < 0.5] > 0.05).all()
    assert 0 < len(hard) and len(hard) + int((gap <= 1e-3).sum()) < n // 10
    return X, C, ref, len(hard)


@functools.lru_cache(maxsize=None)
def underflow_case():
    """screen_case(64, 16) with row 5 at 1e-170: non-zero coordinates whose
    squares all underflow, so its norm is 0.0 and the reference's assert
    fails, as the oracle shows."""
    X, C, _, _ = screen_case(64, 16)
    X = X.copy()
    X[5] = np.random.default_rng(5).normal(size=64) * 1e-170
    assert (X[5] != 0.0).all() and oracle.row_norms(X)[5] == 0.0
    with pytest.raises(AssertionError, match="Cosine distance is not defined"):
        Ref(X, C)
    return X, C


GIVEN = (("off", 2.0 ** -30), ("on", 2.0 ** -45))


@functools.lru_cache(maxsize=None)
def given_norm_case(which):
    """screen_case(64, 16) with the given norm of center 3 scaled by
    1 + 2^-30 (beyond k_cos_centers_unit's 2^-40 gate: the screen is off) or
    1 + 2^-45 (inside it: the screen stays on).  The oracle divides by the
    same given norms; plan.stats computes the statistics from its own norms,
    accumulate from the given ones."""
    X, C, _, hard = screen_case(64, 16)
    cn0 = oracle.row_norms(C)
    cn = cn0.copy()
    cn[3] = cn0[3] * (1.0 + dict(GIVEN)[which])
    rel = abs(cn[3] - cn0[3]) / cn0[3]
    assert (rel > 2.0 ** -39) if which == "off" else (0 < rel < 2.0 ** -41)
    return X, C, cn, Ref(X, C, cn=cn, stats_cn=cn0), Ref(X, C, cn=cn), hard


# ---- sums and update
SIZES = (0, 1, 7, 8, 9, 255, 256, 257, 513)
D_SUMS = (255, 256, 257)
WEIGHTS = ("none", "positive", "zeros")
P, Z = 0, 3                          # the x / -x cluster; the size-7 cluster


@functools.lru_cache(maxsize=None)
def sums_case(d, weights):
    """k = 10: cluster 0 holds exactly x and -x, clusters 1 .. 9 hold SIZES
    rows (kChunk = 256 rows per partial sum, 8 rows per unrolled trip), rows
    interleaved.  Every center is 0.0 in the last coordinate and x is a
    multiple of that unit vector, so x and -x are at distance exactly 1.0
    from every center and stay with center 0 (a later center replaces the
    best only on a strict `<`); their weights are equal, the sums cancel
    exactly, and the oracle's new center 0 is NaN.  weights 'zeros': every
    row of cluster Z (7 rows) and a tenth of the rows of the clusters of 255
    rows and more weigh 0.0, so cluster Z keeps its center and its norm."""
    rng = np.random.default_rng(d)
    k = len(SIZES) + 1
    dirs = rng.normal(size=(k, d))
    dirs[:, d - 1] = 0.0
    C = dirs * rng.uniform(0.5, 3.0, size=(k, 1))
    own = rng.permutation(np.repeat(np.arange(1, k), SIZES))
    X = (dirs[own] + 0.05 * rng.normal(size=(len(own), d))) * \
        rng.uniform(0.5, 20.0, size=(len(own), 1))
    x = np.zeros(d)
    x[d - 1] = 3.0
    X = np.vstack([X[:10], x, X[10:900], -x, X[900:]])
    own = np.concatenate([own[:10], [P], own[10:900], [P], own[900:]])
    n = len(own)
    w = None
    if weights != "none":
        w = np.random.default_rng(d + 1).uniform(0.1, 3.0, n)
        w[own == P] = 1.25
        if weights == "zeros":
            big = np.flatnonzero(np.isin(own, [6, 7, 8, 9]))
            w[big[::10]] = 0.0
            w[own == Z] = 0.0
    ref = Ref(X, C, w)
    assert np.array_equal(ref.a, own)
    assert tuple(np.bincount(ref.a, minlength=k)) == (2,) + SIZES
    assert (ref.c[own == P] == 1.0).all() and (ref.sums[P] == 0.0).all()
    C2, cn2 = C.copy(), ref.cn.copy()
    oracle.cos_update_centers(C2, cn2, ref.sums, ref.wsum, 1e-4)
    assert np.isnan(C2[P]).all() and cn2[P] == 1.0
    assert np.array_equal(C2[1], C[1]) and cn2[1] == ref.cn[1]          # no row
    if weights == "zeros":
        assert ref.wsum[Z] == 0.0 and np.array_equal(C2[Z], C[Z]) and cn2[Z] == ref.cn[Z]
        assert cn2[Z] != 1.0
    return X, C, w, ref


@functools.lru_cache(maxsize=None)
def sums_line_case(weights):
    """d = 1, k = 2: 513 rows of one direction, 257 of the other."""
    rng = np.random.default_rng(1)
    C = np.array([[1.5], [-0.7]])
    own = rng.permutation(np.repeat([0, 1], [513, 257]))
    X = (np.where(own == 0, 1.0, -1.0) * rng.uniform(0.5, 20.0, len(own)))[:, None]
    w = None
    if weights != "none":
        w = rng.uniform(0.1, 3.0, len(own))
        if weights == "zeros":
            w[::10] = 0.0
    ref = Ref(X, C, w)
    assert np.array_equal(ref.a, own)
    return X, C, w, ref


@functools.lru_cache(maxsize=None)
def converge_case():
    """d = 257, k = 3, 20 rows around each center; center 1 stands 0.3 rad
    off its rows' direction, centers 0 and 2 within 0.02 rad.  The three
    epsilons: below every center's move, between the small moves and the
    large one, above all; the oracle's flags are (False, False, True)."""
    rng = np.random.default_rng(257)
    d, k = 257, 3
    dirs = rng.normal(size=(k, d))
    own = np.repeat(np.arange(k), 20)
    X = (dirs[own] + 0.02 * rng.normal(size=(60, d))) * rng.uniform(0.5, 5.0, size=(60, 1))
    C = dirs.copy()
    C[1] += 0.3 * np.linalg.norm(dirs[1]) * rng.normal(size=d) / np.sqrt(d)
    ref = Ref(X, C)
    assert np.array_equal(ref.a, own)
    C2, cn2 = C.copy(), ref.cn.copy()
    oracle.cos_update_centers(C2, cn2, ref.sums, ref.wsum, 1e-4)
    move = np.array([cdist(C[j], ref.cn[j], C2[j], 1.0) for j in range(k)])
    assert move[1] > 100 * max(move[0], move[2]) and min(move[0], move[2]) > 1e-9
    eps = (min(move) / 2, float(np.sqrt(max(move[0], move[2]) * move[1])), 2 * move[1])
    flags = []
    for e in eps:
        Ce, cne = C.copy(), ref.cn.copy()
        flags.append(oracle.cos_update_centers(Ce, cne, ref.sums, ref.wsum, e))
    assert flags == [False, False, True]
    return X, C, ref, eps, flags


# ---- CSR
K_CSR = (1, 64, 65, 66, 129)
LENS_CSR = (1, 2, 63, 64, 65)
D_CSR = 80


@functools.lru_cache(maxsize=None)
def csr_case(k):
    """d = 80, 50 x 5 rows whose stored lengths cycle through LENS_CSR, a
    twentieth of the stored values of the rows of 63 entries and more an
    explicit 0.0 (never a row's first); the centers are k rows of 63 entries
    and more plus noise, the last one without noise, so that row is at
    distance ~0 of center k - 1."""
    rng = np.random.default_rng(900 + k)
    lens = np.tile(LENS_CSR, 50)
    rows = []
    for c, x in S.random_rows(rng, lens, D_CSR):
        x = np.where(x == 0.0, 0.5, x)
        if len(x) >= 63:
            x[1:][rng.random(len(x) - 1) < 0.05] = 0.0
        rows.append((c, x))
    csr = S.from_rows(rows)
    picks = rng.choice(np.flatnonzero(lens >= 63), size=k, replace=False)
    C = csr.dense(D_CSR)[picks] + rng.normal(size=(k, D_CSR)) * 0.05
    C[k - 1] = csr.dense(D_CSR)[picks[k - 1]]
    ref = S.Ref(S.COS, csr, D_CSR, C)
    assert set(np.diff(csr.rp).tolist()) == set(LENS_CSR) and (csr.values == 0.0).sum() >= 20
    assert ref.a[picks[k - 1]] == k - 1 == ref.na[picks[k - 1]]
    assert k == 1 or (np.unique(ref.a).size > k // 2 and np.unique(ref.na).size > k // 2)
    return csr, C, rng.uniform(0.1, 2.0, csr.n), ref


@functools.lru_cache(maxsize=None)
def csr_empty_case():
    """csr_case(65) with row 7 emptied: its norm is 0.0 and the oracle's
    assert fails."""
    csr, C, _, _ = csr_case(65)
    lens = np.diff(csr.rp)
    rows = [(csr.colidx[csr.rp[r]:csr.rp[r + 1]], csr.values[csr.rp[r]:csr.rp[r + 1]])
            for r in range(csr.n)]
    rows[7] = (np.zeros(0, np.int32), np.zeros(0))
    out = S.from_rows(rows)
    assert np.diff(out.rp)[7] == 0 and lens[7] > 0
    with pytest.raises(AssertionError, match="Cosine distance is not defined"):
        S.Ref(S.COS, out, D_CSR, C)
    return out, C


N_CSR_STRIDE = 32769


@functools.lru_cache(maxsize=None)
def csr_stride_case():
    """n = 32769 rows of one stored entry, d = 8, k = 3: min((n + 3) / 4,
    8192) workgroups of four waves, so row 32768 is wave 0's second trip."""
    rng = np.random.default_rng(32769)
    n, d = N_CSR_STRIDE, 8
    csr = S.CSR(np.arange(n + 1), rng.integers(0, d, n), rng.normal(size=n) + 3.0 * rng.choice(
        [-1.0, 1.0], n))
    C = rng.normal(size=(3, d))
    assert (n + 3) // 4 > 8192 and n > 8192 * 4
    return csr, C, rng.uniform(0.1, 2.0, n), S.Ref(S.COS, csr, d, C)


@functools.lru_cache(maxsize=None)
def csr_view_case():
    """rowptr[50:151] of csr_case(66) with the full colidx and values: the
    view keeps its base (rowptr[0] > 0); the oracle gives the same on the
    view and on a rebased copy."""
    csr, C, w, _ = csr_case(66)
    view = csr.view(50, 150)
    copy = view.rebased()
    assert view.rp[0] > 0 and copy.rp[0] == 0
    ref, ref2 = S.Ref(S.COS, view, D_CSR, C), S.Ref(S.COS, copy, D_CSR, C)
    for f in ("xn", "a", "c", "na", "nc"):
        np.testing.assert_array_equal(getattr(ref, f), getattr(ref2, f))
    return view, copy, C, w[50:150], ref


def host_cases():
    """Every case's host half (inputs, reference, conditions on the inputs)."""
    for k in K_STATS:
        for d in D_STATS:
            yield stats_case, (k, d)
    for d in D_STATS:
        yield stats_pair_case, (d,)
    for kd in STATS_CONTENT:
        yield stats_content_case, kd
    for k in K_LOOP:
        yield line_case, (k,)
        for d in D_LOOP:
            yield fan_case, (k, d)
            if k >= 2:
                yield prune_case, (k, d)
    yield stride_case, ()
    for n in N_COST:
        for d in D_COST:
            yield cost_case, (n, d)
    for dk in SCREEN_SHAPES:
        yield screen_case, dk
    yield underflow_case, ()
    for which, _ in GIVEN:
        yield given_norm_case, (which,)
    for wt in WEIGHTS:
        for d in D_SUMS:
            yield sums_case, (d, wt)
        yield sums_line_case, (wt,)
    yield converge_case, ()
    for k in K_CSR:
        yield csr_case, (k,)
    yield csr_empty_case, ()
    yield csr_stride_case, ()
    yield csr_view_case, ()


def test_host_cases():
    """Without a device: every builder's conditions on its inputs hold."""
    seen = 0
    for fn, args in host_cases():
        fn(*args)
        seen += 1
    assert seen >= len(K_STATS) * len(D_STATS) + len(N_COST) * len(D_COST) + 90


# ------------------------------------------------------------------- device
def _dev(a, cuda):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _eq(t, ref, what=""):
    np.testing.assert_array_equal(t.cpu().numpy(), ref, err_msg=what)


def _same_bits(a, b):
    """torch.equal on the words: a NaN equals itself."""
    import torch
    if a.dtype == torch.float64:
        a, b = a.view(torch.int64), b.view(torch.int64)
    return torch.equal(a, b)


def run(cuda, X, C, mode, image=True, w=None, cn=None, per_row=True):
    """One call on a fresh cosine plan (test_kmeans_cosine.py's _gpu, with
    poisoned outputs and given norms).  mode 'assign': stats, then assign
    with the exact count; 'point_cost'; 'lloyd': accumulate into zeroed
    buffers.  Returns the outputs as device tensors."""
    import torch
    from cycloneml_amd.clustering import KMeansPlan, row_norms
    n, d = X.shape
    k = C.shape[0]
    Xd, Cd = _dev(X, cuda), _dev(C, cuda)
    xn = row_norms(Xd)
    cnd = row_norms(Cd) if cn is None else _dev(cn, cuda)
    p = KMeansPlan(d, k, n, "cosine")
    rows = p.rows(Xd) if image else None
    a = torch.full((n,), -1, dtype=torch.int32, device=cuda)
    c = torch.full((n,), float("nan"), dtype=torch.float64, device=cuda)
    out = {"a": a, "c": c}
    try:
        if mode == "assign":
            st = torch.full((k * (k + 1) // 2,), -7.0, dtype=torch.float64, device=cuda)
            p.stats(Cd, st)
            out["n_exact"] = p.assign(Xd, xn, Cd, cnd, a, c, count_exact=True, rows=rows)
            out["stats"] = st
        elif mode == "point_cost":
            p.point_cost(Xd, xn, Cd, cnd, a, c, rows=rows)
        else:
            buf = torch.zeros(k * d + k + 1, dtype=torch.float64, device=cuda)
            p.accumulate(Xd, xn, None if w is None else _dev(w, cuda), Cd, cnd, buf[:k * d],
                         buf[k * d:k * d + k], buf[k * d + k:], a, c if per_row else None,
                         rows=rows)
            out["buf"] = buf
            if not per_row:
                del out["c"]
        torch.cuda.synchronize()
    finally:
        if rows is not None:
            rows.close()
        p.close()
    return out


def check_update(cuda, C, cn, buf, eps=1e-4):
    """update on the device's own sums and weights against the oracle's."""
    import torch
    from cycloneml_amd.clustering import KMeansPlan
    k, d = C.shape
    Cd, cnd = _dev(C, cuda), _dev(cn, cuda)
    conv = torch.zeros(1, dtype=torch.int32, device=cuda)
    p = KMeansPlan(d, k, 1, "cosine")
    p.update(Cd, cnd, buf[:k * d], buf[k * d:k * d + k], eps, conv)
    torch.cuda.synchronize()
    p.close()
    b = buf.cpu().numpy()
    Ch, cnh = C.copy(), cn.copy()
    rconv = oracle.cos_update_centers(Ch, cnh, b[:k * d], b[k * d:k * d + k], eps)
    _eq(Cd, Ch, "updated centers")
    _eq(cnd, cnh, "updated norms")
    assert bool(conv.item()) == rconv
    return Cd.cpu().numpy(), cnd.cpu().numpy(), rconv


def check_assign(cuda, X, C, ref, image, cn=None, what=""):
    """stats + assign and point_cost on fresh plans, each twice."""
    g = run(cuda, X, C, "assign", image, cn=cn)
    np.testing.assert_array_equal(g["stats"].cpu().numpy(), ref.stats, err_msg=f"{what}: stats")
    bad = np.flatnonzero(g["a"].cpu().numpy() != ref.a)
    assert bad.size == 0, f"{what}: {bad.size} assignments differ, first rows {bad[:10]}"
    _eq(g["c"], ref.c, f"{what}: cost")
    g2 = run(cuda, X, C, "assign", image, cn=cn)
    assert all(_same_bits(g[f], g2[f]) for f in ("a", "c", "stats"))
    assert g["n_exact"] == g2["n_exact"]
    q = run(cuda, X, C, "point_cost", image, cn=cn)
    _eq(q["a"], ref.na, f"{what}: point_cost index")
    _eq(q["c"], ref.nc, f"{what}: point_cost")
    q2 = run(cuda, X, C, "point_cost", image, cn=cn)
    assert _same_bits(q["a"], q2["a"]) and _same_bits(q["c"], q2["c"])
    return g["n_exact"]


def check_call(cuda, X, C, ref, w=None, image=True, cn=None, per_row=True, what=""):
    """accumulate on a fresh plan by every bar, a second one on another
    fresh plan bit-equal to it, then update.  Returns update's outputs."""
    n, d = X.shape
    k = C.shape[0]
    kd = k * d
    g = run(cuda, X, C, "lloyd", image, w, cn, per_row)
    bad = np.flatnonzero(g["a"].cpu().numpy() != ref.a)
    assert bad.size == 0, f"{what}: {bad.size} assignments differ, first rows {bad[:10]}"
    if per_row:
        _eq(g["c"], ref.c, f"{what}: per-row cost")
    b = g["buf"].cpu().numpy()
    ts, tw, tc = terms(X, w, ref)
    zero = np.zeros(kd + k + 1)
    check_entries(b[:kd], zero[:kd], [ts], f"{what}: sums")
    if w is None:
        np.testing.assert_array_equal(b[kd:kd + k], np.bincount(ref.a, minlength=k).astype(float),
                                      err_msg=f"{what}: wsum")
    else:
        check_entries(b[kd:kd + k], zero[:k], [tw], f"{what}: wsum")
    check_entries(b[kd + k:], zero[:1], [tc], f"{what}: cost sum")
    g2 = run(cuda, X, C, "lloyd", image, w, cn, per_row)
    assert all(_same_bits(g[f], g2[f]) for f in g)
    return check_update(cuda, C, ref.cn, g["buf"])


# -------------------------------------------------------------------- tests
def _stats(cuda, C):
    import torch
    from cycloneml_amd.clustering import KMeansPlan
    k, d = C.shape
    st = torch.full((k * (k + 1) // 2,), -7.0, dtype=torch.float64, device=cuda)
    p = KMeansPlan(d, k, 1, "cosine")
    p.stats(_dev(C, cuda), st)
    torch.cuda.synchronize()
    p.close()
    return st


def check_stats(cuda, C, st, what):
    g = _stats(cuda, C)
    np.testing.assert_array_equal(g.cpu().numpy(), st, err_msg=what)      # NaN == NaN here
    assert _same_bits(g, _stats(cuda, C))


@gpu
@pytest.mark.parametrize("k", K_STATS)
def test_stats_shapes(cuda, k):
    """Centers either side of the 32-center tile (1, 2 and 3 tiles per side,
    the last one of 1, 31 and 32 centers) at widths either side of the
    32-dimension chunk; k = 1 gives the single NaN."""
    for d in D_STATS:
        C, st = stats_case(k, d)
        check_stats(cuda, C, st, f"k={k}, d={d}")


@gpu
def test_stats_content(cuda):
    """Negative statistics (scaled copies) on and off the diagonal, a NaN
    off it (an exactly antipodal pair), k = 2 with that pair: both diagonal
    entries +Infinity (d = 1: the oracle's finite values)."""
    for k, d in STATS_CONTENT:
        C, st = stats_content_case(k, d)
        check_stats(cuda, C, st, f"content k={k}, d={d}")
    for d in D_STATS:
        C, st = stats_pair_case(d)
        check_stats(cuda, C, st, f"pair d={d}")


@gpu
@pytest.mark.parametrize("k", K_LOOP)
def test_reference_loop(cuda, k):
    """Every row through k_cos_assign_exact (no image), with statistics and
    without: the 64-center replay groups start at center 1 with statistics
    (groups end at 64 and 128) and at center 0 without (63 and 127)."""
    cases = [("line", line_case(k))]
    for d in D_LOOP:
        cases.append((f"fan d={d}", fan_case(k, d)))
        if k >= 2:
            cases.append((f"prune d={d}", prune_case(k, d)))
    for name, (X, C, ref) in cases:
        n_exact = check_assign(cuda, X, C, ref, False, what=f"k={k}, {name}")
        assert n_exact == len(X)


@gpu
def test_reference_loop_grid_stride(cuda):
    """n = 16385 rows on 4096 workgroups: the second trip of the row loop."""
    X, C, ref = stride_case()
    assert check_assign(cuda, X, C, ref, False, what="grid stride") == N_STRIDE


@gpu
@pytest.mark.parametrize("d", D_COST)
def test_row_cost(cuda, d):
    """k_cos_row_cost's 256-row blocks and 16-column double-buffered slices
    (one, two and three slices, a last slice of 1, 15 and 16 columns),
    through point_cost and through accumulate with per-row costs."""
    for n in N_COST:
        X, C, ref, w = cost_case(n, d)
        check_assign(cuda, X, C, ref, False, what=f"n={n}, d={d}")
        check_call(cuda, X, C, ref, image=False, what=f"n={n}, d={d}")
    check_call(cuda, X, C, Ref(X, C, w), w=w, image=False, what=f"n={n}, d={d}, weighted")


@gpu
@pytest.mark.parametrize("d,k", SCREEN_SHAPES)
def test_screen_on_unit_directions(cuda, d, k):
    """Widths either side of the image's forms, uses32's d <= 256 and kMaxD
    = 512; centers either side of the 16-center tile.  The hard rows reach
    the reference loop, most others do not; no image at d = 513."""
    X, C, ref, hard = screen_case(d, k)
    n_exact = check_assign(cuda, X, C, ref, True, what=f"d={d}, k={k}")
    if d <= 512:
        assert 0 < hard <= n_exact < N_SCREEN
        assert n_exact < N_SCREEN // 5
    else:
        assert n_exact == N_SCREEN
    check_call(cuda, X, C, ref, what=f"d={d}, k={k}")


@gpu
@pytest.mark.parametrize("mode", ["assign", "point_cost", "lloyd"])
def test_underflowed_norm_asserts(cuda, mode):
    """A non-zero row whose norm underflows to 0.0: the reference's text."""
    from cycloneml_amd import _native as N
    X, C = underflow_case()
    with pytest.raises(N.JavaAssertionError, match=ASSERT_TEXT):
        run(cuda, X, C, mode)


@gpu
@pytest.mark.parametrize("which", [g[0] for g in GIVEN])
def test_given_center_norms(cuda, which):
    """A given norm 2^-30 off its center's computed norm turns the screen
    off, one 2^-45 off leaves it on; the results follow the given norms."""
    X, C, cn, ref_assign, ref_lloyd, hard = given_norm_case(which)
    n_exact = check_assign(cuda, X, C, ref_assign, True, cn=cn, what=f"given norm, screen {which}")
    if which == "off":
        assert n_exact == N_SCREEN
    else:
        assert hard <= n_exact < N_SCREEN
    check_call(cuda, X, C, ref_lloyd, cn=cn, what=f"given norm, screen {which}")


@gpu
@pytest.mark.parametrize("weights", WEIGHTS)
@pytest.mark.parametrize("d", D_SUMS)
def test_cluster_sizes(cuda, d, weights):
    """Clusters of 0 .. 513 rows in one call at widths either side of the
    256-thread column stride; an empty cluster and one of weight 0 keep
    their centers and norms, the x / -x cluster's new center is NaN."""
    X, C, w, ref = sums_case(d, weights)
    for image, per_row in ((True, True), (False, False)):
        C2, cn2, conv = check_call(cuda, X, C, ref, w=w, image=image, per_row=per_row,
                                   what=f"d={d}, {weights}, image={image}")
        assert np.isnan(C2[P]).all() and cn2[P] == 1.0 and not conv
        keep = [1, Z] if weights == "zeros" else [1]
        for j in keep:
            assert np.array_equal(C2[j].view(np.int64), C[j].view(np.int64))
            assert cn2[j] == ref.cn[j] != 1.0


@gpu
@pytest.mark.parametrize("weights", WEIGHTS)
def test_cluster_sums_one_dimension(cuda, weights):
    X, C, w, ref = sums_line_case(weights)
    for image in (True, False):
        check_call(cuda, X, C, ref, w=w, image=image, what=f"d=1, {weights}, image={image}")


@gpu
def test_convergence_flag(cuda):
    """One center moves by more than epsilon between two that move by less."""
    X, C, ref, eps, flags = converge_case()
    g = run(cuda, X, C, "lloyd", True)
    _eq(g["a"], ref.a)
    got = [check_update(cuda, C, ref.cn, g["buf"], e)[2] for e in eps]
    assert got == flags


@gpu
@pytest.mark.parametrize("k", K_CSR)
def test_csr_center_groups(cuda, k):
    """k_cos_assign_sparse's 64-center groups with and without statistics,
    rows of 1 .. 65 stored entries and stored zeros."""
    csr, C, w, ref = csr_case(k)
    S.check_assign(cuda, S.COS, D_CSR, C, csr, ref)
    S.check_point_cost(cuda, S.COS, D_CSR, C, csr, ref)
    S.check_accumulate(cuda, S.COS, D_CSR, C, [(csr, w, ref)], update=True)
    S.check_accumulate(cuda, S.COS, D_CSR, C, [(csr, None, ref)])


@gpu
def test_csr_empty_row_asserts(cuda):
    import torch
    from cycloneml_amd import _native as N
    from cycloneml_amd.clustering import KMeansPlan, row_norms, row_norms_csr
    csr, C = csr_empty_case()
    k = C.shape[0]
    rp, ci, v = csr.dev(cuda)
    Cd = _dev(C, cuda)
    xn, cn = row_norms_csr(rp, v), row_norms(Cd)
    a, c = S._out(csr.n, cuda)
    p = KMeansPlan(D_CSR, k, csr.n, "cosine")
    with pytest.raises(N.JavaAssertionError, match=ASSERT_TEXT):
        p.point_cost_csr(rp, ci, v, xn, Cd, cn, a, c)
    buf = torch.zeros(k * D_CSR + k + 1, dtype=torch.float64, device=cuda)
    with pytest.raises(N.JavaAssertionError, match=ASSERT_TEXT):
        p.accumulate_csr(rp, ci, v, xn, None, Cd, cn, buf[:k * D_CSR], buf[k * D_CSR:-1], buf[-1:])
    p.close()


@gpu
def test_csr_grid_stride(cuda):
    """n = 32769 rows on 8192 workgroups: the second trip of the row loop."""
    csr, C, w, ref = csr_stride_case()
    S.check_assign(cuda, S.COS, 8, C, csr, ref)
    S.check_point_cost(cuda, S.COS, 8, C, csr, ref)
    S.check_accumulate(cuda, S.COS, 8, C, [(csr, w, ref)])


@gpu
def test_csr_rowptr_view(cuda):
    """A rowptr slice that keeps its base is accepted, as by the Euclidean
    entry points."""
    view, copy, C, w, ref = csr_view_case()
    for csr in (view, copy):
        S.check_norms(cuda, csr, ref)
        S.check_point_cost(cuda, S.COS, D_CSR, C, csr, ref)
        S.check_accumulate(cuda, S.COS, D_CSR, C, [(csr, w, ref)])
