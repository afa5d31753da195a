"""Conformance tests of KMeans over sparse (CSR) points at the wave, launch,
center-tile, row-length and key-width edges of kmeans_sparse.hip, the sparse
half of kmeans_cos.hip and the cyc_*_csr_dev entry points of kmeans.hip.

Bars:
  * assignments, per-row costs and row_norms_csr: bit-exact against the C
    oracle (the kernels restate the reference's operation order);
  * sums, weight sums and the cost sum: entry by entry within the bound that
    check_entries (sum_bounds.py) derives from the terms of that entry alone;
  * a second run of the same calls: torch.equal to the first;
  * update after accumulate: bit-exact against the oracle's update fed the
    device's own sums.

Every case is built on the host by a cached function that also asserts, on
the reference alone, that the inputs reach the edge the case is about (every
center hit, rows past the first grid stride in several clusters, the largest
sort key present, ...): host_cases() lists them, so they can be checked
without a device.
"""
import functools

import numpy as np
import pytest

import oracle
from sum_bounds import check_entries

pytestmark = pytest.mark.gpu

EUC, COS = "euclidean", "cosine"


# --------------------------------------------------------------------- host
class CSR:
    """Rows lo..hi of a CSR matrix as a view: the full colidx and values with
    rowptr[lo:hi + 1], which starts at 0 only when lo == 0."""

    def __init__(self, rowptr, colidx, values, lo=0, hi=None):
        self.rowptr = np.ascontiguousarray(rowptr, dtype=np.int64)
        self.colidx = np.ascontiguousarray(colidx, dtype=np.int32)
        self.values = np.ascontiguousarray(values, dtype=np.float64)
        self.lo = lo
        self.hi = len(self.rowptr) - 1 if hi is None else hi

    @property
    def rp(self):
        return self.rowptr[self.lo:self.hi + 1]

    @property
    def n(self):
        return self.hi - self.lo

    def host(self):
        return (self.rp, self.colidx, self.values)

    def view(self, lo, hi):
        return CSR(self.rowptr, self.colidx, self.values, self.lo + lo, self.lo + hi)

    def rebased(self):
        rp = self.rp
        return CSR(rp - rp[0], self.colidx[rp[0]:rp[-1]], self.values[rp[0]:rp[-1]])

    def dense(self, d):
        rp = self.rp
        X = np.zeros((self.n, d))
        for r in range(self.n):
            X[r, self.colidx[rp[r]:rp[r + 1]]] = self.values[rp[r]:rp[r + 1]]
        return X

    def dev(self, cuda):
        return (_dev(self.rowptr, cuda)[self.lo:self.hi + 1], _dev(self.colidx, cuda),
                _dev(self.values, cuda))


def from_rows(rows):
    """rows: list of (sorted column array, value array)."""
    rp = np.zeros(len(rows) + 1, dtype=np.int64)
    rp[1:] = np.cumsum([len(c) for c, _ in rows])
    ci = np.concatenate([np.asarray(c, np.int32) for c, _ in rows] + [np.zeros(0, np.int32)])
    v = np.concatenate([np.asarray(x, np.float64) for _, x in rows] + [np.zeros(0)])
    return CSR(rp, ci, v)


def random_rows(rng, lens, d, cols=None):
    """One row per entry of lens: that many distinct sorted columns (out of
    the first `cols`, default d), values like tests/test_kmeans_sparse_gpu.py."""
    rows = []
    for m in lens:
        c = np.sort(rng.choice(d if cols is None else cols, size=int(m), replace=False))
        rows.append((c, rng.normal(size=int(m)) * 3.0 + rng.integers(-2, 3)))
    return rows


class Ref:
    """The oracle's answers for one CSR view: norms, findClosest with
    statistics (a, c) and without (na, nc)."""

    def __init__(self, measure, csr, d, C):
        h = csr.host()
        self.xn = oracle.row_norms_csr(h[0], h[2])
        self.cn = oracle.row_norms(C)
        if measure == EUC:
            self.a, self.c, *_ = oracle.kmeans_partition_sparse(h, self.xn, None, C, self.cn,
                                                                oracle.kmeans_stats(C))
            self.na, self.nc, _ = oracle.point_costs_sparse(h, self.xn, C, self.cn)
        else:
            self.a, self.c, *_ = oracle.cos_kmeans_partition_sparse(
                h + (d,), self.xn, None, C, self.cn, oracle.cos_stats(C, self.cn))
            self.na, self.nc, _ = oracle.cos_point_costs_sparse(h + (d,), self.xn, C, self.cn)


def terms(measure, csr, d, w, ref):
    """The terms the device folds, as (entry index, term) arrays, built as the
    kernels build them: sums (k_sp_keys) t = a * x_q at cluster * d + column
    with a = w (Euclidean) or w / |x| (cosine), a == 1.0 passed through;
    weight sums t = w at the cluster; cost sum t = cost * w (k_sp_rowvals)."""
    rp = csr.rp
    n = csr.n
    wr = np.ones(n) if w is None else np.asarray(w, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        a = wr / ref.xn if measure == COS else wr
    rows = np.repeat(np.arange(n), np.diff(rp))
    q = np.arange(rp[0], rp[n])
    x, ar = csr.values[q], a[rows]
    t = np.where(ar == 1.0, x, ar * x)
    keys = ref.a[rows].astype(np.int64) * d + csr.colidx[q]
    return ((keys, t), (ref.a.astype(np.int64), wr), (np.zeros(n, np.int64), ref.c * wr))


def all_hit(a, k, never=()):
    """Every center index is some row's result, except `never`, which no row takes."""
    cnt = np.bincount(a, minlength=k)
    miss = [i for i in range(k) if i not in never and cnt[i] == 0]
    assert not miss, f"centers no row lands on: {miss}"
    assert all(cnt[i] == 0 for i in never), f"rows on a later duplicate: {never}"


# -------------------------------------------------------------- host cases
N_TILE, D_TILE = 600, 24
K_STATS = (1, 2, 3, 64, 65, 66, 128, 129, 130)
K_NOSTATS = (1, 63, 64, 65, 128, 129)
# (measure, k, with_stats) -> seed, where the default leaves a center without a row
TILE_SEED = {(COS, 63, False): 7100}


@functools.lru_cache(maxsize=None)
def tile_case(measure, k, with_stats):
    """n = 600, d = 24, density 0.3; centers are k distinct rows, then
      * one center is a (1 + 1e-15) scaling of another (k >= 2): center k - 1
        of center 1 (of center 0 for k <= 3), so the last center, which is
        the only valid lane of its tile at k = 66 / 130 (with statistics) and
        65 / 129 (without), is won or lost by a few ulps.  Twenty rows are
        positive scalings of that center's row: in exact arithmetic those
        below 1 are nearer the smaller and those above 1 nearer the larger of
        the pair (Euclidean), and all of them tie (cosine);
      * two centers are exact duplicates (k >= 3): indices b - 1 and b + 1
        around the first tile boundary b (b = 65 with statistics, where center
        0 is taken first; 64 without) where k >= b + 3, else 5 and 40 (0 and 1
        at k = 3).  The later copy can never win: findClosest replaces the
        best only on a strict `<` (DistanceMeasure.scala:297-303, :318-340),
        and a prune that skipped the first copy skips the second.  So the
        condition on the inputs is: every center but that copy is some row's
        result in the reference, and that copy is no row's.  The copy is kept
        off b, b - 1 and k - 1, which therefore are all hit."""
    n, d = N_TILE, D_TILE
    rng = np.random.default_rng(TILE_SEED.get((measure, k, with_stats), 7000 + k))
    lens = np.maximum(1, rng.binomial(d, 0.3, n))
    if measure == EUC:
        lens[rng.choice(n, size=5, replace=False)] = 0           # empty rows
    rows = random_rows(rng, lens, d)
    picks = rng.choice(np.flatnonzero(lens > 1), size=k, replace=False)
    src = 0 if k <= 3 else 1
    never = ()
    if k >= 2:
        free = np.setdiff1d(np.flatnonzero(lens > 0), picks)[:20]
        c, x = rows[picks[src]]
        for r, s in zip(free, np.concatenate([rng.uniform(0.4, 0.9, 10), rng.uniform(1.2, 4, 10)])):
            rows[r] = (c, x * s)
    csr = from_rows(rows)
    C = csr.dense(d)[picks]
    if k >= 2:
        C[k - 1] = C[src] * (1 + 1e-15)
    if k >= 3:
        b = 65 if with_stats else 64
        lo, hi = (0, 1) if k == 3 else (b - 1, b + 1) if k >= b + 3 else (5, 40)
        C[hi] = C[lo]
        never = (hi,)
    ref = Ref(measure, csr, d, C)
    all_hit(ref.a if with_stats else ref.na, k, never)
    w = rng.uniform(0.1, 2.0, n)
    return csr, C, w, ref


LENS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 200, 256)


@functools.lru_cache(maxsize=None)
def rowlen_case(measure):
    """d = 256, 22 x 11 rows whose lengths cycle through LENS (cosine: the
    empty rows left out), k = 7.  Rows of at most 64 entries draw their
    columns from the first 128 only, so columns 128.. are reached by longer
    rows alone."""
    d, k = 256, 7
    rng = np.random.default_rng(31)
    lens = np.array([m for _ in range(22) for m in LENS if m > 0 or measure == EUC])
    rows = []
    for m in lens:
        rows += random_rows(rng, [m], d, cols=128 if m <= 64 else d)
    csr = from_rows(rows)
    C = csr.dense(d)[rng.choice(np.flatnonzero(lens >= 63), size=k, replace=False)]
    C += rng.normal(size=C.shape) * 0.01
    ref = Ref(measure, csr, d, C)
    rowof = np.repeat(np.arange(csr.n), np.diff(csr.rp))
    short = np.unique(csr.colidx[lens[rowof] <= 64])
    only_long = np.setdiff1d(np.unique(csr.colidx), short)
    assert only_long.size >= 100 and short.max() < 128
    # entries of the sums all of whose terms sit at position >= 64 of a row
    pos = np.arange(len(rowof)) - csr.rp[rowof]
    keys = ref.a[rowof].astype(np.int64) * d + csr.colidx
    assert np.setdiff1d(keys[pos >= 64], keys[pos < 64]).size > 0
    return csr, C, rng.uniform(0.1, 2.0, csr.n), ref, d


N_LAUNCH = (1, 3, 4, 5, 255, 257, 32768 + 7)


@functools.lru_cache(maxsize=None)
def launch_case(measure, n):
    """d = 12, k = 5, 1-4 nonzeros per row; one wave per row in workgroups of
    4 waves, min((n + 3) / 4, 8192) of them: the row loops take a second trip
    from row 32768 on."""
    d, k = 12, 5
    rng = np.random.default_rng(400 + n)
    csr = from_rows(random_rows(rng, rng.integers(1, 5, n), d))
    C = rng.normal(size=(k, d)) * 2.0
    ref = Ref(measure, csr, d, C)
    if n > 32768:
        assert np.unique(ref.a[32768:]).size > 1 and np.unique(ref.na[32768:]).size > 1
    return csr, C, rng.uniform(0.1, 2.0, n), ref, d


@functools.lru_cache(maxsize=None)
def shard_case(measure):
    """900 rows, d = 30, k = 6; column d - 1 is never stored and center k - 1
    is far from every row, so some entries of every buffer get no term."""
    n, d, k = 900, 30, 6
    rng = np.random.default_rng(55)
    rows = random_rows(rng, np.maximum(1, rng.binomial(d - 1, 0.25, n)), d, cols=d - 1)
    rows = [(c, np.abs(x) + 0.1) for c, x in rows]
    csr = from_rows(rows)
    C = csr.dense(d)[rng.choice(n, size=k, replace=False)] + rng.normal(size=(k, d)) * 0.01
    C[k - 1] = -(50.0 + rng.uniform(size=d))
    w = rng.uniform(0.1, 2.0, n)
    return csr, C, w, d


@functools.lru_cache(maxsize=None)
def degenerate_case(measure):
    """k = 9 with centers 6..8 far from every row (all values are positive,
    these centers negative: far for both measures); 10% of the weights 0.0,
    20% exactly 1.0; about 5% of the stored entries explicit 0.0 (never a
    row's first, so no cosine row is zero)."""
    n, d, k = 500, 20, 9
    rng = np.random.default_rng(77)
    rows = []
    for c, x in random_rows(rng, np.maximum(2, rng.binomial(d, 0.3, n)), d):
        x = np.abs(x) + 0.1
        x[1:][rng.random(len(x) - 1) < 0.05] = 0.0
        rows.append((c, x))
    csr = from_rows(rows)
    assert 0.02 < np.mean(csr.values == 0.0) < 0.08
    C = csr.dense(d)[rng.choice(n, size=k, replace=False)]
    C[6:] = -(50.0 + rng.uniform(size=(3, d)))
    w = rng.uniform(0.1, 2.0, n)
    u = rng.random(n)
    w[u < 0.1] = 0.0
    w[u > 0.8] = 1.0
    ref = Ref(measure, csr, d, C)
    all_hit(ref.a, k, never=(6, 7, 8))
    return csr, C, w, ref, d


@functools.lru_cache(maxsize=None)
def empty_case():
    """70 rows without a stored entry (no colidx, no values), k = 3."""
    n, d, k = 70, 5, 3
    rng = np.random.default_rng(9)
    csr = CSR(np.zeros(n + 1, np.int64), np.zeros(0, np.int32), np.zeros(0))
    C = rng.normal(size=(k, d))
    w = rng.uniform(0.1, 2.0, n)
    w[::7] = 0.0
    return csr, C, w, Ref(EUC, csr, d, C), d


KD = ((4, 16), (4, 17), (5, 13), (2, 32), (3, 43), (256, 1), (257, 1), (1, 1))


@functools.lru_cache(maxsize=None)
def keywidth_case(k, d):
    """k * d and k at a power of two and one past it: the radix sorts take
    bits_for(k * d) and bits_for(max(k - 1, 1)) key bits.  The last center is
    a row that stores column d - 1, so the largest key k * d - 1 occurs."""
    n = 600 if k >= 256 else 400
    rng = np.random.default_rng(800 + k * d)
    csr = from_rows(random_rows(rng, np.maximum(1, rng.binomial(d, 0.4, n)), d))
    last = np.flatnonzero(csr.colidx[csr.rp[1:] - 1] == d - 1)
    picks = rng.choice(np.setdiff1d(np.arange(n), last[:1]), size=k - 1, replace=False)
    C = csr.dense(d)[np.append(picks, last[0])]
    ref = Ref(EUC, csr, d, C)
    rowof = np.repeat(np.arange(n), np.diff(csr.rp))
    assert (ref.a[rowof].astype(np.int64) * d + csr.colidx).max() == k * d - 1
    assert ref.a.max() == k - 1
    return csr, C, rng.uniform(0.1, 2.0, n), ref


def host_cases():
    """Every case's host half (inputs, reference, conditions on the inputs)."""
    for m in (EUC, COS):
        for k in K_STATS:
            yield tile_case, (m, k, True)
        for k in K_NOSTATS:
            yield tile_case, (m, k, False)
        yield rowlen_case, (m,)
        for n in N_LAUNCH:
            yield launch_case, (m, n)
        yield shard_case, (m,)
        yield degenerate_case, (m,)
    yield empty_case, ()
    for kd in KD:
        yield keywidth_case, kd


# ------------------------------------------------------------------- device
def _dev(a, cuda):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _eq(t, ref):
    np.testing.assert_array_equal(t.cpu().numpy(), ref)


def _out(n, cuda):
    import torch
    return (torch.full((n,), -1, dtype=torch.int32, device=cuda),
            torch.full((n,), float("nan"), dtype=torch.float64, device=cuda))


def check_norms(cuda, csr, ref):
    from cycloneml_amd.clustering import row_norms_csr
    rp, _, v = csr.dev(cuda)
    _eq(row_norms_csr(rp, v), ref.xn)


def check_assign(cuda, measure, d, C, csr, ref):
    """assign_csr after stats."""
    from cycloneml_amd.clustering import KMeansPlan, row_norms, row_norms_csr
    rp, ci, v = csr.dev(cuda)
    Cd = _dev(C, cuda)
    p = KMeansPlan(d, C.shape[0], csr.n, measure)
    p.stats(Cd)
    a, c = _out(csr.n, cuda)
    p.assign_csr(rp, ci, v, row_norms_csr(rp, v), Cd, row_norms(Cd), a, c)
    _eq(a, ref.a)
    _eq(c, ref.c)
    p.close()


def check_point_cost(cuda, measure, d, C, csr, ref, after_stats=False):
    """point_cost_csr: findClosest without statistics."""
    from cycloneml_amd.clustering import KMeansPlan, row_norms, row_norms_csr
    rp, ci, v = csr.dev(cuda)
    Cd = _dev(C, cuda)
    p = KMeansPlan(d, C.shape[0], csr.n, measure)
    if after_stats:
        p.stats(Cd)
    a, c = _out(csr.n, cuda)
    p.point_cost_csr(rp, ci, v, row_norms_csr(rp, v), Cd, row_norms(Cd), a, c)
    _eq(a, ref.na)
    _eq(c, ref.nc)
    p.close()


def check_accumulate(cuda, measure, d, C, shards, prior=None, update=False):
    """accumulate_csr of every (csr, weights, ref) shard in turn into the same
    buffers, which start as `prior` (zeros by default)."""
    import torch
    from cycloneml_amd.clustering import KMeansPlan, row_norms, row_norms_csr
    k = C.shape[0]
    kd = k * d
    prior = np.zeros(kd + k + 1) if prior is None else prior
    Cd = _dev(C, cuda)
    cn = row_norms(Cd)
    p = KMeansPlan(d, k, max(s[0].n for s in shards), measure)
    devs = [(csr.dev(cuda), None if w is None else _dev(w, cuda)) for csr, w, _ in shards]

    def run():
        buf = _dev(prior, cuda).clone()
        outs = []
        for (rp, ci, v), wd in devs:
            a, c = _out(rp.shape[0] - 1, cuda)
            p.accumulate_csr(rp, ci, v, row_norms_csr(rp, v), wd, Cd, cn, buf[:kd],
                             buf[kd:kd + k], buf[kd + k:], assign=a, cost=c)
            outs.append((a, c))
        torch.cuda.synchronize()
        return buf, outs

    buf, outs = run()
    for (a, c), (_, _, ref) in zip(outs, shards):
        _eq(a, ref.a)
        _eq(c, ref.c)
    calls = [terms(measure, csr, d, w, ref) for csr, w, ref in shards]
    b = buf.cpu().numpy()
    touched = (check_entries(b[:kd], prior[:kd], [t[0] for t in calls], "sums"),
               check_entries(b[kd:kd + k], prior[kd:kd + k], [t[1] for t in calls], "wsum"),
               check_entries(b[kd + k:], prior[kd + k:], [t[2] for t in calls], "cost sum"))
    assert torch.equal(run()[0], buf)             # fixed-order folds: run to run
    if update:
        conv = torch.zeros(1, dtype=torch.int32, device=cuda)
        p.update(Cd, cn, buf[:kd], buf[kd:kd + k], 1e-4, conv)
        Ch, cnh = C.copy(), oracle.row_norms(C)
        upd = oracle.update_centers if measure == EUC else oracle.cos_update_centers
        rconv = upd(Ch, cnh, b[:kd], b[kd:kd + k], 1e-4)
        _eq(Cd, Ch)
        _eq(cn, cnh)
        assert bool(conv.item()) == rconv
    p.close()
    return touched


def pattern(size, seed):
    """A non-zero prior content of mixed sign and magnitude."""
    rng = np.random.default_rng(seed)
    return rng.normal(size=size) * 10.0 ** rng.integers(-3, 4, size)


# -------------------------------------------------------------------- tests
@pytest.mark.parametrize("measure", [EUC, COS])
@pytest.mark.parametrize("k", K_STATS)
def test_center_tiles_with_stats(cuda, measure, k):
    """Case 1: tiles 1..64, 65..128, 129.. after center 0."""
    csr, C, w, ref = tile_case(measure, k, True)
    if measure == EUC:                          # the per-row reference, row by row
        st = oracle.kmeans_stats(C)
        for r in range(csr.n):
            s, e = csr.rp[r], csr.rp[r + 1]
            assert oracle.find_closest_stats_sparse(C, ref.cn, st, csr.colidx[s:e],
                                                    csr.values[s:e], ref.xn[r]) == \
                (ref.a[r], ref.c[r])
    check_assign(cuda, measure, D_TILE, C, csr, ref)
    check_accumulate(cuda, measure, D_TILE, C, [(csr, w, ref)], update=k == 66)
    check_accumulate(cuda, measure, D_TILE, C, [(csr, None, ref)])


@pytest.mark.parametrize("measure", [EUC, COS])
@pytest.mark.parametrize("k", K_NOSTATS)
def test_center_tiles_without_stats(cuda, measure, k):
    """Case 2: tiles 0..63, 64..127, 128.."""
    csr, C, _, ref = tile_case(measure, k, False)
    check_point_cost(cuda, measure, D_TILE, C, csr, ref, after_stats=True)
    check_point_cost(cuda, measure, D_TILE, C, csr, ref)      # stats never called


@pytest.mark.parametrize("measure", [EUC, COS])
def test_row_lengths(cuda, measure):
    """Case 3: rows of 0 (Euclidean) to 256 stored entries; k_sp_keys walks a
    row 64 entries at a time."""
    csr, C, w, ref, d = rowlen_case(measure)
    check_norms(cuda, csr, ref)
    check_assign(cuda, measure, d, C, csr, ref)
    check_point_cost(cuda, measure, d, C, csr, ref)
    check_accumulate(cuda, measure, d, C, [(csr, w, ref)])
    check_accumulate(cuda, measure, d, C, [(csr, None, ref)])


@pytest.mark.parametrize("measure", [EUC, COS])
@pytest.mark.parametrize("n", N_LAUNCH)
def test_launch_edges(cuda, measure, n):
    """Case 4: (n + 3) / 4 workgroups at n = 1, 3, 4, 5, 255, 257 and the
    second trip of the row loops at n = 32768 + 7."""
    csr, C, w, ref, d = launch_case(measure, n)
    check_norms(cuda, csr, ref)
    check_assign(cuda, measure, d, C, csr, ref)
    check_point_cost(cuda, measure, d, C, csr, ref)
    check_accumulate(cuda, measure, d, C, [(csr, w, ref)])


@pytest.mark.parametrize("measure", [EUC, COS])
def test_shard_view(cuda, measure):
    """Case 5: rowptr[300:701] of a 900-row CSR with the full colidx and
    values, against the oracle on the same view and against a rebased copy."""
    full, C, w, d = shard_case(measure)
    view = full.view(300, 700)
    assert view.rp[0] > 0
    copy = view.rebased()
    ref, ref2 = Ref(measure, view, d, C), Ref(measure, copy, d, C)
    for f in ("xn", "a", "c", "na", "nc"):      # the oracle itself: view == copy
        np.testing.assert_array_equal(getattr(ref, f), getattr(ref2, f))
    for csr in (view, copy):
        check_norms(cuda, csr, ref)
        check_assign(cuda, measure, d, C, csr, ref)
        check_point_cost(cuda, measure, d, C, csr, ref)
        check_accumulate(cuda, measure, d, C, [(csr, w[300:700], ref)])


@pytest.mark.parametrize("measure", [EUC, COS])
def test_accumulate_across_calls(cuda, measure):
    """Case 6: two accumulate_csr calls over two shard views into buffers
    pre-loaded with a non-zero pattern."""
    full, C, w, d = shard_case(measure)
    k = C.shape[0]
    shards = []
    for lo, hi in ((0, 450), (450, 900)):
        v = full.view(lo, hi)
        shards.append((v, w[lo:hi], Ref(measure, v, d, C)))
    for v, _, ref in shards:                    # both calls reach every near center
        all_hit(ref.a, k, never=(k - 1,))
    prior = pattern(k * d + k + 1, 6)
    ts, tw, _ = check_accumulate(cuda, measure, d, C, shards, prior=prior)
    # column d - 1 and cluster k - 1 get no term: their pre-loaded bits stay
    assert not ts.reshape(k, d)[:, d - 1].any() and not ts[(k - 1) * d:].any()
    assert not tw[k - 1] and tw[:k - 1].all()


@pytest.mark.parametrize("measure", [EUC, COS])
def test_empty_clusters_and_degenerate_weights(cuda, measure):
    """Case 7: clusters without a row, weights of exactly 0.0 and 1.0,
    explicit stored zeros."""
    csr, C, w, ref, d = degenerate_case(measure)
    prior = pattern(9 * d + 9 + 1, 7)
    ts, tw, _ = check_accumulate(cuda, measure, d, C, [(csr, w, ref)], prior=prior)
    assert not ts[6 * d:].any() and not tw[6:].any() and tw[:6].all()
    check_accumulate(cuda, measure, d, C, [(csr, w, ref)])


def test_all_rows_empty(cuda):
    """Case 7, second part: no stored entry at all (cluster_sums skips the
    sums' sort); the sums keep their prior bits."""
    csr, C, w, ref, d = empty_case()
    k = C.shape[0]
    check_norms(cuda, csr, ref)
    ts, tw, _ = check_accumulate(cuda, EUC, d, C, [(csr, w, ref)], prior=pattern(k * d + k + 1, 8))
    assert not ts.any() and tw.sum() == 1
    check_accumulate(cuda, EUC, d, C, [(csr, None, ref)])


@pytest.mark.parametrize("k,d", KD)
def test_key_widths(cuda, k, d):
    """Case 8: a dropped top key bit would merge two entries of the sums."""
    csr, C, w, ref = keywidth_case(k, d)
    check_accumulate(cuda, EUC, d, C, [(csr, w, ref)])
