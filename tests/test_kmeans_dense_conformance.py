"""Conformance tests of the dense Euclidean KMeans Lloyd call over a row image
(KMeansPlan.rows + accumulate / update) at the tile, list and tier edges of
kmeans.hip, kmeans_i8*.hip, kmeans_fp64.hip and kmeans_sums.hip, at the
smallest shapes that reach them.

Bars (all derived, none measured):
  * assignments and per-row costs: bit-exact against the C oracle, every row;
  * wsum with unit weights: bit-exact (counts are exact integers);
  * sums, weighted wsum and the cost sum: entry by entry within the bound
    that check_entries (sum_bounds.py) derives from the terms of that entry
    alone, m * 2**-53 * sum|t|;
  * the incremental sums: the same plus 2**-40 * sum|t| per entry, the guard
    under which the path keeps its result (kmeans_sums.hip, the comment above
    kIncRows: "When the bound exceeds 2^-40 of the cost ... the call runs the
    full pass", lines 502-503, enforced by k_inc_check, lines 856-858 and 875);
  * a second identical call on a fresh plan: torch.equal on every output;
  * update after accumulate: bit-exact against the oracle's update fed the
    device's own sums and weights (centers, norms, convergence flag).

The terms (terms() below) are built as the kernels build them: sums fold
w * x (x itself with unit weights); the cost sum folds cost * w per row when
per-row costs are asked for or d > 1024 (k_chunk_sums, k_chunk_sums_nocost),
and w * (c_j - x_j)^2 per row and column otherwise (k_chunk_sums_fast).

Every case is built on the host by a cached function that also asserts, on
the reference alone, that its inputs reach the edge it is about;
host_cases() lists them and test_host_cases walks them without a device.

Two edges of the issue's list cannot be reached through the dense entry
points and are pinned as the library's refusal instead: d = 1280 / 1281
(kExactX) lie beyond d = 1216, the widest row the LDS-resident assign kernels
take (d = 1216 / 1217 is the edge that exists, and is crossed here; the
library named 1240 until this file met the refusal at 1240 itself), and
k = 8193 is refused when the plan is created.
"""
import functools
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
from sum_bounds import U, check_entries

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC_ALLOWANCE = 2.0 ** -40          # kmeans_sums.hip:502-503, :856-858


# --------------------------------------------------------------------- host
class Ref:
    """The oracle's Lloyd call for (X, C): norms, statistics, findClosest for
    every row (a, c) and the partition's own sums, weights and cost."""

    def __init__(self, X, C, w=None):
        self.xn, self.cn = oracle.row_norms(X), oracle.row_norms(C)
        self.a, self.c, self.sums, self.wsum, self.cost = oracle.kmeans_partition(
            X, self.xn, w, C, self.cn, oracle.kmeans_stats(C))

    def next_centers(self, C):
        C2, cn2 = C.copy(), self.cn.copy()
        oracle.update_centers(C2, cn2, self.sums, self.wsum)
        return C2


def terms(X, C, w, a, c, per_row):
    """The terms the device folds into (sums, wsum, cost sum), as (entry
    index, term) arrays; see the module docstring."""
    n, d = X.shape
    a64 = a.astype(np.int64)
    wr = np.ones(n) if w is None else np.asarray(w, np.float64)
    keys = (a64[:, None] * d + np.arange(d)[None, :]).ravel()
    t = X.ravel() if w is None else (wr[:, None] * X).ravel()
    if per_row or d > 1024:
        cost = (np.zeros(n, np.int64), c * wr)
    else:
        df = C[a] - X
        q = df * df
        if w is not None:
            q = wr[:, None] * q
        cost = (np.zeros(n * d, np.int64), q.ravel())
    return (keys, t), (a64, wr), cost


def gaps(X, C):
    """Per row (best, runner-up) squared distance in plain numpy (sizing of
    conditions only; never compared with the device)."""
    D = ((X * X).sum(1)[:, None] - 2.0 * X @ C.T + (C * C).sum(1)[None, :])
    D.sort(axis=1)
    return np.maximum(D[:, 0], 0.0), D[:, 1]


def blobs(n, d, k, seed, hard=None):
    """k centers on a 3.0 grid in coordinate 0 (any d keeps them apart) and
    N(0, 4^2) elsewhere; rows are 0.25-sigma blobs around the centers taken in
    turn, none of them a center.  Then
      * centers a = 0 and b = k - 1 differ in coordinate 0 alone, by 3.0, so
        a + 1.5 there is an exact tie (both squared distances are 2.25) that
        crosses every center tile; one ulp either side is a near tie;
      * center k - 2 is a copy of center 1 (k >= 4) and can never win: the
        reference replaces its best only on a strict `<`;
      * `hard` rows (default n / 16, none below 16 rows), spread evenly from
        row 0 to row n - 1, are in turn a center itself, the exact tie and
        the two near ties.
    Returns X, C and the hard rows' indices by kind."""
    rng = np.random.default_rng(seed)
    C = rng.normal(scale=4.0, size=(k, d))
    g = rng.permutation(k).astype(np.float64)
    a, b = 0, k - 1

    def put(idx, val):
        j = int(np.flatnonzero(g == val)[0])
        g[j], g[idx] = g[idx], g[j]

    if k >= 2:
        put(a, 0.0)
        put(b, 1.0)
    C[:, 0] = 3.0 * g
    if k >= 2:
        C[b, 1:] = C[a, 1:]
    dup = None
    if k >= 4:
        dup = k - 2
        C[dup] = C[1]
    live = [j for j in range(k) if j != dup]
    if hard is None:
        hard = n // 16 if n >= 16 else 0
    hpos = np.unique(np.linspace(0, n - 1, hard).round().astype(np.int64)) if hard else \
        np.zeros(0, np.int64)
    X = np.empty((n, d))
    soft = np.setdiff1d(np.arange(n), hpos)
    own = np.array([live[q % len(live)] for q in range(len(soft))], dtype=np.int64)
    X[soft] = C[own] + 0.25 * rng.normal(size=(len(soft), d))
    kinds = {"center": [], "tie": [], "near": []}
    for q, r in enumerate(hpos.tolist()):
        kind = q % 4 if k >= 2 else 0
        if kind == 0:
            X[r] = C[live[(q // 4) % len(live)]]
            kinds["center"].append(r)
        else:
            X[r] = C[a]
            m = C[a, 0] + 1.5
            X[r, 0] = m if kind == 1 else np.nextafter(m, np.inf if kind == 2 else -np.inf)
            kinds["tie" if kind == 1 else "near"].append(r)
    return X, C, own, dup, kinds


@functools.lru_cache(maxsize=None)
def blob_case(n, d, k, hard=None, seed=0):
    """blobs() with its reference and the conditions on the inputs: every
    center that owns a blob row is some row's result and the copy is no
    row's (so with k > n fewer than k centers are hit, asserted); a row that
    is a center costs exactly 0.0; an exact tie has bit-equal distances to
    centers 0 and k - 1 and goes to 0; a near tie has distances one rounding
    apart."""
    X, C, own, dup, kinds = blobs(n, d, k, 1000 * d + 10 * k + n + seed, hard)
    ref = Ref(X, C)
    hit = set(ref.a.tolist())
    want = set(own.tolist())
    assert want <= hit, f"centers no row lands on: {sorted(want - hit)[:8]}"
    assert dup is None or dup not in hit
    if k > n:
        assert len(hit) < k
    elif len(own) >= k:
        assert len(hit) == k - (dup is not None)
    for r in kinds["center"]:
        assert ref.c[r] == 0.0
    for r in kinds["tie"] + kinds["near"]:
        d0, d1 = oracle.sqdist(C[0], X[r]), oracle.sqdist(C[k - 1], X[r])
        if r in kinds["tie"]:
            assert d0 == d1 == 2.25 and ref.a[r] == 0
        else:
            assert d0 != d1 and abs(d0 - d1) <= 8 * U * 2.25 * max(1.0, abs(C[0, 0]))
            assert ref.a[r] == (0 if d0 < d1 else k - 1)
    return X, C, ref, kinds


N_ROWS = (1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097)
DK_ROWS = ((8, 5), (32, 97))
K_CENTERS = (1, 2, 31, 32, 33, 96, 97, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024,
             1025, 4095, 4096, 4097)
N_CENTERS, D_CENTERS = 520, 8
D_WIDTH = (1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 252, 255, 256, 257, 260, 511, 512, 513, 1024,
           1025, 1216)
D_REFUSED = (1217, 1240, 1280, 1281)
N_WIDTH = 257


def centers_case(k):
    """n = 520, d = 8: 512 blob rows give each of the first 512 centers that
    own a blob a row, 8 hard rows."""
    return blob_case(N_CENTERS, D_CENTERS, k, 8)


CHUNK_SIZES = (255, 256, 257, 511, 512, 513, 1)


@functools.lru_cache(maxsize=None)
def chunk_case():
    """Clusters of exactly 255, 256, 257, 511, 512, 513 and 1 rows (kChunkRows
    = 256 rows per partial sum), interleaved in row order; d = 8, k = 8 with
    center 7 far from every row."""
    rng = np.random.default_rng(256)
    k, d = 8, 8
    C = rng.normal(scale=4.0, size=(k, d))
    C[:, 0] = 3.0 * np.arange(k)
    C[7] = 500.0
    own = rng.permutation(np.repeat(np.arange(7), CHUNK_SIZES))
    X = C[own] + 0.25 * rng.normal(size=(len(own), d))
    ref = Ref(X, C)
    assert tuple(np.bincount(ref.a, minlength=k)) == CHUNK_SIZES + (0,)
    return X, C, ref, rng.uniform(0.1, 2.0, len(own))


QUEUED = (511, 512, 513)


@functools.lru_cache(maxsize=None)
def queue_case(q):
    """q rows whose two nearest centers are the identical centers 1 and 4
    (no margin separates bit-equal distances: they must be queued for the
    exact tier, kExactCap = 512), 30 rows around each other center, d = 8,
    k = 6.  Every other row's runner-up is at least 4 times as far (squared)
    as its center, far beyond the screens' 2^-19 relative margins, so q is
    the queue's length.  That no screen queues a well separated row is the
    screens' contract, not provable from the reference; the device test
    asserts it as n_exact == q."""
    rng = np.random.default_rng(q)
    k, d = 6, 8
    C = rng.normal(scale=4.0, size=(k, d))
    C[:, 0] = 3.0 * np.arange(k)
    C[4] = C[1]
    own = rng.permutation(np.concatenate([np.full(q, 1), np.repeat([0, 2, 3, 5], 30)]))
    X = C[own] + 0.25 * rng.normal(size=(len(own), d))
    ref = Ref(X, C)
    assert int((ref.a == 1).sum()) == q and not (ref.a == 4).any()
    best, second = gaps(X, np.delete(C, 4, axis=0))
    assert (second >= 4.0 * best).all()
    return X, C, ref


@functools.lru_cache(maxsize=None)
def cands_case():
    """The near ties of test_three_limb_candidate_tier at n = 4097: close
    clusters (d = 64, k = 128), the centers rows of X, ten of them copies of
    ten others shifted by 1e-9.  Rows whose two nearest centers are such a
    pair are closer than the candidate pass's 2^-30 relative margin
    (kmeans.hip cand_args), so the two-limb tiers cannot decide them.  Which
    tier after that certifies a row is not provable from the reference; the
    device test asserts the counters."""
    n, d, k = 4097, 64, 128
    rng = np.random.default_rng(n + d + k + 7)
    true_c = rng.normal(scale=1.5, size=(k, d))
    X = true_c[rng.integers(0, k, n)] + rng.normal(size=(n, d))
    C = X[:k].copy()
    C[k // 2:k // 2 + 10] = C[:10] + 1e-9
    ref = Ref(X, C)
    best, second = gaps(X, C)
    assert int(((second - best) <= 2.0 ** -30 * second).sum()) >= 10
    return X, C, ref


@functools.lru_cache(maxsize=None)
def extreme_case(k):
    """n = 257, d = 32: center 3 at 1e20 and center 5 at 1e-40 (beyond the
    image's exponent range kMinExp / kMaxExp = -50 / 50), an all-zero row, a
    row equal to a center, and +-0.0 entries in a tenth of the rows."""
    X, C, _, _, kinds = blobs(257, 32, k, 77 + k)
    rng = np.random.default_rng(k)
    C[3] = rng.normal(size=32) * 1e20
    C[5] = rng.normal(size=32) * 1e-40
    X[100] = 0.0
    X[101] = C[6]
    X[102] = C[5]
    z = rng.choice(257, size=26, replace=False)
    X[z, 4] = 0.0
    X[z, 5] = -0.0
    ref = Ref(X, C)
    assert ref.c[101] == 0.0 and ref.a[101] == 6 and ref.a[100] == 5 and ref.a[102] == 5
    assert np.signbit(X[z, 5]).all() and not (ref.a == 3).any()
    return X, C, ref


@functools.lru_cache(maxsize=None)
def weighted_case(n, d, k):
    """Weights in [0.1, 2) with a tenth exactly 0.0 and a fifth exactly 1.0."""
    X, C, _, kinds = blob_case(n, d, k)
    rng = np.random.default_rng(n + d + k)
    w = rng.uniform(0.1, 2.0, n)
    u = rng.random(n)
    w[u < 0.1] = 0.0
    w[u > 0.8] = 1.0
    assert (w == 0.0).sum() >= 5 and (w == 1.0).sum() >= 5
    return X, C, w, Ref(X, C, w)


LLOYD_SHAPES = ((4097, 32, 130, 1.5), (2049, 256, 257, 1.2))


def _hook(seq, it, C, X):
    if seq == "moved":
        if it == 2:
            C[7] += 5.0                         # one center jumps
        elif it == 3:
            C[[1, 2]] = C[[2, 1]]               # two centers swap indices
        elif it == 4:
            C[12] = C[11]                       # identical centers: 12 empties
    elif seq == "inc":
        if it == 4:
            C[7] = X[40]                        # onto a row of another cluster
        elif it == 6:
            C[12] = C[11]                       # a duplicate: 12 empties


@functools.lru_cache(maxsize=None)
def lloyd_case(n, d, k, sep, seq):
    """Lloyd iterations from centers that are rows of close clusters, the
    last row an outlier that is center k - 1 (a cluster of exactly one row).
    The centers of every iteration are the reference's own (its update of its
    own sums), changed between iterations by _hook; the device is handed the
    same centers, so the reference of each iteration is computed once, here.
    seq: "lloyd" (six iterations), "moved" (six, a center jumps, two swap, two
    become identical), "inc" (eight: the incremental sums' conditions, from
    the reference's assignments: some iteration moves more than n / 16 rows,
    a late one between 1 and n / 16, and the iteration that makes center 12 a
    copy of 11 moves at most n / 16 and leaves cluster 12 without a row)."""
    rng = np.random.default_rng(n + d + k)
    true_c = rng.normal(scale=sep, size=(k, d))
    X = true_c[rng.integers(0, k, n)] + rng.normal(size=(n, d))
    X[n - 1] = 30.0 + rng.normal(size=d)
    C = X[:k].copy()
    C[k - 1] = X[n - 1]
    Cs, refs = [], []
    for it in range(8 if seq == "inc" else 6):
        _hook(seq, it, C, X)
        ref = Ref(X, C)
        Cs.append(C.copy())
        refs.append(ref)
        C = ref.next_centers(C)
        assert ref.wsum[k - 1] == 1.0 and ref.a[n - 1] == k - 1
    moved = [int((refs[t].a != refs[t - 1].a).sum()) for t in range(1, len(refs))]
    if seq == "inc":
        cap = n // 16
        assert any(m > cap for m in moved), moved
        assert any(1 <= m <= cap for m in moved[3:]), moved
        assert 1 <= moved[5] <= cap and refs[5].wsum[12] > 0 and refs[6].wsum[12] == 0.0, moved
    if seq == "moved":
        assert moved[1] > 0 and moved[2] > 0 and moved[3] > 0 and refs[4].wsum[12] == 0.0
    return X, Cs, refs, moved


def host_cases():
    """Every case's host half (inputs, reference, conditions on the inputs)."""
    for d, k in DK_ROWS:
        for n in N_ROWS:
            yield blob_case, (n, d, k)
    for k in K_CENTERS + (8192,):
        yield centers_case, (k,)
    for d in D_WIDTH:
        yield blob_case, (N_WIDTH, d, 33)
        if d <= 257:
            yield blob_case, (N_WIDTH, d, 130)
    yield chunk_case, ()
    for q in QUEUED:
        yield queue_case, (q,)
    yield cands_case, ()
    for k in (33, 130):
        yield extreme_case, (k,)
    yield weighted_case, (257, 33, 33)
    yield weighted_case, (520, 32, 130)
    for shape in LLOYD_SHAPES:
        for seq in ("lloyd", "moved", "inc"):
            yield lloyd_case, shape + (seq,)


def test_host_cases():
    """Without a device: every builder's conditions on its inputs hold."""
    seen = 0
    for fn, args in host_cases():
        fn(*args)
        seen += 1
    assert seen >= 2 * len(N_ROWS) + len(K_CENTERS) + len(D_WIDTH) + 10


# ------------------------------------------------------------------- device
def _dev(a, cuda, offset=0):
    """a on the device; offset: that many doubles past an allocation's start
    (1: 8 bytes past a 16-byte boundary, 2: 16 bytes past a 32-byte one)."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a))
    if not offset:
        return t.to(cuda)
    buf = torch.empty(t.numel() + offset, dtype=t.dtype, device=cuda)
    out = buf[offset:].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 32 == 8 * offset
    return out


def _eq(t, ref, what=""):
    np.testing.assert_array_equal(t.cpu().numpy(), ref, err_msg=what)


def accumulate(cuda, X, C, w=None, per_row=True, offset=0, state=None):
    """One accumulate over a row image into zeroed buffers.  state: (plan,
    rows, Xd, xn) of an earlier call of the same fit, else a fresh plan.
    Returns (assign, cost or None, buf = sums | wsum | cost sum, state)."""
    import torch
    from cycloneml_amd.clustering import KMeansPlan, row_norms
    n, d = X.shape
    k = C.shape[0]
    if state is None:
        Xd = _dev(X, cuda, offset)
        p = KMeansPlan(d, k, n)
        state = (p, p.rows(Xd), Xd, row_norms(Xd))
    p, rows, Xd, xn = state
    Cd = _dev(C, cuda)
    wd = None if w is None else _dev(w, cuda)
    a = torch.full((n,), -1, dtype=torch.int32, device=cuda)
    c = torch.full((n,), float("nan"), dtype=torch.float64, device=cuda) if per_row else None
    buf = torch.zeros(k * d + k + 1, dtype=torch.float64, device=cuda)
    p.accumulate(Xd, xn, wd, Cd, row_norms(Cd), buf[:k * d], buf[k * d:k * d + k], buf[k * d + k:],
                 a, c, rows=rows)
    torch.cuda.synchronize()
    return a, c, buf, state


def check_outputs(X, C, w, ref, a, c, buf, what="", allowance=0.0):
    """One call's outputs against the reference, by the module's bars."""
    n, d = X.shape
    k = C.shape[0]
    kd = k * d
    bad = np.flatnonzero(a.cpu().numpy() != ref.a)
    assert bad.size == 0, f"{what}: {bad.size} assignments differ, first rows {bad[:10]}"
    if c is not None:
        _eq(c, ref.c, f"{what}: per-row cost")
    b = buf.cpu().numpy()
    ts, tw, tc = terms(X, C, w, ref.a, ref.c, c is not None)
    zero = np.zeros(kd + k + 1)
    check_entries(b[:kd], zero[:kd], [ts], f"{what}: sums", allowance)
    if w is None:
        np.testing.assert_array_equal(b[kd:kd + k], np.bincount(ref.a, minlength=k).astype(float),
                                      err_msg=f"{what}: wsum")
    else:
        check_entries(b[kd:kd + k], zero[:k], [tw], f"{what}: wsum")
    check_entries(b[kd + k:], zero[:1], [tc], f"{what}: cost sum", allowance)


def check_update(cuda, C, buf, state):
    """update on the device's own sums and weights against the oracle's."""
    import torch
    from cycloneml_amd.clustering import row_norms
    k, d = C.shape
    Cd = _dev(C, cuda)
    cn = row_norms(Cd)
    conv = torch.zeros(1, dtype=torch.int32, device=cuda)
    state[0].update(Cd, cn, buf[:k * d], buf[k * d:k * d + k], 1e-4, conv)
    b = buf.cpu().numpy()
    Ch, cnh = C.copy(), oracle.row_norms(C)
    rconv = oracle.update_centers(Ch, cnh, b[:k * d], b[k * d:k * d + k], 1e-4)
    _eq(Cd, Ch, "updated centers")
    _eq(cn, cnh, "updated norms")
    assert bool(conv.item()) == rconv


def check_call(cuda, X, C, ref, w=None, per_row=True, offset=0, what=""):
    """A Lloyd call on a fresh plan by every bar, a second one on another
    fresh plan bit-equal to it, and update.  Returns the first call's state."""
    import torch
    a, c, buf, state = accumulate(cuda, X, C, w, per_row, offset)
    check_outputs(X, C, w, ref, a, c, buf, what)
    a2, c2, buf2, _ = accumulate(cuda, X, C, w, per_row, offset)
    assert torch.equal(a, a2) and torch.equal(buf, buf2)
    assert c is None or torch.equal(c, c2)
    check_update(cuda, C, buf, state)
    return state


def lloyd_device(cuda, X, Cs, bounds=True, per_row=True):
    """The centers Cs in turn through one plan and one row image; per
    iteration (assign, cost, buf) on the host and the incremental calls so
    far; then (bounds_info, incremental_info)."""
    state, out = None, []
    for C in Cs:
        if state is None:
            import torch
            from cycloneml_amd.clustering import KMeansPlan, row_norms
            Xd = _dev(X, cuda)
            p = KMeansPlan(X.shape[1], C.shape[0], X.shape[0])
            rows = p.rows(Xd)
            rows.set_bounds(bounds)
            state = (p, rows, Xd, row_norms(Xd))
        a, c, buf, state = accumulate(cuda, X, C, None, per_row, state=state)
        inc = 0 if per_row else state[1].incremental_info()[0]
        out.append((a.cpu().numpy(), None if c is None else c.cpu().numpy(), buf.cpu().numpy(), inc))
    return out, state[1].bounds_info(), state[1].incremental_info()


def digest(out):
    h = hashlib.sha256()
    for a, c, buf, _ in out:
        for x in (a, c, buf):
            h.update(np.ascontiguousarray(x).tobytes())
    return h.hexdigest()


class _Np:
    """A host array with the .cpu().numpy() of a device tensor."""

    def __init__(self, a):
        self.a = a

    def cpu(self):
        return self

    def numpy(self):
        return self.a


def check_lloyd(X, Cs, refs, out, what, inc_path=False):
    prev = 0
    for it, (C, ref, (a, c, buf, inc)) in enumerate(zip(Cs, refs, out)):
        allowance = INC_ALLOWANCE if inc_path and inc > prev else 0.0
        prev = inc
        check_outputs(X, C, None, ref, _Np(a), None if c is None else _Np(c), _Np(buf),
                      f"{what}, iteration {it}", allowance)


# -------------------------------------------------------------------- tests
@gpu
@pytest.mark.parametrize("d,k", DK_ROWS)
@pytest.mark.parametrize("n", N_ROWS)
def test_row_edges(cuda, n, d, k):
    """Rows either side of the 32-row MFMA tile, kBM = 64, kRcBatch =
    kChunkRows = 256, kBndRows = kIncRows = 2048 and kSortTile = 4096; (8, 5)
    runs the two-limb pass over every center without bounds, (32, 97) the
    one-limb pass, refinement and bounds.  n = 1 and n < k: no center is a
    row."""
    X, C, ref, _ = blob_case(n, d, k)
    state = check_call(cuda, X, C, ref, what=f"n={n}")
    assert state[1].bounds_info() == ((1, n) if k > 96 else (0, 0))
    check_call(cuda, X, C, ref, per_row=False, what=f"n={n}, no row costs")


@gpu
@pytest.mark.parametrize("k", K_CENTERS)
def test_center_edges(cuda, k):
    """Centers either side of the 32-center tile, refine_on's k > 96 and
    tiles32(k) * 32 <= 4096, kExactCap = 512 and kExactChunk = 1024.  The
    one-limb pass and the bounds are off at 96, on at 97 and 4096, off at
    4097."""
    X, C, ref, _ = centers_case(k)
    state = check_call(cuda, X, C, ref, what=f"k={k}")
    on = 96 < k <= 4096
    assert state[1].bounds_info() == ((1, N_CENTERS) if on else (0, 0))
    assert (state[0].last_refine()[0] >= 0) == on
    check_call(cuda, X, C, ref, per_row=False, what=f"k={k}, no row costs")


@gpu
def test_center_limit(cuda):
    """kMaxK = 8192 on assign: 8192 centers work, 8193 are refused when the
    plan is created."""
    import torch
    from cycloneml_amd import _native as N
    from cycloneml_amd.clustering import KMeansPlan, row_norms
    X, C, ref, _ = centers_case(8192)
    Xd, Cd = _dev(X, cuda), _dev(C, cuda)
    p = KMeansPlan(D_CENTERS, 8192, N_CENTERS)
    p.stats(Cd)
    a = torch.full((N_CENTERS,), -1, dtype=torch.int32, device=cuda)
    c = torch.full((N_CENTERS,), float("nan"), dtype=torch.float64, device=cuda)
    p.assign(Xd, row_norms(Xd), Cd, row_norms(Cd), a, c, rows=p.rows(Xd))
    _eq(a, ref.a)
    _eq(c, ref.c)
    with pytest.raises(N.CycloneError, match="k > 8192 is not supported"):
        KMeansPlan(D_CENTERS, 8193, N_CENTERS)


@gpu
@pytest.mark.parametrize("d", D_WIDTH)
def test_width_edges(cuda, d):
    """Widths either side of the quantiser's forms (d % 4, 32-byte rows),
    uses32's d <= 256, kMaxD = 512 (no image beyond it), the fused costs' d
    <= 1024 and the assign kernels' d <= 1216; k = 33, and k = 130 (one-limb
    pass and bounds) for d <= 257."""
    for k in (33, 130) if d <= 257 else (33,):
        X, C, ref, _ = blob_case(N_WIDTH, d, k)
        state = check_call(cuda, X, C, ref, what=f"d={d}, k={k}")
        assert state[1].bounds_info() == ((1, N_WIDTH) if k > 96 and d <= 256 else (0, 0))
        check_call(cuda, X, C, ref, per_row=False, what=f"d={d}, k={k}, no row costs")


@gpu
@pytest.mark.parametrize("d", D_REFUSED)
def test_width_refused(cuda, d):
    """d > 1216: the dense Lloyd call is refused with the library's message
    (so kExactX = 1280 is out of the dense entry points' reach)."""
    from cycloneml_amd import _native as N
    rng = np.random.default_rng(d)
    X, C = rng.normal(size=(N_WIDTH, d)), rng.normal(size=(33, d))
    with pytest.raises(N.CycloneError, match="d > 1216 is not supported"):
        accumulate(cuda, X, C)


@gpu
@pytest.mark.parametrize("d", [64, 255, 256])
@pytest.mark.parametrize("offset", [1, 2])
def test_width_unaligned_rows(cuda, d, offset):
    """Rows that start 8 bytes past a 16-byte boundary and 16 bytes past a
    32-byte one: the quantiser's three load forms."""
    X, C, ref, _ = blob_case(N_WIDTH, d, 33)
    check_call(cuda, X, C, ref, offset=offset, what=f"d={d}, offset={offset}")


@gpu
def test_chunk_edges(cuda):
    """Clusters of 255 .. 513 rows: one, two and three 256-row partial sums,
    with and without weights and per-row costs."""
    X, C, ref, w = chunk_case()
    for per_row in (True, False):
        check_call(cuda, X, C, ref, per_row=per_row, what=f"chunks, per_row={per_row}")
        check_call(cuda, X, C, Ref(X, C, w), w=w, per_row=per_row,
                   what=f"weighted chunks, per_row={per_row}")


def _assign_counted(cuda, X, C):
    import torch
    from cycloneml_amd.clustering import KMeansPlan, row_norms
    n, d = X.shape
    Xd, Cd = _dev(X, cuda), _dev(C, cuda)
    p = KMeansPlan(d, C.shape[0], n)
    p.stats(Cd)
    a = torch.full((n,), -1, dtype=torch.int32, device=cuda)
    c = torch.full((n,), float("nan"), dtype=torch.float64, device=cuda)
    n_exact = p.assign(Xd, row_norms(Xd), Cd, row_norms(Cd), a, c, count_exact=True,
                       rows=p.rows(Xd))
    torch.cuda.synchronize()
    return p, a, c, n_exact


@gpu
@pytest.mark.parametrize("d,k", DK_ROWS)
@pytest.mark.parametrize("n", N_ROWS)
def test_row_edges_assign(cuda, n, d, k):
    """The same row counts through assign over the image: the screens and the
    tiers alone, every row's index and cost."""
    X, C, ref, kinds = blob_case(n, d, k)
    _, a, c, n_exact = _assign_counted(cuda, X, C)
    _eq(a, ref.a)
    _eq(c, ref.c)
    assert n_exact >= len(kinds["tie"]) + len(kinds["near"])


@gpu
@pytest.mark.parametrize("n,d,k", [(257, 8, 5), (257, 32, 130), (520, 8, 513)])
def test_exact_tier_reached(cuda, n, d, k):
    """Exact ties, near ties one rounding apart and a duplicate center: at
    least the tie rows reach the exact tier."""
    X, C, ref, kinds = blob_case(n, d, k) if n != 520 else centers_case(k)
    _, a, c, n_exact = _assign_counted(cuda, X, C)
    _eq(a, ref.a)
    _eq(c, ref.c)
    assert n_exact >= len(kinds["tie"]) + len(kinds["near"]) > 0


@gpu
@pytest.mark.parametrize("q", QUEUED)
def test_exact_queue_at_cap(cuda, q):
    """kExactCap - 1, kExactCap and kExactCap + 1 queued rows."""
    X, C, ref = queue_case(q)
    _, a, c, n_exact = _assign_counted(cuda, X, C)
    _eq(a, ref.a)
    _eq(c, ref.c)
    assert n_exact == q
    check_call(cuda, X, C, ref, what=f"queue of {q}")


@gpu
@pytest.mark.parametrize("cands3", [None, "0"])
def test_three_limb_candidates(cuda, monkeypatch, cands3):
    """The three-limb candidate tier on (CYC_KMEANS_CANDS3 unset) and off."""
    if cands3 is None:
        monkeypatch.delenv("CYC_KMEANS_CANDS3", raising=False)
    else:
        monkeypatch.setenv("CYC_KMEANS_CANDS3", cands3)
    X, C, ref = cands_case()
    p, a, c, _ = _assign_counted(cuda, X, C)
    _eq(a, ref.a)
    _eq(c, ref.c)
    cand, fp64 = p.last_candidates(), p.last_candidates3()
    assert cand > 0
    assert fp64 == -1 if cands3 == "0" else 0 <= fp64 <= cand
    check_call(cuda, X, C, ref, what="near ties")


@gpu
@pytest.mark.parametrize("switch", ["CYC_KMEANS_NO_STAGE", "CYC_KMEANS_NO_REFINE", "both"])
@pytest.mark.parametrize("n", [63, 64, 65, 2047, 2048, 2049])
def test_staged_lists_off(cuda, monkeypatch, n, switch):
    """The screens appending straight to their lists, and no one-limb pass
    (so no bounds), at (d, k) = (32, 97)."""
    for name in ("CYC_KMEANS_NO_STAGE", "CYC_KMEANS_NO_REFINE"):
        if switch in (name, "both"):
            monkeypatch.setenv(name, "1")
    X, C, ref, _ = blob_case(n, 32, 97)
    state = check_call(cuda, X, C, ref, what=f"n={n}, {switch}")
    assert state[1].bounds_info() == ((1, n) if switch == "CYC_KMEANS_NO_STAGE" else (0, 0))


@gpu
@pytest.mark.parametrize("k", [33, 130])
def test_extreme_magnitudes(cuda, k):
    X, C, ref = extreme_case(k)
    check_call(cuda, X, C, ref, what=f"extremes, k={k}")
    check_call(cuda, X, C, ref, per_row=False, what=f"extremes, k={k}, no row costs")


@gpu
@pytest.mark.parametrize("n,d,k", [(257, 33, 33), (520, 32, 130)])
def test_weights(cuda, n, d, k):
    """Weights with exact 0.0 and 1.0; with weights, or with per-row costs,
    the incremental path is not taken (k = 130 carries bounds, so it could
    be)."""
    X, C, w, ref = weighted_case(n, d, k)
    for per_row in (True, False):
        state = check_call(cuda, X, C, ref, w=w, per_row=per_row, what=f"weighted {per_row}")
        a, c, buf, state = accumulate(cuda, X, C, w, per_row, state=state)
        check_outputs(X, C, w, ref, a, c, buf, "weighted, second call of the fit")
        assert state[1].incremental_info() == (0, 0)
    a, c, buf, state = accumulate(cuda, X, C, None, True)
    accumulate(cuda, X, C, None, True, state=state)
    assert state[1].incremental_info() == (0, 0)


@gpu
@pytest.mark.parametrize("seq", ["lloyd", "moved"])
@pytest.mark.parametrize("n,d,k,sep", LLOYD_SHAPES)
def test_carried_bounds(cuda, n, d, k, sep, seq):
    """Six iterations with the bounds on and off: bit-identical to each other
    and equal to the reference on every iteration's centers; the bounds
    spared rows the screen; update bit-exact on the last call's sums."""
    X, Cs, refs, _ = lloyd_case(n, d, k, sep, seq)
    on, (calls, screened), inc = lloyd_device(cuda, X, Cs, True)
    off, (calls_off, _), _ = lloyd_device(cuda, X, Cs, False)
    assert digest(on) == digest(off)
    check_lloyd(X, Cs, refs, on, f"{seq}, bounds on")
    assert calls == len(Cs) and calls_off == 0
    assert n <= screened < calls * n
    assert inc == (0, 0)                        # per-row costs: never incremental


@gpu
@pytest.mark.parametrize("n,d,k,sep", LLOYD_SHAPES)
def test_incremental_sums(cuda, n, d, k, sep):
    """Eight iterations without per-row costs: the incremental path is taken
    at least once, every iteration meets the bars (the path's own allowance
    only on the calls that took it), an emptied cluster weighs exactly 0.0
    and the one-row cluster exactly 1.0."""
    X, Cs, refs, moved = lloyd_case(n, d, k, sep, "inc")
    out, _, (inc_calls, inc_moved) = lloyd_device(cuda, X, Cs, True, per_row=False)
    check_lloyd(X, Cs, refs, out, f"incremental, moved {moved}", inc_path=True)
    assert inc_calls >= 1 and inc_moved >= 1, (inc_calls, inc_moved, moved)
    for a, _, buf, _ in out:
        assert buf[k * d + k - 1] == 1.0
    assert out[6][2][k * d + 12] == 0.0 and out[5][2][k * d + 12] > 0.0


_SWITCH_CHILD = r'''
import os, sys
import numpy as np, torch
root = os.getcwd()
for p in (root, os.path.join(root, "oracle"), os.path.join(root, "tests")):
    sys.path.insert(0, p)
import test_kmeans_dense_conformance as T
z = np.load(sys.argv[1])
out, _, _ = T.lloyd_device(torch.device("cuda", 0), z["X"], list(z["Cs"]), True)
print("digest", T.digest(out))
'''

SWITCHES = (None, "CYC_KMEANS_PREP=0", "CYC_KMEANS_RECHECK=1", "CYC_KMEANS_EXACT_SPLIT=0",
            "CYC_KMEANS_LIST_BM=0", "CYC_KMEANS_NBR=0")
_checked = {}


def _default_digest(cuda):
    """This process's run (the defaults), checked against the reference once."""
    if "d" not in _checked:
        X, Cs, refs, _ = lloyd_case(*LLOYD_SHAPES[0], "lloyd")
        out, _, _ = lloyd_device(cuda, X, Cs, True)
        check_lloyd(X, Cs, refs, out, "defaults")
        _checked["d"] = digest(out)
    return _checked["d"]


@gpu
@pytest.mark.parametrize("setting", SWITCHES)
def test_process_wide_switches(cuda, tmp_path, monkeypatch, setting):
    """The switches read once per process, each in a fresh child process (one
    at a time): the six-iteration (4097, 32, 130) fit gives the same bits as
    the defaults, in a child and in this process, where the outputs are
    checked against the reference."""
    names = [s.split("=")[0] for s in SWITCHES if s]
    assert not any(nm in os.environ for nm in names), "the defaults are this process's settings"
    want = _default_digest(cuda)
    X, Cs, _, _ = lloyd_case(*LLOYD_SHAPES[0], "lloyd")
    f = str(tmp_path / "case.npz")
    np.savez(f, X=X, Cs=np.stack(Cs))
    env = dict(os.environ)
    if setting:
        name, value = setting.split("=")
        env[name] = value
    r = subprocess.run([sys.executable, "-c", _SWITCH_CHILD, f], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    got = [ln.split()[1] for ln in r.stdout.splitlines() if ln.startswith("digest ")]
    assert got == [want], (setting, r.stdout[-500:])
