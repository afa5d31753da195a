"""The two every-row passes of a carried Lloyd call, k_bounds_filter
(kmeans_i8_lists.hip) and k_inc_moved (kmeans_sums.hip), at the edges of
their row layout: a lane takes four consecutive rows, a step is 1024 rows, a
workgroup 2048, and the last rows of an n that is no multiple of 4 go element
by element.

Every case is a six-iteration fit (d = 32, k = 130) over one row image with
the carried bounds and the incremental sums on, the centers of each iteration
the reference's own, as in test_kmeans_dense_conformance.py, whose bars hold
here unchanged (all derived, none measured):
  * assignments bit-exact against the C oracle, every row, every iteration;
  * weights exact (unit weights: counts);
  * sums and the cost sum entry by entry within sum_bounds.check_entries,
    plus 2**-40 * sum|t| on the calls that took the incremental path;
  * a second fit with the full pass every step (set_incremental(False)):
    identical assignments at every iteration, final centers within the
    rtol = atol / max|C| = 1e-9 of test_kmeans_gpu.py::test_incremental_sums_fit.

The lists both passes build are order-sensitive (k_inc_part folds a cluster's
moved rows in list order), so the three largest cases also pin the bits of
(sums, weights, cost) of every iteration: DIGESTS below.
"""
import functools
import hashlib

import numpy as np
import pytest

import test_kmeans_dense_conformance as T

gpu = pytest.mark.gpu
D, K, ITERS = 32, 130, 6
N_ROWS = (1, 3, 4, 5, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 6145)
N_CLUMPS = 5003                     # three blocks, a ragged tail of three rows
CLUMP_LENGTHS = (1, 2, 3)

# sha256 over every iteration's (sums | weights | cost) of the first fit,
# recorded from commit 2475828 (the scalar one-row-per-lane passes): the
# same bits mean the same filter decisions and the same moved-list order.
DIGESTS = {
    (4097, False): "f712c48753ffb2c1f17df7eb98f8a5e3f9c525482b19ea3615d4b82052998578",
    (N_CLUMPS, True): "0aa81de6cd156feff3c813c9fbd09528e6fcfbb4e8f22a98a9534251d2ebb402",
    (6145, False): "3d3973b1aa1ca4bc7d8bff37947855262d1745e2f1bfa10694137dcfe12ad445",
}


def _iterate(X, C):
    Cs, refs = [], []
    for _ in range(ITERS):
        ref = T.Ref(X, C)
        Cs.append(C.copy())
        refs.append(ref)
        C = ref.next_centers(C)
    moved = [int((refs[t].a != refs[t - 1].a).sum()) for t in range(1, ITERS)]
    return Cs, refs, moved


@functools.lru_cache(maxsize=None)
def row_case(n):
    """n rows of k heavily overlapping clusters (spread 0.5, unit noise), so
    that rows go on moving for six iterations; the first centers are rows
    0..k-1 as in lloyd_case, or with n < k the clusters' own means disturbed
    by half the noise."""
    rng = np.random.default_rng(7000 + n)
    true_c = rng.normal(scale=0.5, size=(K, D))
    X = true_c[rng.integers(0, K, n)] + rng.normal(size=(n, D))
    C = X[:K].copy() if n >= K else true_c + 0.5 * rng.normal(size=(K, D))
    Cs, refs, moved = _iterate(X, C)
    if n >= 1023:
        # rows move at every iteration, and a late one moves few enough for
        # the incremental path (at most n / 16, kmeans_sums.hip kIncMovedFrac)
        assert all(m > 0 for m in moved), moved
        assert any(1 <= m <= n // 16 for m in moved[2:]), moved
    return X, Cs, refs, moved


@functools.lru_cache(maxsize=None)
def clump_case():
    """Rows in clumps of 1, 2 and 3 (lengths drawn at random), in turn
    "near" (within 1e-3 of a center: the carried bounds keep such a row) and
    "between" (within 1e-3 of the midpoint of two centers, both distances
    equal to 1e-3 of themselves: no bound survives any drift, the row is
    listed at every call).  Centers are ~30 apart.  Over the aligned groups of
    four rows every pattern a lane can see occurs except all-near and
    all-between, which clumps of at most 3 cannot give (asserted)."""
    n = N_CLUMPS
    rng = np.random.default_rng(99)
    C = rng.normal(scale=4.0, size=(K, D))
    between = np.zeros(n, bool)
    r, kind = 0, False
    while r < n:
        ln = int(rng.choice(CLUMP_LENGTHS))
        between[r:r + ln] = kind
        r, kind = r + ln, not kind
    a = rng.integers(0, K, n)
    b = (a + 1 + rng.integers(0, K - 1, n)) % K
    X = np.where(between[:, None], 0.5 * (C[a] + C[b]), C[a]) + 1e-3 * rng.normal(size=(n, D))
    groups = between[:n - n % 4].reshape(-1, 4) @ np.array([1, 2, 4, 8])
    assert set(groups.tolist()) == set(range(1, 15))
    for lane in range(64):          # every (lane, j) slot holds both kinds
        g = groups[lane::64]
        assert np.bitwise_or.reduce(g) == 15 and np.bitwise_and.reduce(g) == 0
    Cs, refs, moved = _iterate(X, C)
    # the between rows pull the centers, so later calls drift and rows move
    assert all(m > 0 for m in moved[:2]), moved
    return X, Cs, refs, moved, between


def fit(cuda, X, Cs, incremental):
    """Cs in turn through one plan and one row image with the bounds on and
    no per-row costs; per iteration (assign, None, buf, incremental calls so
    far), the centers update gives from the last call's sums, bounds_info,
    bounds_rechecked and incremental_info."""
    import torch
    from cycloneml_amd.clustering import KMeansPlan, row_norms
    n = X.shape[0]
    Xd = T._dev(X, cuda)
    p = KMeansPlan(D, K, n)
    rows = p.rows(Xd)
    rows.set_bounds(True)
    rows.set_incremental(incremental)
    state, out = (p, rows, Xd, row_norms(Xd)), []
    for C in Cs:
        a, _, buf, state = T.accumulate(cuda, X, C, None, False, state=state)
        out.append((a.cpu().numpy(), None, buf.cpu().numpy(), rows.incremental_info()[0]))
    Cd = T._dev(Cs[-1], cuda)
    conv = torch.zeros(1, dtype=torch.int32, device=cuda)
    p.update(Cd, row_norms(Cd), buf[:K * D], buf[K * D:K * D + K], 1e-4, conv)
    return out, Cd.cpu().numpy(), rows.bounds_info(), rows.bounds_rechecked(), \
        rows.incremental_info()


def digest(out):
    h = hashlib.sha256()
    for _, _, buf, _ in out:
        h.update(np.ascontiguousarray(buf).tobytes())
    return h.hexdigest()


def check_fits(cuda, X, Cs, refs, moved, what, key):
    n = X.shape[0]
    on, C_on, (calls, screened), rechecked, (inc_calls, inc_moved) = fit(cuda, X, Cs, True)
    print(f"{what}: moved {moved}, screened {screened}, rechecked {rechecked}, "
          f"incremental calls {inc_calls} rows {inc_moved}, digest {digest(on)}")
    T.check_lloyd(X, Cs, refs, on, what, inc_path=True)
    off, C_off, _, _, inc_off = fit(cuda, X, Cs, False)
    T.check_lloyd(X, Cs, refs, off, f"{what}, full pass")
    for it, (x, y) in enumerate(zip(on, off)):
        np.testing.assert_array_equal(x[0], y[0], err_msg=f"{what}: assign, iteration {it}")
    np.testing.assert_allclose(C_on, C_off, rtol=1e-9, atol=1e-9 * np.abs(C_off).max())
    assert calls == ITERS and inc_off == (0, 0)
    if n >= 1023:
        # the carried bounds kept rows, some listed rows were re-checked and
        # some screened: states 0, 1 and 2 / 3 all occurred; k_inc_moved's
        # list was folded at least once
        assert n <= screened < calls * n, (screened, n)
        assert rechecked > 0
        assert inc_calls >= 1 and inc_moved >= 1, (inc_calls, inc_moved, moved)
    if key in DIGESTS:
        assert digest(on) == DIGESTS[key], what
    return on


def test_host_cases():
    """Without a device: the builders' conditions on their inputs hold."""
    for n in N_ROWS:
        row_case(n)
    clump_case()
    assert sorted(k[0] for k in DIGESTS) == sorted((N_ROWS + (N_CLUMPS,)))[-3:]


@gpu
@pytest.mark.parametrize("n", N_ROWS)
def test_row_edges(cuda, n):
    X, Cs, refs, moved = row_case(n)
    check_fits(cuda, X, Cs, refs, moved, f"n = {n}", (n, False))


@gpu
def test_clumps(cuda):
    X, Cs, refs, moved, between = clump_case()
    check_fits(cuda, X, Cs, refs, moved, "clumps", (N_CLUMPS, True))
