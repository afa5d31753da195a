"""The full pass behind the incremental sums' gate (kmeans_sums.hip,
k_*_gated: four launches, the small stages in the last workgroup to finish)
against the ungated full pass (incremental sums off), bit for bit: sums,
weights and cost of a call that opens the gate, of an incremental call on the
same assignments and centers (no moved row: the state's sums are the full
pass's, the cost correction is exactly zero), and of both once more on the
same plan (an arrival counter left non-zero would show there).  The gate is
used with carried bounds, 96 < k <= 4096 and d <= 256; the other shapes run
the ungated pass either way and must agree all the same."""
import functools
import os
import re

import numpy as np
import pytest

import test_kmeans_dense_conformance as conf

gpu = pytest.mark.gpu

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cycloneml_amd",
                    "csrc")


def _constant(name, *files):
    for f in files:
        with open(os.path.join(CSRC, f)) as fh:
            m = re.search(r"constexpr int %s = (\d+);" % name, fh.read())
        if m:
            return int(m.group(1))
    raise AssertionError(name)


CHUNK = _constant("kChunkRows", "kmeans_sums.hpp")
TILE = _constant("kSortTile", "kmeans_sums.hip")
SEGS = _constant("kScanSegs", "kmeans_sums.hip")

# (n, d, k): the row counts at k = 255 and 130, the cluster counts and widths
# at n = 4097, and one n past kScanSegs tiles (segments of two tiles, the last
# segment and the last tile part filled)
SHAPES = sorted({(n, 8, 255) for n in (1, 255, 256, 257, 4097, CHUNK - 1, CHUNK + 1, TILE - 1,
                                       TILE + 1)} |
                {(4097, 8, k) for k in (1, 2, 255, 257, 1024)} |
                {(4097, d, 130) for d in (1, 256, 257)} |
                {(SEGS * TILE + TILE + 1, 2, 130)})


def test_constants():
    assert (CHUNK, TILE, SEGS) == (256, 4096, 64)
    assert (1, 8, 255) in SHAPES and (SEGS * TILE + TILE + 1, 2, 130) in SHAPES


@functools.lru_cache(maxsize=None)
def _case(n, d, k, one_cluster=False):
    rng = np.random.default_rng(1000 * n + 10 * d + k)
    true_c = rng.normal(scale=3.0, size=(min(k, 40), d))      # k = 1024: many empty clusters
    X = true_c[rng.integers(0, true_c.shape[0], n)] + rng.normal(size=(n, d))
    C = rng.normal(scale=3.0, size=(k, d))
    C[:true_c.shape[0]] = true_c
    if one_cluster:
        C[:] = 1e3 + rng.normal(size=(k, d))
        C[k // 2] = X.mean(axis=0)
    return X, C


def _gated(d, k):
    return d <= 256 and 96 < k <= 4096


def _run(cuda, X, C, incremental, calls):
    """calls accumulate calls of one fit on the centers C (no per-row costs).
    Incremental sums on: a call that opens the gate, an incremental one, and
    so on in turn (the state is dropped before every even call).  Off: the
    plan's first call is not returned (a new row image has them on).
    Returns the calls' (assign, buf) and the incremental calls counted."""
    a, _, buf, state = conf.accumulate(cuda, X, C, None, False)
    out = [(a.cpu().numpy(), buf.cpu().numpy())] if incremental else []
    if not incremental:
        state[1].set_incremental(False)
    while len(out) < calls:
        if incremental and len(out) % 2 == 0:
            state[1].set_incremental(True)                     # drops the state
        a, _, buf, state = conf.accumulate(cuda, X, C, None, False, state=state)
        out.append((a.cpu().numpy(), buf.cpu().numpy()))
    return out, state[1].incremental_info()[0]


def _check(cuda, n, d, k, one_cluster=False):
    X, C = _case(n, d, k, one_cluster)
    ((ref_a, ref),), none = _run(cuda, X, C, False, 1)
    assert none == 0
    assert ref[k * d:k * d + k].sum() == n
    if one_cluster:
        assert ref[k * d + k // 2] == n
    out, inc_calls = _run(cuda, X, C, True, 4)
    for t, (a, buf) in enumerate(out):
        np.testing.assert_array_equal(a, ref_a, err_msg=f"call {t}: assignments")
        bad = np.flatnonzero(buf.view(np.uint64) != ref.view(np.uint64))
        assert bad.size == 0, (f"call {t} ({'incremental' if t % 2 else 'gated full pass'}): "
                               f"{bad.size} words differ, first {bad[:8]} of {k * d} sums, {k} "
                               f"weights, 1 cost")
    assert inc_calls == (2 if _gated(d, k) else 0)


@gpu
@pytest.mark.parametrize("n,d,k", SHAPES)
def test_gated_pass_equals_ungated(cuda, n, d, k):
    _check(cuda, n, d, k)


@gpu
def test_all_rows_in_one_cluster(cuda):
    _check(cuda, 4097, 8, 130, one_cluster=True)


@gpu
@pytest.mark.parametrize("n,d,k,sep", conf.LLOYD_SHAPES)
def test_gate_opens_mid_fit(cuda, n, d, k, sep):
    """The conformance suite's incremental fit (a call moves more than n / 16
    rows mid-fit and falls back to the full pass), with the incremental sums
    on and off: the same assignments, and every call that did not take the
    incremental path bit-equal to the ungated pass; twice on fresh plans."""
    X, Cs, refs, moved = conf.lloyd_case(n, d, k, sep, "inc")
    off = _fit(cuda, X, Cs, False)
    assert off[-1][2] == 0
    for rep in range(2):
        on = _fit(cuda, X, Cs, True)
        full = 0
        for t, ((a1, b1, i1), (a0, b0, _)) in enumerate(zip(on, off)):
            np.testing.assert_array_equal(a1, a0, err_msg=f"iteration {t}")
            if i1 == (on[t - 1][2] if t else 0):               # not an incremental call
                assert b1.tobytes() == b0.tobytes(), f"run {rep}, iteration {t}, moved {moved}"
                full += 1
        assert 2 <= full < len(Cs), (full, moved)              # the first call and one mid-fit


def _fit(cuda, X, Cs, incremental):
    state, out = None, []
    for C in Cs:
        a, _, buf, state = conf.accumulate(cuda, X, C, None, False, state=state)
        if len(out) == 0 and not incremental:                  # a new row image has them on
            state[1].set_incremental(False)
            a, _, buf, state = conf.accumulate(cuda, X, C, None, False, state=state)
        out.append((a.cpu().numpy(), buf.cpu().numpy(), state[1].incremental_info()[0]))
    return out
