"""Conformance tests of the row-blocked CSC copy (csrc/csc.hip,
cyc_csc_build_dev) at its row-block, lane-stride, empty-column and sort-width
edges, at the smallest shapes that reach them.

Bar: colptr, rowidx and values are integers or copied doubles, so all three
must equal the reference exactly (values as int64 words: NaN and -0.0 are
copies too).  The reference is numpy's stable argsort of the key
(row // 2^18) * F + col, which keeps each (row block, column)'s rows in
increasing order, and searchsorted for colptr (nblocks * F + 1 entries).

Every case is built on the host by a cached function; test_host_cases walks
them with the reference alone and asserts that each reaches the edge it is
named for.  The SparseVector refusals (Vectors.scala:617-625) are asserted by
message, the lowest offending row first; a rowptr that does not start at 0 is
refused (include/cyclone.h).
"""
import ctypes
import functools

import numpy as np
import pytest

gpu = pytest.mark.gpu
RB = 1 << 18          # kCscRowBlock


# --------------------------------------------------------------------- host
def reference(rp, ci, v, n, F):
    nb = max(-(-n // RB), 1)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    key = (rows // RB) * F + ci
    order = np.argsort(key, kind="stable")
    colptr = np.searchsorted(key[order], np.arange(nb * F + 1), side="left").astype(np.int64)
    return nb, colptr, rows[order].astype(np.int32), np.asarray(v, np.float64)[order]


def _csr(lens, F, rng, cols=None):
    """Rows of the given lengths with strictly increasing random columns
    (drawn from `cols`, all F columns by default) and normal values."""
    lens = np.asarray(lens, np.int64)
    cols = np.arange(F) if cols is None else np.asarray(cols)
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ci = np.empty(int(rp[-1]), np.int32)
    for r, m in enumerate(lens.tolist()):
        ci[rp[r]:rp[r + 1]] = np.sort(rng.choice(cols, size=m, replace=False))
    return rp, ci, rng.normal(size=int(rp[-1]))


N_ROWS = (0, 1, RB - 1, RB, RB + 1)


@functools.lru_cache(maxsize=None)
def rows_case(n, per):
    """n rows of `per` nonzeros in F = 5 columns (vectorised: column j of a
    row is drawn from the j-th stratum)."""
    rng = np.random.default_rng(10 * n + per)
    F = 5
    rp = np.arange(0, n * per + 1, per, dtype=np.int64)
    if per == 1:
        ci = rng.integers(0, F, size=n).astype(np.int32)
    else:
        ci = np.stack([rng.integers(0, 2, size=n), rng.integers(2, F, size=n)], 1)
        ci = ci.astype(np.int32).ravel()
    return rp, ci, rng.normal(size=n * per), n, F


LENS = (0, 1, 63, 64, 65, 129)


@functools.lru_cache(maxsize=None)
def lens_case(F):
    """Rows of 0, 1, 63, 64, 65 and 129 nonzeros (k_row_of strides a row by
    64 lanes), twice, in F columns; F = 129 and 257 are just past a power of
    two, so the sort's endBit is one more than for F - 1 keys."""
    rng = np.random.default_rng(F)
    rp, ci, v = _csr([m for m in LENS + LENS[::-1] if m <= F], F, rng)
    return rp, ci, v, len(rp) - 1, F


@functools.lru_cache(maxsize=None)
def empty_case():
    """F = 9 with columns 0, 4 and 8 (first, middle, last) never used, and
    rows 0 and n - 1 (first, last) and one in the middle empty."""
    rng = np.random.default_rng(5)
    lens = rng.integers(1, 5, size=40)
    lens[[0, 17, 39]] = 0
    rp, ci, v = _csr(lens, 9, rng, cols=[1, 2, 3, 5, 6, 7])
    return rp, ci, v, 40, 9


@functools.lru_cache(maxsize=None)
def no_nonzeros_case():
    return np.zeros(8, np.int64), np.zeros(0, np.int32), np.zeros(0), 7, 4


@functools.lru_cache(maxsize=None)
def one_feature_case():
    """F = 1: every row holds column 0 or nothing; one key per row block."""
    rng = np.random.default_rng(6)
    rp, ci, v = _csr(rng.integers(0, 2, size=300), 1, rng)
    return rp, ci, v, 300, 1


@functools.lru_cache(maxsize=None)
def two_block_wide_case():
    """Two row blocks at F = 129: 2 F = 258 keys, just past 2^8, so the
    second block's high columns need the sort's ninth bit."""
    rng = np.random.default_rng(7)
    n, F = RB + 3, 129
    lens = np.zeros(n, np.int64)
    at = np.concatenate([rng.integers(0, RB, size=50), [RB, RB + 1, RB + 2]])
    lens[at] = 3
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ci = np.tile(np.array([0, 127, 128], np.int32), int(lens.sum()) // 3)
    return rp, ci, rng.normal(size=len(ci)), n, F


@functools.lru_cache(maxsize=None)
def values_case():
    """Values with NaN (two payloads), -0.0, +0.0, the infinities and a
    subnormal: the copy keeps every bit."""
    rng = np.random.default_rng(8)
    rp, ci, v = _csr(rng.integers(0, 6, size=64), 7, rng)
    special = np.array([np.nan, -0.0, 0.0, np.inf, -np.inf, 5e-324, -np.nan])
    v[:len(special)] = special
    v.view(np.int64)[7] = 0x7FF8000000000123          # a NaN with a payload
    v = v[rng.permutation(len(v))]
    return rp, ci, v, 64, 7


def host_cases():
    cases = {f"rows n={n} per={p}": rows_case(n, p) for n in N_ROWS for p in (1, 2)}
    cases.update({f"lens F={F}": lens_case(F) for F in (129, 257)})
    cases["empty rows and columns"] = empty_case()
    cases["no nonzeros"] = no_nonzeros_case()
    cases["one feature"] = one_feature_case()
    cases["two blocks, 258 keys"] = two_block_wide_case()
    cases["values"] = values_case()
    return cases


def test_host_cases():
    cases = host_cases()
    for name, (rp, ci, v, n, F) in cases.items():
        nb, colptr, rowidx, vals = reference(rp, ci, v, n, F)
        assert len(rp) == n + 1 and rp[0] == 0 and rp[-1] == len(ci) == len(v), name
        assert len(colptr) == nb * F + 1 and colptr[0] == 0 and colptr[-1] == len(ci), name
        for r in range(min(n, 200)):       # SparseVector's requires hold
            row = ci[rp[r]:rp[r + 1]]
            assert (np.diff(row) > 0).all() and (row >= 0).all() and (row < F).all(), name
        # a stable sort: inside every (block, column) the rows increase
        inner = np.ones(len(rowidx), bool)
        inner[colptr[:-1][colptr[:-1] < len(rowidx)]] = False
        assert (np.diff(rowidx.astype(np.int64))[inner[1:]] > 0).all(), name
    for n in N_ROWS:
        nb = reference(*rows_case(n, 1))[0]
        assert nb == (2 if n == RB + 1 else 1), n
    _, colptr, rowidx, _ = reference(*rows_case(RB + 1, 2))
    assert colptr[5] == 2 * RB and (rowidx[colptr[5]:] == RB).all()   # block 1 holds one row
    for F in (129, 257):
        rp = lens_case(F)[0]
        assert set(np.diff(rp).tolist()) == set(LENS)
        assert (F - 1) & (F - 2) == 0 and F - 1 > 1        # F - 1 is a power of two
    rp, ci, v, n, F = empty_case()
    _, colptr, _, _ = reference(rp, ci, v, n, F)
    per_col = np.diff(colptr)
    assert (per_col[[0, 4, 8]] == 0).all() and (per_col[[1, 2, 3, 5, 6, 7]] > 0).all()
    assert rp[1] == 0 and rp[-1] == rp[-2] and rp[17] == rp[18]
    assert len(no_nonzeros_case()[1]) == 0
    rp, ci, v, n, F = one_feature_case()
    assert F == 1 and set(np.diff(rp).tolist()) == {0, 1}
    rp, ci, v, n, F = two_block_wide_case()
    nb, colptr, rowidx, _ = reference(rp, ci, v, n, F)
    assert nb == 2 and nb * F == 258 > 256 and np.diff(colptr)[F + 128] == 3
    v = values_case()[2]
    assert np.isnan(v).sum() == 3 and (np.signbit(v) & (v == 0)).any()
    assert (v.view(np.int64) == 0x7FF8000000000123).any()


# ------------------------------------------------------------------- device
class _Raw:
    """A device array the library owns, for torch.as_tensor."""

    def __init__(self, ptr, count, typestr):
        self.__cuda_array_interface__ = {"shape": (count,), "typestr": typestr,
                                         "data": (ptr, False), "version": 2}


def _read(cuda, ptr, count, typestr):
    import torch
    dt = np.dtype(typestr)
    if count == 0:
        return np.zeros(0, dt)
    return torch.as_tensor(_Raw(ptr, count, typestr), device=cuda).clone().cpu().numpy()


def _dev(a, cuda):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def build(cuda, rp, ci, v, n, F):
    """cyc_csc_build_dev, then (rows_per_block, nblocks, colptr, rowidx,
    values) read back."""
    import torch
    from cycloneml_amd import _native as N
    lib = N.load()
    # one spare entry: an empty CSR still hands over valid pointers
    rpd = _dev(rp, cuda)
    cid = _dev(np.concatenate([ci, np.zeros(1, np.int32)]), cuda)
    vd = _dev(np.concatenate([v, np.zeros(1)]), cuda)
    h = ctypes.c_void_p()
    N.check(lib.cyc_csc_build_dev(N.ptr(rpd), N.ptr(cid), N.ptr(vd), n, F, N.stream_handle(),
                                  ctypes.byref(h)))
    try:
        torch.cuda.synchronize()
        rpb, nb = ctypes.c_int64(), ctypes.c_int64()
        N.check(lib.cyc_csc_blocks(h, ctypes.byref(rpb), ctypes.byref(nb)))
        assert lib.cyc_csc_rows(h) == n and lib.cyc_csc_features(h) == F
        p = [ctypes.c_void_p() for _ in range(3)]
        N.check(lib.cyc_csc_arrays(h, *[ctypes.byref(x) for x in p]))
        nnz = len(ci)
        out = (rpb.value, nb.value, _read(cuda, p[0].value, nb.value * F + 1, "<i8"),
               _read(cuda, p[1].value, nnz, "<i4"), _read(cuda, p[2].value, nnz, "<f8"))
    finally:
        lib.cyc_csc_destroy(h)
    return out


def check(cuda, case, what):
    rp, ci, v, n, F = case
    nb, colptr, rowidx, vals = reference(rp, ci, v, n, F)
    rpb, gnb, gc, gr, gv = build(cuda, rp, ci, v, n, F)
    assert (rpb, gnb) == (RB, nb), what
    assert gc.dtype == np.int64 and np.array_equal(gc, colptr), what
    assert gr.dtype == np.int32 and np.array_equal(gr, rowidx), what
    assert np.array_equal(gv.view(np.int64), vals.view(np.int64)), what


@gpu
@pytest.mark.parametrize("per", [1, 2])
@pytest.mark.parametrize("n", N_ROWS)
def test_row_block_edges(cuda, n, per):
    check(cuda, rows_case(n, per), f"n={n} per={per}")


@gpu
@pytest.mark.parametrize("F", [129, 257])
def test_row_lengths(cuda, F):
    check(cuda, lens_case(F), f"F={F}")


@gpu
@pytest.mark.parametrize("name", ["empty rows and columns", "no nonzeros", "one feature",
                                  "two blocks, 258 keys", "values"])
def test_content_edges(cuda, name):
    check(cuda, host_cases()[name], name)


def _refused(cuda, rows, F, match, base=0):
    from cycloneml_amd import _native as N
    lens = [len(r) for r in rows]
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64) + base
    # base entries of padding behind the rows: rowptr[n] stays inside the arrays
    ci = np.concatenate([np.asarray(r) for r in rows] + [np.zeros(base)]).astype(np.int32)
    with pytest.raises(N.IllegalArgumentException, match=match):
        build(cuda, rp, ci, np.ones(len(ci)), len(rows), F)


@gpu
def test_sparse_vector_refusals(cuda):
    good = [[0, 2], [1], [], [0, 1, 2, 3, 4]]
    F = 5
    neg, same, back, oob = [-1, 2], [1, 3, 3], [2, 1], [0, 5]
    many = [0, 1, 2, 3, 4, 5]
    _refused(cuda, good + [neg], F, r"requirement failed: Found negative index: -1\.")
    _refused(cuda, good + [same], F,
             r"requirement failed: Index 3 follows 3 and is not strictly increasing")
    _refused(cuda, good + [back], F,
             r"requirement failed: Index 1 follows 2 and is not strictly increasing")
    _refused(cuda, good + [oob], F,
             r"requirement failed: Index 5 out of bounds for vector of size 5")
    _refused(cuda, good + [many], F,
             r"requirement failed: You provided 6 indices and values, which exceeds the "
             r"specified vector size 5\.")
    # two offending rows: the lowest row's message, whichever kind it is
    _refused(cuda, good + [oob] + good + [neg], F, r"Index 5 out of bounds")
    _refused(cuda, good + [neg] + good + [oob], F, r"Found negative index: -1\.")
    # 300 rows: the two rows sit in different workgroups of the check
    far = [[0]] * 280
    _refused(cuda, [same] + far + [neg], F, r"Index 3 follows 3")


@gpu
def test_rowptr_base_refused(cuda):
    """A CSR slice whose rowptr starts above 0 is refused before any kernel
    indexes with it (include/cyclone.h states the rule)."""
    _refused(cuda, [[0, 2], [1], [0, 1, 2, 3, 4]], 5,
             r"requirement failed: rowptr\[0\] must be 0 for the CSC copy, got 4", base=4)
