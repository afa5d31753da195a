"""Conformance tests of the Summarizer pre-pass (csrc/summarizer.hip) at its
workgroup, unroll, prefetch, merge-branch, special-value and launch edges, at
the smallest shapes that reach them.

Bar: the device runs the reference's per-element operation order over the
same partitions, merged in the same order, so the whole buffer (8 F fields +
5 scalars), the 9 F metrics, the label histogram / invalid count / largest
label and the scaled values must equal the restatement (oracle.summarize,
summarizer_metrics, summarizer_merge, orc_label_summarize; X * s in numpy)
bit for bit, a NaN matching a NaN at the same position.

Every case is built on the host by a cached function; test_host_cases walks
them with the reference alone and asserts that each reaches the edge it is
named for (partition lengths, the merge branch taken, tot == 0, the special
value where it has to show).
"""
import functools

import numpy as np
import pytest

import oracle

gpu = pytest.mark.gpu
NF, NS = 8, 5                      # fields, scalars
MEAN, M2N, M2, L1, WS, NNZ, MAX, MIN = range(8)
RB = 1 << 18                       # rows per CSC row block
DBL_MAX = np.finfo(np.float64).max


def same_bits(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and \
        np.array_equal(a[~na].view(np.int64), b[~nb].view(np.int64))


def first_diff(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    bad = np.flatnonzero(~((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))))
    return [(int(i), float(a[i]), float(b[i])) for i in bad[:5]]


def field(buf, F, f):
    return buf[f * F:(f + 1) * F]


def scalars(buf, F):
    return buf[NF * F:]


def metrics_ref(F, buf):
    m = oracle.summarizer_metrics(F, buf)
    return np.concatenate([m[name] for name in oracle.SUMM_METRICS])


def part_buffers(F, X, w, R):
    """Each partition's own buffer (the reference over its rows alone)."""
    n = X.shape[0]
    return [oracle.summarize(F, X=X[p:p + R], w=None if w is None else w[p:p + R])
            for p in range(0, n, R)]


def merge_trace(F, parts):
    """The branch SummarizerBuffer.merge takes per partition ('merge', 'copy'
    or 'skip'), and per merge the columns with tot == 0."""
    tA, wsA = 0.0, np.zeros(F)
    trace, tot0 = [], []
    for b in parts:
        tB = scalars(b, F)[1]
        if tA != 0.0 and tB != 0.0:
            trace.append("merge")
            tot0.append(np.flatnonzero(wsA + field(b, F, WS) == 0.0).tolist())
            wsA = wsA + field(b, F, WS)
            tA += tB
        elif tA == 0.0 and tB != 0.0:
            trace.append("copy")
            tA, wsA = tB, field(b, F, WS).copy()
        else:
            trace.append("skip")
    return trace, tot0


# ------------------------------------------------------------- dense cases
F_EDGES = (1, 255, 256, 257, 513)
# (n, R): partition lengths 1, 7, 8, 9, 63, 64, 65, 128, 129 (each as a full
# partition and most with a shorter tail), n = R, n = R + 1, R > n, R = 1, n = 0
SHAPES = ((3, 1), (17, 7), (20, 8), (22, 9), (131, 63), (128, 64), (131, 65), (137, 128),
          (136, 129), (40, 40), (41, 40), (5, 100), (0, 4))
LENGTHS = {1, 7, 8, 9, 63, 64, 65, 128, 129}


def lengths(n, R):
    return [min(R, n - p) for p in range(0, n, R)]


@functools.lru_cache(maxsize=None)
def shape_case(F, n, R):
    rng = np.random.default_rng(F + 1000 * n + R)
    X = rng.normal(size=(n, F)) * rng.uniform(0.1, 5.0, size=F)
    X[rng.random((n, F)) < 0.3] = 0.0
    w = rng.uniform(0.1, 2.0, n)
    w[rng.random(n) < 0.15] = 0.0
    return X, w


MERGE_R, MERGE_P, MERGE_F = 4, 6, 5
ZEROED = {"first": (0,), "middle": (3,), "last": (5,), "two in a row": (2, 3),
          "first two": (0, 1), "all": tuple(range(6)), "none": ()}


@functools.lru_cache(maxsize=None)
def merge_case(which):
    """6 partitions of 4 rows, F = 5; `which` partitions weigh 0 as a whole.
    Column 3 is zero in partitions 1 and 2 (tot == 0 when they merge first:
    "first"), column 4's only nonzeros sit in rows of weight 0."""
    rng = np.random.default_rng(len(which))
    n = MERGE_R * MERGE_P
    X = rng.normal(size=(n, MERGE_F))
    X[:12, 3] = 0.0
    w = rng.uniform(0.5, 2.0, n)
    X[:, 4] = 0.0
    X[[1, 6, 22], 4] = [1.5, -2.5, 3.5]
    w[[1, 6, 22]] = 0.0
    for p in ZEROED[which]:
        w[p * MERGE_R:(p + 1) * MERGE_R] = 0.0
    return X, w


@functools.lru_cache(maxsize=None)
def values_case():
    """F = 8, 12 rows, R = 5 (partitions of 5, 5, 2).  Column 0: +-0.0 among
    values; 1: a NaN; 2: +Inf; 3: -Inf; 4: a subnormal; 5: +-1e308 (m2
    overflows); 6: negatives and zeros (nnz < count, max metric 0); 7:
    positives only (nnz == count, min stays positive)."""
    rng = np.random.default_rng(21)
    X = rng.normal(size=(12, 8))
    X[[0, 3, 6], 0] = [-0.0, 0.0, -0.0]
    X[7, 1] = np.nan
    X[2, 2] = np.inf
    X[8, 3] = -np.inf
    X[:, 4] = 0.0
    X[[1, 6], 4] = [5e-324, -5e-324]
    X[[0, 4, 9], 5] = [1e308, -1e308, 1e308]
    X[:, 6] = -np.abs(X[:, 6]) - 0.5
    X[[2, 5, 11], 6] = [0.0, -0.0, 0.0]
    X[:, 7] = np.abs(X[:, 7]) + 0.5
    return X, None


WEIGHT_CASES = ("tiny", "negative zero", "negative then NaN", "NaN then negative")


@functools.lru_cache(maxsize=None)
def weights_case(which):
    """10 rows, F = 3, R = 4 (partitions 4, 4, 2)."""
    rng = np.random.default_rng(22)
    X = rng.normal(size=(10, 3))
    w = rng.uniform(0.5, 2.0, 10)
    if which == "tiny":
        w[[1, 5]] = 1e-300            # w * w underflows to 0
    elif which == "negative zero":
        w[[0, 6]] = -0.0              # weight == 0: the row is skipped
    elif which == "negative then NaN":
        w[2], w[9] = -2.0, np.nan     # partitions 0 and 2
        w[3] = -3.0                   # later in partition 0: not the first
    else:
        w[2], w[9] = np.nan, -2.0
    return X, w


# --------------------------------------------------------------- CSR cases
CSR_CASES = ("edges", "first block weighs 0", "second block weighs 0", "no nonzeros",
             "one feature")


@functools.lru_cache(maxsize=None)
def csr_case(which):
    """2^18 + 1 rows of at most two nonzeros: two row blocks, the second of
    one row.  Values carry the dense value edges and explicit zeros, weights
    the weight edges."""
    rng = np.random.default_rng(30 + len(which))
    n, F = RB + 1, (1 if which == "one feature" else 6)
    per = rng.integers(0, 2 if F == 1 else 3, size=n)
    per[-1] = 1 if F == 1 else 2
    if which == "no nonzeros":
        per[:] = 0
    rp = np.concatenate([[0], np.cumsum(per)]).astype(np.int64)
    nnz = int(rp[-1])
    first = np.ones(nnz, bool)
    first[rp[1:][per == 2] - 1] = False          # the second entry of a two-entry row
    ci = np.where(first, rng.integers(0, max(F // 2, 1), size=nnz),
                  rng.integers(F // 2, F, size=nnz) if F > 1 else 0).astype(np.int32)
    v = rng.normal(size=nnz)
    w = rng.uniform(0.25, 2.0, n)
    w[rng.random(n) < 0.05] = 0.0
    if nnz:
        v[rng.random(nnz) < 0.05] = 0.0          # explicit zeros
        sp = rng.choice(nnz, size=9, replace=False)
        v[sp] = [-0.0, np.nan, np.inf, -np.inf, 5e-324, 1e308, -1e308, 1e308, 0.0]
    if which == "edges":
        w[[5, 70000]] = 1e-300
        w[[9, RB]] = [-0.0, 1.5]
        w[[100, RB - 1]] = [np.nan, -1.0]
    if which == "first block weighs 0":
        w[:RB] = 0.0
    if which == "second block weighs 0":
        w[RB] = 0.0
    return (rp, ci, v), w, n, F


# ------------------------------------------------------------- merge cases
@functools.lru_cache(maxsize=None)
def merge_inputs():
    """Five finished buffers of F = 7 over different rows, and an empty one."""
    rng = np.random.default_rng(40)
    F = 7
    bufs = []
    for i in range(5):
        X = rng.normal(size=(9 + i, F))
        X[rng.random(X.shape) < 0.4] = 0.0
        bufs.append(oracle.summarize(F, X=X, w=rng.uniform(0.1, 2.0, 9 + i), rows_per_partition=4))
    return F, bufs, oracle.summarizer_new(F)


def merged_ref(F, bufs):
    out = oracle.summarizer_new(F)
    for b in bufs:
        oracle.summarizer_merge(F, out, b)
    return out


def merge_lists():
    """(count, position of the empty buffer or None)."""
    return [(c, e) for c in (1, 3, 5) for e in [None] + list(range(c))]


@functools.lru_cache(maxsize=None)
def metrics_buffers():
    """Hand-written buffers, F = 3: columns (max < 0, min > 0, mixed).
      'one row': count 1, TW = TW2 = 1: TW2 / TW == TW, the variance
                 denominator is 0;
      'full': nnz == count in every column: max and min stay;
      'sparse': nnz < count: column 0's max (< 0) and column 1's min (> 0)
                become 0;
      'negative zero': m2n = -0.0, mean 0 and a column weight above TW, so
                the variance expression is -0.0 and Math.max(-0.0, 0.0) has
                to give +0.0 (the signbit arm of jmax)."""
    F = 3

    def buf(cnt, tw, tw2, nnz, mean, ws, m2n=(0.5, 0.25, 2.0)):
        b = oracle.summarizer_new(F)
        b[MEAN * F:MEAN * F + F] = mean
        b[M2N * F:M2N * F + F] = m2n
        b[M2 * F:M2 * F + F] = [9.0, 16.0, 2.0]
        b[L1 * F:L1 * F + F] = [3.0, 4.0, 1.5]
        b[WS * F:WS * F + F] = ws
        b[NNZ * F:NNZ * F + F] = nnz
        b[MAX * F:MAX * F + F] = [-1.0, 5.0, 2.0]
        b[MIN * F:MIN * F + F] = [-3.0, 0.5, -2.0]
        b[NF * F:NF * F + 3] = [cnt, tw, tw2]
        return b
    return F, {"one row": buf(1.0, 1.0, 1.0, [1, 1, 1], [-1.0, 5.0, 2.0], [1.0, 1.0, 1.0]),
               "full": buf(4.0, 6.0, 10.0, [4, 4, 4], [-2.0, 2.0, 0.1], [6.0, 6.0, 6.0]),
               "sparse": buf(4.0, 6.0, 10.0, [2, 3, 1], [-2.0, 2.0, 0.1], [2.5, 4.0, 1.0]),
               "negative zero": buf(4.0, 6.0, 10.0, [4, 4, 4], [0.0, 2.0, 0.1], [7.0, 6.0, 6.0],
                                    m2n=(-0.0, 0.25, 2.0))}


# ------------------------------------------------------------- label cases
LABEL_LENGTHS = (1, 63, 64, 65, 129)


def labels_ref(y, w, R, maxc):
    """(hist[maxc], invalid, largest valid label or -1)."""
    y = np.ascontiguousarray(y, np.float64)
    hist = np.empty(maxc)
    inv, mx = np.zeros(1, np.int64), np.zeros(1, np.int64)
    wp = None if w is None else np.ascontiguousarray(w, np.float64)
    oracle.lib().orc_label_summarize(len(y), oracle._p(y), oracle._p(wp), int(R), int(maxc),
                                     oracle._p(hist), oracle._p(inv, oracle._I64),
                                     oracle._p(mx, oracle._I64))
    return hist, int(inv[0]), int(mx[0])


@functools.lru_cache(maxsize=None)
def label_case(R, maxc, weighted):
    """2 R + R // 2 + 1 rows (partitions R, R and a tail): classes below
    maxc, the labels -0.0 (class 0), 2.5, -1, NaN, +-Inf, 1e10 (invalid),
    maxc - 1, and maxc + 2 (valid, past the histogram); with weights, rows of
    weight 0, -1 and NaN (skipped, whatever their label)."""
    rng = np.random.default_rng(1000 * R + maxc + weighted)
    n = 2 * R + R // 2 + 1
    y = rng.integers(0, min(maxc, 40), size=n).astype(np.float64)
    special = [-0.0, 2.5, -1.0, np.nan, np.inf, -np.inf, 1e10, maxc - 1.0, maxc + 2.0]
    at = rng.permutation(n)[:len(special)]
    y[at[:min(n, len(special))]] = special[:min(n, len(special))]
    w = None
    if weighted:
        w = rng.uniform(0.25, 2.0, n)
        skip = rng.permutation(n)[:min(n, 6)]
        w[skip] = np.resize([0.0, -1.0, np.nan], len(skip))
    return y, w


# ------------------------------------------------------------- scale cases
GRID_CAP = 8192 * 256
SCALE_DENSE = ((85, 3), (64, 4), (257, 1), (GRID_CAP // 3 + 1, 3))
SCALE_NNZ = (255, 256, 257, GRID_CAP + 1)


@functools.lru_cache(maxsize=None)
def scale_dense_case(n, F):
    rng = np.random.default_rng(n + F)
    X = rng.normal(size=(n, F))
    X[rng.random((n, F)) < 0.1] = 0.0
    s = np.array([0.0, np.inf, np.nan, 1.5])[:F] if F > 1 else np.array([np.inf])
    return X, s


@functools.lru_cache(maxsize=None)
def scale_csr_case(nnz):
    rng = np.random.default_rng(nnz)
    v = rng.normal(size=nnz)
    v[rng.random(nnz) < 0.1] = 0.0
    return rng.integers(0, 5, size=nnz).astype(np.int32), v, np.array([0.0, np.inf, np.nan, 2.5, -1.0])


# --------------------------------------------------------------- host test
def test_host_cases():
    seen = set()
    for n, R in SHAPES:
        seen |= set(lengths(n, R))
        for F in (1, 257):
            X, w = shape_case(F, n, R)
            assert X.shape == (n, F)
    assert LENGTHS <= seen
    assert (40, 40) in SHAPES and (41, 40) in SHAPES and lengths(41, 40) == [40, 1]
    assert any(R > n > 0 for n, R in SHAPES) and any(R == 1 for n, R in SHAPES)
    assert any(n == 0 for n, R in SHAPES)
    empty = oracle.summarize(3, X=np.zeros((0, 3)), rows_per_partition=4)
    assert same_bits(empty, oracle.summarizer_new(3))
    # merge branches
    want = {"first": ["skip", "copy", "merge", "merge", "merge", "merge"],
            "middle": ["copy", "merge", "merge", "skip", "merge", "merge"],
            "last": ["copy", "merge", "merge", "merge", "merge", "skip"],
            "two in a row": ["copy", "merge", "skip", "skip", "merge", "merge"],
            "first two": ["skip", "skip", "copy", "merge", "merge", "merge"],
            "all": ["skip"] * 6,
            "none": ["copy"] + ["merge"] * 5}
    for which in ZEROED:
        X, w = merge_case(which)
        trace, tot0 = merge_trace(MERGE_F, part_buffers(MERGE_F, X, w, MERGE_R))
        assert trace == want[which], (which, trace)
        if which == "none":
            # partitions 0 and 1 merge with column 3 empty in both: tot == 0
            assert 3 in tot0[0] and 3 in tot0[1] and 3 not in tot0[2]
        if which in ("none", "first"):
            assert all(4 in t for t in tot0)      # nonzeros only in rows of weight 0
            ref = oracle.summarize(MERGE_F, X=X, w=w, rows_per_partition=MERGE_R)
            assert field(ref, MERGE_F, NNZ)[4] == 0 and field(ref, MERGE_F, MAX)[4] == -DBL_MAX
    # values
    X, _ = values_case()
    ref = oracle.summarize(8, X=X, rows_per_partition=5)
    met = oracle.summarizer_metrics(8, ref)
    assert field(ref, 8, NNZ)[0] == 9                      # three signed zeros skipped
    assert np.isnan(field(ref, 8, MEAN)[1]) and np.isnan(met["variance"][1])
    assert field(ref, 8, MAX)[2] == np.inf and field(ref, 8, MIN)[3] == -np.inf
    assert field(ref, 8, NNZ)[4] == 2 and field(ref, 8, MIN)[4] == -5e-324
    assert field(ref, 8, M2)[5] == np.inf
    assert field(ref, 8, MAX)[6] < 0 and field(ref, 8, NNZ)[6] == 9 and met["max"][6] == 0.0
    assert field(ref, 8, NNZ)[7] == 12 and met["min"][7] == field(ref, 8, MIN)[7] > 0
    one = oracle.summarizer_metrics(8, oracle.summarize(8, X=X[:1]))
    assert not one["variance"].any()                       # denominator 0
    # weights
    X, w = weights_case("tiny")
    ref = oracle.summarize(3, X=X, w=w, rows_per_partition=4)
    assert w[1] * w[1] == 0.0 and scalars(ref, 3)[0] == 10
    X, w = weights_case("negative zero")
    assert scalars(oracle.summarize(3, X=X, w=w, rows_per_partition=4), 3)[0] == 8
    X, w = weights_case("negative then NaN")
    s = scalars(oracle.summarize(3, X=X, w=w, rows_per_partition=4), 3)
    assert s[3] == 1.0 and s[4] == -2.0
    X, w = weights_case("NaN then negative")
    s = scalars(oracle.summarize(3, X=X, w=w, rows_per_partition=4), 3)
    assert s[3] == 1.0 and np.isnan(s[4])
    # CSR
    for which in CSR_CASES:
        (rp, ci, v), w, n, F = csr_case(which)
        assert n == RB + 1 and len(rp) == n + 1 and np.diff(rp).max() <= 2
        assert ((np.diff(ci) > 0) | (np.diff(rp)[np.searchsorted(rp, np.arange(1, len(ci)),
                                                                  side="right") - 1] < 2)
                | np.isin(np.arange(1, len(ci)), rp)).all()
        assert (len(ci) == 0) == (which == "no nonzeros") and (ci < F).all()
        if which == "first block weighs 0":
            assert not w[:RB].any() and w[RB] > 0
        if which == "second block weighs 0":
            assert w[RB] == 0 and w[:RB].any()
        if which == "edges":
            assert (v == 0).sum() > 100 and np.isnan(v).any() and np.isinf(v).any()
            ref = oracle.summarize(F, csr=(rp, ci, v), w=w, rows_per_partition=RB)
            assert scalars(ref, F)[3] == 1.0 and np.isnan(scalars(ref, F)[4])
    # merge lists, metrics buffers
    F, bufs, empty = merge_inputs()
    assert scalars(empty, F)[1] == 0 and all(scalars(b, F)[1] > 0 for b in bufs)
    assert {c for c, _ in merge_lists()} == {1, 3, 5}
    F, hand = metrics_buffers()
    s = scalars(hand["one row"], F)
    assert s[2] / s[1] == s[1]
    m = oracle.summarizer_metrics(F, hand["one row"])
    assert not m["variance"].any()
    m = oracle.summarizer_metrics(F, hand["full"])
    assert m["max"][0] == -1.0 and m["min"][1] == 0.5
    m = oracle.summarizer_metrics(F, hand["sparse"])
    assert m["max"][0] == 0.0 and m["min"][1] == 0.0 and m["max"][2] == 2.0 and m["min"][2] == -2.0
    b = hand["negative zero"]
    raw = (b[M2N * F] + b[MEAN * F] * b[MEAN * F] * b[WS * F] * (6.0 - b[WS * F]) / 6.0) / \
        (6.0 - 10.0 / 6.0)
    v0 = oracle.summarizer_metrics(F, b)["variance"][0]
    assert raw == 0.0 and np.signbit(raw) and v0 == 0.0 and not np.signbit(v0)
    # labels
    for R in LABEL_LENGTHS:
        for maxc in (1, 8, 8192):
            for weighted in (False, True):
                y, w = label_case(R, maxc, weighted)
                assert set(lengths(len(y), R)) == {R, R // 2 + 1}
                hist, inv, mx = labels_ref(y, w, R, maxc)
                if R >= 63 and not weighted:
                    assert inv == 6 and mx == maxc + 2
                    assert hist[maxc - 1] >= 1.0
    hist, inv, mx = labels_ref(np.array([-0.0, -0.0]), None, 4, 3)
    assert hist[0] == 2.0 and inv == 0 and mx == 0
    # scaling
    assert [n * F for n, F in SCALE_DENSE[:3]] == [255, 256, 257]
    n, F = SCALE_DENSE[3]
    assert GRID_CAP < n * F <= 2 * GRID_CAP and F == 3
    assert GRID_CAP < SCALE_NNZ[3] <= 2 * GRID_CAP


# ------------------------------------------------------------------- device
def _dev(a, cuda):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def dev_dense(cuda, X, w, R, check=True):
    import torch
    from cycloneml_amd import _native as N
    n, F = X.shape
    buf = torch.full((NF * F + NS,), 7.0, dtype=torch.float64, device=cuda)
    Xd, wd = _dev(X, cuda), _dev(w, cuda)
    N.check(N.load().cyc_summarizer_dense_dev(N.ptr(Xd), N.ptr(wd), n, F, int(R), N.ptr(buf),
                                              N.stream_handle()))
    return buf


def dev_metrics(cuda, buf, F):
    import torch
    from cycloneml_amd import _native as N
    out = torch.empty(9 * F, dtype=torch.float64, device=cuda)
    N.check(N.load().cyc_summarizer_metrics_dev(F, N.ptr(buf), N.ptr(out), N.stream_handle()))
    return out.cpu().numpy()


def check_dense(cuda, X, w, R, what):
    F = X.shape[1]
    ref = oracle.summarize(F, X=X, w=w, rows_per_partition=R)
    buf = dev_dense(cuda, X, w, R)
    got = buf.cpu().numpy()
    assert same_bits(got, ref), (what, first_diff(got, ref))
    gm = dev_metrics(cuda, buf, F)
    with np.errstate(all="ignore"):
        rm = metrics_ref(F, ref)
    assert same_bits(gm, rm), (what, "metrics", first_diff(gm, rm))


@gpu
@pytest.mark.parametrize("F", F_EDGES)
def test_dense_partition_lengths(cuda, F):
    for n, R in SHAPES:
        X, w = shape_case(F, n, R)
        check_dense(cuda, X, w, R, f"F={F} n={n} R={R}")
        check_dense(cuda, X, None, R, f"F={F} n={n} R={R} unweighted")


@gpu
def test_dense_partition_count_limit(cuda):
    from cycloneml_amd import _native as N
    rng = np.random.default_rng(2)
    X = rng.normal(size=(65536, 1))
    X[rng.random(65536) < 0.3] = 0.0
    w = rng.uniform(0.0, 2.0, 65536)
    check_dense(cuda, X[:65535], w[:65535], 1, "P=65535")
    with pytest.raises(N.IllegalArgumentException,
                       match=r"at most 65535 partitions per call \(raise rows_per_partition\)"):
        dev_dense(cuda, X, w, 1)


@gpu
@pytest.mark.parametrize("which", list(ZEROED))
def test_dense_merge_branches(cuda, which):
    X, w = merge_case(which)
    check_dense(cuda, X, w, MERGE_R, which)


@gpu
def test_dense_values(cuda):
    X, _ = values_case()
    check_dense(cuda, X, None, 5, "values")
    check_dense(cuda, X, np.linspace(0.5, 2.0, 12), 5, "values weighted")
    check_dense(cuda, X[:1], None, 5, "single row")
    check_dense(cuda, X[7:8], np.array([2.0]), 1, "single NaN row")


@gpu
@pytest.mark.parametrize("which", WEIGHT_CASES)
def test_dense_weights(cuda, which):
    X, w = weights_case(which)
    check_dense(cuda, X, w, 4, which)


@gpu
@pytest.mark.parametrize("which", CSR_CASES)
def test_csr_two_row_blocks(cuda, which):
    from cycloneml_amd.optim import DeviceInstanceBlock
    from cycloneml_amd.stat import SummarizerBuffer
    (rp, ci, v), w, n, F = csr_case(which)
    ref = oracle.summarize(F, csr=(rp, ci, v), w=w, rows_per_partition=RB)
    # one spare entry: an empty CSR still hands over valid pointers
    blk = DeviceInstanceBlock.from_numpy(np.zeros(n), w, csr=(rp, np.append(ci, 0), np.append(v, 0.0)),
                                         numFeatures=F, device=cuda)
    sb = SummarizerBuffer.of_block(blk)
    got = sb.buf.cpu().numpy()
    assert same_bits(got, ref), (which, first_diff(got, ref))
    with np.errstate(all="ignore"):
        rm = metrics_ref(F, ref)
    gm = dev_metrics(cuda, sb.buf, F)
    assert same_bits(gm, rm), (which, "metrics", first_diff(gm, rm))


@gpu
@pytest.mark.parametrize("alias", [None, "first", "last"])
def test_merge_counts_and_aliasing(cuda, alias):
    import torch
    from cycloneml_amd import _native as N
    F, bufs, empty = merge_inputs()
    for count, e in merge_lists():
        ins = [b.copy() for b in bufs[:count]]
        if e is not None:
            ins[e] = empty.copy()
        ref = merged_ref(F, ins)
        stack = _dev(np.stack(ins), cuda)
        out = {None: torch.full((NF * F + NS,), 7.0, dtype=torch.float64, device=cuda),
               "first": stack[0], "last": stack[count - 1]}[alias]
        N.check(N.load().cyc_summarizer_merge_dev(F, N.ptr(stack), count, N.ptr(out),
                                                  N.stream_handle()))
        got = out.cpu().numpy()
        assert same_bits(got, ref), (count, e, alias, first_diff(got, ref))
        after = stack.cpu().numpy()
        keep = [i for i in range(count) if alias is None or i != (0 if alias == "first" else count - 1)]
        assert all(same_bits(after[i], ins[i]) for i in keep), (count, e, alias)


@gpu
def test_metrics_of_hand_written_buffers(cuda):
    F, hand = metrics_buffers()
    for name, b in hand.items():
        got = dev_metrics(cuda, _dev(b, cuda), F)
        ref = metrics_ref(F, b)
        assert same_bits(got, ref), (name, first_diff(got, ref))


def dev_labels(cuda, y, w, R, maxc):
    import torch
    from cycloneml_amd import _native as N
    hist = torch.full((max(maxc, 1),), 7.0, dtype=torch.float64, device=cuda)
    inv = torch.full((1,), 9, dtype=torch.int64, device=cuda)
    mx = torch.full((1,), 9, dtype=torch.int32, device=cuda)
    yd, wd = _dev(y, cuda), _dev(w, cuda)
    N.check(N.load().cyc_label_summarizer_dev(N.ptr(yd), N.ptr(wd), len(y), int(R), int(maxc),
                                              N.ptr(hist), N.ptr(inv), N.ptr(mx),
                                              N.stream_handle()))
    return hist.cpu().numpy(), int(inv.item()), int(mx.item())


@gpu
@pytest.mark.parametrize("maxc", [1, 8, 8192])
@pytest.mark.parametrize("weighted", [False, True])
def test_label_partition_lengths(cuda, weighted, maxc):
    for R in LABEL_LENGTHS:
        y, w = label_case(R, maxc, weighted)
        hist, inv, mx = labels_ref(y, w, R, maxc)
        gh, gi, gm = dev_labels(cuda, y, w, R, maxc)
        assert (gi, gm) == (inv, mx), (R, gi, gm, inv, mx)
        assert same_bits(gh, hist), (R, first_diff(gh, hist))


@gpu
def test_label_limits_empty_and_second_pass(cuda):
    from cycloneml_amd import _native as N
    from cycloneml_amd.stat import MultiClassSummarizer
    y = np.array([0.0, 1.0])
    for maxc in (0, 8193):
        with pytest.raises(N.IllegalArgumentException, match=r"max_classes must be in \[1, 8192\]"):
            dev_labels(cuda, y, None, 4, maxc)
    gh, gi, gm = dev_labels(cuda, np.zeros(0), None, 4, 5)
    assert not gh.any() and (gi, gm) == (0, -1)
    # a valid label >= max_classes: of_labels runs again with max label + 1
    y, w = label_case(65, 8, True)
    m = MultiClassSummarizer.of_labels(_dev(y, cuda), _dev(w, cuda), rows_per_partition=65,
                                       max_classes=8)
    hist, inv, mx = labels_ref(y, w, 65, 11)
    assert mx == 10 and m.numClasses == 11 and m.countInvalid == inv
    assert same_bits(m.histogram, hist)


@gpu
@pytest.mark.parametrize("n,F", SCALE_DENSE)
def test_scale_dense(cuda, n, F):
    from cycloneml_amd import _native as N
    X, s = scale_dense_case(n, F)
    Xd = _dev(X, cuda)
    N.check(N.load().cyc_scale_columns_dense_dev(N.ptr(Xd), n, F, N.ptr(_dev(s, cuda)),
                                                 N.stream_handle()))
    with np.errstate(all="ignore"):
        ref = X * s
    assert same_bits(Xd.cpu().numpy(), ref)


@gpu
@pytest.mark.parametrize("nnz", SCALE_NNZ)
def test_scale_csr(cuda, nnz):
    from cycloneml_amd import _native as N
    ci, v, s = scale_csr_case(nnz)
    vd, cd = _dev(v, cuda), _dev(ci, cuda)
    N.check(N.load().cyc_scale_columns_csr_dev(N.ptr(cd), N.ptr(vd), nnz, N.ptr(_dev(s, cuda)),
                                               N.stream_handle()))
    with np.errstate(all="ignore"):
        ref = v * s[ci]
    assert same_bits(vd.cpu().numpy(), ref)
    assert np.array_equal(cd.cpu().numpy(), ci)
