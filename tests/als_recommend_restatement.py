"""Plain numpy restatement of ALSModel.recommendForAll's arithmetic and order
(ml/recommendation/ALS.scala, cited from memory), as cycloneml_amd fixes it.

Score: per (source row, destination) pair an fp32 dot product, one float32
multiply and one float32 add per factor, left to right from +0.0 (sgemv("T")
through the Java BLAS; the bits of als_restatement.sdot).  Absent destinations
are no candidates.  Order: score descending under java.lang.Float.compare
(every NaN equal to the canonical one and above +infinity; -0.0 below +0.0),
equal scores to the lower destination id.  Output rows are padded with -1 /
NaN; a source id that is negative, past the rows or absent gives a row of
padding.  A NaN score is returned as the canonical NaN (0x7fc00000).
"""
import numpy as np

NAN = np.float32(np.nan)


def scores(S, D):
    """(m x n float32): the chain, vectorised over the pairs."""
    S = np.asarray(S, dtype=np.float32)
    D = np.asarray(D, dtype=np.float32)
    acc = np.zeros((S.shape[0], D.shape[0]), dtype=np.float32)
    with np.errstate(all="ignore"):
        for f in range(S.shape[1]):
            prod = S[:, f:f + 1] * D[None, :, f]          # float32 x float32 -> float32
            acc = acc + prod                               # float32 + float32 -> float32
    assert acc.dtype == np.float32
    return acc


def float_compare_rank(x):
    """uint32 that grows with java.lang.Float.compare's order: floatToIntBits
    (NaN -> 0x7fc00000), then negative floats reversed below the positive."""
    x = np.array(x, dtype=np.float32)
    x[np.isnan(x)] = NAN
    b = x.view(np.uint32)
    return np.where(b >> 31 != 0, ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def top(row_scores, present, num):
    """(ids int32 [num], scores float32 [num]) of one source row."""
    ids = np.nonzero(np.asarray(present) != 0)[0]
    sc = np.array(row_scores, dtype=np.float32)[ids]
    sc[np.isnan(sc)] = NAN
    order = np.lexsort((ids, -float_compare_rank(sc).astype(np.int64)))[:num]
    out_i = np.full(num, -1, dtype=np.int32)
    out_s = np.full(num, NAN, dtype=np.float32)
    out_i[:len(order)] = ids[order]
    out_s[:len(order)] = sc[order]
    return out_i, out_s


def recommend(S, srcPresent, D, dstPresent, num, srcIds=None):
    """(ids int32 [m x num], scores float32 [m x num])."""
    S = np.asarray(S, dtype=np.float32)
    D = np.asarray(D, dtype=np.float32)
    sp = np.ones(len(S), dtype=np.uint8) if srcPresent is None else np.asarray(srcPresent)
    dp = np.ones(len(D), dtype=np.uint8) if dstPresent is None else np.asarray(dstPresent)
    src = np.arange(len(S)) if srcIds is None else np.asarray(srcIds, dtype=np.int64)
    ok = (src >= 0) & (src < len(S))
    ok[ok] = sp[src[ok]] != 0
    ids = np.full((len(src), num), -1, dtype=np.int32)
    out = np.full((len(src), num), NAN, dtype=np.float32)
    if ok.any():
        sc = scores(S[src[ok]], D)
        for r, row in zip(np.nonzero(ok)[0], sc):
            ids[r], out[r] = top(row, dp, num)
    return ids, out
