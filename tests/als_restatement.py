"""Plain numpy restatement of ml.recommendation.ALS's half-step
(computeFactors: NormalEquation.add per rating in the row's order, then
CholeskySolver.solve) and of the whole loop, cited from memory of ALS.scala.

Per rating (i, r) of row u: da = (double) Y[i]; dspr(c, da) on the packed
upper triangle (ap[j(j+1)/2 + i] += da_i (c da_j), i <= j); daxpy(b, da) on atb.
Explicit c = 1, b = r; implicit c1 = alpha |r|, c = c1, b = 1 + c1 if r > 0 else
0, ata starting from YtY.  Then the diagonal += regParam numExplicits, dppsv
(dpptrf 'U' column by column, then the two dtpsv sweeps) and a round to float32.
"""
import numpy as np


def tri_index(rank):
    """(ia, ib) of the packed upper triangle: position j(j+1)/2 + i holds (i, j)."""
    ib = np.concatenate([np.full(j + 1, j) for j in range(rank)])
    ia = np.concatenate([np.arange(j + 1) for j in range(rank)])
    return ia, ib


def unpack(ap, rank):
    ia, ib = tri_index(rank)
    A = np.zeros((rank, rank))
    A[ia, ib] = ap
    A[ib, ia] = ap
    return A


def yty(Y):
    """Packed sum of da da^T over every row of Y, in row order."""
    rank = Y.shape[1]
    ia, ib = tri_index(rank)
    ap = np.zeros(rank * (rank + 1) // 2)
    for y in Y:
        da = y.astype(np.float64)
        ap += da[ia] * (1.0 * da[ib])
    return ap


def dppsv(ap, b, rank):
    """(x, info): the upper packed Cholesky solve; info = j + 1 at the first
    pivot that is not positive (x is then None)."""
    U = np.zeros((rank, rank))
    ia, ib = tri_index(rank)
    U[ia, ib] = ap
    for j in range(rank):
        # dtpsv('U', 'T', 'N'): U[0:j, 0:j]^T x = a[0:j, j]
        for i in range(j):
            U[i, j] = (U[i, j] - np.dot(U[:i, i], U[:i, j])) / U[i, i]
        ajj = U[j, j] - np.dot(U[:j, j], U[:j, j])
        if not ajj > 0.0:
            return None, j + 1
        U[j, j] = np.sqrt(ajj)
    x = np.array(b, dtype=np.float64)
    for i in range(rank):                     # U^T y = b
        x[i] = (x[i] - np.dot(U[:i, i], x[:i])) / U[i, i]
    for i in range(rank - 1, -1, -1):         # U x = y
        x[i] = (x[i] - np.dot(U[i, i + 1:], x[i + 1:])) / U[i, i]
    return x, 0


def half_step(rowptr, colidx, values, Y, regParam, implicitPrefs=False, alpha=1.0, YtY=None):
    """dict: X (m x rank float32), x64 (the solutions before rounding), A (m x
    rank x rank, the regularised systems), present (m bool), singular (rows
    whose factorization failed; their factor is zero)."""
    m = len(rowptr) - 1
    rank = Y.shape[1]
    ia, ib = tri_index(rank)
    if implicitPrefs and YtY is None:
        YtY = yty(Y)
    diag = np.arange(rank) * (np.arange(rank) + 1) // 2 + np.arange(rank)
    X = np.zeros((m, rank), dtype=np.float32)
    x64 = np.zeros((m, rank))
    A = np.zeros((m, rank, rank))
    present = np.zeros(m, dtype=bool)
    singular = []
    for u in range(m):
        lo, hi = int(rowptr[u]), int(rowptr[u + 1])
        if hi == lo:
            continue
        present[u] = True
        ata = YtY.copy() if implicitPrefs else np.zeros(rank * (rank + 1) // 2)
        atb = np.zeros(rank)
        nexp = 0
        for e in range(lo, hi):
            da = Y[colidx[e]].astype(np.float64)
            r = float(values[e])
            if implicitPrefs:
                c1 = alpha * abs(r)
                c, b = c1, (1.0 + c1 if r > 0.0 else 0.0)
                nexp += r > 0.0
            else:
                c, b = 1.0, r
                nexp += 1
            ata += da[ia] * (c * da[ib])
            if b != 0.0:
                atb += b * da
        ata[diag] += regParam * nexp
        A[u] = unpack(ata, rank)
        x, info = dppsv(ata, atb, rank)
        if info:
            singular.append(u)
            continue
        x64[u] = x
        X[u] = x.astype(np.float32)
    return {"X": X, "x64": x64, "A": A, "present": present, "singular": singular}


def sdot(a, b):
    """fp32, the products added left to right, unfused."""
    s = np.float32(0.0)
    for x, y in zip(a.astype(np.float32), b.astype(np.float32)):
        s = np.float32(s + np.float32(x * y))
    return s


def predict(U, userPresent, V, itemPresent, users, items):
    out = np.full(len(users), np.nan, dtype=np.float32)
    for p, (u, i) in enumerate(zip(users, items)):
        if 0 <= u < len(U) and 0 <= i < len(V) and userPresent[u] and itemPresent[i]:
            out[p] = sdot(U[u], V[i])
    return out


def build_side(dst, src, ratings, m):
    """(rowptr int64, colidx int32, values float32): a stable sort by dst."""
    order = np.argsort(dst, kind="stable")
    rowptr = np.zeros(m + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum(np.bincount(dst, minlength=m))
    return rowptr, src[order].astype(np.int32), ratings[order].astype(np.float32)


def fit(users, items, ratings, numUsers, numItems, U0, maxIter, regParam, implicitPrefs=False,
        alpha=1.0):
    """[(itemFactors, userFactors)] after every iteration: the item half-step
    from the user factors first, then the user half-step."""
    userSide = build_side(users, items, ratings, numUsers)
    itemSide = build_side(items, users, ratings, numItems)
    U = U0.astype(np.float32)
    out = []
    for _ in range(maxIter):
        V = half_step(*itemSide, U, regParam, implicitPrefs, alpha)["X"]
        U = half_step(*userSide, V, regParam, implicitPrefs, alpha)["X"]
        out.append((V, U))
    return out


def objective(users, items, ratings, U, V, regParam):
    """sum (r - x.y)^2 + lambda sum_u n_u |x_u|^2 + lambda sum_i n_i |y_i|^2, fp64."""
    U = U.astype(np.float64)
    V = V.astype(np.float64)
    err = ratings.astype(np.float64) - (U[users] * V[items]).sum(axis=1)
    nu = np.bincount(users, minlength=len(U))
    ni = np.bincount(items, minlength=len(V))
    return float((err * err).sum() + regParam * (nu * (U * U).sum(axis=1)).sum()
                 + regParam * (ni * (V * V).sum(axis=1)).sum())


def rmse(users, items, ratings, U, V):
    err = ratings.astype(np.float64) - (U.astype(np.float64)[users]
                                        * V.astype(np.float64)[items]).sum(axis=1)
    return float(np.sqrt((err * err).mean()))
