"""ALS (ml/recommendation/ALS.scala) over device COO ratings.  The kernels are
csrc/als.hip (cyc_als_* in include/cyclone.h).  The Scala is cited from
memory (computeFactors, NormalEquation, CholeskySolver); the arithmetic below
is the contract the tests hold the device to.

Half-step.  One side is the ratings grouped by destination id in CSR form:
rowptr (int64, m + 1), colidx (int32 source ids), values (float32); duplicates
of a (user, item) pair stay separate entries.  With the source factors Y (nsrc
x rank float32), row u walks its ratings (i, r) in order, all fp64:
    da = (double) Y[i];  ata += c da da^T (packed upper, dspr);  atb += b da
explicit: c = 1, b = r, numExplicits = n_u (the row's rating count).
implicitPrefs: c1 = alpha |r|, c = c1, b = 1 + c1 if r > 0 else 0 (atb takes b,
not c b), numExplicits = #{r > 0}, and ata starts from YtY = sum_i da_i da_i^T
over all source rows.  Then ata's diagonal += regParam numExplicits, a Cholesky
solve (dppsv) in fp64, X[u] = (float) solution.  A row without ratings gets a
zero factor and is marked absent.  A pivot that is not positive raises
SingularMatrixException naming the lowest such row.

The loop (ALS.train): for maxIter iterations, the ITEM half-step from the user
factors first, then the user half-step from the new item factors.

The initial user factors have the reference's shape (rank standard normals per
id, scaled to unit 2-norm in float32; ids without ratings get zero rows), but
they are drawn by numpy.random.default_rng(seed) over the id range.  Spark's
per-block XORShiftRandom draws and its in / out block partitioning are NOT
restated, so a fit does not reproduce a Spark run's factors.

Top-N (ALSModel.recommendForAll, csrc/als_recommend.hip).  The reference blocks
both factor sets, scores a source row against a block of destinations by
sgemv("T") through the Java BLAS (per destination an fp32 dot product, the
products added left to right, unfused), keeps the num greatest per block and
merges the blocks with TopByKeyAggregator.  Here one fused kernel scores and
selects; the scores never reach memory.  score(u, j) has the same bits as
predict gives for the pair.  Absent destinations are never candidates.  The
order is score descending under java.lang.Float.compare (NaN canonical and above
everything, -0.0 below +0.0); EQUAL SCORES GO TO THE LOWER DESTINATION ID.  Spark
leaves ties to its bounded queue's internals; the rule is this project's, and
it makes the order total, so blockSize (accepted, as in Spark) and the kernel's
tiles and splits cannot change a result.  ALSModel.recommendForAllUsers /
recommendForAllItems / recommendForUserSubset / recommendForItemSubset return
(srcIds int32 [P], recIds int32 [P x n'], ratings float32 [P x n']) on the
device: the P present source ids ascending (a subset: its distinct known and
present ids; Spark's join drops the others too) and n' = min(num, present
destinations), the length of Spark's arrays.

Not provided: multi-rank fits (the factor all-gather between half-steps),
nonnegative = True (NNLS), rank > 64, more than MAX_RECOMMEND = 128
recommendations per id.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _native as N
from .regression import SingularMatrixException

MAX_RANK = 64
SEGMENT = 1024                # csrc/als.hip kSegment (cyc_als_segment)
COLD_START = ("nan", "drop")
MAX_RECOMMEND = 128           # csrc/als_recommend.hip kMaxNum (cyc_als_recommend_max_num)


def check_num(num):
    if int(num) < 1 or int(num) > MAX_RECOMMEND:
        raise N.IllegalArgumentException(
            "requirement failed: the number of recommendations must be in "
            f"[1, {MAX_RECOMMEND}] but got {num}")


def check_rank(rank):
    if int(rank) < 1 or int(rank) > MAX_RANK:
        raise N.IllegalArgumentException(
            f"requirement failed: ALS supports rank 1 to {MAX_RANK} but got {rank}")


def _dev(t, dtype, what, n=None):
    import torch
    if not torch.is_tensor(t) or t.dtype != dtype or not t.is_contiguous() \
            or (n is not None and t.numel() != n):
        size = "" if n is None else f"{n} "
        raise N.IllegalArgumentException(
            f"requirement failed: {what} must be {size}contiguous {dtype} device values")
    return t


class ALSSide:
    """cyc_als_side: one side's device CSR (kept alive here), checked on the
    device and cut into segments once."""

    def __init__(self, lib, rowptr, colidx, values, m, nsrc, rank):
        import torch
        self.m, self.nsrc, self.rank = int(m), int(nsrc), int(rank)
        self.rowptr = _dev(rowptr, torch.int64, "rowptr", self.m + 1)
        self.nnz = int(colidx.numel()) if torch.is_tensor(colidx) else -1
        self.colidx = _dev(colidx, torch.int32, "colidx")
        self.values = _dev(values, torch.float32, "values", self.nnz)
        self._lib = lib
        h = ctypes.c_void_p()
        N.check(lib.cyc_als_side_create(N.ptr(self.rowptr), N.ptr(self.colidx),
                                        N.ptr(self.values), self.m, self.nnz, self.nsrc,
                                        self.rank, N.stream_handle(), ctypes.byref(h)))
        self.handle = h

    def close(self):
        if getattr(self, "handle", None):
            self._lib.cyc_als_side_destroy(self.handle)
            self.handle = None

    __del__ = close


class ALSPlan:
    """A thin wrapper over cyc_als_*: sides, YtY, the half-step and predict of
    one rank."""

    segment = SEGMENT         # L: at most this many ratings of a row per workgroup

    def __init__(self, rank: int):
        check_rank(rank)
        self.rank = int(rank)
        # torch (and the HIP runtime it carries) before libcyclone's: a process
        # that loads them the other way round finds no device
        import torch  # noqa: F401
        self._lib = N.load()

    def side(self, rowptr, colidx, values, m: int, nsrc: int) -> ALSSide:
        return ALSSide(self._lib, rowptr, colidx, values, m, nsrc, self.rank)

    def _factors(self, Y, n, what):
        import torch
        return _dev(Y, torch.float32, what, n * self.rank)

    def yty(self, side: ALSSide, Y):
        """sum_i da_i da_i^T over all rows of Y (rank x rank fp64, device)."""
        import torch
        self._factors(Y, side.nsrc, "the source factors")
        out = torch.empty((self.rank, self.rank), dtype=torch.float64, device=Y.device)
        N.check(self._lib.cyc_als_yty_dev(side.handle, N.ptr(Y), N.ptr(out), N.stream_handle()))
        return out

    def solve(self, side: ALSSide, Y, regParam, implicitPrefs=False, alpha=1.0, yty=None):
        """(X (m x rank float32), present (m uint8)), both on the device."""
        import torch
        self._factors(Y, side.nsrc, "the source factors")
        if yty is not None:
            _dev(yty, torch.float64, "yty", self.rank * self.rank)
        X = torch.empty((side.m, self.rank), dtype=torch.float32, device=Y.device)
        present = torch.empty(side.m, dtype=torch.uint8, device=Y.device)
        info = torch.empty(1, dtype=torch.int64, device=Y.device)
        N.check(self._lib.cyc_als_solve_dev(side.handle, N.ptr(Y), float(regParam),
                                            int(bool(implicitPrefs)), float(alpha), N.ptr(yty),
                                            N.ptr(X), N.ptr(present), N.ptr(info),
                                            N.stream_handle()))
        self.lastX = X        # what the other rows got, when the call raises
        row = int(info.item())
        if row >= 0:
            raise SingularMatrixException(
                f"ALS: the normal equation of row {row} is not positive definite (a pivot of "
                "its Cholesky factorization is not positive); is regParam 0 and the row short "
                "of ratings?")
        return X, present

    def predict(self, U, userPresent, V, itemPresent, users, items):
        import torch
        nu, nv = int(U.shape[0]), int(V.shape[0])
        self._factors(U, nu, "the user factors")
        self._factors(V, nv, "the item factors")
        n = int(users.numel()) if torch.is_tensor(users) else -1
        _dev(users, torch.int32, "users")
        _dev(items, torch.int32, "items", n)
        if userPresent is not None:
            _dev(userPresent, torch.uint8, "the user mask", nu)
        if itemPresent is not None:
            _dev(itemPresent, torch.uint8, "the item mask", nv)
        out = torch.empty(n, dtype=torch.float32, device=U.device)
        N.check(self._lib.cyc_als_predict_dev(N.ptr(U), N.ptr(userPresent), nu, N.ptr(V),
                                              N.ptr(itemPresent), nv, self.rank, N.ptr(users),
                                              N.ptr(items), n, N.ptr(out), N.stream_handle()))
        return out

    # the shapes of csrc/als_recommend.hip (pure functions, no device needed)
    def recommend_src_tile(self) -> int:
        """Source rows per workgroup."""
        return int(self._lib.cyc_als_recommend_src_tile())

    def recommend_dst_tile(self) -> int:
        """Destination rows per LDS tile at this rank."""
        return int(self._lib.cyc_als_recommend_dst_tile(self.rank))

    def recommend_max_num(self) -> int:
        return int(self._lib.cyc_als_recommend_max_num())

    def recommend_lds_num(self) -> int:
        """The greatest num whose lists are kept in LDS (another path above)."""
        return int(self._lib.cyc_als_recommend_lds_num())

    def recommend_splits(self, m: int, ndst: int) -> int:
        """Pieces the destination range is cut into for m requested rows."""
        return int(self._lib.cyc_als_recommend_splits(int(m), int(ndst)))

    def recommend_span(self, m: int, ndst: int) -> int:
        """Destinations per piece: piece s is [s span, min(ndst, (s + 1) span))."""
        return int(self._lib.cyc_als_recommend_span(int(m), int(ndst)))

    def recommend_workspace(self, m: int, ndst: int, num: int) -> int:
        return int(self._lib.cyc_als_recommend_workspace(int(m), int(ndst), self.rank, int(num)))

    def recommend(self, S, srcPresent, D, dstPresent, num, srcIds=None):
        """(ids int32 [m x num], scores float32 [m x num]) on the device: per
        requested source row (srcIds, any order, repeats allowed; None: every
        row of S) the num best present destinations, score descending under
        Float.compare, ties to the lower id; -1 / NaN past the candidates and
        in the whole row of a source id that is out of range or absent."""
        import torch
        check_num(num)
        num = int(num)
        ns, nd = int(S.shape[0]), int(D.shape[0])
        self._factors(S, ns, "the source factors")
        self._factors(D, nd, "the destination factors")
        if srcPresent is not None:
            _dev(srcPresent, torch.uint8, "the source mask", ns)
        if dstPresent is not None:
            _dev(dstPresent, torch.uint8, "the destination mask", nd)
        m = ns
        if srcIds is not None:
            m = int(srcIds.numel()) if torch.is_tensor(srcIds) else -1
            _dev(srcIds, torch.int32, "srcIds")
        ids = torch.empty((m, num), dtype=torch.int32, device=S.device)
        scores = torch.empty((m, num), dtype=torch.float32, device=S.device)
        nbytes = self.recommend_workspace(m, nd, num)
        ws = torch.empty(max(1, nbytes // 8), dtype=torch.int64, device=S.device)
        N.check(self._lib.cyc_als_recommend_dev(
            N.ptr(S), N.ptr(srcPresent), ns, N.ptr(srcIds), m, N.ptr(D), N.ptr(dstPresent), nd,
            self.rank, num, N.ptr(ids), N.ptr(scores), N.ptr(ws), nbytes, N.stream_handle()))
        return ids, scores


def init_factors(present, rank: int, seed: int) -> np.ndarray:
    """len(present) x rank float32: a unit-norm row of standard normals per
    present id (normalized in float32, snrm2 / sscal), zero rows elsewhere."""
    present = np.asarray(present).astype(bool)
    g = np.random.default_rng(int(seed)).standard_normal((present.size, int(rank)))
    g = g.astype(np.float32)
    nrm = np.sqrt((g * g).sum(axis=1, dtype=np.float32))
    g *= (np.float32(1.0) / nrm)[:, None]
    g[~present] = 0.0
    return g


def build_side(dst, src, ratings, m: int):
    """(rowptr, colidx, values) of the ratings grouped by dst (device int32 ids;
    a stable sort, so a row keeps its ratings in the COO order)."""
    import torch
    order = torch.sort(dst, stable=True)[1]
    counts = torch.bincount(dst.to(torch.int64), minlength=m)
    rowptr = torch.zeros(m + 1, dtype=torch.int64, device=dst.device)
    rowptr[1:] = torch.cumsum(counts, 0)
    return rowptr, src[order].contiguous(), ratings[order].contiguous()


class ALSModel:
    """rank, userFactors / itemFactors (float32, one row per id) and the
    presence masks (uint8).  Device tensors or host arrays; predict and
    transform need device tensors, save / load work on the host."""

    def __init__(self, rank, userFactors, itemFactors, userPresent=None, itemPresent=None,
                 coldStartStrategy="nan"):
        check_cold_start(coldStartStrategy)
        self.rank = int(rank)
        self.userFactors = userFactors
        self.itemFactors = itemFactors
        for f in (userFactors, itemFactors):
            if len(f.shape) != 2 or int(f.shape[1]) != self.rank:
                raise N.IllegalArgumentException(
                    f"requirement failed: factors must be (ids x {self.rank}) float32")
        self.userPresent = _mask(userPresent, userFactors)
        self.itemPresent = _mask(itemPresent, itemFactors)
        self.coldStartStrategy = coldStartStrategy

    def _device(self, like):
        import torch

        def up(a, dtype):
            if torch.is_tensor(a):
                return a.to(device=like.device, dtype=dtype).contiguous()
            return torch.from_numpy(np.ascontiguousarray(a)).to(like.device).to(dtype)
        return (up(self.userFactors, torch.float32), up(self.userPresent, torch.uint8),
                up(self.itemFactors, torch.float32), up(self.itemPresent, torch.uint8))

    def predict(self, users, items):
        """sdot of the two factors per pair (device float32); NaN where an id
        is negative, unknown or without ratings in the fit."""
        import torch
        if not torch.is_tensor(users) or not torch.is_tensor(items):
            raise N.IllegalArgumentException(
                "requirement failed: users and items must be int32 device tensors")
        if users.numel() != items.numel():
            raise N.IllegalArgumentException(
                f"requirement failed: {users.numel()} users but {items.numel()} items")
        U, up, V, vp = self._device(users)
        return ALSPlan(self.rank).predict(U, up, V, vp, users.to(torch.int32).contiguous(),
                                          items.to(torch.int32).contiguous())

    def transform(self, users, items):
        """"nan": the predictions; "drop": (kept_index (int64), predictions of
        the kept pairs), the NaN rows removed."""
        import torch
        p = self.predict(users, items)
        if self.coldStartStrategy == "nan":
            return p
        keep = torch.nonzero(~torch.isnan(p)).view(-1)
        return keep, p[keep]

    def _recommend(self, forUsers, num, subset, blockSize):
        import torch
        check_num(num)
        if int(blockSize) < 1:
            raise N.IllegalArgumentException(f"ALS_blockSize given invalid value {blockSize}")
        like = self.userFactors
        if not (torch.is_tensor(like) and like.is_cuda):
            like = torch.empty(0, device="cuda")
        U, up, V, vp = self._device(like)
        S, sp, D, dp = (U, up, V, vp) if forUsers else (V, vp, U, up)
        src = subset_ids(torch.arange(S.shape[0], device=S.device) if subset is None else subset,
                         sp)
        keep = min(int(num), int(dp.sum()))
        ids, scores = ALSPlan(self.rank).recommend(S, sp, D, dp, num, src)
        return src, ids[:, :keep].contiguous(), scores[:, :keep].contiguous()

    def recommendForAllUsers(self, numItems, blockSize=4096):
        """(users int32 [P], items int32 [P x n'], ratings float32 [P x n']) on
        the device: for each of the P present users, ascending, the n' =
        min(numItems, present items) best items (score descending under
        Float.compare, ties to the lower item id).  blockSize is accepted as in
        Spark and has no effect on the result."""
        return self._recommend(True, numItems, None, blockSize)

    def recommendForAllItems(self, numUsers, blockSize=4096):
        """The same with the sides swapped: per present item its best users."""
        return self._recommend(False, numUsers, None, blockSize)

    def recommendForUserSubset(self, users, numItems, blockSize=4096):
        """recommendForAllUsers for the distinct ids of `users` that are known
        and present, ascending (the others are dropped, as Spark's join does)."""
        return self._recommend(True, numItems, users, blockSize)

    def recommendForItemSubset(self, items, numUsers, blockSize=4096):
        return self._recommend(False, numUsers, items, blockSize)

    def save(self, path, overwrite=False):
        from . import persist
        persist.save_als_model(self, path, overwrite=overwrite)

    @staticmethod
    def load(path):
        from . import persist
        return persist.load_als_model(path)


def _mask(present, factors):
    if present is not None:
        if int(present.shape[0]) != int(factors.shape[0]):
            raise N.IllegalArgumentException(
                "requirement failed: one presence flag per factor row")
        return present
    import torch
    if torch.is_tensor(factors):
        return torch.ones(int(factors.shape[0]), dtype=torch.uint8, device=factors.device)
    return np.ones(int(factors.shape[0]), dtype=np.uint8)


def subset_ids(ids, present):
    """The distinct ids that are in [0, len(present)) and present, ascending
    (int32, on present's device).  ids: a tensor, an array or a list of
    integers; present: a uint8 / bool tensor or array."""
    import torch
    present = present if torch.is_tensor(present) else torch.as_tensor(np.asarray(present))
    ids = ids if torch.is_tensor(ids) else torch.as_tensor(np.asarray(ids))
    if ids.numel() and (ids.dtype.is_floating_point or ids.dtype == torch.bool):
        raise N.IllegalArgumentException("requirement failed: ids must be integers")
    ids = torch.unique(ids.to(device=present.device, dtype=torch.int64).view(-1))
    ids = ids[(ids >= 0) & (ids < present.numel())]
    return ids[present[ids] != 0].to(torch.int32).contiguous()


def check_cold_start(s):
    if s not in COLD_START:
        raise N.IllegalArgumentException(
            f"ALS_coldStartStrategy given invalid value {s}. Supported: "
            + ", ".join(COLD_START))


class ALS:
    """ALS.train on one device: both CSR sides by torch sorts, then maxIter
    times the item half-step and the user half-step (csrc/als.hip).
    initialUserFactors (numUsers x rank float32, host or device) replaces the
    drawn initial factors."""

    def __init__(self, rank=10, maxIter=10, regParam=0.1, implicitPrefs=False, alpha=1.0,
                 nonnegative=False, seed=0, coldStartStrategy="nan", initialUserFactors=None):
        check_rank(rank)
        if int(maxIter) < 0:
            raise N.IllegalArgumentException(f"ALS_maxIter given invalid value {maxIter}")
        if not regParam >= 0:
            raise N.IllegalArgumentException(f"ALS_regParam given invalid value {regParam}")
        if not alpha >= 0:
            raise N.IllegalArgumentException(f"ALS_alpha given invalid value {alpha}")
        if nonnegative:
            raise N.IllegalArgumentException(
                "requirement failed: nonnegative = true (the NNLS solver) is not supported")
        check_cold_start(coldStartStrategy)
        self.rank = int(rank)
        self.maxIter = int(maxIter)
        self.regParam = float(regParam)
        self.implicitPrefs = bool(implicitPrefs)
        self.alpha = float(alpha)
        self.seed = int(seed)
        self.coldStartStrategy = coldStartStrategy
        self.initialUserFactors = initialUserFactors

    @staticmethod
    def check_ratings(users, items, ratings, numUsers=None, numItems=None):
        """(numUsers, numItems) after the input requires."""
        import torch
        for t, dt, what in ((users, torch.int32, "users"), (items, torch.int32, "items"),
                            (ratings, torch.float32, "ratings")):
            if not torch.is_tensor(t) or t.dtype != dt or t.dim() != 1:
                raise N.IllegalArgumentException(
                    f"requirement failed: {what} must be a 1-d {dt} device tensor")
        n = users.numel()
        if items.numel() != n or ratings.numel() != n:
            raise N.IllegalArgumentException(
                f"requirement failed: users, items and ratings must have one length but got "
                f"{n}, {items.numel()} and {ratings.numel()}")
        if n == 0:
            raise N.IllegalArgumentException("requirement failed: No ratings available")
        lo_u, hi_u = int(users.min()), int(users.max())
        lo_i, hi_i = int(items.min()), int(items.max())
        if lo_u < 0 or lo_i < 0:
            raise N.IllegalArgumentException(
                "requirement failed: ALS only supports non-negative ids but got "
                f"{min(lo_u, lo_i)}")
        nu = hi_u + 1 if numUsers is None else int(numUsers)
        ni = hi_i + 1 if numItems is None else int(numItems)
        if hi_u >= nu or hi_i >= ni:
            raise N.IllegalArgumentException(
                f"requirement failed: ids must be below numUsers = {nu} and numItems = {ni} "
                f"but got user {hi_u} and item {hi_i}")
        return nu, ni

    def fit(self, users, items, ratings, numUsers=None, numItems=None) -> ALSModel:
        """users, items (int32), ratings (float32): device COO tensors of one
        length; the id counts default to max id + 1."""
        import torch
        nu, ni = self.check_ratings(users, items, ratings, numUsers, numItems)
        dev = users.device
        users, items, ratings = users.contiguous(), items.contiguous(), ratings.contiguous()
        plan = ALSPlan(self.rank)
        userSide = plan.side(*build_side(users, items, ratings, nu), nu, ni)
        itemSide = plan.side(*build_side(items, users, ratings, ni), ni, nu)
        try:
            up = (userSide.rowptr[1:] > userSide.rowptr[:-1]).to(torch.uint8)
            ip = (itemSide.rowptr[1:] > itemSide.rowptr[:-1]).to(torch.uint8)
            if self.initialUserFactors is not None:
                U = self.initialUserFactors
                if not torch.is_tensor(U):
                    U = torch.from_numpy(np.array(U, dtype=np.float32))
                U = U.to(dev).to(torch.float32).contiguous()
                if tuple(U.shape) != (nu, self.rank):
                    raise N.IllegalArgumentException(
                        f"requirement failed: initialUserFactors must be {nu} x {self.rank} but "
                        f"got {tuple(U.shape)}")
            else:
                U = torch.from_numpy(init_factors(up.cpu().numpy(), self.rank, self.seed)).to(dev)
            V = torch.zeros((ni, self.rank), dtype=torch.float32, device=dev)
            for _ in range(self.maxIter):
                V, ip = plan.solve(itemSide, U, self.regParam, self.implicitPrefs, self.alpha)
                U, up = plan.solve(userSide, V, self.regParam, self.implicitPrefs, self.alpha)
        finally:
            userSide.close()
            itemSide.close()
        return ALSModel(self.rank, U, V, up, ip, self.coldStartStrategy)
