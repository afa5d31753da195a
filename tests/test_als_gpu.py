"""ALS on the device (csrc/als.hip) against the numpy restatement of
tests/als_restatement.py, which walks every row's ratings in order.

Half-step bar (derived, not measured), from the project's 1e-10 fp64 contract
on the system and one fp32 rounding of the solution.  With ref64 the
restatement's solution before rounding, A_u its regularised system and kappa_u
= cond(A_u):
    e_u = 1e-10 kappa_u max_i |ref64_i|
    |got_i - ref64_i| <= 2^-24 (|ref64_i| + e_u) + e_u
Condition, asserted on the reference alone: kappa_u <= 1e4 for every row.  The
inputs keep it: unit-norm source rows, regParam = 0.1, at least one positive
rating per non-empty implicit row, nsrc >= 4 rank where YtY carries a row.

Every device call runs twice and the two results are compared by tobytes().
"""
import functools

import numpy as np
import pytest

import als_restatement as R
from cycloneml_amd import _native as N
from cycloneml_amd import recommendation as rec
from cycloneml_amd.recommendation import ALS, ALSModel, ALSPlan
from cycloneml_amd.regression import SingularMatrixException

pytestmark = pytest.mark.gpu

L = ALSPlan.segment
LENGTHS = [0, 1, 3, 4, 5, L - 1, L, L + 1, 2 * L + 1, 3 * L + 5]
SHORT = [0, 1, 3, 4, 5]
RANKS = [1, 3, 10, 15, 16, 17, 32, 33, 64]
MS = [1, 63, 64, 65, 257]
REG = 0.1
ALPHA = 0.5
# every rank at m = 65, every m at ranks 10 and 17; explicit and implicit
CASES = [(rank, 65, imp) for rank in RANKS for imp in (False, True)] + \
        [(rank, m, imp) for rank in (10, 17) for m in MS if m != 65 for imp in (False, True)]


def dev():
    import torch
    return torch.device("cuda:0")


def to_dev(a):
    import torch
    return torch.from_numpy(np.array(a)).to(dev())     # a copy: the cached inputs are frozen


def unit_rows(rng, n, rank):
    Y = rng.standard_normal((n, rank))
    Y /= np.sqrt((Y * Y).sum(axis=1))[:, None]
    return Y.astype(np.float32)


def nsrc_of(rank, m, imp):
    """7 .. 5000: a handful of source rows gathered over and over, or gathers
    scattered over thousands; implicit sides keep nsrc >= 4 rank."""
    n = [7, 100, 5000][(rank + m) % 3]
    return max(n, 4 * rank) if imp else n


@functools.lru_cache(maxsize=None)
def side_of(rank, m, imp):
    """One side with every length of LENGTHS (the first ten rows; a single row
    takes the longest), short rows after, duplicates of (row, source) pairs,
    and its restatement.  Implicit ratings hold zeros and negatives, and the
    first rating of a row is positive."""
    rng = np.random.default_rng(1000003 * rank + 101 * m + imp)
    nsrc = nsrc_of(rank, m, imp)
    shift = 9 if m == 1 else 0
    lens = [LENGTHS[(u + shift) % 10] if u < 10 else SHORT[u % 5] for u in range(m)]
    rowptr = np.zeros(m + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum(lens)
    nnz = int(rowptr[-1])
    colidx = rng.integers(0, nsrc, nnz).astype(np.int32)
    if imp:
        vals = rng.integers(-2, 6, nnz).astype(np.float32)
        vals[rowptr[:-1][np.array(lens) > 0]] = 3.0
    else:
        vals = rng.uniform(-2.0, 5.0, nnz).astype(np.float32)
    for u in range(m):                      # duplicate pairs, also in short rows
        if lens[u] >= 3:
            colidx[rowptr[u] + 2] = colidx[rowptr[u]]
    Y = unit_rows(rng, nsrc, rank)
    ref = R.half_step(rowptr, colidx, vals, Y, REG, imp, ALPHA)
    for a in (rowptr, colidx, vals, Y, *[v for v in ref.values() if isinstance(v, np.ndarray)]):
        a.setflags(write=False)
    return rowptr, colidx, vals, Y, nsrc, ref


def check_half_step(X, present, ref):
    """The module docstring's bar, row by row."""
    assert not ref["singular"]
    assert np.array_equal(present.astype(bool), ref["present"])
    assert X.dtype == np.float32 and not np.isnan(X).any()
    for u in range(len(present)):
        if not ref["present"][u]:
            assert not X[u].any(), f"row {u} has no ratings but a factor"
            continue
        kappa = np.linalg.cond(ref["A"][u])
        assert kappa <= 1e4, (u, kappa)
        x = ref["x64"][u]
        e = 1e-10 * kappa * np.abs(x).max()
        bar = 2.0 ** -24 * (np.abs(x) + e) + e
        err = np.abs(X[u].astype(np.float64) - x)
        assert np.all(err <= bar), (u, float((err / bar).max()))


def twice(fn):
    """fn() twice; every returned device tensor must repeat bit for bit."""
    a, b = fn(), fn()
    a = a if isinstance(a, tuple) else (a,)
    b = b if isinstance(b, tuple) else (b,)
    outs = [t.cpu().numpy() for t in a]
    for x, y in zip(outs, b):
        assert x.tobytes() == y.cpu().numpy().tobytes(), "two calls differ"
    return outs if len(outs) > 1 else outs[0]


@pytest.mark.parametrize("rank,m,imp", CASES)
def test_half_step(cuda, rank, m, imp):
    rowptr, colidx, vals, Y, nsrc, ref = side_of(rank, m, imp)
    plan = ALSPlan(rank)
    side = plan.side(to_dev(rowptr), to_dev(colidx), to_dev(vals), m, nsrc)
    Yd = to_dev(Y)
    X, present = twice(lambda: plan.solve(side, Yd, REG, imp, ALPHA))
    check_half_step(X, present, ref)
    if imp:
        # YtY on its own: the same bits as inside the call, and the restatement's
        # within 1e-10 of the sum of absolute products
        G = twice(lambda: plan.yty(side, Yd))
        want = R.unpack(R.yty(Y), rank)
        Ya = np.abs(Y.astype(np.float64))
        assert np.all(np.abs(G - want) <= 1e-10 * (Ya.T @ Ya))
        assert np.array_equal(G, G.T)
        X2, _ = twice(lambda: plan.solve(side, Yd, REG, imp, ALPHA, yty=to_dev(G)))
        assert X2.tobytes() == X.tobytes()
    side.close()


@pytest.mark.parametrize("what", ["colidx_high", "colidx_negative", "rowptr_decreasing",
                                  "rowptr_end", "rowptr_start"])
def test_side_validation(cuda, what):
    """A bad structure is refused when the side is created: nothing gathers
    through it."""
    rowptr = np.array([0, 2, 5, 5, 9], dtype=np.int64)
    colidx = np.array([0, 1, 2, 3, 4, 0, 1, 2, 3], dtype=np.int32)
    vals = np.ones(9, dtype=np.float32)
    match = "source ids must be in"
    if what == "colidx_high":
        colidx[6] = 5
    elif what == "colidx_negative":
        colidx[2] = -1
    elif what == "rowptr_decreasing":
        rowptr[2], match = 1, "non-decreasing"
    elif what == "rowptr_end":
        rowptr[4], match = 8, "must end at nnz"
    else:
        rowptr[0], match = 1, "must start at 0"
    plan = ALSPlan(3)
    with pytest.raises(N.IllegalArgumentException, match=match):
        plan.side(to_dev(rowptr), to_dev(colidx), to_dev(vals), 4, 5)


def test_singular_row_is_named_and_the_others_solved(cuda):
    """Explicit, regParam 0, rank 3: a row of one rating has a rank-1 system."""
    rng = np.random.default_rng(11)
    rowptr = np.array([0, 6, 12, 13, 13, 20], dtype=np.int64)
    colidx = rng.integers(0, 40, 20).astype(np.int32)
    vals = rng.uniform(1.0, 5.0, 20).astype(np.float32)
    Y = unit_rows(rng, 40, 3)
    # the lone rating's source row in exact arithmetic: ata = 0.25 everywhere,
    # so the second pivot is 0.25 - 0.5 * 0.5 = 0 on every side, not a rounding
    Y[colidx[12]] = 0.5
    ref = R.half_step(rowptr, colidx, vals, Y, 0.0)
    assert ref["singular"] == [2]
    plan = ALSPlan(3)
    side = plan.side(to_dev(rowptr), to_dev(colidx), to_dev(vals), 5, 40)
    for _ in range(2):
        with pytest.raises(SingularMatrixException, match="row 2 "):
            plan.solve(side, to_dev(Y), 0.0)
        X = plan.lastX.cpu().numpy()
        assert not np.isnan(X).any() and not X[2].any() and not X[3].any()
        ref_ok = dict(ref, singular=[])
        ref_ok["present"] = ref["present"].copy()
        ref_ok["present"][2] = False           # checked above: a zero factor
        present = ref_ok["present"].astype(np.uint8)
        check_half_step(X, present, ref_ok)
    side.close()


@pytest.mark.parametrize("rank", [1, 10, 17, 64])
def test_predict(cuda, rank):
    rng = np.random.default_rng(rank)
    nu, ni, n = 37, 23, 1000
    U = rng.standard_normal((nu, rank)).astype(np.float32)
    V = rng.standard_normal((ni, rank)).astype(np.float32)
    up = (rng.random(nu) < 0.9).astype(np.uint8)
    vp = (rng.random(ni) < 0.9).astype(np.uint8)
    users = rng.integers(0, nu, n).astype(np.int32)
    items = rng.integers(0, ni, n).astype(np.int32)
    users[[3, 500]] = [-1, nu]
    items[[7, 900]] = [ni + 5, -3]
    want = R.predict(U, up, V, vp, users, items)
    model = ALSModel(rank, to_dev(U), to_dev(V), to_dev(up), to_dev(vp))
    got = twice(lambda: model.predict(to_dev(users), to_dev(items)))
    assert got.dtype == np.float32
    nan = np.isnan(want)
    assert nan[[3, 500, 7, 900]].all() and nan.sum() > 4 and not nan.all()
    assert np.array_equal(np.isnan(got), nan)
    assert got[~nan].tobytes() == want[~nan].tobytes()
    # the model on host arrays predicts the same, and "drop" keeps the rest
    host = ALSModel(rank, U, V, up, vp, "drop")
    keep, p = host.transform(to_dev(users), to_dev(items))
    assert np.array_equal(keep.cpu().numpy(), np.nonzero(~nan)[0])
    assert p.cpu().numpy().tobytes() == want[~nan].tobytes()


@functools.lru_cache(maxsize=None)
def ratings_60x45():
    """60 x 45 ids, about 1200 ratings with duplicates; user 13 and item 7
    have none."""
    rng = np.random.default_rng(2024)
    nu, ni, n, rank = 60, 45, 1200, 5
    users = rng.integers(0, nu, n).astype(np.int32)
    items = rng.integers(0, ni, n).astype(np.int32)
    users[users == 13] = 14
    items[items == 7] = 8
    Ut = rng.standard_normal((nu, rank))
    Vt = rng.standard_normal((ni, rank))
    ratings = ((Ut[users] * Vt[items]).sum(axis=1) * 0.5 + 3.0
               + 0.1 * rng.standard_normal(n)).astype(np.float32)
    up = np.bincount(users, minlength=nu) > 0
    U0 = rec.init_factors(up, rank, 3)
    for a in (users, items, ratings, U0):
        a.setflags(write=False)
    return users, items, ratings, nu, ni, rank, U0


def test_fit_teacher_forced(cuda):
    """Three iterations; every device half-step is fed the restatement's
    previous factors and meets the half-step bar."""
    users, items, ratings, nu, ni, rank, U0 = ratings_60x45()
    userSide = R.build_side(users, items, ratings, nu)
    itemSide = R.build_side(items, users, ratings, ni)
    plan = ALSPlan(rank)
    du, di, dr = to_dev(users), to_dev(items), to_dev(ratings)
    dUser = plan.side(*rec.build_side(du, di, dr, nu), nu, ni)
    dItem = plan.side(*rec.build_side(di, du, dr, ni), ni, nu)
    for got, want in zip((dUser, dItem), (userSide, itemSide)):     # the same CSR
        assert np.array_equal(got.rowptr.cpu().numpy(), want[0])
        assert np.array_equal(got.colidx.cpu().numpy(), want[1])
        assert got.values.cpu().numpy().tobytes() == want[2].tobytes()
    U = U0
    for _ in range(3):
        ref = R.half_step(*itemSide, U, REG)
        X, present = twice(lambda: plan.solve(dItem, to_dev(U), REG))
        check_half_step(X, present, ref)
        assert not present[7]
        V = ref["X"]
        ref = R.half_step(*userSide, V, REG)
        X, present = twice(lambda: plan.solve(dUser, to_dev(V), REG))
        check_half_step(X, present, ref)
        assert not present[13]
        U = ref["X"]


def test_fit_free_running_objective_never_rises(cuda, capsys):
    """Explicit feedback.  Each half-step is the exact minimiser of the
    regularised objective in its own factors, so it cannot raise it; rounding
    the minimiser to fp32 moves the objective at second order only (about
    1e-14 relative), a wrong solve at order one: obj_next <= obj_prev (1 +
    1e-6) after every half-step."""
    users, items, ratings, nu, ni, rank, U0 = ratings_60x45()
    plan = ALSPlan(rank)
    du, di, dr = to_dev(users), to_dev(items), to_dev(ratings)
    dUser = plan.side(*rec.build_side(du, di, dr, nu), nu, ni)
    dItem = plan.side(*rec.build_side(di, du, dr, ni), ni, nu)
    iters = 4
    U = to_dev(U0)
    objs = []
    for _ in range(iters):
        V, _ = plan.solve(dItem, U, REG)
        objs.append(R.objective(users, items, ratings, U.cpu().numpy(), V.cpu().numpy(), REG))
        U, _ = plan.solve(dUser, V, REG)
        objs.append(R.objective(users, items, ratings, U.cpu().numpy(), V.cpu().numpy(), REG))
    for prev, nxt in zip(objs, objs[1:]):
        assert nxt <= prev * (1.0 + 1e-6), objs
    assert objs[-1] < 0.5 * objs[0]
    # the estimator runs this very loop
    est = ALS(rank=rank, maxIter=iters, regParam=REG, initialUserFactors=U0)
    model = twice(lambda: (lambda m: (m.userFactors, m.itemFactors, m.userPresent,
                                      m.itemPresent))(est.fit(du, di, dr)))
    assert model[0].tobytes() == U.cpu().numpy().tobytes()
    assert model[1].tobytes() == V.cpu().numpy().tobytes()
    assert not model[2][13] and not model[3][7] and model[2].sum() == nu - 1
    # recorded in DESIGN.md, not asserted: the free-running drift of the RMSE
    refV, refU = R.fit(users, items, ratings, nu, ni, U0, iters, REG)[-1]
    got = R.rmse(users, items, ratings, model[0], model[1])
    want = R.rmse(users, items, ratings, refU, refV)
    with capsys.disabled():
        print(f"\nALS free-running, {iters} iterations: rmse device {got:.12g} restatement "
              f"{want:.12g} drift {abs(got - want):.3g}")


def test_fit_drawn_initial_factors_and_implicit(cuda):
    """fit() without initialUserFactors draws them from the seed; an implicit
    fit runs and marks the ids without ratings."""
    users, items, ratings, nu, ni, rank, _ = ratings_60x45()
    du, di, dr = to_dev(users), to_dev(items), to_dev(ratings)
    a = ALS(rank=rank, maxIter=2, seed=9).fit(du, di, dr)
    b = ALS(rank=rank, maxIter=2, seed=9).fit(du, di, dr)
    c = ALS(rank=rank, maxIter=2, seed=10).fit(du, di, dr)
    assert a.userFactors.cpu().numpy().tobytes() == b.userFactors.cpu().numpy().tobytes()
    assert a.userFactors.cpu().numpy().tobytes() != c.userFactors.cpu().numpy().tobytes()
    up = np.bincount(users, minlength=nu) > 0
    U0 = rec.init_factors(up, rank, 9)
    U0 = rec.init_factors(np.bincount(users, minlength=nu + 2) > 0, rank, 9)
    m = ALS(rank=rank, maxIter=1, implicitPrefs=True, alpha=ALPHA, seed=9).fit(du, di, dr, nu + 2)
    assert m.userFactors.shape == (nu + 2, rank)
    assert not m.userPresent.cpu().numpy()[[13, nu, nu + 1]].any()
    # one iteration is two chained half-steps: the item factors from the drawn
    # U0, then the user factors from the DEVICE's item factors (teacher-forced
    # the other way round), each to the half-step bar
    V = m.itemFactors.cpu().numpy()
    ref = R.half_step(*R.build_side(items, users, ratings, ni), U0, REG, True, ALPHA)
    check_half_step(V, m.itemPresent.cpu().numpy(), ref)
    ref = R.half_step(*R.build_side(users, items, ratings, nu + 2), V, REG, True, ALPHA)
    check_half_step(m.userFactors.cpu().numpy(), m.userPresent.cpu().numpy(), ref)
