"""FM over CSR rows on the device (csrc/fm_csr.hip) against the restatement on
the densified rows: exact inputs by bytes at the kernels' edges (the wave's
chunk of 64 non-zeros, the lane layouts of every factor count, the segment
length of a column, the run), real inputs within the sums' bars and against the
dense kernels, predict, the label refusal, one whole fit per solver and the
header's symbols.  Every device call runs twice and must give the same bytes."""
import functools

import numpy as np
import pytest
import torch

import fm_restatement as R
from cycloneml_amd import _native as N
from cycloneml_amd import fm
from cycloneml_amd.linalg import CSRRows

pytestmark = pytest.mark.gpu
RUN = 1024              # cyc_fm_run_rows


def dev(a, cuda, dtype=np.float64):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(cuda)


def csr(X, cuda, base=0):
    """The non-zeros of dense host rows as device CSRRows."""
    mask = X != 0
    rowptr = np.concatenate([[0], np.cumsum(mask.sum(1))]) + base
    return CSRRows(dev(rowptr, cuda, np.int64), dev(np.nonzero(mask)[1], cuda, np.int32),
                   dev(X[mask], cuda), X.shape[1])


def evaluate_twice(plan, rows, y, coef, cuda, **kw):
    yd, cd = dev(y, cuda), dev(coef, cuda)
    a = plan.evaluate(rows, yd, cd, **kw).cpu().numpy()
    b = plan.evaluate(rows, yd, cd, **kw).cpu().numpy()
    assert a.tobytes() == b.tobytes()
    return a


@functools.lru_cache(maxsize=None)
def exact(n, d, k, lens=(6,), cols=(), fitIntercept=True, fitLinear=True):
    """R.exact_rows' recipe (x integer in [-2, 2], coefficients and labels in
    quarters) with row r holding lens[r % len(lens)] non-zeros and column c
    then reset to `length` non-zeros for every (c, length) of cols; forward and
    reverse row order must give the same reference bytes."""
    rng = np.random.default_rng(11)
    X = np.zeros((n, d))
    for r in range(n):
        at = rng.choice(d, size=min(d, lens[r % len(lens)]), replace=False)
        X[r, at] = rng.choice([-2.0, -1.0, 1.0, 2.0], size=at.size)
    for c, length in cols:
        X[:, c] = 0.0
        X[n - length:, c] = rng.choice([-2.0, -1.0, 1.0, 2.0], size=length)
    size = d * k + (d if fitLinear else 0) + (1 if fitIntercept else 0)
    coef = rng.integers(-2, 3, size=size) / 4.0
    y = rng.integers(-4, 5, size=n) / 4.0
    ref = R.evaluate(X, y, coef, k, "squared", fitIntercept, fitLinear)
    rev = R.evaluate(X, y, coef, k, "squared", fitIntercept, fitLinear, order=range(n - 1, -1, -1))
    assert ref[0].tobytes() == rev[0].tobytes() and ref[1:] == rev[1:]
    return X, y, coef, ref


def check_exact(cuda, case, k, fitIntercept=True, fitLinear=True):
    X, y, coef, (G, L, cnt) = case
    plan = fm.FMPlan(X.shape[1], k, fitIntercept, fitLinear)
    got = evaluate_twice(plan, fm.FMSparseRows(csr(X, cuda)), y, coef, cuda)
    assert got.tobytes() == np.concatenate([G, [L, cnt]]).tobytes()


ROW_LENS = (0, 1, 63, 0, 64, 65, 129, 0)     # an empty row first, in the middle and last


@pytest.mark.parametrize("k", [1, 2, 3, 8, 9, 63, 64])
def test_row_lengths_at_the_wave_chunk(cuda, k):
    check_exact(cuda, exact(len(ROW_LENS), 200, k, ROW_LENS), k)


@pytest.mark.parametrize("k", [1, 3, 8, 64])
def test_column_lengths_at_the_segment(cuda, k):
    seg = int(N.load().cyc_fmcsr_segment_entries())
    lengths = (0, 1, seg - 1, seg, seg + 1, 2 * seg + 3)
    case = exact(2 * seg + 3, len(lengths), k, (0,), tuple(enumerate(lengths)))
    assert tuple((case[0] != 0).sum(0)) == lengths
    check_exact(cuda, case, k)


@pytest.mark.parametrize("n, d, k", [(1, 17, 8), (63, 17, 8), (65, 17, 8), (RUN + 1, 17, 8),
                                     (33, 65537, 2)])
def test_row_counts_and_a_width_beyond_the_dense_limit(cuda, n, d, k):
    assert N.load().cyc_fm_max_features() < 65537
    check_exact(cuda, exact(n, d, k), k)


@pytest.mark.parametrize("fitIntercept, fitLinear", [(False, True), (True, False)])
def test_flag_off_layouts(cuda, fitIntercept, fitLinear):
    check_exact(cuda, exact(33, 40, 8, (6,), (), fitIntercept, fitLinear), 8, fitIntercept,
                fitLinear)


def test_fraction_takes_the_host_rules_rows(cuda):
    X, y, coef, _ = exact(200, 17, 8)
    G, L, cnt = R.evaluate(X, y, coef, 8, "squared", i=3, fraction=0.5, rowOffset=7)
    assert 0 < cnt < 200
    got = evaluate_twice(fm.FMPlan(17, 8), fm.FMSparseRows(csr(X, cuda)), y, coef, cuda, iter=3,
                         fraction=0.5, rowOffset=7)
    assert got.tobytes() == np.concatenate([G, [L, cnt]]).tobytes()


def test_nonzero_rowptr_base(cuda):
    X, y, coef, (G, L, cnt) = exact(65, 17, 8)
    got = evaluate_twice(fm.FMPlan(17, 8), csr(X, cuda, base=5), y, coef, cuda)   # bare CSRRows
    assert got.tobytes() == np.concatenate([G, [L, cnt]]).tobytes()


def thin_rows(n, d, seed, classifier=False):
    X, y = R.real_rows(n, d, seed, classifier)                  # 70 % dense
    return X * (np.random.default_rng(seed + 1).random((n, d)) < 0.07), y


@pytest.mark.parametrize("loss", ["squared", "logistic"])
def test_real_inputs_within_the_sums_bars(cuda, loss):
    d = 400
    X, y = thin_rows(50, d, 5, loss == "logistic")
    coef = np.random.default_rng(6).normal(size=d * 3 + d + 1) * 0.1
    G, L, cnt, _, _, GAbs, LAbs = R.evaluate(X, y, coef, 3, loss, bars=True)
    plan = fm.FMPlan(d, 3, loss=loss)
    got = evaluate_twice(plan, fm.FMSparseRows(csr(X, cuda)), y, coef, cuda)
    assert np.all(np.abs(got[:-2] - G) <= 1e-10 * GAbs)
    assert abs(got[-2] - L) <= 1e-10 * LAbs and got[-1] == cnt
    dense = evaluate_twice(plan, dev(X, cuda), y, coef, cuda)
    assert np.all(np.abs(got[:-2] - dense[:-2]) <= 1e-10 * GAbs)
    assert abs(got[-2] - dense[-2]) <= 1e-10 * LAbs and got[-1] == dense[-1]


def test_predict_of_both_models(cuda):
    d = 400
    X, _ = thin_rows(37, d, 8)
    rng = np.random.default_rng(9)
    b, w, V = rng.normal(), rng.normal(size=d) * 0.1, rng.normal(size=(d, 8)) * 0.1
    coef = np.concatenate([V.ravel(), w, [b]])
    _, _, _, raw, bar = R.evaluate(X, np.zeros(37), coef, 8, "squared", bars=True)[:5]
    rows = fm.FMSparseRows(csr(X, cuda))
    reg, cls = fm.FMRegressionModel(b, w, V), fm.FMClassificationModel(b, w, V)
    got = reg.predict(rows).cpu().numpy()
    assert reg.predict(csr(X, cuda)).cpu().numpy().tobytes() == got.tobytes()
    assert np.all(np.abs(got - raw) <= 1e-10 * bar)
    r2, p2, lab = (t.cpu().numpy() for t in (cls.predictRaw(rows), cls.predictProbability(rows),
                                             cls.predict(rows)))
    assert np.array_equal(r2[:, 1], got) and np.array_equal(r2[:, 0], -got)
    p = 1.0 / (1.0 + np.exp(-raw))
    # |dp / draw| <= 1/4, and a few ulps of exp and the division on p <= 1
    assert np.all(np.abs(p2[:, 1] - p) <= 1e-10 * 0.25 * bar + 1e-15)
    assert np.array_equal(p2[:, 0], 1.0 - p2[:, 1])
    sure = np.abs(raw) > 1e-10 * bar
    assert np.array_equal(lab[sure], (raw > 0).astype(np.float64)[sure])


def test_classifier_names_the_lowest_bad_row(cuda):
    X, y = R.real_rows(RUN + 40, 9, 1, True)
    y[RUN + 6] = 2.0
    y[5] = -1.0
    plan = fm.FMPlan(9, 2, loss="logistic")
    with pytest.raises(N.IllegalArgumentException, match="row 105 "):
        plan.evaluate(csr(X, cuda), dev(y, cuda), dev(np.zeros(9 * 3 + 1), cuda), rowOffset=100)


@pytest.mark.parametrize("solver", ["gd", "adamW"])
def test_whole_fit_on_the_device_step(cuda, solver):
    """max|dcoef| / max|coef| against the FMNumpyStep fit on the densified rows.
    Measured on an MI355X: 1.111e-16 (gd), 1.133e-14 (adamW); asserted at 100 x
    that, rounded up to a power of ten (never looser than 1e-8)."""
    X, y = thin_rows(300, 400, 2, True)
    kw = dict(factorSize=3, maxIter=5, solver=solver, stepSize=0.1, seed=1)
    want, _ = fm.fit_step(fm.FMNumpyStep(X, y, 3, "logistic"), 400, **kw)
    step = fm.FMDeviceStep(csr(X, cuda), dev(y, cuda), 3, "logistic")
    got, history = fm.fit_step(step, 400, **kw)
    deviation = float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
    print(f"fm csr fit deviation {solver}: {deviation:.3e}")
    assert len(history) == 5 and deviation <= BOUND[solver]


BOUND = {"gd": 1e-13, "adamW": 1e-11}


def test_header_symbols():
    syms = {s for s in N.header_symbols() if s.startswith("cyc_fmcsr_")}
    assert syms == {"cyc_fmcsr_segment_entries", "cyc_fmcsr_rows_create",
                    "cyc_fmcsr_rows_destroy", "cyc_fmcsr_evaluate_dev", "cyc_fmcsr_predict_dev"}
    assert all(hasattr(N.load(), s) and s in N.SIGNATURES for s in syms)
