"""FM on the device (csrc/fm.hip) against the restatement: exact inputs by
bytes at the kernels' edges, real inputs within the sums' bars, predict, the
label refusal, one whole fit per solver and the header's symbols.  Every device
call runs twice and must give the same bytes."""
import functools

import numpy as np
import pytest
import torch

import fm_restatement as R
from cycloneml_amd import _native as N
from cycloneml_amd import fm

pytestmark = pytest.mark.gpu
LIMIT = 1024            # cyc_fm_fused_features(8), asserted below
TILE, RUN = 16, 1024    # cyc_fm_tile_rows, cyc_fm_run_rows


def dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(cuda)


def evaluate_twice(plan, X, y, coef, cuda, **kw):
    Xd, yd, cd = dev(X, cuda), dev(y, cuda), dev(coef, cuda)
    a = plan.evaluate(Xd, yd, cd, **kw).cpu().numpy()
    b = plan.evaluate(Xd, yd, cd, **kw).cpu().numpy()
    assert a.tobytes() == b.tobytes()
    return a


@functools.lru_cache(maxsize=None)
def exact(n, d, k, fitIntercept=True, fitLinear=True):
    return R.exact_rows(n, d, k, 11, fitIntercept, fitLinear)


EDGES = [(33, d, 8) for d in (1, 15, 16, 17, 65, LIMIT - 1, LIMIT, LIMIT + 1)] \
    + [(33, 20, k) for k in (1, 15, 16, 17, 64)] + [(33, 193, 64), (33, 513, 17)] \
    + [(n, 17, 8) for n in (1, 15, 17, TILE + 1, RUN + 1, 2 * RUN + 3)] \
    + [(2 * RUN + 3, LIMIT + 1, 8)]


@pytest.mark.parametrize("n, d, k", EDGES)
def test_exact_inputs_by_bytes(cuda, n, d, k):
    X, y, coef, (G, L, cnt) = exact(n, d, k)
    plan = fm.FMPlan(d, k)
    assert (plan.tileRows, plan.runRows) == (TILE, RUN)
    assert fm.FMPlan(3, 8).fusedFeatures == LIMIT
    got = evaluate_twice(plan, X, y, coef, cuda)
    assert got.tobytes() == np.concatenate([G, [L, cnt]]).tobytes()


@pytest.mark.parametrize("fitIntercept, fitLinear", [(False, True), (True, False)])
@pytest.mark.parametrize("d", [17, LIMIT + 1])
def test_flag_off_layouts(cuda, d, fitIntercept, fitLinear):
    X, y, coef, (G, L, cnt) = exact(33, d, 8, fitIntercept, fitLinear)
    got = evaluate_twice(fm.FMPlan(d, 8, fitIntercept, fitLinear), X, y, coef, cuda)
    assert got.tobytes() == np.concatenate([G, [L, cnt]]).tobytes()


@pytest.mark.parametrize("n, d", [(2 * RUN + 3, 17), (40, LIMIT + 1)])
def test_fraction_takes_the_host_rules_rows(cuda, n, d):
    X, y, coef, _ = exact(n, d, 8)
    G, L, cnt = R.evaluate(X, y, coef, 8, "squared", i=3, fraction=0.5, rowOffset=7)
    assert 0 < cnt < n
    got = evaluate_twice(fm.FMPlan(d, 8), X, y, coef, cuda, iter=3, fraction=0.5, rowOffset=7)
    assert got.tobytes() == np.concatenate([G, [L, cnt]]).tobytes()


@pytest.mark.parametrize("d", [17, LIMIT + 1])
def test_small_workspace_same_bytes(cuda, d):
    X, y, coef, (G, L, cnt) = exact(2 * RUN + 3, d, 8)
    small = fm.FMPlan(d, 8, workspaceBytes=2 * 8 * (d * 10 + 3))      # two partials
    got = evaluate_twice(small, X, y, coef, cuda)
    assert got.tobytes() == np.concatenate([G, [L, cnt]]).tobytes()


@pytest.mark.parametrize("loss", ["squared", "logistic"])
@pytest.mark.parametrize("d", [17, LIMIT + 1])
def test_real_inputs_within_the_sums_bars(cuda, loss, d):
    X, y = R.real_rows(50, d, 5, loss == "logistic")
    coef = np.random.default_rng(6).normal(size=d * 3 + d + 1) * 0.1
    G, L, cnt, _, _, GAbs, LAbs = R.evaluate(X, y, coef, 3, loss, bars=True)
    got = evaluate_twice(fm.FMPlan(d, 3, loss=loss), X, y, coef, cuda)
    assert np.all(np.abs(got[:-2] - G) <= 1e-10 * GAbs)
    assert abs(got[-2] - L) <= 1e-10 * LAbs and got[-1] == cnt


@pytest.mark.parametrize("d", [1, 15, 16, 17, 65, LIMIT - 1, LIMIT, LIMIT + 1])
def test_predict_of_both_models(cuda, d):
    X, _ = R.real_rows(37, d, 8)
    rng = np.random.default_rng(9)
    b, w, V = rng.normal(), rng.normal(size=d) * 0.1, rng.normal(size=(d, 8)) * 0.1
    coef = np.concatenate([V.ravel(), w, [b]])
    _, _, _, raw, bar = R.evaluate(X, np.zeros(37), coef, 8, "squared", bars=True)[:5]
    Xd = dev(X, cuda)
    reg, cls = fm.FMRegressionModel(b, w, V), fm.FMClassificationModel(b, w, V)
    got = reg.predict(Xd).cpu().numpy()
    assert reg.predict(Xd).cpu().numpy().tobytes() == got.tobytes()
    assert np.all(np.abs(got - raw) <= 1e-10 * bar)
    r2, p2, lab = (t.cpu().numpy() for t in (cls.predictRaw(Xd), cls.predictProbability(Xd),
                                             cls.predict(Xd)))
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
        plan.evaluate(dev(X, cuda), dev(y, cuda), dev(np.zeros(9 * 3 + 1), cuda), rowOffset=100)


@pytest.mark.parametrize("solver", ["gd", "adamW"])
def test_whole_fit_on_the_device_step(cuda, solver):
    """max|dcoef| / max|coef| against the FMNumpyStep fit.  Measured on an
    MI355X: 1.196e-16 (gd), 1.518e-15 (adamW); asserted at 100 x that, rounded
    up to a power of ten (never looser than 1e-8)."""
    X, y = R.real_rows(300, 17, 2, True)
    kw = dict(factorSize=3, maxIter=5, solver=solver, stepSize=0.1, seed=1)
    want, _ = fm.fit_step(fm.FMNumpyStep(X, y, 3, "logistic"), 17, **kw)
    got, history = fm.fit_step(fm.FMDeviceStep(dev(X, cuda), dev(y, cuda), 3, "logistic"), 17, **kw)
    deviation = float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
    print(f"fm fit deviation {solver}: {deviation:.3e}")
    assert len(history) == 5 and deviation <= BOUND[solver]


BOUND = {"gd": 1e-13, "adamW": 1e-12}


def test_header_symbols():
    syms = {s for s in N.header_symbols() if s.startswith("cyc_fm_")}
    assert syms == {"cyc_fm_run_rows", "cyc_fm_tile_rows", "cyc_fm_max_factors",
                    "cyc_fm_max_features", "cyc_fm_fused_features", "cyc_fm_plan_create",
                    "cyc_fm_plan_destroy", "cyc_fm_evaluate_dev", "cyc_fm_predict_dev"}
    assert all(hasattr(N.load(), s) for s in syms)
