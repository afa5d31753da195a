"""NaiveBayes' dense aggregate on the device (csrc/naive_bayes.hip) against
the numpy restatement of tests/naive_bayes_restatement.py.

  exact inputs (integers below 2^20, weights in eighths): every sum is exact
              in any order, so the device buffer equals the restatement's by
              bytes; a dropped, doubled or misfiled row cannot hide
  real inputs entry (c, j) within 1e-10 sum |w_i x_ij| (|w_i| x_ij^2 for Q);
              rounding is below n 2^-53 of that sum
Every device call runs twice and the two results are compared by tobytes().
Scoring, the CSR aggregate and their tests are not part of the package yet.
"""
import numpy as np
import pytest
import torch

import naive_bayes_restatement as R
from cycloneml_amd import _native as N
from cycloneml_amd import naive_bayes as nb
from cycloneml_amd.classification import NaiveBayes, NaiveBayesModel

pytestmark = pytest.mark.gpu

SHAPES = R.shape_cases()


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def host(t):
    return None if t is None else t.cpu().numpy()


def twice(fn):
    a, b = fn(), fn()
    a = a if isinstance(a, tuple) else (a,)
    b = b if isinstance(b, tuple) else (b,)
    for x, y in zip(a, b):
        assert (x is None) == (y is None)
        if x is not None:
            assert x.tobytes() == y.tobytes(), "two calls differ"
    return a if len(a) > 1 else a[0]


def device_sums(plan, X, y, w):
    def run():
        sums = torch.zeros(plan.sumsLength, dtype=torch.float64, device="cuda:0")
        plan.accumulate(X, y, w, sums)
        return host(sums)
    return twice(run)


def ref_sums(X, y, w, C, t):
    W, S, Q, aS, aQ = R.aggregate(X, y, w, C, t)
    bar = np.concatenate([np.abs(W), aS.ravel()] + ([aQ.ravel()] if aQ is not None else []))
    return R.sums_buffer(W, S, Q), 1e-10 * bar


def test_plan_constants(cuda):
    for t in R.TYPES:
        for d in (1, 14, 15, 16, 31, 63, 64, 127, 254, 255, 256, 5000):
            p = nb.NBPlan(3, d, t)
            want = next((T for T in R.COL_TILES if T >= d + 1), R.COL_TILES[-1])
            assert (p.colTile, p.rowsPerRun, p.classesPerPass) == \
                (want, R.ROWS_PER_RUN, R.CLASSES_PER_PASS[t])
            p.close()


@pytest.mark.parametrize("t", R.TYPES)
@pytest.mark.parametrize("d,C,n", SHAPES)
def test_exact_aggregate_dense(cuda, t, d, C, n):
    X, y, w = R.exact_rows(t, d, C, n)
    plan = nb.NBPlan(C, d, t)
    got = device_sums(plan, dev(X), dev(y), dev(w))
    ref, _ = ref_sums(X, y, w, C, t)
    assert got.tobytes() == ref.tobytes()
    if n == 257 and d in (3, 65):      # unit weights: w = None
        got = device_sums(plan, dev(X), dev(y), None)
        assert got.tobytes() == ref_sums(X, y, None, C, t)[0].tobytes()
    plan.close()


@pytest.mark.parametrize("t", R.TYPES)
def test_small_workspace_aggregate(cuda, t):
    """3000 rows = 3 runs folded in 3 launches: the same bytes as in one."""
    d, C, n, wsb = R.SMALL_WS_AGG
    X, y, w = R.exact_rows(t, d, C, n)
    ref, _ = ref_sums(X, y, w, C, t)
    Xr, yr, wr = R.real_rows(t, d, C, n)
    real = []
    for b in (wsb, 0):
        plan = nb.NBPlan(C, d, t, b)
        assert device_sums(plan, dev(X), dev(y), dev(w)).tobytes() == ref.tobytes()
        real.append(device_sums(plan, dev(Xr), dev(yr), dev(wr)))
        plan.close()
    assert real[0].tobytes() == real[1].tobytes()     # never other sums for the same split


@pytest.mark.parametrize("t", R.TYPES)
@pytest.mark.parametrize("d,C,n", [(d, C, 257) for d in R.DS for C in (3, 17)] +
                         [(17, 3, n) for n in (1, 64, 1000)] + [(3, 2, 2049)])
def test_real_aggregate_dense(cuda, t, d, C, n):
    X, y, w = R.real_rows(t, d, C, n)
    plan = nb.NBPlan(C, d, t)
    got = device_sums(plan, dev(X), dev(y), dev(w))
    plan.close()
    ref, bar = ref_sums(X, y, w, C, t)
    worst = np.max(np.abs(got - ref) - bar)
    print(f"aggregate {t} d={d} C={C} n={n}: max |err| - bar = {worst:.3e}")
    assert np.all(np.abs(got - ref) <= bar)


def refused(fn, match, plan=None, row=None, rule=None):
    with pytest.raises(N.IllegalArgumentException, match=match):
        fn()
    if plan is not None:
        assert (plan.badRow, plan.badRule) == (row, rule)


def test_device_refusals_in_fit(cuda):
    d, C, n = 17, 3, 1500
    X, y, w = (a.copy() for a in R.exact_rows("bernoulli", d, C, n))

    def run(t, X, y, w):
        plan = nb.NBPlan(C, d, t)
        sums = torch.zeros(plan.sumsLength, dtype=torch.float64, device="cuda:0")
        return plan, (lambda: plan.accumulate(dev(X), dev(y), dev(w), sums))

    # a negative value: rows 1100 and 40, the lowest is named
    Xb = X.copy()
    Xb[1100, 3] = -2.5
    Xb[40, 16] = -0.5
    for t in ("multinomial", "complement"):
        plan, fn = run(t, Xb, y, w)
        refused(fn, r"requires nonnegative feature values but found -0\.5\. \(row 40\)", plan, 40,
                nb.RULE_VALUE)
    # 0.5 under bernoulli
    Xb = X.copy()
    Xb[1030, 0] = 0.5
    Xb[1400, 2] = 2.0
    plan, fn = run("bernoulli", Xb, y, w)
    refused(fn, r"requires 0 or 1 feature values but found 0\.5\. \(row 1030\)", plan, 1030,
            nb.RULE_VALUE)
    # labels: 2.5, -1, C -- each the lowest bad row, beside a later one
    for bad, text in ((2.5, r"Found 2\.5\."), (-1.0, r"Found -1\.0\."), (float(C), r"Found 3\.0\."),
                      (1e300, r"Found 1\.0E300\."), (float("nan"), r"Found NaN\.")):
        yb = y.copy()
        yb[77] = bad
        yb[1200] = 1e9
        plan, fn = run("multinomial", X, yb, w)
        refused(fn, text + r" \(row 77\)", plan, 77, nb.RULE_LABEL)
    # a NaN weight, a negative weight
    for bad in (float("nan"), -0.125):
        wb = w.copy()
        wb[1025] = bad
        plan, fn = run("multinomial", X, y, wb)
        refused(fn, r"illegal weight value: .* \(row 1025\)", plan, 1025, nb.RULE_WEIGHT)
    # a class without weight (through the estimator: the M step refuses)
    wb = w.copy()
    wb[y == 1.0] = 0.0
    refused(lambda: NaiveBayes().fit(dev(X), dev(y), dev(wb)), "class 1 has no weight")
    refused(lambda: NaiveBayes().fit(dev(X), dev(y), dev(w), numClasses=4),
            "class 3 has no weight")
    refused(lambda: NaiveBayes().fit(dev(X), dev(y), dev(w), numClasses=2), r"Found 2\.0\.")


@pytest.mark.parametrize("t", R.TYPES)
def test_whole_fit(cuda, tmp_path, t):
    """The fitted model within the M step's propagated bars of the
    restatement's fit (sums within 1e-10 of their absolute sums move a log by
    the relative change of its argument), and the same bytes after save and
    load."""
    d, C, n = 17, 3, 1000
    X, y, w = R.real_rows(t, d, C, n)
    m = NaiveBayes(modelType=t).fit(dev(X), dev(y), dev(w))
    pi, theta, sigma = R.model_of(t, d, C, n)
    assert (m.numClasses, m.numFeatures, m.modelType) == (C, d, t)
    W, S, Q, aS, aQ = R.aggregate(X, y, w, C, t)
    if t == "gaussian":
        tb = 2e-10 * aS / W[:, None]
        sb = 1e-9 * np.abs(sigma).max() + 2e-10 * aQ / W[:, None] + 4 * np.abs(theta) * tb
        assert np.all(np.abs(m.theta - theta) <= tb) and np.all(np.abs(m.sigma - sigma) <= sb)
    else:
        assert np.all(np.abs(m.theta - theta) <= 4e-10)
        assert m.sigma.shape == (0, 0)
    assert np.all(np.abs(m.pi - pi) <= 4e-10)
    path = str(tmp_path / "nb")
    m.save(path)
    back = NaiveBayesModel.load(path)
    for a, b in ((m.pi, back.pi), (m.theta, back.theta), (m.sigma, back.sigma)):
        assert a.tobytes() == b.tobytes()


def test_header_symbols():
    names = ["cyc_nb_plan_create", "cyc_nb_plan_destroy", "cyc_nb_col_tile",
             "cyc_nb_rows_per_run", "cyc_nb_classes_per_pass", "cyc_nb_aggregate_dev"]
    syms = set(N.header_symbols())
    lib = N.load()
    for name in names:
        assert name in syms and name in N.SIGNATURES and hasattr(lib, name)
    assert sorted(s for s in syms if s.startswith("cyc_nb_")) == sorted(names)
