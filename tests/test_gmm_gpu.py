"""GaussianMixture on the device (csrc/gmm.hip) against the numpy restatement
of tests/gmm_restatement.py, which walks the rows in order.

With delta = x_i - mu_j, B_ij = sum_c (sum_f |A_j[c, f]| |delta_f|)^2 is the sum
of absolute products behind q_ij; both sides round below about d 2^-53 of it.
Bars (derived, not measured), prob_ij = p_ij / s_i:
  logpdf      |got - ref| <= 1e-10 (|u_j| + B_ij)
  prob        |got - ref| <= 1e-10 prob_ij (2 + B_ij + sum_l prob_il B_il), from
              dr_j = r_j (dlog p_j - sum_l r_l dlog p_l); the 2 covers exp and
              the divide
  ll          |got - ref| <= 1e-10 sum_i om_i (1 + sum_j prob_ij B_ij)
  mstep       entry (a, b) of S_j: 1e-10 sum_i r_ij |x_ia| |x_ib| (|x_ia| for M,
              1 for W), the device fed the restatement's own R
  accumulate  the mstep bar plus sum_i (om_i times the prob bar) |x_ia x_ib|
Every call runs twice and the two results are compared by tobytes().
"""
import functools

import numpy as np
import pytest

import gmm_restatement as R
from cycloneml_amd import _native as N
from cycloneml_amd import gmm
from cycloneml_amd.clustering import GaussianMixture

pytestmark = pytest.mark.gpu

DS = [1, 3, 15, 16, 17, 64, 65, 130]
KS = [1, 2, 5, 16, 17]
ROWS = [1, 63, 64, 65, 255, 256, 257, 1000]
# every (d, k) at 257 rows, every row count at (17, 5), and 1000 rows in chunks
# of 256 (a chunk edge inside the data, a 232-row tail)
CASES = [(d, k, 257, 0) for d in DS for k in KS] + \
        [(17, 5, n, 0) for n in ROWS if n != 257] + [(17, 5, 1000, 256)]


def sigma(d):
    """The blobs' standard deviation.  Standard-normal blobs stop at d = 17:
    at d >= 64 even the matching component's density is below EPSILON (0.5 d
    log 2 pi alone is 59 at d = 64, log EPSILON is -36), so every p_ij would be
    EPSILON, every responsibility 1 / k and every label a tie -- on the
    restatement's side already.  At 0.2 the densities stay above EPSILON."""
    return 1.0 if d <= 17 else 0.2


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def blobs(d, rows, k=5, offset=0.0, seed=0):
    """3 to 5 separated blobs (standard normal up to d = 17, see sigma); weights uniform in (0, 2) with
    exact zeros (row 0 keeps a positive weight).  A model of k components sits
    on the first k blobs (model_of), so the rows come from those: a row of a
    blob no component covers has every pdf underflow, all its p_ij are EPSILON
    and its label is a k-way tie."""
    rng = np.random.default_rng(7919 * d + rows + seed)
    nb = 3 + (d + rows) % 3
    centers = rng.normal(size=(nb, d)) * 2.0 + 8.0 * np.arange(nb)[:, None] + offset
    which = rng.integers(0, min(nb, k), rows)
    X = centers[which] + sigma(d) * rng.standard_normal((rows, d))
    om = rng.uniform(0.0, 2.0, rows)
    om[rng.random(rows) < 0.1] = 0.0
    om[0] = 1.25
    return frozen(X, om, centers)


@functools.lru_cache(maxsize=None)
def model_of(d, k, rows, offset=0.0):
    """k components near the blobs: random weights, SPD covariances."""
    _, _, centers = blobs(d, rows, k, offset)
    rng = np.random.default_rng(104729 * d + k)
    w = rng.uniform(0.5, 1.5, k)
    w /= w.sum()
    means = centers[np.arange(k) % len(centers)] + 0.3 * sigma(d) * rng.standard_normal((k, d))
    G = rng.standard_normal((k, d, d))
    covs = (np.eye(d)[None] * rng.uniform(0.5, 2.0, (k, 1, 1)) +
            0.1 * np.einsum("kab,kcb->kac", G, G) / d) * sigma(d) ** 2
    return frozen(w, means, covs)


@functools.lru_cache(maxsize=None)
def reference(d, k, rows, offset=0.0):
    X, om, _ = blobs(d, rows, k, offset)
    w, means, covs = model_of(d, k, rows, offset)
    return reference_of(X, om, w, means, covs)


def reference_of(X, om, w, means, covs):
    sums, e, bounds = R.em_step(X, om, w, means, covs)
    return dict(sums=sums, e=e, bounds=bounds, bar_acc=R.sums_bars(X, e, bounds),
                bar_m=R.sums_bars(X, e, bounds, with_estep=False))


def gaussians_of(means, covs):
    return [gmm.MultivariateGaussian(means[j], covs[j]) for j in range(len(means))]


def twice(fn):
    """fn() run twice: the same bits; returns the first result (host)."""
    a, b = fn(), fn()
    assert a.tobytes() == b.tobytes()
    return a


def check_within(got, ref, bar, what):
    err = np.abs(got - ref)
    bad = ~(err <= bar)
    assert not bad.any(), (what, int(bad.sum()), float(err[bad].max()), float(bar[bad].min()))


def accumulate(plan, Xd, omd):
    import torch
    sums = torch.zeros(plan.sumsLength, dtype=torch.float64, device=Xd.device)
    plan.accumulate(Xd, omd, sums)
    return sums.cpu().numpy()


def check_plan(cuda, X, om, w, means, covs, ref, chunkRows=0, max_undecided=0.01):
    """logpdf, prob, label, accumulate and mstep of one model over one shard."""
    import torch
    n, d = X.shape
    k = len(w)
    e = ref["e"]
    Xd = torch.from_numpy(np.array(X)).to(cuda)
    omd = None if om is None else torch.from_numpy(np.array(om)).to(cuda)
    plan = gmm.GMMPlan(k, d, chunkRows)
    try:
        plan.set_model(w, gaussians_of(means, covs), cuda)
        us = np.array([R.consts(means[j], covs[j])[1] for j in range(k)])
        lp = twice(lambda: plan.logpdf(Xd).cpu().numpy())
        check_within(lp, e["logpdf"], 1e-10 * (np.abs(us)[None, :] + e["B"]), "logpdf")
        prob = twice(lambda: plan.predict(Xd, prob=True)[0].cpu().numpy())
        rbar = R.r_bar(e)
        check_within(prob, e["prob"], rbar, "prob")
        lab = twice(lambda: plan.predict(Xd, label=True)[1].cpu().numpy())
        assert lab.dtype == np.int32
        both = plan.predict(Xd, prob=True, label=True, logpdf=True)
        assert both[0].cpu().numpy().tobytes() == prob.tobytes()
        assert both[1].cpu().numpy().tobytes() == lab.tobytes()
        assert both[2].cpu().numpy().tobytes() == lp.tobytes()
        want = np.argmax(e["prob"], axis=1)
        if k > 1:
            order = np.argsort(-e["prob"], axis=1, kind="stable")[:, :2]
            top = np.take_along_axis(e["prob"], order, axis=1)
            tb = np.take_along_axis(rbar, order, axis=1)
            decided = top[:, 0] - top[:, 1] > 2.0 * tb.max(axis=1)
        else:
            decided = np.ones(n, dtype=bool)
        assert np.array_equal(lab[decided], want[decided])
        assert (~decided).sum() <= max_undecided * n
        acc = twice(lambda: accumulate(plan, Xd, omd))
        check_within(acc, ref["sums"], ref["bar_acc"], "accumulate")
        Rd = torch.from_numpy(e["R"]).to(cuda)

        def run_mstep():
            sums = torch.zeros(plan.sumsLength, dtype=torch.float64, device=cuda)
            plan.mstep(Xd, Rd, sums)
            return sums.cpu().numpy()
        ms = twice(run_mstep)
        assert ms[0] == 0.0
        check_within(ms[1:], ref["sums"][1:], ref["bar_m"][1:], "mstep")
        return dict(logpdf=lp, prob=prob, label=lab, sums=acc)
    finally:
        plan.close()


@pytest.mark.parametrize("d,k,rows,chunkRows", CASES)
def test_em_step_matches_restatement(cuda, d, k, rows, chunkRows):
    X, om, _ = blobs(d, rows, k)
    w, means, covs = model_of(d, k, rows)
    check_plan(cuda, X, om, w, means, covs, reference(d, k, rows), chunkRows)


def test_centre_before_multiply(cuda):
    """Unit-variance blobs 1e6 from the origin: A x - A mu would miss the bars
    by about six orders; x - mu first is exact to the inputs' last bit."""
    d, k, rows, off = 17, 3, 257, 1e6
    X, om, _ = blobs(d, rows, k, off)
    w, means, covs = model_of(d, k, rows, off)
    ref = reference(d, k, rows, off)
    assert ref["e"]["B"].min() < 1e3
    check_plan(cuda, X, om, w, means, covs, ref)


def test_singular_covariance(cuda):
    """A duplicated column: the M step's covariances are singular, rootSigmaInv
    has a zero row, and the bars hold."""
    d, k, rows = 5, 2, 257
    X0, om, centers = blobs(d, rows, k, seed=1)
    X = np.array(X0)
    X[:, 4] = X[:, 0]
    means0 = np.array(centers[:k])
    means0[:, 4] = means0[:, 0]
    sums, _, _ = R.em_step(X, om, [0.5, 0.5], means0, np.stack([np.eye(d) * 4.0] * k))
    w, means, covs = R.mstep(sums, k, d)
    for j in range(k):
        A, _ = R.consts(means[j], covs[j])
        assert (np.abs(A).sum(axis=1) == 0.0).sum() >= 1
    check_plan(cuda, X, om, w, means, covs, reference_of(X, om, w, means, covs))


def test_underflow_leaves_epsilon(cuda):
    """A component 1e3 standard deviations away: its pdf underflows to 0, so
    p_ij is EPSILON exactly and r_ij = EPSILON / s_i on both sides."""
    d, k, rows = 3, 3, 257
    X, om, centers = blobs(d, rows, 2, seed=2)      # rows of blobs 0 and 1
    w = np.array([0.3, 0.3, 0.4])
    means = np.array(centers[:3])
    means[2] = centers[0] + 1e3
    covs = np.stack([np.eye(d)] * 3)
    ref = reference_of(X, None, w, means, covs)
    e = ref["e"]
    assert (e["p"][:, 2] == R.EPSILON).all()
    assert np.array_equal(e["prob"][:, 2], R.EPSILON / e["s"])
    out = check_plan(cuda, X, None, w, means, covs, ref)
    assert (out["logpdf"][:, 2] < -745.0).all()          # exp gives exactly 0
    # s_i carries the near components' bars and nothing else
    near = (e["prob"][:, :2] * e["B"][:, :2]).sum(axis=1)
    got = out["prob"][:, 2] * e["s"] / R.EPSILON
    assert (np.abs(got - 1.0) <= 1e-10 * (2.0 + near)).all()
    assert (out["prob"][:, 2] > 0.0).all()


def test_shard_merge(cuda):
    """[0, 300) and then [300, 1000) into one buffer: the restatement over all
    1000 rows, within the accumulate bars."""
    import torch
    d, k, rows = 17, 5, 1000
    X, om, _ = blobs(d, rows, k)
    w, means, covs = model_of(d, k, rows)
    ref = reference(d, k, rows)
    Xd = torch.from_numpy(np.array(X)).to(cuda)
    omd = torch.from_numpy(np.array(om)).to(cuda)
    plan = gmm.GMMPlan(k, d)
    try:
        plan.set_model(w, gaussians_of(means, covs), cuda)

        def run():
            sums = torch.zeros(plan.sumsLength, dtype=torch.float64, device=cuda)
            plan.accumulate(Xd[:300], omd[:300], sums)
            plan.accumulate(Xd[300:], omd[300:], sums)
            return sums.cpu().numpy()
        check_within(twice(run), ref["sums"], ref["bar_acc"], "merge")
    finally:
        plan.close()


def test_row_weights(cuda):
    """Weight-0 rows holding NaN change no bit; a negative and a NaN weight
    raise the reference's require."""
    import torch
    d, k, rows = 17, 5, 257
    X, om, _ = blobs(d, rows, k)
    w, means, covs = model_of(d, k, rows)
    assert (om == 0.0).sum() >= 5
    Xn = np.array(X)
    Xn[om == 0.0] = np.nan
    plan = gmm.GMMPlan(k, d)
    try:
        plan.set_model(w, gaussians_of(means, covs), cuda)
        omd = torch.from_numpy(np.array(om)).to(cuda)
        clean = accumulate(plan, torch.from_numpy(np.array(X)).to(cuda), omd)
        dirty = accumulate(plan, torch.from_numpy(Xn).to(cuda), omd)
        assert np.isfinite(dirty).all()
        assert clean.tobytes() == dirty.tobytes()
        for bad in (-0.5, np.nan):
            ob = np.array(om)
            ob[100] = bad
            with pytest.raises(N.IllegalArgumentException, match="requirement failed"):
                accumulate(plan, torch.from_numpy(np.array(X)).to(cuda),
                           torch.from_numpy(ob).to(cuda))
    finally:
        plan.close()


def test_univariate_known_answer(cuda):
    """GaussianMixtureSuite's univariate fit through the device."""
    import torch
    from test_gmm_host import UNI, UNI_INIT
    model = GaussianMixture(k=2, initialModel=UNI_INIT).fit(torch.from_numpy(UNI).to(cuda))
    assert model.summary.numIter == 3
    np.testing.assert_allclose(model.weights, [1 / 3, 2 / 3], atol=1e-3)
    np.testing.assert_allclose([g.mean[0] for g in model.gaussians], [-4.3673, 5.1604], atol=1e-3)
    np.testing.assert_allclose([g.cov[0, 0] for g in model.gaussians], [1.1098, 0.86644],
                               atol=1e-3)
    assert abs(model.summary.logLikelihood - -30.3754783) <= 1e-6
    assert model.summary.clusterSizes.tolist() == [5, 10]
    assert model.predict(torch.from_numpy(UNI).to(cuda)).cpu().tolist() == [0] * 5 + [1] * 10


def test_random_initial_model_fits(cuda):
    """Without initialModel: the seed fixes the draws and so the fit."""
    import torch
    X, _, _ = blobs(4, 600, 3, seed=3)
    Xd = torch.from_numpy(np.array(X)).to(cuda)
    a = GaussianMixture(k=3, maxIter=3, seed=11).fit(Xd)
    b = GaussianMixture(k=3, maxIter=3, seed=11).fit(Xd)
    assert a.weights.tobytes() == b.weights.tobytes()
    assert a.summary.objectiveHistory.tobytes() == b.summary.objectiveHistory.tobytes()
    assert a.summary.clusterSizes.sum() == 600 and a.summary.numIter == 3
    assert np.isfinite(a.summary.objectiveHistory).all()


def test_whole_fit(cuda, capsys):
    """Three blobs in d = 4, 600 rows, initialModel given, maxIter = 5, tol = 0.
    Step parity: each iteration's model (the restatement's) goes to both
    sides and the buffers meet the accumulate bars.  Then the free-running
    device fit against the free-running restatement: the yardstick is the
    restatement's own sensitivity to summation order (rows forward against
    rows reversed: the largest absolute difference in the final weights,
    means and covariances, and in ll); the device, whose sums are MFMA-tiled
    and split-K -- a third summation order and nothing more -- gets 16 x that,
    with a floor of 1e-12 of the largest parameter (of |ll|).  Both numbers
    are printed.  One MI355X run: yardstick 9.6e-14 on the parameters and
    4.1e-12 on ll (-4001.4); the device differed by 8.3e-14 (tolerance 5.8e-12)
    and 5.0e-12 (tolerance 4.0e-9).
    """
    import torch
    d, k, rows, iters = 4, 3, 600, 5
    # blobs 2.5 apart overlap, so EM still moves ll by whole units at iteration
    # 5.  (Blobs 8 apart reach the fixed point in 3 iterations; from there
    # |ll - llPrev| > 0 is decided by the last bit and numIter at tol = 0 by the
    # summation order.)
    rng = np.random.default_rng(4)
    centers = 2.5 * np.arange(k)[:, None] + 0.5 * rng.normal(size=(k, d))
    X = centers[rng.integers(0, k, rows)] + rng.standard_normal((rows, d))
    init = (np.full(k, 1.0 / k), centers + 0.5, np.stack([np.eye(d) * 2.0] * k))
    Xd = torch.from_numpy(X).to(cuda)
    # step parity
    w, means, covs = init
    plan = gmm.GMMPlan(k, d)
    try:
        for _ in range(iters):
            ref = reference_of(X, None, w, means, covs)
            plan.set_model(w, gaussians_of(means, covs), cuda)
            got = twice(lambda: accumulate(plan, Xd, None))
            check_within(got, ref["sums"], ref["bar_acc"], "step")
            w, means, covs = R.mstep(ref["sums"], k, d)
    finally:
        plan.close()
    # free-running
    fwd = R.fit(X, None, init, maxIter=iters, tol=0.0)
    rev = R.fit(X[::-1], None, init, maxIter=iters, tol=0.0)
    yard_p = max(np.abs(fwd[i] - rev[i]).max() for i in range(3))
    yard_ll = abs(fwd[3] - rev[3])
    model = GaussianMixture(k=k, maxIter=iters, tol=0.0, initialModel=init).fit(Xd)
    gm = np.stack([g.mean for g in model.gaussians])
    gc = np.stack([g.cov for g in model.gaussians])
    err_p = max(np.abs(model.weights - fwd[0]).max(), np.abs(gm - fwd[1]).max(),
                np.abs(gc - fwd[2]).max())
    err_ll = abs(model.summary.logLikelihood - fwd[3])
    scale = max(np.abs(fwd[i]).max() for i in range(3))
    tol_p = max(16.0 * yard_p, 1e-12 * scale)
    tol_ll = max(16.0 * yard_ll, 1e-12 * abs(fwd[3]))
    with capsys.disabled():
        print(f"\nwhole fit: yardstick params {yard_p:.3e} ll {yard_ll:.3e}; "
              f"device params {err_p:.3e} (tol {tol_p:.3e}) ll {err_ll:.3e} (tol {tol_ll:.3e})")
    assert fwd[4] == rev[4] == iters and min(np.diff(fwd[5])) > 1.0
    assert model.summary.numIter == fwd[4]
    assert len(model.summary.objectiveHistory) == len(fwd[5])
    assert err_p <= tol_p
    assert err_ll <= tol_ll
