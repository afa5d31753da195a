"""NaiveBayesModel's device predictions (csrc/naive_bayes_score.hip) against
the numpy restatement of tests/naive_bayes_restatement.py.

  real inputs   |raw - r| <= rawBar and |prob - p| <= probBar per entry (the
                restatement's own error magnitudes, 1e-10 of the absolute sums
                behind each value), the prediction equal on every row whose two
                best raw values are further apart than their bars
  exact inputs  theta and pi in eighths, integer rows below 2^20 (gaussian:
                integer means, variances powers of two): every product and sum
                is exact in any order, so raw equals the restatement's by
                bytes, on the product path and on the plain path
Every device call runs twice and the two results are compared by tobytes().
The ambiguity cap of the extra shapes needs no device.
"""
import ctypes

import numpy as np
import pytest
import torch

import naive_bayes_restatement as R
from cycloneml_amd import _native as N
from cycloneml_amd import naive_bayes as nb
from cycloneml_amd.classification import NaiveBayes, NaiveBayesModel

gpu = pytest.mark.gpu

# both sides of the 16-column tile and of the 64-column panel with 1, 2 and 3
# remainder tiles, and C > 128
EXTRA = [(17, 48, 257), (17, 49, 257), (17, 64, 257), (17, 65, 257), (33, 80, 257),
         (17, 129, 300)]
SHAPES = R.shape_cases() + EXTRA


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


def model_for(t, pi, theta, sigma):
    return NaiveBayesModel(pi, theta, sigma if t == "gaussian" else None, t)


def predictions(model, X):
    """(raw, prob, pred) of the model's three methods, each called twice."""
    Xd = dev(X)
    return (twice(lambda: host(model.predictRaw(Xd))),
            twice(lambda: host(model.predictProbability(Xd))),
            twice(lambda: host(model.predict(Xd))))


def scorer_outputs(s, X, **which):
    Xd = dev(X)
    return twice(lambda: tuple(host(o) for o in s.score(Xd, **which)))


@gpu
@pytest.mark.parametrize("t", R.TYPES)
@pytest.mark.parametrize("d,C,n", SHAPES)
def test_real_inputs(cuda, t, d, C, n):
    X, _, _ = R.real_rows(t, d, C, n)
    model = model_for(t, *R.model_of(t, d, C, n))
    raw, prob, pred = predictions(model, X)
    r, B, rawBar, probBar, p, yhat, amb = R.scored(t, d, C, n)
    assert raw.shape == prob.shape == (n, C) and pred.shape == (n,) and pred.dtype == np.float64
    print(f"score {t} d={d} C={C} n={n}: max (|raw err| - bar) = "
          f"{np.max(np.abs(raw - r) - rawBar):.3e}, max (|prob err| - bar) = "
          f"{np.max(np.abs(prob - p) - probBar):.3e}, ambiguous = {int(amb.sum())}")
    assert np.all(np.abs(raw - r) <= rawBar)
    assert np.all(np.abs(prob - p) <= probBar)
    assert np.array_equal(pred[~amb], yhat[~amb].astype(np.float64))


@pytest.mark.parametrize("t", R.TYPES)
def test_extra_shapes_leave_few_rows_ambiguous(t):
    """The condition of test_generators_leave_few_rows_ambiguous for the
    shapes this file adds, on the restatement alone."""
    for (d, C, n) in EXTRA:
        amb = R.scored(t, d, C, n)[6]
        assert amb.sum() <= 0.01 * amb.size, (t, d, C, n, int(amb.sum()))


def exact_model(t, d, C):
    rng = np.random.default_rng(811 * d + C)
    pi = rng.integers(-40, 1, size=C) / 8.0
    if t == "gaussian":
        theta = rng.integers(-50, 51, size=(C, d)).astype(np.float64)
        sigma = 2.0 ** rng.integers(-2, 4, size=(C, d))
        return pi, theta, sigma
    return pi, rng.integers(-64, 1, size=(C, d)) / 8.0, np.zeros((0, 0))


@gpu
@pytest.mark.parametrize("t", ("multinomial", "gaussian"))
@pytest.mark.parametrize("d,C,n", [(17, 3, 257), (65, 17, 65)])
def test_exact_inputs(cuda, t, d, C, n):
    X = R.exact_rows(t, d, C, n)[0]
    pi, theta, sigma = exact_model(t, d, C)
    ref = R.raw(X, pi, theta, sigma, t)[0]
    got = predictions(model_for(t, pi, theta, sigma), X)[0]
    assert got.tobytes() == ref.tobytes()
    if t == "multinomial":
        both = []
        for scorer in ("product", "plain"):
            s = nb.NBScorer(pi, theta, None, t, scorer=scorer)
            assert s.path == scorer
            both.append(scorer_outputs(s, X, raw=True)[0])
            s.close()
            assert both[-1].tobytes() == ref.tobytes(), scorer
        assert both[0].tobytes() == both[1].tobytes()


@gpu
def test_smoothing_zero(cuda):
    """-inf in theta: a zero feature skips it, a nonzero one gives -inf; the
    product path is not taken."""
    inf = np.inf
    pi = np.array([-1.0, -1.5, -0.75])
    theta = np.array([[-1.0, -inf, -2.0, -0.5], [-0.5, -1.0, -1.5, -2.0],
                      [-inf, -1.0, -1.0, -1.0]])
    X = np.array([[0.0, 0.0, 2.0, 1.0], [1.0, 3.0, 0.0, 0.0]])
    want = np.array([[-1.0 + (2.0 * -2.0 + 1.0 * -0.5), -1.5 + (2.0 * -1.5 + 1.0 * -2.0),
                      -0.75 + (2.0 * -1.0 + 1.0 * -1.0)],
                     [-inf, -1.5 + (1.0 * -0.5 + 3.0 * -1.0), -inf]])
    assert np.array_equal(R.raw(X, pi, theta, None, "multinomial")[0], want)
    raw, prob, pred = predictions(NaiveBayesModel(pi, theta), X)
    assert np.array_equal(raw, want)
    assert pred.tolist() == [2.0, 1.0]
    assert prob[1].tolist() == [0.0, 1.0, 0.0]
    s = nb.NBScorer(pi, theta)
    assert s.path == "plain" and not s.finite
    s.close()
    with pytest.raises(N.IllegalArgumentException, match="product scorer"):
        nb.NBScorer(pi, theta, scorer="product")
    with pytest.raises(N.IllegalArgumentException, match="product scorer"):
        nb.NBScorer(pi[:1], np.zeros((1, 2)), np.ones((1, 2)), "gaussian", scorer="product")
    # the library's own refusal, past the wrapper's
    lib = N.load()
    h = ctypes.c_void_p()
    bd, Md = dev(pi), dev(theta)
    rc = lib.cyc_nbmodel_create(3, 4, 0, 0, N.ptr(bd), N.ptr(Md), None, None, 1,
                                N.stream_handle(), ctypes.byref(h))
    assert rc == N.CYC_ERR_INVALID_ARG and b"finite" in lib.cyc_last_error()


@gpu
@pytest.mark.parametrize("t", R.TYPES)
def test_argmax_rule(cuda, t):
    """Two bit-identical classes predict the lower index; one class predicts 0
    with probability 1."""
    d, C, n = 17, 3, 257
    X = R.real_rows(t, d, C, n)[0]
    pi, theta, sigma = R.model_of(t, d, C, n)
    twin = [0, 1, 1, 2]
    pi2, theta2 = pi[twin], theta[twin]
    sigma2 = sigma[twin] if t == "gaussian" else sigma
    assert R.duplicates(pi2, theta2, sigma2, t).tolist() == [False, False, True, False]
    r, B = R.raw(X, pi2, theta2, sigma2, t)
    rb, _ = R.bars(r, B, t)
    amb = R.ambiguous(r, rb, R.duplicates(pi2, theta2, sigma2, t))
    yhat = R.predict(r)
    assert (yhat == 1).sum() > 10 and not (yhat == 2).any()
    raw, prob, pred = predictions(model_for(t, pi2, theta2, sigma2), X)
    assert raw[:, 1].tobytes() == raw[:, 2].tobytes()
    assert not (pred == 2.0).any()
    assert np.array_equal(pred[~amb], yhat[~amb].astype(np.float64))
    raw, prob, pred = predictions(model_for(t, *R.model_of(t, d, 1, n)), R.real_rows(t, d, 1, n)[0])
    assert not pred.any() and np.array_equal(prob, np.ones((n, 1)))


@gpu
def test_argmax_keeps_a_nan_in_class_zero(cuda):
    X = np.array([[1.0, 2.0], [0.0, 1.0]])
    theta = np.array([[-1.0, -2.0], [-2.0, -1.0], [-0.5, -0.5]])
    nan = float("nan")
    for pi, want in (([nan, -1.0, -1.0], [0.0, 0.0]), ([-1.0, nan, -1.0], [2.0, 2.0]),
                     ([-1.0, -1.0, nan], [1.0, 1.0]), ([nan, nan, nan], [0.0, 0.0])):
        for scorer in ("product", "plain"):
            s = nb.NBScorer(np.array(pi), theta, scorer=scorer)
            raw, _, pred = scorer_outputs(s, X, raw=True, pred=True)
            s.close()
            assert np.array_equal(pred, R.predict(raw).astype(np.float64))
            assert pred.tolist() == want, (pi, scorer)


@gpu
def test_row_checks(cuda):
    d, C, n = 17, 3, 513
    X = R.real_rows("multinomial", d, C, n)[0].copy()
    X[300, 5] = -1.0
    X[400, 2] = -1.0
    for t in ("multinomial", "complement"):
        pi, theta, sigma = R.model_of(t, d, C, n)
        s = nb.NBScorer(pi, theta, None, t)
        with pytest.raises(N.IllegalArgumentException,
                           match=r"requires nonnegative feature values but found -1\.0\. "
                                 r"\(row 300\)"):
            s.score(dev(X), pred=True)
        assert s.badRow == 300
        s.score(dev(np.abs(X)), pred=True)
        assert s.badRow == -1
        s.close()
        with pytest.raises(N.IllegalArgumentException, match=r"found -1\.0\. \(row 300\)"):
            model_for(t, pi, theta, sigma).predictRaw(dev(X))
    Xn = np.abs(X)
    Xn[77, 0] = float("nan")
    with pytest.raises(N.IllegalArgumentException, match=r"found NaN\. \(row 77\)"):
        model_for("multinomial", *R.model_of("multinomial", d, C, n)).predict(dev(Xn))
    Xb = R.real_rows("bernoulli", d, C, n)[0].copy()
    Xb[512, 16] = 0.5
    s = nb.NBScorer(*R.model_of("bernoulli", d, C, n)[:2], None, "bernoulli")
    with pytest.raises(N.IllegalArgumentException,
                       match=r"requires 0 or 1 feature values but found 0\.5\. \(row 512\)"):
        s.score(dev(Xb), prob=True)
    assert s.badRow == 512
    s.close()
    # gaussian takes any value
    Xg = -np.abs(R.real_rows("gaussian", d, C, n)[0])
    pi, theta, sigma = R.model_of("gaussian", d, C, n)
    raw = predictions(model_for("gaussian", pi, theta, sigma), Xg)[0]
    r, B = R.raw(Xg, pi, theta, sigma, "gaussian")
    assert np.all(np.abs(raw - r) <= R.bars(r, B, "gaussian")[0])


@gpu
@pytest.mark.parametrize("t", R.TYPES)
def test_small_workspace(cuda, t):
    """Fewer than 1024 rows of raw per chunk: more launches, the same bytes."""
    d, C, n = 17, 3, 3000
    X = R.real_rows(t, d, C, n)[0]
    pi, theta, sigma = R.model_of(t, d, C, n)
    outs = []
    for wsb in (1000 * C * 8, 0):
        s = nb.NBScorer(pi, theta, sigma, t, workspaceBytes=wsb)
        assert (s.chunkRows < 1024) == (wsb != 0) and s.chunkRows >= 1
        outs.append(scorer_outputs(s, X, raw=True) + scorer_outputs(s, X, prob=True)
                    + scorer_outputs(s, X, pred=True)
                    + scorer_outputs(s, X, raw=True, prob=True, pred=True))
        s.close()
    for a, b in zip(*outs):
        assert (a is None) == (b is None)
        if a is not None:
            assert a.tobytes() == b.tobytes()
    # asked for alone or together: the same bytes
    raw, prob, pred = outs[0][9:12]
    assert raw.tobytes() == outs[0][0].tobytes() and prob.tobytes() == outs[0][4].tobytes() \
        and pred.tobytes() == outs[0][8].tobytes()


@gpu
def test_empty_rows(cuda):
    m = model_for("multinomial", *R.model_of("multinomial", 17, 3, 257))
    X = torch.zeros((0, 17), dtype=torch.float64, device="cuda:0")
    assert tuple(m.predictRaw(X).shape) == (0, 3) and tuple(m.predict(X).shape) == (0,)
    assert tuple(m.predictProbability(X).shape) == (0, 3)


@gpu
def test_score_header_symbols(cuda):
    names = ["cyc_nbmodel_create", "cyc_nbmodel_destroy", "cyc_nbmodel_score_dev",
             "cyc_nbmodel_path", "cyc_nbmodel_chunk_rows"]
    syms = set(N.header_symbols())
    lib = N.load()
    for name in names:
        assert name in syms and name in N.SIGNATURES and hasattr(lib, name)
        assert not name.startswith("cyc_nb_")
    assert sorted(s for s in syms if s.startswith("cyc_nbmodel_")) == sorted(names)


@gpu
def test_fit_then_predict(cuda):
    t, d, C, n = "multinomial", 17, 3, 257
    X, y, w = R.real_rows(t, d, C, n)
    model = NaiveBayes().fit(dev(X), dev(y), dev(w))
    pred = twice(lambda: host(model.predict(dev(X))))
    yhat, amb = R.scored(t, d, C, n)[5:7]
    assert np.array_equal(pred[~amb], yhat[~amb].astype(np.float64))
