"""NaiveBayes scoring without a device: the scoring operands against the
restatement's inline forms by bytes, the device's arithmetic restated over
those operands, the refusals that need no device, and a host-array model's
persistence."""
import numpy as np
import pytest
import torch

import naive_bayes_restatement as R
from cycloneml_amd import _native as N
from cycloneml_amd import naive_bayes as nb
from cycloneml_amd.classification import NaiveBayesModel

CASES = [(1, 1, 5), (17, 3, 257), (65, 17, 65)]


@pytest.mark.parametrize("d,C,n", CASES)
def test_operands_equal_the_inline_forms(d, C, n):
    pi, theta, _ = R.model_of("bernoulli", d, C, n)
    b, M, V, ls, finite = nb.score_operands(pi, theta, None, "bernoulli")
    L = np.log1p(-np.exp(theta))
    s = np.zeros(C)
    for j in range(d):
        s = s + L[:, j]
    assert b.tobytes() == (pi + s).tobytes() and M.tobytes() == (theta - L).tobytes()
    assert V is None and ls is None and finite
    pi, theta, _ = R.model_of("complement", d, C, n)
    b, M, V, ls, finite = nb.score_operands(pi, theta, None, "complement")
    assert b.tobytes() == np.zeros(C).tobytes() and M.tobytes() == theta.tobytes() and finite
    pi, theta, _ = R.model_of("multinomial", d, C, n)
    b, M, V, ls, finite = nb.score_operands(pi, theta, np.zeros((0, 0)), "multinomial")
    assert b.tobytes() == pi.tobytes() and M.tobytes() == theta.tobytes() and V is None
    pi, theta, sigma = R.model_of("gaussian", d, C, n)
    b, M, V, ls, finite = nb.score_operands(pi, theta, sigma, "gaussian")
    want = np.zeros(C)
    for j in range(d):
        want = want + np.log(sigma[:, j])
    assert ls.tobytes() == want.tobytes() and V.tobytes() == sigma.tobytes()
    assert b.tobytes() == pi.tobytes() and M.tobytes() == theta.tobytes()
    for a in (b, M, V, ls):
        assert a.dtype == np.float64 and a.flags.c_contiguous


def plain_path(X, b, M, V, ls, modelType):
    """The plain kernel's arithmetic over the operands: j ascending, a zero
    skipped, b added last (before complement's normalization)."""
    n = X.shape[0]
    acc = np.zeros((n, b.size))
    with np.errstate(all="ignore"):
        for j in range(X.shape[1]):
            xj = X[:, j, None]
            if modelType == "gaussian":
                df = xj - M[None, :, j]
                acc = acc + df * df / V[None, :, j]
            else:
                acc = acc + np.where(xj != 0.0, xj * M[None, :, j], 0.0)
        if modelType == "gaussian":
            return b[None, :] - (acc + ls[None, :]) / 2.0
        return b[None, :] + acc


@pytest.mark.parametrize("t", ("multinomial", "bernoulli", "gaussian"))
@pytest.mark.parametrize("d,C,n", CASES)
def test_operands_give_the_restated_raw(t, d, C, n):
    X = R.real_rows(t, d, C, n)[0]
    pi, theta, sigma = R.model_of(t, d, C, n)
    got = plain_path(X, *nb.score_operands(pi, theta, sigma, t)[:4], t)
    assert got.tobytes() == R.raw(X, pi, theta, sigma, t)[0].tobytes()


def test_finite_flag():
    theta = np.array([[-1.0, -np.inf], [-2.0, -0.5]])
    pi = np.array([-0.5, -1.0])
    assert not nb.score_operands(pi, theta, None, "multinomial")[4]
    assert not nb.score_operands(pi, theta, None, "complement")[4]
    b, M, _, _, finite = nb.score_operands(pi, theta, None, "bernoulli")
    assert not finite and M[0, 1] == -np.inf and np.isfinite(b).all()
    # theta = 0 (probability 1): L = -inf, so M = +inf and b = -inf
    b, M, _, _, finite = nb.score_operands(pi, np.array([[0.0, -1.0], [-2.0, -0.5]]), None,
                                           "bernoulli")
    assert not finite and M[0, 0] == np.inf and b[0] == -np.inf
    assert nb.score_operands(pi, np.nan_to_num(theta, neginf=-700.0), None, "multinomial")[4]
    # a NaN is not finite either; b does not count
    assert not nb.score_operands(pi, np.array([[np.nan, 0.0], [0.0, 0.0]]), None)[4]
    assert nb.score_operands(np.array([-np.inf, 0.0]), np.zeros((2, 2)), None)[4]


def test_refusals_without_a_device():
    from cycloneml_amd.linalg import CSRRows
    m = NaiveBayesModel([-0.5, -1.0], [[-1.0, -2.0, -3.0], [-3.0, -2.0, -1.0]])
    z = np.zeros(2, dtype=np.int64)
    rows = CSRRows(z, np.zeros(0, dtype=np.int32), np.zeros(0), 3)
    for fn in (m.predictRaw, m.predictProbability, m.predict):
        with pytest.raises(N.IllegalArgumentException, match="CSR form is not provided"):
            fn(rows)
        with pytest.raises(N.IllegalArgumentException, match="have 4 features but the model has 3"):
            fn(torch.zeros((2, 4), dtype=torch.float64))
        with pytest.raises(N.IllegalArgumentException, match="contiguous fp64 device tensor"):
            fn(torch.zeros((2, 3), dtype=torch.float32))
        with pytest.raises(N.IllegalArgumentException, match="contiguous fp64 device tensor"):
            fn(torch.zeros((3, 2), dtype=torch.float64).t())
        with pytest.raises(N.IllegalArgumentException, match="contiguous fp64 device tensor"):
            fn(torch.zeros(3, dtype=torch.float64))
        with pytest.raises(N.IllegalArgumentException, match="contiguous fp64 device tensor"):
            fn(np.zeros((2, 3)))
        with pytest.raises(N.IllegalArgumentException, match="contiguous fp64 device tensor"):
            fn(torch.zeros((2, 3), dtype=torch.float64))       # host rows
    with pytest.raises(N.IllegalArgumentException, match="scorer given invalid value"):
        nb.NBScorer(m.pi, m.theta, scorer="fast")
    with pytest.raises(N.IllegalArgumentException, match="product scorer"):
        nb.NBScorer(m.pi, np.full((2, 3), -np.inf), scorer="product")
    with pytest.raises(N.IllegalArgumentException, match="product scorer"):
        nb.NBScorer(m.pi, m.theta, np.ones((2, 3)), "gaussian", scorer="product")
    # the library's argument checks come before it looks for a device
    lib = N.load()
    for args in ((0, 3, 0, 0, 1, 1, None, None, 0), (2, 3, 4, 0, 1, 1, None, None, 0),
                 (2, 3, 0, 0, 1, 1, None, None, 3), (2, 3, 3, 0, 1, 1, 1, 1, 1),
                 (2, 3, 3, 0, 1, 1, None, None, 0), (2, 3, 0, 0, None, 1, None, None, 0)):
        import ctypes
        assert lib.cyc_nbmodel_create(*args, None, ctypes.byref(ctypes.c_void_p())) \
            == N.CYC_ERR_INVALID_ARG, args
    assert lib.cyc_nbmodel_path(None) == -1 and lib.cyc_nbmodel_chunk_rows(None) == -1


@pytest.mark.parametrize("modelType", R.TYPES)
def test_host_model_still_saves_and_loads(tmp_path, modelType):
    pi, theta, sigma = R.model_of(modelType, 17, 3, 257)
    m = NaiveBayesModel(pi, theta, sigma if modelType == "gaussian" else None, modelType)
    path = str(tmp_path / "nb")
    m.save(path)
    back = NaiveBayesModel.load(path)
    for a, b in ((m.pi, back.pi), (m.theta, back.theta), (m.sigma, back.sigma)):
        assert a.shape == b.shape and a.tobytes() == b.tobytes()
    assert all(hasattr(back, f) for f in ("predictRaw", "predictProbability", "predict"))
