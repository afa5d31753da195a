"""NaiveBayes without a device: the M step's known answers and its equality
with the restatement, the refusals, persistence, and the restated raw forms with
the condition on the generators (at most 1 % of a case's rows ambiguous)."""
import json
import os

import numpy as np
import pytest

import naive_bayes_restatement as R
from cycloneml_amd import _native as N
from cycloneml_amd import naive_bayes as nb
from cycloneml_amd import persist
from cycloneml_amd.classification import NaiveBayes, NaiveBayesModel

log = np.log

# class 0: [1, 0] and [2, 1]; class 1: [0, 3]
KX = np.array([[1.0, 0.0], [2.0, 1.0], [0.0, 3.0]])
KY = np.array([0.0, 0.0, 1.0])


def known_sums(X):
    W, S, Q, _, _ = R.aggregate(X, KY, None, 2, "multinomial")
    return R.sums_buffer(W, S, Q)


def test_known_answer_multinomial():
    pi, theta, sigma = nb.m_step(known_sums(KX), 2, 2, "multinomial", 1.0)
    assert np.array_equal(pi, [log(3.0) - log(5.0), log(2.0) - log(5.0)])
    np.testing.assert_allclose(theta, [[log(4 / 6), log(2 / 6)], [log(1 / 5), log(4 / 5)]],
                               rtol=4e-16, atol=0)
    assert np.array_equal(theta, [[log(4.0) - log(6.0), log(2.0) - log(6.0)],
                                  [log(1.0) - log(5.0), log(4.0) - log(5.0)]])
    assert sigma.shape == (0, 0)


def test_known_answer_complement():
    # S = [[3, 1], [0, 3]]: T = [3, 4], K = [[0, 3], [3, 1]]
    pi, theta, _ = nb.m_step(known_sums(KX), 2, 2, "complement", 1.0)
    assert np.array_equal(pi, [log(3.0) - log(5.0), log(2.0) - log(5.0)])
    assert np.array_equal(theta, [[-(log(1.0) - log(5.0)), -(log(4.0) - log(5.0))],
                                  [-(log(4.0) - log(6.0)), -(log(2.0) - log(6.0))]])


def test_known_answer_bernoulli():
    # the same rows as 0/1: S = [[2, 1], [0, 1]], W = [2, 1]
    pi, theta, _ = nb.m_step(known_sums((KX > 0).astype(np.float64)), 2, 2, "bernoulli", 1.0)
    assert np.array_equal(pi, [log(3.0) - log(5.0), log(2.0) - log(5.0)])
    assert np.array_equal(theta, [[log(3.0) - log(4.0), log(2.0) - log(4.0)],
                                  [log(1.0) - log(3.0), log(2.0) - log(3.0)]])


def test_known_answer_gaussian():
    W, S, Q, _, _ = R.aggregate(KX, KY, None, 2, "gaussian")
    pi, theta, sigma = nb.m_step(R.sums_buffer(W, S, Q), 2, 2, "gaussian")
    assert np.array_equal(pi, [log(2.0) - log(3.0), log(1.0) - log(3.0)])
    assert np.array_equal(theta, [[1.5, 0.5], [0.0, 3.0]])
    # per-feature variances over all rows: [5/3 - 1, 10/3 - 16/9]
    eps = 1e-9 * max(5.0 / 3.0 - 3.0 * 3.0 / 3.0 / 3.0, 10.0 / 3.0 - 4.0 * 4.0 / 3.0 / 3.0)
    assert np.array_equal(sigma, [[eps + 2.5 - 2.25, eps + 0.5 - 0.25],
                                  [eps + 0.0 - 0.0, eps + 9.0 - 9.0]])


@pytest.mark.parametrize("modelType", R.TYPES)
@pytest.mark.parametrize("d,C,n", [(1, 1, 5), (17, 3, 257), (65, 17, 300)])
def test_m_step_equals_restatement(modelType, d, C, n):
    X, y, w = R.real_rows(modelType, d, C, n)
    W, S, Q, _, _ = R.aggregate(X, y, w, C, modelType)
    for lam in (1.0, 0.25):
        got = nb.m_step(R.sums_buffer(W, S, Q), C, d, modelType, lam)
        ref = R.m_step(W, S, Q, modelType, lam)
        for g, r in zip(got, ref):
            assert g.shape == r.shape and g.tobytes() == r.tobytes()


def test_sums_layout():
    assert nb.sums_length(3, 5) == 18 and nb.sums_length(3, 5, "gaussian") == 33
    W, S, Q = nb.split_sums(np.arange(33.0), 3, 5, "gaussian")
    assert W.tolist() == [0, 1, 2] and S[1, 0] == 8 and Q[0, 0] == 18 and Q[2, 4] == 32
    with pytest.raises(N.IllegalArgumentException):
        nb.split_sums(np.zeros(17), 3, 5)


def test_refusals():
    with pytest.raises(N.IllegalArgumentException, match="smoothing"):
        NaiveBayes(smoothing=-1.0)
    with pytest.raises(N.IllegalArgumentException, match="smoothing"):
        NaiveBayes(smoothing=float("nan"))
    with pytest.raises(N.IllegalArgumentException, match="unknown modelType"):
        NaiveBayes(modelType="poisson")
    with pytest.raises(N.IllegalArgumentException, match="unknown modelType"):
        NaiveBayesModel([0.0], [[0.0]], modelType="poisson")
    # a class without weight
    sums = known_sums(KX)
    sums[1] = 0.0
    with pytest.raises(N.IllegalArgumentException, match="class 1 has no weight"):
        nb.m_step(sums, 2, 2)
    # 1 to 1024 classes
    with pytest.raises(N.IllegalArgumentException, match="1 to 1024 classes"):
        NaiveBayesModel(np.zeros(1025), np.zeros((1025, 1)))
    with pytest.raises(N.IllegalArgumentException, match="1 to 1024 classes"):
        nb.check_shape(0)
    with pytest.raises(N.IllegalArgumentException):
        NaiveBayesModel([0.0, 0.0], [[0.0]])
    # sigma goes with gaussian alone
    with pytest.raises(N.IllegalArgumentException, match="needs sigma"):
        NaiveBayesModel([0.0], [[0.0]], None, "gaussian")
    with pytest.raises(N.IllegalArgumentException, match="has no sigma"):
        NaiveBayesModel([0.0], [[0.0]], [[1.0]], "multinomial")
    assert not hasattr(NaiveBayes(), "thresholds")


@pytest.mark.parametrize("modelType", R.TYPES)
def test_fit_refuses_csr(modelType):
    from cycloneml_amd.linalg import CSRRows
    z = np.zeros(2, dtype=np.int64)
    rows = CSRRows(z, np.zeros(0, dtype=np.int32), np.zeros(0), 3)
    with pytest.raises(N.IllegalArgumentException, match="dense rows"):
        NaiveBayes(modelType=modelType).fit(rows, np.zeros(1))


def test_model_on_host_arrays():
    m = NaiveBayesModel([-0.5, -1.0], [[-1.0, -2.0, -3.0], [-3.0, -2.0, -1.0]])
    assert (m.numClasses, m.numFeatures, m.modelType) == (2, 3, "multinomial")
    assert m.sigma.shape == (0, 0)


@pytest.mark.parametrize("modelType", R.TYPES)
def test_save_load_same_bytes(tmp_path, modelType):
    pi, theta, sigma = R.model_of(modelType, 17, 3, 257)
    m = NaiveBayesModel(pi, theta, sigma if modelType == "gaussian" else None, modelType, 0.25)
    path = str(tmp_path / "nb")
    m.save(path)
    meta = persist.read_metadata(path)
    assert meta["class"] == "org.apache.spark.ml.classification.NaiveBayesModel"
    assert meta["paramMap"] == {"modelType": modelType, "smoothing": 0.25}
    back = NaiveBayesModel.load(path)
    assert back.modelType == modelType and back.smoothing == 0.25
    for a, b in ((m.pi, back.pi), (m.theta, back.theta), (m.sigma, back.sigma)):
        assert a.shape == b.shape and a.tobytes() == b.tobytes()
    row = persist._read_parquet_rows(os.path.join(path, "data"))[0]
    assert list(row) == ["pi", "theta", "sigma"]
    if modelType != "gaussian":
        assert (row["sigma"]["numRows"], row["sigma"]["numCols"]) == (0, 0)
    with pytest.raises(IOError):
        m.save(path)
    m.save(path, overwrite=True)


def test_load_spark2_layout_without_sigma(tmp_path):
    pa, _ = persist._pa()
    pi, theta, _ = R.model_of("multinomial", 17, 3, 257)
    path = str(tmp_path / "nb2")
    meta = {"class": persist.NB_CLASS, "timestamp": 1, "sparkVersion": "2.4.8", "uid": "nb_x",
            "paramMap": {"smoothing": 1.0, "modelType": "multinomial"}}
    persist._write_text(os.path.join(path, "metadata"), json.dumps(meta))
    fields = [pa.field("pi", persist._arrow_vector()), pa.field("theta", persist._arrow_matrix())]
    spark = [persist._field("pi", persist._udt("vector")),
             persist._field("theta", persist._udt("matrix"))]
    persist._write_parquet(os.path.join(path, "data"), fields, spark,
                           [{"pi": persist.encode_dense_vector(pi),
                             "theta": persist.encode_dense_matrix(theta, True)}])
    m = persist.load_naive_bayes_model(path)
    assert m.modelType == "multinomial" and m.sigma.shape == (0, 0)
    assert m.pi.tobytes() == pi.tobytes() and m.theta.tobytes() == theta.tobytes()


def test_restated_raw_forms_known_answers():
    """The four raw forms, the probability and the argmax on two classes x two
    features, against the formulas written out."""
    pi = np.array([log(0.25), log(0.75)])
    theta = np.array([[log(0.5), log(0.25)], [log(0.125), log(0.5)]])
    X = np.array([[1.0, 0.0], [0.0, 1.0], [1.0, 1.0]])
    r, B = R.raw(X, pi, theta, None, "multinomial")
    want = pi[None, :] + X @ theta.T
    assert np.array_equal(r, want)
    assert np.array_equal(B, np.abs(pi)[None, :] + X @ np.abs(theta).T)
    t = X @ theta.T
    r, _ = R.raw(X, pi, theta, None, "complement")
    m = t.max(axis=1, keepdims=True)
    np.testing.assert_allclose(r, t - (m + log(np.exp(t - m).sum(axis=1, keepdims=True))),
                               rtol=0, atol=1e-15)
    np.testing.assert_allclose(np.exp(r).sum(axis=1), 1.0, rtol=0, atol=1e-15)
    r, _ = R.raw(X, pi, theta, None, "bernoulli")
    L = np.log1p(-np.exp(theta))
    want = (pi + L.sum(axis=1))[None, :] + X @ (theta - L).T
    np.testing.assert_allclose(r, want, rtol=1e-15, atol=0)
    # row [1, 0] under class 0: log(1/4) + log(1/2) + log(1 - 1/4)
    assert abs(r[0, 0] - (log(0.25) + log(0.5) + log(0.75))) < 1e-15
    mu, sg = np.array([[0.0, 1.0], [2.0, -1.0]]), np.array([[1.0, 4.0], [0.25, 1.0]])
    r, B = R.raw(X, pi, mu, sg, "gaussian")
    want = np.array([[pi[c] - (((x - mu[c]) ** 2 / sg[c]).sum() + log(sg[c]).sum()) / 2.0
                      for c in range(2)] for x in X])
    np.testing.assert_allclose(r, want, rtol=1e-15, atol=0)
    assert np.all(B >= np.abs(r))
    p = R.probability(r)
    np.testing.assert_allclose(p, np.exp(want) / np.exp(want).sum(axis=1, keepdims=True),
                               rtol=1e-14, atol=0)
    assert R.predict(np.array([[1.0, 3.0, 3.0], [2.0, 2.0, 1.0], [np.nan, 5.0, 1.0]])).tolist() \
        == [1, 0, 0]
    # identical classes are constructed ties, never ambiguous
    th2 = np.array([theta[0], theta[0]])
    assert R.duplicates(np.zeros(2), th2, None, "complement").tolist() == [False, True]
    assert R.duplicates(pi, th2, None, "multinomial").tolist() == [False, False]


def test_generators_leave_few_rows_ambiguous():
    """The condition on the generators for prediction checks: per case (every
    model type at every shape of shape_cases) at most 1 % of the rows have
    their two best raw values within the sum of the two bars, counted on the
    restatement alone."""
    for t in R.TYPES:
        for (d, C, n) in R.shape_cases():
            r, B, rb, pb, p, yhat, amb = R.scored(t, d, C, n)
            assert r.shape == B.shape == rb.shape == pb.shape == p.shape == (n, C)
            assert yhat.shape == (n,) and np.all(pb >= 0) and np.all(rb >= 0)
            assert amb.sum() <= 0.01 * amb.size, (t, d, C, n, int(amb.sum()))


def test_plan_refuses_too_many_features():
    with pytest.raises(N.IllegalArgumentException, match="features"):
        nb.NBPlan(1, (1 << 24), "multinomial")
