"""FM on the host: fit_step over FMNumpyStep against the restatement's fit by
bytes, next_gaussian's anchor, the save / load round trip and the refusals."""
import numpy as np
import pytest

import fm_restatement as R
from cycloneml_amd import _native as N
from cycloneml_amd import fm, persist
from cycloneml_amd.kmeans_init import JavaRandom


@pytest.mark.parametrize("loss, solver, kw", [
    ("squared", "adamW", {}),
    ("squared", "gd", {"regParam": 0.01, "stepSize": 0.1}),
    ("logistic", "adamW", {"regParam": 0.001}),
    ("logistic", "gd", {"stepSize": 0.5}),
    ("squared", "adamW", {"fitLinear": False}),
    ("logistic", "gd", {"fitIntercept": False, "stepSize": 0.5}),
    ("squared", "adamW", {"fraction": 0.5}),
    ("squared", "gd", {"tol": 0.05, "stepSize": 0.01, "maxIter": 50}),
])
def test_fit_matches_restatement_by_bytes(loss, solver, kw):
    X, y = R.real_rows(40, 5, 3, loss == "logistic")
    kw = dict({"maxIter": 6, "seed": 7}, **kw)
    want, hist = R.fit(X, y, 3, loss, solver, **kw)
    fraction = kw.pop("fraction", 1.0)
    step = fm.FMNumpyStep(X, y, 3, loss, kw.get("fitIntercept", True), kw.get("fitLinear", True),
                          fraction)
    got, history = fm.fit_step(step, 5, 3, solver=solver, miniBatchFraction=fraction, **kw)
    assert got.tobytes() == want.tobytes()
    assert history == hist
    if "tol" in kw:
        assert 2 <= len(history) < kw["maxIter"]      # converged by tol
    else:
        assert len(history) == kw["maxIter"]


def test_next_gaussian_anchor():
    assert JavaRandom(0).next_gaussian() == 0.8025330637390305
    assert JavaRandom(42).next_gaussian() == 1.1419053154730547
    rnd = JavaRandom(42)
    a, b = rnd.next_gaussian(), rnd.next_gaussian()      # the cached second value
    rnd.set_seed(42)
    assert (rnd.next_gaussian(), rnd.next_gaussian()) == (a, b) and a != b


@pytest.mark.parametrize("cls", [fm.FMRegressionModel, fm.FMClassificationModel])
def test_save_load_round_trip(tmp_path, cls):
    rng = np.random.default_rng(0)
    m = cls(rng.normal(), rng.normal(size=5), rng.normal(size=(5, 3)))
    persist.save_fm_model(m, str(tmp_path / "m"))
    back = persist.load_fm_model(str(tmp_path / "m"))
    assert type(back) is cls and back.intercept == m.intercept
    assert back.linear.tobytes() == m.linear.tobytes()
    assert back.factors.tobytes() == m.factors.tobytes()
    assert persist.read_metadata(str(tmp_path / "m"))["class"].endswith(cls.__name__)


@pytest.mark.parametrize("kw", [
    {"factorSize": 0}, {"factorSize": 65}, {"miniBatchFraction": 0.0}, {"miniBatchFraction": 1.5},
    {"stepSize": 0.0}, {"regParam": -1.0}, {"tol": -1.0}, {"initStd": -1.0}, {"maxIter": -1},
    {"solver": "lbfgs"},
])
def test_parameter_refusals(kw):
    with pytest.raises(N.IllegalArgumentException):
        fm.FMRegressor(**kw)


def test_label_and_width_refusals():
    X, y = R.real_rows(6, 4, 0, True)
    y[2] = y[4] = 2.0
    with pytest.raises(N.IllegalArgumentException, match="row 12 "):
        fm.FMNumpyStep(X, y, 2, "logistic", rowOffset=10)
    with pytest.raises(N.IllegalArgumentException):
        fm.split_coef(np.zeros(7), 4, 2, True, True)
