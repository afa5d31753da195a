"""MultilayerPerceptronClassifier, host side: the numpy restatement the GPU
tests compare against (tests/mlp_restatement.py) checked against finite
differences, the weight layout and initialiser, the estimator's validation,
the C ABI's argument errors (no device needed) and model persistence."""
import ctypes
import os

import numpy as np
import pytest

import mlp_restatement as R
from cycloneml_amd import _native as N
from cycloneml_amd import ann, persist
from cycloneml_amd.classification import (
    MultilayerPerceptronClassificationModel,
    MultilayerPerceptronClassifier,
)
from cycloneml_amd.kmeans_init import XORShiftRandom

FIX = os.path.join(os.path.dirname(__file__), "golden", "ml-models", "mlp-2.4.4")


def test_restatement_gradient_matches_finite_differences():
    layers, rows, bs, h = [3, 4, 2], 7, 3, 1e-6
    rng = np.random.default_rng(5)
    X = rng.standard_normal((rows, layers[0]))
    y = rng.integers(0, layers[-1], rows).astype(np.float64)
    w = rng.uniform(-1.0, 1.0, ann.weight_length(layers))
    _, grad, _, B = R.loss_grad(layers, w, [(X, y)], bs)
    assert B == 3
    fd = np.empty_like(w)
    for k in range(w.size):
        e = np.zeros_like(w)
        e[k] = h
        fd[k] = (R.loss_grad(layers, w + e, [(X, y)], bs)[0] -
                 R.loss_grad(layers, w - e, [(X, y)], bs)[0]) / (2 * h)
    # relative to the gradient's largest entry (central differences: h^2 f''' and
    # eps f / h are both ~1e-10 here)
    assert np.max(np.abs(fd - grad)) <= 1e-6 * np.max(np.abs(grad))


def test_weight_length_and_layout():
    layers = [4, 5, 3]
    assert ann.weight_length(layers) == 5 * 4 + 5 + 3 * 5 + 3 == 43
    assert ann.layer_offsets(layers) == [(0, 20), (25, 40)]
    w = np.arange(43, dtype=np.float64)
    (W1, b1), (W2, b2) = R.split(layers, w)
    assert W1.shape == (5, 4) and W2.shape == (3, 5)
    # W_l[o, i] at i n_l + o; b_l after W_l
    assert W1[2, 3] == 3 * 5 + 2 and W2[1, 4] == 25 + 4 * 3 + 1
    assert list(b1) == [20, 21, 22, 23, 24] and list(b2) == [40, 41, 42]


def test_initial_weights_follow_xorshift():
    layers, seed = [4, 5, 3], 11
    w = ann.initial_weights(layers, seed)
    rng = XORShiftRandom(seed)
    draws = [rng.next_double() for _ in range(w.size)]
    assert w[0] == (draws[0] * 4.8 - 2.4) / np.sqrt(4.0)
    assert w[24] == (draws[24] * 4.8 - 2.4) / np.sqrt(4.0)      # the last of layer 1: b_1
    assert w[25] == (draws[25] * 4.8 - 2.4) / np.sqrt(5.0)      # the first of layer 2
    assert w[-1] == (draws[-1] * 4.8 - 2.4) / np.sqrt(5.0)
    assert np.all(np.abs(w[:25]) <= 2.4 / 2.0) and np.all(np.abs(w[25:]) <= 2.4 / np.sqrt(5.0))


def test_default_seed_is_the_class_name_hash():
    assert ann.java_string_hash("") == 0 and ann.java_string_hash("a") == 97
    assert ann.java_string_hash("hello") == 99162322
    assert MultilayerPerceptronClassifier([2, 2]).seed == ann.DEFAULT_SEED
    assert -2 ** 31 <= ann.DEFAULT_SEED < 2 ** 31


def test_estimator_validation():
    IAE = N.IllegalArgumentException
    with pytest.raises(IAE):
        MultilayerPerceptronClassifier([3, 2], solver="gd")
    with pytest.raises(IAE):
        MultilayerPerceptronClassifier([3])
    with pytest.raises(IAE):
        MultilayerPerceptronClassifier([])
    with pytest.raises(IAE):
        MultilayerPerceptronClassifier([3, 2], blockSize=0)
    with pytest.raises(IAE):
        MultilayerPerceptronClassifier([3, 2], blockSize=-4)
    with pytest.raises(IAE):
        MultilayerPerceptronClassifier([3, 4097, 2])
    with pytest.raises(IAE):
        MultilayerPerceptronClassifier([3, 0, 2])
    with pytest.raises(IAE):
        MultilayerPerceptronClassifier([3, 2], initialWeights=np.zeros(7))
    est = MultilayerPerceptronClassifier([3, 2], initialWeights=np.zeros(8))
    assert est.blockSize == 128 and est.maxIter == 100 and est.tol == 1e-6
    assert est.solver == "l-bfgs" and est.stepSize == 0.03


def test_fit_refuses_wrong_width_and_csr_rows():
    import torch
    from cycloneml_amd.linalg import CSRRows
    est = MultilayerPerceptronClassifier([3, 2])
    with pytest.raises(N.IllegalArgumentException):
        est.fit(torch.zeros((4, 5), dtype=torch.float64), torch.zeros(4, dtype=torch.float64))
    csr = CSRRows.__new__(CSRRows)      # fit looks at the type alone
    with pytest.raises(N.IllegalArgumentException):
        est.fit(csr, torch.zeros(4, dtype=torch.float64))


def _create(layers, blockSize=128, chunkRows=0, nlayers=None, plan=True):
    lib = N.load()
    arr = (ctypes.c_int32 * max(1, len(layers)))(*layers)
    h = ctypes.c_void_p()
    rc = lib.cyc_mlp_plan_create(arr, len(layers) if nlayers is None else nlayers, blockSize,
                                 chunkRows, ctypes.byref(h) if plan else None)
    if rc == N.CYC_OK:
        lib.cyc_mlp_plan_destroy(h)
    return rc, lib.cyc_last_error().decode()


def test_c_abi_argument_errors_need_no_device():
    lib = N.load()
    for bad in ([3], [3, 0, 2], [3, 4097, 2], [-1, 2]):
        rc, msg = _create(bad)
        assert rc == N.CYC_ERR_INVALID_ARG and msg.startswith("requirement failed"), (bad, msg)
    assert "4097" in _create([3, 4097, 2])[1]
    assert _create([3, 2], blockSize=0)[0] == N.CYC_ERR_INVALID_ARG
    assert _create([3, 2], chunkRows=-1)[0] == N.CYC_ERR_INVALID_ARG
    assert _create([3, 2], plan=False)[0] == N.CYC_ERR_INVALID_ARG
    assert lib.cyc_mlp_plan_create(None, 2, 128, 0, ctypes.byref(ctypes.c_void_p())) == \
        N.CYC_ERR_INVALID_ARG
    # valid arguments: a plan with a device, CYC_ERR_NO_DEVICE without
    assert _create([3, 4, 2])[0] in (N.CYC_OK, N.CYC_ERR_NO_DEVICE)
    assert lib.cyc_mlp_loss_grad_dev(None, None, None, 0, None, 1, None, None, None) == \
        N.CYC_ERR_INVALID_ARG
    assert lib.cyc_mlp_forward_dev(None, None, 0, None, None, None, None, None) == \
        N.CYC_ERR_INVALID_ARG
    assert lib.cyc_mlp_plan_destroy(None) == N.CYC_OK


def test_reference_written_model_loads():
    m = persist.load_mlp_model(FIX)
    assert isinstance(m, MultilayerPerceptronClassificationModel)
    assert len(m.layers) >= 2 and all(n >= 1 for n in m.layers)
    assert sum(o * (i + 1) for i, o in zip(m.layers[:-1], m.layers[1:])) == len(m.weights)
    assert m.numFeatures == m.layers[0] and m.numClasses == m.layers[-1]
    assert np.all(np.isfinite(m.weights))


def test_save_load_round_trip_is_bit_identical(tmp_path):
    layers = [4, 5, 3]
    w = ann.initial_weights(layers, 3)
    w[0], w[1], w[2] = -0.0, 5e-324, 1.7976931348623157e308
    m = MultilayerPerceptronClassificationModel(layers, w)
    path = str(tmp_path / "mlp")
    m.save(path)
    meta = persist.read_metadata(path)
    assert meta["class"] == persist.MLP_CLASS and meta["paramMap"]["layers"] == layers
    back = MultilayerPerceptronClassificationModel.load(path)
    assert back.layers == layers
    assert back.weights.tobytes() == w.tobytes()
    with pytest.raises(IOError):
        m.save(path)
    m.save(path, overwrite=True)
