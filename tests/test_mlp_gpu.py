"""MultilayerPerceptronClassifier on the device (csrc/mlp.hip) against the
numpy restatement of tests/mlp_restatement.py, which walks the rows block
after block.

Bars (derived, not measured):
  loss      |got - ref| <= 1e-10 ref: every term of the sum is non-negative.
  gradient  entry (l, o, j): |got - ref| <= 1e-10 sum_i s_i Dbar_l,i[o]
            |a_{l-1,i}[j]|, Dbar the restatement's back-propagation run with
            |W| and |delta| (the sum of absolute products through the chain,
            so cancellation cannot fake a failure).  Both sides round below
            about L n 2^-53 of that sum.
  forward   z_L: 1e-10 of the sum of absolute products behind the entry (a
            hidden activation's error carried on at the sigmoid's slope
            <= 1/4); probability c: 1e-10 (p_c + 2 max_c of that sum), from
            dp_c = p_c (dz_c - sum_k p_k dz_k).
A topology with one output class ([1,1], [5,1]) has softmax = 1: its loss and
gradient are exactly 0 on both sides, which is all that is checked there (the
restatement's mean loss is asserted above 0.1 everywhere else).
"""
import functools

import numpy as np
import pytest

import mlp_restatement as R
from cycloneml_amd import _native as N
from cycloneml_amd import ann
from cycloneml_amd.classification import (
    MultilayerPerceptronClassificationModel,
    MultilayerPerceptronClassifier,
)

pytestmark = pytest.mark.gpu

# (5, 20) and (5, 40): the top layer's bias epilogue on 2 and 3 column tiles
LAYERS = [(1, 1), (3, 2), (5, 1), (4, 5, 3), (17, 16, 15, 2), (16, 33, 4), (130, 65, 17, 3),
          (64, 64, 64), (1025, 8, 129), (5, 20), (5, 40)]
# (rows, blockSize, chunkRows): the row counts at blockSize 128, the block
# sizes at 257 rows, and 1000 rows in chunks of 256 (chunk edges inside
# blocks, a 104-row tail block, a 232-row tail chunk)
SHAPES = [(1, 128, 0), (127, 128, 0), (128, 128, 0), (129, 128, 0), (257, 128, 0),
          (1000, 128, 0), (257, 1, 0), (257, 7, 0), (257, 4096, 0), (1000, 128, 256)]


@functools.lru_cache(maxsize=None)
def weights_of(layers):
    w = ann.initial_weights(list(layers), 42)
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def data_of(layers, rows):
    rng = np.random.default_rng(1000 * len(layers) + layers[0] + rows)
    X = rng.standard_normal((rows, layers[0]))
    y = rng.integers(0, layers[-1], rows).astype(np.float64)
    X.setflags(write=False)
    y.setflags(write=False)
    return X, y


@functools.lru_cache(maxsize=None)
def reference(layers, rows, blockSize):
    X, y = data_of(layers, rows)
    out = R.loss_grad(list(layers), weights_of(layers), [(X, y)], blockSize)
    for a in out[1:3]:
        a.setflags(write=False)
    return out


def device_loss_grad(cuda, layers, shards, blockSize, chunkRows, totalBlocks):
    import torch
    w = torch.from_numpy(np.array(weights_of(layers))).to(cuda)
    buf = torch.zeros(w.numel() + 1, dtype=torch.float64, device=cuda)
    plan = ann.MLPPlan(list(layers), blockSize, chunkRows)
    try:
        for X, y in shards:
            plan.loss_grad(torch.from_numpy(np.array(X)).to(cuda),
                           torch.from_numpy(np.array(y)).to(cuda), w, totalBlocks,
                           buf[:-1], buf[-1:])
        torch.cuda.synchronize()
    finally:
        plan.close()
    host = buf.cpu().numpy()
    return float(host[-1]), host[:-1].copy()


def check(layers, got, ref):
    loss, grad = got
    rloss, rgrad, bound = ref
    if layers[-1] == 1:
        assert rloss == 0.0 and not rgrad.any()
        assert loss == 0.0 and not grad.any()
        return
    assert rloss > 0.1
    print(f"loss {loss!r} ref {rloss!r} rel {abs(loss - rloss) / rloss:.3e}; "
          f"grad worst {np.max(np.abs(grad - rgrad) / np.maximum(bound, 1e-300)):.3e} of bound")
    assert abs(loss - rloss) <= 1e-10 * rloss
    assert np.all(np.abs(grad - rgrad) <= 1e-10 * bound)


@pytest.mark.parametrize("rows,blockSize,chunkRows", SHAPES)
@pytest.mark.parametrize("layers", LAYERS, ids=lambda t: "-".join(map(str, t)))
def test_loss_and_gradient(cuda, layers, rows, blockSize, chunkRows):
    rloss, rgrad, bound, B = reference(layers, rows, blockSize)
    shard = [data_of(layers, rows)]
    got = device_loss_grad(cuda, layers, shard, blockSize, chunkRows, B)
    check(layers, got, (rloss, rgrad, bound))
    again = device_loss_grad(cuda, layers, shard, blockSize, chunkRows, B)
    assert again[0] == got[0] and again[1].tobytes() == got[1].tobytes()


@pytest.mark.parametrize("layers", [(4, 5, 3), (130, 65, 17, 3)],
                         ids=lambda t: "-".join(map(str, t)))
def test_two_shards_share_total_blocks(cuda, layers):
    # 257 rows as shards of 129 and 128 rows, blocks of 100: 100 + 29 and
    # 100 + 28 rows, B = 4; both shards into one buffer
    X, y = data_of(layers, 257)
    shards = [(X[:129], y[:129]), (X[129:], y[129:])]
    rloss, rgrad, bound, B = R.loss_grad(list(layers), weights_of(layers), shards, 100)
    assert B == 4
    check(layers, device_loss_grad(cuda, layers, shards, 100, 0, 4), (rloss, rgrad, bound))


def test_bad_label_is_an_error(cuda):
    import torch
    layers = (4, 5, 3)
    X, y = data_of(layers, 129)
    for bad in (3.0, -1.0, 1.5, float("nan")):
        yb = np.array(y)
        yb[77] = bad
        with pytest.raises(N.IllegalArgumentException):
            device_loss_grad(cuda, layers, [(X, yb)], 128, 0, 2)
    torch.cuda.synchronize()


@pytest.mark.parametrize("rows,chunkRows", [(1, 0), (129, 0), (257, 0), (1000, 256)])
@pytest.mark.parametrize("layers", LAYERS, ids=lambda t: "-".join(map(str, t)))
def test_forward(cuda, layers, rows, chunkRows):
    import torch
    X, _ = data_of(layers, rows)
    w = weights_of(layers)
    _, z, p = R.forward(list(layers), w, X)
    E = R.forward_bounds(list(layers), w, X)
    plan = ann.MLPPlan(list(layers), 128, chunkRows)
    try:
        raw, prob, pred = plan.forward(torch.from_numpy(np.array(X)).to(cuda),
                                       torch.from_numpy(np.array(w)).to(cuda), True, True, True)
        torch.cuda.synchronize()
    finally:
        plan.close()
    raw, prob, pred = raw.cpu().numpy(), prob.cpu().numpy(), pred.cpu().numpy()
    assert np.all(np.abs(raw - z) <= 1e-10 * E)
    assert np.all(np.abs(prob - p) <= 1e-10 * (p + 2.0 * E.max(axis=1, keepdims=True)))
    assert np.array_equal(pred, np.argmax(prob, axis=1).astype(np.float64))


def test_model_predictions(cuda):
    import torch
    layers = (16, 33, 4)
    X, _ = data_of(layers, 257)
    w = weights_of(layers)
    m = MultilayerPerceptronClassificationModel(list(layers), w)
    Xd = torch.from_numpy(np.array(X)).to(cuda)
    raw, prob, pred = m.predictRaw(Xd), m.predictProbability(Xd), m.predict(Xd)
    assert raw.is_cuda and prob.is_cuda and pred.is_cuda
    _, z, p = R.forward(list(layers), w, X)
    E = R.forward_bounds(list(layers), w, X)
    assert np.all(np.abs(raw.cpu().numpy() - z) <= 1e-10 * E)
    assert np.all(np.abs(prob.cpu().numpy() - p) <=
                  1e-10 * (p + 2.0 * E.max(axis=1, keepdims=True)))
    assert torch.equal(pred, torch.argmax(prob, dim=1).to(torch.float64))
    # ties: zero weights make every class equal, and the lowest index wins
    zero = MultilayerPerceptronClassificationModel(list(layers), np.zeros(w.size))
    assert torch.equal(zero.predictProbability(Xd), torch.full_like(prob, 0.25))
    assert not zero.predict(Xd).any()


XOR_X = np.array([[0.0, 0.0], [0.0, 1.0], [1.0, 0.0], [1.0, 1.0]])
XOR_Y = np.array([0.0, 1.0, 1.0, 0.0])


def _fit_xor(cuda, **kw):
    import torch
    est = MultilayerPerceptronClassifier([2, 5, 2], blockSize=1, seed=123, maxIter=100, **kw)
    Xd = torch.from_numpy(XOR_X).to(cuda)
    return est.fit(Xd, torch.from_numpy(XOR_Y).to(cuda)), Xd


def test_fit_xor(cuda):
    model, Xd = _fit_xor(cuda)
    assert np.array_equal(model.predict(Xd).cpu().numpy(), XOR_Y)
    hist = model.summary.objectiveHistory
    assert len(hist) >= 2 and np.all(np.diff(hist) <= 0.0)
    assert model.summary.totalIterations == len(hist) - 1
    assert model.layers == [2, 5, 2] and model.numFeatures == 2 and model.numClasses == 2
    again, _ = _fit_xor(cuda)
    assert again.weights.tobytes() == model.weights.tobytes()


def test_fit_honours_initial_weights(cuda):
    import torch
    init = np.linspace(-1.0, 1.0, ann.weight_length([2, 5, 2]))
    est = MultilayerPerceptronClassifier([2, 5, 2], blockSize=1, maxIter=0, initialWeights=init)
    model = est.fit(torch.from_numpy(XOR_X).to(cuda), torch.from_numpy(XOR_Y).to(cuda))
    assert model.weights.tobytes() == init.tobytes()
    assert model.summary.totalIterations == 0 and len(model.summary.objectiveHistory) == 1
    ref = R.loss_grad([2, 5, 2], init, [(XOR_X, XOR_Y)], 1)[0]
    assert abs(model.summary.objectiveHistory[0] - ref) <= 1e-10 * ref
