"""The feed-forward network behind MultilayerPerceptronClassifier (ml/ann/
Layer.scala, ml/ann/LossFunction.scala; the kernels are csrc/mlp.hip).

Topology (FeedForwardTopology.multiLayerPerceptron, softmaxOnTop): layers =
[n_0 .. n_L], L >= 1; layer l = 1..L is affine n_{l-1} -> n_l, followed by a
sigmoid for l < L and by softmax with cross-entropy for l = L.

Weights: one flat fp64 vector; for l = 1..L in order W_l, then b_l.  W_l is
column-major n_l x n_{l-1} (W_l[o, i] at i n_l + o), b_l has n_l entries; the
length is sum n_l (n_{l-1} + 1).

Per row x (a_0 = x): z_l = W_l a_{l-1} + b_l; a_l = 1 / (1 + exp(-z_l)) for
l < L; a_L = softmax(z_L) (max-subtracted exp over its sum); the row's loss is
-log a_L[y]; delta_L = a_L - onehot(y), delta_l = (W_{l+1}^T delta_{l+1})
a_l (1 - a_l).

Blocks (DataStacker): a block is blockSize consecutive rows of a rank's shard
(the last one of a shard may be shorter).  Block b of S_b rows gives the mean
loss and mean gradient of its rows, and the objective is the mean of those
over the B blocks of all ranks -- so row i weighs s_i = 1 / (S_b(i) B).  There
is no regularization (ANNUpdater adds none).

One departure from the reference: SoftmaxLayerModelWithCrossEntropyLoss sums
target * log(output) over all classes, so an underflowed probability of a
non-target class makes the block's loss NaN (0 * -Inf).  Here only the target
class's term is taken.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np

from . import _native as N

MAX_LAYER_WIDTH = 4096


def java_string_hash(s: str) -> int:
    """java.lang.String.hashCode (a signed 32-bit int)."""
    h = 0
    for ch in s:
        h = (31 * h + ord(ch)) & 0xFFFFFFFF
    return h - (1 << 32) if h >= (1 << 31) else h


# HasSeed's default: this.getClass.getName.hashCode.toLong
DEFAULT_SEED = java_string_hash(
    "org.apache.spark.ml.classification.MultilayerPerceptronClassifier")


def check_layers(layers):
    layers = [int(n) for n in layers]
    if len(layers) < 2:
        raise N.IllegalArgumentException(
            "requirement failed: layers must hold at least the input and the output size "
            f"but got {len(layers)} entries")
    for n in layers:
        if n < 1:
            raise N.IllegalArgumentException(
                f"requirement failed: layer sizes must be positive but got {n}")
        if n > MAX_LAYER_WIDTH:
            raise N.IllegalArgumentException(
                f"requirement failed: layer sizes up to {MAX_LAYER_WIDTH} are supported "
                f"but got {n}")
    return layers


def weight_length(layers) -> int:
    return sum(int(o) * (int(i) + 1) for i, o in zip(layers[:-1], layers[1:]))


def layer_offsets(layers):
    """[(offset of W_l, offset of b_l)] for l = 1..L in the flat vector."""
    out, off = [], 0
    for i, o in zip(layers[:-1], layers[1:]):
        out.append((off, off + o * i))
        off += o * (i + 1)
    return out


def initial_weights(layers, seed: int) -> np.ndarray:
    """FeedForwardModel(topology, seed): one XORShiftRandom(seed) walks the
    layers in order; AffineLayer.initModel fills the layer's whole slice (W,
    then b) with (nextDouble * 4.8 - 2.4) / sqrt(numIn)."""
    from .kmeans_init import XORShiftRandom
    rng = XORShiftRandom(seed)
    w = np.empty(weight_length(layers), dtype=np.float64)
    pos = 0
    for i, o in zip(layers[:-1], layers[1:]):
        s = math.sqrt(i)
        for _ in range(o * (i + 1)):
            w[pos] = (rng.next_double() * 4.8 - 2.4) / s
            pos += 1
    return w


class MLPPlan:
    """cyc_mlp_plan: the topology, the DataStacker block size and the device
    workspace of one network (chunkRows 0: sized to a 1 GiB workspace)."""

    def __init__(self, layers, blockSize: int = 128, chunkRows: int = 0):
        self.layers = [int(n) for n in layers]
        self.blockSize = int(blockSize)
        self.numWeights = weight_length(self.layers) if len(self.layers) >= 2 else 0
        self._lib = N.load()
        arr = (ctypes.c_int32 * max(1, len(self.layers)))(*self.layers)
        h = ctypes.c_void_p()
        N.check(self._lib.cyc_mlp_plan_create(arr, len(self.layers), self.blockSize,
                                              int(chunkRows), ctypes.byref(h)))
        self.handle = h

    def close(self):
        if getattr(self, "handle", None):
            self._lib.cyc_mlp_plan_destroy(self.handle)
            self.handle = None

    __del__ = close

    def _rows(self, X):
        import torch
        if not torch.is_tensor(X) or X.dtype != torch.float64 or X.dim() != 2 \
                or not X.is_contiguous():
            raise N.IllegalArgumentException(
                "requirement failed: rows must be a contiguous fp64 device tensor (n x "
                f"{self.layers[0]})")
        if int(X.shape[1]) != self.layers[0]:
            raise N.IllegalArgumentException(
                f"requirement failed: the rows have {int(X.shape[1])} features but the input "
                f"layer has {self.layers[0]}")
        return int(X.shape[0])

    def _weights(self, weights):
        import torch
        if not torch.is_tensor(weights) or weights.dtype != torch.float64 \
                or weights.numel() != self.numWeights or not weights.is_contiguous():
            raise N.IllegalArgumentException(
                f"requirement failed: weights must be {self.numWeights} contiguous fp64 values")

    def loss_grad(self, X, labels, weights, totalBlocks: int, grad, loss):
        """grad (numWeights) and loss (1) += this shard's share; all device fp64."""
        import torch
        n = self._rows(X)
        self._weights(weights)
        if not torch.is_tensor(labels) or labels.dtype != torch.float64 \
                or labels.numel() != n or not labels.is_contiguous():
            raise N.IllegalArgumentException(
                f"requirement failed: labels must be {n} contiguous fp64 values")
        if grad.dtype != torch.float64 or grad.numel() != self.numWeights \
                or not grad.is_contiguous() or loss.dtype != torch.float64 or loss.numel() != 1:
            raise N.IllegalArgumentException(
                "requirement failed: grad and loss must be fp64 buffers of the weights' "
                "length and of length 1")
        N.check(self._lib.cyc_mlp_loss_grad_dev(
            self.handle, N.ptr(X), N.ptr(labels), n, N.ptr(weights), int(totalBlocks),
            N.ptr(grad), N.ptr(loss), N.stream_handle()))

    def forward(self, X, weights, raw: bool = False, prob: bool = False, pred: bool = False):
        """(raw, prob, pred) device tensors of the requested outputs (else None)."""
        import torch
        n = self._rows(X)
        self._weights(weights)
        C = self.layers[-1]
        r = torch.empty((n, C), dtype=torch.float64, device=X.device) if raw else None
        p = torch.empty((n, C), dtype=torch.float64, device=X.device) if prob else None
        y = torch.empty(n, dtype=torch.float64, device=X.device) if pred else None
        N.check(self._lib.cyc_mlp_forward_dev(self.handle, N.ptr(X), n, N.ptr(weights), N.ptr(r),
                                              N.ptr(p), N.ptr(y), N.stream_handle()))
        return r, p, y
