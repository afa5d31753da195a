"""numpy restatement of the MultilayerPerceptronClassifier arithmetic
(cycloneml_amd/ann.py's docstring), block after block as the DataStacker
feeds it, for tests/test_mlp_host.py and tests/test_mlp_gpu.py."""
import numpy as np


def split(layers, w):
    """[(W_l (n_l x n_{l-1}), b_l)] for l = 1..L: W_l column-major, then b_l."""
    out, off = [], 0
    for i, o in zip(layers[:-1], layers[1:]):
        W = w[off:off + o * i].reshape(i, o).T
        b = w[off + o * i:off + o * (i + 1)]
        out.append((W, b))
        off += o * (i + 1)
    assert off == w.size
    return out


def forward(layers, w, X):
    """a_0 .. a_{L-1}, z_L, a_L = softmax(z_L) of every row."""
    acts = [X]
    wb = split(layers, w)
    for l, (W, b) in enumerate(wb, 1):
        z = acts[-1] @ W.T + b
        if l < len(wb):
            acts.append(1.0 / (1.0 + np.exp(-z)))
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return acts, z, e / e.sum(axis=1, keepdims=True)


def _block(layers, w, X, y):
    """(loss_b, g_b, bound_b) of one block: means over its S_b rows; bound_b
    the same sums with |W|, |delta| and |a| (no cancellation)."""
    wb = split(layers, w)
    acts, _, p = forward(layers, w, X)
    S = X.shape[0]
    yi = y.astype(np.int64)
    loss = -np.log(p[np.arange(S), yi]).sum() / S
    d = p.copy()
    d[np.arange(S), yi] -= 1.0
    dbar = np.abs(d)
    g, gbar = [], []
    for l in range(len(wb), 0, -1):
        a = acts[l - 1]
        # column-major n_l x n_{l-1}, then the bias
        g.append(np.concatenate([(d.T @ a).T.ravel(), d.sum(axis=0)]) / S)
        gbar.append(np.concatenate([(dbar.T @ np.abs(a)).T.ravel(), dbar.sum(axis=0)]) / S)
        if l > 1:
            W = wb[l - 1][0]
            d = (d @ W) * a * (1.0 - a)
            dbar = (dbar @ np.abs(W)) * a * (1.0 - a)
    return loss, np.concatenate(g[::-1]), np.concatenate(gbar[::-1])


def loss_grad(layers, w, shards, blockSize):
    """(loss, grad, bound, B) over the shards [(X, y)]: every shard cut into
    blocks of blockSize rows (its last one may be shorter), the mean over all
    B blocks of the blocks' mean loss and mean gradient."""
    loss, grad, bound, B = 0.0, np.zeros(w.size), np.zeros(w.size), 0
    for X, y in shards:
        for r0 in range(0, X.shape[0], blockSize):
            lb, gb, bb = _block(layers, w, X[r0:r0 + blockSize], y[r0:r0 + blockSize])
            loss += lb
            grad += gb
            bound += bb
            B += 1
    return loss / B, grad / B, bound / B, B


def forward_bounds(layers, w, X):
    """E (n x n_L): the sum of absolute products behind every z_L entry, the
    error of a hidden activation carried on at the sigmoid's slope <= 1/4."""
    wb = split(layers, w)
    acts, _, _ = forward(layers, w, X)
    E = None
    for l, (W, b) in enumerate(wb, 1):
        zbar = np.abs(acts[l - 1]) @ np.abs(W).T + np.abs(b)
        E = zbar if E is None else zbar + (E / 4.0) @ np.abs(W).T
    return E
