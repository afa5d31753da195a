#!/usr/bin/env python3
"""Times one MultilayerPerceptronClassifier loss + gradient evaluation
(cyc_mlp_loss_grad_dev, csrc/mlp.hip) beside the same chain written with
torch.matmul in fp64, on the same device rows in one process: HIP events, the
median of --runs runs after --warmup warm-ups, the two alternating.  One JSON
line (also appended to --out when given): rows/s of both, the share of the
fp64 MFMA peak (78.6 Tflop/s) at 6 sum n_l n_{l-1} - 2 n_1 n_0 flop per row
(forward, delta and gradient products; no delta below layer 1), the plan's
per-kernel times from the library's event hooks, and the largest difference
between the two gradients relative to the gradient's largest entry.

    python tools/probe/mlp_probe.py                       # 10M x 512, layers 512,256,100
    python tools/probe/mlp_probe.py --rows 1000000 --layers 64,64,64
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

FP64_MFMA = 78.6e12          # flop / s


def flop_per_row(layers):
    prod = sum(i * o for i, o in zip(layers[:-1], layers[1:]))
    return 6 * prod - 2 * layers[1] * layers[0]


def torch_chain(layers, X, y, w, blockSize, totalBlocks, grad, loss, chunk):
    """grad, loss += the objective's share of these rows (ann.py's arithmetic)."""
    import torch
    from cycloneml_amd import ann
    n = X.shape[0]
    offs = ann.layer_offsets(layers)
    Ws = [w[a:b].view(i, o) for (a, b), i, o in zip(offs, layers[:-1], layers[1:])]   # W_l^T
    bs = [w[b:b + o] for (a, b), o in zip(offs, layers[1:])]
    for r0 in range(0, n, chunk):
        rows = torch.arange(r0, min(n, r0 + chunk), device=X.device)
        blk = torch.div(rows, blockSize, rounding_mode="floor")
        s = 1.0 / (torch.clamp(n - blk * blockSize, max=blockSize).to(torch.float64) *
                   totalBlocks)
        acts = [X[r0:r0 + chunk]]
        for l, (Wt, b) in enumerate(zip(Ws, bs), 1):
            z = torch.addmm(b, acts[-1], Wt)
            if l < len(Ws):
                acts.append(torch.sigmoid(z))
        p = torch.softmax(z, dim=1)
        yi = y[r0:r0 + chunk].to(torch.int64).unsqueeze(1)
        loss -= (torch.log(p.gather(1, yi)).squeeze(1) * s).sum()
        d = p.scatter_add_(1, yi, torch.full_like(yi, -1, dtype=torch.float64)) * s.unsqueeze(1)
        for l in range(len(Ws), 0, -1):
            (a, b), i, o = offs[l - 1], layers[l - 1], layers[l]
            grad[a:b].view(i, o).addmm_(acts[l - 1].t(), d)
            grad[b:b + o] += d.sum(dim=0)
            if l > 1:
                d = torch.mm(d, Ws[l - 1].t()) * acts[l - 1] * (1.0 - acts[l - 1])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--layers", default="512,256,100")
    ap.add_argument("--block-size", type=int, default=128)
    ap.add_argument("--chunk-rows", type=int, default=0, help="the plan's chunkRows (0: default)")
    ap.add_argument("--torch-chunk", type=int, default=1_000_000)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None, help="append the JSON line to this file")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("mlp_probe.py needs a GPU")
    from cycloneml_amd import _native as N
    from cycloneml_amd import ann
    device = torch.device("cuda:0")
    layers = [int(v) for v in a.layers.split(",")]
    n, nw = a.rows, ann.weight_length(layers)
    g = torch.Generator(device=device).manual_seed(7)
    X = torch.empty((n, layers[0]), dtype=torch.float64, device=device)
    step = max(1, (1 << 28) // layers[0])                  # 2 GiB of rows at a time
    for r in range(0, n, step):
        X[r:r + step].normal_(generator=g)
    y = torch.randint(0, layers[-1], (n,), device=device, generator=g).to(torch.float64)
    w = torch.from_numpy(ann.initial_weights(layers, 7)).to(device)
    B = (n + a.block_size - 1) // a.block_size
    plan = ann.MLPPlan(layers, a.block_size, a.chunk_rows)
    bufs = {k: torch.zeros(nw + 1, dtype=torch.float64, device=device) for k in ("mlp", "torch")}

    def ours():
        bufs["mlp"].zero_()
        plan.loss_grad(X, y, w, B, bufs["mlp"][:nw], bufs["mlp"][nw:])

    def theirs():
        bufs["torch"].zero_()
        torch_chain(layers, X, y, w, a.block_size, B, bufs["torch"][:nw], bufs["torch"][nw:],
                    a.torch_chunk)

    for _ in range(a.warmup):
        ours()
        theirs()
    torch.cuda.synchronize()
    ms = {"mlp": [], "torch": []}
    for _ in range(a.runs):
        for name, fn in (("mlp", ours), ("torch", theirs)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1))
    # per-kernel times of one more evaluation (the hooks add events: not timed above)
    N.profile_enable(True)
    ours()
    torch.cuda.synchronize()
    kernels = {k: round(N.profile_query(k)[0], 3) for k in ("k_mlp_gemm", "k_mlp_grad")}
    N.profile_enable(False)
    gm, gt = bufs["mlp"][:nw], bufs["torch"][:nw]
    res = {"rows": n, "layers": layers, "blockSize": a.block_size,
           "device": torch.cuda.get_device_name(device), "warmup": a.warmup, "runs": a.runs,
           "flop_per_row": flop_per_row(layers), "kernel_ms": kernels,
           "loss": [float(bufs["mlp"][nw]), float(bufs["torch"][nw])],
           "grad_diff_over_max": float((gm - gt).abs().max() / gt.abs().max())}
    for name in ("mlp", "torch"):
        med = statistics.median(ms[name])
        res[name + "_ms"] = round(med, 3)
        res[name + "_range"] = [round(min(ms[name]), 3), round(max(ms[name]), 3)]
        res[name + "_rows_per_s"] = round(n / (med * 1e-3))
        res[name + "_mfma_peak_share"] = round(flop_per_row(layers) * n / (med * 1e-3) / FP64_MFMA,
                                               4)
    res["mlp_over_torch"] = round(res["mlp_ms"] / res["torch_ms"], 3)
    plan.close()
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
