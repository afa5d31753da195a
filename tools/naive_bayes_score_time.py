#!/usr/bin/env python3
"""Times NaiveBayesModel's predictRaw and predict (csrc/naive_bayes_score.hip)
on synthetic count rows, multinomial (the MFMA product path) and gaussian (the
plain path).  HIP events around each call (a checked model type's call ends in
the read of its flag), the median of --runs runs after --warmup warm-ups.  One
JSON line per item, with DESIGN.md 5i's floor beside the time:

    predictRaw  bytes = n (8 d + 8 C)      HBM, 8 TB/s   (flop = 2 n C d)
    predict     bytes = n (8 d + 8)

the same product in torch (torch.addmm(pi, X, theta.T), which checks no row and
skips no zero), and, from one more call under the library's kernel timers, the
time of each kernel (k_nbs_check is the separate row-check pass).

    python tools/naive_bayes_score_time.py
    python tools/naive_bayes_score_time.py --rows 1000000 --features 64 --classes 4
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_BYTES = 8.0e12       # HBM3E
KERNELS = ("k_nbs_check", "k_nbs_gemm", "k_nbs_plain", "k_nbs_finish")


def _median_ms(fn, warmup, runs):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--features", type=int, default=256)
    ap.add_argument("--classes", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=7)
    a = ap.parse_args()
    import numpy as np
    import torch
    from cycloneml_amd import _native as N
    from cycloneml_amd.classification import NaiveBayesModel
    dev = torch.device("cuda:0")
    n, d, C = a.rows, a.features, a.classes
    g = torch.Generator(device=dev).manual_seed(0)
    X = torch.randint(0, 8, (n, d), device=dev, generator=g).to(torch.float64)
    rng = np.random.default_rng(0)
    prof = rng.random((C, d)) + 0.05
    pi = np.log(np.full(C, 1.0 / C))
    theta = np.log(prof / prof.sum(axis=1, keepdims=True))

    def emit(item, ms, floor_ms, bound, **more):
        med, lo, hi = ms
        print(json.dumps(dict(item=item, rows=n, features=d, classes=C, median_ms=round(med, 4),
                              min_ms=round(lo, 4), max_ms=round(hi, 4),
                              floor_ms=round(floor_ms, 4), bound=bound,
                              ratio_to_floor=round(med / floor_ms, 2), **more)), flush=True)

    raw_floor = n * (8 * d + 8 * C) / PEAK_BYTES * 1e3
    pred_floor = n * (8 * d + 8) / PEAK_BYTES * 1e3
    models = {"multinomial": NaiveBayesModel(pi, theta),
              "gaussian": NaiveBayesModel(pi, 8.0 * prof, 1.0 + prof, "gaussian")}
    for t, m in models.items():
        emit(f"predictRaw_{t}", _median_ms(lambda: m.predictRaw(X), a.warmup, a.runs), raw_floor,
             "hbm", gflop=round(2.0 * n * C * d / 1e9, 1))
        emit(f"predict_{t}", _median_ms(lambda: m.predict(X), a.warmup, a.runs), pred_floor, "hbm")
        N.profile_enable(True)
        for k in KERNELS:
            N.profile_query(k)
        m.predict(X)
        torch.cuda.synchronize()
        print(json.dumps(dict(item=f"predict_{t}_kernels",
                              **{k: round(N.profile_query(k)[0], 4) for k in KERNELS})),
              flush=True)
        N.profile_enable(False)
    pid, thd = torch.from_numpy(pi).to(dev), torch.from_numpy(theta).to(dev)
    emit("torch_addmm", _median_ms(lambda: torch.addmm(pid, X, thd.T), a.warmup, a.runs),
         raw_floor, "hbm")


if __name__ == "__main__":
    main()
