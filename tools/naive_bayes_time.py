#!/usr/bin/env python3
"""Times NaiveBayes' dense aggregate (csrc/naive_bayes.hip) on synthetic count
rows, multinomial and gaussian.  HIP events around each call (which ends in the
read of its check flag), the median of --runs runs after --warmup warm-ups.
One JSON line per item, with DESIGN.md 5i's floor beside the time:

    aggregate  bytes = n (8 d + 16)        HBM, 8 TB/s

and the same sums in torch (index_add_ of the weighted rows).

    python tools/naive_bayes_time.py
    python tools/naive_bayes_time.py --rows 1000000 --features 64 --classes 4
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_BYTES = 8.0e12       # HBM3E


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
    import torch
    from cycloneml_amd import naive_bayes as nb
    dev = torch.device("cuda:0")
    n, d, C = a.rows, a.features, a.classes
    g = torch.Generator(device=dev).manual_seed(0)
    X = torch.randint(0, 8, (n, d), device=dev, generator=g).to(torch.float64)
    y = torch.randint(0, C, (n,), device=dev, generator=g).to(torch.float64)
    w = torch.rand(n, device=dev, generator=g, dtype=torch.float64)
    yi = y.to(torch.int64)

    def emit(item, ms, floor_ms, bound, **more):
        med, lo, hi = ms
        print(json.dumps(dict(item=item, rows=n, features=d, classes=C, median_ms=round(med, 4),
                              min_ms=round(lo, 4), max_ms=round(hi, 4),
                              floor_ms=round(floor_ms, 4), bound=bound,
                              ratio_to_floor=round(med / floor_ms, 2), **more)), flush=True)

    agg_floor = n * (8 * d + 16) / PEAK_BYTES * 1e3
    for t in ("multinomial", "gaussian"):
        plan = nb.NBPlan(C, d, t)
        sums = torch.zeros(plan.sumsLength, dtype=torch.float64, device=dev)
        emit(f"aggregate_dense_{t}", _median_ms(lambda: plan.accumulate(X, y, w, sums), a.warmup,
                                                a.runs), agg_floor, "hbm")
        plan.close()
    S = torch.zeros((C, d), dtype=torch.float64, device=dev)
    emit("torch_index_add", _median_ms(lambda: S.index_add_(0, yi, X * w[:, None]), a.warmup,
                                       a.runs), agg_floor, "hbm")


if __name__ == "__main__":
    main()
