#!/usr/bin/env python3
"""Times the device steps of a DecisionTree fit (csrc/decision_tree.hip) on
synthetic rows: the binning of the rows, one level's histogram and route with
--nodes nodes that each hold an equal share of the rows, and the model's
predict over a balanced tree of --depth levels.  HIP events around each call,
the median of --runs runs after --warmup warm-ups.  One JSON line per item,
with DESIGN.md 5k's floor beside the time:

    bin        bytes = 8 n d     one read of the rows (the image adds n d)
    histogram  bytes = n d       one read of the image
    route      bytes = n d       counted with the histogram: a level is both
    predict    bytes = 8 n d     one read of the rows

The kernels' own times come from cyc_profile_query.

    python tools/decision_tree_time.py
    python tools/decision_tree_time.py --rows 1000000 --features 64 --classes 0
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_BYTES = 8.0e12       # HBM3E
KERNELS = ("k_dt_check", "k_dt_bin", "k_dt_key", "k_dt_runs", "k_dt_hist", "k_dt_fold",
           "k_dt_route", "k_dt_predict")


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
    ap.add_argument("--classes", type=int, default=2, help="0: the variance statistics")
    ap.add_argument("--bins", type=int, default=32)
    ap.add_argument("--nodes", type=int, default=16)
    ap.add_argument("--depth", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--runs", type=int, default=3)
    a = ap.parse_args()
    import numpy as np
    import torch
    from cycloneml_amd import _native as N
    from cycloneml_amd import tree as T
    dev = torch.device("cuda:0")
    n, d, C, B, K = a.rows, a.features, a.classes, a.bins, a.nodes
    g = torch.Generator(device=dev).manual_seed(0)
    X = torch.randn((n, d), device=dev, generator=g, dtype=torch.float64)
    y = (torch.randint(0, max(C, 2), (n,), device=dev, generator=g).to(torch.float64) if C
         else torch.randn(n, device=dev, generator=g, dtype=torch.float64))
    slot0 = torch.randint(0, K, (n,), device=dev, generator=g).to(torch.int32)
    # B - 1 thresholds per feature at the normal quantiles: every bin is used
    q = torch.distributions.Normal(0.0, 1.0).icdf(torch.arange(1, B, dtype=torch.float64) / B)
    thr = [q.numpy().copy() for _ in range(d)]
    plan = T.DTPlan(d, C)

    def emit(item, ms, floor_ms, **more):
        med, lo, hi = ms
        print(json.dumps(dict(item=item, rows=n, features=d, classes=C, bins=B,
                              median_ms=round(med, 4), min_ms=round(lo, 4), max_ms=round(hi, 4),
                              floor_ms=round(floor_ms, 4), bound="hbm",
                              ratio_to_floor=round(med / floor_ms, 2), **more)), flush=True)

    rows_floor = 8.0 * n * d / PEAK_BYTES * 1e3
    level_floor = 1.0 * n * d / PEAK_BYTES * 1e3
    emit("bin", _median_ms(lambda: plan.bin(X, thr), a.warmup, a.runs), rows_floor)
    image = plan.bin(X, thr)
    nodeOf = np.arange(K, dtype=np.int32)
    emit("histogram", _median_ms(lambda: plan.histogram(image, y, None, slot0, nodeOf, K, B),
                                 a.warmup, a.runs), level_floor, nodes=K,
         runs_per_launch=plan.runs_per_launch(B))
    rng = np.random.default_rng(0)
    table = np.stack([rng.integers(0, d, size=K), np.full(K, B // 2 - 1),
                      2 * np.arange(K), 2 * np.arange(K) + 1], axis=1).astype(np.int32)
    slot = slot0.clone()

    def level():
        slot.copy_(slot0)
        plan.histogram(image, y, None, slot, nodeOf, K, B)
        plan.route(image, slot, table)
    emit("level", _median_ms(level, a.warmup, a.runs), level_floor, nodes=K)
    # a balanced tree of 2^depth leaves, breadth first: node i's children are 2 i + 1, 2 i + 2
    L = 1 << a.depth
    m = 2 * L - 1
    first = np.array([2 * i + 1 if 2 * i + 2 < m else -1 for i in range(m)], dtype=np.int32)
    feature = np.where(first >= 0, rng.integers(0, d, size=m), -1).astype(np.int32)
    leaf = np.where(first < 0, np.arange(m) - (L - 1), -1).astype(np.int32)
    thresholds = rng.normal(size=m) * 0.5
    leafPred = rng.normal(size=L)
    leafRaw = rng.uniform(size=(L, C)) if C else None
    emit("predict", _median_ms(lambda: plan.predict(X, feature, thresholds, first, leaf, leafPred),
                               a.warmup, a.runs), rows_floor, levels=a.depth)
    if C:
        emit("predict_probability",
             _median_ms(lambda: plan.predict(X, feature, thresholds, first, leaf, leafPred,
                                             leafRaw, pred=False, prob=True), a.warmup, a.runs),
             rows_floor, levels=a.depth)
    # the kernels' own times, one profiled call each
    N.profile_enable(True)
    for name in KERNELS:
        N.profile_query(name)
    plan.check(X, y, None)
    plan.bin(X, thr)
    level()
    plan.predict(X, feature, thresholds, first, leaf, leafPred)
    torch.cuda.synchronize()
    out = {}
    for name in KERNELS:
        ms, cnt = N.profile_query(name)
        if cnt:
            out[name + "_ms"] = round(ms, 4)
            out[name + "_launches"] = cnt
    print(json.dumps(dict(item="kernels", rows=n, features=d, classes=C, bins=B, **out)),
          flush=True)
    N.profile_enable(False)


if __name__ == "__main__":
    main()
