#!/usr/bin/env python3
"""Times one level of a RandomForest fit (csrc/random_forest.hip) on a synthetic
binned image: --trees trees with --nodes live nodes each, every (tree, row)
pair in one of the tree's nodes, Poisson(1) bags, for m = --subset features per
node (several: --subset 16,10,40) and for m = d, against the baseline a forest
costs without the kernel: the
unchanged cyc_dt_histogram_dev called once per tree over all features on the same
slots (no bag).  Also the forest's predictProbability over balanced trees of
--depth levels.  HIP events around each call, the median (min - max) of --runs
runs after --warmup warm-ups; run it in two separate processes and compare the
medians.  One JSON line per item, with DESIGN.md 5l's floor beside the time:

    histogram  bytes = T n (m + 1 + 4 + 4)   per pair: m image bytes, the bag's
                                             byte, the slot and the key
    baseline   bytes = T n d                 one read of the image per tree
    predict    bytes = 8 n d                 one read of the rows

    python tools/random_forest_time.py
    python tools/random_forest_time.py --rows 1000000 --features 64 --subset 8
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_BYTES = 8.0e12       # HBM3E
KERNELS = ("k_rf_key", "k_rf_runs", "k_rf_hist", "k_rf_fold", "k_rf_route", "k_rf_predict",
           "k_rf_bag", "k_dt_hist", "k_dt_fold")


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
    ap.add_argument("--trees", type=int, default=20)
    ap.add_argument("--nodes", type=int, default=16, help="live nodes per tree")
    ap.add_argument("--subset", default="16", help="features per node (m), or several: 16,10")
    ap.add_argument("--depth", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--skip-predict", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import torch
    from cycloneml_amd import _native as N
    from cycloneml_amd import forest as RF
    from cycloneml_amd import tree as T
    dev = torch.device("cuda:0")
    n, d, C, B, nt, per = a.rows, a.features, a.classes, a.bins, a.trees, a.nodes
    g = torch.Generator(device=dev).manual_seed(0)
    image = torch.randint(0, B, (n, d), device=dev, generator=g, dtype=torch.uint8)
    y = (torch.randint(0, max(C, 2), (n,), device=dev, generator=g).to(torch.float64) if C
         else torch.randn(n, device=dev, generator=g, dtype=torch.float64))
    slot = torch.randint(0, per, (nt, n), device=dev, generator=g).to(torch.int32)
    rf, dt = RF.RFPlan(d, C), T.DTPlan(d, C)
    bag = rf.bag(n, nt, RF.poisson_table(1.0), 0, 0, dev)
    K = nt * per
    slotStart = per * np.arange(nt + 1, dtype=np.int32)
    nodeOf = np.arange(K, dtype=np.int32)
    rng = np.random.default_rng(0)

    def emit(item, ms, floor_ms, **more):
        med, lo, hi = ms
        print(json.dumps(dict(item=item, rows=n, features=d, classes=C, bins=B, trees=nt,
                              median_ms=round(med, 4), min_ms=round(lo, 4), max_ms=round(hi, 4),
                              floor_ms=round(floor_ms, 4), bound="hbm",
                              ratio_to_floor=round(med / floor_ms, 2), **more)), flush=True)

    subsets = [min(int(v), d) for v in str(a.subset).split(",")]
    for m in sorted(set(subsets) | {d}):
        feats = None if m == d else np.stack(
            [np.sort(rng.choice(d, size=m, replace=False)) for _ in range(K)]).astype(np.int32)
        floor = nt * n * (m + 9.0) / PEAK_BYTES * 1e3
        emit(f"histogram_m{m}", _median_ms(
            lambda: rf.histogram(image, y, None, bag, slot, 0, nt, slotStart, nodeOf, K, m, feats, B),
            a.warmup, a.runs), floor, nodes=K, subset=m, sub_runs=rf.sub_runs(m),
            runs_per_launch=rf.runs_per_launch(m, B))
    one = np.arange(per, dtype=np.int32)

    def baseline():
        for t in range(nt):
            dt.histogram(image, y, None, slot[t], one, per, B)
    emit("baseline_tree_histograms", _median_ms(baseline, a.warmup, a.runs),
         nt * n * float(d) / PEAK_BYTES * 1e3, nodes=K)
    table = np.stack([rng.integers(0, d, size=K), np.full(K, B // 2 - 1),
                      np.tile(np.arange(per), nt), np.tile(np.arange(per), nt)],
                     axis=1).astype(np.int32)
    emit("route", _median_ms(lambda: rf.route(image, slot, slotStart, table), a.warmup, a.runs),
         nt * n * 9.0 / PEAK_BYTES * 1e3, nodes=K)
    # the kernels' own times, one profiled call each
    N.profile_enable(True)
    for name in KERNELS:
        N.profile_query(name)
    m = subsets[0]
    feats = None if m == d else np.stack(
        [np.sort(rng.choice(d, size=m, replace=False)) for _ in range(K)]).astype(np.int32)
    rf.histogram(image, y, None, bag, slot, 0, nt, slotStart, nodeOf, K, m, feats, B)
    dt.histogram(image, y, None, slot[0], one, per, B)
    torch.cuda.synchronize()
    out = {}
    for name in KERNELS:
        ms, cnt = N.profile_query(name)
        if cnt:
            out[name + "_ms"] = round(ms, 4)
            out[name + "_launches"] = cnt
    print(json.dumps(dict(item="kernels", rows=n, features=d, subset=m, **out)), flush=True)
    N.profile_enable(False)
    if a.skip_predict or not C:
        return
    del image, slot, bag
    torch.cuda.empty_cache()
    X = torch.randn((n, d), device=dev, generator=g, dtype=torch.float64)
    # balanced trees of 2^depth leaves, breadth first: node i's children are 2 i + 1, 2 i + 2
    L = 1 << a.depth
    nn = 2 * L - 1
    first = np.array([2 * i + 1 if 2 * i + 2 < nn else -1 for i in range(nn)], dtype=np.int32)
    trees = []
    for _ in range(nt):
        feature = np.where(first >= 0, rng.integers(0, d, size=nn), -1)
        trees.append(T.DecisionTreeClassificationModel.from_arrays(
            feature, rng.normal(size=nn) * 0.5, first, rng.uniform(size=(nn, C)), d, numClasses=C))
    model = RF.RandomForestClassificationModel.from_trees(trees, d, C)
    emit("predict_probability", _median_ms(lambda: model.predictProbability(X), a.warmup, a.runs),
         8.0 * n * d / PEAK_BYTES * 1e3, levels=a.depth)


if __name__ == "__main__":
    main()
