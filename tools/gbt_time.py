#!/usr/bin/env python3
"""Times the two GBT kernels (csrc/gbt.hip) on synthetic rows, by default 10 M x
256 and a balanced tree of --depth 5 levels:

  update        cyc_gbt_update_dev over the uint8 image (squared loss, weights,
                residuals written), against its HBM floor and against
  composition   what the package offered before the kernel: DTPlan.predict over
                the fp64 rows, then torch elementwise ops for pred, the residual
                and the error, and two torch.sum (whose order is not fixed);
  update_rows   cyc_gbt_update_dev over the fp64 rows (evaluateEachIteration's form);
  predict       cyc_gbt_predict_dev (margin, raw and probability) for --trees 20
                trees against its floor.

HIP events around each call, the median (min - max) of --runs runs after --warmup
warm-ups.  One JSON line per item, with DESIGN.md 5m's floors beside the time:

    update       bytes = n (40 + depth)        pred in and out, y, w, resid, and one
                                               image byte per level of the path
                 lines = n (40 + 128 min(depth, ceil(d / 128)))   the same with the
                                               image fetched in 128-byte lines
    update_rows  lines = n (40 + 128 min(depth, ceil(8 d / 128)))
    predict      bytes = n (8 d + 48)          one read of the rows; margin, raw, prob

No threshold is asserted here.

    python tools/gbt_time.py
    python tools/gbt_time.py --rows 1000000 --features 64
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_BYTES = 8.0e12       # HBM3E
KERNELS = ("k_gbt_update", "k_gbt_fold", "k_gbt_predict", "k_dt_predict")


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
    ap.add_argument("--bins", type=int, default=32)
    ap.add_argument("--depth", type=int, default=5)
    ap.add_argument("--trees", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=7)
    a = ap.parse_args()
    import numpy as np
    import torch
    from cycloneml_amd import _native as N
    from cycloneml_amd import gbt as GB
    from cycloneml_amd import tree as T
    dev = torch.device("cuda:0")
    n, d, B, depth, nt = a.rows, a.features, a.bins, a.depth, a.trees
    g = torch.Generator(device=dev).manual_seed(0)
    rng = np.random.default_rng(0)
    X = torch.randn((n, d), device=dev, generator=g, dtype=torch.float64)
    y = torch.randn(n, device=dev, generator=g, dtype=torch.float64)
    w = torch.rand(n, device=dev, generator=g, dtype=torch.float64) + 0.5
    pred = torch.zeros(n, device=dev, dtype=torch.float64)
    resid = torch.empty_like(pred)
    # the image of the rows under B - 1 thresholds per feature
    grid = np.linspace(-1.5, 1.5, B - 1)
    thresholds = [grid] * d
    dt = T.DTPlan(d, 0)
    image = dt.bin(X, thresholds)
    # a balanced tree of 2^depth leaves, breadth first: node i's children are 2 i + 1, 2 i + 2
    nn = 2 * (1 << depth) - 1

    def balanced():
        first = np.array([2 * i + 1 if 2 * i + 2 < nn else -1 for i in range(nn)], dtype=np.int32)
        feature = np.where(first >= 0, rng.integers(0, d, size=nn), -1)
        split = np.where(first >= 0, rng.integers(B // 4, 3 * B // 4, size=nn), -1)
        thr = np.where(first >= 0, grid[np.maximum(split, 0)], 0.0)
        return T.DecisionTreeRegressionModel.from_arrays(feature, thr, first,
                                                         list(rng.normal(size=nn)), d)

    tree = balanced()
    flat = GB.flat_tree(tree.rootNode, thresholds)
    plan = GB.GBTPlan(d)
    sums = torch.empty(2, device=dev, dtype=torch.float64)

    def emit(item, ms, floor_ms, **more):
        med, lo, hi = ms
        print(json.dumps(dict(item=item, rows=n, features=d, depth=depth,
                              median_ms=round(med, 4), min_ms=round(lo, 4), max_ms=round(hi, 4),
                              floor_ms=round(floor_ms, 4), bound="hbm",
                              ratio_to_floor=round(med / floor_ms, 2), **more)), flush=True)

    def lines(rowBytes):
        return n * (40.0 + 128.0 * min(depth, -(-rowBytes // 128))) / PEAK_BYTES * 1e3

    byte_floor = n * (40.0 + depth) / PEAK_BYTES * 1e3
    emit("update", _median_ms(
        lambda: plan.update(image, flat, 0.1, "squared", y, w, pred, resid, sums),
        a.warmup, a.runs), byte_floor, line_floor_ms=round(lines(d), 4))
    got = (pred.clone(), resid.clone(), sums.clone())

    def composition():
        leaf = dt.predict(X, tree._feature, tree._threshold, tree._first, tree._leaf,
                          tree._leafPred)[1]
        pred.add_(leaf * 0.1)
        diff = y - pred
        torch.mul(diff, 2.0, out=resid)
        e = diff * diff
        return torch.sum(e * w), torch.sum(w)

    emit("composition", _median_ms(composition, a.warmup, a.runs), byte_floor,
         line_floor_ms=round(lines(8 * d), 4))
    flat_rows = GB.flat_model_tree(tree)
    emit("update_rows", _median_ms(
        lambda: plan.update(X, flat_rows, 0.1, "squared", y, w, pred, resid, sums),
        a.warmup, a.runs), lines(8 * d))
    # the two forms agree on one call from the same start
    pred.zero_()
    plan.update(image, flat, 0.1, "squared", y, w, pred, resid, sums)
    a1 = (pred.clone(), resid.clone(), sums.clone())
    pred.zero_()
    plan.update(X, flat_rows, 0.1, "squared", y, w, pred, resid, sums)
    same = all(torch.equal(p, q) for p, q in zip(a1, (pred, resid, sums)))
    print(json.dumps(dict(item="forms_agree", same_bytes=bool(same))), flush=True)
    del got, image
    model = GB.GBTClassificationModel.from_trees([balanced() for _ in range(nt)],
                                                 [1.0] + [0.1] * (nt - 1), d)

    def predict():
        return model._run(X, margin=True, raw=True, prob=True)

    emit("predict", _median_ms(predict, a.warmup, a.runs),
         n * (8.0 * d + 48.0) / PEAK_BYTES * 1e3, trees=nt)
    # the kernels' own times, one profiled call each
    N.profile_enable(True)
    for name in KERNELS:
        N.profile_query(name)
    image = dt.bin(X, thresholds)
    plan.update(image, flat, 0.1, "squared", y, w, pred, resid, sums)
    dt.predict(X, tree._feature, tree._threshold, tree._first, tree._leaf, tree._leafPred)
    predict()
    torch.cuda.synchronize()
    out = {}
    for name in KERNELS:
        ms, cnt = N.profile_query(name)
        if cnt:
            out[name + "_ms"] = round(ms, 4)
            out[name + "_launches"] = cnt
    print(json.dumps(dict(item="kernels", rows=n, features=d, **out)), flush=True)
    N.profile_enable(False)


if __name__ == "__main__":
    main()
