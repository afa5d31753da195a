#!/usr/bin/env python3
"""Times one inner iteration of BisectingKMeans (the assign step with its
summary, csrc/bisecting_kmeans.hip) and the model's predict on synthetic rows:
k / 2 clusters that each divide in two, every row active, and a balanced tree of
k leaves.  HIP events around each call, the median of --runs runs after
--warmup warm-ups.  One JSON line per item, with DESIGN.md 5j's floor beside
the time:

    assign     bytes = n (8 d + 8 + 4 + 4)         HBM, 8 TB/s
    iteration  bytes = n (16 d + 8 + 4 + 4 + 28)   the summary reads the rows again
    predict    bytes = n (8 d + 4)                 one read of the rows

and the same pick of two centers in torch (cdist of a chunk of rows against all
the children, a gather of each row's two, the comparison).  The kernels' own
times come from cyc_profile_query.

    python tools/bisecting_kmeans_time.py
    python tools/bisecting_kmeans_time.py --rows 1000000 --features 64 --k 8
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_BYTES = 8.0e12       # HBM3E
KERNELS = ("k_bkm_assign", "k_bkm_chunk", "k_bkm_fold", "k_bkm_predict")


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
    ap.add_argument("--k", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    import numpy as np
    import torch
    from cycloneml_amd import _native as N
    from cycloneml_amd import bisecting_kmeans as bk
    from cycloneml_amd.clustering import row_norms
    dev = torch.device("cuda:0")
    n, d, K = a.rows, a.features, a.k
    S = K // 2
    g = torch.Generator(device=dev).manual_seed(0)
    X = torch.randn((n, d), device=dev, generator=g, dtype=torch.float64)
    slot = torch.randint(0, S, (n,), device=dev, generator=g).to(torch.int32)
    C = torch.randn((K, d), device=dev, generator=g, dtype=torch.float64)
    xn, cn = row_norms(X), row_norms(C)
    table = np.array([[2 * s, 2 * s + 1, -1] for s in range(S)], dtype=np.int32)
    new = torch.empty(n, dtype=torch.int32, device=dev)
    count = torch.zeros(K, dtype=torch.int64, device=dev)
    sums = torch.zeros(bk.sums_length(K, d), dtype=torch.float64, device=dev)
    plan = bk.BKMPlan(d)

    def emit(item, ms, floor_ms, **more):
        med, lo, hi = ms
        print(json.dumps(dict(item=item, rows=n, features=d, k=K, median_ms=round(med, 4),
                              min_ms=round(lo, 4), max_ms=round(hi, 4),
                              floor_ms=round(floor_ms, 4), bound="hbm",
                              ratio_to_floor=round(med / floor_ms, 2), **more)), flush=True)

    def kernels(calls):
        out = {}
        for name in KERNELS:
            ms, cnt = N.profile_query(name)
            if cnt:
                out[name + "_ms"] = round(ms / calls, 4)
        return out

    assign_floor = n * (8 * d + 16) / PEAK_BYTES * 1e3
    iter_floor = n * (16 * d + 44) / PEAK_BYTES * 1e3
    predict_floor = n * (8 * d + 4) / PEAK_BYTES * 1e3
    emit("assign", _median_ms(lambda: plan.step(X, xn, None, slot, table, C, cn, new), a.warmup,
                              a.runs), assign_floor)
    emit("iteration", _median_ms(lambda: plan.step(X, xn, None, slot, table, C, cn, new, count,
                                                   sums), a.warmup, a.runs), iter_floor)
    # a balanced tree of K leaves, breadth first: node i's children are 2 i + 1, 2 i + 2
    m = 2 * K - 1
    first = [2 * i + 1 if 2 * i + 2 < m else -1 for i in range(m)]
    num = [2 if 2 * i + 2 < m else 0 for i in range(m)]
    leaf = [i - (K - 1) if num[i] == 0 else -1 for i in range(m)]
    T = torch.randn((m, d), device=dev, generator=g, dtype=torch.float64)
    emit("predict", _median_ms(lambda: plan.predict(X, first, num, leaf, T, cost=False),
                               a.warmup, a.runs), predict_floor,
         levels=int(np.log2(K)))
    # the kernels' own times, one profiled call each
    N.profile_enable(True)
    for name in KERNELS:
        N.profile_query(name)
    plan.step(X, xn, None, slot, table, C, cn, new, count, sums)
    plan.predict(X, first, num, leaf, T, cost=False)
    torch.cuda.synchronize()
    print(json.dumps(dict(item="kernels", rows=n, features=d, k=K, **kernels(1))), flush=True)
    N.profile_enable(False)

    chunk = 1 << 20
    sl = slot.to(torch.int64)

    def torch_pick():
        for r0 in range(0, n, chunk):
            D = torch.cdist(X[r0:r0 + chunk], C)
            s = sl[r0:r0 + chunk]
            dl = D.gather(1, (2 * s)[:, None])
            dr = D.gather(1, (2 * s + 1)[:, None])
            new[r0:r0 + chunk] = (2 * s + (dr < dl)[:, 0]).to(torch.int32)
    emit("torch_cdist_pick", _median_ms(torch_pick, 1, 3), assign_floor)


if __name__ == "__main__":
    main()
