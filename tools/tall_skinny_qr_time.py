#!/usr/bin/env python3
"""Times RowMatrix.tallSkinnyQR's device steps (csrc/tsqr.hip) on synthetic
rows: `factor` (runs, fold and copy: cyc_tsqr_factor_dev) at each --shape, the
plain Gramian syrk of the same rows in the same process, and computeQ's
multiply by an n x n matrix.  HIP events around each call, the median and
min - max of --runs runs after --warmup warm-ups.  One JSON line per item,
with DESIGN.md 5p's floor beside the time:

    factor    flop = 2 m n^2 at the fp64 MFMA rate, bytes = 8 m n
    syrk      flop = m n^2 (the triangle's share of 2 m n^2)
    multiply  flop = 2 m n^2, bytes = 16 m n

The kernels' own times come from cyc_profile_query.

    python tools/tall_skinny_qr_time.py
    python tools/tall_skinny_qr_time.py --shape 1000000x64
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_FLOPS = 78.6e12      # fp64 MFMA
PEAK_BYTES = 8.0e12       # HBM3E
KERNELS = ("k_tsqr_run", "k_tsqr_fold", "k_gram_dma", "k_rmm_dense")


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
    ap.add_argument("--shape", action="append", help="MxN; default 30000000x256 and 4000000x1024")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    import torch
    from cycloneml_amd import _native as N
    from cycloneml_amd.linalg import GramianPlan, RowMatrix, TSQRPlan
    dev = torch.device("cuda:0")
    for shape in a.shape or ["30000000x256", "4000000x1024"]:
        m, n = (int(v) for v in shape.split("x"))
        g = torch.Generator(device=dev).manual_seed(0)
        X = torch.randn((m, n), device=dev, generator=g, dtype=torch.float64)

        def emit(item, ms, flop, nbytes, **more):
            med, lo, hi = ms
            floor = max(flop / PEAK_FLOPS, nbytes / PEAK_BYTES) * 1e3
            print(json.dumps(dict(item=item, rows=m, cols=n, median_ms=round(med, 3),
                                  min_ms=round(lo, 3), max_ms=round(hi, 3),
                                  floor_ms=round(floor, 3),
                                  bound="mfma" if flop / PEAK_FLOPS > nbytes / PEAK_BYTES
                                  else "hbm", ratio_to_floor=round(med / floor, 2), **more)),
                  flush=True)

        plan = TSQRPlan(n)
        factor = _median_ms(lambda: plan.factor(X), a.warmup, a.runs)
        emit("factor", factor, 2.0 * m * n * n, 8.0 * m * n,
             runs_of_rows=-(-m // N.load().cyc_tsqr_run_rows()),
             tile_rows=N.load().cyc_tsqr_tile_rows(n))
        gram = GramianPlan(n)
        U = torch.zeros(n * (n + 1) // 2, dtype=torch.float64, device=dev)
        syrk = _median_ms(lambda: gram.accumulate(X, U), a.warmup, a.runs)
        emit("syrk", syrk, 1.0 * m * n * n, 8.0 * m * n,
             factor_over_syrk=round(factor[0] / syrk[0], 2))
        B = torch.eye(n, dtype=torch.float64, device=dev)
        A = RowMatrix(X, m, n)
        emit("multiply", _median_ms(lambda: A.multiply(B), a.warmup, a.runs),
             2.0 * m * n * n, 16.0 * m * n)
        # the kernels' own times, one profiled call each
        N.profile_enable(True)
        for name in KERNELS:
            N.profile_query(name)
        plan.factor(X)
        gram.accumulate(X, U)
        A.multiply(B)
        torch.cuda.synchronize()
        out = {}
        for name in KERNELS:
            ms, cnt = N.profile_query(name)
            if cnt:
                out[name + "_ms"] = round(ms, 3)
                out[name + "_launches"] = cnt
        print(json.dumps(dict(item="kernels", rows=m, cols=n, **out)), flush=True)
        N.profile_enable(False)
        plan.close()
        gram.close()
        del X, A, B, U
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
