#!/usr/bin/env python3
"""Times one ALS half-step (cyc_als_solve_dev, csrc/als.hip) on a synthetic
problem of MovieLens-20M's shape: 138,493 users x 26,744 items, 20 M ratings,
users uniform, item degrees Zipf (so the item side has rows of many segments
and the user side rows of one).  Rank 10 and rank 64, explicit and implicit,
both sides.  HIP events around the call (which ends in the read of its info
flag), the median of --runs runs after --warmup warm-ups.  One JSON line per
(rank, feedback, side), with DESIGN.md's model beside the time:

    flop  = nnz rank (rank + 1) + m rank^3 / 3     (+ nsrc rank (rank + 1), implicit)
    bytes = nnz (4 rank + 8) + 4 rank (m + nsrc)
    model = max(flop / 78.6e12, bytes / 8e12)      fp64 MFMA peak, HBM peak

    python tools/als_time.py
    python tools/als_time.py --users 20000 --items 5000 --ratings 1000000 --rank 10
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_FLOPS = 78.6e12      # fp64 MFMA, MI355X
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


def ratings(nu, ni, nnz, device, seed=0):
    """(users, items, ratings): users uniform, items Zipf(1), ratings 0.5 .. 5."""
    import torch
    g = torch.Generator(device=device).manual_seed(seed)
    users = torch.randint(0, nu, (nnz,), device=device, generator=g, dtype=torch.int32)
    p = 1.0 / torch.arange(1, ni + 1, device=device, dtype=torch.float64)
    items = torch.empty(nnz, dtype=torch.int32, device=device)
    step = 1 << 22
    for lo in range(0, nnz, step):
        n = min(step, nnz - lo)
        items[lo:lo + n] = torch.multinomial(p, n, replacement=True, generator=g).to(torch.int32)
    r = torch.randint(1, 11, (nnz,), device=device, generator=g).to(torch.float32) * 0.5
    return users, items, r


def model_ms(nnz, m, nsrc, rank, implicit):
    flop = nnz * rank * (rank + 1) + m * rank ** 3 / 3.0
    if implicit:
        flop += nsrc * rank * (rank + 1)
    nbytes = nnz * (4 * rank + 8) + 4 * rank * (m + nsrc)
    tf, tb = flop / PEAK_FLOPS * 1e3, nbytes / PEAK_BYTES * 1e3
    return max(tf, tb), ("mfma" if tf > tb else "hbm"), flop, nbytes


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--users", type=int, default=138493)
    ap.add_argument("--items", type=int, default=26744)
    ap.add_argument("--ratings", type=int, default=20000263)
    ap.add_argument("--rank", type=int, action="append", default=None)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("als_time.py needs a GPU")
    from cycloneml_amd import recommendation as rec
    device = torch.device("cuda:0")
    users, items, r = ratings(a.users, a.items, a.ratings, device)
    nnz = a.ratings
    for rank in a.rank or [10, 64]:
        plan = rec.ALSPlan(rank)
        sides = {"item": (plan.side(*rec.build_side(items, users, r, a.items), a.items, a.users)),
                 "user": (plan.side(*rec.build_side(users, items, r, a.users), a.users, a.items))}
        for name, side in sides.items():
            counts = side.rowptr[1:] - side.rowptr[:-1]
            Y = torch.randn((side.nsrc, rank), device=device, dtype=torch.float32)
            Y /= Y.norm(dim=1, keepdim=True)
            for implicit in (False, True):
                med, lo, hi = _median_ms(lambda: plan.solve(side, Y, 0.1, implicit, 1.0),
                                         a.warmup, a.runs)
                model, bound, flop, nbytes = model_ms(nnz, side.m, side.nsrc, rank, implicit)
                line = json.dumps({
                    "users": a.users, "items": a.items, "ratings": nnz, "rank": rank,
                    "side": name, "implicit": implicit, "rows": side.m,
                    "longest_row": int(counts.max()),
                    "rows_over_segment": int((counts > plan.segment).sum()),
                    "half_step_ms": round(med, 3), "range_ms": [round(lo, 3), round(hi, 3)],
                    "model_ms": round(model, 3), "model_bound": bound,
                    "fraction_of_model": round(model / med, 3),
                    "tflops": round(flop / (med * 1e-3) / 1e12, 2),
                    "gather_gbps": round(nbytes / (med * 1e-3) / 1e9, 1),
                    "device": torch.cuda.get_device_name(device), "warmup": a.warmup,
                    "runs": a.runs})
                print(line, flush=True)
                if a.out:
                    with open(a.out, "a") as f:
                        f.write(line + "\n")
        for side in sides.values():
            side.close()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
