#!/usr/bin/env python3
"""Times ALS top-N (cyc_als_recommend_dev, csrc/als_recommend.hip) at
MovieLens-20M's shape, the shape of tools/als_time.py: 138,493 users x 26,744
items, unit-norm random factors, every id present.  Ranks 10 and 64, num = 10,
both directions (per user its items, per item its users).  HIP events around
ALSPlan.recommend (its output and workspace allocations from torch's caching
allocator included), the median of --runs runs after --warmup warm-ups.  One
JSON line per (rank, direction), with DESIGN.md 5h's floor beside the time:

    lane-ops = m n 2 rank         one multiply and one add per factor, unfused
    floor    = lane-ops / 78.6e12 (157.3 TF fp32 vector peak = 78.6 T lane-FMA/s)

and, for comparison only, the plain alternative: torch.matmul over row chunks
of the sources followed by torch.topk.  Its scores are rocBLAS's, not the
reference's chain: it is NOT bit-equal to the reference and breaks ties its own
way; `agree` is the fraction of its ids that equal the kernel's.

    python tools/als_recommend_time.py
    python tools/als_recommend_time.py --users 20000 --items 5000 --rank 10
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_LANE_OPS = 78.6e12       # fp32 VALU lane-operations per second, MI355X
CHUNK_ELEMS = 1 << 28         # scores per matmul chunk of the torch alternative (1 GiB)


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


def torch_topk(S, D, num):
    import torch
    rows = max(1, CHUNK_ELEMS // D.shape[0])
    ids = torch.empty((S.shape[0], num), dtype=torch.int64, device=S.device)
    scores = torch.empty((S.shape[0], num), dtype=torch.float32, device=S.device)
    Dt = D.t()
    for lo in range(0, S.shape[0], rows):
        sc, ix = torch.topk(torch.matmul(S[lo:lo + rows], Dt), num, dim=1)
        ids[lo:lo + rows], scores[lo:lo + rows] = ix, sc
    return ids, scores


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--users", type=int, default=138493)
    ap.add_argument("--items", type=int, default=26744)
    ap.add_argument("--rank", type=int, action="append", default=None)
    ap.add_argument("--num", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("als_recommend_time.py needs a GPU")
    from cycloneml_amd import recommendation as rec
    device = torch.device("cuda:0")
    g = torch.Generator(device=device).manual_seed(0)
    for rank in a.rank or [10, 64]:
        plan = rec.ALSPlan(rank)
        F = {}
        for name, n in (("user", a.users), ("item", a.items)):
            Y = torch.randn((n, rank), device=device, dtype=torch.float32, generator=g)
            F[name] = (Y / Y.norm(dim=1, keepdim=True)).contiguous()
        for src, dst in (("user", "item"), ("item", "user")):
            S, D = F[src], F[dst]
            m, n = S.shape[0], D.shape[0]
            med, lo, hi = _median_ms(lambda: plan.recommend(S, None, D, None, a.num),
                                     a.warmup, a.runs)
            tmed, tlo, thi = _median_ms(lambda: torch_topk(S, D, a.num), a.warmup, a.runs)
            ids = plan.recommend(S, None, D, None, a.num)[0]
            agree = float((torch_topk(S, D, a.num)[0] == ids).float().mean())
            floor = m * n * 2.0 * rank / PEAK_LANE_OPS * 1e3
            line = json.dumps({
                "users": a.users, "items": a.items, "rank": rank, "num": a.num,
                "sources": src, "rows": m, "destinations": n,
                "splits": plan.recommend_splits(m, n), "span": plan.recommend_span(m, n),
                "workspace_mb": round(plan.recommend_workspace(m, n, a.num) / 1e6, 1),
                "recommend_ms": round(med, 3), "range_ms": [round(lo, 3), round(hi, 3)],
                "floor_ms": round(floor, 3), "fraction_of_floor": round(floor / med, 3),
                "torch_matmul_topk_ms": round(tmed, 3),
                "torch_range_ms": [round(tlo, 3), round(thi, 3)],
                "torch_over_kernel": round(tmed / med, 3), "agree": round(agree, 6),
                "device": torch.cuda.get_device_name(device), "warmup": a.warmup,
                "runs": a.runs})
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(line + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
