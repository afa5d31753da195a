#!/usr/bin/env python3
"""Times cyc_wls_accumulate_dev (the weighted augmented syrk of width p + 2
behind LinearRegression's normal-equation fit) beside
cyc_gramian_accumulate_dev at the same rows and width p, in one process:
HIP events, the median of --runs runs after --warmup warm-ups.  One JSON
line per shape (also appended to --out when given).

    python tools/wls_time.py                       # 4M x 1024 and 30M x 126
    python tools/wls_time.py --shape 100000x126    # anything else
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


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


def time_shape(n, p, warmup, runs, device):
    import torch
    from cycloneml_amd.linalg import GramianPlan
    from cycloneml_amd.regression import WLSPlan
    g = torch.Generator(device=device).manual_seed(p)
    X = torch.empty((n, p), dtype=torch.float64, device=device)
    step = max(1, (1 << 28) // p)                      # 2 GiB of rows at a time
    for r in range(0, n, step):
        X[r:r + step].normal_(generator=g)
    y = torch.randn(n, dtype=torch.float64, device=device, generator=g)
    w = torch.rand(n, dtype=torch.float64, device=device, generator=g) + 0.5
    wls, gram = WLSPlan(p), GramianPlan(p)
    Uw = torch.zeros(wls.packedSize, dtype=torch.float64, device=device)
    Ug = torch.zeros(p * (p + 1) // 2, dtype=torch.float64, device=device)
    res = {"rows": n, "features": p, "device": torch.cuda.get_device_name(device),
           "warmup": warmup, "runs": runs}
    for name, fn in (("wls_ms", lambda: wls.accumulate(X, y, w, Uw)),
                     ("wls_unit_weights_ms", lambda: wls.accumulate(X, y, None, Uw)),
                     ("gramian_ms", lambda: gram.accumulate(X, Ug))):
        med, lo, hi = _median_ms(fn, warmup, runs)
        res[name] = round(med, 3)
        res[name + "_range"] = [round(lo, 3), round(hi, 3)]
    res["wls_splits"] = wls.last_splits()
    res["ratio"] = round(res["wls_ms"] / res["gramian_ms"], 3)
    # the syrk's useful work: n q (q + 1) flops over the upper triangle
    q = p + 2
    res["wls_tflops"] = round(n * q * (q + 1) / (res["wls_ms"] * 1e-3) / 1e12, 2)
    res["wls_read_gbps"] = round(n * (p + 2) * 8 / (res["wls_ms"] * 1e-3) / 1e9, 1)
    wls.close()
    gram.close()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--shape", action="append", default=None, help="ROWSxFEATURES (repeatable)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("wls_time.py needs a GPU")
    shapes = a.shape or ["4000000x1024", "30000000x126"]
    device = torch.device("cuda:0")
    for s in shapes:
        n, p = (int(v) for v in s.lower().split("x"))
        line = json.dumps(time_shape(n, p, a.warmup, a.runs, device))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
