#!/usr/bin/env python3
"""Times the dense STEP reweight of GeneralizedLinearRegression's IRLS
(cyc_glm_reweight_dev, k_glm_rows) beside one cyc_wls_accumulate_dev call
(k_wls_tiles) on the same rows, in one process: HIP events, the median of
--runs runs after --warmup warm-ups.  One JSON line per shape (also appended
to --out when given), with the share of HBM's achievable rate that the
8 n p bytes of one read of X reach.

    python tools/glm_time.py                       # 4M x 64 and 4M x 510
    python tools/glm_time.py --shape 100000x126 --family binomial
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_ACHIEVABLE = 6.3e12      # bytes / s, streaming reads on an MI355X


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


def time_shape(n, p, family, warmup, runs, device):
    import torch
    from cycloneml_amd.glm import FamilyAndLink, GLMPlan
    from cycloneml_amd.regression import WLSPlan
    g = torch.Generator(device=device).manual_seed(p)
    X = torch.empty((n, p), dtype=torch.float64, device=device)
    step = max(1, (1 << 28) // p)                      # 2 GiB of rows at a time
    for r in range(0, n, step):
        X[r:r + step].normal_(generator=g)
    coef = torch.randn(p, dtype=torch.float64, device=device, generator=g) * (0.5 / p ** 0.5)
    w = torch.rand(n, dtype=torch.float64, device=device, generator=g) + 0.5
    off = torch.rand(n, dtype=torch.float64, device=device, generator=g) * 0.1
    y = torch.rand(n, dtype=torch.float64, device=device, generator=g).round()
    z, wz = torch.empty_like(y), torch.empty_like(y)
    glm, wls = GLMPlan(FamilyAndLink(family, None, 0.0, None), p), WLSPlan(p)
    U = torch.zeros(wls.packedSize, dtype=torch.float64, device=device)
    glm.reweight(X, y, w, off, coef, 0.1, z, wz)       # the first WLS call reads real (z, w')
    res = {"rows": n, "features": p, "family": family,
           "device": torch.cuda.get_device_name(device), "warmup": warmup, "runs": runs}
    for name, fn in (("reweight_ms", lambda: glm.reweight(X, y, w, off, coef, 0.1, z, wz)),
                     ("wls_ms", lambda: wls.accumulate(X, z, wz, U))):
        med, lo, hi = _median_ms(fn, warmup, runs)
        res[name] = round(med, 3)
        res[name + "_range"] = [round(lo, 3), round(hi, 3)]
        # one read of X; the 40 n bytes of y, w, offset, z, w' are not counted
        res[name.replace("_ms", "_hbm_frac")] = round(8.0 * n * p / (med * 1e-3) / HBM_ACHIEVABLE, 3)
    res["reweight_over_wls"] = round(res["reweight_ms"] / res["wls_ms"], 3)
    glm.close()
    wls.close()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--shape", action="append", default=None, help="ROWSxFEATURES (repeatable)")
    ap.add_argument("--family", default="poisson")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("glm_time.py needs a GPU")
    device = torch.device("cuda:0")
    for s in a.shape or ["4000000x64", "4000000x510"]:
        n, p = (int(v) for v in s.lower().split("x"))
        line = json.dumps(time_shape(n, p, a.family, a.warmup, a.runs, device))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
