#!/usr/bin/env python3
"""Times the evaluate pass of linear models (cyc_linreg_stats_dev,
k_linreg_rows) beside cyc_glm_stats_dev (k_glm_stats, gaussian / identity) on
the same rows, and one l-bfgs cost evaluation of LinearRegression
(LeastSquaresBlockAggregator add + all-reduce + the host's copies) beside one
cyc_wls_accumulate_dev call (k_wls_tiles), in one process: HIP events, the
median of --runs runs after --warmup warm-ups.  One JSON line per shape (also
appended to --out when given), with the share of HBM's achievable rate that
the 8 n p bytes of one read of X reach (CSR: the 12 bytes per nonzero).

    python tools/linreg_time.py                  # 4M x 64, 4M x 510, CSR 1M x 1M / 64
    python tools/linreg_time.py --shape 100000x126
    python tools/linreg_time.py --csr 200000x1000000x64
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


def _record(res, name, fn, nbytes, warmup, runs):
    med, lo, hi = _median_ms(fn, warmup, runs)
    res[name + "_ms"] = round(med, 3)
    res[name + "_range"] = [round(lo, 3), round(hi, 3)]
    res[name + "_hbm_frac"] = round(nbytes / (med * 1e-3) / HBM_ACHIEVABLE, 3)


def time_dense(n, p, warmup, runs, device):
    import numpy as np
    import torch
    from cycloneml_amd import optim
    from cycloneml_amd.glm import FamilyAndLink, GLMPlan
    from cycloneml_amd.regression import BlockCost, WLSPlan
    from cycloneml_amd.regression_summary import linreg_stats
    g = torch.Generator(device=device).manual_seed(p)
    X = torch.empty((n, p), dtype=torch.float64, device=device)
    step = max(1, (1 << 28) // p)                      # 2 GiB of rows at a time
    for r in range(0, n, step):
        X[r:r + step].normal_(generator=g)
    coef = torch.randn(p, dtype=torch.float64, device=device, generator=g) * (0.5 / p ** 0.5)
    w = torch.rand(n, dtype=torch.float64, device=device, generator=g) + 0.5
    y = torch.randn(n, dtype=torch.float64, device=device, generator=g)
    res = {"rows": n, "features": p, "layout": "dense",
           "device": torch.cuda.get_device_name(device), "warmup": warmup, "runs": runs}
    nbytes = 8.0 * n * p      # one read of X; the 16 n bytes of y and w are not counted
    _record(res, "linreg_stats", lambda: linreg_stats(X, y, w, coef, 0.1, 0.0), nbytes, warmup,
            runs)
    _record(res, "linreg_stats_pred",
            lambda: linreg_stats(X, y, w, coef, 0.1, 0.0, want_pred=True), nbytes, warmup, runs)
    glm = GLMPlan(FamilyAndLink("gaussian", None, 0.0, None), p)
    sums = torch.empty(6, dtype=torch.float64, device=device)
    _record(res, "glm_stats", lambda: glm.stats(X, y, w, None, coef, 0.1, sums), nbytes, warmup,
            runs)
    glm.close()
    res["linreg_over_glm_stats"] = round(res["linreg_stats_ms"] / res["glm_stats_ms"], 3)
    # one cost evaluation as the l-bfgs fit runs it, host copies included
    block = optim.DeviceInstanceBlock(y, w, X=X)
    ones, mean = np.ones(p), np.zeros(p)
    cost = BlockCost(block, lambda raw: optim.LeastSquaresBlockAggregator(
        ones, mean, True, 1.0, 0.0, raw, device=device), ones)
    x = coef.cpu().numpy()
    _record(res, "lbfgs_eval", lambda: cost(x), nbytes, warmup, runs)
    wls = WLSPlan(p)
    U = torch.zeros(wls.packedSize, dtype=torch.float64, device=device)
    _record(res, "wls", lambda: wls.accumulate(X, y, w, U), nbytes, warmup, runs)
    wls.close()
    res["lbfgs_eval_over_wls"] = round(res["lbfgs_eval_ms"] / res["wls_ms"], 3)
    return res


def time_csr(n, p, nnz, warmup, runs, device):
    import torch
    from cycloneml_amd.glm import FamilyAndLink, GLMPlan
    from cycloneml_amd.linalg import CSRRows
    from cycloneml_amd.regression_summary import linreg_stats
    g = torch.Generator(device=device).manual_seed(p)
    # one index in each of nnz equal column ranges: increasing and distinct per row
    span = p // nnz
    colidx = torch.randint(0, span, (n, nnz), device=device, generator=g, dtype=torch.int32)
    colidx += torch.arange(nnz, device=device, dtype=torch.int32) * span
    colidx = colidx.reshape(-1).contiguous()
    vals = torch.randn(n * nnz, dtype=torch.float64, device=device, generator=g)
    rowptr = torch.arange(n + 1, dtype=torch.int64, device=device) * nnz
    rows = CSRRows(rowptr, colidx, vals, p)
    coef = torch.randn(p, dtype=torch.float64, device=device, generator=g)
    w = torch.rand(n, dtype=torch.float64, device=device, generator=g) + 0.5
    y = torch.randn(n, dtype=torch.float64, device=device, generator=g)
    res = {"rows": n, "features": p, "nnz_per_row": nnz, "layout": "csr",
           "device": torch.cuda.get_device_name(device), "warmup": warmup, "runs": runs}
    nbytes = 12.0 * n * nnz
    _record(res, "linreg_stats", lambda: linreg_stats(rows, y, w, coef, 0.1, 0.0), nbytes, warmup,
            runs)
    if p <= 4096:          # k_glm_stats stages the coefficients in LDS: 4096 features at most
        glm = GLMPlan(FamilyAndLink("gaussian", None, 0.0, None), p)
        sums = torch.empty(6, dtype=torch.float64, device=device)
        _record(res, "glm_stats", lambda: glm.stats(rows, y, w, None, coef, 0.1, sums), nbytes,
                warmup, runs)
        glm.close()
        res["linreg_over_glm_stats"] = round(res["linreg_stats_ms"] / res["glm_stats_ms"], 3)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--shape", action="append", default=None, help="ROWSxFEATURES (repeatable)")
    ap.add_argument("--csr", action="append", default=None,
                    help="ROWSxFEATURESxNNZ_PER_ROW (repeatable)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("linreg_time.py needs a GPU")
    device = torch.device("cuda:0")
    dense, csr = a.shape, a.csr
    if dense is None and csr is None:
        dense = ["4000000x64", "4000000x510"]
        csr = ["1000000x1000000x64", "1000000x4096x64"]
    jobs = [(time_dense, s) for s in dense or []] + [(time_csr, s) for s in csr or []]
    for fn, s in jobs:
        dims = [int(v) for v in s.lower().split("x")]
        line = json.dumps(fn(*dims, a.warmup, a.runs, device))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
