"""Time one FM evaluation (cyc_fm_evaluate_dev) on the device against the HBM
floor and the torch composition X @ V, (X * X) @ (V * V), X.T @ [m o S | m].

    python tools/fm_time.py [--shapes 10000000x256,2000000x1024] [--factors 8,32]
                            [--reps 5] [--out bench_out/fm_time.jsonl]

Per (shape, k): device-event times of `reps` evaluations after a warm-up of
each path (median and spread), the floor 8 n d bytes (fused; twice that in the
two-pass form) over the HBM peak, and the same for the torch composition.  The
data is seeded on the device.  No GPU: an error, not a fallback.

    python tools/fm_time.py --csr 1048576x1048576 --nnz 64 --factors 8 --reps 20

times cyc_fmcsr_evaluate_dev over prepared CSR rows instead: against the gather
floor (csr_floor_bytes over the HBM peak) and against the same evaluation as
torch sparse-CSR products (csr_composed), with the kernels' own times from the
library's profile hook in a separate pass."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12      # bytes / s, MI355X


def timed(fn, reps):
    import torch
    fn()                                        # warm-up: code objects, workspaces
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e-3)
    return out


def csr_rows(n, d, nnz, dev, seed=1):
    """n rows of nnz non-zeros: non-zero s of a row falls uniformly in stratum
    s of d / nnz columns, so a row's columns are distinct and ascending."""
    import torch
    g = torch.Generator(device=dev).manual_seed(seed)
    width = d // nnz
    col = torch.randint(0, width, (n, nnz), device=dev, generator=g) \
        + torch.arange(nnz, device=dev) * width
    val = torch.randn(n * nnz, dtype=torch.float64, device=dev, generator=g)
    rowptr = torch.arange(n + 1, device=dev, dtype=torch.int64) * nnz
    y = torch.randn(n, dtype=torch.float64, device=dev, generator=g)
    return rowptr, col.reshape(-1).to(torch.int32), val, y


def csr_composed(rowptr, colidx, val, n, d):
    """The evaluation as torch sparse-CSR products: X @ [V | w], (X o X) @ (V o
    V), X^T @ [m o S | m] and (X o X)^T @ m; the transposes are made once, like
    the kernels' column copy."""
    import torch
    if int(rowptr[-1]) < 2 ** 31:               # one index type, the narrow one where it fits
        rowptr = rowptr.to(torch.int32)
    else:
        colidx = colidx.to(torch.int64)
    X = torch.sparse_csr_tensor(rowptr, colidx, val, (n, d))
    X2 = torch.sparse_csr_tensor(rowptr, colidx, val * val, (n, d))
    XT, X2T = X.t().to_sparse_csr(), X2.t().to_sparse_csr()

    def composed(V, w, b, y):
        k = V.shape[1]
        SW = X @ torch.cat([V, w[:, None]], 1)
        S = SW[:, :k]
        raw = b + SW[:, k] + 0.5 * (S * S - X2 @ (V * V)).sum(1)
        m = 2.0 * (raw - y)
        PW = XT @ torch.cat([m[:, None] * S, m[:, None]], 1)
        gV = PW[:, :k] - V * (X2T @ m[:, None])
        return gV, PW[:, k], m.sum(), ((raw - y) ** 2).sum()

    return composed


def csr_floor_bytes(n, nnz_total, k, coef_len):
    """What the two passes must move: per non-zero its (index, value) pair and
    the k + 1 gathered doubles, in each pass; the write of M; the write of out."""
    return 2 * nnz_total * (12 + 8 * (k + 1)) + 8 * n * (k + 1) + 8 * (coef_len + 2)


def csr_mode(a, dev):
    import torch
    from cycloneml_amd import _native as N
    from cycloneml_amd import fm
    from cycloneml_amd.linalg import CSRRows
    n, d = (int(v) for v in a.csr.split("x"))
    rowptr, colidx, val, y = csr_rows(n, d, a.nnz, dev)
    rows = fm.FMSparseRows(CSRRows(rowptr, colidx, val, d))
    lines = []
    for k in (int(v) for v in a.factors.split(",")):
        plan = fm.FMPlan(d, k)
        g = torch.Generator(device=dev).manual_seed(2)
        coef = torch.randn(plan.coefLen, dtype=torch.float64, device=dev, generator=g) * 0.01
        out = torch.empty(plan.coefLen + 2, dtype=torch.float64, device=dev)
        V, w, b = coef[:d * k].view(d, k), coef[d * k:d * k + d], coef[-1]
        ours = timed(lambda: plan.evaluate(rows, y, coef, out), a.reps)
        floor = csr_floor_bytes(n, n * a.nnz, k, plan.coefLen) / HBM_PEAK
        line = {"layout": "csr", "n": n, "d": d, "nnz_per_row": a.nnz, "k": k,
                "segment_entries": rows.segmentEntries,
                "evaluate_s_median": statistics.median(ours), "evaluate_s_min": min(ours),
                "evaluate_s_max": max(ours), "gather_floor_s": floor,
                "floor_over_evaluate": floor / statistics.median(ours)}
        N.profile_enable(True)                  # the kernels' split, in a pass of its own
        for name in KERNELS:
            N.profile_query(name)
        for _ in range(a.reps):
            plan.evaluate(rows, y, coef, out)
        torch.cuda.synchronize()
        for name in KERNELS:
            ms, cnt = N.profile_query(name)
            line[name + "_s"] = ms * 1e-3 / max(cnt, 1)
        N.profile_enable(False)
        try:
            composed = csr_composed(rowptr, colidx, val, n, d)
            ref = timed(lambda: composed(V, w, b, y), a.reps)
            gV = composed(V, w, b, y)[0]
            line.update({"torch_s_median": statistics.median(ref), "torch_s_min": min(ref),
                         "torch_s_max": max(ref),
                         "torch_over_evaluate": statistics.median(ref) / statistics.median(ours),
                         "gV_max_rel_diff_vs_torch":
                             float((out[:d * k].view(d, k) - gV).abs().max() / gV.abs().max())})
            del composed, gV
        except RuntimeError as e:               # a sparse product this torch build lacks
            line["torch_error"] = str(e).splitlines()[0][:200]
        print(json.dumps(line), flush=True)
        lines.append(line)
        plan.close()
        torch.cuda.empty_cache()
    return lines


KERNELS = ("k_fmcsr_forward", "k_fmcsr_grad", "k_fmcsr_grad_seg")


def main():
    import torch
    from cycloneml_amd import fm
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="10000000x256,2000000x1024")
    ap.add_argument("--factors", default="8,32")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--csr", default=None, metavar="NxD",
                    help="time the CSR kernels at this shape instead (1048576x1048576)")
    ap.add_argument("--nnz", type=int, default=64, help="non-zeros per row of --csr")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fm_time needs a GPU")
    dev = torch.device("cuda:0")
    lines = csr_mode(a, dev) if a.csr else []
    for shape in ([] if a.csr else a.shapes.split(",")):
        n, d = (int(v) for v in shape.split("x"))
        g = torch.Generator(device=dev).manual_seed(1)
        X = torch.randn((n, d), dtype=torch.float64, device=dev, generator=g)
        y = torch.randn(n, dtype=torch.float64, device=dev, generator=g)
        for k in (int(v) for v in a.factors.split(",")):
            plan = fm.FMPlan(d, k)
            coef = torch.randn(plan.coefLen, dtype=torch.float64, device=dev, generator=g) * 0.01
            out = torch.empty(plan.coefLen + 2, dtype=torch.float64, device=dev)
            fused = d <= plan.fusedFeatures
            V, w, b = coef[:d * k].view(d, k), coef[d * k:d * k + d], coef[-1]

            def composed():
                S = X @ V
                X2 = X * X
                raw = b + X @ w + 0.5 * (S * S - X2 @ (V * V)).sum(1)
                m = 2.0 * (raw - y)
                gV = X.T @ (m[:, None] * S) - V * (X2.T @ m)[:, None]
                return gV, X.T @ m, m.sum(), ((raw - y) ** 2).sum()

            ours = timed(lambda: plan.evaluate(X, y, coef, out), a.reps)
            ref = timed(composed, a.reps)
            gV = composed()[0]
            err = float((out[:d * k].view(d, k) - gV).abs().max() / gV.abs().max())
            floor = 8.0 * n * d * (1 if fused else 2) / HBM_PEAK
            line = {"n": n, "d": d, "k": k, "form": "fused" if fused else "two-pass",
                    "evaluate_s_median": statistics.median(ours), "evaluate_s_min": min(ours),
                    "evaluate_s_max": max(ours), "hbm_floor_s": floor,
                    "floor_over_evaluate": floor / statistics.median(ours),
                    "torch_s_median": statistics.median(ref), "torch_s_min": min(ref),
                    "torch_s_max": max(ref),
                    "torch_over_evaluate": statistics.median(ref) / statistics.median(ours),
                    "gV_max_rel_diff_vs_torch": err}
            print(json.dumps(line), flush=True)
            lines.append(line)
            plan.close()
            del composed, gV
        del X, y
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.writelines(json.dumps(l) + "\n" for l in lines)


if __name__ == "__main__":
    main()
