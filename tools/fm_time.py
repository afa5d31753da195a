"""Time one FM evaluation (cyc_fm_evaluate_dev) on the device against the HBM
floor and the torch composition X @ V, (X * X) @ (V * V), X.T @ [m o S | m].

    python tools/fm_time.py [--shapes 10000000x256,2000000x1024] [--factors 8,32]
                            [--reps 5] [--out bench_out/fm_time.jsonl]

Per (shape, k): device-event times of `reps` evaluations after a warm-up of
each path (median and spread), the floor 8 n d bytes (fused; twice that in the
two-pass form) over the HBM peak, and the same for the torch composition.  The
data is seeded on the device.  No GPU: an error, not a fallback."""
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


def main():
    import torch
    from cycloneml_amd import fm
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="10000000x256,2000000x1024")
    ap.add_argument("--factors", default="8,32")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fm_time needs a GPU")
    dev = torch.device("cuda:0")
    lines = []
    for shape in a.shapes.split(","):
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
