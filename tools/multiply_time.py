#!/usr/bin/env python3
"""Times RowMatrix.multiply (cyc_rowmatrix_multiply_dev, the shared k_row_gemm
under the timer label k_rmm_dense; CSR: cyc_rowmatrix_multiply_csr_dev,
k_rmm_csr) beside torch.matmul (rocBLAS dgemm)
on the same device tensors, in one process: HIP events, the median of --runs
runs after --warmup warm-ups.  One JSON line per shape (also appended to --out
when given), with the share of
max(bytes / 6.3e12, 2 nrows n k / 78.6e12) the median reaches: bytes =
8 nrows (n + k) for dense rows, the CSR arrays plus Y for CSR rows.

    python tools/multiply_time.py                 # the shapes of DESIGN.md
    python tools/multiply_time.py --shape 1000000x256x16 --shape 4000000x1024x16:64
                                                  # ROWSxNxK[:NNZ_PER_ROW]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_ACHIEVABLE = 6.3e12      # bytes / s, streaming reads on an MI355X
FP64_MFMA = 78.6e12          # flop / s

DEFAULT = ["4000000x1024x8", "4000000x1024x64", "4000000x1024x256", "4000000x256x16",
           "4000000x1024x16:64"]


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


def time_shape(nrows, n, k, nnz, warmup, runs, device):
    import torch
    from cycloneml_amd import _native as N
    from cycloneml_amd.linalg import CSRRows
    lib = N.load()
    g = torch.Generator(device=device).manual_seed(n + k)
    B = torch.randn((n, k), dtype=torch.float64, device=device, generator=g)
    Bcm = B.t().contiguous()                       # column-major values
    Y = torch.empty((nrows, k), dtype=torch.float64, device=device)
    res = {"rows": nrows, "n": n, "k": k, "device": torch.cuda.get_device_name(device),
           "warmup": warmup, "runs": runs}
    if nnz:
        # nnz sorted distinct columns per row: a random start and stride
        res["nnz_per_row"] = nnz
        step = n // nnz
        start = torch.randint(0, step, (nrows, 1), device=device, generator=g)
        colidx = (start + step * torch.arange(nnz, device=device)).to(torch.int32).reshape(-1)
        vals = torch.randn(nrows * nnz, dtype=torch.float64, device=device, generator=g)
        rowptr = torch.arange(nrows + 1, dtype=torch.int64, device=device) * nnz
        rows = CSRRows(rowptr, colidx, vals, n)
        nbytes = 8 * (nrows + 1) + 12 * nrows * nnz + 8 * nrows * k
        flops = 2.0 * nrows * nnz * k
        Xs = torch.sparse_csr_tensor(rowptr, colidx.to(torch.int64), vals, (nrows, n))

        def ours():
            N.check(lib.cyc_rowmatrix_multiply_csr_dev(
                N.ptr(rows.rowptr), N.ptr(rows.colidx), N.ptr(rows.values), nrows, n, N.ptr(Bcm),
                k, N.ptr(Y), N.stream_handle()))

        def theirs():
            torch.matmul(Xs, B)
    else:
        X = torch.empty((nrows, n), dtype=torch.float64, device=device)
        step = max(1, (1 << 28) // n)                  # 2 GiB of rows at a time
        for r in range(0, nrows, step):
            X[r:r + step].normal_(generator=g)
        nbytes = 8 * nrows * (n + k)
        flops = 2.0 * nrows * n * k
        Yt = torch.empty_like(Y)

        def ours():
            N.check(lib.cyc_rowmatrix_multiply_dev(N.ptr(X), nrows, n, N.ptr(Bcm), k, N.ptr(Y),
                                                   N.stream_handle()))

        def theirs():
            torch.matmul(X, B, out=Yt)
    floor_ms = max(nbytes / HBM_ACHIEVABLE, flops / FP64_MFMA) * 1e3
    res["floor_ms"] = round(floor_ms, 3)
    res["bound"] = "hbm" if nbytes / HBM_ACHIEVABLE >= flops / FP64_MFMA else "mfma"
    for name, fn in (("multiply", ours), ("matmul", theirs)):
        try:
            med, lo, hi = _median_ms(fn, warmup, runs)
        except RuntimeError as e:          # torch without a kernel for this product
            if name == "multiply":
                raise
            res["matmul_error"] = str(e).splitlines()[0][:200]
            return res
        res[name + "_ms"] = round(med, 3)
        res[name + "_range"] = [round(lo, 3), round(hi, 3)]
        res[name + "_floor_share"] = round(floor_ms / med, 3)
    res["multiply_over_matmul"] = round(res["multiply_ms"] / res["matmul_ms"], 3)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--shape", action="append", default=None,
                    help="ROWSxNxK, or ROWSxNxK:NNZ for CSR rows (repeatable)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("multiply_time.py needs a GPU")
    device = torch.device("cuda:0")
    for s in a.shape or DEFAULT:
        dims, _, nnz = s.lower().partition(":")
        nrows, n, k = (int(v) for v in dims.split("x"))
        line = json.dumps(time_shape(nrows, n, k, int(nnz or 0), a.warmup, a.runs, device))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
