// rowmatrix_multiply.hip -- Y = X B on gfx950 (MI355X): RowMatrix.multiply
// (mllib/linalg/distributed/RowMatrix.scala:400-423), the pass behind
// computeSVD's U and PCAModel.transform.  X is the resident shard (nrows x n,
// row-major dense or CSR), B a local n x k matrix (column-major, DenseMatrix
// .values), Y the nrows x k row-major product.
//
// Kernels
//   dense          row_gemm.hpp: pack() writes B's image once per call and
//                  k_row_gemm<CT, Store> multiplies (timer "k_rmm_dense").
//   k_rmm_transpose
//                  B^T (n x k row-major) for the CSR kernel's gathers.
//   k_rmm_csr<LPR, NA>
//                  LPR = 16 / 32 / 64 lanes per row, the lanes across the
//                  output columns (NA columns per lane and pass over the
//                  row's entries); the sub-group reads LPR entries at a time
//                  and broadcasts them in order, each one gathering the k
//                  contiguous doubles of its row of B^T.  Absent entries are
//                  skipped (the reference's sparse dot).
// Each Y[i][l] is summed by one wave in a fixed order and nothing is split
// over the contraction: no atomics, the same bits on every call.  Padded
// operand elements are explicit zeros and padded accumulators are never
// stored, so a NaN or Inf reaches the outputs the reference's dot gives it.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include <algorithm>
#include <map>
#include <mutex>
#include <string>
#include <utility>

#include "common.hpp"
#include "row_gemm.hpp"

namespace {

using namespace cyc::rowgemm;

// Bt[f k + l] = B[f + l n]
__global__ __launch_bounds__(256) void k_rmm_transpose(const double* __restrict__ B, int n, int k,
                                                       double* __restrict__ Bt) {
  const int64_t total = (int64_t)n * k;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * 256)
    Bt[e] = B[e / k + (e % k) * n];
}

template <int LPR, int NA>
__global__ __launch_bounds__(256) void k_rmm_csr(const int64_t* __restrict__ rowptr,
                                                 const int32_t* __restrict__ colidx,
                                                 const double* __restrict__ vals, int64_t nrows,
                                                 int k, const double* __restrict__ Bt,
                                                 double* __restrict__ Y) {
  constexpr int RPW = 64 / LPR;   // rows per wave
  const int lane = threadIdx.x & 63, sl = lane % LPR, sub = lane / LPR;
  const int64_t gw = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t stride = (int64_t)gridDim.x * 4 * RPW;
  for (int64_t rb = gw * RPW; rb < nrows; rb += stride) {
    const int64_t row = rb + sub;
    const bool ok = row < nrows;
    const int64_t p0 = ok ? rowptr[row] : 0, p1 = ok ? rowptr[row + 1] : 0;
    for (int c0 = 0; c0 < k; c0 += LPR * NA) {
      double acc[NA];
#pragma unroll
      for (int a = 0; a < NA; ++a) acc[a] = 0.0;
      for (int64_t q0 = p0;; q0 += LPR) {
        // entries of this sub-group's row in this round, and the most of any
        // row of the wave (the shuffles below run wave-wide)
        const int cnt = (int)std::min<int64_t>(LPR, std::max<int64_t>(0, p1 - q0));
        int most = cnt;
#pragma unroll
        for (int m = LPR; m < 64; m <<= 1) most = max(most, __shfl_xor(most, m));
        if (most == 0) break;
        int c = 0;
        double v = 0.0;
        if (sl < cnt) {
          c = colidx[q0 + sl];
          v = vals[q0 + sl];
        }
        for (int t = 0; t < most; ++t) {
          const double vt = __shfl(v, t, LPR);
          const int ct = __shfl(c, t, LPR);
          if (t < cnt) {
            const double* b = Bt + (int64_t)ct * k + c0 + sl;
#pragma unroll
            for (int a = 0; a < NA; ++a)
              if (c0 + a * LPR + sl < k) acc[a] += vt * b[a * LPR];
          }
        }
      }
      if (ok) {
#pragma unroll
        for (int a = 0; a < NA; ++a)
          if (c0 + a * LPR + sl < k) Y[row * k + c0 + a * LPR + sl] = acc[a];
      }
    }
  }
}

// The packed / transposed copy of B: one per (device, stream), since calls on
// one stream are ordered and calls on two may overlap.  Never destroyed: the
// HIP runtime may be gone when static destructors run.
std::mutex g_mu;
std::map<std::pair<int, hipStream_t>, cyc::DeviceBuffer>* g_scratch = nullptr;

int scratch_for(hipStream_t st, size_t bytes, double** out) {
  int dev = 0;
  CYC_HIP(hipGetDevice(&dev));
  if (!g_scratch) g_scratch = new std::map<std::pair<int, hipStream_t>, cyc::DeviceBuffer>();
  cyc::DeviceBuffer& b = (*g_scratch)[std::make_pair(dev, st)];
  if (int rc = b.reserve(bytes)) return rc;
  *out = (double*)b.ptr;
  return CYC_OK;
}

int check_args(int64_t nrows, int32_t n, const double* B, int32_t k, const double* Y) {
  CYC_REQUIRE(nrows >= 0, "nrows >= 0");
  CYC_REQUIRE(n >= 1, "numCols must be positive but got " + std::to_string(n));
  CYC_REQUIRE(k >= 1, "B.numCols must be positive but got " + std::to_string(k));
  // DenseMatrix (mllib/linalg/Matrices.scala): one JVM array of n k doubles
  CYC_REQUIRE((int64_t)n * k <= INT32_MAX, std::to_string(n) + " x " + std::to_string(k) +
                                               " dense matrix is too large to allocate");
  CYC_REQUIRE(B != nullptr, "B must not be null");
  CYC_REQUIRE(nrows == 0 || Y != nullptr, "Y must not be null");
  return CYC_OK;
}

template <int LPR, int NA>
void launch_csr(const int64_t* rowptr, const int32_t* colidx, const double* vals, int64_t nrows,
                int k, const double* Bt, double* Y, hipStream_t st) {
  const int64_t waves = (nrows + 64 / LPR - 1) / (64 / LPR);
  hipLaunchKernelGGL((k_rmm_csr<LPR, NA>), dim3((unsigned)std::min((waves + 3) / 4, kMaxGrid)),
                     dim3(256), 0, st, rowptr, colidx, vals, nrows, k, Bt, Y);
}

}  // namespace

extern "C" {

int cyc_rowmatrix_multiply_dev(const double* X, int64_t nrows, int32_t n, const double* B,
                               int32_t k, double* Y, void* stream) {
  if (int rc = check_args(nrows, n, B, k, Y)) return rc;
  if (nrows == 0) return CYC_OK;
  CYC_REQUIRE(X != nullptr, "non-null rows");
  hipStream_t st = cyc::as_stream(stream);
  std::lock_guard<std::mutex> lock(g_mu);
  double* Bp = nullptr;
  if (int rc = scratch_for(st, sizeof(double) * (size_t)packed_len(n, k), &Bp)) return rc;
  // B(f, col) = B[f + col n]
  if (int rc = pack(B, n, k, 1, n, 1, 0, Bp, st)) return rc;
  return gemm(X, nrows, n, k, Bp, Store{}, Y, "k_rmm_dense", st);
}

int cyc_rowmatrix_multiply_csr_dev(const int64_t* rowptr, const int32_t* colidx,
                                   const double* vals, int64_t nrows, int32_t n, const double* B,
                                   int32_t k, double* Y, void* stream) {
  if (int rc = check_args(nrows, n, B, k, Y)) return rc;
  if (nrows == 0) return CYC_OK;
  CYC_REQUIRE(rowptr != nullptr, "non-null CSR arrays");
  hipStream_t st = cyc::as_stream(stream);
  int64_t base = 0, end = 0;
  CYC_HIP(hipMemcpyAsync(&base, rowptr, sizeof(base), hipMemcpyDeviceToHost, st));
  CYC_HIP(hipMemcpyAsync(&end, rowptr + nrows, sizeof(end), hipMemcpyDeviceToHost, st));
  CYC_HIP(hipStreamSynchronize(st));
  if (end <= base) {   // rows without entries (their arrays may be null): Y = 0
    CYC_HIP(hipMemsetAsync(Y, 0, sizeof(double) * (size_t)nrows * (size_t)k, st));
    return CYC_OK;
  }
  CYC_REQUIRE(colidx && vals, "non-null CSR arrays");
  // the check reads row r's indices at rowptr[r] - rowptr[0]; the kernel, as
  // the Gramian's CSR pass, at rowptr[r] (a slice keeps the whole arrays)
  if (int rc = cyc::check_csr_indices(rowptr, colidx + base, nrows, n, st)) return rc;
  const int64_t elems = (int64_t)n * k;
  std::lock_guard<std::mutex> lock(g_mu);
  double* Bt = nullptr;
  if (int rc = scratch_for(st, sizeof(double) * (size_t)elems, &Bt)) return rc;
  hipLaunchKernelGGL(k_rmm_transpose, dim3((unsigned)std::min<int64_t>((elems + 255) / 256, 4096)),
                     dim3(256), 0, st, B, (int)n, (int)k, Bt);
  CYC_LAUNCH_CHECK("k_rmm_transpose");
  cyc::KernelTimer timer("k_rmm_csr", st);
  if (k <= 16) launch_csr<16, 1>(rowptr, colidx, vals, nrows, k, Bt, Y, st);
  else if (k <= 32) launch_csr<32, 1>(rowptr, colidx, vals, nrows, k, Bt, Y, st);
  else if (k <= 64) launch_csr<64, 1>(rowptr, colidx, vals, nrows, k, Bt, Y, st);
  else launch_csr<64, 4>(rowptr, colidx, vals, nrows, k, Bt, Y, st);
  CYC_LAUNCH_CHECK("k_rmm_csr");
  return CYC_OK;
}

}  // extern "C"
