// rowmatrix_multiply.hip -- Y = X B on gfx950 (MI355X): RowMatrix.multiply
// (mllib/linalg/distributed/RowMatrix.scala:400-423), the pass behind
// computeSVD's U and PCAModel.transform.  X is the resident shard (nrows x n,
// row-major dense or CSR), B a local n x k matrix (column-major, DenseMatrix
// .values), Y the nrows x k row-major product.
//
// Kernels
//   k_rmm_pack     B into the image the dense kernel stages: for every chunk
//                  of kChunk contraction indices and every 16-column tile, the
//                  256 doubles in the order the MFMA B operand is read (k-step,
//                  then lane), zero where the index or the column is past the
//                  matrix.  n k elements, once per call.
//   k_rmm_dense<CT>
//                  v_mfma_f64_16x16x4f64, 8 waves x 32 rows per workgroup, a
//                  panel of CT <= kPanelTiles column tiles (64 columns)
//                  per pass over the rows.  X goes from HBM straight into
//                  registers in the MFMA A layout -- lane (row l & 15, group
//                  g = l >> 4) holds indices f0 + 4g .. 4g + 3 of its row for
//                  k-steps 0..3 (the order within a chunk is permuted, the
//                  same for every call: 128 contiguous bytes per row per
//                  chunk) -- one chunk ahead of the multiply.  The chunk's
//                  packed B panel is copied into one of two LDS buffers one
//                  chunk ahead, one barrier per chunk; every B read is 64
//                  consecutive doubles (no bank conflict, no padding).
//                  k > 64: a launch over the full panels (consecutive
//                  workgroups take the panels of one row tile, so the re-read
//                  of X comes from L2) and one for the remaining CT tiles.
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

namespace {

constexpr int kChunk = 16;                  // contraction indices per LDS chunk
constexpr int kPanelTiles = 4;              // 16-column tiles per pass over the rows
constexpr int kWaves = 8;                   // waves per workgroup, 32 rows each
constexpr int kTileRows = 32 * kWaves;
constexpr int64_t kMaxGrid = 1 << 20;

// four doubles of a row: rows start at any multiple of 8 bytes
typedef double rmm_double4 __attribute__((ext_vector_type(4), aligned(8)));

// Bp[((chunk KT + tile) 4 + kk) 64 + lane] = B[chunk kChunk + 4 (lane >> 4) + kk]
// [16 tile + (lane & 15)], KT = column tiles of B
__global__ __launch_bounds__(256) void k_rmm_pack(const double* __restrict__ B, int n, int k,
                                                  int KT, int64_t total,
                                                  double* __restrict__ Bp) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * 256) {
    const int lane = (int)(e & 63), kk = (int)((e >> 6) & 3);
    const int64_t t = e >> 8;
    const int tile = (int)(t % KT);
    const int64_t f = (t / KT) * kChunk + 4 * (lane >> 4) + kk;
    const int col = tile * 16 + (lane & 15);
    Bp[e] = (f < n && col < k) ? B[f + (int64_t)col * n] : 0.0;
  }
}

// Column tiles [ct0 + panel CT, + CT) of Y for every 256-row tile; work item
// w = row tile x panels + panel.
// Two workgroups per CU (4 waves per SIMD) up to CT = 2; the 16 CT accumulator
// registers of a wider panel leave room for one (more would spill).
template <int CT>
__global__ __launch_bounds__(64 * kWaves, CT <= 2 ? 4 : 2) void k_rmm_dense(
    const double* __restrict__ X, int64_t nrows, int n, int k, const double* __restrict__ Bp,
    int KT, int ct0, int panels, double* __restrict__ Y) {
  constexpr int CH = 256 * CT;                                  // doubles per staged chunk
  constexpr int PT = (CH + 64 * kWaves - 1) / (64 * kWaves);    // per thread
  __shared__ double Bs[2][CH];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4;
  const int nfull = n / kChunk, nch = nfull + (n % kChunk != 0);
  const int64_t total = (nrows + kTileRows - 1) / kTileRows * panels;
  for (int64_t w = blockIdx.x; w < total; w += gridDim.x) {
    const int ctb = ct0 + (int)(w % panels) * CT;
    const int64_t r0 = w / panels * kTileRows + wave * 32;
    // rows past nrows read the last row and indices past n the last index: a
    // valid address and no branch around a load.  The multiply replaces both
    // by explicit zeros when it reads the registers (not here: a select on a
    // loaded value would wait for the load one chunk early).
    const double* xp[2];
    bool ok[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int64_t row = r0 + t * 16 + (lane & 15);
      ok[t] = row < nrows;
      xp[t] = X + (ok[t] ? row : nrows - 1) * n;
    }
    auto loadX = [&](int ch, double (&x)[2][4]) {
      const int64_t f0 = (int64_t)ch * kChunk + 4 * g;   // n + 15 may pass 2^31
      if (ch < nfull) {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          const rmm_double4 v = *reinterpret_cast<const rmm_double4*>(xp[t] + f0);
#pragma unroll
          for (int j = 0; j < 4; ++j) x[t][j] = v[j];
        }
      } else {
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int j = 0; j < 4; ++j) x[t][j] = xp[t][std::min<int64_t>(f0 + j, n - 1)];
      }
    };
    auto loadB = [&](int ch, double (&b)[PT]) {
      const double* src = Bp + ((int64_t)ch * KT + ctb) * 256;
#pragma unroll
      for (int q = 0; q < PT; ++q) {
        b[q] = src[min(tid + q * 64 * kWaves, CH - 1)];   // unconditional: no branch to wait at
      }
    };
    auto storeB = [&](int ch, const double (&b)[PT]) {
#pragma unroll
      for (int q = 0; q < PT; ++q) {
        const int e = tid + q * 64 * kWaves;
        if (e < CH) Bs[ch & 1][e] = b[q];
      }
    };
    cyc_double4 acc[2][CT];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) acc[t][ct] = cyc_double4{0.0, 0.0, 0.0, 0.0};
    double xa[2][4], xb[2][4], bn[PT];
    __syncthreads();   // the previous item's last chunk is read
    loadB(0, bn);
    loadX(0, xa);
    storeB(0, bn);
    __syncthreads();
    // chunk ch: issue chunk ch + 1's loads, multiply, park the next B chunk
    // in the other buffer (free since the barrier that ended chunk ch - 1)
    auto step = [&](int ch, double (&xc)[2][4], double (&xn)[2][4]) {
      const bool more = ch + 1 < nch;
      if (more) {
        loadB(ch + 1, bn);
        loadX(ch + 1, xn);
      }
      const double* W = Bs[ch & 1];
      const int64_t f0 = (int64_t)ch * kChunk + 4 * g;
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        const bool in = f0 + kk < n;
        const double a0 = (ok[0] && in) ? xc[0][kk] : 0.0;
        const double a1 = (ok[1] && in) ? xc[1][kk] : 0.0;
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
          const double b = W[(ct * 4 + kk) * 64 + lane];
          acc[0][ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b, acc[0][ct], 0, 0, 0);
          acc[1][ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b, acc[1][ct], 0, 0, 0);
        }
      }
      if (more) {
        storeB(ch + 1, bn);
        __syncthreads();
      }
    };
    for (int ch = 0; ch < nch; ch += 2) {
      step(ch, xa, xb);
      if (ch + 1 < nch) step(ch + 1, xb, xa);
    }
    // lane holds rows 16 t + g + 4 r, column (lane & 15) of each tile
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t row = r0 + t * 16 + g + 4 * r;
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
          const int col = (ctb + ct) * 16 + (lane & 15);
          if (row < nrows && col < k) Y[row * k + col] = acc[t][ct][r];
        }
      }
  }
}

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

template <int CT>
void launch_dense(const double* X, int64_t nrows, int n, int k, const double* Bp, int KT, int ct0,
                  int panels, double* Y, hipStream_t st) {
  const int64_t total = (nrows + kTileRows - 1) / kTileRows * panels;
  hipLaunchKernelGGL((k_rmm_dense<CT>), dim3((unsigned)std::min(total, kMaxGrid)),
                     dim3(64 * kWaves), 0, st, X, nrows, n, k, Bp, KT, ct0, panels, Y);
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
  const int KT = k / 16 + (k % 16 != 0), nch = n / kChunk + (n % kChunk != 0);
  const int64_t packed = (int64_t)nch * KT * 256;
  std::lock_guard<std::mutex> lock(g_mu);
  double* Bp = nullptr;
  if (int rc = scratch_for(st, sizeof(double) * (size_t)packed, &Bp)) return rc;
  hipLaunchKernelGGL(k_rmm_pack, dim3((unsigned)std::min<int64_t>((packed + 255) / 256, 4096)),
                     dim3(256), 0, st, B, (int)n, (int)k, KT, packed, Bp);
  CYC_LAUNCH_CHECK("k_rmm_pack");
  cyc::KernelTimer timer("k_rmm_dense", st);
  const int full = KT / kPanelTiles, rem = KT % kPanelTiles;
  if (full)
    launch_dense<kPanelTiles>(X, nrows, n, k, Bp, KT, 0, full, Y, st);
  if (rem == 1) launch_dense<1>(X, nrows, n, k, Bp, KT, full * kPanelTiles, 1, Y, st);
  if (rem == 2) launch_dense<2>(X, nrows, n, k, Bp, KT, full * kPanelTiles, 1, Y, st);
  if (rem == 3) launch_dense<3>(X, nrows, n, k, Bp, KT, full * kPanelTiles, 1, Y, st);
  CYC_LAUNCH_CHECK("k_rmm_dense");
  return CYC_OK;
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
