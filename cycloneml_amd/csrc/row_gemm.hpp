// row_gemm.hpp -- Y = epilogue(X B) on gfx950 (MI355X) for a tall X (nrows x
// n, row-major) and a small B (n x k): the fp64 MFMA product behind
// RowMatrix.multiply (rowmatrix_multiply.hip) and the MLP's forward and delta
// passes (mlp.hip), and the packed image of B that they and the GMM E step
// (gmm.hip) stage.  Kernels here are templates or static: every translation
// unit that includes this file gets its own copy.
//
// The image.  pack() writes, for every chunk of kChunk contraction indices and
// every 16-column tile, the 256 doubles in the order the MFMA B operand is
// read (k-step kk, then lane):
//   Bp[((chunk KT + tile) 4 + kk) 64 + lane] = B(f, col),
//   f = chunk kChunk + 4 (lane >> 4) + kk, col = 16 tile + (lane & 15),
// KT = tiles16(k), explicit zeros where f >= n or col >= k: packed_len(n, k)
// doubles.  A reader copies 256 CT consecutive doubles per chunk and panel
// into LDS, and every B read of a wave is 64 consecutive doubles (no bank
// conflict, no padding).
//
// The product.  k_row_gemm<CT, Epi>: v_mfma_f64_16x16x4f64, kWaves waves x 32
// rows per workgroup, a panel of CT <= kPanelTiles column tiles (64 columns)
// per pass over the rows.  X goes from HBM straight into registers in the MFMA
// A layout -- lane (row l & 15, group g = l >> 4) holds indices f0 + 4g ..
// 4g + 3 of its row for k-steps 0..3 (the order within a chunk is permuted,
// the same for every call: 128 contiguous bytes per row per chunk) -- one
// chunk ahead of the multiply.  The chunk's packed B panel is copied into one
// of two LDS buffers one chunk ahead, one barrier per chunk.  k > 64: gemm()
// launches over the full panels (consecutive workgroups take the panels of
// one row tile, so the re-read of X comes from L2) and once more for the
// remaining CT tiles.
//
// Each output is summed by one wave in a fixed order and nothing is split over
// the contraction: no atomics, the same bits on every call.  Padded operand
// elements are explicit zeros and padded accumulators are never stored, so a
// NaN or Inf reaches the outputs the reference's dot gives it.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>

#include "common.hpp"

namespace cyc::rowgemm {

constexpr int kChunk = 16;                  // contraction indices per LDS chunk
constexpr int kPanelTiles = 4;              // 16-column tiles per pass over the rows
constexpr int kWaves = 8;                   // waves per workgroup, 32 rows each
constexpr int kTileRows = 32 * kWaves;
constexpr int64_t kMaxGrid = 1 << 20;

// four doubles of a row: rows start at any multiple of 8 bytes
typedef double double4_a8 __attribute__((ext_vector_type(4), aligned(8)));

inline int tiles16(int x) { return x / 16 + (x % 16 != 0); }
// doubles of the image of an n x k matrix
inline int64_t packed_len(int n, int k) {
  return (int64_t)(n / kChunk + (n % kChunk != 0)) * tiles16(k) * 256;
}

// `batches` images of imgLen doubles, one after the other; B(f, col) of batch
// j is B[j batchStride + f sf + col sc]
static __global__ __launch_bounds__(256) void k_row_pack(const double* __restrict__ B, int n,
                                                         int k, int64_t sf, int64_t sc,
                                                         int64_t batchStride, int KT,
                                                         int64_t imgLen, int64_t total,
                                                         double* __restrict__ Bp) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * 256) {
    const int64_t j = e / imgLen, i = e % imgLen;
    const int lane = (int)(i & 63), kk = (int)((i >> 6) & 3);
    const int64_t t = i >> 8;
    const int tile = (int)(t % KT);
    const int64_t f = (t / KT) * kChunk + 4 * (lane >> 4) + kk;
    const int col = tile * 16 + (lane & 15);
    Bp[e] = (f < n && col < k) ? B[j * batchStride + f * sf + col * sc] : 0.0;
  }
}

inline int pack(const double* B, int n, int k, int64_t sf, int64_t sc, int64_t batches,
                int64_t batchStride, double* Bp, hipStream_t st) {
  const int64_t imgLen = packed_len(n, k), total = batches * imgLen;
  hipLaunchKernelGGL(k_row_pack, dim3((unsigned)std::min<int64_t>((total + 255) / 256, 4096)),
                     dim3(256), 0, st, B, n, k, sf, sc, batchStride, tiles16(k), imgLen, total,
                     Bp);
  CYC_LAUNCH_CHECK("k_row_pack");
  return CYC_OK;
}

// An epilogue is a device functor passed by value: epi(v, row, col, k) is
// called once per owned output with the finished sum v and returns the double
// to store at Y[row k + col].  kWideCT: the widest panel that still runs two
// workgroups per CU (4 waves per SIMD); the 16 CT accumulator registers of a
// wider one leave room for one (more would spill).
struct Store {
  static constexpr int kWideCT = 2;
  __device__ double operator()(double v, int64_t, int, int) const { return v; }
};

// Column tiles [ct0 + panel CT, + CT) of Y = epilogue(X B) for every 256-row
// tile; work item w = row tile x panels + panel.
template <int CT, class Epi>
__global__ __launch_bounds__(64 * kWaves, CT <= Epi::kWideCT ? 4 : 2) void k_row_gemm(
    const double* __restrict__ X, int64_t nrows, int n, int k, const double* __restrict__ Bp,
    int KT, int ct0, int panels, Epi epi, double* __restrict__ Y) {
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
          const double4_a8 v = *reinterpret_cast<const double4_a8*>(xp[t] + f0);
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
    // lane holds rows 16 t + g + 4 r, column (lane & 15) of each tile.  The
    // column outermost and a lane without a first row out of the way, so what
    // an epilogue reads per column (the bias) is loaded once: the first
    // output's load then stands before all the others
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      const int col = (ctb + ct) * 16 + (lane & 15);
      if (col >= k || r0 + g >= nrows) continue;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int64_t row = r0 + t * 16 + g + 4 * r;
          if (row >= nrows) continue;
          Y[row * k + col] = epi(acc[t][ct][r], row, col, k);
        }
    }
  }
}

template <int CT, class Epi>
void launch_gemm(const double* X, int64_t nrows, int n, int k, const double* Bp, int KT, int ct0,
                 int panels, Epi epi, double* Y, hipStream_t st) {
  const int64_t total = (nrows + kTileRows - 1) / kTileRows * panels;
  hipLaunchKernelGGL((k_row_gemm<CT, Epi>), dim3((unsigned)std::min(total, kMaxGrid)),
                     dim3(64 * kWaves), 0, st, X, nrows, n, k, Bp, KT, ct0, panels, epi, Y);
}

// Y (nrows x k) = epilogue(X (nrows x n) B), Bp the image of B: the full
// panels, then the remaining tiles.  timerName labels the KernelTimer and the
// launch check.
template <class Epi>
int gemm(const double* X, int64_t nrows, int n, int k, const double* Bp, Epi epi, double* Y,
         const char* timerName, hipStream_t st) {
  cyc::KernelTimer timer(timerName, st);
  const int KT = tiles16(k);
  const int full = KT / kPanelTiles, rem = KT % kPanelTiles, c0 = full * kPanelTiles;
  if (full) launch_gemm<kPanelTiles>(X, nrows, n, k, Bp, KT, 0, full, epi, Y, st);
  if (rem == 1) launch_gemm<1>(X, nrows, n, k, Bp, KT, c0, 1, epi, Y, st);
  if (rem == 2) launch_gemm<2>(X, nrows, n, k, Bp, KT, c0, 1, epi, Y, st);
  if (rem == 3) launch_gemm<3>(X, nrows, n, k, Bp, KT, c0, 1, epi, Y, st);
  CYC_LAUNCH_CHECK(timerName);
  return CYC_OK;
}

// *dst += sum_w slab[w]: thread t sums w = t, t + 256, .. in order, then a
// fixed LDS tree.
static __global__ __launch_bounds__(256) void k_fold_add(const double* __restrict__ slab,
                                                         int64_t count, double* __restrict__ dst) {
  __shared__ double sh[256];
  const int t = threadIdx.x;
  double s = 0.0;
  for (int64_t w = t; w < count; w += 256) s += slab[w];
  sh[t] = s;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (t < h) sh[t] += sh[t + h];
    __syncthreads();
  }
  if (t == 0) *dst += sh[0];
}

inline int fold_add(const double* slab, int64_t count, double* dst, hipStream_t st) {
  hipLaunchKernelGGL(k_fold_add, dim3(1), dim3(256), 0, st, slab, count, dst);
  CYC_LAUNCH_CHECK("k_fold_add");
  return CYC_OK;
}

}  // namespace cyc::rowgemm
