// kmeans_centers.hpp -- bodies of kmeans.hip's center kernels, shared by its
// stand-alone launches and the fused levels of centers_prepare_all
// (kmeans_i8_centers.hip).  bid / tid: the block and thread index the
// stand-alone kernel has.  Device code: included by those two units only.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.hpp"

namespace cyc {
namespace kmc {

constexpr unsigned long long kInfBits = 0x7FF0000000000000ull;   // +Infinity
constexpr int kStT = 32;    // centers per statistics tile side
constexpr int kStC = 32;    // dimensions per LDS chunk of the statistics

// C (k x d) -> Ct (d4 x kpad), zero padded; p (optional): k words filled with v
__device__ __forceinline__ void center_transpose_fill(const double* __restrict__ C, int k, int d,
                                                      int d4, int kpad, double* __restrict__ Ct,
                                                      unsigned long long* __restrict__ p,
                                                      unsigned long long v, unsigned bid,
                                                      unsigned tid) {
  const int64_t idx = (int64_t)bid * 256 + tid;
  if (p && idx < k) p[idx] = v;
  const int64_t total = (int64_t)d4 * kpad;
  if (idx >= total) return;
  const int j = (int)(idx / kpad), i = (int)(idx % kpad);
  Ct[idx] = (i < k && j < d) ? C[(int64_t)i * d + j] : 0.0;
}

__device__ __forceinline__ void zero2(unsigned int* __restrict__ a, unsigned int* __restrict__ b,
                                      unsigned tid) {
  if (tid == 0) *a = 0u;
  if (tid == 1 && b) *b = 0u;
}

// computeStatistics pairs (DistanceMeasure.scala:55-66, Euclidean :275-277):
// s = 0.25 * distance * distance, distance = Math.sqrt(sqdist(c_i, c_j)).
// One workgroup per 32 x 32 tile of the upper block triangle: 32-dimension
// chunks of both center tiles in LDS, 2 x 2 pairs per thread, every pair's
// sum sequential over the dimensions in order (bit-exact).  The row minima
// of the diagonal (:62-63) go to dmin as fp64 bit patterns: a statistic is
// >= +0 or NaN, and for those the unsigned bit order is the value order with
// every NaN above +Infinity, so atomicMin never keeps a NaN -- just as the
// reference's `if (s < diagValues(i))` skips it.  dmin starts at kInfBits or
// above (stats_diag's `empty`).
__device__ __forceinline__ void stats_pairs(const double* __restrict__ C, int k, int d, int tps,
                                            double* __restrict__ packed,
                                            unsigned long long* __restrict__ dmin, unsigned bid,
                                            unsigned tid) {
  __shared__ double Ci[kStT][kStC + 1], Cj[kStT][kStC + 1];
  __shared__ unsigned long long rmin[kStT], cmin[kStT];
  int t = (int)bid, bi = 0;
  while (t >= tps - bi) {
    t -= tps - bi;
    ++bi;
  }
  const int bj = bi + t;
  const int tx = tid & 15, ty = tid >> 4;
  if (tid < kStT) rmin[tid] = cmin[tid] = kInfBits;
  double s00 = 0.0, s01 = 0.0, s10 = 0.0, s11 = 0.0;
  for (int c0 = 0; c0 < d; c0 += kStC) {
    __syncthreads();
    for (int e = tid; e < kStT * kStC; e += 256) {
      const int r = e >> 5, cc = e & 31, col = c0 + cc;
      const int gi = bi * kStT + r, gj = bj * kStT + r;
      Ci[r][cc] = (gi < k && col < d) ? C[(int64_t)gi * d + col] : 0.0;
      Cj[r][cc] = (gj < k && col < d) ? C[(int64_t)gj * d + col] : 0.0;
    }
    __syncthreads();
    const int lim = min(kStC, d - c0);
    for (int cc = 0; cc < lim; ++cc) {
      const double a0 = Ci[ty][cc], a1 = Ci[ty + 16][cc];
      const double b0 = Cj[tx][cc], b1 = Cj[tx + 16][cc];
      double q = dsub(a0, b0);
      s00 = dadd(s00, dmul(q, q));
      q = dsub(a0, b1);
      s01 = dadd(s01, dmul(q, q));
      q = dsub(a1, b0);
      s10 = dadd(s10, dmul(q, q));
      q = dsub(a1, b1);
      s11 = dadd(s11, dmul(q, q));
    }
  }
  const double sv[2][2] = {{s00, s01}, {s10, s11}};
#pragma unroll
  for (int a = 0; a < 2; ++a) {
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int i = bi * kStT + ty + 16 * a, j = bj * kStT + tx + 16 * b;
      if (i < k && j < k && j > i) {
        const double dist = __builtin_sqrt(sv[a][b]);
        const double v = dmul(dmul(0.25, dist), dist);
        packed[iut(i, j)] = v;
        const unsigned long long bits = (unsigned long long)__double_as_longlong(v);
        atomicMin(&rmin[ty + 16 * a], bits);
        atomicMin(&cmin[tx + 16 * b], bits);
      }
    }
  }
  __syncthreads();
  if (tid < kStT) {
    const int i = bi * kStT + tid, j = bj * kStT + tid;
    if (i < k && rmin[tid] != kInfBits) atomicMin(&dmin[i], rmin[tid]);
    if (j < k && cmin[tid] != kInfBits) atomicMin(&dmin[j], cmin[tid]);
  }
}

// diagonal (:69-74): packed(i, i) = min over j != i (+Infinity when every
// statistic of the row is NaN); k == 1 gives the single NaN of :50.
// empty: the word dmin was preset to (kInfBits, or ~0 from a byte fill; no
// statistic has those bits unless it is +Infinity itself).
__device__ __forceinline__ void stats_diag(int k, double* __restrict__ packed,
                                           const unsigned long long* __restrict__ dmin,
                                           unsigned long long empty, unsigned bid, unsigned tid) {
  const int i = (int)(bid * 256 + tid);
  if (i >= k) return;
  if (k == 1) {
    packed[0] = __builtin_nan("");
    return;
  }
  const unsigned long long b = dmin[i];
  packed[iut(i, i)] = __longlong_as_double((long long)(b == empty ? kInfBits : b));
}

// MLUtils.fastSquaredDistance's require(norm1 >= 0.0 && norm2 >= 0.0) as a
// with-statistics Lloyd step meets it (kmeans.hip k_require_norms); nblocks:
// the grid of 256-thread blocks the rows and centers are strided over.
__device__ __forceinline__ void require_norms(const double* __restrict__ C, int k, int d,
                                              const double* __restrict__ xnorm, int64_t n,
                                              unsigned long long* __restrict__ req,
                                              unsigned nblocks, unsigned bid, unsigned tid) {
  const int64_t stride = (int64_t)nblocks * 256;
  const int64_t t0 = (int64_t)bid * 256 + tid;
  const int64_t kd = (int64_t)k * d;
  for (int64_t i = t0; i < kd; i += stride)
    if (__builtin_isnan(C[i])) atomicMin(&req[0], (unsigned long long)(i / d));
  for (int64_t r = t0; r < n; r += stride)
    if (__builtin_isnan(xnorm[r])) atomicMin(&req[1], (unsigned long long)r);
  double* out = reinterpret_cast<double*>(req + 2);
  if (t0 < 2 && t0 < k) out[t0] = seq_norm2(C + t0 * d, d);
  if (t0 == 2) out[2] = n > 0 ? xnorm[0] : 0.0;
}

}  // namespace kmc
}  // namespace cyc
