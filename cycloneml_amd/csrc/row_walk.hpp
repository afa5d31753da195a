// row_walk.hpp -- the row walk shared by the per-row passes of glm.hip and
// linreg.hip: one wave per run of 64-row batches, the wave
// forming the 64 dot products of a batch so that lane i ends up holding row
// i's, and the launch geometry that goes with it.
//
// Rows: DenseRows<LPR> (LPR = 8 / 16 / 32 / 64 lanes per row, the smallest
// that holds numFeatures, 64 / LPR rows in flight per wave), CsrRows (a wave
// per row, coefficients gathered by column index) and NoRows (no features).
// `cf` is the coefficient vector the dots read: the caller's LDS copy, or
// the global vector itself where it is too long to stage.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#pragma clang fp contract(off)

namespace cyc {
namespace rowwalk {

constexpr int64_t kMaxWaves = 16384;

// ---- the rows of a batch: lane i's return value is row (base + i)'s dot -----
// A row that is not live (lane i's flag: weight 0, or past n) is not read.

// LPR lanes per row: sub-group g = lane / LPR walks rows g LPR .. g LPR + LPR - 1
// of the batch, four at a time (four loads in flight per lane), the four
// dots reduced over the sub-group in a fixed order; lane g LPR + t keeps
// row t's.
template <int LPR>
struct DenseRows {
  const double* X;
  __device__ __forceinline__ double dot(int64_t base, int lane, bool live, int p,
                                        const double* cf) const {
    const int g = lane / LPR, sl = lane % LPR;
    const unsigned long long liveRows = __ballot(live);
    double mine = 0.0;
    for (int t0 = 0; t0 < LPR; t0 += 4) {
      double s[4];
      bool on[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        on[u] = (liveRows >> (g * LPR + t0 + u)) & 1;
        s[u] = 0.0;
      }
      const double* x0 = X + (base + g * LPR + t0) * p;
      for (int f = sl; f < p; f += LPR) {
        const double c = cf[f];
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (on[u]) s[u] += x0[(int64_t)u * p + f] * c;
      }
      // four rows' partials to one value per lane: after the two exchanges
      // lane sl holds row t0 + (sl & 3)'s, then the xor tree over the rest
      const bool odd = sl & 1, hi = sl & 2;
      double a0 = odd ? s[1] : s[0], a1 = odd ? s[3] : s[2];
      a0 += __shfl_xor(odd ? s[0] : s[1], 1);
      a1 += __shfl_xor(odd ? s[2] : s[3], 1);
      double c = hi ? a1 : a0;
      c += __shfl_xor(hi ? a0 : a1, 2);
#pragma unroll
      for (int m = 4; m < LPR; m <<= 1) c += __shfl_xor(c, m);
      if ((sl & ~3) == t0) mine = c;
    }
    return mine;
  }
};

struct CsrRows {
  const int64_t* rowptr;
  const int32_t* colidx;
  const double* vals;
  __device__ __forceinline__ double dot(int64_t base, int lane, bool live, int p,
                                        const double* cf) const {
    int64_t b = 0, e = 0;
    if (live) {
      b = rowptr[base + lane];
      e = rowptr[base + lane + 1];
    }
    double mine = 0.0;
    for (int t = 0; t < 64; ++t) {
      const int64_t p0 = __shfl(b, t), p1 = __shfl(e, t);
      if (p0 >= p1) continue;   // wave-uniform: an empty, dead or absent row
      double s = 0.0;
      for (int64_t q = p0 + lane; q < p1; q += 64) s += vals[q] * cf[colidx[q]];
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m);
      if (lane == t) mine = s;
    }
    return mine;
  }
};

struct NoRows {
  __device__ __forceinline__ double dot(int64_t, int, bool, int, const double*) const {
    return 0.0;
  }
};

// One wave per run of 64-row batches: blocks of 4 waves, at most kMaxWaves.
struct Geometry {
  int64_t batchesPerWave, blocks, waves;
};

inline Geometry geometry(int64_t n) {
  const int64_t batches = (n + 63) / 64;
  const int64_t want = std::min<int64_t>(kMaxWaves, batches);
  Geometry g;
  g.batchesPerWave = (batches + want - 1) / want;
  const int64_t nw = (batches + g.batchesPerWave - 1) / g.batchesPerWave;
  g.blocks = (nw + 3) / 4;
  g.waves = g.blocks * 4;
  return g;
}

// The features of one call: dense X, CSR, or none (coef == NULL).
struct RowsArg {
  const double* X = nullptr;
  const int64_t* rowptr = nullptr;
  const int32_t* colidx = nullptr;
  const double* vals = nullptr;
  bool sparse = false;
};

inline RowsArg dense_rows(const double* X) {
  RowsArg r;
  r.X = X;
  return r;
}

inline RowsArg csr_rows(const int64_t* rowptr, const int32_t* colidx, const double* vals) {
  RowsArg r;
  r.rowptr = rowptr;
  r.colidx = colidx;
  r.vals = vals;
  r.sparse = true;
  return r;
}

// f(rows) with the Rows type of this call: NoRows without coefficients, the
// narrowest DenseRows that holds p, or CsrRows.
template <class F>
void with_rows(const RowsArg& r, const double* coef, int p, F f) {
  if (!coef) f(NoRows{});
  else if (r.sparse) f(CsrRows{r.rowptr, r.colidx, r.vals});
  else if (p <= 8) f(DenseRows<8>{r.X});
  else if (p <= 16) f(DenseRows<16>{r.X});
  else if (p <= 32) f(DenseRows<32>{r.X});
  else f(DenseRows<64>{r.X});
}

}  // namespace rowwalk
}  // namespace cyc
