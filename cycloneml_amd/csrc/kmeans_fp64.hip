// kmeans_fp64.hip -- the dense KMeans screens that decide in fp64, and the
// exact tier, on gfx950 (MI355X): the tiers of a Euclidean Lloyd call behind
// the i8 screens of kmeans_i8.hip and kmeans_i8_cands.hip (kmeans.hip has the
// order of the tiers).
//
//   k_kmeans_assign / k_kmeans_assign2   fp64 MFMA (v_mfma_f64_16x16x4f64)
//       screen of |x|^2 + |c|^2 - 2 x.c for an LDS tile of rows against every
//       center, with a rigorous error margin; a row whose best center is
//       separated from every other by more than the margin gets that center
//       (and, when asked, the exact sequential sqdist); other rows are queued.
//       Over every row, or over the rows an earlier screen queued.
//   k_center_split + k_kmeans_assign3    the bf16x3 screen in front of it for
//       a plan without a row image.
//   k_exact_dist + k_exact_replay / k_assign_exact   the reference's
//       findClosest-with-statistics loop (DistanceMeasure.scala:282-313),
//       restated instruction for instruction, for the queued rows (ties, near
//       ties, NaN/Inf).
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include <algorithm>

#include "common.hpp"
#include "kmeans_fp64.hpp"

namespace {

constexpr int kWaves = 8;                 // waves per assign workgroup
constexpr int kAssignThreads = kWaves * 64;

// --------------------------------------------------------------- assign
// Screening state of one (row, lane) slot: smallest lower bound L1 with its
// center index I1 and upper bound U1, and the second smallest lower bound L2.
// A row is decided when L2 > U1: every other center is provably farther than
// I1 by more than the combined fp64 error, so the reference's pruned loop
// (whose prunes only skip centers that cannot win) returns I1 as well.
//
// The bounds are kept in fp32 rounded outward (L down, U up): the interval
// only widens, so a decided row is still provably decided; rows whose gap is
// below fp32 resolution (~1e-7 relative) simply go to the exact path.  This
// halves the per-lane state (16 slots per lane) and keeps the kernel in
// registers.
struct Slot {
  float L1, U1, L2;
  int I1;
};

// one fp32 ulp toward -inf / +inf (f finite, not NaN)
__device__ __forceinline__ float ulp_down(float f) {
  int b = __float_as_int(f);
  if (f == 0.0f) return -__int_as_float(1);
  return __int_as_float(f > 0.0f ? b - 1 : b + 1);
}
__device__ __forceinline__ float f_down(double x) {
  float f = (float)x;
  return ((double)f > x) ? ulp_down(f) : f;
}
__device__ __forceinline__ float f_up(double x) {
  float f = (float)x;
  return ((double)f < x) ? -ulp_down(-f) : f;
}

__device__ __forceinline__ void slot_merge(Slot& a, float oL1, float oU1, float oL2, int oI1) {
  float hi = fmaxf(a.L1, oL1);
  float l2 = fminf(hi, fminf(a.L2, oL2));
  if (oL1 < a.L1 || (oL1 == a.L1 && oI1 >= 0 && (a.I1 < 0 || oI1 < a.I1))) {
    a.L1 = oL1;
    a.U1 = oU1;
    a.I1 = oI1;
  }
  a.L2 = l2;
}

// BM rows per workgroup (BM/16 MFMA row tiles per wave); 8 waves split the
// centers in 16-wide slabs.  X tile lives in LDS with a row stride of
// ldsStride doubles (== 2 mod 32: conflict-free ds_read_b64 A fragments).
template <int BM>
__global__ __launch_bounds__(kAssignThreads, 1) void k_kmeans_assign(
    const double* __restrict__ X, const double* __restrict__ xnorm, int64_t n, int d, int d4,
    int ldsStride, const double* __restrict__ Ct, const double* __restrict__ C,
    const double* __restrict__ cnorm, int k, int kpad, double marginFac,
    int32_t* __restrict__ assign, double* __restrict__ cost, int32_t* __restrict__ slowList,
    unsigned int* __restrict__ slowCount, const int32_t* __restrict__ rowList,
    const unsigned int* __restrict__ rowCount) {
  constexpr int T = BM / 16;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  double* Xs = smem;                                   // BM x ldsStride
  double* xnS = Xs + BM * ldsStride;                   // BM
  double* mrg = xnS + BM;                              // kWaves x BM x 4

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // Row source: rows row0.. of X (full pass, one block per tile), or the
  // rows an earlier screen queued in rowList (grid-stride over its tiles).
  const int64_t nsrc = rowList ? (int64_t)*rowCount : n;
  for (int64_t blk = blockIdx.x; blk * BM < nsrc; blk += gridDim.x) {
#define CYC_GROW1(i) (rowList ? (int64_t)rowList[row0 + (i)] : row0 + (i))
  const int64_t row0 = blk * BM;
  const int rows = (int)min<int64_t>(BM, nsrc - row0);

  // Stage the BM x d block of X (zero padded to d4 and BM).
  {
    const int total = rows * d;  // < 2^31: BM * d <= 64 * 1216
    for (int e = tid; e < total; e += kAssignThreads) {
      int r = e / d, c = e - r * d;
      Xs[r * ldsStride + c] = X[CYC_GROW1(r) * d + c];
    }
    for (int e = tid; e < BM * d4; e += kAssignThreads) {
      int r = e / d4, c = e - r * d4;
      if (r >= rows || c >= d) Xs[r * ldsStride + c] = 0.0;
    }
    if (tid < BM) xnS[tid] = (tid < rows) ? xnorm[CYC_GROW1(tid)] : 0.0;
  }
  __syncthreads();

  // Per-(row slot, lane) screening state in plain scalar arrays (static
  // indices only, so they stay in registers).
  float sL1[T * 4], sU1[T * 4], sL2[T * 4];
  int sI1[T * 4];
#pragma unroll
  for (int q = 0; q < T * 4; ++q) {
    sL1[q] = sU1[q] = sL2[q] = __builtin_inff();
    sI1[q] = -1;
  }
  unsigned poison = 0;  // bit (4t + r): a NaN reached this slot
  const double* arow = Xs + (lane & 15) * ldsStride + (lane >> 4);
  cyc_double4 acc[T];

  // Screening update for one finished 16-center slab (centers nb .. nb+15).
#define CYC_EPILOGUE(NB, CN)                                                   \
  do {                                                                         \
    const int c_ = (NB) + (lane & 15);                                         \
    if (c_ < k) {                                                              \
      const double cn_ = (CN);                                                 \
      const double cn2_ = cn_ * cn_;                                           \
      _Pragma("unroll") for (int t = 0; t < T; ++t) {                          \
        _Pragma("unroll") for (int r = 0; r < 4; ++r) {                        \
          const int q = 4 * t + r;                                             \
          const double xn = xnS[t * 16 + (lane >> 4) + 4 * r];                 \
          const double approx = (xn * xn + cn2_) - 2.0 * acc[t][r];            \
          const double sm = xn + cn_;                                          \
          const double M = (sm * sm) * marginFac;                              \
          const double L = approx - M, U = approx + M;                         \
          if (!(L == L) || !(U == U)) poison |= 1u << q;                       \
          if (L < sL1[q]) {                                                    \
            sL2[q] = sL1[q];                                                   \
            sL1[q] = f_down(L);                                                \
            sU1[q] = f_up(U);                                                  \
            sI1[q] = c_;                                                       \
          } else if (L < sL2[q]) {                                             \
            sL2[q] = f_down(L);                                                \
          }                                                                    \
        }                                                                      \
      }                                                                        \
    }                                                                          \
  } while (0)

  const int nslabs = (kpad - wave * 16 + kWaves * 16 - 1) / (kWaves * 16);
  if ((d4 & 15) == 0) {
    // Flat software pipeline over (slab, 16-dim group) steps: the B fragments
    // of step i+1 are in flight while step i's 4 x T MFMAs run.  Two named
    // register buffers keep every index static.
    const int G = d4 / 16;
    const int total = nslabs * G;
    double cn = 0.0;
    double b0[4], b1[4];
#define CYC_LOADB(B, I)                                                             \
  do {                                                                              \
    const int nb_ = wave * 16 + ((I) / G) * (kWaves * 16);                          \
    const double* bc_ = Ct + (int64_t)(((I) % G) * 16 + (lane >> 4)) * kpad + nb_ + \
                        (lane & 15);                                                \
    _Pragma("unroll") for (int s = 0; s < 4; ++s) B[s] = bc_[(int64_t)(s * 4) * kpad]; \
  } while (0)
#define CYC_COMPUTE(B, I)                                                           \
  do {                                                                              \
    const int g_ = (I) % G;                                                         \
    const int nb_ = wave * 16 + ((I) / G) * (kWaves * 16);                          \
    if (g_ == 0) {                                                                  \
      _Pragma("unroll") for (int t = 0; t < T; ++t) acc[t] = cyc_double4{0.0, 0.0, 0.0, 0.0}; \
      const int c0_ = nb_ + (lane & 15);                                            \
      cn = c0_ < k ? cnorm[c0_] : 0.0;                                              \
    }                                                                               \
    _Pragma("unroll") for (int s = 0; s < 4; ++s) {                                 \
      _Pragma("unroll") for (int t = 0; t < T; ++t) {                               \
        const double a_ = arow[t * 16 * ldsStride + g_ * 16 + s * 4];               \
        acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a_, B[s], acc[t], 0, 0, 0);   \
      }                                                                             \
    }                                                                               \
    if (g_ == G - 1) CYC_EPILOGUE(nb_, cn);                                         \
  } while (0)
    if (total > 0) CYC_LOADB(b0, 0);
    for (int i = 0; i < total; i += 2) {
      if (i + 1 < total) CYC_LOADB(b1, i + 1);
      CYC_COMPUTE(b0, i);
      if (i + 2 < total) CYC_LOADB(b0, i + 2);
      if (i + 1 < total) CYC_COMPUTE(b1, i + 1);
    }
#undef CYC_LOADB
#undef CYC_COMPUTE
  } else {
    for (int nb = wave * 16; nb < kpad; nb += kWaves * 16) {
#pragma unroll
      for (int t = 0; t < T; ++t) acc[t] = cyc_double4{0.0, 0.0, 0.0, 0.0};
      const double* bcol = Ct + (int64_t)(lane >> 4) * kpad + nb + (lane & 15);
      for (int kb = 0; kb < d4; kb += 4) {
        const double b = bcol[(int64_t)kb * kpad];
#pragma unroll
        for (int t = 0; t < T; ++t) {
          const double a = arow[t * 16 * ldsStride + kb];
          acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[t], 0, 0, 0);
        }
      }
      const int c = nb + (lane & 15);
      CYC_EPILOGUE(nb, c < k ? cnorm[c] : 0.0);
    }
  }
#undef CYC_EPILOGUE

  // Reduce each slot over the 16 lanes that hold the same row.
#pragma unroll
  for (int t = 0; t < T; ++t) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int q = 4 * t + r;
      Slot S{sL1[q], sU1[q], sL2[q], sI1[q]};
#pragma unroll
      for (int m = 1; m < 16; m <<= 1) {
        float oL1 = __shfl_xor(S.L1, m), oU1 = __shfl_xor(S.U1, m), oL2 = __shfl_xor(S.L2, m);
        int oI1 = __shfl_xor(S.I1, m);
        slot_merge(S, oL1, oU1, oL2, oI1);
      }
      sL1[q] = S.L1;
      sU1[q] = S.U1;
      sL2[q] = S.L2;
      sI1[q] = S.I1;
    }
  }
#pragma unroll
  for (int m = 1; m < 16; m <<= 1) poison |= __shfl_xor(poison, m);

  if ((lane & 15) == 0) {
#pragma unroll
    for (int t = 0; t < T; ++t) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = t * 16 + (lane >> 4) + 4 * r;
        double* m = mrg + ((size_t)wave * BM + row) * 4;
        const int q = 4 * t + r;
        m[0] = sL1[q];
        m[1] = sU1[q];
        m[2] = ((poison >> q) & 1u) ? -__builtin_inf() : (double)sL2[q];
        m[3] = (double)sI1[q];
      }
    }
  }
  __syncthreads();

  // One lane per row: merge the 8 waves, then decide or queue.
  if (tid < rows) {
    const int row = tid;
    Slot S{__builtin_inff(), __builtin_inff(), __builtin_inff(), -1};
    for (int w = 0; w < kWaves; ++w) {
      const double* m = mrg + ((size_t)w * BM + row) * 4;
      slot_merge(S, (float)m[0], (float)m[1], (float)m[2], (int)m[3]);
    }
    const int64_t grow = CYC_GROW1(row);
    if (S.I1 >= 0 && S.L2 > S.U1) {
      // Exact fastSquaredDistance(centers(I1), point) = Vectors.sqdist(c, x)
      // (when the caller wants per-row costs; the Lloyd path computes them
      // in k_chunk_sums).
      if (cost) {
        const double* crow = C + (int64_t)S.I1 * d;
        const double* xrow = Xs + row * ldsStride;
        double s = 0.0;
        for (int j = 0; j < d; ++j) {
          double sc = dsub(crow[j], xrow[j]);
          s = dadd(s, dmul(sc, sc));
        }
        cost[grow] = s;
      }
      assign[grow] = S.I1;
    } else {
      unsigned slot = atomicAdd(slowCount, 1u);
      slowList[slot] = (int32_t)grow;
    }
  }
  __syncthreads();   // LDS is restaged by the next tile
  }
#undef CYC_GROW1
}

// Second-generation assign kernel (the default when d4 % 32 == 0 and the
// center norms fit in LDS):
//   - per (row slot, lane) only the lower bounds L1 (best), L2 (second) in
//     fp32 rounded down and the best index; the upper bound of the best
//     center is rebuilt at the end as next_up(L1) + 2 M(best) from its norm,
//     which is >= its true upper bound, so certification stays conservative;
//   - branch-free epilogue (selects), center norms read from LDS (no global
//     load that would force a vmcnt(0) drain of the B prefetch);
//   - B fragments for 32 dims (8 MFMA k-steps) ping-pong between two named
//     register sets, one step ahead.
template <int BM>
__global__ __launch_bounds__(kAssignThreads, 1) void k_kmeans_assign2(
    const double* __restrict__ X, const double* __restrict__ xnorm, int64_t n, int d, int d4,
    int ldsStride, const double* __restrict__ Ct, const double* __restrict__ C,
    const double* __restrict__ cnorm, int k, int kpad, double marginFac,
    int32_t* __restrict__ assign, double* __restrict__ cost, int32_t* __restrict__ slowList,
    unsigned int* __restrict__ slowCount, const int32_t* __restrict__ rowList,
    const unsigned int* __restrict__ rowCount) {
  constexpr int T = BM / 16;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  double* Xs = smem;                      // BM x ldsStride
  double* xnS = Xs + BM * ldsStride;      // BM
  double* mrg = xnS + BM;                 // kWaves x BM x 4
  double* cnS = mrg + kWaves * BM * 4;    // kpad center norms
  double* xqS = cnS + kpad;               // BM: xn^2 (1 - 2 fac)
  // Row source: rows row0.. of X (full pass, one block per tile), or the
  // rows queued in rowList by the bf16 screen (grid-stride over its tiles).
  const int64_t nsrc = rowList ? (int64_t)*rowCount : n;
  for (int64_t blk = blockIdx.x; blk * BM < nsrc; blk += gridDim.x) {
#define CYC_GROW(i) (rowList ? (int64_t)rowList[row0 + (i)] : row0 + (i))
  // Margin M' = 2 fac (|x|^2 + |c|^2) >= fac (|x| + |c|)^2, so the lower bound
  // is L = (xq + cq) - 2 x.c with xq = |x|^2 (1 - 2 fac), cq likewise.
  const double fac2 = 2.0 * marginFac;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform (SGPR)
  const int64_t row0 = blk * BM;
  const int rows = (int)min<int64_t>(BM, nsrc - row0);
  {
    const int total = rows * d;
    for (int e = tid; e < total; e += kAssignThreads) {
      int r = e / d, c = e - r * d;
      Xs[r * ldsStride + c] = X[CYC_GROW(r) * d + c];
    }
    for (int e = tid; e < BM * d4; e += kAssignThreads) {
      int r = e / d4, c = e - r * d4;
      if (r >= rows || c >= d) Xs[r * ldsStride + c] = 0.0;
    }
    if (tid < BM) {
      const double xn = (tid < rows) ? xnorm[CYC_GROW(tid)] : 0.0;
      xnS[tid] = xn;
      xqS[tid] = (xn * xn) * (1.0 - fac2);
    }
    for (int c = tid; c < kpad; c += kAssignThreads) cnS[c] = c < k ? cnorm[c] : 0.0;
  }
  __syncthreads();
  // B fragments through a buffer descriptor: per-lane byte offset constant,
  // the (group, k-step, slab) part in an SGPR soffset -> no VALU address math.
  const auto ctR = __builtin_amdgcn_make_buffer_rsrc((void*)Ct, (short)0, d4 * kpad * 8,
                                                     0x00020000);
  const int laneOff = ((lane >> 4) * kpad + (lane & 15)) * 8;

  float sL1[T * 4], sL2[T * 4];
  int sI1[T * 4];
#pragma unroll
  for (int q = 0; q < T * 4; ++q) {
    sL1[q] = sL2[q] = __builtin_inff();
    sI1[q] = -1;
  }
  unsigned poison = 0;
  const double* arow = Xs + (lane & 15) * ldsStride + (lane >> 4);
  cyc_double4 acc[T];
  const int G = d4 / 32;
  const int nslabs = (kpad - wave * 16 + kWaves * 16 - 1) / (kWaves * 16);
  const int total = nslabs * G;
  double b0[8], b1[8];

#define CYC_LOADB(B, I)                                                              \
  do {                                                                               \
    const int nb_ = wave * 16 + ((I) / G) * (kWaves * 16);                           \
    const int so_ = ((((I) % G) * 32) * kpad + nb_) * 8;                             \
    _Pragma("unroll") for (int s = 0; s < 8; ++s)                                    \
      B[s] = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(          \
          ctR, laneOff, so_ + s * 32 * kpad, 0));                                    \
  } while (0)
#define CYC_COMPUTE(B, I)                                                            \
  do {                                                                               \
    const int g_ = (I) % G;                                                          \
    if (g_ == 0) {                                                                   \
      _Pragma("unroll") for (int t = 0; t < T; ++t) acc[t] = cyc_double4{0.0, 0.0, 0.0, 0.0}; \
    }                                                                                \
    _Pragma("unroll") for (int s = 0; s < 8; ++s) {                                  \
      _Pragma("unroll") for (int t = 0; t < T; ++t) {                                \
        const double a_ = arow[t * 16 * ldsStride + g_ * 32 + s * 4];                \
        acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a_, B[s], acc[t], 0, 0, 0);    \
      }                                                                              \
    }                                                                                \
    if (g_ == G - 1) {                                                               \
      const int c_ = wave * 16 + ((I) / G) * (kWaves * 16) + (lane & 15);            \
      const double cn_ = cnS[c_];                                                    \
      const double cq_ = (cn_ * cn_) * (1.0 - fac2);                                 \
      const bool cok_ = c_ < k;                                                      \
      _Pragma("unroll") for (int t = 0; t < T; ++t) {                                \
        _Pragma("unroll") for (int r = 0; r < 4; ++r) {                              \
          const int q = 4 * t + r;                                                   \
          const double xq = xqS[t * 16 + (lane >> 4) + 4 * r];                       \
          const double L = (xq + cq_) - (acc[t][r] + acc[t][r]);                      \
          poison |= (cok_ && !(L == L)) ? (1u << q) : 0u;                            \
          const float fL = (float)L;   /* f32 rounding mode is toward -inf here */   \
          const bool lt = cok_ && fL < sL1[q];                                       \
          const float l2 = cok_ ? fminf(sL2[q], fL) : sL2[q];                        \
          sL2[q] = lt ? sL1[q] : l2;                                                 \
          sI1[q] = lt ? c_ : sI1[q];                                                 \
          sL1[q] = lt ? fL : sL1[q];                                                 \
        }                                                                            \
      }                                                                              \
    }                                                                                \
  } while (0)
  // MODE.FP_ROUND single-precision bits [1:0] = 2 (toward -inf): every
  // (float) conversion of a lower bound in the loop rounds down.
  __builtin_amdgcn_s_setreg(0x801, 2);
  if (total > 0) CYC_LOADB(b0, 0);
  for (int i = 0; i < total; i += 2) {
    if (i + 1 < total) CYC_LOADB(b1, i + 1);
    CYC_COMPUTE(b0, i);
    if (i + 2 < total) CYC_LOADB(b0, i + 2);
    if (i + 1 < total) CYC_COMPUTE(b1, i + 1);
  }
  __builtin_amdgcn_s_setreg(0x801, 0);   // back to round-to-nearest-even
#undef CYC_LOADB
#undef CYC_COMPUTE

  // Reduce each slot over the 16 lanes that hold the same row.
#pragma unroll
  for (int q = 0; q < T * 4; ++q) {
#pragma unroll
    for (int m = 1; m < 16; m <<= 1) {
      const float oL1 = __shfl_xor(sL1[q], m), oL2 = __shfl_xor(sL2[q], m);
      const int oI1 = __shfl_xor(sI1[q], m);
      const float hi = fmaxf(sL1[q], oL1);
      sL2[q] = fminf(hi, fminf(sL2[q], oL2));
      const bool take = oL1 < sL1[q] || (oL1 == sL1[q] && oI1 >= 0 && (sI1[q] < 0 || oI1 < sI1[q]));
      sI1[q] = take ? oI1 : sI1[q];
      sL1[q] = take ? oL1 : sL1[q];
    }
  }
#pragma unroll
  for (int m = 1; m < 16; m <<= 1) poison |= __shfl_xor(poison, m);
  if ((lane & 15) == 0) {
#pragma unroll
    for (int t = 0; t < T; ++t) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int q = 4 * t + r;
        double* m = mrg + ((size_t)wave * BM + t * 16 + (lane >> 4) + 4 * r) * 4;
        m[0] = sL1[q];
        m[1] = ((poison >> q) & 1u) ? -__builtin_inf() : (double)sL2[q];
        m[2] = (double)sI1[q];
      }
    }
  }
  __syncthreads();

  if (tid < rows) {
    const int row = tid;
    float L1 = __builtin_inff(), L2 = __builtin_inff();
    int I1 = -1;
    for (int w = 0; w < kWaves; ++w) {
      const double* m = mrg + ((size_t)w * BM + row) * 4;
      const float oL1 = (float)m[0], oL2 = (float)m[1];
      const int oI1 = (int)m[2];
      const float hi = fmaxf(L1, oL1);
      L2 = fminf(hi, fminf(L2, oL2));
      if (oL1 < L1 || (oL1 == L1 && oI1 >= 0 && (I1 < 0 || oI1 < I1))) {
        L1 = oL1;
        I1 = oI1;
      }
    }
    const int64_t grow = CYC_GROW(row);
    bool decided = false;
    if (I1 >= 0 && L1 == L1 && L1 < __builtin_inff()) {
      const double xn = xnS[row], cn = cnS[I1];
      const double M = (xn * xn + cn * cn) * fac2;
      const double U = (double)(-ulp_down(-L1)) + 2.0 * M * (1.0 + 0x1p-40);
      decided = (double)L2 > U;
    }
    if (decided) {
      if (cost) {
        const double* crow = C + (int64_t)I1 * d;
        const double* xrow = Xs + row * ldsStride;
        double s = 0.0;
        for (int j = 0; j < d; ++j) {
          double sc = dsub(crow[j], xrow[j]);
          s = dadd(s, dmul(sc, sc));
        }
        cost[grow] = s;
      }
      assign[grow] = I1;
    } else {
      unsigned slot = atomicAdd(slowCount, 1u);
      slowList[slot] = (int32_t)grow;
    }
  }
  __syncthreads();   // LDS is restaged by the next tile
  }
#undef CYC_GROW
}

// ---------------------------------------------------- bf16x3 screen (tier 1)
// Third-generation assign (the default where it fits): the screen's dot
// products x.c run on the bf16 matrix cores instead of fp64 ones, 32x the
// MFMA rate, with a rigorous error bound; fp64 only decides.
//
// Split every value v (fp64) into v = vh + vl + ev with vh = bf16(v),
// vl = bf16(v - vh) (the subtraction is exact), |ev| <= 2^-16 |v| (1.0001).
// Then s = xh.ch + xl.ch + xh.cl (three bf16 products per element, f32
// accumulation: v_mfma_f32_16x16x32_bf16 over K = 3 d32) satisfies
//   |x.c - s| <= E = eps (|x|^2 + |c|^2) / 2 + tau,
//   eps = 3.1 * 2^-16 (split) + 2 * 1.03 * (3 d32 + 64) * 2^-23 (f32 sums of
//         up to 3 d32 terms, any faithful/directed rounding, 2x headroom)
//         + 2^-20,
// using sum|x_i||c_i| <= |x||c| <= (|x|^2 + |c|^2)/2, and tau = 2^-58 for
// bf16 / f32 underflow (values are capped at |v| <= 2^56: a row with
// |x| > 2^56 or a NaN goes to the fp64 tier, and a center beyond the cap
// turns the screen off for the launch).  Lower bound of every distance:
//   L_j = xq + cq_j - 2 s_j,  xq = |x|^2 (1 - eps) - 2 tau,  cq = |c|^2 (1 - eps),
// computed with f32 rounding toward -inf (MODE register) so it stays a lower
// bound; the best center's upper bound is L1 + (2 eps + 2^-20)(|x|^2 + |c|^2)
// + 4 tau.  A row whose second-smallest lower bound exceeds that is decided
// exactly as in the fp64 screen (k_kmeans_assign2) and gets the sequential
// fp64 sqdist; every other row is queued for the fp64 screen.
//
// Tiling: 64 rows per workgroup (4 waves, two workgroups per CU), the rows'
// bf16 hi / lo images in LDS; each wave owns every 4th 16-center tile and
// streams its centers' pre-split B fragments (1 KiB per wave-load) from L2,
// TB tiles at a time, each fragment feeding 4 row tiles.
typedef __bf16 cyc_bf16x8 __attribute__((ext_vector_type(8)));
typedef float cyc_float4 __attribute__((ext_vector_type(4)));

constexpr int kS3Waves = 4;
constexpr int kS3Threads = kS3Waves * 64;
constexpr int kS3BM = 64;

__device__ __forceinline__ void split_bf16(double v, unsigned short& h, unsigned short& l) {
  const __bf16 hb = (__bf16)(float)v;
  const double r = v - (double)(float)hb;   // exact: hb is within 2^-8 |v| of v
  const __bf16 lb = (__bf16)(float)r;
  h = __builtin_bit_cast(unsigned short, hb);
  l = __builtin_bit_cast(unsigned short, lb);
}

// Centers -> B fragments of v_mfma_f32_16x16x32_bf16 (lane l of 16-center tile
// ct, k-step ks holds centers ct*16 + (l & 15), dims ks*32 + 8 (l >> 4) + 0..7),
// hi image then lo image per (ct, ks): Cb[((ct KS + ks) 2 + part) 64 + l].
// cq[c] = |c|^2 (1 - eps) rounded down (+inf for padding); screenOk cleared if
// a center is beyond the 2^56 cap or not finite.
__global__ void k_center_split(const double* __restrict__ C, const double* __restrict__ cnorm,
                               int k, int d, int KS, int ktp, double omE, uint4* __restrict__ Cb,
                               float* __restrict__ cq, int* __restrict__ screenOk) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t total = (int64_t)ktp * KS * 64;
  if (idx < total) {
    const int lane = (int)(idx & 63);
    const int64_t t = idx >> 6;
    const int ks = (int)(t % KS), ct = (int)(t / KS);
    const int c = ct * 16 + (lane & 15), j0 = ks * 32 + 8 * (lane >> 4);
    unsigned short h[8], l[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int j = j0 + e;
      split_bf16((c < k && j < d) ? C[(int64_t)c * d + j] : 0.0, h[e], l[e]);
    }
    uint4 ph, pl;
    ph.x = h[0] | ((unsigned)h[1] << 16); ph.y = h[2] | ((unsigned)h[3] << 16);
    ph.z = h[4] | ((unsigned)h[5] << 16); ph.w = h[6] | ((unsigned)h[7] << 16);
    pl.x = l[0] | ((unsigned)l[1] << 16); pl.y = l[2] | ((unsigned)l[3] << 16);
    pl.z = l[4] | ((unsigned)l[5] << 16); pl.w = l[6] | ((unsigned)l[7] << 16);
    Cb[((t * 2) + 0) * 64 + lane] = ph;
    Cb[((t * 2) + 1) * 64 + lane] = pl;
  }
  if (idx < (int64_t)ktp * 16) {
    const int c = (int)idx;
    if (c < k) {
      const double cn = cnorm[c];
      if (!(cn <= 0x1p56)) atomicAnd(screenOk, 0);
      cq[c] = f_down((cn * cn) * omE);
    } else {
      cq[c] = __builtin_inff();
    }
  }
}

template <int TB>
__global__ __launch_bounds__(kS3Threads, 2) void k_kmeans_assign3(
    const double* __restrict__ X, const double* __restrict__ xnorm, int64_t n, int d, int KS,
    const uint4* __restrict__ Cb, const float* __restrict__ cq, int ktp,
    const int* __restrict__ screenOk, const double* __restrict__ C,
    const double* __restrict__ cnorm, double omE, double tauL,
    double facU, double tauU, int32_t* __restrict__ assign, double* __restrict__ cost,
    int32_t* __restrict__ list, unsigned int* __restrict__ listCount) {
  constexpr int BM = kS3BM, TA = BM / 16, W = kS3Waves;
  extern __shared__ __attribute__((aligned(16))) uint4 smem3[];
  const int SA = KS * 4 + 1;                       // 16-byte chunks per row (+1 pad)
  uint4* Ah = smem3;                               // BM x SA: bf16 hi image
  uint4* Al = Ah + BM * SA;                        // BM x SA: bf16 lo image
  float* mL1 = (float*)(Al + BM * SA);             // W x BM
  float* mL2 = mL1 + W * BM;                       // W x BM
  int* mI1 = (int*)(mL2 + W * BM);                 // W x BM
  float* xqS = (float*)(mI1 + W * BM);             // BM
  int* exI = (int*)(xqS + BM);                     // BM: decided center or -1
  double* Xd = (double*)smem3;                     // exact phase: 32 x (d + 1), over Ah/Al

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t row0 = (int64_t)blockIdx.x * BM;
  const int rows = (int)min<int64_t>(BM, n - row0);
  if (*screenOk == 0) {
    if (tid < rows) {
      const unsigned slot = atomicAdd(listCount, 1u);
      list[slot] = (int32_t)(row0 + tid);
    }
    return;
  }
  // Stage: one 8-element chunk per thread-step, split into the two images.
  const int chunks = KS * 4;
  for (int e = tid; e < BM * chunks; e += kS3Threads) {
    const int r = e / chunks, ch = e - r * chunks;
    const double* src = X + (row0 + r) * d;
    unsigned short h[8], l[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int j = ch * 8 + q;
      split_bf16((r < rows && j < d) ? src[j] : 0.0, h[q], l[q]);
    }
    uint4 ph, pl;
    ph.x = h[0] | ((unsigned)h[1] << 16); ph.y = h[2] | ((unsigned)h[3] << 16);
    ph.z = h[4] | ((unsigned)h[5] << 16); ph.w = h[6] | ((unsigned)h[7] << 16);
    pl.x = l[0] | ((unsigned)l[1] << 16); pl.y = l[2] | ((unsigned)l[3] << 16);
    pl.z = l[4] | ((unsigned)l[5] << 16); pl.w = l[6] | ((unsigned)l[7] << 16);
    Ah[r * SA + ch] = ph;
    Al[r * SA + ch] = pl;
  }
  if (tid < BM) {
    const double xn = tid < rows ? xnorm[row0 + tid] : 0.0;
    xqS[tid] = (xn <= 0x1p56) ? f_down((xn * xn) * omE - tauL) : -__builtin_inff();
  }
  __syncthreads();

  float sL1[TA * 4], sL2[TA * 4];
  int sI1[TA * 4];
#pragma unroll
  for (int q = 0; q < TA * 4; ++q) {
    sL1[q] = sL2[q] = __builtin_inff();
    sI1[q] = -1;
  }
  const uint4* ah = Ah + (lane & 15) * SA + (lane >> 4);
  const uint4* al = Al + (lane & 15) * SA + (lane >> 4);
  const int groups = ktp / (W * TB);
  const int total = groups * KS;
  cyc_float4 acc[TA][TB];
  uint4 bh0[TB], bl0[TB], bh1[TB], bl1[TB];
  float cqv[TB];

  // tile tb of group g of this wave: ct = (g TB + tb) W + wave
#define CYC_LOADB3(BH, BL, I)                                                        \
  do {                                                                               \
    const int g_ = (I) / KS, ks_ = (I) - g_ * KS;                                    \
    _Pragma("unroll") for (int tb = 0; tb < TB; ++tb) {                              \
      const int ct_ = (g_ * TB + tb) * W + wave;                                     \
      const uint4* p_ = Cb + ((size_t)(ct_ * KS + ks_) * 2) * 64 + lane;             \
      BH[tb] = p_[0];                                                                \
      BL[tb] = p_[64];                                                               \
    }                                                                                \
  } while (0)
#define CYC_COMPUTE3(BH, BL, I)                                                      \
  do {                                                                               \
    const int g_ = (I) / KS, ks_ = (I) - g_ * KS;                                    \
    if (ks_ == 0) {                                                                  \
      _Pragma("unroll") for (int tb = 0; tb < TB; ++tb) {                            \
        cqv[tb] = cq[((g_ * TB + tb) * W + wave) * 16 + (lane & 15)];                \
        _Pragma("unroll") for (int ta = 0; ta < TA; ++ta)                            \
          acc[ta][tb] = cyc_float4{0.f, 0.f, 0.f, 0.f};                              \
      }                                                                              \
    }                                                                                \
    _Pragma("unroll") for (int ta = 0; ta < TA; ++ta) {                              \
      const cyc_bf16x8 xh_ = __builtin_bit_cast(cyc_bf16x8, ah[ta * 16 * SA + ks_ * 4]); \
      const cyc_bf16x8 xl_ = __builtin_bit_cast(cyc_bf16x8, al[ta * 16 * SA + ks_ * 4]); \
      _Pragma("unroll") for (int tb = 0; tb < TB; ++tb) {                            \
        const cyc_bf16x8 ch_ = __builtin_bit_cast(cyc_bf16x8, BH[tb]);               \
        const cyc_bf16x8 cl_ = __builtin_bit_cast(cyc_bf16x8, BL[tb]);               \
        acc[ta][tb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xh_, ch_, acc[ta][tb], 0, 0, 0); \
        acc[ta][tb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xl_, ch_, acc[ta][tb], 0, 0, 0); \
        acc[ta][tb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xh_, cl_, acc[ta][tb], 0, 0, 0); \
      }                                                                              \
    }                                                                                \
    if (ks_ == KS - 1) {                                                             \
      _Pragma("unroll") for (int tb = 0; tb < TB; ++tb) {                            \
        const int c_ = ((g_ * TB + tb) * W + wave) * 16 + (lane & 15);               \
        _Pragma("unroll") for (int ta = 0; ta < TA; ++ta) {                          \
          _Pragma("unroll") for (int r = 0; r < 4; ++r) {                            \
            const int q = 4 * ta + r;                                                \
            const float L = (xqS[ta * 16 + 4 * (lane >> 4) + r] + cqv[tb]) -         \
                            2.0f * acc[ta][tb][r];                                   \
            const bool lt = L < sL1[q];                                              \
            const float l2 = fminf(sL2[q], L);                                       \
            sL2[q] = lt ? sL1[q] : l2;                                               \
            sI1[q] = lt ? c_ : sI1[q];                                               \
            sL1[q] = lt ? L : sL1[q];                                                \
          }                                                                          \
        }                                                                            \
      }                                                                              \
    }                                                                                \
  } while (0)
  // MODE.FP_ROUND single-precision bits [1:0] = 2 (toward -inf) for the
  // bounds (and the f32 accumulation, which the error bound allows).
  __builtin_amdgcn_s_setreg(0x801, 2);
  if (total > 0) CYC_LOADB3(bh0, bl0, 0);
  for (int i = 0; i < total; i += 2) {
    if (i + 1 < total) CYC_LOADB3(bh1, bl1, i + 1);
    CYC_COMPUTE3(bh0, bl0, i);
    if (i + 2 < total) CYC_LOADB3(bh0, bl0, i + 2);
    if (i + 1 < total) CYC_COMPUTE3(bh1, bl1, i + 1);
  }
  __builtin_amdgcn_s_setreg(0x801, 0);
#undef CYC_LOADB3
#undef CYC_COMPUTE3

  // Reduce each slot over the 16 lanes (columns) that hold the same row.
#pragma unroll
  for (int q = 0; q < TA * 4; ++q) {
#pragma unroll
    for (int m = 1; m < 16; m <<= 1) {
      const float oL1 = __shfl_xor(sL1[q], m), oL2 = __shfl_xor(sL2[q], m);
      const int oI1 = __shfl_xor(sI1[q], m);
      const float hi = fmaxf(sL1[q], oL1);
      sL2[q] = fminf(hi, fminf(sL2[q], oL2));
      const bool take = oL1 < sL1[q] || (oL1 == sL1[q] && oI1 >= 0 && (sI1[q] < 0 || oI1 < sI1[q]));
      sI1[q] = take ? oI1 : sI1[q];
      sL1[q] = take ? oL1 : sL1[q];
    }
  }
  if ((lane & 15) == 0) {
#pragma unroll
    for (int ta = 0; ta < TA; ++ta) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int q = 4 * ta + r, row = ta * 16 + 4 * (lane >> 4) + r;
        mL1[wave * BM + row] = sL1[q];
        mL2[wave * BM + row] = sL2[q];
        mI1[wave * BM + row] = sI1[q];
      }
    }
  }
  __syncthreads();
  if (tid < BM) {
    const int row = tid;
    float L1 = __builtin_inff(), L2 = __builtin_inff();
    int I1 = -1;
    for (int w = 0; w < W; ++w) {
      const float oL1 = mL1[w * BM + row], oL2 = mL2[w * BM + row];
      const int oI1 = mI1[w * BM + row];
      const float hi = fmaxf(L1, oL1);
      L2 = fminf(hi, fminf(L2, oL2));
      if (oL1 < L1 || (oL1 == L1 && oI1 >= 0 && (I1 < 0 || oI1 < I1))) {
        L1 = oL1;
        I1 = oI1;
      }
    }
    bool decided = false;
    if (row < rows && I1 >= 0 && L1 > -__builtin_inff() && L1 < __builtin_inff()) {
      const double xn = xnorm[row0 + row], cn = cnorm[I1];
      const double U = (double)L1 + facU * (xn * xn + cn * cn) + tauU;
      decided = (double)L2 > U;
    }
    exI[row] = -1;
    if (row < rows) {
      if (decided) {
        exI[row] = I1;
      } else {
        const unsigned slot = atomicAdd(listCount, 1u);
        list[slot] = (int32_t)(row0 + row);
      }
    }
  }
  __syncthreads();
  if (!cost) {
    if (tid < rows && exI[tid] >= 0) assign[row0 + tid] = exI[tid];
    return;
  }
  // Exact phase: the decided rows' sequential fp64 sqdist, 32 rows at a time
  // staged (coalesced, second read of the tile, from L2 / MALL) over the
  // images' LDS.
  for (int half = 0; half < BM / 32; ++half) {
    const int r0 = half * 32, nr = min(32, rows - r0);
    if (nr <= 0) break;
    for (int e = tid; e < nr * d; e += kS3Threads) {
      const int r = e / d, c = e - r * d;
      Xd[r * (d + 1) + c] = X[(row0 + r0 + r) * d + c];
    }
    __syncthreads();
    if (tid < nr && exI[r0 + tid] >= 0) {
      const int I1 = exI[r0 + tid];
      const double* crow = C + (int64_t)I1 * d;
      const double* xrow = Xd + tid * (d + 1);
      double s = 0.0;
      for (int j = 0; j < d; ++j) {
        const double sc = dsub(crow[j], xrow[j]);
        s = dadd(s, dmul(sc, sc));
      }
      assign[row0 + r0 + tid] = I1;
      cost[row0 + r0 + tid] = s;
    }
    __syncthreads();
  }
}

// The exact tier for a short queue (<= kExactCap rows, the usual few): the
// distances of one row to all k centers spread over ceil(k / 256)
// workgroups -- one thread per center, the same sequential sqdist as
// k_assign_exact -- into dist (kExactCap x kpad), then one wave per row
// replays the reference loop over them (k_exact_replay).  One workgroup per
// row streamed all k centers' coordinates through a single CU (~2 MB at
// k = 1024, d = 256: ~80 us for one row); spread over workgroups the queue
// finishes in a few microseconds.  A longer queue takes k_assign_exact.
constexpr int kExactCap = 512;

__global__ __launch_bounds__(256) void k_exact_dist(const double* __restrict__ X, int d,
                                                    const double* __restrict__ Ct, int kpad, int k,
                                                    const int32_t* __restrict__ slowList,
                                                    const unsigned int* __restrict__ slowCount,
                                                    double* __restrict__ dist) {
  __shared__ double xs[1280];
  const unsigned cnt = *slowCount;
  const unsigned idx = blockIdx.y;
  if (cnt > (unsigned)kExactCap || idx >= cnt) return;
  const int tid = threadIdx.x;
  const int c = blockIdx.x * 256 + tid;
  const int64_t r = slowList[idx];
  const double* x = X + r * d;
  const bool xl = d <= 1280;
  if (xl)
    for (int j = tid; j < d; j += 256) xs[j] = x[j];
  __syncthreads();
  const double* xv = xl ? xs : x;
  double acc = 0.0;
  // 16 dimensions' loads out before their adds (the adds are sequential)
  for (int j0 = 0; j0 < d; j0 += 16) {
    double cv[16];
#pragma unroll
    for (int jj = 0; jj < 16; ++jj)
      cv[jj] = (j0 + jj < d && c < k) ? Ct[(int64_t)(j0 + jj) * kpad + c] : 0.0;
#pragma unroll
    for (int jj = 0; jj < 16; ++jj) {
      if (j0 + jj < d) {
        const double sc = dsub(cv[jj], xv[j0 + jj]);
        acc = dadd(acc, dmul(sc, sc));
      }
    }
  }
  if (c < k) dist[(int64_t)idx * kpad + c] = acc;
}

__global__ __launch_bounds__(64) void k_exact_replay(const double* __restrict__ X,
                                                     const double* __restrict__ xnorm, int d,
                                                     int kpad, const double* __restrict__ cnorm,
                                                     int k, const double* __restrict__ stats,
                                                     const int32_t* __restrict__ slowList,
                                                     const unsigned int* __restrict__ slowCount,
                                                     const double* __restrict__ dist,
                                                     int32_t* __restrict__ assign,
                                                     double* __restrict__ cost, int exactNorm) {
  const unsigned cnt = *slowCount;
  const unsigned idx = blockIdx.x;
  if (cnt > (unsigned)kExactCap || idx >= cnt) return;
  const int lane = threadIdx.x;
  const int64_t r = slowList[idx];
  const bool ns = stats == nullptr;
  // the reference's Vectors.norm in index order when the caller's norms are
  // the row image's (k_assign_exact)
  double xn = 0.0;
  if (exactNorm) {
    if (lane == 0) xn = seq_norm2(X + r * d, d);
    xn = __shfl(xn, 0);
  } else {
    xn = xnorm[r];
  }
  const double* dds = dist + (int64_t)idx * kpad;
  double best = __builtin_inf();
  int bi = 0;
  bool done = false;
  int first = 0;
  if (!ns) {
    best = dds[0];                      // :286
    done = best < stats[0];             // :287
    first = 1;
  }
  for (int i0 = first; !done && i0 < k; i0 += 64) {
    const int i = i0 + lane;
    const bool valid = i < k;
    double lb = __builtin_inf(), sii = 0.0, dd = 0.0;
    if (valid) {
      const double nd = dsub(cnorm[i], xn);     // :294-295
      lb = dmul(nd, nd);
      sii = ns ? 0.0 : stats[iut(i, i)];
      dd = dds[i];
    }
    int pos = 0;
    for (;;) {
      const bool visit = valid && lane >= pos && lb < best && (ns || stats[iut(i, bi)] < best);
      const bool brk = !ns && visit && dd < sii;
      const bool ev = visit && (brk || dd < best);
      const unsigned long long m = __ballot(ev);
      if (!m) break;
      const int f = __ffsll((long long)m) - 1;
      best = __shfl(dd, f);
      bi = i0 + f;
      if (__shfl((int)brk, f)) {
        done = true;
        break;
      }
      pos = f + 1;
    }
  }
  if (lane == 0) {
    assign[r] = bi;
    if (cost) cost[r] = best;
  }
}

// EuclideanDistanceMeasure.findClosest with statistics, DistanceMeasure.scala:
// 282-313, for the rows the screens could not decide.  One workgroup per
// queued row: the exact sequential sqdist (Vectors.scala:580-587, the same
// operation order as the reference) of every center, 1024 at a time, then
// the replay on one wave.  The reference loop visits centers in order; its
// state (bestDistance, bestIndex) changes only at an update, so the wave
// evaluates 64 consecutive centers at once against the current state: a
// ballot over the lanes whose center the loop would visit finds the first lane
// whose visit changes the state (a `return` at :303 or an update at :304-306),
// the state advances to it, and the lanes after it are re-evaluated against
// the new state (reusing the distances already computed).  Lanes before the
// first event have no side effect in the reference either, so the returned
// (index, distance) is the reference's, bit for bit; distances of centers the
// reference would not visit may be computed speculatively and are discarded.
constexpr int kExactChunk = 1024;   // centers whose distances one pass stages in LDS
constexpr int kExactX = 1280;       // widest row staged in LDS

__global__ __launch_bounds__(256) void k_assign_exact(
    const double* __restrict__ X, const double* __restrict__ xnorm, int d,
    const double* __restrict__ C, const double* __restrict__ Ct, int kpad,
    const double* __restrict__ cnorm, int k,
    const double* __restrict__ stats, const int32_t* __restrict__ slowList,
    const unsigned int* __restrict__ slowCount, int32_t* __restrict__ assign,
    double* __restrict__ cost, int exactNorm, unsigned int skipUpTo) {
  // One workgroup per listed row.  A distance is a pure function of (center,
  // row), so the workgroup first computes Vectors.sqdist(center, x) -- in
  // order j = 0..d-1 (Vectors.scala:580-587) -- for a chunk of 1024 centers
  // at once (thread t: centers t, t + 256, ..; center i read from the
  // transposed copy, coalesced over the threads), and wave 0 then replays the
  // reference loop's visits and events over them.
  __shared__ double xs[kExactX];
  __shared__ double dds[kExactChunk];
  __shared__ int doneS;
  __shared__ double xnS;
  const unsigned cnt = *slowCount;
  if (cnt <= skipUpTo) return;   // the split kernels took the queue
  const int tid = threadIdx.x, lane = tid & 63;
  // stats == nullptr: findClosest(centers, point) (:318-340), best from +inf
  const bool ns = stats == nullptr;
  for (unsigned idx = blockIdx.x; idx < cnt; idx += gridDim.x) {
    const int64_t r = slowList[idx];
    const double* x = X + r * d;
    __syncthreads();   // the previous row's reads of xs / dds / xnS are done
    const bool xl = d <= kExactX;
    if (xl)
      for (int j = tid; j < d; j += 256) xs[j] = x[j];
    const double* xv = xl ? xs : x;
    // exactNorm: the caller's norms are the row image's (any summation
    // order, for the screens' margins); the loop's prune needs the
    // reference's Vectors.norm, in index order (seq_norm2)
    if (exactNorm) {
      __syncthreads();
      if (tid == 0) xnS = seq_norm2(xv, d);
      __syncthreads();
    }
    const double xn = exactNorm ? xnS : xnorm[r];
    double best = __builtin_inf();   // wave 0's replay state
    int bi = 0;
    bool done = false;
    for (int c0 = 0; c0 < k; c0 += kExactChunk) {
      __syncthreads();   // xs written; the previous chunk's replay is done
      double acc[kExactChunk / 256];
#pragma unroll
      for (int u = 0; u < kExactChunk / 256; ++u) acc[u] = 0.0;
      // 16 dimensions' loads go out before their adds (the add chains are
      // sequential; the loads are not)
      for (int j0 = 0; j0 < d; j0 += 16) {
        double cv[16][kExactChunk / 256];
#pragma unroll
        for (int jj = 0; jj < 16; ++jj) {
          const double* row = Ct + (int64_t)(j0 + jj) * kpad + c0 + tid;
#pragma unroll
          for (int u = 0; u < kExactChunk / 256; ++u)
            cv[jj][u] = (j0 + jj < d && c0 + tid + 256 * u < k) ? row[256 * u] : 0.0;
        }
#pragma unroll
        for (int jj = 0; jj < 16; ++jj) {
          if (j0 + jj < d) {
            const double xj = xv[j0 + jj];
#pragma unroll
            for (int u = 0; u < kExactChunk / 256; ++u) {
              const double sc = dsub(cv[jj][u], xj);
              acc[u] = dadd(acc[u], dmul(sc, sc));
            }
          }
        }
      }
#pragma unroll
      for (int u = 0; u < kExactChunk / 256; ++u)
        if (c0 + tid + 256 * u < k) dds[tid + 256 * u] = acc[u];
      __syncthreads();
      if (tid < 64) {
        int first = c0;
        if (c0 == 0 && !ns) {
          best = dds[0];                      // :286
          done = best < stats[0];             // :287
          first = 1;
        }
        const int end = min(k, c0 + kExactChunk);
        for (int i0 = first; !done && i0 < end; i0 += 64) {
          const int i = i0 + lane;
          const bool valid = i < end;
          double lb = __builtin_inf(), sii = 0.0, dd = 0.0;
          if (valid) {
            const double nd = dsub(cnorm[i], xn);     // :294-295
            lb = dmul(nd, nd);
            sii = ns ? 0.0 : stats[iut(i, i)];
            dd = dds[i - c0];
          }
          int pos = 0;
          for (;;) {
            const bool visit = valid && lane >= pos && lb < best && (ns || stats[iut(i, bi)] < best);
            const bool brk = !ns && visit && dd < sii;
            const bool ev = visit && (brk || dd < best);
            const unsigned long long m = __ballot(ev);
            if (!m) break;
            const int f = __ffsll((long long)m) - 1;
            best = __shfl(dd, f);
            bi = i0 + f;
            if (__shfl((int)brk, f)) {
              done = true;
              break;
            }
            pos = f + 1;
          }
        }
        if (tid == 0) doneS = done;
      }
      __syncthreads();
      if (doneS) break;
    }
    if (tid == 0) {
      assign[r] = bi;
      if (cost) cost[r] = best;
    }
  }
}

}  // namespace

namespace cyc {
namespace kmfp64 {

namespace {

constexpr int kS3TB = 2;   // center tiles per wave group of k_kmeans_assign3

// Widest d that fits: 16 rows need (16 s + 16 + kWaves * 16 * 4) * 8 <= 160 KiB,
// s <= 1247; the strides == 2 (mod 32) below that are 1218 (d4 <= 1216) and
// 1250 (d4 >= 1220), so d <= 1216.
int pick_bm(int d4, int& stride, size_t& lds) {
  const int cands[3] = {64, 32, 16};
  const int maxbm = 64;
  for (int bm : cands) {
    if (bm > maxbm) continue;
    int s = d4 + ((2 - d4 % 32) + 32) % 32;  // stride == 2 (mod 32)
    size_t bytes = ((size_t)bm * s + bm + (size_t)kWaves * bm * 4) * sizeof(double);
    if (bytes <= 160 * 1024) {
      stride = s;
      lds = bytes;
      return bm;
    }
  }
  return 0;
}

template <int BM>
int launch_assign_bm(const Sizing& s, const double* X, const double* xnorm, int64_t n,
                     const double* C, const double* cnorm, const double* ct, int32_t* assign,
                     double* cost, int32_t* slowList, unsigned int* slowCount, hipStream_t st,
                     const int32_t* rowList, const unsigned int* rowCount) {
  static bool attr_set = false;
  if (!attr_set) {
    CYC_HIP(hipFuncSetAttribute((const void*)k_kmeans_assign<BM>,
                                hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    CYC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_kmeans_assign2<BM>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    attr_set = true;
  }
  const double marginFac = (double)(s.d + 16) * 0x1p-46;
  // list mode (rows queued by an earlier screen): persistent grid over the queue
  const int64_t blocks = rowList ? std::min<int64_t>((n + BM - 1) / BM, 1024) : (n + BM - 1) / BM;
  cyc::KernelTimer timer(rowList ? "k_kmeans_assign_fp64" : "k_kmeans_assign", st);
  if (s.variant == 2 || s.variant == 3)
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_kmeans_assign2<BM>), dim3((unsigned)blocks),
                       dim3(kAssignThreads), s.assignLds2, st, X, xnorm, n, s.d, s.d4,
                       s.ldsStride2, ct, C, cnorm, s.k, s.kpad, marginFac, assign, cost, slowList,
                       slowCount, rowList, rowCount);
  else
    hipLaunchKernelGGL(k_kmeans_assign<BM>, dim3((unsigned)blocks), dim3(kAssignThreads),
                       s.assignLds, st, X, xnorm, n, s.d, s.d4, s.ldsStride, ct, C, cnorm, s.k,
                       s.kpad, marginFac, assign, cost, slowList, slowCount, rowList, rowCount);
  CYC_LAUNCH_CHECK("k_kmeans_assign");
  return CYC_OK;
}

}  // namespace

Sizing sizing(int d, int k, int want) {
  Sizing s;
  s.d = d;
  s.k = k;
  s.d4 = (int)cyc::round_up(d, 4);
  s.kpad = (int)cyc::round_up(k, 16);
  s.bm = pick_bm(s.d4, s.ldsStride, s.assignLds);
  s.ldsStride2 = s.d4 + 1;
  s.assignLds2 = s.assignLds + sizeof(double) * ((size_t)s.kpad + s.bm) -
                 sizeof(double) * (size_t)s.bm * (s.ldsStride - s.ldsStride2);
  s.variant = ((s.d4 % 32) == 0 && s.assignLds2 <= 160 * 1024) ? 2 : 1;
  // bf16x3 screen in front of the fp64 one where its LDS tile fits
  s.ks3 = (int)((d + 31) / 32);
  s.lds3 = (size_t)2 * kS3BM * (s.ks3 * 4 + 1) * 16 + (size_t)kS3Waves * kS3BM * 12 +
           (size_t)kS3BM * 8;
  const bool fits3 = s.variant == 2 && s.lds3 <= 160 * 1024;
  if (fits3) s.variant = 3;
  if (want == 1 || (s.d4 % 32 == 0 && s.assignLds2 <= 160 * 1024 && want >= 2 && want <= 3 &&
                    (want != 3 || fits3)))
    s.variant = want;
  s.ktp3 = (int)cyc::round_up((k + 15) / 16, kS3Waves * kS3TB);
  const double d32 = 32.0 * s.ks3;
  const double eps = 3.1 * 0x1p-16 + 2.0 * 1.03 * (3.0 * d32 + 64.0) * 0x1p-23 + 0x1p-20;
  const double tau = 0x1p-58;
  s.omE3 = 1.0 - eps;
  s.tauL3 = 2.0 * tau;
  s.facU3 = (2.0 * eps + 0x1p-20) * (1.0 + 0x1p-20);
  s.tauU3 = 4.0 * tau;
  return s;
}

int launch_assign(const Sizing& s, int bm, const double* X, const double* xnorm, int64_t n,
                  const double* C, const double* cnorm, const double* ct, int32_t* assign,
                  double* cost, int32_t* slowList, unsigned int* slowCount, hipStream_t st,
                  const int32_t* rowList, const unsigned int* rowCount) {
  switch (bm) {
    case 64:
      return launch_assign_bm<64>(s, X, xnorm, n, C, cnorm, ct, assign, cost, slowList, slowCount,
                                  st, rowList, rowCount);
    case 32:
      return launch_assign_bm<32>(s, X, xnorm, n, C, cnorm, ct, assign, cost, slowList, slowCount,
                                  st, rowList, rowCount);
    default:
      return launch_assign_bm<16>(s, X, xnorm, n, C, cnorm, ct, assign, cost, slowList, slowCount,
                                  st, rowList, rowCount);
  }
}

int launch_assign3(const Sizing& s, const double* X, const double* xnorm, int64_t n,
                   const double* C, const double* cnorm, void* cb3, float* cq3, int* ok3,
                   int32_t* assign, double* cost, int32_t* list3, unsigned int* list3Count,
                   hipStream_t st) {
  static bool attr_set = false;
  if (!attr_set) {
    CYC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_kmeans_assign3<kS3TB>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    attr_set = true;
  }
  CYC_HIP(hipMemsetAsync(list3Count, 0, sizeof(unsigned int), st));
  CYC_HIP(hipMemsetAsync(ok3, 1, sizeof(int), st));
  const int64_t tot = (int64_t)s.ktp3 * s.ks3 * 64;
  hipLaunchKernelGGL(k_center_split, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, C,
                     cnorm, s.k, s.d, s.ks3, s.ktp3, s.omE3, (uint4*)cb3, cq3, ok3);
  CYC_LAUNCH_CHECK("k_center_split");
  cyc::KernelTimer timer("k_kmeans_assign", st);
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_kmeans_assign3<kS3TB>),
                     dim3((unsigned)((n + kS3BM - 1) / kS3BM)), dim3(kS3Threads), s.lds3, st, X,
                     xnorm, n, s.d, s.ks3, (const uint4*)cb3, (const float*)cq3, s.ktp3,
                     (const int*)ok3, C, cnorm, s.omE3, s.tauL3, s.facU3, s.tauU3, assign, cost,
                     list3, list3Count);
  CYC_LAUNCH_CHECK("k_kmeans_assign3");
  return CYC_OK;
}

int launch_exact(const Sizing& s, const double* X, const double* xnorm, int64_t n,
                 const double* C, const double* cnorm, const double* ct, const double* statsArg,
                 const int32_t* slowList, const unsigned int* slowCount, DeviceBuffer& exactDist,
                 int32_t* assign, double* cost, bool approxNorm, int64_t known, bool allowSplit,
                 hipStream_t st) {
  cyc::KernelTimer timer("k_kmeans_exact", st);
  const int k = s.k, kpad = s.kpad;
  const bool split = allowSplit && s.d <= 1280 && (known < 0 || known <= kExactCap);
  if (split) {
    int rc;
    if ((rc = exactDist.reserve(sizeof(double) * (size_t)kExactCap * kpad))) return rc;
    const unsigned rowsMax = (unsigned)std::min<int64_t>(known < 0 ? n : known, kExactCap);
    hipLaunchKernelGGL(k_exact_dist, dim3((unsigned)((k + 255) / 256), rowsMax), dim3(256), 0, st,
                       X, s.d, ct, kpad, k, slowList, slowCount, (double*)exactDist.ptr);
    CYC_LAUNCH_CHECK("k_exact_dist");
    hipLaunchKernelGGL(k_exact_replay, dim3(rowsMax), dim3(64), 0, st, X, xnorm, s.d, kpad, cnorm,
                       k, statsArg, slowList, slowCount, (const double*)exactDist.ptr, assign,
                       cost, approxNorm ? 1 : 0);
    CYC_LAUNCH_CHECK("k_exact_replay");
    if (known >= 0) return CYC_OK;
  }
  // the long queue (or no split): one workgroup per row, grid-stride
  const unsigned grid = known >= 0 ? (unsigned)std::min<int64_t>(known, 4096)
                                   : (unsigned)std::min<int64_t>((n + 3) / 4, 2048);
  hipLaunchKernelGGL(k_assign_exact, dim3(grid), dim3(256), 0, st, X, xnorm, s.d, C, ct, kpad,
                     cnorm, k, statsArg, slowList, slowCount, assign, cost, approxNorm ? 1 : 0,
                     split ? (unsigned)kExactCap : 0u);
  CYC_LAUNCH_CHECK("k_assign_exact");
  return CYC_OK;
}

}  // namespace kmfp64
}  // namespace cyc
