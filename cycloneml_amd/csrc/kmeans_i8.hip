// kmeans_i8.hip -- tier 1 of the KMeans assignment (EuclideanDistanceMeasure.
// findClosest, mllib/clustering/DistanceMeasure.scala:282-313) on gfx950: an
// exact-integer screen of the dot products x.c on the i8 matrix cores
// (v_mfma_i32_16x16x64_i8), with a rigorous error bound; fp64 only decides.
//
// Fixed-point split.  A row x (fp64) gets the exponent ex with every
// |x_j| 2^(7-ex) <= 127 and is written as three int8 limbs per element,
//   x_j 2^(7-ex) = a_j + b_j / 2^7 + c_j / 2^14 + r_j / 2^14,  |r_j| <= 1/2,
// a = rint(u), b = rint(128 (u - a)), c = rint(128 (128 (u - a) - b)): every
// step is exact in fp64, |a| <= 127, |b|, |c| <= 64, so |x_j - xh_j| <= 2^(ex-22).
// Centers use ONE exponent ec for the launch.  Then
//   xh.ch = 2^(ex+ec-14) (S1 + S2 / 2^7 + S3 / 2^14 + dropped),
//   S1 = a.a', S2 = a.b' + b.a', S3 = a.c' + b.b' + c.a'   (6 i8 MFMAs / 64 dims)
// accumulated EXACTLY in int32 (d <= 512: |128 S1 + S2| < 2^31), and
//   |x.c - 2^(ex+ec-14)(S1 + S2/2^7 + S3/2^14)|
//      <= Ax |c|_1 + Ac |xh|_1 + 1.004 d 2^22 Ax Ac,   Ax = 2^(ex-22), Ac = 2^(ec-22)
// (quantization of both operands, plus the dropped b.c', c.b', c.c' terms,
// |b|,|c| <= 64).  AM-GM with one balance mu > 0 per launch makes the bound
// separable: <= fx + gc with
//   fx = mu Ax^2 / 2 + |xh|_1^2 / (2 mu) + 0.502 d 2^22 Ax^2,   gc likewise.
// So every distance obeys
//   |x|^2 + |c|^2 - 2 s - 2 (fx + gc) <= |x - c|^2 <= |x|^2 + |c|^2 - 2 s + 2 (fx + gc),
//   2 s = 2^(ex+ec-20) (128 S1 + S2 + S3 / 2^7).
// The kernel keeps, per row, the two smallest of L'_c = cq_c - 2 s (f32,
// MODE rounding toward -inf; cq_c = |c|^2 (1 - epsF) - 2 gc rounded down) and
// the index of the smallest; f32 conversion / fma errors are below
// 2^-21 (|x|^2 + |c|^2) and absorbed by epsF = 2^-20.  A row is certified
// when  L'_2 - L'_1 > 4 (fx + g_1) + 2 epsF (|x|^2 + |c_1|^2) + slack: then
// its best center's upper bound lies below every other center's lower
// bound, the reference's pruned loop (whose prunes only skip centers that
// cannot win) returns the same index, and the row is assigned here.  Every
// other row (ties, near ties, NaN/Inf, |x_j| >= 2^50) is queued for the fp64
// MFMA screen and, behind it, the reference loop itself.
//
// The margin is ~1e-6 relative (vs ~2.5e-4 for a bf16 x3 split with f32
// accumulation), so practically only true near-ties reach the fp64 tiers.
//
// Data flow: the row image (3 D bytes per row, D = 64 ceil(d/64)) is built
// once per fit (rows_quantize; the reference likewise caches the rows with
// their norms once per fit, KMeans.scala:263-270); the center image (3 D
// bytes per center, ~0.75 MB at k=1024, d=256) is rebuilt per iteration and
// stays in each XCD's L2 while every workgroup streams it.
//
// This unit: the screen kernels and the driver that strings the stages
// together (screen).  The other stages: kmeans_i8_rows.hip (row image),
// kmeans_i8_centers.hip (center image, center-only kernels),
// kmeans_i8_cands.hip (candidate tiers, re-check), kmeans_i8_lists.hip (shard
// compaction, carried-bounds filter); kmeans_i8_dev.hpp is what they share.
#include "kmeans_i8_dev.hpp"

#include <initializer_list>

// tools/probe/screen1_probe.hip builds the one-limb pass with parts removed
// to time them (results then meaningless): bits 2 = no center DMA / waits,
// 4 = no reduction / certification tail, 8 = every wave's rows read from row
// 0 (no HBM stream).  0 in the library.
#ifndef CYC_PROBE_MODE
#define CYC_PROBE_MODE 0
#endif

namespace cyc {
namespace km8 {
namespace {

typedef int v16i __attribute__((ext_vector_type(16)));

__device__ __forceinline__ v4i as_v4i(uint4 u) { return __builtin_bit_cast(v4i, u); }

// BM = 64 rows per workgroup (4 row tiles), 4 waves; wave w owns the 16-center
// tiles w, w+4, w+8, ...  The row image lives in LDS with a row stride of
// 12 KS + 2 16-byte chunks (== 2 mod 4: conflict-free ds_read_b128 fragment
// reads); B fragments come from L2 one 64-dim step ahead.
template <int KS>
__global__ __launch_bounds__(256, KS <= 4 ? 3 : 2) void k_screen(
    const uint4* __restrict__ Xq, const int2* __restrict__ meta, const double* __restrict__ xnorm,
    int64_t n, int d, const uint4* __restrict__ Cb, const float* __restrict__ cq,
    const double* __restrict__ g, const double* __restrict__ cnorm,
    const CenterParams* __restrict__ prm, int ktp, int32_t* __restrict__ assign,
    int32_t* __restrict__ list, unsigned int* __restrict__ listCount) {
  constexpr int BM = kBM, W = kWaves, CH = 12 * KS, STR = CH + 2;
  extern __shared__ __attribute__((aligned(16))) uint4 smem8[];
  uint4* As = smem8;                          // BM x STR chunks
  int* exS = (int*)(As + BM * STR);           // BM
  // after the main loop the row image is dead: the per-wave slot minima
  // reuse it (3 KB), so d <= 256 fits three workgroups per CU
  float* mL1 = (float*)As;                    // W x BM
  float* mL2 = mL1 + W * BM;                  // W x BM
  int* mI1 = (int*)(mL2 + W * BM);            // W x BM

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t row0 = (int64_t)blockIdx.x * BM;
  const int rows = (int)min<int64_t>(BM, n - row0);
  const CenterParams P = *prm;
  if (!P.ok) {
    if (tid < rows) list[atomicAdd(listCount, 1u)] = (int32_t)(row0 + tid);
    return;
  }
  {
    // every load in flight before the first LDS write (3 KS chunks per thread)
    constexpr int PER = BM * CH / 256;
    const uint4* src = Xq + row0 * CH;
    const int lim = rows * CH;
    v4u st[PER];
#pragma unroll
    for (int i = 0; i < PER; ++i)
      st[i] = __builtin_nontemporal_load((const v4u*)(src + min(tid + 256 * i, lim - 1)));
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int e = tid + 256 * i, r = e / CH, ch = e - r * CH;
      As[r * STR + ch] = e < lim ? make_uint4(st[i].x, st[i].y, st[i].z, st[i].w)
                                 : make_uint4(0u, 0u, 0u, 0u);
    }
    if (tid < BM) exS[tid] = tid < rows ? meta[row0 + tid].x : INT_MIN;
  }
  __syncthreads();

  // Per row slot q = 4 ta + r (row ta*16 + 4 (lane >> 4) + r): 2^(ex+ec-20).
  float F1[16];
#pragma unroll
  for (int ta = 0; ta < 4; ++ta) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int ex = exS[ta * 16 + 4 * (lane >> 4) + r];
      F1[4 * ta + r] = ex == INT_MIN ? 0.0f : __builtin_ldexpf(1.0f, ex + P.ec - 20);
    }
  }
  float sL1[16], sL2[16];
  int sI1[16];
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    sL1[q] = sL2[q] = __builtin_inff();
    sI1[q] = -1;
  }
  const uint4* ap = As + (lane & 15) * STR + (lane >> 4);
  const int nT = ktp / W;
  const uint4* cb = Cb + (size_t)wave * KS * 192 + lane;
  const size_t tstride = (size_t)W * KS * 192;
  // Register rings, all indices static after unrolling: B fragments one
  // 64-dim step ahead (KS is even, so a tile always starts on B0), A
  // fragments one (step, row tile) ahead (4 per step, so always on A0).
  v4i B0[3], B1[3], A0[3], A1[3];
#define CYC_LDB(DST, P)                                  \
  do {                                                   \
    DST[0] = as_v4i((P)[0]);                             \
    DST[1] = as_v4i((P)[64]);                            \
    DST[2] = as_v4i((P)[128]);                           \
  } while (0)
#define CYC_LDA(DST, KS_, TA_)                           \
  do {                                                   \
    const uint4* a_ = ap + (TA_) * 16 * STR + (KS_) * 4; \
    DST[0] = as_v4i(a_[0]);                              \
    DST[1] = as_v4i(a_[4 * KS]);                         \
    DST[2] = as_v4i(a_[8 * KS]);                         \
  } while (0)
#define CYC_MM(ACC, A, B)                                                    \
  do {                                                                       \
    ACC[0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[0], B[0], ACC[0], 0, 0, 0); \
    ACC[1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[0], B[1], ACC[1], 0, 0, 0); \
    ACC[1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[1], B[0], ACC[1], 0, 0, 0); \
    ACC[2] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[0], B[2], ACC[2], 0, 0, 0); \
    ACC[2] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[1], B[1], ACC[2], 0, 0, 0); \
    ACC[2] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[2], B[0], ACC[2], 0, 0, 0); \
  } while (0)
  // one (step, row tile): prefetch the next A, then 6 MFMAs
#define CYC_TA(KS_, TA_, AC, AN, BC)                                          \
  do {                                                                        \
    if ((TA_) < 3) CYC_LDA(AN, KS_, (TA_) + 1);                               \
    else CYC_LDA(AN, ((KS_) + 1 < KS ? (KS_) + 1 : 0), 0);                    \
    CYC_MM(acc[TA_], AC, BC);                                                 \
    __builtin_amdgcn_sched_group_barrier(0x100, 3, 0);                        \
    __builtin_amdgcn_sched_group_barrier(0x008, 6, 0);                        \
  } while (0)
#define CYC_KSTEP(KS_, BC, BN)                                                \
  do {                                                                        \
    CYC_LDB(BN, ((KS_) + 1 < KS ? cb + ((KS_) + 1) * 192 : cbn));             \
    __builtin_amdgcn_sched_group_barrier(0x020, 3, 0);                        \
    CYC_TA(KS_, 0, A0, A1, BC);                                               \
    CYC_TA(KS_, 1, A1, A0, BC);                                               \
    CYC_TA(KS_, 2, A0, A1, BC);                                               \
    CYC_TA(KS_, 3, A1, A0, BC);                                               \
  } while (0)
  CYC_LDB(B0, cb);
  CYC_LDA(A0, 0, 0);

  // MODE.FP_ROUND single precision = toward -inf (the L' are lower bounds)
  __builtin_amdgcn_s_setreg(0x801, 2);
  for (int t = 0; t < nT; ++t) {
    const float cqv = cq[(t * W + wave) * 16 + (lane & 15)];
    // next tile's B (the last tile re-reads its own: harmless, branch free)
    const uint4* cbn = cb + (t + 1 < nT ? tstride : 0);
    v4i acc[4][3];
#pragma unroll
    for (int ta = 0; ta < 4; ++ta)
#pragma unroll
      for (int s = 0; s < 3; ++s) acc[ta][s] = v4i{0, 0, 0, 0};
#pragma unroll
    for (int kp = 0; kp < KS; kp += 2) {
      CYC_KSTEP(kp, B0, B1);
      CYC_KSTEP(kp + 1, B1, B0);
    }
#undef CYC_KSTEP
#undef CYC_TA
#undef CYC_MM
#undef CYC_LDA
#undef CYC_LDB
    cb = cbn;
    const int c = (t * W + wave) * 16 + (lane & 15);
#pragma unroll
    for (int ta = 0; ta < 4; ++ta) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int q = 4 * ta + r;
        const int T = acc[ta][0][r] * 128 + acc[ta][1][r];
        const float V = __builtin_fmaf((float)acc[ta][2][r], 0x1p-7f, (float)T);
        const float L = __builtin_fmaf(-F1[q], V, cqv);
        // two smallest with sL1 <= sL2: the median of (sL1, sL2, L) is the
        // new second smallest
        const bool lt = L < sL1[q];
        sL2[q] = __builtin_amdgcn_fmed3f(sL1[q], sL2[q], L);
        sI1[q] = lt ? c : sI1[q];
        sL1[q] = __builtin_fminf(sL1[q], L);
      }
    }
  }
  __builtin_amdgcn_s_setreg(0x801, 0);

  // Reduce each slot over the 16 lanes (centers) that hold the same row.
#pragma unroll
  for (int q = 0; q < 16; ++q) {
#pragma unroll
    for (int m = 1; m < 16; m <<= 1) {
      const float oL1 = __shfl_xor(sL1[q], m), oL2 = __shfl_xor(sL2[q], m);
      const int oI1 = __shfl_xor(sI1[q], m);
      sL2[q] = __builtin_fminf(__builtin_fmaxf(sL1[q], oL1), __builtin_fminf(sL2[q], oL2));
      const bool take = oL1 < sL1[q] || (oL1 == sL1[q] && oI1 >= 0 && (sI1[q] < 0 || oI1 < sI1[q]));
      sI1[q] = take ? oI1 : sI1[q];
      sL1[q] = take ? oL1 : sL1[q];
    }
  }
  __syncthreads();   // every wave is done reading the row image (mL1.. alias it)
  if ((lane & 15) == 0) {
#pragma unroll
    for (int ta = 0; ta < 4; ++ta) {
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
  if (tid < rows) {
    const int row = tid;
    const int ex = exS[row];
    float L1 = __builtin_inff(), L2 = __builtin_inff();
    int I1 = -1;
#pragma unroll
    for (int w = 0; w < W; ++w) {
      const float oL1 = mL1[w * BM + row], oL2 = mL2[w * BM + row];
      const int oI1 = mI1[w * BM + row];
      L2 = __builtin_fminf(__builtin_fmaxf(L1, oL1), __builtin_fminf(L2, oL2));
      if (oL1 < L1 || (oL1 == L1 && oI1 >= 0 && (I1 < 0 || oI1 < I1))) {
        L1 = oL1;
        I1 = oI1;
      }
    }
    bool decided = false;
    if (ex != INT_MIN && I1 >= 0 && __builtin_isfinite(L1)) {
      const double xn = xnorm[row0 + row], cn = cnorm[I1];
      const double xx = xn * xn, cc = cn * cn;
      const double n1 = (double)__int_as_float(meta[row0 + row].y);
      const double fx = err_term(ex, n1, P.mu, d);
      const double l1 = (double)L1;
      const double M = (4.0 * (fx + g[I1]) + 2.0 * kEpsF * (xx + cc) +
                        0x1p-20 * (__builtin_fabs(l1) + cc + 2.0 * g[I1]) +
                        0x1p-24 * (2.0 * (xx + cc) + __builtin_fabs(l1) +
                                   __builtin_fmin(__builtin_fabs((double)L2), 0x1p120)) +
                        0x1p-90) *
                       (1.0 + 0x1p-30);
      // exact difference of two floats; L2 = +inf: no other real center
      decided = !__builtin_isfinite(L2) || ((double)L2 - l1) > M;
    }
    if (decided) {
      assign[row0 + row] = I1;
    } else {
      list[atomicAdd(listCount, 1u)] = (int32_t)(row0 + row);
    }
  }
}

// ---------------------------------------------------------------------------
// 32x32 form (d <= 256): v_mfma_i32_32x32x32_i8 holds the SIMD's issue for 8
// of its 32 cycles (the 16x16x64 form: 8 of 16), leaving room for the top-2
// epilogue (9 VALU per (row, center): ~3 per MFMA).
//
// One wave = 32 rows, held in REGISTERS in the MFMA A layout (lane l: row
// l & 31, dims 32 s + 16 (l >> 5) + 0..15 of substep s, three limbs: 96
// VGPRs at d = 256).  A workgroup of 4 waves (128 rows) sweeps every
// 32-center tile; each tile's B fragments (24 KiB at d = 256) are DMA'd
// into a ring of three LDS slots (global_load_lds, 1 KiB per wave-
// instruction, split over the waves, counted vmcnt + raw s_barrier so the
// next tile stays in flight) and read by conflict-free ds_read_b128.
// 252 VGPRs: two waves per SIMD (two workgroups per CU, 2 x 74.5 KB LDS).
// Measured at 10M x 256, k = 1024 (profiles/r02_kmeans_*): 14.4 ms per
// launch vs 14.0-15.4 for the 16x16x64 screen; PMC: 32 MFMA-busy cycles per
// MFMA, 53 % of the SIMD cycles at the 1.89 GHz the chip holds under this
// load.  Tried and slower: B fragments per wave straight from L2 (18.1 ms),
// one wave per SIMD with two accumulator sets so the epilogue of tile t
// interleaves tile t+1's MFMAs (18.1 ms), 8-wave workgroups (one tile load
// per 256 rows: 14.8-15.0 ms).
// B fragments: k_centers_pack32 (kmeans_i8_centers.hip).

// the largest of each row's per-lane values over its 32 lanes (the screens'
// register layout: lane (r, h) holds row (reg & 3) + 8 (reg >> 2) + 4 h of
// register reg): halving shuffles, then per row into out[32] (LDS)
__device__ __forceinline__ void rows_max32(int (&v)[16], int lane, int* out) {
#pragma unroll
  for (int lev = 0; lev < 4; ++lev) {
    const int half = 8 >> lev, m = 16 >> lev;
    const bool hi = (lane & m) != 0;
#pragma unroll
    for (int i = 0; i < half; ++i) {
      const int o = __shfl_xor(hi ? v[i] : v[i + half], m);
      v[i] = max(hi ? v[i + half] : v[i], o);
    }
  }
  v[0] = max(v[0], __shfl_xor(v[0], 1));
  if ((lane & 1) == 0) {
    const int q = (lane >> 1) & 15;
    out[(q & 3) + 8 * (q >> 2) + 4 * (lane >> 5)] = v[0];
  }
}

// One screen pass over 32-row groups.  LIMBS = 3: the exact-integer screen
// (S1, S2, S3: six MFMAs per 32-dim substep).  LIMBS = 2: the same over the
// a and b limbs only (S1, S2: three MFMAs), certified with err_term2 --
// config 2's rows certify 90 % of the time at this precision vs 99.9 % at
// three limbs, so the two-limb pass runs over every row and the three-limb
// pass only over its leftovers (LIST: rows taken from `rowsIn`, a device
// list of *rowsInCount row indices).  Both read the
// same center image (3 limb fragments per substep; LIMBS = 2 DMAs the first
// two) and write assign[] for certified rows, the rest to list.
// Two workgroups per CU; three for the two-limb pass (<= 168 VGPRs, LDS
// 3 x 49 KB at S = 8), measured 7 % faster than two.
// the one-limb pass screens a row whose exponent exceeds its wave's smallest
// by at most this much (larger shifts could overflow its 32-bit bounds)
constexpr int kShMax = 2;

template <int S, int W, int LIMBS, bool LIST>
__global__ __launch_bounds__(64 * W, W == 8 ? 2 : (LIMBS < 3 ? 12 : 8) / W) void k_screen32(
    const uint4* __restrict__ Xq, const int2* __restrict__ meta, const double* __restrict__ xnorm,
    int64_t n, int d, const uint4* __restrict__ Cb, const float* __restrict__ cq,
    const double* __restrict__ g, const double* __restrict__ cnorm,
    const CenterParams* __restrict__ prm, int ktp, const int32_t* __restrict__ rowsIn,
    const unsigned int* __restrict__ rowsInCount, int32_t* __restrict__ assign,
    int32_t* __restrict__ list, unsigned int* __restrict__ listCount,
    int32_t* __restrict__ candRows, int32_t* __restrict__ cands,
    unsigned int* __restrict__ candCount, unsigned int scap, float2* __restrict__ bnd) {
  constexpr int D = 32 * S, CH = 3 * D / 16;      // 16-byte chunks per image row
  // LIMBS = 1 takes two 32-center tiles per step (one barrier and one ring
  // slot per 64 centers: its tiles carry a third of the MFMAs)
  constexpr bool PAIR = LIMBS == 1;
  constexpr int FR = PAIR ? 2 * S : LIMBS * S;     // 1 KiB B fragments per ring step
  constexpr int TB = FR * 1024 + 256;              // tile slot: fragments, then 64 cq floats
  constexpr int G = FR / W;                        // fragment DMAs per wave per tile (+1: wave 0's cq)
  static_assert(FR % W == 0, "fragments split evenly over the waves");
  // ONE shared array (a second __shared__ object can make hipcc drain vmcnt
  // before every ds_read): three tile slots, reused for the final reduction.
  __shared__ __attribute__((aligned(16))) char lds[3 * TB];
  const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const CenterParams P = *prm;
  // any mu > 0 is valid; scaled with each limb count's quantum
  const double mu = LIMBS == 3 ? P.mu : LIMBS == 2 ? P.mu * 0x1p-7 : P.mu * 0x1p-14;
  // integer bounds (LIMBS < 3) in units F1 = 2^(ex + ec - SH): 2 s = F1 T
  constexpr int SH = LIMBS == 1 ? 13 : 20;
  // candidate sets per row: the two-limb pass's for the fp64 candidate pass
  // (kCandMax), the one-limb pass's for the two-limb refinement (kCand1)
  constexpr int CMAX = LIMBS == 1 ? kCand1 : kCandMax;
  const int64_t total = LIST ? (int64_t)*rowsInCount : n;
  // one group of 32 W rows (positions)
  auto group = [&](int64_t grp) {
  const int64_t pos0 = (grp * W + wave) * 32;        // first position of this wave
  // waves past the end still take part in every barrier (zero rows)
  const int rows = (int)max<int64_t>(0, min<int64_t>(32, total - pos0));
  // scap > 0: list / cand appends go to this group's shard (kmeans_i8.hpp)
  const unsigned shard = (unsigned)((grp * W + wave) % kShards);
  int32_t* const listS = scap ? list + (size_t)shard * scap : list;
  unsigned int* const listCountS = scap ? listCount + shard * kShardStride : listCount;
  int32_t* const candRowsS = scap && candRows ? candRows + (size_t)shard * scap : candRows;
  int32_t* const candsS = scap && cands ? cands + (size_t)shard * scap * CMAX : cands;
  unsigned int* const candCountS =
      scap && candCount ? candCount + shard * kShardStride : candCount;
  auto rowAt = [&](int i) -> int64_t {   // global row of position pos0 + i (i < rows)
    if constexpr (LIST) return rowsIn[pos0 + i];
    else return pos0 + i;
  };
  if (!P.ok) {   // uniform over the grid
    if (lane < rows) {
      listS[atomicAdd(listCountS, 1u)] = (int32_t)rowAt(lane);
      if (LIMBS == 1 && bnd) bnd[rowAt(lane)] = make_float2(-1.0f, -1.0f);
    }
    return;
  }
  // tile t -> slot t % 3: each wave DMAs fragments wave, wave + W, ... and the
  // tile's cq (all waves write the same 256 bytes); past the last tile the
  // last one is re-read into the free slot, so every wave always has exactly
  // G DMAs per tile in flight and one counted wait fits all tiles.
  const int nsteps = PAIR ? ktp / 2 : ktp;          // ktp is even
  auto issue = [&](int t, int slot) {
    if constexpr (PAIR && (CYC_PROBE_MODE & 2)) return;
    const int tt = t < nsteps ? t : nsteps - 1;
    char* dst = lds + slot * TB;
#pragma unroll
    for (int j = 0; j < FR / W; ++j) {
      const int f = wave + W * j;
      // PAIR: fragment f = limb a of substep f % S of tile 2 tt + f / S;
      // else substep f / LIMBS, limb f % LIMBS of tile tt
      const int tile = PAIR ? 2 * tt + f / S : tt;
      const int piece = PAIR ? (f % S) * 3 : (f / LIMBS) * 3 + f % LIMBS;
      const char* src = (const char*)Cb + (size_t)tile * (3 * S) * 1024 + lane * 16;
      __builtin_amdgcn_global_load_lds((const void*)(src + piece * 1024),
                                       (__attribute__((address_space(3))) void*)(dst + f * 1024),
                                       16, 0, 0);
    }
    if (wave == 0)   // the step's cq: 32 (lanes 32..63 repeat them) or PAIR's 64
      __builtin_amdgcn_global_load_lds(
          (const void*)(cq + (PAIR ? (size_t)tt * 64 + lane : (size_t)tt * 32 + r)),
          (__attribute__((address_space(3))) void*)(dst + FR * 1024), 4, 0, 0);
  };
  issue(0, 0);
  issue(1, 1);
  // A fragments of the wave's 32 rows, all substeps and limbs
  v4i A[S][LIMBS];
  const bool rowOk = r < rows;
  const int64_t myRow = rowOk ? rowAt(r) : 0;   // lane's row (row 0 exists: n > 0)
  {
    // loads from a valid row, zeroed after the load; the one-limb pass
    // with plain loads (3.40 -> 3.30 ms measured against nontemporal ones)
    const bool ok = rowOk;
    const uint4* src = Xq + ((PAIR && (CYC_PROBE_MODE & 8)) ? 0 : myRow) * CH + h;
#pragma unroll
    for (int s = 0; s < S; ++s)
#pragma unroll
      for (int L = 0; L < LIMBS; ++L) {
        const v4u* a = (const v4u*)(src + L * (D / 16) + 2 * s);
        const v4u t = PAIR ? *a : __builtin_nontemporal_load(a);
        A[s][L] = ok ? __builtin_bit_cast(v4i, t) : v4i{0, 0, 0, 0};
      }
  }
  // row of accumulator register reg: (reg & 3) + 8 (reg >> 2) + 4 h
  const int exr = rowOk ? meta[myRow].x : INT_MIN;
  // LIMBS = 3: per-row unit F1 = 2^(ex + ec - 20) of T in f32 bounds.
  // LIMBS = 2: integer bounds in the same units: L / F1 = Q - T with
  // Q = cq / F1 rounded, from one per-lane base per tile at the wave's
  // smallest exponent exmin, shifted right by sh = ex - exmin per row.
  float F1[16];
  int sh[16];
  int exmin = 0;
  if constexpr (LIMBS == 3) {
    const float f = exr == INT_MIN ? 0.0f : __builtin_ldexpf(1.0f, exr + P.ec - 20);
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) F1[reg] = __shfl(f, (reg & 3) + 8 * (reg >> 2) + 4 * h);
  } else {
    int e = exr == INT_MIN ? INT_MAX : exr;
#pragma unroll
    for (int m = 1; m < 32; m <<= 1) e = min(e, __shfl_xor(e, m));
    exmin = __builtin_amdgcn_readfirstlane(e == INT_MAX ? 0 : e);
    const int s0 = exr == INT_MIN ? 31 : min(exr - exmin, 31);
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) sh[reg] = __shfl(s0, (reg & 3) + 8 * (reg >> 2) + 4 * h);
  }
  // cq scaled to the units 2^(exmin + ec - SH)
  const float qscale = __builtin_ldexpf(1.0f, max(-160, min(160, SH - P.ec - exmin)));
  // |Q| clamp in those units: LIMBS = 1 keeps (Q << IB) in 31 bits
  constexpr float QCLAMP = LIMBS == 1 ? 0x1p25f : 0x1p30f;
  bool qbad = false;   // a cq below -QCLAMP units: the wave certifies nothing
  // LIMBS = 3: the two smallest f32 bounds; LIMBS = 2: the two largest
  // V = T - Q (the smallest L = -F1 V), tile index in the low IB bits
  float sL1[16], sL2[16];
  int sV1[16], sV2[16];
  int sI1[16];
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    sL1[q] = sL2[q] = __builtin_inff();
    sV1[q] = sV2[q] = INT_MIN;
    sI1[q] = -1;
  }
  // tile ct from its slot: LIMBS = 3: six limb products per substep,
  // LIMBS = 2: three; B fragments by conflict-free ds_read_b128
  auto tile = [&](int slot, v16i (&acc)[LIMBS]) {   // acc: initialised by the caller
    const v4i* B = (const v4i*)(lds + slot * TB) + lane;
    // (reading the B fragments a substep ahead measured no faster)
#pragma unroll
    for (int s = 0; s < S; ++s) {
      v4i Bc[LIMBS];
#pragma unroll
      for (int L = 0; L < LIMBS; ++L) Bc[L] = B[(LIMBS * s + L) * 64];
      const v4i B0 = Bc[0], B1 = Bc[LIMBS >= 2 ? 1 : 0];
      // (separating the two acc[1] products by sched_barrier measured 3 % slower)
      acc[0] = __builtin_amdgcn_mfma_i32_32x32x32_i8(A[s][0], B0, acc[0], 0, 0, 0);
      if constexpr (LIMBS >= 2) {
        acc[1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(A[s][0], B1, acc[1], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(A[s][1], B0, acc[1], 0, 0, 0);
      }
      if constexpr (LIMBS == 3) {
        const v4i B2 = Bc[2];
        acc[2] = __builtin_amdgcn_mfma_i32_32x32x32_i8(A[s][0], B2, acc[2], 0, 0, 0);
        acc[2] = __builtin_amdgcn_mfma_i32_32x32x32_i8(A[s][1], B1, acc[2], 0, 0, 0);
        acc[2] = __builtin_amdgcn_mfma_i32_32x32x32_i8(A[s][2], B0, acc[2], 0, 0, 0);
      }
    }
  };
  // LIMBS = 2 keeps the tile index in the low IB bits of V (moving it by
  // < 2^IB units either way, charged in the certification): a max and a med3
  // per (row, center) instead of a compare, a med3 and two selects.
  const int IB = 32 - __builtin_clz((unsigned)max(ktp - 1, 1));
  const unsigned IM = (1u << IB) - 1u;
  // LIMBS = 2, after the tile's MFMAs: acc[1] started at -Q
  int vzero;
  asm volatile("v_mov_b32 %0, 0" : "=v"(vzero));
  auto epi2 = [&](int ct, const v16i (&acc)[LIMBS]) {
    // ct in a VGPR (one v_and_or_b32 may read only one SGPR, the mask), by
    // a VALU add to an opaque zero: no inline asm in the loop, which would
    // split its scheduling region
    const unsigned ctv = (unsigned)(vzero + ct);
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      // T - Q (LIMBS = 1: acc[0] started at -Q)
      const int V = LIMBS == 1 ? acc[0][reg] : acc[0][reg] * 128 + acc[LIMBS - 1][reg];
      const int Ve = (int)(((unsigned)V & ~IM) | ctv);                  // ct < 2^IB
      sV2[reg] = max(min(sV1[reg], sV2[reg]), min(max(sV1[reg], sV2[reg]), Ve));   // v_med3_i32
      sV1[reg] = max(sV1[reg], Ve);
    }
  };
  auto epi = [&](int ct, float cqv, const v16i (&acc)[LIMBS]) {
    const int c = ct * 32 + r;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      if constexpr (LIMBS == 3) {
        const int T = acc[0][reg] * 128 + acc[1][reg];
        const float V = __builtin_fmaf((float)acc[2][reg], 0x1p-7f, (float)T);
        const float L = __builtin_fmaf(-F1[reg], V, cqv);
        const bool lt = L < sL1[reg];
        sL2[reg] = __builtin_amdgcn_fmed3f(sL1[reg], sL2[reg], L);
        sI1[reg] = lt ? c : sI1[reg];
        sL1[reg] = lt ? L : sL1[reg];   // L is never NaN: a select, no canonicalize
      }
    }
  };
  auto cq_of = [&](int slot, int half = 0) {
    return *(const float*)(lds + slot * TB + FR * 1024 + (half * 32 + r) * 4);
  };
  // tile t in `slot`: wait for this wave's DMAs of t (those of t + 1 may stay
  // in flight), barrier (every wave's part of t landed; every wave is past
  // t - 1, whose slot the DMAs of t + 2 now refill)
  auto arrive = [&](int t, int slot) {
    if constexpr (PAIR && (CYC_PROBE_MODE & 2)) {
      __builtin_amdgcn_s_barrier();
      return;
    }
    if (wave == 0) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(G + 1) : "memory");
    else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(G) : "memory");
    __builtin_amdgcn_s_barrier();
    issue(t + 2, slot == 0 ? 2 : slot - 1);
  };
  auto next_slot = [](int slot) { return slot == 2 ? 0 : slot + 1; };

  // MODE.FP_ROUND single precision = toward -inf (the L' are lower bounds)
  __builtin_amdgcn_s_setreg(0x801, 2);
  // (software-pipelining the epilogue beside the next tile's MFMAs needs a
  // second accumulator set: 193 VGPRs, two waves per SIMD, 4 % slower than
  // this form at 168 VGPRs and three waves per SIMD)
  int sl = 0;
  if constexpr (PAIR) {
    // The one-limb bounds in the units 2^(exmin + ec - SH) of the wave's
    // smallest exponent, shifted left by IB with the tile index in the low
    // bits: Ve = (T << (sh + IB)) + ((-Q << IB) + ct), one v_lshl_add_u32 per
    // (row, center) on an accumulator started at 0 (the -Q start value of
    // the two-limb form is gone, and Q needs no per-row rounding).
    // |T| < 2^22 (d <= 256), sh <= kShMax (rows past it are not screened),
    // |Q| <= 2^25: |Ve| < 2^31.
    int shIB[16];
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) shIB[reg] = min(sh[reg], kShMax) + IB;
    auto epi_reg = [&](int reg, int cpr, int T) {
      const int Ve = (int)(((unsigned)T << shIB[reg]) + (unsigned)cpr);
      sV2[reg] = max(min(sV1[reg], sV2[reg]), min(max(sV1[reg], sV2[reg]), Ve));   // v_med3_i32
      sV1[reg] = max(sV1[reg], Ve);
    };
    // Software-pipelined by hand: each gap between two MFMAs of one tile
    // carries the epilogue of 16 / S rows of the tile before (tile 2 st - 1's
    // beside 2 st's, across the barrier) and the B fragment of the next MFMA;
    // sched_barrier pins that order.  X1 starts as zero rows with cpr =
    // INT_MIN: an epilogue that changes no sV.
    constexpr int RPG = 16 / S;   // accumulator rows per MFMA gap
    static_assert(16 % S == 0, "the gaps split the 16 rows evenly");
    const v16i Z = {};
    v16i X0, X1 = Z;
    int cprPrev = INT_MIN;
    for (int st = 0; st < nsteps; ++st) {
      arrive(st, sl);
      // (-Q << IB) + ct of tiles 2 st and 2 st + 1
      int cpr[2];
#pragma unroll
      for (int hf = 0; hf < 2; ++hf) {
        const float pf = cq_of(sl, hf) * qscale;
        qbad |= pf < -QCLAMP;
        const int nb = -(int)__builtin_floorf(__builtin_fminf(pf, QCLAMP));
        cpr[hf] = (int)(((unsigned)nb << IB) + (unsigned)(vzero + 2 * st + hf));
      }
      // opaque: one register each, not re-associated into every element's add
      asm volatile("" : "+v"(cpr[0]), "+v"(cpr[1]));
      const v4i* B = (const v4i*)(lds + sl * TB) + lane;
      v4i Bn = B[0];
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int s = 0; s < S; ++s) {
        const v4i Bc = Bn;
        Bn = B[(s + 1) * 64];   // s = S - 1: tile 2 st + 1's first fragment
        X0 = __builtin_amdgcn_mfma_i32_32x32x32_i8(A[s][0], Bc, s == 0 ? Z : X0, 0, 0, 0);
#pragma unroll
        for (int q = RPG * s; q < RPG * (s + 1); ++q) epi_reg(q, cprPrev, X1[q]);
        __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
      for (int s = 0; s < S; ++s) {
        const v4i Bc = Bn;
        if (s + 1 < S) Bn = B[(S + s + 1) * 64];
        X1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(A[s][0], Bc, s == 0 ? Z : X1, 0, 0, 0);
#pragma unroll
        for (int q = RPG * s; q < RPG * (s + 1); ++q) epi_reg(q, cpr[0], X0[q]);
        __builtin_amdgcn_sched_barrier(0);
      }
      cprPrev = cpr[1];
      sl = next_slot(sl);
    }
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) epi_reg(reg, cprPrev, X1[reg]);
  }
  for (int ct = 0; ct < (PAIR ? 0 : ktp); ++ct) {
    v16i X[LIMBS];
    arrive(ct, sl);
    const float cqv = cq_of(sl);
    if constexpr (LIMBS < 3) {
      // -Q per row: ceil(floor(cq 2^k) / 2^sh) >= Q - 1 unit; cq above 2^30
      // units clamps (a smaller Q: still a lower bound)
      const float pf = cqv * qscale;   // exact (a power of two; round-down mode)
      qbad |= pf < -QCLAMP;
      const int nb = -(int)__builtin_floorf(__builtin_fminf(pf, QCLAMP));
      X[0] = v16i{};
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) X[LIMBS - 1][reg] = nb >> sh[reg];
      tile(sl, X);
      epi2(ct, X);
    } else {
#pragma unroll
      for (int L = 0; L < LIMBS; ++L) X[L] = v16i{};
      tile(sl, X);
      epi(ct, cqv, X);
    }
    sl = next_slot(sl);
  }
  __builtin_amdgcn_s_setreg(0x801, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the trailing re-read DMAs
  if constexpr (PAIR && (CYC_PROBE_MODE & 4)) {   // probe: no reduction / certification
    if (lane < rows) assign[rowAt(lane)] = sV1[lane & 15] ^ sV2[(lane + 1) & 15];
    return;
  }

  // LIMBS = 2: each lane's own best and second best (one center column per
  // lane) before the reduction merges them: the candidate sets below
  int cV1[16], cV2[16];
  if constexpr (LIMBS < 3) {
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      sI1[q] = (int)((unsigned)sV1[q] & IM) * 32 + r;
      cV1[q] = sV1[q];
      cV2[q] = sV2[q];
    }
  }
  // each row's (L1, L2, I1) over the 32 lanes (centers) of its half: every
  // xor step halves the registers a lane keeps (lanes with the step's bit
  // keep the upper half and send the lower), so 16 rows cost 8 + 4 + 2 + 1 + 1
  // shuffles per quantity.  Equal L1 from two centers leave L2 = L1, which
  // never certifies, so the merge needs no index tie-break.
  auto mergeL = [](float& L1, float& L2, int& I1, float oL1, float oL2, int oI1) {
    L2 = __builtin_fminf(__builtin_fmaxf(L1, oL1), __builtin_fminf(L2, oL2));
    I1 = oL1 < L1 ? oI1 : I1;
    L1 = __builtin_fminf(L1, oL1);
  };
  auto mergeV = [](int& V1, int& V2, int& I1, int oV1, int oV2, int oI1) {
    V2 = max(min(V1, oV1), max(V2, oV2));
    I1 = oV1 > V1 ? oI1 : I1;
    V1 = max(V1, oV1);
  };
#define CYC_REDUCE(K1, K2, MERGE)                                                   \
  _Pragma("unroll") for (int lev = 0; lev < 4; ++lev) {                             \
    const int half = 8 >> lev, m = 16 >> lev;                                       \
    const bool hi = (lane & m) != 0;                                                \
    _Pragma("unroll") for (int i = 0; i < half; ++i) {                              \
      const auto o1 = __shfl_xor(hi ? K1[i] : K1[i + half], m);                     \
      const auto o2 = __shfl_xor(hi ? K2[i] : K2[i + half], m);                     \
      const int oI1 = __shfl_xor(hi ? sI1[i] : sI1[i + half], m);                   \
      auto k1 = hi ? K1[i + half] : K1[i];                                          \
      auto k2 = hi ? K2[i + half] : K2[i];                                          \
      int I1 = hi ? sI1[i + half] : sI1[i];                                         \
      MERGE(k1, k2, I1, o1, o2, oI1);                                               \
      K1[i] = k1;                                                                   \
      K2[i] = k2;                                                                   \
      sI1[i] = I1;                                                                  \
    }                                                                               \
  }                                                                                 \
  MERGE(K1[0], K2[0], sI1[0], __shfl_xor(K1[0], 1), __shfl_xor(K2[0], 1),           \
        __shfl_xor(sI1[0], 1));
  if constexpr (LIMBS < 3) {
    CYC_REDUCE(sV1, sV2, mergeV)
  } else {
    CYC_REDUCE(sL1, sL2, mergeL)
  }
#undef CYC_REDUCE
  // lane holds row register q = lane bits 1..4
  // per-wave reduction area in the (now idle) slots: L1, L2, I1 x 32 rows
  __syncthreads();
  float* redL1 = (float*)lds + wave * 96;   // LIMBS = 2: the V1, V2 bits
  float* redL2 = redL1 + 32;
  int* redI1 = (int*)(redL1 + 64);
  if ((lane & 1) == 0) {
    const int q = (lane >> 1) & 15;
    const int row = (q & 3) + 8 * (q >> 2) + 4 * h;
    redL1[row] = LIMBS < 3 ? __int_as_float(sV1[0]) : sL1[0];
    redL2[row] = LIMBS < 3 ? __int_as_float(sV2[0]) : sL2[0];
    redI1[row] = sI1[0];
  }
  const bool waveBad = __builtin_amdgcn_ballot_w64(qbad) != 0;
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  bool want = false;   // LIMBS < 3: an undecided row for the candidate pass
  int thrV = 0;
  int64_t grow = 0;
  // LIMBS = 1 with bnd: the row's terms for its candidate rows' bound
  double bxx = 0.0, bfx = 0.0, benc = 0.0, bf1 = 0.0;
  int bsb = 0;
  if (lane < rows) {
    grow = rowAt(lane);
    const int2 mt = meta[grow];
    const int I1 = redI1[lane];
    // L1, L2 as fp64 (LIMBS < 3: -F1 V; V2 = INT_MIN: no second)
    double l1, l2, f1 = 0.0;
    int v1 = 0;
    bool clamped = false, shOk = true;
    int sb = 0;   // LIMBS = 1: the row's Ve = V 2^sb (+ index bits)
    if constexpr (LIMBS < 3) {
      f1 = __builtin_ldexp(1.0, mt.x + P.ec - SH);
      v1 = __float_as_int(redL1[lane]);
      int v2 = __float_as_int(redL2[lane]);
      if constexpr (LIMBS == 1) {
        // back to the row's units, floored (< 1 unit, inside enc below)
        const int shr = mt.x - exmin;
        shOk = shr >= 0 && shr <= kShMax;
        sb = min(max(shr, 0), kShMax) + IB;
        if (v1 != INT_MIN) v1 >>= sb;
        if (v2 != INT_MIN) v2 >>= sb;
      }
      l1 = -f1 * (double)v1;
      l2 = v2 == INT_MIN ? __builtin_inf() : -f1 * (double)v2;
      // the winner's Q must not have clamped (its bound would be too low)
      if (I1 >= 0 && I1 < P.k)
        clamped = !((double)cq[I1] * (double)qscale <= (double)QCLAMP);
    } else {
      l1 = (double)redL1[lane];
      l2 = (double)redL2[lane];
    }
    bool decided = false, eligible = false;
    double M = 0.0;
    float2 bb = make_float2(-1.0f, -1.0f);   // LIMBS = 1 with bnd: the row's bounds (none)
    if (mt.x != INT_MIN && I1 >= 0 && I1 < P.k && !clamped && shOk && !waveBad &&
        __builtin_isfinite(l1)) {
      bsb = sb;
      bf1 = f1;
      const double xn = xnorm[grow], cn = cnorm[I1];
      const double xx = xn * xn, cc = cn * cn;
      const double n1 = (double)__int_as_float(mt.y);   // bounds |xh3|_1
      const double fx =
          LIMBS == 3 ? err_term(mt.x, n1, mu, d)
          : LIMBS == 2 ? err_term2(mt.x, n1 + (double)d * __builtin_ldexp(1.0078125, mt.x - 15), mu, d)
                       : err_term1(mt.x, n1 + (double)d * __builtin_ldexp(1.0078125, mt.x - 8), mu);
      // LIMBS = 2: the index bits move each V by < 2^IB units and the
      // rounded Q adds < 1 more: |L1 - L1'|, |L2 - L2'| < (2^IB + 1) F1
      // (LIMBS = 1: < 1 unit, the floor of V 2^sb)
      const double enc = LIMBS == 3 ? 0.0
                                    : __builtin_ldexp((double)(IM + 3u), mt.x + P.ec - SH);
      M = (4.0 * (fx + g[I1]) + 2.0 * kEpsF * (xx + cc) + 2.0 * enc +
           0x1p-20 * (__builtin_fabs(l1) + cc + 2.0 * g[I1]) +
           0x1p-24 * (2.0 * (xx + cc) + __builtin_fabs(l1) +
                      __builtin_fmin(__builtin_fabs(l2), 0x1p120)) +
           0x1p-90) *
          (1.0 + 0x1p-30);
      decided = !__builtin_isfinite(l2) || (l2 - l1) > M;
      eligible = __builtin_isfinite(M);
      if constexpr (LIMBS == 1) {
        bxx = xx;
        bfx = fx;
        benc = enc;
        // carried bounds of a certified row: every center but I1 has a
        // computed bound >= l2 (bnd_ub_sq / bnd_lb_sq)
        if (bnd && decided && __builtin_isfinite(l2)) {
          bb.x = bnd_dist_up(bnd_ub_sq(xx, cc, l1, fx, g[I1], enc));
          if (bb.x < 0x1p120f) bb.y = bnd_dist_dn(bnd_lb_sq(xx, l2, fx, enc, 0.0));
        }
      }
    }
    // (rows listed with candidates get their lower bound for the centers
    // outside the set below; every other undecided row none)
    if (LIMBS == 1 && bnd) bnd[grow] = bb;
    if (decided) {
      assign[grow] = I1;
    } else if (LIMBS < 3 && candRows != nullptr && eligible) {
      // candidates: the centers c with f1 (V1 - V_c) <= M, i.e. V_c >= v1 -
      // floor(M / f1) -- the certification test against I1, failed by
      // every candidate and passed by every other center
      const double tv = (double)v1 - __builtin_floor(M / f1);
      if (tv > (double)INT_MIN + 2.0) {
        want = true;
        thrV = (int)tv;
        // LIMBS = 1: in the lanes' Ve units (a lower threshold only adds
        // candidates)
        if constexpr (LIMBS == 1) thrV = (int)((unsigned)max(thrV, -(1 << 23)) << sb);
      } else {
        listS[atomicAdd(listCountS, 1u)] = (int32_t)grow;
      }
    } else {
      listS[atomicAdd(listCountS, 1u)] = (int32_t)grow;
    }
  }
  if constexpr (LIMBS < 3) {
    if (candRows != nullptr) {
      // Candidate sets of the undecided rows from the saved per-lane states:
      // lane (r, h) saw the centers 32 ct + r of row (reg & 3) + 8 (reg >> 2)
      // + 4 h; its best is a candidate when it reaches the row's threshold,
      // and a lane whose SECOND best reaches it too (an index not kept)
      // sends the row to the three-limb pass.  <= kCandMax candidates go to
      // the candidate list (exact fp64 distances, screen_cands).
      int* thrS = (int*)lds + W * 96 + wave * (64 + 32 * (CMAX + 1));
      int* wantS = thrS + 32;
      int* candS = thrS + 64;
      if (lane < 32) {
        thrS[lane] = thrV;
        wantS[lane] = want ? 1 : 0;
      }
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const int row = (reg & 3) + 8 * (reg >> 2) + 4 * h;
        const bool w = wantS[row] != 0;
        const int t = thrS[row];
        const bool ok = w && cV1[reg] >= t;
        const bool ov = w && cV2[reg] >= t;
        const unsigned long long m = __builtin_amdgcn_ballot_w64(ok);
        const unsigned long long mo = __builtin_amdgcn_ballot_w64(ov);
        const unsigned bits = (unsigned)(m >> (32 * h));
        if (ok) {
          const int slot = __builtin_popcount(bits & ((1u << r) - 1u));
          if (slot < CMAX)
            candS[row * (CMAX + 1) + 1 + slot] = (int)((unsigned)cV1[reg] & IM) * 32 + r;
        }
        if (r == 0 && w)
          candS[row * (CMAX + 1)] = (unsigned)(mo >> (32 * h)) ? -1 : __builtin_popcount(bits);
      }
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      // LIMBS = 1 with bnd: the best computed bound among the centers OUTSIDE
      // each candidate row's set -- per lane its best below the threshold
      // (a candidate row has at most one candidate per lane: cV2 is below),
      // the largest V over the row's lanes -- into thrS (read above)
      int* ncS = thrS;
      if constexpr (LIMBS == 1) {
        if (bnd) {
          int nc[16];
#pragma unroll
          for (int reg = 0; reg < 16; ++reg) {
            const int row = (reg & 3) + 8 * (reg >> 2) + 4 * h;
            const int t = thrS[row];
            nc[reg] = cV1[reg] < t ? cV1[reg] : cV2[reg];
          }
          __builtin_amdgcn_wave_barrier();
          rows_max32(nc, lane, ncS);
          __builtin_amdgcn_wave_barrier();
          __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        }
      }
      if (want) {
        const int* cs = candS + lane * (CMAX + 1);
        const int cnt = cs[0];
        if (cnt >= 1 && cnt <= CMAX) {
          const unsigned idx = atomicAdd(candCountS, 1u);
          candRowsS[idx] = (int32_t)grow;
#pragma unroll
          for (int i = 0; i < CMAX; ++i) candsS[(size_t)idx * CMAX + i] = i < cnt ? cs[1 + i] : -1;
          if constexpr (LIMBS == 1) {
            if (bnd) {
              // (-2, lower bound of every center outside the set): the
              // refinement and the three-limb candidate tier finish it
              const int vnc = ncS[lane];
              const double lnc = vnc == INT_MIN ? __builtin_inf() : -bf1 * (double)(vnc >> bsb);
              bnd[grow] = make_float2(-2.0f, vnc == INT_MIN ? __builtin_inff()
                                                            : bnd_dist_dn(bnd_lb_sq(bxx, lnc, bfx, benc, 0.0)));
            }
          }
        } else {
          listS[atomicAdd(listCountS, 1u)] = (int32_t)grow;
        }
      }
    }
  }
  __syncthreads();   // the reduction area is the next group's tile ring
  };
  // LIST: the grid covers n rows; groups past the count leave at once (a
  // grid-stride loop here costs the three-limb S = 8 form ~30 spilled VGPRs)
  if ((int64_t)blockIdx.x * 32 * W < total) group(blockIdx.x);
}

// LIMBS picks the pass's constants (pass_consts); cand (optional): where the
// pass lists rows with their candidate sets; scap: list and cand are shard
// sets of that capacity.
template <int S, int W, int LIMBS, bool LIST>
int launch_screen32(const ScreenCall& sc, const int32_t* rowsIn, const unsigned int* rowsInCount,
                    const AppendTarget& list, const AppendTarget& cand = {},
                    unsigned int scap = 0, float2* bnd = nullptr) {
  KernelTimer timer(LIMBS == 1 ? "k_kmeans_screen1" : LIMBS == 2 ? "k_kmeans_screen2"
                                                    : "k_kmeans_screen3", sc.st);
  const int64_t wg = (sc.n + 32 * W - 1) / (32 * W);   // W waves x 32 rows
  const size_t pc = pass_consts(sc.ktp, LIMBS);
  // launched over the padded center range (sc.ktp / 2 32-center tiles; cq = +inf)
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_screen32<S, W, LIMBS, LIST>), dim3((unsigned)wg),
                     dim3(64 * W), 0, sc.st, (const uint4*)sc.img, sc.meta, sc.xnorm, sc.n, sc.d,
                     (const uint4*)sc.Cb, sc.cq + pc, sc.g + pc, sc.cnorm, sc.prm, sc.ktp / 2,
                     rowsIn, rowsInCount, sc.assign, list.rows, list.count, cand.rows, cand.cands,
                     cand.count, scap, bnd);
  CYC_LAUNCH_CHECK("k_kmeans_screen32_i8");
  return CYC_OK;
}
// LIST from the row list's presence
template <int S, int W, int LIMBS>
int launch_screen32(const ScreenCall& sc, const int32_t* rowsIn, const unsigned int* rowsInCount,
                    const AppendTarget& list, const AppendTarget& cand, unsigned int scap,
                    float2* bnd) {
  return rowsIn ? launch_screen32<S, W, LIMBS, true>(sc, rowsIn, rowsInCount, list, cand, scap, bnd)
                : launch_screen32<S, W, LIMBS, false>(sc, nullptr, nullptr, list, cand, scap, bnd);
}

// ---------------------------------------------------------------------------
// Two-limb refinement (d <= 256) of the one-limb pass.
//
// The one-limb pass (k_screen32<S, W, 1, false>: S1 = a.a' only, one MFMA
// per 32-dim substep, a third of the two-limb pass's) screens every row
// against every center.  It certifies the rows it can; for each other row
// it lists the centers its bounds cannot exclude (<= kCand1: rowsIn /
// candsIn) -- every other center c has a one-limb lower bound above the
// one-limb winner w1's upper bound, i.e. |x - c|^2 > |x - w1|^2 (by the
// certification margin).  Here each wave takes 32 listed rows, forms the
// UNION of their candidate sets (<= 32 kPruneTiles centers: virtual tiles
// of 32, B fragments gathered per lane from the center image) and runs the
// two-limb screen over that union only.  A row certified there (w2 beats
// every union center by the two-limb margin) beats w1 (in the union, or w2
// = w1), hence every center outside the union too, by more than the
// reference's fp64 rounding: the reference's pruned loop returns w2.  Its
// other rows get the two-limb pass's treatment: candidate sets (<=
// kCandMax, within the union) for the fp64 candidate pass, else the
// three-limb pass.  Waves whose union is too large go to fullList (the
// full two-limb pass over every center).
constexpr int kPruneTiles = 3;

template <int S>
__global__ __launch_bounds__(256, 2) void k_screen32r(
    const uint4* __restrict__ Xq, const int2* __restrict__ meta, const double* __restrict__ xnorm,
    int64_t n, int d, const uint4* __restrict__ Cb, const float* __restrict__ cq,
    const double* __restrict__ g, const double* __restrict__ cnorm,
    const CenterParams* __restrict__ prm, int kstride, const int32_t* __restrict__ rowsIn,
    const unsigned int* __restrict__ rowsInCount, const int32_t* __restrict__ candsIn,
    int32_t* __restrict__ assign, int32_t* __restrict__ list, unsigned int* __restrict__ listCount,
    int32_t* __restrict__ candRows, int32_t* __restrict__ cands,
    unsigned int* __restrict__ candCount, int32_t* __restrict__ fullList,
    unsigned int* __restrict__ fullCount, unsigned int* __restrict__ stat, unsigned int scap,
    float2* __restrict__ bnd) {
  constexpr int D = 32 * S, CH = 3 * D / 16;
  constexpr int W = 4;
  // per wave: the candidate list, then the candidate-set scratch (the union
  // bitmap, kstride bits, aliases the latter)
  constexpr int PER_WAVE = 32 * kPruneTiles + 64 + 32 * (kCandMax + 1);
  static_assert(64 + 32 * (kCandMax + 1) >= 4096 / 32, "bitmap fits the scratch");
  __shared__ int ldsw[W * PER_WAVE];
  const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  int* candL = ldsw + wave * PER_WAVE;
  const CenterParams P = *prm;
  const double mu = P.mu * 0x1p-7;
  const int64_t total = (int64_t)*rowsInCount;
  const int64_t pos0 = ((int64_t)blockIdx.x * W + wave) * 32;
  const int rows = (int)max<int64_t>(0, min<int64_t>(32, total - pos0));
  if (rows == 0) return;
  const bool rowOk = r < rows;
  const int64_t myRow = rowOk ? rowsIn[pos0 + r] : 0;
  // scap > 0: appends (and the stat adds) go to this wave's shard
  const unsigned shard = (unsigned)((blockIdx.x * W + wave) % kShards);
  if (scap) {
    list += (size_t)shard * scap;
    listCount += shard * kShardStride;
    fullList += (size_t)shard * scap;
    fullCount += shard * kShardStride;
    if (candRows) {
      candRows += (size_t)shard * scap;
      cands += (size_t)shard * scap * kCandMax;
      candCount += shard * kShardStride;
    }
    if (stat) stat += shard * kShardStride;
  }
  auto to_full = [&]() {
    if (lane < rows) {
      fullList[atomicAdd(fullCount, 1u)] = (int32_t)myRow;
      // the full two-limb pass keeps no bound for the centers it excludes
      if (bnd) bnd[myRow] = make_float2(-1.0f, -1.0f);
    }
  };
  if (!P.ok) {   // uniform over the grid: every row to the fp64 tier
    if (lane < rows) list[atomicAdd(listCount, 1u)] = (int32_t)myRow;
    return;
  }
  // the union of the rows' candidate sets: bitmap, then the compacted list
  unsigned* bm = (unsigned*)(candL + 32 * kPruneTiles);
  const int words = kstride >> 5;                      // <= 128
  for (int q = lane; q < words; q += 64) bm[q] = 0u;
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  bool bad = false;
  if (lane < 32 && rowOk) {
    const int32_t* cs = candsIn + (pos0 + r) * kCand1;
#pragma unroll
    for (int i = 0; i < kCand1; ++i) {
      const int c = cs[i];
      if (c >= P.k) bad = true;
      if (c >= 0 && c < P.k) atomicOr(&bm[c >> 5], 1u << (c & 31));
    }
  }
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  const unsigned wA = lane < words ? bm[lane] : 0u;
  const unsigned wB = lane + 64 < words ? bm[lane + 64] : 0u;
  const int cnt = __builtin_popcount(wA) + __builtin_popcount(wB);
  int pre = cnt;                                       // inclusive prefix over lanes
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    const int t = __shfl_up(pre, m);
    if (lane >= m) pre += t;
  }
  const int ncand = __shfl(pre, 63);
  if (__builtin_amdgcn_ballot_w64(bad) != 0 || ncand > 32 * kPruneTiles || ncand == 0) {
    to_full();
    return;
  }
  {
    int o = pre - cnt;
    for (unsigned b = wA; b; b &= b - 1) candL[o++] = lane * 32 + __builtin_ffs((int)b) - 1;
    for (unsigned b = wB; b; b &= b - 1) candL[o++] = (lane + 64) * 32 + __builtin_ffs((int)b) - 1;
    const int nt = (ncand + 31) >> 5;
    for (int q = ncand + lane; q < nt * 32; q += 64) candL[q] = -1;
  }
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  const int ntiles = (ncand + 31) >> 5;
  // A fragments of the wave's rows (two limbs)
  v4i A[S][2];
  {
    const uint4* src = Xq + myRow * CH + h;
#pragma unroll
    for (int s = 0; s < S; ++s)
#pragma unroll
      for (int L = 0; L < 2; ++L) {
        const v4u t = __builtin_nontemporal_load((const v4u*)(src + L * (D / 16) + 2 * s));
        A[s][L] = rowOk ? __builtin_bit_cast(v4i, t) : v4i{0, 0, 0, 0};
      }
  }
  const int2 mt = rowOk ? meta[myRow] : make_int2(INT_MIN, 0);
  const int exr = mt.x;
  int e0 = exr == INT_MIN ? INT_MAX : exr;
#pragma unroll
  for (int m = 1; m < 32; m <<= 1) e0 = min(e0, __shfl_xor(e0, m));
  const int exmin = __builtin_amdgcn_readfirstlane(e0 == INT_MAX ? 0 : e0);
  int sh[16];
  {
    const int s0 = exr == INT_MIN ? 31 : min(exr - exmin, 31);
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) sh[reg] = __shfl(s0, (reg & 3) + 8 * (reg >> 2) + 4 * h);
  }
  const float qscale = __builtin_ldexpf(1.0f, max(-160, min(160, 20 - P.ec - exmin)));
  bool qbad = false;
  double xxj = 0.0;
  if (lane < 32 && rowOk) {
    const double xn = xnorm[myRow];
    xxj = xn * xn;
  }
  // B fragments of center c (c < 0: a padding column, zero), from the
  // center-major copy behind the fragment image (k_centers_pack32): a lane's
  // 16 pieces of its center lie in 512 contiguous bytes (from the fragments
  // every piece was a separate cache line)
  const uint4* Cr = Cb + (size_t)(kstride >> 5) * S * 3 * 64;
  auto loadB = [&](int c, v4i (&B)[S][2]) {
    const bool on = c >= 0;
    const uint4* src = Cr + (size_t)(on ? c : 0) * (6 * S) + h;
#pragma unroll
    for (int s = 0; s < S; ++s)
#pragma unroll
      for (int L = 0; L < 2; ++L) {
        const v4u t = *(const v4u*)(src + L * 2 * S + 2 * s);
        B[s][L] = on ? __builtin_bit_cast(v4i, t) : v4i{0, 0, 0, 0};
      }
  };
  // one virtual tile: column r holds center col (lane's), acc[1] from -Q
  auto tileMfma = [&](int col, const v4i (&B)[S][2], v16i (&X)[2]) {
    const float cqv = col >= 0 ? cq[col] : 0x1.fffffep127f;
    const float pf = cqv * qscale;
    qbad |= pf < -0x1p30f;
    const int nb = -(int)__builtin_floorf(__builtin_fminf(pf, 0x1p30f));
    X[0] = v16i{};
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) X[1][reg] = nb >> sh[reg];
#pragma unroll
    for (int s = 0; s < S; ++s) {
      X[0] = __builtin_amdgcn_mfma_i32_32x32x32_i8(A[s][0], B[s][0], X[0], 0, 0, 0);
      X[1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(A[s][0], B[s][1], X[1], 0, 0, 0);
      X[1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(A[s][1], B[s][0], X[1], 0, 0, 0);
    }
  };
  // the two-limb certification margin of row (mt, xx) against center c
  // (lower bounds l1, runner-up l2; IM: the index bits in V)
  auto margin = [&](int c, double xx, double l1, double l2, unsigned IM) {
    const double cn = cnorm[c];
    const double cc = cn * cn;
    const double n1 = (double)__int_as_float(mt.y);
    const double fx = err_term2(mt.x, n1 + (double)d * __builtin_ldexp(1.0078125, mt.x - 15), mu, d);
    const double enc = __builtin_ldexp((double)(IM + 3u), mt.x + P.ec - 20);
    return (4.0 * (fx + g[c]) + 2.0 * kEpsF * (xx + cc) + 2.0 * enc +
            0x1p-20 * (__builtin_fabs(l1) + cc + 2.0 * g[c]) +
            0x1p-24 * (2.0 * (xx + cc) + __builtin_fabs(l1) +
                       __builtin_fmin(__builtin_fabs(l2), 0x1p120)) +
            0x1p-90) *
           (1.0 + 0x1p-30);
  };
  __builtin_amdgcn_s_setreg(0x801, 2);     // f32 rounding toward -inf (lower bounds)
  const int total_ = ncand;
  // 4. the screen over the candidate tiles (top two V per row slot, the
  // virtual tile index in the low IB bits)
  const int IB = 32 - __builtin_clz((unsigned)max(ntiles - 1, 1));
  const unsigned IM = (1u << IB) - 1u;
  int sV1[16], sV2[16], sI1[16];
#pragma unroll
  for (int q = 0; q < 16; ++q) sV1[q] = sV2[q] = INT_MIN;
  for (int t = 0; t < ntiles; ++t) {
    const int col = candL[t * 32 + r];
    v4i B[S][2];
    loadB(col, B);
    v16i X[2];
    tileMfma(col, B, X);
    unsigned ctv;
    asm("v_mov_b32 %0, %1" : "=v"(ctv) : "s"(t));
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int V = X[0][reg] * 128 + X[1][reg];
      const int Ve = (int)(((unsigned)V & ~IM) | ctv);
      sV2[reg] = max(min(sV1[reg], sV2[reg]), min(max(sV1[reg], sV2[reg]), Ve));
      sV1[reg] = max(sV1[reg], Ve);
    }
  }
  __builtin_amdgcn_s_setreg(0x801, 0);
  const bool waveBad = __builtin_amdgcn_ballot_w64(qbad) != 0;
  // each lane's own best / second best (its column) before the reduction:
  // the candidate sets; centers through the candidate list
  int cV1[16], cV2[16];
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    sI1[q] = candL[(int)((unsigned)sV1[q] & IM) * 32 + r];
    cV1[q] = sV1[q];
    cV2[q] = sV2[q];
  }
  auto mergeV = [](int& V1, int& V2, int& I1, int oV1, int oV2, int oI1) {
    V2 = max(min(V1, oV1), max(V2, oV2));
    I1 = oV1 > V1 ? oI1 : I1;
    V1 = max(V1, oV1);
  };
#pragma unroll
  for (int lev = 0; lev < 4; ++lev) {
    const int half = 8 >> lev, m = 16 >> lev;
    const bool hi = (lane & m) != 0;
#pragma unroll
    for (int i = 0; i < half; ++i) {
      const int o1 = __shfl_xor(hi ? sV1[i] : sV1[i + half], m);
      const int o2 = __shfl_xor(hi ? sV2[i] : sV2[i + half], m);
      const int oI1 = __shfl_xor(hi ? sI1[i] : sI1[i + half], m);
      int k1 = hi ? sV1[i + half] : sV1[i];
      int k2 = hi ? sV2[i + half] : sV2[i];
      int I1 = hi ? sI1[i + half] : sI1[i];
      mergeV(k1, k2, I1, o1, o2, oI1);
      sV1[i] = k1;
      sV2[i] = k2;
      sI1[i] = I1;
    }
  }
  mergeV(sV1[0], sV2[0], sI1[0], __shfl_xor(sV1[0], 1), __shfl_xor(sV2[0], 1),
         __shfl_xor(sI1[0], 1));
  // lane holds row register q = lane bits 1..4: per-row results through LDS
  int* red = candL + 32 * kPruneTiles;                // 3 x 32 ints (reused below)
  int* redV1 = red;
  int* redV2 = red + 32;
  int* thrS = red;                                    // after the reads below
  int* wantS = red + 32;
  int* candS = red + 64;
  int* redI1 = candS;                                 // 32 ints, read before candS is written
  if ((lane & 1) == 0) {
    const int q = (lane >> 1) & 15;
    const int row = (q & 3) + 8 * (q >> 2) + 4 * h;
    redV1[row] = sV1[0];
    redV2[row] = sV2[0];
    redI1[row] = sI1[0];
  }
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  bool want = false;
  int thrV = 0;
  // with bnd: the row's lower bound for the centers outside its one-limb
  // set (the one-limb pass left it in bnd[row].y), and its terms
  float lncPrev = -1.0f;
  double bfx = 0.0, benc = 0.0, bf1 = 0.0;
  if (lane < rows) {
    const int I1 = redI1[lane];
    const int v1 = redV1[lane];
    const int v2 = redV2[lane];
    const double f1 = __builtin_ldexp(1.0, exr + P.ec - 20);
    const double l1 = -f1 * (double)v1;
    const double l2 = v2 == INT_MIN ? __builtin_inf() : -f1 * (double)v2;
    bool decided = false, eligible = false;
    double M = 0.0;
    if (exr != INT_MIN && I1 >= 0 && I1 < P.k && !waveBad && __builtin_isfinite(l1) &&
        (double)cq[I1] * (double)qscale <= 0x1p30) {
      M = margin(I1, xxj, l1, l2, IM);
      decided = !__builtin_isfinite(l2) || (l2 - l1) > M;
      eligible = __builtin_isfinite(M);
      if (bnd) {
        const float2 pb = bnd[myRow];
        lncPrev = pb.x == -2.0f ? pb.y : -1.0f;
        const double n1 = (double)__int_as_float(mt.y);
        bfx = err_term2(mt.x, n1 + (double)d * __builtin_ldexp(1.0078125, mt.x - 15), mu, d);
        benc = __builtin_ldexp((double)(IM + 3u), mt.x + P.ec - 20);
        bf1 = f1;
        if (decided && __builtin_isfinite(l2) && lncPrev >= 0.0f) {
          // certified over the union: the union's other centers have
          // computed bounds >= l2, the rest the one-limb pass's bound
          const double cn = cnorm[I1];
          const float ub = bnd_dist_up(bnd_ub_sq(xxj, cn * cn, l1, bfx, g[I1], benc));
          const float lb = bnd_dist_dn(bnd_lb_sq(xxj, l2, bfx, benc, 0.0));
          bnd[myRow] = ub < 0x1p120f ? make_float2(ub, __builtin_fminf(lb, lncPrev))
                                     : make_float2(-1.0f, -1.0f);
        }
      }
    }
    if (decided) {
      assign[myRow] = I1;
    } else if (candRows != nullptr && eligible) {
      const double tv = (double)v1 - __builtin_floor(M / f1);
      if (tv > (double)INT_MIN + 2.0) {
        want = true;
        thrV = (int)tv;
      } else {
        list[atomicAdd(listCount, 1u)] = (int32_t)myRow;
      }
    } else {
      list[atomicAdd(listCount, 1u)] = (int32_t)myRow;
    }
  }
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  if (candRows != nullptr) {
    // candidate sets of the undecided rows (as the full pass; the centers
    // pruned in step 3 are excluded by margin)
    if (lane < 32) {
      thrS[lane] = thrV;
      wantS[lane] = want ? 1 : 0;
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int row = (reg & 3) + 8 * (reg >> 2) + 4 * h;
      const bool w = wantS[row] != 0;
      const int t = thrS[row];
      const bool ok = w && cV1[reg] >= t;
      const bool ov = w && cV2[reg] >= t;
      const unsigned long long m = __builtin_amdgcn_ballot_w64(ok);
      const unsigned long long mo = __builtin_amdgcn_ballot_w64(ov);
      const unsigned bts = (unsigned)(m >> (32 * h));
      if (ok) {
        const int slot = __builtin_popcount(bts & ((1u << r) - 1u));
        if (slot < kCandMax)
          candS[row * (kCandMax + 1) + 1 + slot] = candL[(int)((unsigned)cV1[reg] & IM) * 32 + r];
      }
      if (r == 0 && w)
        candS[row * (kCandMax + 1)] = (unsigned)(mo >> (32 * h)) ? -1 : __builtin_popcount(bts);
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    // with bnd: the best computed bound among the union's centers outside
    // each candidate row's set (the one-limb pass's ncS, over the union)
    int* ncS = thrS;
    if (bnd) {
      int nc[16];
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const int row = (reg & 3) + 8 * (reg >> 2) + 4 * h;
        const int t = thrS[row];
        nc[reg] = cV1[reg] < t ? cV1[reg] : cV2[reg];
      }
      __builtin_amdgcn_wave_barrier();
      rows_max32(nc, lane, ncS);
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    }
    if (want) {
      const int* cs = candS + lane * (kCandMax + 1);
      const int c0 = cs[0];
      if (c0 >= 1 && c0 <= kCandMax) {
        const unsigned idx = atomicAdd(candCount, 1u);
        candRows[idx] = (int32_t)myRow;
#pragma unroll
        for (int i = 0; i < kCandMax; ++i) cands[(size_t)idx * kCandMax + i] = i < c0 ? cs[1 + i] : -1;
        if (bnd) {
          // (-2, lower bound outside the set): the union's other centers and
          // (lncPrev) the centers outside the union; the three-limb
          // candidate tier finishes it
          const int vnc = ncS[lane];
          const float l2nc = vnc == INT_MIN ? __builtin_inff()
                                            : bnd_dist_dn(bnd_lb_sq(xxj, -bf1 * (double)vnc, bfx, benc, 0.0));
          bnd[myRow] = make_float2(-2.0f, lncPrev >= 0.0f ? __builtin_fminf(lncPrev, l2nc) : -1.0f);
        }
      } else {
        list[atomicAdd(listCount, 1u)] = (int32_t)myRow;
      }
    }
  }
  if (stat && lane == 0) atomicAdd(stat, (unsigned)total_);
}

template <int S>
int launch_refine(const ScreenCall& sc, const RefineArgs& ra, const AppendTarget& list,
                  const AppendTarget& cand, const AppendTarget& full, unsigned int* stat,
                  unsigned int scap, float2* bnd) {
  KernelTimer timer("k_kmeans_refine2", sc.st);
  const size_t pc = pass_consts(sc.ktp, 2);
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_screen32r<S>), dim3((unsigned)((sc.n + 127) / 128)),
                     dim3(256), 0, sc.st, (const uint4*)sc.img, sc.meta, sc.xnorm, sc.n, sc.d,
                     (const uint4*)sc.Cb, sc.cq + pc, sc.g + pc, sc.cnorm, sc.prm, ra.kstride,
                     (const int32_t*)ra.cand1Rows, (const unsigned int*)ra.cand1Count,
                     (const int32_t*)ra.cand1, sc.assign, list.rows, list.count, cand.rows,
                     cand.cands, cand.count, full.rows, full.count, stat, scap, bnd);
  CYC_LAUNCH_CHECK("k_screen32r");
  return CYC_OK;
}

template <int KS>
int launch_screen(const ScreenCall& sc, int32_t* list, unsigned int* listCount) {
  constexpr int STR = 12 * KS + 2;
  const size_t lds = (size_t)kBM * STR * 16 + (size_t)kBM * 4;   // slot minima alias the image
  static bool attr = false;
  if (!attr) {
    CYC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_screen<KS>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    attr = true;
  }
  KernelTimer timer("k_kmeans_screen3", sc.st);
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_screen<KS>), dim3((unsigned)((sc.n + kBM - 1) / kBM)),
                     dim3(256), lds, sc.st, (const uint4*)sc.img, sc.meta, sc.xnorm, sc.n, sc.d,
                     (const uint4*)sc.Cb, sc.cq, sc.g, sc.cnorm, sc.prm, sc.ktp, sc.assign, list,
                     listCount);
  CYC_LAUNCH_CHECK("k_kmeans_screen_i8");
  return CYC_OK;
}

// One destination of a launch's appends: the list itself or, with a stage,
// the stage's shard set `set`, which `job` then moves behind the list (the
// pairing of shard set and list is said once, here).
struct Append {
  AppendTarget at;   // what the kernel gets
  CompactJob job;    // stage only
};
Append append_to(const AppendStage* sg, int set, int32_t* rows, unsigned int* count,
                 int32_t* cands = nullptr, int width = 0) {
  if (!sg) return {{rows, count, cands}, {}};
  int32_t* const srows = set == kSetRowsA   ? sg->rowsA
                         : set == kSetRowsB ? sg->rowsB
                         : set == kSetCand  ? sg->candRows
                                            : nullptr;   // kSetStat: a counter alone
  int32_t* const scands = cands ? sg->cands : nullptr;
  return {{srows, sg->set(set), scands},
          {sg->set(set), srows, rows, srows ? 1 : 0, scands, cands, width, count}};
}
// With a stage: a launch's shard sets moved behind their (distinct) lists.
int compact_appends(const AppendStage* sg, std::initializer_list<const Append*> as,
                    hipStream_t st) {
  if (!sg) return CYC_OK;
  CompactJob jb[kMaxCompactJobs];
  int nj = 0;
  for (const Append* a : as) jb[nj++] = a->job;
  return compact_jobs(jb, nj, sg->cap, st);
}

// A side stream of this host thread (one per device: a host thread may drive
// plans on several GPUs; the caller's DeviceGuard made `st`'s device
// current) that waits for st's work so far; *join brings it back.
int fork_side(hipStream_t st, hipStream_t* side, hipEvent_t* join) {
  constexpr int kMaxDev = 64;
  thread_local hipStream_t sides[kMaxDev] = {};
  thread_local hipEvent_t forks[kMaxDev] = {}, joins[kMaxDev] = {};
  int dev = 0;
  CYC_HIP(hipGetDevice(&dev));
  if (dev < 0 || dev >= kMaxDev) {
    cyc::set_error("device index out of range");
    return CYC_ERR_INVALID_ARG;
  }
  if (!sides[dev]) {
    CYC_HIP(hipStreamCreateWithFlags(&sides[dev], hipStreamNonBlocking));
    CYC_HIP(hipEventCreateWithFlags(&forks[dev], hipEventDisableTiming));
    CYC_HIP(hipEventCreateWithFlags(&joins[dev], hipEventDisableTiming));
  }
  CYC_HIP(hipEventRecord(forks[dev], st));
  CYC_HIP(hipStreamWaitEvent(sides[dev], forks[dev], 0));
  *side = sides[dev];
  *join = joins[dev];
  return CYC_OK;
}

// The d <= 256 screen.  Two-limb pass over every row; its undecided rows with
// a small candidate set get exact fp64 distances to those candidates
// (k_screen_cands, behind the three-limb tier k_screen_cands3), the others
// the three-limb pass.  With ra (and ca) the one-limb pass over every center
// and the two-limb refinement over the union of the listed rows' candidates
// come first, and the two-limb pass takes only the rows neither can handle
// (fullList).  With carried bounds (bd) the rows bounds_filter sent to a
// re-check go before that, and the one-limb pass screens only the rows that
// need a full screen.  With `stg` (and ca) every 32x32 kernel appends
// through its shards, compacted after each launch.
template <int S, int W>
int screen32(const ScreenCall& sc, int32_t* list, unsigned int* listCount, int32_t* list2,
             unsigned int* list2Count, const CandArgs* ca, const RefineArgs* ra,
             const AppendStage* stg, const Bounds* bd, bool countersZeroed) {
  const AppendStage* sg = ca ? stg : nullptr;
  const unsigned scap = sg ? sg->cap : 0u;
  const hipStream_t st = sc.st;
  int rc;
  // every counter of the pass zeroed by one launch (six fills before)
  if (!countersZeroed &&
      (rc = launch_zero_counters(screen_zero_args(list2Count, ca, ra, stg), st)))
    return rc;
  // the two-limb kernels' outputs: list2 (rows) and the candidate lists
  const Append rows2 = append_to(sg, kSetRowsA, list2, list2Count);
  const Append cand2 =
      ca ? append_to(sg, kSetCand, ca->candRows, ca->candCount, ca->cands, kCandMax) : Append{};
  if (ra && ca) {
    float2* const bnd = bd ? bd->ub_lb : nullptr;
    if (bd && bd->rcRows) {
      if ((rc = launch_recheck(sc, *bd))) return rc;
      if (bd->dump) dump_dev("state_rc", bd->state, (size_t)bd->n, st);
      if (!(bd->collected && recheck_two_phase()) && (rc = bounds_collect(*bd, st))) return rc;
    }
    // the one-limb pass: rows beyond it to fullList, candidate rows to cand1
    const Append full1 = append_to(sg, kSetRowsA, ra->fullList, ra->fullCount);
    const Append cand1 =
        append_to(sg, kSetCand, ra->cand1Rows, ra->cand1Count, ra->cand1, kCand1);
    if ((rc = launch_screen32<S, W, 1>(sc, bd ? bd->rowsIn : nullptr,
                                       bd ? bd->rowsInCount : nullptr, full1.at, cand1.at, scap,
                                       bnd)) ||
        (rc = compact_appends(sg, {&full1, &cand1}, st)))
      return rc;
    // the refinement: the two-limb outputs, the waves it leaves to the full
    // pass (behind the one-limb pass's in fullList) and their statistic
    const Append fullR = append_to(sg, kSetRowsB, ra->fullList, ra->fullCount);
    const Append stat = append_to(sg, kSetStat, nullptr, ra->fullCount + 1);
    if ((rc = launch_refine<S>(sc, *ra, rows2.at, cand2.at, fullR.at, stat.at.count, scap,
                               bnd)) ||
        (rc = compact_appends(sg, {&rows2, &cand2, &fullR, &stat}, st)))
      return rc;
    rc = launch_screen32<S, W, 2, true>(sc, ra->fullList, ra->fullCount, rows2.at, cand2.at,
                                        scap);
  } else {
    rc = launch_screen32<S, W, 2, false>(sc, nullptr, nullptr, rows2.at, cand2.at, scap);
  }
  if (rc || (rc = compact_appends(sg, {&rows2, &cand2}, st))) return rc;
  if (!ca) return launch_screen32<S, W, 3, true>(sc, list2, list2Count, {list, listCount});
  // the three-limb tier of the candidate rows (CandArgs::candRows2 set):
  // the rows it cannot certify go on, with their candidates, to the fp64
  // candidate pass
  CandArgs caF = *ca;
  if (ca->candRows2) {
    const Append out =
        append_to(sg, kSetCand, ca->candRows2, ca->candCount2, ca->cands2, kCandMax);
    if ((rc = launch_cands3(sc, *ca, out.at, scap, bd)) ||
        (rc = compact_appends(sg, {&out}, st)))
      return rc;
    caF.candRows = ca->candRows2;
    caF.cands = ca->cands2;
    caF.candCount = ca->candCount2;
  }
  // the three-limb pass (rows with more than kCandMax candidates) and the
  // candidate pass touch disjoint rows and only append to `list` (through
  // two separate shard sets with a stage), so either order, or side by
  // side, gives the same result.
  // The three-limb pass (0.19 ms of work: ~115K rows on config 2) runs on
  // the main stream before the candidate pass: beside it on a side stream
  // (CYC_KMEANS_SIDE=1, the round-4 form) the two shared the CUs and the
  // iteration measured 9.77 vs 9.71 ms (same box, interleaved).
  const Append list3 = append_to(sg, kSetRowsA, list, listCount);
  const Append listC = append_to(sg, kSetRowsB, list, listCount);
  if (!screen_side_stream()) {
    if ((rc = launch_screen32<S, W, 3, true>(sc, list2, list2Count, list3.at, {}, scap)) ||
        (rc = launch_cands(caF, sc.n, sc.d, sc.assign, listC.at, st, scap)))
      return rc;
  } else {
    ScreenCall scSide = sc;
    hipEvent_t join;
    if ((rc = fork_side(st, &scSide.st, &join)) ||
        (rc = launch_screen32<S, W, 3, true>(scSide, list2, list2Count, list3.at, {}, scap)))
      return rc;
    rc = launch_cands(caF, sc.n, sc.d, sc.assign, listC.at, st, scap);
    CYC_HIP(hipEventRecord(join, scSide.st));
    CYC_HIP(hipStreamWaitEvent(st, join, 0));
    if (rc) return rc;
  }
  // (both behind *listCount: a launch each)
  if ((rc = compact_appends(sg, {&list3}, st))) return rc;
  return compact_appends(sg, {&listC}, st);
}

}  // namespace

bool screen_side_stream() {
  static const bool on = [] {
    const char* e = std::getenv("CYC_KMEANS_SIDE");
    return e && e[0] == '1';
  }();
  return on;
}

int screen(const ScreenCall& sc, int32_t* list, unsigned int* listCount, int32_t* list2,
           unsigned int* list2Count, const CandArgs* ca, const RefineArgs* ra,
           const AppendStage* stg, const Bounds* bd, bool countersZeroed) {
  if (sc.n <= 0) return CYC_OK;
  if (stg && stg->cap < shard_cap(sc.n)) {
    set_error("append stage smaller than shard_cap(n)");
    return CYC_ERR_INVALID_ARG;
  }
  if (bd && !(ra && ca && uses32(sc.d))) {
    set_error("carried bounds need the one-limb pass (d <= 256, refinement, candidate pass)");
    return CYC_ERR_INVALID_ARG;
  }
  if (uses32(sc.d))   // S = 2 ksteps(d) 32-dim substeps
    return ksteps(sc.d) == 2
               ? screen32<4, 4>(sc, list, listCount, list2, list2Count, ca, ra, stg, bd,
                                countersZeroed)
               : screen32<8, 4>(sc, list, listCount, list2, list2Count, ca, ra, stg, bd,
                                countersZeroed);
  switch (ksteps(sc.d)) {
#define CYC_S8(K) \
  case K: return launch_screen<K>(sc, list, listCount);
    CYC_S8(2) CYC_S8(4) CYC_S8(6) CYC_S8(8)
#undef CYC_S8
    default:
      set_error("the i8 screen supports d <= 512");
      return CYC_ERR_UNSUPPORTED;
  }
}

}  // namespace km8
}  // namespace cyc
