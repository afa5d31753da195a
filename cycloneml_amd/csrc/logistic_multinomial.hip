// logistic_multinomial.hip -- MultinomialLogisticBlockAggregator on gfx950
// (MI355X): ml/optim/aggregator/MultinomialLogisticBlockAggregator.scala:101-189
// over all blocks of a shard held as one matrix (dense row-major n x F, or
// CSR with its row-blocked CSC copy).  Plan and shared folds: logistic_plan.hpp.
//
// Kernels
//   k_mlr_offset         marginOffset per class (fitWithMean)
//   k_mlr_margins<CT>    margins = X W^T on fp64 MFMA (16x16x4), X from HBM
//                        into registers in the MFMA A layout, W chunks (16
//                        features x C classes) DMA'd into LDS; softmax / loss /
//                        multiplier epilogue in registers (cross-lane max and
//                        sum); writes the multiplier matrix (n x CP) and
//                        per-wave partials.
//   k_mlr_grad<CT>       grad^T (CP x F) = mult^T X on fp64 MFMA, split-K
//                        over rows, 32-row chunks, partial tiles to slabs.
//   k_mlr_fold           the slabs folded in fixed order into the gradient
//   k_fold_columns       per-wave class sums folded per class
//   k_mlr_csr_margins<CQ>, k_mlr_csc_grad<CQ>, k_mlr_icpt   the CSR rows' path
//   k_softmax_exp        exp_neg over an array (cyc_softmax_exp_dev)
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <mutex>
#include <type_traits>

#include "logistic_plan.hpp"

namespace {

using cyc::check_common;
using cyc::wave_sum_bcast;

// marginOffset (Multinomial :86-92): intercept + gemv(-1.0, linear, scaledMean)
// with netlib dgemv "N" column order.
__global__ void k_mlr_offset(const double* __restrict__ coef, const double* __restrict__ sm,
                             int F, int C, double* __restrict__ off) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  double o = coef[(int64_t)C * F + c];
  for (int f = 0; f < F; ++f) {
    if (sm[f] != 0.0) {
      const double t = -1.0 * sm[f];
      o = o + t * coef[(int64_t)f * C + c];
    }
  }
  off[c] = o;
}

typedef int v4i32 __attribute__((ext_vector_type(4)));
typedef int v2i32 __attribute__((ext_vector_type(2)));

// tools/probe/mlr_probe.hip builds k_mlr_margins with parts removed to time
// them (results then meaningless): bits 1 = X loaded for chunk 0 only, 2 = no
// softmax epilogue, 4 = no W DMA, 8 = no multiplier stores, 16 = no exp.
// 0 in the library.
#ifndef CYC_MLR_PROBE
#define CYC_MLR_PROBE 0
#endif
// k_mlr_margins: waves per workgroup; dephased workgroup pairs (see the kernel)
#ifndef CYC_MLR_NW
#define CYC_MLR_NW 8
#endif
#ifndef CYC_MLR_DEPHASE
#define CYC_MLR_DEPHASE false
#endif

// 2^(j/32), j = 0..31, correctly rounded (exp_neg's table)
__constant__ double kExp2Tab[32] = {
    1.0, 1.0218971486541166, 1.0442737824274138, 1.0671404006768237,
    1.0905077326652577, 1.1143867425958924, 1.1387886347566916, 1.1637248587775775,
    1.189207115002721, 1.215247359980469, 1.241857812073484, 1.2690509571917332,
    1.2968395546510096, 1.3252366431597413, 1.3542555469368927, 1.383909881963832,
    1.4142135623730951, 1.4451808069770467, 1.4768261459394993, 1.5091644275934228,
    1.5422108254079407, 1.5759808451078865, 1.6104903319492543, 1.645755478153965,
    1.681792830507429, 1.718619298122478, 1.7562521603732995, 1.7947090750031072,
    1.8340080864093424, 1.8741676341103, 1.9152065613971474, 1.9571441241754002};

// e^x for x <= 0 (the softmax terms m - max): x = (32 e + j) ln2/32 + r with
// |r| <= ln2/64 (Cody-Waite, a 38-bit high part), e^x = 2^e 2^(j/32) e^r,
// e^r by its degree-6 Taylor polynomial (truncation < 2^-57 relative),
// 2^(j/32) from the LDS table T: within a few ulp, against Math.exp's 1 ulp
// in the reference -- far inside the aggregator's 1e-10 bar -- at 15 f64
// VALU where the libm exp takes ~23.  Below -708.4 the result is subnormal:
// the final ldexp rounds it onto the subnormal grid (a second rounding, and
// past kd = 2^15 the reduction's high product is no longer exact: a relative
// error of ~1e-13 there), so a label whose probability is subnormal keeps
// the reference's finite -log(p).  Below -746 (where e^x rounds to 0 in any
// libm) it returns 0, so -inf gives 0; NaN stays NaN.  tests/
// test_logistic_gpu.py sweeps it against the host libm.
__device__ __forceinline__ double exp_neg(double x, const double* __restrict__ T) {
  // a select, not a branch (a branch here splits the softmax epilogue's wave)
  const bool under = x < -746.0;
  x = under ? -746.0 : x;
  const double kd = __builtin_rint(x * 46.16624130844683);   // 32 / ln2
  double r = __builtin_fma(kd, -0.021660849392446835, x);
  r = __builtin_fma(kd, -5.145609244655338e-14, r);
  const int k = (int)kd;
  double q = 1.0 / 720.0;
  q = __builtin_fma(q, r, 1.0 / 120.0);
  q = __builtin_fma(q, r, 1.0 / 24.0);
  q = __builtin_fma(q, r, 1.0 / 6.0);
  q = __builtin_fma(q, r, 0.5);
  q = __builtin_fma(q, r, 1.0);
  q = __builtin_fma(q, r, 1.0);
  double e = __builtin_ldexp(T[k & 31] * q, k >> 5);
  asm volatile("" : "+v"(e));   // computed on every lane (no branch around it)
  return under ? 0.0 : e;
}

// exp_neg over an array (cyc_softmax_exp_dev: its accuracy test)
__global__ void k_softmax_exp(const double* __restrict__ x, int64_t n, double* __restrict__ out) {
  __shared__ double T[32];
  if (threadIdx.x < 32) T[threadIdx.x] = kExp2Tab[threadIdx.x];
  __syncthreads();
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    out[i] = exp_neg(x[i], T);
}

// a row-16 DPP move of a double (both halves; all lanes active)
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xF, 0xF, false);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xF, 0xF, false);
  return __hiloint2double(hi, lo);
}

constexpr int MR = 256;    // rows per margin tile, at most (8 waves x 32 rows)
constexpr int MK = 16;     // features per LDS chunk

// margins = X W^T (+ offset) for 256-row tiles, 16-feature chunks, on
// v_mfma_f64_16x16x4f64: 2 row tiles x CT class tiles of 16x16 per wave;
// softmax / loss / multiplier epilogue in registers.  Persistent over tiles,
// one 8-wave workgroup per CU.
// X goes from HBM straight into registers in the MFMA A layout -- lane (row
// r = l & 15, group g = l >> 4) holds features f0 + 4g .. 4g + 3 of its row
// for k-steps 0..3 (the contraction order within a chunk is permuted: 128
// contiguous bytes per row per chunk, two dwordx4 loads per lane per row
// tile) -- loaded one chunk ahead into a second register set: no LDS, no
// barrier for X.  W chunks (16 features x C classes, contiguous in coef,
// 12.8 KB at C = 100) are DMA'd into two LDS buffers (buffer_load ... lds,
// 1 KiB pieces spread over the waves, one chunk ahead; no registers), one
// barrier per chunk.  Padding classes read the next coefficients (finite;
// their margins are never used) or zero past the end of coef.
// (The last class tile on v_mfma_f64_4x4x4f64, as k_mlr_grad does, measured
// 4-5 % slower here at C = 100, with or without sched_barrier fences.)
// NW waves per workgroup (32 NW rows per tile; NW = 4: two workgroups per
// CU); DEPHASE: the workgroups whose index bit 0 differs from bit 8 start
// half a tile late, so the two workgroups of a CU (consecutive indices, or
// i and i + 256) run their softmax epilogues while the other one's MFMAs
// keep the matrix pipe busy.
template <int CT, int NW = 8, bool DEPHASE = false>
__global__ __launch_bounds__(64 * NW, 2) void k_mlr_margins(
    const double* __restrict__ X, const double* __restrict__ labels,
    const double* __restrict__ weights, int64_t n, int F, int C, const double* __restrict__ coef,
    const double* __restrict__ offset, double* __restrict__ mult, double* __restrict__ slabS,
    double* __restrict__ slabMS) {
  constexpr int MR = 32 * NW, MT = 64 * NW;
  constexpr int CP = CT * 16;
  static_assert(MK == 16, "the A layout covers 16 features per chunk");
  constexpr int WBUF = MK * CP + 128;   // doubles per W buffer (whole 1 KiB pieces)
  // the two W buffers, then exp_neg's table and the per-class offsets (never
  // DMA targets)
  __shared__ __attribute__((aligned(16))) double Ws[2][WBUF + 32 + CP];
  double* const expT = Ws[1] + WBUF;
  double* const offS = expT + 32;
  __shared__ double plS[MR];   // each wave's 32 label probabilities of a tile
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4;
  const int64_t tiles = (n + MR - 1) / MR;
  const int nch = (F + MK - 1) / MK;
  if constexpr (DEPHASE) {
    // half a tile at ~2 GHz with two waves per SIMD sharing the pipe:
    // nch chunks x 8 CT MFMAs x 64 cycles, on the 100 MHz constant clock
    if (((blockIdx.x ^ (blockIdx.x >> 8)) & 1) != 0) {
      const int64_t ticks = (int64_t)nch * 8 * CT * 64 / 20;
      const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
      while ((int64_t)(__builtin_amdgcn_s_memrealtime() - t0) < ticks)
        __builtin_amdgcn_s_sleep(32);
    }
  }
  // read after a barrier: the epilogue reads them by ds_read, so none of
  // its waits is a vmcnt that would also drain the multiplier stores
  if (threadIdx.x < 32) expT[threadIdx.x] = kExp2Tab[threadIdx.x];
  if (threadIdx.x < CP) offS[threadIdx.x] = (offset && (int)threadIdx.x < C) ? offset[threadIdx.x] : 0.0;
  double loss = 0.0, wsum = 0.0;
  double ms[CT];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) ms[ct] = 0.0;
  // Loads go through buffer descriptors: 32-bit offsets; rows past n read
  // as zero (out-of-range offsets).  Host guarantees MR * F * 8 < 2^31 and
  // (C * F + C) * 8 < 2^31.
  constexpr int OOB = 0x7ff00000;
  const auto wR = __builtin_amdgcn_make_buffer_rsrc((void*)coef, (short)0, (C * F + C) * 8,
                                                    0x00020000);
  // pieces covering every index the B reads touch: (MK - 1) C + CP doubles
  const int wpieces = (((MK - 1) * C + CP) * 8 + 1023) / 1024;
  auto loadW = [&](int ch) {      // chunk ch's 16 x C run of coef into buffer ch & 1
    if constexpr ((CYC_MLR_PROBE & 4) != 0) return;
    double* dst = Ws[ch & 1];
    const int base = ch * MK * C * 8;
    for (int q = wave; q < wpieces; q += MT / 64)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(
          wR, (__attribute__((address_space(3))) void*)(dst + q * 128), 16, base + q * 1024 +
          lane * 16, 0, 0, 0);
  };
  auto loadX = [&](int64_t r0, int ch, double (&x)[2][4]) {
    if constexpr ((CYC_MLR_PROBE & 1) != 0) {
      if (ch > 0) return;
    }
    const int f0 = ch * MK + 4 * g;
    const int64_t nr = min<int64_t>(MR, n - r0);
    const auto xR = __builtin_amdgcn_make_buffer_rsrc((void*)(X + r0 * F), (short)0,
                                                      (int)(nr * F * 8), 0x00020000);
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int off = ((wave * 32 + t * 16 + (lane & 15)) * F + f0) * 8;
      if (f0 + 3 < F) {
        // nontemporal (aux 2): X streams through once per evaluation pass
        const v4i32 lo = __builtin_amdgcn_raw_buffer_load_b128(xR, off, 0, 2);
        const v4i32 hi = __builtin_amdgcn_raw_buffer_load_b128(xR, off + 16, 0, 2);
        x[t][0] = __builtin_bit_cast(double, (v2i32){lo[0], lo[1]});
        x[t][1] = __builtin_bit_cast(double, (v2i32){lo[2], lo[3]});
        x[t][2] = __builtin_bit_cast(double, (v2i32){hi[0], hi[1]});
        x[t][3] = __builtin_bit_cast(double, (v2i32){hi[2], hi[3]});
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          x[t][j] = __builtin_bit_cast(
              double, __builtin_amdgcn_raw_buffer_load_b64(xR, f0 + j < F ? off + 8 * j : OOB, 0,
                                                           0));
      }
    }
  };
  cyc_double4 acc[2][CT];
  // labL / wL: lane l holds label and weight of row 32 wave + (l & 31)
  auto epilogue = [&](int64_t r0, double labL, double wL) {
    if constexpr ((CYC_MLR_PROBE & 2) != 0) {
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) ms[ct] += acc[t][ct][0];
      wsum += lane < 32 ? 1.0 : 0.0;   // a nonzero weight for the host's check
      return;
    }
    // Epilogue: lane holds rows 32 wave + 16 t + (lane>>4) + 4r, classes
    // 16 ct + (lane & 15).  Branch-free (selects, DPP row reductions, the
    // multiplier stores through a per-tile buffer descriptor that drops rows
    // past n), so the wave never splits; the only branch is the wave-uniform
    // one into the +inf margin case.  Each row's label probability is parked
    // in LDS and the tile's 32 logs per wave run once, one row per lane.
    // l15: the lane's class within a tile, opaque to the optimizer: values derived
    // from it are recomputed per tile instead of hoisted out of the tile loop
    // into registers (which spilled)
    int l15 = lane & 15;
    asm volatile("" : "+v"(l15));
    const int64_t nr = min<int64_t>(MR, n - r0);
    const auto mR = __builtin_amdgcn_make_buffer_rsrc((void*)(mult + r0 * CP), (short)0,
                                                      (int)(nr * CP * 8), 0x00020000);
#pragma unroll
    for (int t = 0; t < 2; ++t) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int rl = wave * 32 + t * 16 + (lane >> 4) + 4 * r;   // row within the tile
        const bool rowok = r0 + rl < n;
        double m[CT];
        // the row's max by fmax, +inf included (the reference leaves +inf
        // out of its max; a row holding one takes the branch below)
        double mx = -1.7976931348623157e308;  // Double.MinValue (Utils.scala:113)
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
          const int c = ct * 16 + l15;
          m[ct] = acc[t][ct][r] + offS[c];  // 1.0*temp + 1.0*offset (netlib dgemm)
          mx = fmax(mx, (ct < CT - 1 || c < C) ? m[ct] : mx);
        }
        mx = fmax(mx, dpp_f64<0xB1>(mx));   // quad_perm [1,0,3,2]
        mx = fmax(mx, dpp_f64<0x4E>(mx));   // quad_perm [2,3,0,1]
        mx = fmax(mx, dpp_f64<0x141>(mx));  // row_half_mirror
        mx = fmax(mx, dpp_f64<0x140>(mx));  // row_mirror
        // the probabilities replace the margins in place (p = m).  INF: the
        // wave holds a +inf margin (a wave-uniform branch, never taken on
        // finite margins): the max over the other classes, and for a row
        // holding one, probability 1 for the first such class and 0 * m for
        // the rest.
        auto softmax = [&](auto infTag) {
          constexpr bool INF = decltype(infTag)::value;
          int infc = 1 << 30;
          if constexpr (INF) {
            mx = -1.7976931348623157e308;
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) {
              const int c = ct * 16 + l15;
              const bool valid = ct < CT - 1 || c < C;
              if (valid && m[ct] == __builtin_inf()) infc = min(infc, c);
              else if (valid && m[ct] > mx) mx = m[ct];
            }
#pragma unroll
            for (int k = 1; k < 16; k <<= 1) {
              mx = fmax(mx, __shfl_xor(mx, k));
              infc = min(infc, __shfl_xor(infc, k));
            }
          }
          const bool rowInf = INF && infc < (1 << 30);
          double sum = 0.0;
#pragma unroll
          for (int ct = 0; ct < CT; ++ct) {
            const int c = ct * 16 + l15;
            const double e = (CYC_MLR_PROBE & 16) ? (m[ct] - mx) : exp_neg(m[ct] - mx, expT);
            const double pe = (ct < CT - 1 || c < C) ? e : 0.0;
            m[ct] = rowInf ? ((c == infc) ? 1.0 : 0.0 * m[ct]) : pe;
            sum += m[ct];
          }
          // butterfly sums in which both lanes of a pair add the same two
          // values: every lane of the row ends with the same bits
          sum += dpp_f64<0xB1>(sum);
          sum += dpp_f64<0x4E>(sum);
          sum += dpp_f64<0x141>(sum);
          sum += dpp_f64<0x140>(sum);
          const double inv = 1.0 / sum;
#pragma unroll
          for (int ct = 0; ct < CT; ++ct) m[ct] = rowInf ? m[ct] : inv * m[ct];
        };
        if (__builtin_amdgcn_ballot_w64(mx == __builtin_inf()) != 0)
          softmax(std::true_type{});
        else
          softmax(std::false_type{});
        double (&p)[CT] = m;
        // unconditional shuffles: a shuffle under `rowok` made the compiler
        // wait vmcnt(0) on labL / wL at every row, draining the stores
        const int q = 16 * t + 4 * r + (lane >> 4);   // the row within the wave's 32
        const double wq = __shfl(wL, q), lq = __shfl(labL, q);
        const double w = (rowok && wq > 0) ? wq : 0.0;
        const int label = rowok ? (int)lq : 0;
        const int voff = rowok ? (rl * CP + l15) * 8 : OOB;   // rows past n: dropped
        double pl = 0.0;
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) pl = (ct == (label >> 4)) ? p[ct] : pl;
        if ((lane & 15) == (label & 15)) plS[wave * 32 + q] = pl;
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
          const int c = ct * 16 + l15;
          // w p - w at the label (w * p is p at w = 1); 0 * p at w <= 0
          double mu = w * p[ct] - (c == label ? w : 0.0);
          mu = (ct < CT - 1 || c < C) && rowok ? mu : 0.0;
          if constexpr ((CYC_MLR_PROBE & 8) == 0)
            __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(v2i32, mu), mR,
                                                  voff + ct * 128, 0, 2);   // nontemporal
          ms[ct] += mu;
        }
        // one row group at a time: interleaving them spills
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    // the loss: row 32 wave + (lane & 31) on lanes 0..31
    const double pl = plS[wave * 32 + (lane & 31)];
    const double wr = (lane < 32 && r0 + wave * 32 + lane < n) ? wL : 0.0;
    wsum += wr;
    loss -= (wr > 0) ? wr * log(pl) : 0.0;
  };
  double xa[2][4], xb[2][4];
  bool pre = false;   // chunk 0 of this tile already in flight (xa, Ws[0])
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t r0 = tile * MR;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) acc[t][ct] = cyc_double4{0.0, 0.0, 0.0, 0.0};
    if (!pre) {
      __syncthreads();   // the previous tile's last W buffer is free
      loadW(0);
    }
    loadX(r0, 0, xa);
    // chunk ch: wait for its loads, barrier (its W visible everywhere, every
    // wave past chunk ch - 1), issue chunk ch + 1's loads, multiply
    auto step = [&](int ch, double (&xc)[2][4], double (&xn)[2][4]) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      if (ch + 1 < nch) {
        loadX(r0, ch + 1, xn);
        loadW(ch + 1);
      }
      const double* W = Ws[ch & 1];
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
          const double b = W[(4 * g + kk) * C + ct * 16 + (lane & 15)];
          acc[0][ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(xc[0][kk], b, acc[0][ct], 0, 0, 0);
          acc[1][ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(xc[1][kk], b, acc[1][ct], 0, 0, 0);
        }
      }
    };
    for (int ch = 0; ch < nch; ch += 2) {
      step(ch, xa, xb);
      if (ch + 1 < nch) step(ch + 1, xb, xa);
    }
    // the next tile's W chunk 0 goes out before this tile's epilogue (the X
    // registers stay free for it: prefetching X too spills at CT = 7): with
    // an even chunk count the last chunk read Ws[1], and every wave is past
    // chunk nch - 2 (Ws[0]) since the last barrier
    const int64_t next = tile + gridDim.x;
    pre = (nch % 2) == 0 && next < tiles;
    // the tile's labels and weights, loaded (unconditionally, from a
    // clamped row) before the W DMA and the stores of the epilogue
    const int64_t lr = min<int64_t>(r0 + wave * 32 + (lane & 31), n - 1);
    const double labL = labels[lr];
    const double wL = weights ? weights[lr] : 1.0;
    if (pre) loadW(0);
    epilogue(r0, labL, wL);
  }
  // per-wave partials: loss/wsum over the lanes (one row of each tile per
  // lane 0..31), multSum per class summed over the 4 row groups of the wave.
#pragma unroll
  for (int k = 1; k < 64; k <<= 1) {
    loss += __shfl_xor(loss, k);
    wsum += __shfl_xor(wsum, k);
  }
#pragma unroll
  for (int k = 16; k < 64; k <<= 1) {
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) ms[ct] += __shfl_xor(ms[ct], k);
  }
  const int64_t gw = (int64_t)blockIdx.x * (MT / 64) + wave;
  if (lane == 0) {
    slabS[gw * 2 + 0] = loss;
    slabS[gw * 2 + 1] = wsum;
  }
  if (lane < 16) {
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) slabMS[gw * CP + ct * 16 + lane] = ms[ct];
  }
}

constexpr int GR = 32;    // rows per chunk in the gradient GEMM
constexpr int GF = 256;   // features per workgroup

// grad^T (CP x GF per workgroup) = mult^T X over one split of rows, on
// v_mfma_f64_16x16x4f64 (8 waves x 32 features x CP classes).  Per 32-row
// chunk: the multipliers (32 x CP, contiguous) are DMA'd into one of two LDS
// buffers (buffer_load ... lds, 1 KiB pieces over the waves), X goes from
// HBM straight into registers in the MFMA B layout (lane: feature l & 15 of
// its 16-feature tile, row 4 kk + (l >> 4) of k-step kk; 128 contiguous
// bytes per row), both one chunk ahead; one barrier per chunk.
// T4 (C mod 16 in 1..4): the last class tile on v_mfma_f64_4x4x4f64, a
// quarter of the 16x16x4 cycles: 4 blocks of 4 x 4 x 4, lane 16k + 4b + i
// holding A(i, k), lane 16k + 4b + j B(k, j) of block b and lane 16i + 4b + j
// the result (measured on gfx950: tools/probe/mfma_f64_4x4.hip).  Here A =
// the 4 classes' multipliers of row k (the same for every block), B = the
// 16x16x4 X operand (block b: features 4b .. 4b + 3), so the result is class
// l >> 4, feature l & 15.
template <int CT, bool T4>
__global__ __launch_bounds__(512) void k_mlr_grad(const double* __restrict__ mult,
                                                  const double* __restrict__ X, int64_t n, int F,
                                                  int64_t rowsPerSplit, int ftiles, int splits,
                                                  double* __restrict__ slab) {
  constexpr int CP = CT * 16;
  constexpr int MB = GR * CP;                       // doubles per multiplier chunk
  constexpr int MPIECES = (MB * 8 + 1023) / 1024;
  __shared__ __attribute__((aligned(16))) double Ms[2][MPIECES * 128];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // 1-D grid: block b runs on XCD b % 8; the ftiles workgroups of a split
  // share that XCD (consecutive b / 8), so the split's multipliers come from
  // HBM once and from that XCD's L2 for the other feature tiles
  const int xq = (int)blockIdx.x >> 3;
  const int ft = xq % ftiles;
  const int sp = (xq / ftiles) * 8 + ((int)blockIdx.x & 7);
  if (sp >= splits) return;   // splits padded to a multiple of 8
  const int F0 = ft * GF;
  const int64_t r0 = (int64_t)sp * rowsPerSplit;
  const int64_t r1 = min<int64_t>(n, r0 + rowsPerSplit);
  cyc_double4 acc[CT][2];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) acc[ct][0] = acc[ct][1] = cyc_double4{0.0, 0.0, 0.0, 0.0};
  double acc4[2] = {0.0, 0.0};
  // Buffer descriptors over this split's rows: 32-bit offsets, rows past the
  // split and features past F read as zero.  Host: rowsPerSplit * max(F, CP)
  // * 8 < 2^31.
  constexpr int OOB = 0x7ff00000;
  const int64_t nr = r1 > r0 ? r1 - r0 : 0;
  const auto mR = __builtin_amdgcn_make_buffer_rsrc((void*)(mult + r0 * CP), (short)0,
                                                    (int)(nr * CP * 8), 0x00020000);
  const auto xR = __builtin_amdgcn_make_buffer_rsrc((void*)(X + r0 * F), (short)0,
                                                    (int)(nr * F * 8), 0x00020000);
  const int g = lane >> 4;
  const int fcol = F0 + wave * 32 + (lane & 15);
  auto loadM = [&](int64_t rb, int buf) {
    const int base = (int)(rb - r0) * CP * 8;
    for (int q = wave; q < MPIECES; q += 8)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(
          mR, (__attribute__((address_space(3))) void*)(&Ms[buf][q * 128]), 16,
          base + q * 1024 + lane * 16, 0, 0, 0);
  };
  auto loadX = [&](int64_t rb, double (&x)[GR / 4][2]) {
    const int rowOff = (int)(rb - r0);
#pragma unroll
    for (int kk = 0; kk < GR / 4; ++kk)
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int f = fcol + 16 * q;
        const int off = f < F ? ((rowOff + 4 * kk + g) * F + f) * 8 : OOB;
        x[kk][q] = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(xR, off, 0, 2));
      }
  };
  auto step = [&](int64_t rb, int buf, double (&xc)[GR / 4][2], double (&xn)[GR / 4][2]) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();   // chunk rb's multipliers visible; every wave past the previous chunk
    if (rb + GR < r1) {
      loadX(rb + GR, xn);
      loadM(rb + GR, buf ^ 1);
    }
    const double* M = Ms[buf];
#pragma unroll
    for (int kk = 0; kk < GR / 4; ++kk) {
#pragma unroll
      for (int ct = 0; ct < (T4 ? CT - 1 : CT); ++ct) {
        const double a = M[(4 * kk + g) * CP + ct * 16 + (lane & 15)];
        acc[ct][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, xc[kk][0], acc[ct][0], 0, 0, 0);
        acc[ct][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, xc[kk][1], acc[ct][1], 0, 0, 0);
      }
      if constexpr (T4) {
        const double a = M[(4 * kk + g) * CP + (CT - 1) * 16 + (lane & 3)];
        acc4[0] = __builtin_amdgcn_mfma_f64_4x4x4f64(a, xc[kk][0], acc4[0], 0, 0, 0);
        acc4[1] = __builtin_amdgcn_mfma_f64_4x4x4f64(a, xc[kk][1], acc4[1], 0, 0, 0);
      }
    }
  };
  if (r0 < r1) {
    double xa[GR / 4][2], xb[GR / 4][2];
    loadX(r0, xa);
    loadM(r0, 0);
    for (int64_t rb = r0; rb < r1; rb += 2 * GR) {
      step(rb, 0, xa, xb);
      if (rb + GR < r1) step(rb + GR, 1, xb, xa);
    }
  }
  // slab[split][ftile][c][f_local]
  double* out = slab + ((size_t)sp * ftiles + ft) * CP * GF;
#pragma unroll
  for (int ct = 0; ct < (T4 ? CT - 1 : CT); ++ct)
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int c = ct * 16 + (lane >> 4) + 4 * r;
        const int fl = wave * 32 + q * 16 + (lane & 15);
        out[(size_t)c * GF + fl] = acc[ct][q][r];
      }
  if constexpr (T4) {   // classes (CT - 1) 16 + 0..3; the fold reads only c < C
#pragma unroll
    for (int q = 0; q < 2; ++q)
      out[(size_t)((CT - 1) * 16 + (lane >> 4)) * GF + wave * 32 + q * 16 + (lane & 15)] = acc4[q];
  }
}

// grad[f*C + c] += sum_s slab (fixed order); the dger fitWithMean correction
// (:180-181) and the intercept daxpy (:184-185).  ms[CP] = total multSum.
__global__ void k_mlr_fold(const double* __restrict__ slab, int splits, int ftiles, int CP, int F,
                           int C, const double* __restrict__ ms, int fitIntercept,
                           int fitWithMean, const double* __restrict__ sm,
                           double* __restrict__ grad) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // c * F + f
  if (e < (int64_t)C * F) {
    const int c = (int)(e / F), f = (int)(e % F);
    const int ft = f / GF, fl = f % GF;
    double s = 0.0;
    for (int sp = 0; sp < splits; ++sp)
      s += slab[(((size_t)sp * ftiles + ft) * CP + c) * GF + fl];
    double g = 1.0 * s + 1.0 * grad[(int64_t)f * C + c];
    if (fitIntercept && fitWithMean && sm[f] != 0.0) g = g + ms[c] * (-1.0 * sm[f]);
    grad[(int64_t)f * C + c] = g;
  }
  if (fitIntercept && e < C) grad[(int64_t)C * F + e] = grad[(int64_t)C * F + e] + 1.0 * ms[e];
}

// Fold per-wave class sums: out[c] = sum_w slabMS[w][c].  One 256-thread
// workgroup per column: thread t sums rows t, t+256, ... in order, then a
// fixed LDS tree -- deterministic, and no 2048-long dependent chain.
__global__ __launch_bounds__(256) void k_fold_columns(const double* __restrict__ slab,
                                                      int64_t rows, int width,
                                                      double* __restrict__ out) {
  __shared__ double sh[256];
  const int c = blockIdx.x, t = threadIdx.x;
  double s = 0.0;
  for (int64_t w = t; w < rows; w += 256) s += slab[w * width + c];
  sh[t] = s;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (t < h) sh[t] += sh[t + h];
    __syncthreads();
  }
  if (t == 0) out[c] = sh[0];
}

// ----------------------------------------------------- multinomial, CSR rows
// margins (:112-122 with the sparse-A gemm of ml/linalg/BLAS.scala:430-536:
// per row, t = sum over its nonzeros in order of value * linear(c, col), then
// C(i, c) = 1.0 * C(i, c) + t * 1.0 over the offset), Utils.softmax, loss and
// multipliers (:129-142) as in k_mlr_margins.  One wave per row, class
// c = lane + 64 q on its lane (CQ = classes per lane); mult is n x C.
// Per-wave partials: slabS[w][2] = (loss, weight), slabMS[w][C] = multSum.
template <int CQ>
__global__ __launch_bounds__(256) void k_mlr_csr_margins(
    const int64_t* __restrict__ rowptr, const int32_t* __restrict__ colidx,
    const double* __restrict__ vals, const double* __restrict__ labels,
    const double* __restrict__ weights, int64_t n, int C, const double* __restrict__ coef,
    const double* __restrict__ offset, double* __restrict__ mult, double* __restrict__ slabS,
    double* __restrict__ slabMS) {
  const int lane = threadIdx.x & 63;
  const int64_t gw = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
  double offc[CQ], ms[CQ];
#pragma unroll
  for (int q = 0; q < CQ; ++q) {
    const int c = lane + 64 * q;
    offc[q] = (offset && c < C) ? offset[c] : 0.0;
    ms[q] = 0.0;
  }
  double loss = 0.0, wsum = 0.0;
  for (int64_t r = gw; r < n; r += nw) {
    double t[CQ];
#pragma unroll
    for (int q = 0; q < CQ; ++q) t[q] = 0.0;
    const int64_t p1 = rowptr[r + 1];
    for (int64_t p = rowptr[r]; p < p1; ++p) {
      const double v = vals[p];
      const double* lin = coef + (int64_t)colidx[p] * C;
#pragma unroll
      for (int q = 0; q < CQ; ++q) {
        const int c = lane + 64 * q;
        if (c < C) t[q] = t[q] + v * lin[c];
      }
    }
    double m[CQ];
    double mx = -1.7976931348623157e308;   // Double.MinValue (Utils.scala:113)
    int infc = 1 << 30;
#pragma unroll
    for (int q = 0; q < CQ; ++q) {
      const int c = lane + 64 * q;
      m[q] = 1.0 * offc[q] + t[q] * 1.0;
      if (c < C) {
        if (m[q] == __builtin_inf()) infc = min(infc, c);
        else if (m[q] > mx) mx = m[q];
      }
    }
#pragma unroll
    for (int k = 1; k < 64; k <<= 1) {
      mx = fmax(mx, __shfl_xor(mx, k));
      infc = min(infc, __shfl_xor(infc, k));
    }
    double pr[CQ];
    if (infc < (1 << 30)) {
#pragma unroll
      for (int q = 0; q < CQ; ++q) {
        const int c = lane + 64 * q;
        pr[q] = (c == infc) ? 1.0 : 0.0 * m[q];
      }
    } else {
      double sum = 0.0;
#pragma unroll
      for (int q = 0; q < CQ; ++q) {
        const int c = lane + 64 * q;
        pr[q] = (c < C) ? exp(m[q] - mx) : 0.0;
        sum += pr[q];
      }
      sum = wave_sum_bcast(sum);
      const double inv = 1.0 / sum;
#pragma unroll
      for (int q = 0; q < CQ; ++q) pr[q] = inv * pr[q];
    }
    const double w = weights ? weights[r] : 1.0;
    const int label = (int)labels[r];
    double pl = 0.0;
#pragma unroll
    for (int q = 0; q < CQ; ++q)
      if (q == (label >> 6)) pl = pr[q];
    pl = __shfl(pl, label & 63);
    wsum += w;
    if (w > 0) loss -= w * log(pl);
#pragma unroll
    for (int q = 0; q < CQ; ++q) {
      const int c = lane + 64 * q;
      double mu;
      if (w > 0) {
        mu = (w != 1.0) ? w * pr[q] : pr[q];
        if (c == label) mu -= w;
      } else {
        mu = 0.0 * pr[q];
      }
      if (c < C) {
        mult[r * C + c] = mu;
        ms[q] += mu;
      }
    }
  }
  if (lane == 0) {
    slabS[gw * 2 + 0] = loss;
    slabS[gw * 2 + 1] = wsum;
  }
#pragma unroll
  for (int q = 0; q < CQ; ++q) {
    const int c = lane + 64 * q;
    if (c < C) slabMS[gw * C + c] = ms[q];
  }
}

// gradient over the row-blocked CSC copy (:156-162, linearGradSumMat =
// sm^T x mat): one wave per feature f, classes on lanes, blocks in order and
// each block's rows in order; then gradientSumArray(f C + c) += v and the
// fitWithMean dger correction (:175-182) with the total multiplier sums ms.
template <int CQ>
__global__ __launch_bounds__(256) void k_mlr_csc_grad(
    const int64_t* __restrict__ colptr, const int32_t* __restrict__ rowidx,
    const double* __restrict__ cv, int64_t nb, int F, int C, const double* __restrict__ mult,
    const double* __restrict__ ms, int fitIntercept, int fitWithMean,
    const double* __restrict__ sm, double* __restrict__ grad) {
  const int lane = threadIdx.x & 63;
  const int64_t f = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (f >= F) return;
  double tot[CQ];
#pragma unroll
  for (int q = 0; q < CQ; ++q) tot[q] = 0.0;
  for (int64_t b = 0; b < nb; ++b) {
    const int64_t e = b * F + f;
    double sb[CQ];
#pragma unroll
    for (int q = 0; q < CQ; ++q) sb[q] = 0.0;
    const int64_t k1 = colptr[e + 1];
    for (int64_t k = colptr[e]; k < k1; ++k) {
      const double v = cv[k];
      const double* mrow = mult + (int64_t)rowidx[k] * C;
#pragma unroll
      for (int q = 0; q < CQ; ++q) {
        const int c = lane + 64 * q;
        if (c < C) sb[q] = sb[q] + v * mrow[c];
      }
    }
#pragma unroll
    for (int q = 0; q < CQ; ++q) tot[q] = tot[q] + sb[q];
  }
#pragma unroll
  for (int q = 0; q < CQ; ++q) {
    const int c = lane + 64 * q;
    if (c >= C) continue;
    double g = grad[f * C + c] + tot[q];
    if (fitIntercept && fitWithMean && sm[f] != 0.0) g = g + ms[c] * (-1.0 * sm[f]);
    grad[f * C + c] = g;
  }
}

// intercept gradient (:184-185): grad[C F + c] += 1.0 * multSum[c]
__global__ void k_mlr_icpt(int F, int C, const double* __restrict__ ms, double* __restrict__ grad) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < C) grad[(int64_t)C * F + c] = grad[(int64_t)C * F + c] + 1.0 * ms[c];
}

// The per-class margin offsets in HBM (held under the plan mutex): *off is
// nullptr without an intercept, the intercepts themselves without centering.
int mlr_offset(cyc_logistic_plan p, const double* coef, const double* scaledMean, hipStream_t st,
               const double** off) {
  const int F = p->F, C = p->C;
  *off = nullptr;
  if (!p->fitIntercept) return CYC_OK;
  if (!p->fitWithMean) {
    *off = coef + (int64_t)C * F;
    return CYC_OK;
  }
  if (int rc = p->offset.reserve(sizeof(double) * (size_t)C)) return rc;
  hipLaunchKernelGGL(k_mlr_offset, dim3((C + 63) / 64), dim3(64), 0, st, coef, scaledMean, F, C,
                     (double*)p->offset.ptr);
  CYC_LAUNCH_CHECK("k_mlr_offset");
  *off = (const double*)p->offset.ptr;
  return CYC_OK;
}

// launch(std::integral_constant<int, N>) for the kernels' class-count template
// argument: CT = 16-class tiles, 1..8 (dense); CQ = classes per lane, the
// power of two >= cq up to 16 (CSR)
template <class Launch>
void for_ct(int CT, Launch&& launch) {
  switch (CT) {
    case 1: launch(std::integral_constant<int, 1>{}); break;
    case 2: launch(std::integral_constant<int, 2>{}); break;
    case 3: launch(std::integral_constant<int, 3>{}); break;
    case 4: launch(std::integral_constant<int, 4>{}); break;
    case 5: launch(std::integral_constant<int, 5>{}); break;
    case 6: launch(std::integral_constant<int, 6>{}); break;
    case 7: launch(std::integral_constant<int, 7>{}); break;
    default: launch(std::integral_constant<int, 8>{}); break;
  }
}

template <class Launch>
void for_cq(int cq, Launch&& launch) {
  if (cq <= 1) launch(std::integral_constant<int, 1>{});
  else if (cq <= 2) launch(std::integral_constant<int, 2>{});
  else if (cq <= 4) launch(std::integral_constant<int, 4>{});
  else if (cq <= 8) launch(std::integral_constant<int, 8>{});
  else launch(std::integral_constant<int, 16>{});
}

}  // namespace

extern "C" {

int cyc_multinomial_logistic_add_dense_dev(cyc_logistic_plan p, const double* X,
                                           const double* labels, const double* weights,
                                           int64_t n, const double* coef,
                                           const double* scaledMean, double* grad,
                                           double* lossSum, double* weightSum, void* stream) {
  int rc = check_common(p, coef, scaledMean);
  if (rc) return rc;
  CYC_REQUIRE(n >= 0, "n >= 0");
  if (n == 0) return CYC_OK;
  const int F = p->F, C = p->C;
  if (C > 128) {
    cyc::set_error("multinomial aggregator supports numClasses <= 128");
    return CYC_ERR_UNSUPPORTED;
  }
  if (((int64_t)C * F + C) * 8 >= INT32_MAX || (int64_t)MR * F * 8 >= INT32_MAX) {
    cyc::set_error("dense multinomial aggregator supports numClasses * numFeatures < 2^28 "
                   "and numFeatures < 2^20");
    return CYC_ERR_UNSUPPORTED;
  }
  const int CT = (C + 15) / 16, CP = CT * 16;
  std::lock_guard<std::mutex> g(p->mu);
  hipStream_t st = cyc::as_stream(stream);
  // Rows are processed in chunks of up to 8M so the multiplier matrix stays
  // bounded (8M x CP doubles: 7.3 GB at C = 100); a whole 6.25M-row shard of
  // the 8-GPU config is one launch (no second partial round of tiles).
  const int64_t chunk = std::min<int64_t>(n, 8 << 20);
  // k_mlr_grad: the last class tile on the 4x4x4 form when it holds 1..4
  // classes (2.6 % faster at C = 100)
  const bool t4 = C % 16 != 0 && C % 16 <= 4;
  // persistent: one 8-wave workgroup per CU (CYC_MLR_NW = 4: two 4-wave ones)
  constexpr int mnw = CYC_MLR_NW, mrows = 32 * mnw;
  const int mblocks = 256 * 8 / mnw;
  const int64_t mwaves = (int64_t)mblocks * mnw;
  const int ftiles = (F + GF - 1) / GF;
  if ((rc = p->multBuf.reserve(sizeof(double) * (size_t)chunk * CP)) ||
      (rc = p->slabS.reserve(sizeof(double) * (size_t)mwaves * 2)) ||
      (rc = p->slabMS.reserve(sizeof(double) * (size_t)mwaves * CP)) ||
      (rc = p->scal.reserve(sizeof(double) * 4)) ||
      (rc = p->msTot.reserve(sizeof(double) * CP)))
    return rc;
  const double* off = nullptr;
  if ((rc = mlr_offset(p, coef, scaledMean, st, &off))) return rc;
  for (int64_t c0 = 0; c0 < n; c0 += chunk) {
    const int64_t m = std::min(chunk, n - c0);
    const double* Xc = X + c0 * F;
    const double* lc = labels + c0;
    const double* wc = weights ? weights + c0 : nullptr;
    const int64_t tiles = (m + mrows - 1) / mrows;
    const unsigned mb = (unsigned)std::min<int64_t>(mblocks, tiles);
    CYC_HIP(hipMemsetAsync(p->slabS.ptr, 0, sizeof(double) * (size_t)mwaves * 2, st));
    CYC_HIP(hipMemsetAsync(p->slabMS.ptr, 0, sizeof(double) * (size_t)mwaves * CP, st));
    {
      cyc::KernelTimer tm("k_mlr_margins", st);
      for_ct(CT, [&](auto ct) {
        hipLaunchKernelGGL(
            HIP_KERNEL_NAME(k_mlr_margins<decltype(ct)::value, mnw, CYC_MLR_DEPHASE>), dim3(mb),
            dim3(64 * mnw), 0, st, Xc, lc, wc, m, F, C, coef, off, (double*)p->multBuf.ptr,
            (double*)p->slabS.ptr, (double*)p->slabMS.ptr);
      });
      CYC_LAUNCH_CHECK("k_mlr_margins");
    }
    // split-K over rows for the gradient GEMM: ~1024 workgroups (4 rounds of
    // one per CU; fewer splits keep the k_mlr_fold read of the partials small)
    int64_t splits = std::max<int64_t>(1, 1024 / ftiles);
    splits = std::min<int64_t>(splits, std::max<int64_t>(1, m / 64));
    int64_t rps = cyc::round_up((m + splits - 1) / splits, GR);
    // k_mlr_grad's buffer descriptors span one split: keep it under 2^31 bytes
    const int64_t maxRps = ((int64_t)INT32_MAX / 8 / std::max(F, CP)) / GR * GR - GR;
    if (rps > maxRps) rps = std::max<int64_t>(GR, maxRps);
    splits = (m + rps - 1) / rps;
    if ((rc = p->gslab.reserve(sizeof(double) * (size_t)splits * ftiles * CP * GF))) return rc;
    const unsigned gblocks = (unsigned)(ftiles * cyc::round_up(splits, (int64_t)8));
    {
      cyc::KernelTimer tg("k_mlr_grad", st);
      for_ct(CT, [&](auto ct) {
        constexpr int CTV = decltype(ct)::value;
        const auto kern = t4 ? k_mlr_grad<CTV, true> : k_mlr_grad<CTV, false>;
        hipLaunchKernelGGL(kern, dim3(gblocks), dim3(512), 0, st, (const double*)p->multBuf.ptr,
                           Xc, m, F, rps, ftiles, (int)splits, (double*)p->gslab.ptr);
      });
      CYC_LAUNCH_CHECK("k_mlr_grad");
    }
    hipLaunchKernelGGL(k_fold_columns, dim3(CP), dim3(256), 0, st,
                       (const double*)p->slabMS.ptr, mwaves, CP, (double*)p->msTot.ptr);
    CYC_LAUNCH_CHECK("k_fold_columns");
    if ((rc = cyc::fold_scalars((const double*)p->slabS.ptr, mwaves, 2, (double*)p->scal.ptr, st)))
      return rc;
    const int64_t tot = std::max<int64_t>((int64_t)C * F, C);
    hipLaunchKernelGGL(k_mlr_fold, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st,
                       (const double*)p->gslab.ptr, (int)splits, ftiles, CP, F, C,
                       (const double*)p->msTot.ptr, p->fitIntercept, p->fitWithMean, scaledMean,
                       grad);
    CYC_LAUNCH_CHECK("k_mlr_fold");
    if ((rc = cyc::add_scalars((const double*)p->scal.ptr, lossSum, weightSum, st))) return rc;
  }
  return CYC_OK;
}

int cyc_multinomial_logistic_add_csr_dev(cyc_logistic_plan p, const int64_t* rowptr,
                                         const int32_t* colidx, const double* vals,
                                         const double* labels, const double* weights, int64_t n,
                                         const double* coef, const double* scaledMean,
                                         double* grad, double* lossSum, double* weightSum,
                                         cyc_csc csc, void* stream) {
  int rc = check_common(p, coef, scaledMean);
  if (rc) return rc;
  CYC_REQUIRE(n >= 0, "n >= 0");
  if (n == 0) return CYC_OK;
  const int F = p->F, C = p->C;
  CYC_REQUIRE(csc != nullptr && cyc_csc_rows(csc) == n && cyc_csc_features(csc) == F,
              "a CSC copy of these rows is required (cyc_csc_build_dev)");
  if (C > 1024) {
    cyc::set_error("multinomial CSR aggregator supports numClasses <= 1024");
    return CYC_ERR_UNSUPPORTED;
  }
  const int cq = (C + 63) / 64;
  std::lock_guard<std::mutex> g(p->mu);
  hipStream_t st = cyc::as_stream(stream);
  const int64_t waves = std::min<int64_t>(n, 8192);
  const unsigned blocks = (unsigned)((waves + 3) / 4);
  const int64_t wtot = (int64_t)blocks * 4;
  if ((rc = p->multBuf.reserve(sizeof(double) * (size_t)n * C)) ||
      (rc = p->slabS.reserve(sizeof(double) * (size_t)wtot * 2)) ||
      (rc = p->slabMS.reserve(sizeof(double) * (size_t)wtot * C)) ||
      (rc = p->scal.reserve(sizeof(double) * 4)) ||
      (rc = p->msTot.reserve(sizeof(double) * (size_t)C)))
    return rc;
  const double* off = nullptr;
  if ((rc = mlr_offset(p, coef, scaledMean, st, &off))) return rc;
  CYC_HIP(hipMemsetAsync(p->slabS.ptr, 0, sizeof(double) * (size_t)wtot * 2, st));
  CYC_HIP(hipMemsetAsync(p->slabMS.ptr, 0, sizeof(double) * (size_t)wtot * C, st));
  double* mult = (double*)p->multBuf.ptr;
  {
    cyc::KernelTimer tm("k_mlr_csr_margins", st);
    for_cq(cq, [&](auto q) {
      hipLaunchKernelGGL(k_mlr_csr_margins<decltype(q)::value>, dim3(blocks), dim3(256), 0, st,
                         rowptr, colidx, vals, labels, weights, n, C, coef, off, mult,
                         (double*)p->slabS.ptr, (double*)p->slabMS.ptr);
    });
    CYC_LAUNCH_CHECK("k_mlr_csr_margins");
  }
  hipLaunchKernelGGL(k_fold_columns, dim3(C), dim3(256), 0, st,
                     (const double*)p->slabMS.ptr, wtot, C, (double*)p->msTot.ptr);
  CYC_LAUNCH_CHECK("k_fold_columns");
  if ((rc = cyc::fold_scalars((const double*)p->slabS.ptr, wtot, 2, (double*)p->scal.ptr, st)))
    return rc;
  int64_t R = 0, nb = 0;
  if ((rc = cyc_csc_blocks(csc, &R, &nb))) return rc;
  const int64_t* colptr;
  const int32_t* rowidx;
  const double* cv;
  if ((rc = cyc_csc_arrays(csc, &colptr, &rowidx, &cv))) return rc;
  const unsigned gblocks = (unsigned)(((int64_t)F + 3) / 4);
  {
    cyc::KernelTimer tg("k_mlr_csc_grad", st);
    for_cq(cq, [&](auto q) {
      hipLaunchKernelGGL(k_mlr_csc_grad<decltype(q)::value>, dim3(gblocks), dim3(256), 0, st,
                         colptr, rowidx, cv, nb, F, C, (const double*)mult,
                         (const double*)p->msTot.ptr, p->fitIntercept, p->fitWithMean, scaledMean,
                         grad);
    });
    CYC_LAUNCH_CHECK("k_mlr_csc_grad");
  }
  if (p->fitIntercept) {
    hipLaunchKernelGGL(k_mlr_icpt, dim3((C + 255) / 256), dim3(256), 0, st, F, C,
                       (const double*)p->msTot.ptr, grad);
    CYC_LAUNCH_CHECK("k_mlr_icpt");
  }
  return cyc::add_scalars((const double*)p->scal.ptr, lossSum, weightSum, st);
}

int cyc_softmax_exp_dev(const double* x, int64_t n, double* out, void* stream) {
  CYC_REQUIRE(n >= 0 && (n == 0 || (x && out)), "n >= 0 and non-null buffers");
  if (n == 0) return CYC_OK;
  const int64_t grid = std::min<int64_t>((n + 255) / 256, 8192);
  hipLaunchKernelGGL(k_softmax_exp, dim3((unsigned)grid), dim3(256), 0, cyc::as_stream(stream), x,
                     n, out);
  CYC_LAUNCH_CHECK("k_softmax_exp");
  return CYC_OK;
}

}  // extern "C"
