// kmeans_i8_cands.hip -- the candidate tiers of the d <= 256 screen: rows a
// screen pass could not certify but left with a small candidate set are
// decided against that set alone, by exact fp64 distances (k_screen_cands)
// or, ahead of it, by the three-limb integer products (k_screen_cands3); and
// the re-check of the carried sets (k_recheck).  The bounds they certify with
// are derived at the head of kmeans_i8.hip.
#include "kmeans_i8_dev.hpp"

namespace cyc {
namespace km8 {
namespace {

// Candidate rows (one wave each): fp64 squared distances to the <= kCandMax
// candidates, summed over the lanes' dimensions (any order: the error is
// <= (d + 2) 2^-53 2 (|x|^2 + |c|^2) < 2^-40 (|x|^2 + |c|^2)); |c| from the
// screen's center norms (an fp64 norm: its rounding sits far inside margin).  The row is
// certified when the second smallest exceeds the smallest by margin (|x|^2
// + |c_best|^2) plus both errors: every other center was already excluded by
// the two-limb bounds (by the screen's own margin), so the best candidate
// is the reference loop's answer as for any certified row.  Ties and near
// ties go on to list (the fp64 screen, then the reference loop).
// 16-lane row sum by DPP row rotations (VALU, no LDS): every lane of the
// row ends with the total.
__device__ __forceinline__ double row16_sum(double v) {
#define CYC_ROR(CTRL)                                                                        \
  {                                                                                          \
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xF, 0xF, false); \
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xF, 0xF, false); \
    v += __hiloint2double(hi, lo);                                                           \
  }
  CYC_ROR(0x128) CYC_ROR(0x124) CYC_ROR(0x122) CYC_ROR(0x121)
#undef CYC_ROR
  return v;
}

__global__ __launch_bounds__(256) void k_screen_cands(
    const double* __restrict__ X, const double* __restrict__ xnorm, int d,
    const double* __restrict__ C, const double* __restrict__ cnorm, int k, bool unit,
    double margin, const int32_t* __restrict__ candRows, const int32_t* __restrict__ cands,
    const unsigned int* __restrict__ candCount, int32_t* __restrict__ assign,
    int32_t* __restrict__ list, unsigned int* __restrict__ listCount, unsigned int scap) {
  // 2 rows per wave, 32 lanes per row; lane s of a row holds the dimensions
  // s, s + 32, ... (each load instruction reads 256 contiguous bytes per
  // row), and every load of a row -- its x and all kCandMax candidate rows
  // -- is in flight at once: one memory latency per row after its indices
  // (4 rows x 16 lanes with the candidates in two batches took three)
  const unsigned cnt = *candCount;
  const int lane = threadIdx.x & 63, q = lane >> 5, sl = lane & 31;
  const unsigned nw = (gridDim.x * blockDim.x) >> 6;
  const unsigned w0 = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (scap) {   // this wave's shard (<= 4 rows per grid stride: shard_cap)
    list += (size_t)(w0 % kShards) * scap;
    listCount += (w0 % kShards) * kShardStride;
  }
  for (unsigned base = w0 * 2; base < cnt; base += nw * 2) {
    const unsigned idx = base + q;
    const bool live = idx < cnt;
    const int64_t row = live ? candRows[idx] : 0;
    int ci[kCandMax];
#pragma unroll
    for (int i = 0; i < kCandMax; ++i) ci[i] = live ? cands[(size_t)idx * kCandMax + i] : -1;
    bool bad = false;
#pragma unroll
    for (int i = 0; i < kCandMax; ++i) bad = bad || ci[i] >= k;   // a padding center
    const double* x = X + row * d;
    double u[8], cv[kCandMax][8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int j = e * 32 + sl;   // d <= 256
      u[e] = (live && j < d) ? x[j] : 0.0;
    }
#pragma unroll
    for (int i = 0; i < kCandMax; ++i) {
      const int c = ci[i];
      const bool on = c >= 0 && c < k;
      const double* cr = C + (int64_t)(on ? c : 0) * d;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int j = e * 32 + sl;
        cv[i][e] = (on && j < d) ? cr[j] : 0.0;
      }
    }
    if (unit) {
      const double inv = live ? 1.0 / xnorm[row] : 0.0;
#pragma unroll
      for (int e = 0; e < 8; ++e) u[e] = u[e] * inv;
    }
    double xx = 0.0;
#pragma unroll
    for (int e = 0; e < 8; ++e) xx += u[e] * u[e];
    double part[kCandMax];
#pragma unroll
    for (int i = 0; i < kCandMax; ++i) {
      double s2 = 0.0;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const double t = cv[i][e] - u[e];
        s2 += t * t;
      }
      part[i] = s2;
    }
    // sums over the row's 32 lanes: within each 16-lane row by DPP, then
    // the two halves
    xx = row16_sum(xx);
    xx += __shfl_xor(xx, 16);
#pragma unroll
    for (int i = 0; i < kCandMax; ++i) {
      part[i] = row16_sum(part[i]);
      part[i] += __shfl_xor(part[i], 16);
    }
    double best = __builtin_inf(), second = __builtin_inf();
    int bi = -1, si = -1;
#pragma unroll
    for (int i = 0; i < kCandMax; ++i) {
      if (ci[i] < 0 || ci[i] >= k) continue;
      const double s2 = part[i];
      if (s2 < best) {
        second = best;
        si = bi;
        best = s2;
        bi = ci[i];
      } else if (s2 < second) {   // an equal distance lands here: no certification
        second = s2;
        si = ci[i];
      }
    }
    bool ok = !bad && bi >= 0 && __builtin_isfinite(best) && __builtin_isfinite(xx);
    if (ok && second != __builtin_inf()) {   // one candidate: certified as it is
      const double cb = cnorm[bi], cs = si >= 0 ? cnorm[si] : 0.0;
      const double ccb = cb * cb, ccs = cs * cs;
      const double M = margin * (xx + ccb) + 0x1p-40 * (2.0 * xx + ccb + ccs);
      ok = __builtin_isfinite(M) && (second - best) > M * (1.0 + 0x1p-30);
    }
    if (live && sl == 0) {
      if (ok) assign[row] = bi;
      else list[atomicAdd(listCount, 1u)] = (int32_t)row;
    }
  }
}

// Three-limb tier of the candidate rows, ahead of k_screen_cands: for each
// of a row's <= kCandMax candidates the exact integer limb products S1 =
// a.a', S2 = a.b' + b.a', S3 = a.c' + b.b' + c.a' of the row image and the
// center-major copy of the center image (v_dot4 over 2S lanes per row, 16
// dimensions a lane: 768 B per row and per candidate at d = 256, against
// 2 KB of fp64 each in k_screen_cands), bounded exactly as the three-limb
// pass bounds them (k_screen32<.., 3, ..>: the same f32 lower bounds L,
// rounded down, and the same certification margin M), over the candidates
// instead of every center.  A row is certified when its best candidate
// beats every other candidate by M: the candidates exclude every other
// center (by the two-limb margin against the two-limb winner, itself a
// candidate), so the best candidate is the reference loop's answer, as in
// k_screen_cands.  The other rows go on with their candidates to
// k_screen_cands (out*).
__device__ __forceinline__ int dot16(uint4 u, uint4 v, int acc) {
  acc = __builtin_amdgcn_sdot4((int)u.x, (int)v.x, acc, false);
  acc = __builtin_amdgcn_sdot4((int)u.y, (int)v.y, acc, false);
  acc = __builtin_amdgcn_sdot4((int)u.z, (int)v.z, acc, false);
  return __builtin_amdgcn_sdot4((int)u.w, (int)v.w, acc, false);
}
__device__ __forceinline__ int dot16(uint2 u, uint2 v, int acc) {
  acc = __builtin_amdgcn_sdot4((int)u.x, (int)v.x, acc, false);
  return __builtin_amdgcn_sdot4((int)u.y, (int)v.y, acc, false);
}

// 16-lane integer row sum by DPP row rotations: every lane of the row ends
// with the total
__device__ __forceinline__ int row16_isum(int v) {
  v += __builtin_amdgcn_update_dpp(0, v, 0x128, 0xF, 0xF, false);   // row_ror:8
  v += __builtin_amdgcn_update_dpp(0, v, 0x124, 0xF, 0xF, false);   // row_ror:4
  v += __builtin_amdgcn_update_dpp(0, v, 0x122, 0xF, 0xF, false);   // row_ror:2
  return v + __builtin_amdgcn_update_dpp(0, v, 0x121, 0xF, 0xF, false);   // row_ror:1
}

// PB: bytes of a limb plane per lane (16: 2S lanes per row; 8: 4S lanes,
// measured 0.94 vs 0.59 ms at 5 waves per SIMD against 4)
// RC (the carried candidate sets, kmeans_i8.hpp Bounds): the rows of
// candRows re-checked against the candidate set their last screen left
// (cands = Bounds::sets, indexed by ROW), certified when the best candidate
// beats the others by M and its upper bound stays below the set's carried
// lower bound for every other center (Bounds::lnc, moved by the drift) by
// the reference's slack; state[row] = 0 (certified) or 1 (a full screen).
template <int S, int PB, bool RC = false>
__global__ __launch_bounds__(256) void k_screen_cands3(
    const uint4* __restrict__ Xq, const int2* __restrict__ meta, const double* __restrict__ xnorm,
    int d, const uint4* __restrict__ Cr, const float* __restrict__ cq,
    const double* __restrict__ g, const double* __restrict__ cnorm,
    const CenterParams* __restrict__ prm, const int32_t* __restrict__ candRows,
    const int32_t* __restrict__ cands, const unsigned int* __restrict__ candCount,
    int32_t* __restrict__ assign, int32_t* __restrict__ outRows, int32_t* __restrict__ outCands,
    unsigned int* __restrict__ outCount, unsigned int scap, float2* __restrict__ bnd,
    float* __restrict__ lncA, int32_t* __restrict__ sets, unsigned char* __restrict__ state,
    const DriftParams* __restrict__ dp, const int32_t* __restrict__ nbr,
    const float* __restrict__ nbrR) {
  using Pc = std::conditional_t<PB == 16, uint4, uint2>;
  constexpr int P16 = 32 * S / PB;    // pieces per limb plane = lanes per row
  constexpr int RPW = 64 / P16;       // rows per wave
  const unsigned cnt = *candCount;
  const int lane = threadIdx.x & 63, q = lane / P16, li = lane % P16;
  const unsigned nw = (gridDim.x * blockDim.x) >> 6;
  const unsigned w0 = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (scap) {   // this wave's shard (<= RPW rows per grid stride: shard_cap)
    const unsigned sh = w0 % kShards;
    outRows += (size_t)sh * scap;
    outCands += (size_t)sh * scap * kCandMax;
    outCount += sh * kShardStride;
  }
  const CenterParams P = *prm;
  const auto cR = __builtin_amdgcn_make_buffer_rsrc(
      (void*)Cr, (short)0, (int)std::min<int64_t>((int64_t)P.k * 3 * P16 * PB, 0x7fffffff),
      0x00020000);
  for (unsigned base = w0 * RPW; base < cnt; base += nw * RPW) {
    const unsigned idx = base + q;
    const bool live = idx < cnt;
    const int32_t rw = live ? candRows[idx] : 0;
    // RC: a row listed as ~row re-checks the neighbourhood of its center
    // (set slot 0 = that center; the filter's state 3)
    const bool nbrMode = RC && rw < 0;
    const int64_t row = nbrMode ? ~rw : rw;
    const int32_t* setp = nbrMode ? nbr + (size_t)assign[row] * kCandMax
                                  : cands + (size_t)(RC ? row : (int64_t)idx) * kCandMax;
    int ci[kCandMax];
#pragma unroll
    for (int i = 0; i < kCandMax; ++i) ci[i] = live ? setp[i] : -1;
    const Pc* xr = (const Pc*)Xq + row * (3 * P16) + li;
    const Pc xa = xr[0], xb = xr[P16], xc = xr[2 * P16];
    // the row's and the candidates' scalars issued with the gathers (each
    // one waited for on its own after them cost a round trip apiece)
    const int2 mt = live ? meta[row] : make_int2(INT_MIN, 0);
    const double xnr = xnorm[row];
    float cqv[kCandMax];
#pragma unroll
    for (int i = 0; i < kCandMax; ++i) cqv[i] = cq[(ci[i] >= 0 && ci[i] < P.k) ? ci[i] : 0];
    float lncR = 0.0f;
    float2 bndR = make_float2(0.0f, 0.0f);
    double cnA = 0.0, gA = 0.0;
    float RA = 0.0f;
    if (bnd) {
      if (RC) lncR = lncA[row];
      else bndR = bnd[row];
    }
    if (nbrMode) {   // the anchor's terms for its fresh upper bound
      const int a0 = (ci[0] >= 0 && ci[0] < P.k) ? ci[0] : 0;
      cnA = cnorm[a0];
      gA = g[a0];
      RA = nbrR[a0];
    }
    int s1[kCandMax], s2[kCandMax], s3[kCandMax];
#pragma unroll
    for (int i = 0; i < kCandMax; ++i) {
      const int c = ci[i];
      Pc ca, cb, cc;
      if constexpr (PB == 16) {
        // empty slots fetch nothing: an out-of-range buffer offset reads
        // zeros without a memory access (the kernel is bound by these L2
        // gathers, 768 B per candidate), and every slot's loads stay in
        // flight together
        const unsigned off = (c >= 0 && c < P.k) ? (unsigned)(c * 3 * P16 + li) * 16u
                                                 : 0x80000000u;
        ca = __builtin_bit_cast(Pc, __builtin_amdgcn_raw_buffer_load_b128(cR, (int)off, 0, 0));
        cb = __builtin_bit_cast(Pc, __builtin_amdgcn_raw_buffer_load_b128(
                                        cR, (int)(off + 16u * P16), 0, 0));
        cc = __builtin_bit_cast(Pc, __builtin_amdgcn_raw_buffer_load_b128(
                                        cR, (int)(off + 32u * P16), 0, 0));
      } else {
        const Pc* cr = (const Pc*)Cr + (size_t)((c >= 0 && c < P.k) ? c : 0) * (3 * P16) + li;
        ca = cr[0];
        cb = cr[P16];
        cc = cr[2 * P16];
      }
      s1[i] = dot16(xa, ca, 0);
      s2[i] = dot16(xb, ca, dot16(xa, cb, 0));
      s3[i] = dot16(xc, ca, dot16(xb, cb, dot16(xa, cc, 0)));
    }
    // sums over the row's P16 lanes (integers: any order); 16 lanes: DPP
    // row rotations (VALU), else cross-lane permutes
    if constexpr (P16 == 16) {
#pragma unroll
      for (int i = 0; i < kCandMax; ++i) {
        s1[i] = row16_isum(s1[i]);
        s2[i] = row16_isum(s2[i]);
        s3[i] = row16_isum(s3[i]);
      }
    } else {
#pragma unroll
      for (int m = 1; m < P16; m <<= 1)
#pragma unroll
        for (int i = 0; i < kCandMax; ++i) {
          s1[i] += __shfl_xor(s1[i], m);
          s2[i] += __shfl_xor(s2[i], m);
          s3[i] += __shfl_xor(s3[i], m);
        }
    }
    // the three-limb pass's bounds: T = S1 2^7 + S2, V = T + S3 2^-7 and L =
    // cq - F1 V in f32 rounded toward -inf (lower bounds), F1 = 2^(ex + ec - 20)
    __builtin_amdgcn_s_setreg(0x801, 2);
    const float F1 = mt.x == INT_MIN ? 0.0f : __builtin_ldexpf(1.0f, mt.x + P.ec - 20);
    float L1 = __builtin_inff(), L2 = __builtin_inff();
    int I1 = -1;
    bool bad = false;
    float cqMax = 0.0f;   // the f32 bounds' rounding slack (carried bounds)
    float LA = __builtin_inff();   // the anchor's bound (slot 0, state-3 re-checks)
#pragma unroll
    for (int i = 0; i < kCandMax; ++i) {
      const int c = ci[i];
      bad = bad || c >= P.k;   // a padding center
      if (c < 0 || c >= P.k) continue;
      const int T = s1[i] * 128 + s2[i];
      const float V = __builtin_fmaf((float)s3[i], 0x1p-7f, (float)T);
      const float L = __builtin_fmaf(-F1, V, cqv[i]);
      if (i == 0) LA = L;
      cqMax = __builtin_fmaxf(cqMax, __builtin_fabsf(cqv[i]));
      const bool lt = L < L1;
      L2 = __builtin_amdgcn_fmed3f(L1, L2, L);
      I1 = lt ? c : I1;
      L1 = lt ? L : L1;
    }
    __builtin_amdgcn_s_setreg(0x801, 0);
    bool decided = false;
    const double l1 = (double)L1, l2 = (double)L2;
    if (live && P.ok && !bad && mt.x != INT_MIN && I1 >= 0 && __builtin_isfinite(l1)) {
      const double xn = xnr, cn = cnorm[I1];
      const double gw = g[I1];
      const double xx = xn * xn, cc = cn * cn;
      const double n1 = (double)__int_as_float(mt.y);   // bounds |xh3|_1
      const double fx = err_term(mt.x, n1, P.mu, d);
      const double M = (4.0 * (fx + gw) + 2.0 * kEpsF * (xx + cc) +
                        0x1p-20 * (__builtin_fabs(l1) + cc + 2.0 * gw) +
                        0x1p-24 * (2.0 * (xx + cc) + __builtin_fabs(l1) +
                                   __builtin_fmin(__builtin_fabs(l2), 0x1p120)) +
                        0x1p-90) *
                       (1.0 + 0x1p-30);
      decided = !__builtin_isfinite(l2) || (l2 - l1) > M;
      if (bnd && (decided || RC)) {
        // carried bounds: the other candidates' bounds are >= l2 (f32,
        // rounded down after a rounded-down V: slack 2^-20 max |cq|), the
        // centers outside the set below the earlier tiers' bound (RC: the
        // set's carried bound)
        float lnc0 = RC ? lncR : bndR.y;
        const bool mark = RC || bndR.x == -2.0f;
        const double ub2 = bnd_ub_sq(xx, cc, l1, fx, gw, 0.0) + 0x1p-20 * (double)cqMax;
        if (nbrMode) {
          // every center outside the neighbourhood: |x - c| >= |c - c_a| -
          // |x - c_a| >= nbrR[a] - (the anchor's fresh upper bound)
          const double ua2 = __builtin_isfinite(LA)
                                 ? bnd_ub_sq(xx, cnA * cnA, (double)LA, fx, gA, 0.0) +
                                       0x1p-20 * (double)cqMax
                                 : __builtin_inf();
          const double Ln = ((double)RA - __builtin_sqrt(ua2) * (1.0 + 0x1p-50)) * (1.0 - 0x1p-50);
          lnc0 = Ln > 0.0 ? fdown(Ln) : -1.0f;
        }
        if (RC && decided) {
          // every center outside the set: |x - c| >= lnc0, above the winner
          // by the reference's slack (the filter's test)
          const double L = (double)lnc0, tau = 0x1p-29 * (xx + dp->cmax2) + 0x1p-48 * (L * L + ub2);
          decided = lnc0 >= 0.0f && !dp->bad && L * L - ub2 > tau;
        }
        if (decided && mark && lnc0 >= 0.0f && li == 0) {
          const float ub = bnd_dist_up(ub2);
          // (l2 = +inf: a set of one, nothing but the outside bound)
          const float lb = __builtin_isfinite(l2)
                               ? bnd_dist_dn(bnd_lb_sq(xx, l2, fx, 0.0, 0x1p-20 * (double)cqMax))
                               : __builtin_inff();
          bnd[row] = ub < 0x1p120f ? make_float2(ub, __builtin_fminf(lb, lnc0))
                                   : make_float2(-1.0f, -1.0f);
          if ((!RC || nbrMode) && sets && ub < 0x1p120f) {
            // the set and its outside bound, for the next iterations' re-checks
            lncA[row] = lnc0;
#pragma unroll
            for (int i = 0; i < kCandMax; ++i) sets[(size_t)row * kCandMax + i] = ci[i];
          }
        }
      }
    }
    if (RC) decided = decided && bnd != nullptr;
    if (live && li == 0) {
      if (RC) {
        if (decided) assign[row] = I1;
        state[row] = decided ? 0 : 1;
      } else if (decided) {
        assign[row] = I1;
      } else {
        const unsigned o = atomicAdd(outCount, 1u);
        outRows[o] = (int32_t)row;
#pragma unroll
        for (int i = 0; i < kCandMax; ++i) outCands[(size_t)o * kCandMax + i] = ci[i];
      }
    }
  }
}

// The re-check of the carried candidate sets and neighbourhoods (the rows of
// bounds_filter's list; k_screen_cands3<.., RC>'s arithmetic, bit for bit)
// in two phases per batch of kRcBatch listed rows.  Phase A, 2S lanes a row
// as in k_screen_cands3: the limb products of the row's <= kCandMax
// candidates, their f32 lower bounds L, and the row's best two, its
// anchor's bound and its flags into LDS.  Phase B, one row a lane: the fp64
// certification, the outside-bound test, the bounds and the state.  In
// k_screen_cands3 every lane of a row ran that fp64 tail (~170 f64 of ~700
// VALU instructions a 4-row step): the kernel was VALU-issue bound (neither
// five waves per SIMD nor rows grouped by center changed its time).
constexpr int kRcBatch = 256;
template <int S>
__global__ __launch_bounds__(kRcBatch) void k_recheck(
    const uint4* __restrict__ Xq, const int2* __restrict__ meta, const double* __restrict__ xnorm,
    int d, const uint4* __restrict__ Cr, const float* __restrict__ cq,
    const double* __restrict__ g, const double* __restrict__ cnorm,
    const CenterParams* __restrict__ prm, const int32_t* __restrict__ candRows,
    const unsigned int* __restrict__ candCount, int32_t* __restrict__ assign,
    float2* __restrict__ bnd, float* __restrict__ lncA, int32_t* __restrict__ sets,
    unsigned char* __restrict__ state, const DriftParams* __restrict__ dp,
    const int32_t* __restrict__ nbr, const float* __restrict__ nbrR,
    int32_t* __restrict__ failList, unsigned int* __restrict__ failCount,
    unsigned long long* __restrict__ failCum) {
  constexpr int P16 = 2 * S;        // 16-byte pieces of a limb plane
  constexpr int LPR = 8;            // lanes per row, PPL pieces each
  __shared__ unsigned sFail, sFailBase;
  constexpr int PPL = P16 / LPR;
  constexpr int RPW = 64 / LPR;     // rows per wave and step; LPR steps fill a wave's 64 slots
  static_assert(P16 % LPR == 0, "whole pieces per lane");
  __shared__ int sRow[kRcBatch], sI1[kRcBatch], sA0[kRcBatch], sMx[kRcBatch], sMy[kRcBatch],
      sFl[kRcBatch];
  __shared__ float sL1[kRcBatch], sL2[kRcBatch], sLA[kRcBatch], sCq[kRcBatch];
  const unsigned cnt = *candCount;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, q = lane / LPR, li = lane % LPR;
  const CenterParams P = *prm;
  const auto cR = __builtin_amdgcn_make_buffer_rsrc(
      (void*)Cr, (short)0, (int)std::min<int64_t>((int64_t)P.k * 3 * P16 * 16, 0x7fffffff),
      0x00020000);
  for (unsigned bb = blockIdx.x * kRcBatch; bb < cnt; bb += gridDim.x * kRcBatch) {
    if (t == 0) sFail = 0u;   // (ordered by the barrier after phase A)
    // ---- phase A
    for (int gi = 0; gi < LPR; ++gi) {
      const int slot = wave * 64 + gi * RPW + q;
      const unsigned idx = bb + slot;
      const bool live = idx < cnt;
      // (a slot past the list reads the batch's first entry, then drops it:
      // every load below is unconditional)
      const int32_t rw = candRows[live ? idx : bb];
      const bool nbrMode = rw < 0;   // ~row: the neighbourhood of its center
      const int64_t row = nbrMode ? ~(int64_t)rw : (int64_t)rw;
      const int32_t* setp = nbrMode ? nbr + (size_t)assign[row] * kCandMax
                                    : sets + (size_t)row * kCandMax;
      int ci[kCandMax];
      static_assert(kCandMax % 2 == 0, "sets read as int2");
#pragma unroll
      for (int i = 0; i < kCandMax; i += 2) {
        const int2 v = *reinterpret_cast<const int2*>(setp + i);   // 8-byte aligned rows
        ci[i] = live ? v.x : -1;
        ci[i + 1] = live ? v.y : -1;
      }
      const uint4* xr = Xq + row * (3 * P16) + li;
      uint4 xa[PPL], xb[PPL], xc[PPL];
#pragma unroll
      for (int j = 0; j < PPL; ++j) {
        xa[j] = xr[j * LPR];
        xb[j] = xr[P16 + j * LPR];
        xc[j] = xr[2 * P16 + j * LPR];
      }
      const int2 mt0 = meta[row];
      const int2 mt = live ? mt0 : make_int2(INT_MIN, 0);
      float cqv[kCandMax];
#pragma unroll
      for (int i = 0; i < kCandMax; ++i) cqv[i] = cq[(unsigned)ci[i] < (unsigned)P.k ? ci[i] : 0];
      // T = 2^7 S1 + S2 summed per lane (integers: exact in any order; the
      // row's total is k_screen_cands3's T), and S3
      int tt[kCandMax], s3[kCandMax];
#pragma unroll
      for (int i = 0; i < kCandMax; ++i) {
        const int c = ci[i];
        // an empty slot reads zeros without a memory access (out of range)
        const unsigned off =
            (unsigned)c < (unsigned)P.k ? (unsigned)(c * 3 * P16 + li) * 16u : 0x80000000u;
        int ti = 0, si = 0;
#pragma unroll
        for (int j = 0; j < PPL; ++j) {
          const unsigned o = off + 16u * LPR * j;
          const uint4 ca = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(cR, (int)o, 0, 0));
          const uint4 cb = __builtin_bit_cast(
              uint4, __builtin_amdgcn_raw_buffer_load_b128(cR, (int)(o + 16u * P16), 0, 0));
          const uint4 cc = __builtin_bit_cast(
              uint4, __builtin_amdgcn_raw_buffer_load_b128(cR, (int)(o + 32u * P16), 0, 0));
          ti = dot16(xb[j], ca, dot16(xa[j], cb, ti + dot16(xa[j], ca, 0) * 128));
          si = dot16(xc[j], ca, dot16(xb[j], cb, dot16(xa[j], cc, si)));
        }
        tt[i] = ti;
        s3[i] = si;
      }
      // sums over the row's 8 lanes by DPP: quad_perm [1,0,3,2], [2,3,0,1],
      // then row_half_mirror (lane i of a half with lane 7 - i: the other quad)
#pragma unroll
      for (int i = 0; i < kCandMax; ++i) {
        tt[i] += __builtin_amdgcn_update_dpp(0, tt[i], 0xB1, 0xF, 0xF, false);
        s3[i] += __builtin_amdgcn_update_dpp(0, s3[i], 0xB1, 0xF, 0xF, false);
        tt[i] += __builtin_amdgcn_update_dpp(0, tt[i], 0x4E, 0xF, 0xF, false);
        s3[i] += __builtin_amdgcn_update_dpp(0, s3[i], 0x4E, 0xF, 0xF, false);
        tt[i] += __builtin_amdgcn_update_dpp(0, tt[i], 0x141, 0xF, 0xF, false);
        s3[i] += __builtin_amdgcn_update_dpp(0, s3[i], 0x141, 0xF, 0xF, false);
      }
      // the three-limb bounds L = cq - F1 (T + S3 2^-7), rounded toward -inf.
      // The empty asm statements pin every rounding operation between the
      // two mode switches (the compiler does not order FP arithmetic against
      // s_setreg: without them it scheduled five candidates' conversions and
      // FMAs after the switch back)
      __builtin_amdgcn_s_setreg(0x801, 2);
#pragma unroll
      for (int i = 0; i < kCandMax; ++i) asm volatile("" : "+v"(tt[i]), "+v"(s3[i]));
      const float F1 = mt.x == INT_MIN ? 0.0f : __builtin_ldexpf(1.0f, mt.x + P.ec - 20);
      float L1 = __builtin_inff(), L2 = __builtin_inff(), LA = __builtin_inff(), cqMax = 0.0f;
      int I1 = -1;
      bool bad = false;
      // (branch-free: an empty slot's L = +inf changes none of L1, L2, I1)
#pragma unroll
      for (int i = 0; i < kCandMax; ++i) {
        const int c = ci[i];
        const bool ok = c >= 0 && c < P.k;
        bad = bad || c >= P.k;   // a padding center
        const float V = __builtin_fmaf((float)s3[i], 0x1p-7f, (float)tt[i]);
        const float L = ok ? __builtin_fmaf(-F1, V, cqv[i]) : __builtin_inff();
        if (i == 0) LA = L;
        cqMax = ok ? __builtin_fmaxf(cqMax, __builtin_fabsf(cqv[i])) : cqMax;
        const bool lt = L < L1;
        L2 = __builtin_amdgcn_fmed3f(L1, L2, L);
        I1 = lt ? c : I1;
        L1 = lt ? L : L1;
      }
      asm volatile("" : "+v"(L1), "+v"(L2), "+v"(LA), "+v"(cqMax), "+v"(I1));
      __builtin_amdgcn_s_setreg(0x801, 0);
      if (li == 0) {
        sRow[slot] = live ? (int)row : -1;
        sI1[slot] = I1;
        sA0[slot] = ci[0];
        sMx[slot] = mt.x;
        sMy[slot] = mt.y;
        sFl[slot] = (bad ? 1 : 0) | (nbrMode ? 2 : 0);
        sL1[slot] = L1;
        sL2[slot] = L2;
        sLA[slot] = LA;
        sCq[slot] = cqMax;
      }
    }
    __syncthreads();
    // ---- phase B: row sRow[t]
    const int row = sRow[t];
    unsigned rank = ~0u;   // this row's place among the batch's failures
    if (row >= 0) {
      const int I1 = sI1[t], mx = sMx[t], fl = sFl[t];
      const bool bad = fl & 1, nbrMode = fl & 2;
      const double l1 = (double)sL1[t], l2 = (double)sL2[t];
      const float cqMax = sCq[t];
      bool decided = false;
      if (P.ok && !bad && mx != INT_MIN && I1 >= 0 && __builtin_isfinite(l1)) {
        const double xn = xnorm[row], cn = cnorm[I1];
        const double gw = g[I1];
        const double xx = xn * xn, cc = cn * cn;
        const double n1 = (double)__int_as_float(sMy[t]);   // bounds |xh3|_1
        const double fx = err_term(mx, n1, P.mu, d);
        const double M = (4.0 * (fx + gw) + 2.0 * kEpsF * (xx + cc) +
                          0x1p-20 * (__builtin_fabs(l1) + cc + 2.0 * gw) +
                          0x1p-24 * (2.0 * (xx + cc) + __builtin_fabs(l1) +
                                     __builtin_fmin(__builtin_fabs(l2), 0x1p120)) +
                          0x1p-90) *
                         (1.0 + 0x1p-30);
        decided = !__builtin_isfinite(l2) || (l2 - l1) > M;
        // every center outside the set at least lnc0 away (the carried bound,
        // or the neighbourhood's), the other members at least l2
        float lnc0 = lncA[row];
        const double ub2 = bnd_ub_sq(xx, cc, l1, fx, gw, 0.0) + 0x1p-20 * (double)cqMax;
        const int a0 = (sA0[t] >= 0 && sA0[t] < P.k) ? sA0[t] : 0;
        if (nbrMode) {
          // |x - c| >= |c - c_a| - |x - c_a| >= nbrR[a] - (the anchor's fresh upper bound)
          const float LA = sLA[t];
          const double cnA = cnorm[a0];
          const double ua2 = __builtin_isfinite(LA)
                                 ? bnd_ub_sq(xx, cnA * cnA, (double)LA, fx, g[a0], 0.0) +
                                       0x1p-20 * (double)cqMax
                                 : __builtin_inf();
          const double Ln =
              ((double)nbrR[a0] - __builtin_sqrt(ua2) * (1.0 + 0x1p-50)) * (1.0 - 0x1p-50);
          lnc0 = Ln > 0.0 ? fdown(Ln) : -1.0f;
        }
        if (decided) {
          // above the winner by the reference's slack (the filter's test)
          const double L = (double)lnc0, tau = 0x1p-29 * (xx + dp->cmax2) + 0x1p-48 * (L * L + ub2);
          decided = lnc0 >= 0.0f && !dp->bad && L * L - ub2 > tau;
        }
        if (decided) {
          const float ub = bnd_dist_up(ub2);
          // (l2 = +inf: a set of one, nothing but the outside bound)
          const float lb = __builtin_isfinite(l2)
                               ? bnd_dist_dn(bnd_lb_sq(xx, l2, fx, 0.0, 0x1p-20 * (double)cqMax))
                               : __builtin_inff();
          bnd[row] = ub < 0x1p120f ? make_float2(ub, __builtin_fminf(lb, lnc0))
                                   : make_float2(-1.0f, -1.0f);
          if (nbrMode && ub < 0x1p120f) {
            // the neighbourhood (slot 0: a itself) becomes the row's carried set
            lncA[row] = lnc0;
#pragma unroll
            for (int i = 0; i < kCandMax; ++i)
              sets[(size_t)row * kCandMax + i] = nbr[(size_t)a0 * kCandMax + i];
          }
        }
      }
      if (decided) assign[row] = I1;
      state[row] = decided ? 0 : 1;
      if (failList && !decided) rank = atomicAdd(&sFail, 1u);
    }
    if (failList) {
      // the failures behind the filter's state-1 rows in the screen's list:
      // one reservation per workgroup and batch
      __syncthreads();
      if (t == 0 && sFail) {
        sFailBase = atomicAdd(failCount, sFail);
        atomicAdd(failCum, (unsigned long long)sFail);
      }
      __syncthreads();
      if (rank != ~0u) failList[sFailBase + rank] = row;
    }
    __syncthreads();   // the records are rewritten by the next batch
  }
}

// the candidate kernels' grid over at most n listed rows
unsigned cands_grid(int64_t n) {
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 127) / 128, 4096));
}
// the center-major copy behind the fragment image (k_centers_pack32)
template <int S>
const uint4* center_rows(const ScreenCall& sc) {
  return (const uint4*)sc.Cb + (size_t)(sc.ktp / 2) * S * 3 * 64;
}

template <int S>
int cands3(const ScreenCall& sc, const CandArgs& ca, const AppendTarget& out, unsigned int scap,
           const Bounds* bd) {
  KernelTimer timer("k_kmeans_cands3", sc.st);
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_screen_cands3<S, 16>), dim3(cands_grid(sc.n)), dim3(256), 0,
                     sc.st, (const uint4*)sc.img, sc.meta, sc.xnorm, sc.d, center_rows<S>(sc),
                     sc.cq, sc.g, sc.cnorm, sc.prm, (const int32_t*)ca.candRows,
                     (const int32_t*)ca.cands, (const unsigned int*)ca.candCount, sc.assign,
                     out.rows, out.cands, out.count, scap, bd ? bd->ub_lb : nullptr,
                     bd ? bd->lnc : nullptr, bd ? bd->sets : nullptr, nullptr, nullptr, nullptr,
                     nullptr);
  CYC_LAUNCH_CHECK("k_screen_cands3");
  return CYC_OK;
}

template <int S>
int recheck(const ScreenCall& sc, const Bounds& bd) {
  KernelTimer timer("k_kmeans_recheck", sc.st);
  if (!recheck_two_phase()) {
    // CYC_KMEANS_RECHECK=1: the one-phase form (k_screen_cands3<.., true>)
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_screen_cands3<S, 16, true>), dim3(cands_grid(sc.n)),
                       dim3(256), 0, sc.st, (const uint4*)sc.img, sc.meta, sc.xnorm, sc.d,
                       center_rows<S>(sc), sc.cq, sc.g, sc.cnorm, sc.prm, bd.rcRows,
                       (const int32_t*)bd.sets, bd.rcCount, sc.assign, nullptr, nullptr, nullptr,
                       0u, bd.ub_lb, bd.lnc, bd.sets, bd.state, bd.dp, bd.nbr, bd.nbrR);
    CYC_LAUNCH_CHECK("k_screen_cands3 (re-check)");
    return CYC_OK;
  }
  const unsigned grid =
      (unsigned)std::max<int64_t>(1, std::min<int64_t>((sc.n + kRcBatch - 1) / kRcBatch, 2048));
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_recheck<S>), dim3(grid), dim3(kRcBatch), 0, sc.st,
                     (const uint4*)sc.img, sc.meta, sc.xnorm, sc.d, center_rows<S>(sc), sc.cq,
                     sc.g, sc.cnorm, sc.prm, bd.rcRows, bd.rcCount, sc.assign, bd.ub_lb, bd.lnc,
                     bd.sets, bd.state, bd.dp, bd.nbr, bd.nbrR, bd.collected ? bd.list : nullptr,
                     bd.collected ? bd.listCount : nullptr, bd.collected ? bd.cum : nullptr);
  CYC_LAUNCH_CHECK("k_recheck");
  return CYC_OK;
}

}  // namespace

// S = 2 ksteps(d) 32-dim substeps: 4 (d <= 128) or 8
int launch_cands3(const ScreenCall& sc, const CandArgs& ca, const AppendTarget& out,
                  unsigned int scap, const Bounds* bd) {
  return ksteps(sc.d) == 2 ? cands3<4>(sc, ca, out, scap, bd) : cands3<8>(sc, ca, out, scap, bd);
}

int launch_recheck(const ScreenCall& sc, const Bounds& bd) {
  return ksteps(sc.d) == 2 ? recheck<4>(sc, bd) : recheck<8>(sc, bd);
}

int launch_cands(const CandArgs& ca, int64_t n, int d, int32_t* assign, const AppendTarget& out,
                 hipStream_t st, unsigned int scap) {
  KernelTimer timer("k_kmeans_cands", st);
  hipLaunchKernelGGL(k_screen_cands, dim3(cands_grid(n)), dim3(256), 0, st, ca.X, ca.xnorm, d,
                     ca.C, ca.cnorm, ca.k, ca.unit, ca.margin, (const int32_t*)ca.candRows,
                     (const int32_t*)ca.cands, (const unsigned int*)ca.candCount, assign, out.rows,
                     out.count, scap);
  CYC_LAUNCH_CHECK("k_screen_cands");
  return CYC_OK;
}

}  // namespace km8
}  // namespace cyc
