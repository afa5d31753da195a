// logistic_binary.hip -- the binary block aggregators on gfx950 (MI355X):
// logistic, hinge, least squares, Huber and AFT share the kernels below and
// differ in the per-row epilogue (binary_rows.hpp, chosen by the plan's kind).
//
// Binary: ml/optim/aggregator/BinaryLogisticBlockAggregator.scala:81-145 (and
//         the Hinge / LeastSquares / Huber / AFT block aggregators beside it)
//
// The device holds all blocks of a shard as one matrix (InstanceBlock rows
// concatenated: dense row-major n x F, CSR, or the tiles layout of tiles.hip);
// one call is the whole treeAggregate seqOp over the shard.  Deterministic
// except the plain-CSR gradient (atomics).
//
// Kernels
//   k_binlog_dense<FPL>    HBM-bound: one wave per row stream, each lane holds
//                          FPL coefficients and FPL gradient accumulators in
//                          registers; margin by a fixed-shape wave reduction,
//                          loss/multiplier epilogue, grad += mult * x.  One pass
//                          over X.  Per-wave partials folded in wave order.
//   k_binlog_csr           one wave per row: coef gathered by column index,
//                          gradient scattered with hardware fp64 atomics
//                          (global_atomic_add_f64).  One pass over the CSR.
//   k_binlog_csr_mult8     with a CSC copy, pass 1: the rows' multipliers
//   k_binlog_csc_grad_blk  pass 2: column sums over one row block of the CSC
//   k_binlog_offset_part, k_binlog_offset   the margin offset, left in HBM
//   k_effective_coef       least squares' effectiveCoef
//   k_binlog_fold          partial gradients, corrections and scalars into the
//                          aggregator state
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <mutex>

#include "binary_rows.hpp"
#include "logistic_plan.hpp"
#include "tiles.hpp"

namespace {

using cyc::bin_row;
using cyc::check_common;
using cyc::LossKind;
using cyc::row_margin;
using cyc::wave_sum_bcast;

template <int FPL>
__global__ __launch_bounds__(256) void k_binlog_dense(
    const double* __restrict__ X, const double* __restrict__ labels,
    const double* __restrict__ weights, int64_t n, int F, const double* __restrict__ coef,
    int fitIntercept, int kind, double offset, double lscale, double sigma, double eps, int64_t rowsPerWave, double* __restrict__ slabG,
    double* __restrict__ slabS) {
  const int lane = threadIdx.x & 63;
  const int64_t gw = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t r0 = gw * rowsPerWave;
  const int64_t r1 = min<int64_t>(n, r0 + rowsPerWave);
  double cf[FPL], g[FPL];
#pragma unroll
  for (int j = 0; j < FPL; ++j) {
    const int f = lane + 64 * j;
    cf[j] = f < F ? coef[f] : 0.0;
    g[j] = 0.0;
  }
  double loss = 0.0, wsum = 0.0, msum = 0.0, sgs = 0.0;
  for (int64_t r = r0; r < r1; ++r) {
    const double* xr = X + r * F;
    double x[FPL];
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < FPL; ++j) {
      const int f = lane + 64 * j;
      x[j] = f < F ? xr[f] : 0.0;
      s += x[j] * cf[j];
    }
    const double dot = wave_sum_bcast(s);
    const double margin = row_margin(kind, fitIntercept, offset, lscale, labels[r], dot);
    const double w = weights ? weights[r] : 1.0;
    const double mult = bin_row(kind, margin, w, labels[r], loss, wsum, sgs, sigma, eps);
    msum += mult;
    if (mult != 0.0) {
#pragma unroll
      for (int j = 0; j < FPL; ++j) g[j] += mult * x[j];
    }
  }
#pragma unroll
  for (int j = 0; j < FPL; ++j) {
    const int f = lane + 64 * j;
    if (f < F) slabG[gw * F + f] = g[j];
  }
  if (lane == 0) {
    slabS[gw * 4 + 0] = loss;
    slabS[gw * 4 + 1] = wsum;
    slabS[gw * 4 + 2] = msum;
    slabS[gw * 4 + 3] = sgs;
  }
}

__global__ __launch_bounds__(256) void k_binlog_csr(
    const int64_t* __restrict__ rowptr, const int32_t* __restrict__ colidx,
    const double* __restrict__ vals, const double* __restrict__ labels,
    const double* __restrict__ weights, int64_t n, const double* __restrict__ coef,
    int fitIntercept, int kind, double offset, double lscale, double sigma, double eps, int64_t rowsPerWave, double* __restrict__ gradAcc,
    double* __restrict__ slabS) {
  const int lane = threadIdx.x & 63;
  const int64_t gw = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t r0 = gw * rowsPerWave;
  const int64_t r1 = min<int64_t>(n, r0 + rowsPerWave);
  double loss = 0.0, wsum = 0.0, msum = 0.0, sgs = 0.0;
  for (int64_t r = r0; r < r1; ++r) {
    const int64_t p0 = rowptr[r], p1 = rowptr[r + 1];
    // first 64 nonzeros stay in registers for the scatter
    const int64_t q = p0 + lane;
    double v0 = 0.0;
    int c0 = 0;
    if (q < p1) {
      v0 = vals[q];
      c0 = colidx[q];
    }
    double s = (q < p1) ? v0 * coef[c0] : 0.0;
    for (int64_t p = q + 64; p < p1; p += 64) s += vals[p] * coef[colidx[p]];
    const double dot = wave_sum_bcast(s);
    const double margin = row_margin(kind, fitIntercept, offset, lscale, labels[r], dot);
    const double w = weights ? weights[r] : 1.0;
    const double mult = bin_row(kind, margin, w, labels[r], loss, wsum, sgs, sigma, eps);
    msum += mult;
    if (mult != 0.0) {
      if (q < p1) unsafeAtomicAdd(&gradAcc[c0], v0 * mult);
      for (int64_t p = q + 64; p < p1; p += 64) unsafeAtomicAdd(&gradAcc[colidx[p]], vals[p] * mult);
    }
  }
  if (lane == 0) {
    slabS[gw * 4 + 0] = loss;
    slabS[gw * 4 + 1] = wsum;
    slabS[gw * 4 + 2] = msum;
    slabS[gw * 4 + 3] = sgs;
  }
}

// Pass 1, grouped: a wave takes 64 consecutive rows at a time, 8 lanes per
// row (8 rows per round, each row's nonzeros strided over its 8 lanes and
// summed by a 3-step butterfly), then hands row i's partial dot to lane i so
// the per-row epilogue (log1p/exp, BinaryLogisticBlockAggregator.scala:
// 104-122) runs once per row instead of once per lane; dots[r] receives the
// multiplier, written coalesced.
constexpr int CSR_IT = 2;   // nonzeros per lane per chunk (16 loads in flight)
constexpr int RP = 8;       // rows per pass
__global__ __launch_bounds__(256) void k_binlog_csr_mult8(
    const int64_t* __restrict__ rowptr, const int32_t* __restrict__ colidx,
    const double* __restrict__ vals, const double* __restrict__ labels,
    const double* __restrict__ weights, int64_t n, const double* __restrict__ coef,
    int fitIntercept, int kind, double offset, double lscale, double sigma, double eps,
    double* __restrict__ dots, double* __restrict__ slabS) {
  const int lane = threadIdx.x & 63, sub = lane & 7, grp = lane >> 3;
  const int64_t gw = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t nw = (int64_t)gridDim.x * 4;
  double loss = 0.0, wsum = 0.0, msum = 0.0, sgs = 0.0;
  for (int64_t g0 = gw * 64; g0 < n; g0 += nw * 64) {
    // row bounds of the 64 rows by one coalesced load, then shuffles
    const int64_t myr = g0 + lane < n ? g0 + lane : n;
    const int64_t rp0 = rowptr[myr];
    const int64_t rp1 = rowptr[myr + 1 < n ? myr + 1 : n];
    // the 8 rounds advance together in 16-nonzero chunks (8 lanes x 2 per
    // row): each chunk issues all 16 index/value loads, then the 16 gathers,
    // then the products, so every chunk has 16 loads in flight per lane and
    // the dependent index->coefficient latency is paid once per chunk rather
    // than once per nonzero.  A lane's products still add in ascending
    // nonzero order (sub, sub+8, sub+16, ...), as the single-row loop did.
    // RP rows per pass (8 / RP passes per round group) bound the live state.
    int64_t maxlen = rp1 - rp0;
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
      const int64_t o = __shfl_xor(maxlen, m);
      maxlen = o > maxlen ? o : maxlen;
    }
    double mydot = 0.0;
#pragma unroll
    for (int h = 0; h < 8; h += RP) {
      int64_t beg[RP], end[RP];
      double sr[RP];
#pragma unroll
      for (int rr = 0; rr < RP; ++rr) {
        beg[rr] = __shfl(rp0, (h + rr) * 8 + grp);
        end[rr] = __shfl(rp1, (h + rr) * 8 + grp);
        sr[rr] = 0.0;
      }
      for (int64_t k = 0; k < maxlen; k += 8 * CSR_IT) {
        int ci[RP][CSR_IT];
        double vv[RP][CSR_IT], cf[RP][CSR_IT];
#pragma unroll
        for (int rr = 0; rr < RP; ++rr)
#pragma unroll
          for (int it = 0; it < CSR_IT; ++it) {
            const int64_t p = beg[rr] + k + sub + 8 * it;
            const bool ok = p < end[rr];
            ci[rr][it] = ok ? __builtin_nontemporal_load(colidx + p) : -1;
            vv[rr][it] = ok ? __builtin_nontemporal_load(vals + p) : 0.0;
          }
#pragma unroll
        for (int rr = 0; rr < RP; ++rr)
#pragma unroll
          for (int it = 0; it < CSR_IT; ++it) cf[rr][it] = ci[rr][it] >= 0 ? coef[ci[rr][it]] : 0.0;
#pragma unroll
        for (int rr = 0; rr < RP; ++rr)
#pragma unroll
          for (int it = 0; it < CSR_IT; ++it)
            if (ci[rr][it] >= 0) sr[rr] += vv[rr][it] * cf[rr][it];
      }
#pragma unroll
      for (int rr = 0; rr < RP; ++rr) {
        double s = sr[rr];
        s += __shfl_xor(s, 1);
        s += __shfl_xor(s, 2);
        s += __shfl_xor(s, 4);
        const double v = __shfl(s, 8 * (lane & 7));
        if ((lane >> 3) == h + rr) mydot = v;
      }
    }
    const int64_t row = g0 + lane;
    if (row < n) {
      const double margin = row_margin(kind, fitIntercept, offset, lscale, labels[row], mydot);
      const double w = weights ? weights[row] : 1.0;
      const double m = bin_row(kind, margin, w, labels[row], loss, wsum, sgs, sigma, eps);
      msum += m;
      dots[row] = m;
    }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    loss += __shfl_xor(loss, m);
    wsum += __shfl_xor(wsum, m);
    msum += __shfl_xor(msum, m);
    sgs += __shfl_xor(sgs, m);
  }
  if (lane == 0) {
    slabS[gw * 4 + 0] = loss;
    slabS[gw * 4 + 1] = wsum;
    slabS[gw * 4 + 2] = msum;
    slabS[gw * 4 + 3] = sgs;
  }
}

// Pass 2 over one row block of the row-blocked CSC (csc.hip): LPC lanes per
// column, products vals * mult[row] (the block's 2 MB multiplier slice stays
// in L2), fixed butterfly, gradAcc[c] = (first ? 0 : gradAcc[c]) + s.
// Deterministic: blocks in order, a block's rows in order within each lane.
constexpr int LPC = 32, IT = 1, CPG = 4;   // lanes per group of CPG columns
__global__ __launch_bounds__(256) void k_binlog_csc_grad_blk(
    const int64_t* __restrict__ colptrB, const int32_t* __restrict__ rowidx,
    const double* __restrict__ cvals, const double* __restrict__ mult, int F, int first,
    double* __restrict__ gradAcc) {
  // LPC lanes per group of CPG consecutive columns; the first LPC*IT
  // nonzeros of each column are loaded before any gather (all in flight)
  const int sub = threadIdx.x & (LPC - 1), lane = threadIdx.x & 63, gbase = lane & (64 - LPC);
  const int64_t c0 = (((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / LPC) * CPG;
  const int64_t ci = c0 + (sub < CPG + 1 ? sub : CPG);
  const int64_t cp = colptrB[ci < F ? ci : (int64_t)F];
  int64_t b[CPG + 1];
#pragma unroll
  for (int i = 0; i <= CPG; ++i) b[i] = __shfl(cp, gbase + i);
  int ri[CPG][IT];
  double vv[CPG][IT], mm[CPG][IT];
#pragma unroll
  for (int i = 0; i < CPG; ++i)
#pragma unroll
    for (int it = 0; it < IT; ++it) {
      const int64_t q = b[i] + sub + LPC * it;
      const bool ok = c0 + i < F && q < b[i + 1];
      ri[i][it] = ok ? __builtin_nontemporal_load(rowidx + q) : -1;
      vv[i][it] = ok ? __builtin_nontemporal_load(cvals + q) : 0.0;
    }
#pragma unroll
  for (int i = 0; i < CPG; ++i)
#pragma unroll
    for (int it = 0; it < IT; ++it) mm[i][it] = ri[i][it] >= 0 ? mult[ri[i][it]] : 0.0;
  double mine = 0.0;
#pragma unroll
  for (int i = 0; i < CPG; ++i) {
    double s = vv[i][0] * mm[i][0];
#pragma unroll
    for (int it = 1; it < IT; ++it) s += vv[i][it] * mm[i][it];
    if (c0 + i < F)
      for (int64_t q = b[i] + sub + LPC * IT; q < b[i + 1]; q += LPC)
        s += __builtin_nontemporal_load(cvals + q) * mult[__builtin_nontemporal_load(rowidx + q)];
#pragma unroll
    for (int m = LPC / 2; m >= 1; m >>= 1) s += __shfl_xor(s, m);
    if (sub == i) mine = s;
  }
  if (sub < CPG && c0 + sub < F) gradAcc[c0 + sub] = first ? mine : gradAcc[c0 + sub] + mine;
}

// grad[f] += sum_w slabG[w][f] (or += gradAcc[f]); then the fitWithMean
// correction (daxpy(-multiplierSum, scaledMean), :132-137) and the intercept
// (:139-142).  scal = {loss, wsum, msum, sigmaGradSum}.
__global__ void k_binlog_fold(const double* __restrict__ slabG, int64_t waves,
                              const double* __restrict__ gradAcc, int F,
                              const double* __restrict__ scal, int fitIntercept, int fitWithMean,
                              int sigmaIdx, const double* __restrict__ scaledMean,
                              double* __restrict__ grad, double* __restrict__ lossSum,
                              double* __restrict__ weightSum) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  const double msum = scal[2];
  if (f < F) {
    double s = 0.0;
    if (slabG) {
      for (int64_t w = 0; w < waves; ++w) s += slabG[w * F + f];
    } else {
      s = gradAcc[f];
    }
    double gf = grad[f] + s;
    if (fitWithMean) gf = gf + (-msum) * scaledMean[f];
    grad[f] = gf;
  }
  if (f == 0) {
    if (fitIntercept) grad[F] += msum;
    if (sigmaIdx >= 0) grad[sigmaIdx] += scal[3];   // Huber :138
    *lossSum += scal[0];
    *weightSum += scal[1];
  }
}

// marginOffset: coef[F] - ddot(coef, scaledMean) (Binary :67-72, Hinge
// :62-71), or for least squares (:57-62) labelMean / labelStd - ddot(...)
// (base passed in, useBase = 1).
// Two stages: kOffParts workgroups each sum a contiguous stretch of the
// products, then one thread adds the parts in order -- deterministic (the
// reference's sequential ddot order is not pinned below 1e-10 anyway).
constexpr int kOffParts = 256;                 // partial sums of the offset dot

// stage 1: part p sums the products of its contiguous range, lane-strided
// (coalesced), each thread in index order, then a fixed shuffle / wave tree
__global__ __launch_bounds__(256) void k_binlog_offset_part(const double* __restrict__ coef,
                                                            const double* __restrict__ sm, int F,
                                                            double* __restrict__ part) {
  __shared__ double sh[4];
  const int t = threadIdx.x;
  const int64_t per = ((int64_t)F + kOffParts - 1) / kOffParts;
  const int64_t f0 = blockIdx.x * per, f1 = std::min<int64_t>(F, f0 + per);
  double dd = 0.0;
  for (int64_t f = f0 + t; f < f1; f += 256) dd += coef[f] * sm[f];
  for (int m = 32; m >= 1; m >>= 1) dd += __shfl_xor(dd, m);
  if ((t & 63) == 0) sh[t >> 6] = dd;
  __syncthreads();
  if (t == 0) part[blockIdx.x] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// stage 2: the parts in order; out = (base or intercept) - dot
__global__ void k_binlog_offset(const double* __restrict__ part, const double* __restrict__ coef,
                                int F, int useBase, double base, double* __restrict__ out) {
  if (threadIdx.x != 0) return;
  double s = 0.0;
  for (int i = 0; i < kOffParts; ++i) s += part[i];
  out[0] = (useBase ? base : coef[F]) - s;
}

// LeastSquaresBlockAggregator.effectiveCoef (:48-55): coefficient or 0.0
// where the feature's inverseStd is 0.
__global__ void k_effective_coef(const double* __restrict__ coef,
                                 const double* __restrict__ inverseStd, int F,
                                 double* __restrict__ out) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f < F) out[f] = inverseStd[f] != 0 ? coef[f] : 0.0;
}

// ------------------------------------------------------------ the call core
// Every entry point is: argument checks, then under the plan mutex one
// binary_call (what all rows share), the layout's row kernels, binary_finish.

// The plan was made for aggregator `kind`.  Least squares names its plan in
// its first check; the others leave a null plan to check_common.
int check_kind(cyc_logistic_plan p, LossKind kind) {
  static const char* const what[] = {
      "the plan is not a binary logistic plan",
      "the plan is not a hinge plan (cyc_hinge_plan_create)",
      "the plan is not a least squares plan (cyc_least_squares_plan_create)",
      "the plan is not a Huber plan (cyc_huber_plan_create)",
      "the plan is not an AFT plan (cyc_aft_plan_create)"};
  CYC_REQUIRE(p != nullptr ? p->loss == kind : kind != cyc::kLeastSquares, what[kind]);
  return CYC_OK;
}

// least squares' own arguments (p is a least squares plan)
int check_least_squares(cyc_logistic_plan p, const double* coef, const double* inverseStd,
                        const double* scaledMean) {
  CYC_REQUIRE(coef != nullptr && inverseStd != nullptr, "coef and inverseStd must not be null");
  CYC_REQUIRE(!p->fitIntercept || scaledMean != nullptr,
              "scaled means is required when fitting an intercept");
  return CYC_OK;
}

// The checks of a dense or CSR entry point of `kind`, up to n >= 0.
int check_rows_call(cyc_logistic_plan p, LossKind kind, const double* coef,
                    const double* inverseStd, const double* scaledMean, int64_t n) {
  if (int rc = check_kind(p, kind)) return rc;
  if (kind == cyc::kLeastSquares) {
    if (int rc = check_least_squares(p, coef, inverseStd, scaledMean)) return rc;
    if (n < 0) {
      cyc::set_error("n >= 0");
      return CYC_ERR_INVALID_ARG;
    }
    return CYC_OK;
  }
  if (int rc = check_common(p, coef, scaledMean)) return rc;
  CYC_REQUIRE(n >= 0, "n >= 0");
  return CYC_OK;
}

// The margin offset every row starts from (see k_binlog_offset), left in
// HBM: *offDev points at it (nullptr without an intercept: offset 0).  The
// original coefficients go in (least squares: not the effective ones).
int binary_offset_dev(cyc_logistic_plan p, const double* coef, const double* scaledMean,
                      hipStream_t st, const double** offDev) {
  *offDev = nullptr;
  if (!p->fitIntercept) return CYC_OK;
  if (!p->fitWithMean && p->loss != cyc::kLeastSquares) {
    *offDev = coef + p->F;   // the intercept itself
    return CYC_OK;
  }
  if (int rc = p->offset.reserve(sizeof(double) * (2 + kOffParts))) return rc;
  double* part = (double*)p->offset.ptr + 2;
  hipLaunchKernelGGL(k_binlog_offset_part, dim3(kOffParts), dim3(256), 0, st, coef, scaledMean,
                     p->F, part);
  CYC_LAUNCH_CHECK("k_binlog_offset_part");
  hipLaunchKernelGGL(k_binlog_offset, dim3(1), dim3(64), 0, st, (const double*)part, coef, p->F,
                     p->loss == cyc::kLeastSquares ? 1 : 0, p->labelMean / p->labelStd,
                     (double*)p->offset.ptr);
  CYC_LAUNCH_CHECK("k_binlog_offset");
  *offDev = (const double*)p->offset.ptr;
  return CYC_OK;
}

// What the rows of one add share, resolved once under the plan mutex.
struct BinaryCall {
  hipStream_t st = nullptr;
  const double* kc = nullptr;       // the coefficients the margins use
  const double* offDev = nullptr;   // the margin offset in HBM (nullptr: 0)
  double offset = 0.0;              // the same on the host, when asked for
  double lscale = 0.0;              // least squares: -1 / labelStd on the label
  int foldIcpt = 0;                 // the fold adds multiplierSum to grad[F]
  int sigIdx = -1;                  // index of sigma in coef and grad, or -1
  double sigma = 0.0, eps = 0.0;    // Huber / AFT
};

// hostOffset: the dense and CSR kernels take the offset as a scalar (one
// copy and stream sync); the tiles path reads it from HBM with no sync.
int binary_call(cyc_logistic_plan p, const double* coef, const double* inverseStd,
                const double* scaledMean, void* stream, bool hostOffset, BinaryCall* c) {
  const int F = p->F;
  const hipStream_t st = c->st = cyc::as_stream(stream);
  int rc;
  if ((rc = p->scal.reserve(sizeof(double) * 4))) return rc;
  c->kc = coef;
  if (p->loss == cyc::kLeastSquares) {   // effectiveCoef (:48-55); the offset takes coef itself
    if ((rc = p->effCoef.reserve(sizeof(double) * (size_t)F))) return rc;
    hipLaunchKernelGGL(k_effective_coef, dim3((F + 255) / 256), dim3(256), 0, st, coef, inverseStd,
                       F, (double*)p->effCoef.ptr);
    CYC_LAUNCH_CHECK("k_effective_coef");
    c->kc = (const double*)p->effCoef.ptr;
  }
  if ((rc = binary_offset_dev(p, coef, scaledMean, st, &c->offDev))) return rc;
  if (hostOffset && c->offDev) {
    CYC_HIP(hipMemcpyAsync(&c->offset, c->offDev, sizeof(double), hipMemcpyDeviceToHost, st));
    CYC_HIP(hipStreamSynchronize(st));
  }
  c->lscale = -1.0 / p->labelStd;
  c->foldIcpt = p->loss == cyc::kLeastSquares ? 0 : p->fitIntercept;
  // Huber: sigma = coefficientsArray.last (:97), its gradient entry last
  // AFT: sigma = math.exp(coefficientsArray(dim - 1)) (:91), dim = F + 2
  c->sigIdx = p->loss == cyc::kHuber ? F + (p->fitIntercept ? 1 : 0)
              : p->loss == cyc::kAft ? F + 1 : -1;
  if (c->sigIdx >= 0) {
    CYC_HIP(hipMemcpyAsync(&c->sigma, coef + c->sigIdx, sizeof(double), hipMemcpyDeviceToHost,
                           st));
    CYC_HIP(hipStreamSynchronize(st));
    if (p->loss == cyc::kAft) c->sigma = std::exp(c->sigma);
  }
  c->eps = p->epsilon;
  return CYC_OK;
}

// The `partials` rows of slabS folded into the scalars, then k_binlog_fold
// from the slab (slabG, slabRows) or, with slabG null, from gradAcc.
int binary_finish(cyc_logistic_plan p, const BinaryCall& c, int64_t partials, const double* slabG,
                  int64_t slabRows, const double* scaledMean, double* grad, double* lossSum,
                  double* weightSum) {
  const int F = p->F;
  if (int rc = cyc::fold_scalars((const double*)p->slabS.ptr, partials, 4, (double*)p->scal.ptr,
                                 c.st))
    return rc;
  hipLaunchKernelGGL(k_binlog_fold, dim3((F + 255) / 256), dim3(256), 0, c.st, slabG, slabRows,
                     slabG ? nullptr : (const double*)p->gradAcc.ptr, F,
                     (const double*)p->scal.ptr, c.foldIcpt, p->fitWithMean, c.sigIdx, scaledMean,
                     grad, lossSum, weightSum);
  CYC_LAUNCH_CHECK("k_binlog_fold");
  return CYC_OK;
}

int binary_add_dense(cyc_logistic_plan p, LossKind kind, const double* X, const double* labels,
                     const double* weights, int64_t n, const double* coef,
                     const double* inverseStd, const double* scaledMean, double* grad,
                     double* lossSum, double* weightSum, void* stream) {
  int rc = check_rows_call(p, kind, coef, inverseStd, scaledMean, n);
  if (rc || n == 0) return rc;
  const int F = p->F;
  if (F > 64 * 32) {
    cyc::set_error("dense binary aggregator supports numFeatures <= 2048 (use CSR blocks)");
    return CYC_ERR_UNSUPPORTED;
  }
  std::lock_guard<std::mutex> g(p->mu);
  const int64_t waves = std::min<int64_t>(4096, n);
  const int64_t rpw = (n + waves - 1) / waves;
  const int64_t nw = (n + rpw - 1) / rpw;
  const int64_t blocks = (nw + 3) / 4;
  const int64_t wtot = blocks * 4;
  if ((rc = p->slabG.reserve(sizeof(double) * (size_t)wtot * F)) ||
      (rc = p->slabS.reserve(sizeof(double) * (size_t)wtot * 4)))
    return rc;
  BinaryCall c;
  if ((rc = binary_call(p, coef, inverseStd, scaledMean, stream, true, &c))) return rc;
  // FPL = features per lane, the power of two covering F
  const int fpl = (F + 63) / 64;
  const auto kern = fpl <= 1 ? k_binlog_dense<1> : fpl <= 2 ? k_binlog_dense<2>
                    : fpl <= 4 ? k_binlog_dense<4> : fpl <= 8 ? k_binlog_dense<8>
                    : fpl <= 16 ? k_binlog_dense<16> : k_binlog_dense<32>;
  {
    // waves past the last row still write (zero) partials, so the fold reads all
    cyc::KernelTimer timer("k_binlog_dense", c.st);
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(256), 0, c.st, X, labels, weights, n, F,
                       c.kc, p->fitIntercept, (int)p->loss, c.offset, c.lscale, c.sigma, c.eps,
                       rpw, (double*)p->slabG.ptr, (double*)p->slabS.ptr);
    CYC_LAUNCH_CHECK("k_binlog_dense");
  }
  return binary_finish(p, c, wtot, (const double*)p->slabG.ptr, wtot, scaledMean, grad, lossSum,
                       weightSum);
}

int binary_add_csr(cyc_logistic_plan p, LossKind kind, const int64_t* rowptr,
                   const int32_t* colidx, const double* vals, const double* labels,
                   const double* weights, int64_t n, const double* coef,
                   const double* inverseStd, const double* scaledMean, double* grad,
                   double* lossSum, double* weightSum, cyc_csc csc, void* stream) {
  int rc = check_rows_call(p, kind, coef, inverseStd, scaledMean, n);
  if (rc || n == 0) return rc;
  const int F = p->F;
  std::lock_guard<std::mutex> g(p->mu);
  const int64_t waves = csc ? std::min<int64_t>(8192, (n + 63) / 64) : std::min<int64_t>(16384, n);
  const int64_t rpw = (n + waves - 1) / waves;
  const int64_t nw = csc ? waves : (n + rpw - 1) / rpw;
  const int64_t blocks = (nw + 3) / 4;
  const int64_t wtot = blocks * 4;
  if ((rc = p->gradAcc.reserve(sizeof(double) * (size_t)F)) ||
      (rc = p->slabS.reserve(sizeof(double) * (size_t)wtot * 4)))
    return rc;
  BinaryCall c;
  if ((rc = binary_call(p, coef, inverseStd, scaledMean, stream, true, &c))) return rc;
  if (csc) {
    // Deterministic two-pass path: CSR margins -> mult, then the row-blocked
    // CSC's column sums, one row block at a time.  (The row-block x
    // column-tile layout, cyc_binary_add_tiles_dev, is the fast path for
    // large sparse shards.)
    CYC_REQUIRE(cyc_csc_rows(csc) == n && cyc_csc_features(csc) == F,
                "the CSC copy does not match the CSR rows (cyc_csc_build_dev of these rows)");
    const int64_t* colptr = nullptr;
    const int32_t* rowidx = nullptr;
    const double* cvals = nullptr;
    cyc_csc_arrays(csc, &colptr, &rowidx, &cvals);
    if ((rc = p->rowMult.reserve(sizeof(double) * (size_t)n))) return rc;
    {
      cyc::KernelTimer timer("k_binlog_csr", c.st);
      hipLaunchKernelGGL(k_binlog_csr_mult8, dim3((unsigned)blocks), dim3(256), 0, c.st, rowptr,
                         colidx, vals, labels, weights, n, c.kc, p->fitIntercept, (int)p->loss,
                         c.offset, c.lscale, c.sigma, c.eps, (double*)p->rowMult.ptr,
                         (double*)p->slabS.ptr);
      CYC_LAUNCH_CHECK("k_binlog_csr_mult8");
    }
    int64_t rpb = 0, nb = 0;
    cyc_csc_blocks(csc, &rpb, &nb);
    // 32 lanes per group of 4 columns (8 / 16 / 64 lanes and 2 / 8 columns
    // per group measured slower or flat)
    const unsigned cgrid = (unsigned)((((int64_t)F + 3) / 4 * 32 + 255) / 256);
    cyc::KernelTimer timer("k_binlog_csc_grad", c.st);
    for (int64_t b = 0; b < nb; ++b) {
      hipLaunchKernelGGL(k_binlog_csc_grad_blk, dim3(cgrid), dim3(256), 0, c.st,
                         colptr + b * F, rowidx, cvals, (const double*)p->rowMult.ptr, F,
                         b == 0 ? 1 : 0, (double*)p->gradAcc.ptr);
    }
    CYC_LAUNCH_CHECK("k_binlog_csc_grad_blk");
  } else {
    CYC_HIP(hipMemsetAsync(p->gradAcc.ptr, 0, sizeof(double) * (size_t)F, c.st));
    cyc::KernelTimer timer("k_binlog_csr", c.st);
    hipLaunchKernelGGL(k_binlog_csr, dim3((unsigned)blocks), dim3(256), 0, c.st, rowptr, colidx,
                       vals, labels, weights, n, c.kc, p->fitIntercept, (int)p->loss, c.offset,
                       c.lscale, c.sigma, c.eps, rpw, (double*)p->gradAcc.ptr,
                       (double*)p->slabS.ptr);
    CYC_LAUNCH_CHECK("k_binlog_csr");
  }
  return binary_finish(p, c, wtot, nullptr, 0, scaledMean, grad, lossSum, weightSum);
}

}  // namespace

extern "C" {

int cyc_binary_add_tiles_dev(cyc_logistic_plan p, cyc_tiles tiles, const double* labels,
                             const double* weights, const double* coef, const double* inverseStd,
                             const double* scaledMean, double* grad, double* lossSum,
                             double* weightSum, void* stream) {
  int rc = check_common(p, coef, scaledMean);
  if (rc) return rc;
  CYC_REQUIRE(tiles != nullptr, "tiles must not be null");
  cyc::TilesView v;
  if ((rc = cyc::tiles_view(tiles, &v))) return rc;
  const int F = p->F;
  CYC_REQUIRE(v.F == F, "Dimensions mismatch when adding new instance. Expecting " +
                            std::to_string(F) + " but got " + std::to_string(v.F) + ".");
  const int64_t n = v.n;
  if (n == 0) return CYC_OK;
  CYC_REQUIRE(labels != nullptr, "labels must not be null");
  if (p->loss == cyc::kLeastSquares &&
      (rc = check_least_squares(p, coef, inverseStd, scaledMean)))
    return rc;
  std::lock_guard<std::mutex> g(p->mu);
  const int R = cyc::tiles_ranges(v);
  const int64_t wgMax = cyc::tiles_rows_blocks(n);
  if ((rc = p->rowMult.reserve(sizeof(double) * (size_t)n)) ||
      (rc = p->slabG.reserve(sizeof(double) * (size_t)R * F)) ||
      (rc = p->slabS.reserve(sizeof(double) * (size_t)wgMax * 4)))
    return rc;
  // the margin offset stays in HBM for k_tiles_rows: no host round trip
  // (and no stream sync) before the margin pass
  BinaryCall c;
  if ((rc = binary_call(p, coef, inverseStd, scaledMean, stream, false, &c))) return rc;
  int64_t wgs = 0;
  {
    cyc::KernelTimer timer("k_tiles_margin", c.st);
    if ((rc = cyc::tiles_margin(v, c.kc, (double*)p->rowMult.ptr, c.st))) return rc;
  }
  {
    cyc::KernelTimer timer("k_tiles_rows", c.st);
    if ((rc = cyc::tiles_rows(n, labels, weights, p->fitIntercept, p->loss, 0.0, c.offDev,
                              c.lscale, c.sigma, c.eps, (double*)p->rowMult.ptr,
                              (double*)p->slabS.ptr, &wgs, c.st)))
      return rc;
  }
  int ranges = 0;
  {
    cyc::KernelTimer timer("k_tiles_grad", c.st);
    if ((rc = cyc::tiles_grad(v, (const double*)p->rowMult.ptr, (double*)p->slabG.ptr, &ranges,
                              c.st)))
      return rc;
  }
  return binary_finish(p, c, wgs, (const double*)p->slabG.ptr, ranges, scaledMean, grad, lossSum,
                       weightSum);
}


// The per-kind dense and CSR entry points: the core checks the plan's kind.

int cyc_binary_logistic_add_dense_dev(cyc_logistic_plan p, const double* X, const double* labels,
                                      const double* weights, int64_t n, const double* coef,
                                      const double* scaledMean, double* grad, double* lossSum,
                                      double* weightSum, void* stream) {
  return binary_add_dense(p, cyc::kLogistic, X, labels, weights, n, coef, nullptr, scaledMean,
                          grad, lossSum, weightSum, stream);
}

int cyc_binary_logistic_add_csr_dev(cyc_logistic_plan p, const int64_t* rowptr,
                                    const int32_t* colidx, const double* vals,
                                    const double* labels, const double* weights, int64_t n,
                                    const double* coef, const double* scaledMean, double* grad,
                                    double* lossSum, double* weightSum, cyc_csc csc,
                                    void* stream) {
  return binary_add_csr(p, cyc::kLogistic, rowptr, colidx, vals, labels, weights, n, coef, nullptr,
                        scaledMean, grad, lossSum, weightSum, csc, stream);
}

int cyc_hinge_add_dense_dev(cyc_logistic_plan p, const double* X, const double* labels,
                            const double* weights, int64_t n, const double* coef,
                            const double* scaledMean, double* grad, double* lossSum,
                            double* weightSum, void* stream) {
  return binary_add_dense(p, cyc::kHinge, X, labels, weights, n, coef, nullptr, scaledMean, grad,
                          lossSum, weightSum, stream);
}

int cyc_hinge_add_csr_dev(cyc_logistic_plan p, const int64_t* rowptr, const int32_t* colidx,
                          const double* vals, const double* labels, const double* weights,
                          int64_t n, const double* coef, const double* scaledMean, double* grad,
                          double* lossSum, double* weightSum, cyc_csc csc, void* stream) {
  return binary_add_csr(p, cyc::kHinge, rowptr, colidx, vals, labels, weights, n, coef, nullptr,
                        scaledMean, grad, lossSum, weightSum, csc, stream);
}

int cyc_huber_add_dense_dev(cyc_logistic_plan p, const double* X, const double* labels,
                            const double* weights, int64_t n, const double* coef,
                            const double* scaledMean, double* grad, double* lossSum,
                            double* weightSum, void* stream) {
  return binary_add_dense(p, cyc::kHuber, X, labels, weights, n, coef, nullptr, scaledMean, grad,
                          lossSum, weightSum, stream);
}

int cyc_huber_add_csr_dev(cyc_logistic_plan p, const int64_t* rowptr, const int32_t* colidx,
                          const double* vals, const double* labels, const double* weights,
                          int64_t n, const double* coef, const double* scaledMean, double* grad,
                          double* lossSum, double* weightSum, cyc_csc csc, void* stream) {
  return binary_add_csr(p, cyc::kHuber, rowptr, colidx, vals, labels, weights, n, coef, nullptr,
                        scaledMean, grad, lossSum, weightSum, csc, stream);
}

// AFT: the rows' weights are the censors (AFTBlockAggregator.scala:97)
int cyc_aft_add_dense_dev(cyc_logistic_plan p, const double* X, const double* labels,
                          const double* censors, int64_t n, const double* coef,
                          const double* scaledMean, double* grad, double* lossSum,
                          double* weightSum, void* stream) {
  return binary_add_dense(p, cyc::kAft, X, labels, censors, n, coef, nullptr, scaledMean, grad,
                          lossSum, weightSum, stream);
}

int cyc_aft_add_csr_dev(cyc_logistic_plan p, const int64_t* rowptr, const int32_t* colidx,
                        const double* vals, const double* labels, const double* censors,
                        int64_t n, const double* coef, const double* scaledMean, double* grad,
                        double* lossSum, double* weightSum, cyc_csc csc, void* stream) {
  return binary_add_csr(p, cyc::kAft, rowptr, colidx, vals, labels, censors, n, coef, nullptr,
                        scaledMean, grad, lossSum, weightSum, csc, stream);
}

int cyc_least_squares_add_dense_dev(cyc_logistic_plan p, const double* X, const double* labels,
                                    const double* weights, int64_t n, const double* coef,
                                    const double* inverseStd, const double* scaledMean,
                                    double* grad, double* lossSum, double* weightSum,
                                    void* stream) {
  return binary_add_dense(p, cyc::kLeastSquares, X, labels, weights, n, coef, inverseStd,
                          scaledMean, grad, lossSum, weightSum, stream);
}

int cyc_least_squares_add_csr_dev(cyc_logistic_plan p, const int64_t* rowptr,
                                  const int32_t* colidx, const double* vals, const double* labels,
                                  const double* weights, int64_t n, const double* coef,
                                  const double* inverseStd, const double* scaledMean,
                                  double* grad, double* lossSum, double* weightSum, cyc_csc csc,
                                  void* stream) {
  return binary_add_csr(p, cyc::kLeastSquares, rowptr, colidx, vals, labels, weights, n, coef,
                        inverseStd, scaledMean, grad, lossSum, weightSum, csc, stream);
}

}  // extern "C"
