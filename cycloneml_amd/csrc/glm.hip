// glm.hip -- the per-row passes of GeneralizedLinearRegression's IRLS fit on
// gfx950 (MI355X): ml/regression/GeneralizedLinearRegression.scala
// (FamilyAndLink.initialize / reweightFunc / fitted, the families' deviance
// and aic terms) around the WLS aggregate of wls.hip (k_wls_tiles).
//
// Family and link are two integer codes in the plan, dispatched per row by
// the __device__ functions below: one kernel per pass and row layout, not
// one per pair.
//
// Kernels (HBM-bound: one read of the rows, no MFMA, coefficients in LDS)
//   k_glm_rows<Rows>   one wave per run of 64-row batches.  The wave forms
//                      the 64 dot products of a batch so that lane i ends up
//                      holding row i's, then every lane runs its own row's
//                      epilogue (link, variance, the exp / log / pow behind
//                      them) once: the transcendental work is per row, not
//                      per row and lane.  Modes: reweight (z, w'), mean (mu)
//                      and link prediction (eta).
//   k_glm_init         FamilyAndLink.initialize: elementwise, no features.
//   k_glm_stats<Rows>  the same batches with the summary's six sums as the
//                      epilogue; per-wave partials to a slab.
//   k_glm_fold         the slab folded in a fixed order (k_fold_scalars'
//                      shape, one block per sum).
// Rows (row_walk.hpp): DenseRows<LPR> (LPR = 8 / 16 / 32 / 64 lanes per row,
// the smallest that holds numFeatures, 64 / LPR rows in flight per wave),
// CsrRows (a wave per row, coefficients gathered by column index) and NoRows
// (coef == NULL: eta = intercept + offset).
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <mutex>

#include "common.hpp"
#include "row_walk.hpp"

namespace {

// the row walk (DenseRows / CsrRows / NoRows, geometry, with_rows), shared
// with linreg.hip
using namespace cyc::rowwalk;

constexpr double kEps = 1e-16;     // GeneralizedLinearRegression.epsilon
constexpr double kDelta = 0.1;     // Poisson / Tweedie delta
constexpr int kSums = 6;

struct GlmSpec {
  int family;
  int link;
  double vp;   // variancePower (tweedie)
  double lp;   // linkPower (power link)
};

// The large math routines once each, as calls: inlined at every use they
// drive the row kernels to 256 VGPRs and one wave per SIMD.
__device__ __noinline__ double glm_pow(double x, double e) { return pow(x, e); }
__device__ __noinline__ double glm_lgamma(double x) { return lgamma(x); }
__device__ __noinline__ double glm_normcdfinv(double x) { return normcdfinv(x); }
__device__ __noinline__ double glm_normcdf(double x) { return normcdf(x); }

// ---- families ---------------------------------------------------------------
__device__ __forceinline__ bool fam_label_ok(const GlmSpec& s, double y) {
  switch (s.family) {
    case CYC_GLM_BINOMIAL: return y >= 0.0 && y <= 1.0;
    case CYC_GLM_POISSON: return y >= 0.0;
    case CYC_GLM_GAMMA: return y > 0.0;
    case CYC_GLM_TWEEDIE: return s.vp >= 2.0 ? y > 0.0 : (s.vp >= 1.0 ? y >= 0.0 : true);
    default: return true;
  }
}

__device__ __forceinline__ double fam_initialize(const GlmSpec& s, double y, double w) {
  switch (s.family) {
    case CYC_GLM_BINOMIAL: return (w * y + 0.5) / (w + 1.0);
    case CYC_GLM_POISSON: return fmax(y, kDelta);
    case CYC_GLM_TWEEDIE: return y == 0.0 ? kDelta : y;
    default: return y;
  }
}

__device__ __forceinline__ double fam_variance(const GlmSpec& s, double mu) {
  switch (s.family) {
    case CYC_GLM_BINOMIAL: return mu * (1.0 - mu);
    case CYC_GLM_POISSON: return mu;
    case CYC_GLM_GAMMA: return mu * mu;
    case CYC_GLM_TWEEDIE: return glm_pow(mu, s.vp);
    default: return 1.0;
  }
}

__device__ __forceinline__ double fam_project(const GlmSpec& s, double mu) {
  switch (s.family) {
    case CYC_GLM_GAUSSIAN: return mu;
    case CYC_GLM_BINOMIAL: return mu < kEps ? kEps : (mu > 1.0 - kEps ? 1.0 - kEps : mu);
    default: return mu < kEps ? kEps : (isinf(mu) ? DBL_MAX : mu);
  }
}

__device__ __forceinline__ double ylogy(double y, double mu) {
  return y == 0.0 ? 0.0 : y * log(y / mu);
}

__device__ __forceinline__ double tweedie_yp(double y, double mu, double p) {
  return p == 0.0 ? log(y / mu) : (glm_pow(y, p) - glm_pow(mu, p)) / p;
}

__device__ __forceinline__ double fam_deviance(const GlmSpec& s, double y, double mu, double w) {
  switch (s.family) {
    case CYC_GLM_BINOMIAL: return 2.0 * w * (ylogy(y, mu) + ylogy(1.0 - y, 1.0 - mu));
    case CYC_GLM_POISSON: return 2.0 * w * (ylogy(y, mu) - (y - mu));
    case CYC_GLM_GAMMA: return -2.0 * w * (log(y / mu) - (y - mu) / mu);
    case CYC_GLM_TWEEDIE: {
      // y >= delta inside the first term for Poisson and compound Poisson
      const double y1 = (s.vp >= 1.0 && s.vp < 2.0) ? fmax(y, kDelta) : y;
      return 2.0 * w * (y * tweedie_yp(y1, mu, 1.0 - s.vp) - tweedie_yp(y, mu, 2.0 - s.vp));
    }
    default: return w * (y - mu) * (y - mu);
  }
}

// The log-likelihood term of family.aic (0 where aic needs none).
__device__ __forceinline__ double fam_loglik(const GlmSpec& s, double y, double mu, double w,
                                             double dispersion) {
  switch (s.family) {
    case CYC_GLM_BINOMIAL: {
      const double n = floor(w + 0.5);          // math.round
      if (n == 0.0) return 0.0;
      const double k = floor(y * w + 0.5);
      return glm_lgamma(n + 1.0) - glm_lgamma(k + 1.0) - glm_lgamma(n - k + 1.0) + k * log(mu) +
             (n - k) * log(1.0 - mu);
    }
    case CYC_GLM_POISSON: {
      const double k = trunc(y);                // y.toInt
      return w * (k * log(mu) - mu - glm_lgamma(k + 1.0));
    }
    case CYC_GLM_GAMMA: {
      const double a = 1.0 / dispersion, sc = mu * dispersion;
      return w * ((a - 1.0) * log(y) - y / sc - glm_lgamma(a) - a * log(sc));
    }
    default: return 0.0;
  }
}

// ---- links --------------------------------------------------------------------
__device__ __forceinline__ double std_normal_pdf(double x) {
  return exp(-0.5 * x * x) * 0.3989422804014327;   // 1 / sqrt(2 pi)
}

__device__ __forceinline__ double link_link(const GlmSpec& s, double mu) {
  switch (s.link) {
    case CYC_GLM_LOG: return log(mu);
    case CYC_GLM_INVERSE: return 1.0 / mu;
    case CYC_GLM_LOGIT: return log(mu / (1.0 - mu));
    case CYC_GLM_PROBIT: return glm_normcdfinv(mu);
    case CYC_GLM_CLOGLOG: return log(-log(1.0 - mu));
    case CYC_GLM_SQRT: return sqrt(mu);
    case CYC_GLM_POWER: return s.lp == 0.0 ? log(mu) : glm_pow(mu, s.lp);
    default: return mu;
  }
}

__device__ __forceinline__ double link_deriv(const GlmSpec& s, double mu) {
  switch (s.link) {
    case CYC_GLM_LOG: return 1.0 / mu;
    case CYC_GLM_INVERSE: return -1.0 / (mu * mu);
    case CYC_GLM_LOGIT: return 1.0 / (mu * (1.0 - mu));
    case CYC_GLM_PROBIT: return 1.0 / std_normal_pdf(glm_normcdfinv(mu));
    case CYC_GLM_CLOGLOG: return 1.0 / ((mu - 1.0) * log(1.0 - mu));
    case CYC_GLM_SQRT: return 1.0 / (2.0 * sqrt(mu));
    case CYC_GLM_POWER: return s.lp == 0.0 ? 1.0 / mu : s.lp * glm_pow(mu, s.lp - 1.0);
    default: return 1.0;
  }
}

__device__ __forceinline__ double link_unlink(const GlmSpec& s, double eta) {
  switch (s.link) {
    case CYC_GLM_LOG: return exp(eta);
    case CYC_GLM_INVERSE: return 1.0 / eta;
    case CYC_GLM_LOGIT: return 1.0 / (1.0 + exp(-eta));
    case CYC_GLM_PROBIT: return glm_normcdf(eta);
    case CYC_GLM_CLOGLOG: return 1.0 - exp(-exp(eta));
    case CYC_GLM_SQRT: return eta * eta;
    case CYC_GLM_POWER: return s.lp == 0.0 ? exp(eta) : glm_pow(eta, 1.0 / s.lp);
    default: return eta;
  }
}

struct GlmArgs {
  const double* y;
  const double* w;
  const double* off;
  const double* coef;   // NULL with NoRows
  double intercept;
  int64_t n;
  int p;
  int64_t batchesPerWave;
  GlmSpec s;
};

enum { MODE_STEP = 0, MODE_MU = 1, MODE_ETA = 2 };

__device__ __forceinline__ void stage_coef(const GlmArgs& a, double* cf) {
  if (a.coef)
    for (int f = threadIdx.x; f < a.p; f += blockDim.x) cf[f] = a.coef[f];
  __syncthreads();
}

// One row's outputs from its dot product (mode: MODE_*).
__device__ __forceinline__ void row_out(const GlmArgs& a, int mode, int64_t r, double w,
                                        double dot, double* __restrict__ out0,
                                        double* __restrict__ out1, int* __restrict__ flag) {
  const double off = a.off ? a.off[r] : 0.0;
  const double eta = dot + a.intercept + off;
  if (mode == MODE_ETA) {
    out0[r] = eta;
    return;
  }
  const double mu = fam_project(a.s, link_unlink(a.s, eta));
  if (mode == MODE_MU) {
    out0[r] = mu;
    return;
  }
  const double y = a.y[r];
  if (!fam_label_ok(a.s, y)) atomicOr(flag, 1);
  double z = 0.0, wo = 0.0;
  if (w != 0.0) {
    const double g = link_deriv(a.s, mu);
    z = eta - off + (y - mu) * g;
    wo = w / (g * g * fam_variance(a.s, mu));
  }
  out0[r] = z;
  out1[r] = wo;
}

template <class Rows>
__global__ __launch_bounds__(256) void k_glm_rows(Rows rows, GlmArgs a, int mode,
                                                  double* __restrict__ out0,
                                                  double* __restrict__ out1,
                                                  int* __restrict__ flag) {
  extern __shared__ double cf[];
  stage_coef(a, cf);
  const int lane = threadIdx.x & 63;
  const int64_t gw = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t batches = (a.n + 63) / 64;
  const int64_t b0 = gw * a.batchesPerWave;
  const int64_t b1 = min<int64_t>(batches, b0 + a.batchesPerWave);
  for (int64_t b = b0; b < b1; ++b) {
    const int64_t base = b * 64, r = base + lane;
    const bool in = r < a.n;
    const double w = in ? (a.w ? a.w[r] : 1.0) : 0.0;
    const double dot = rows.dot(base, lane, in && w != 0.0, a.p, cf);
    if (in) row_out(a, mode, r, w, dot, out0, out1, flag);
  }
}

__global__ __launch_bounds__(256) void k_glm_init(GlmArgs a, double* __restrict__ z,
                                                  double* __restrict__ wOut,
                                                  int* __restrict__ flag) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= a.n) return;
  const double y = a.y[r];
  const double w = a.w ? a.w[r] : 1.0;
  if (!fam_label_ok(a.s, y)) atomicOr(flag, 1);
  const double mu = fam_initialize(a.s, y, w);
  z[r] = link_link(a.s, mu) - (a.off ? a.off[r] : 0.0);
  wOut[r] = w;
}

template <class Rows>
__global__ __launch_bounds__(256) void k_glm_stats(Rows rows, GlmArgs a, int project,
                                                   double dispersion, double* __restrict__ slab) {
  extern __shared__ double cf[];
  stage_coef(a, cf);
  const int lane = threadIdx.x & 63;
  const int64_t gw = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t batches = (a.n + 63) / 64;
  const int64_t b0 = gw * a.batchesPerWave;
  const int64_t b1 = min<int64_t>(batches, b0 + a.batchesPerWave);
  double acc[kSums];
#pragma unroll
  for (int c = 0; c < kSums; ++c) acc[c] = 0.0;
  for (int64_t b = b0; b < b1; ++b) {
    const int64_t base = b * 64, r = base + lane;
    const bool in = r < a.n;
    const double w = in ? (a.w ? a.w[r] : 1.0) : 0.0;
    const bool live = in && w != 0.0;
    const double dot = rows.dot(base, lane, live, a.p, cf);
    if (in) acc[5] += log(w);
    if (live) {
      const double y = a.y[r];
      const double eta = dot + a.intercept + (a.off ? a.off[r] : 0.0);
      double mu = link_unlink(a.s, eta);
      if (project) mu = fam_project(a.s, mu);
      acc[0] += w;
      acc[1] += w * y;
      acc[2] += fam_deviance(a.s, y, mu, w);
      acc[3] += w * (y - mu) * (y - mu) / fam_variance(a.s, mu);
      acc[4] += fam_loglik(a.s, y, mu, w, dispersion);
    }
  }
  // waves past the last batch write zero partials, so the fold reads all
#pragma unroll
  for (int c = 0; c < kSums; ++c) {
    double v = acc[c];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    if (lane == 0) slab[gw * kSums + c] = v;
  }
}

// out[c] = sum over waves of slab[wave][c], c = blockIdx.x: each thread a
// contiguous run in wave order, then the 256 partials in thread order.
__global__ __launch_bounds__(256) void k_glm_fold(const double* __restrict__ slab, int64_t waves,
                                                  double* __restrict__ out) {
  __shared__ double sh[256];
  const int c = blockIdx.x;
  const int64_t per = (waves + 255) / 256;
  const int64_t w0 = threadIdx.x * per, w1 = min<int64_t>(waves, w0 + per);
  double v = 0.0;
  for (int64_t w = w0; w < w1; ++w) v += slab[w * kSums + c];
  sh[threadIdx.x] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int i = 0; i < 256; ++i) t += sh[i];
    out[c] = t;
  }
}

}  // namespace

struct cyc_glm_plan_s {
  int p = 0;   // numFeatures
  GlmSpec spec{};
  std::mutex mu;
  cyc::DeviceBuffer flag;
  cyc::DeviceBuffer slab;
};

namespace {

const char* label_message(const GlmSpec& s) {
  switch (s.family) {
    case CYC_GLM_BINOMIAL: return "The response variable of Binomial family should be in range [0, 1].";
    case CYC_GLM_POISSON: return "The response variable of Poisson family should be non-negative.";
    case CYC_GLM_GAMMA: return "The response variable of Gamma family should be positive.";
    default:
      return s.vp >= 2.0 ? "The response variable of the specified Tweedie distribution should be positive."
                         : "The response variable of the specified Tweedie distribution should be non-negative.";
  }
}

GlmArgs make_args(cyc_glm_plan plan, int64_t n, const double* y, const double* w,
                  const double* off, const double* coef, double intercept, const Geometry& g) {
  GlmArgs a;
  a.y = y;
  a.w = w;
  a.off = off;
  a.coef = coef;
  a.intercept = intercept;
  a.n = n;
  a.p = plan->p;
  a.batchesPerWave = g.batchesPerWave;
  a.s = plan->spec;
  return a;
}

int check_rows(cyc_glm_plan plan, const RowsArg& r, const double* coef, int64_t nrows,
               hipStream_t st) {
  if (!coef) return CYC_OK;
  if (r.sparse) {
    CYC_REQUIRE(r.rowptr && r.colidx && r.vals, "non-null CSR arrays");
    return cyc::check_csr_indices(r.rowptr, r.colidx, nrows, plan->p, st);
  }
  CYC_REQUIRE(r.X != nullptr, "non-null rows");
  return CYC_OK;
}

int rows_pass(cyc_glm_plan plan, const RowsArg& r, int64_t nrows, const double* y,
              const double* w, const double* off, const double* coef, double intercept, int mode,
              double* out0, double* out1, hipStream_t st) {
  const Geometry g = geometry(nrows);
  const GlmArgs a = make_args(plan, nrows, y, w, off, coef, intercept, g);
  const size_t lds = coef ? sizeof(double) * (size_t)plan->p : 0;
  cyc::KernelTimer timer("k_glm_rows", st);
  with_rows(r, coef, plan->p, [&](auto rows) {
    hipLaunchKernelGGL(k_glm_rows<decltype(rows)>, dim3((unsigned)g.blocks), dim3(256), lds, st,
                       rows, a, mode, out0, out1, (int*)plan->flag.ptr);
  });
  CYC_LAUNCH_CHECK("k_glm_rows");
  return CYC_OK;
}

int reweight(cyc_glm_plan plan, const RowsArg& r, int64_t nrows, const double* y, const double* w,
             const double* off, const double* coef, double intercept, int init, double* z,
             double* wOut, void* stream) {
  CYC_REQUIRE(plan != nullptr, "plan must not be null");
  CYC_REQUIRE(nrows >= 0, "nrows >= 0");
  if (nrows == 0) return CYC_OK;
  CYC_REQUIRE(y != nullptr && z != nullptr && wOut != nullptr,
              "labels, z and wOut must not be null");
  hipStream_t st = cyc::as_stream(stream);
  if (!init)
    if (int rc = check_rows(plan, r, coef, nrows, st)) return rc;
  std::lock_guard<std::mutex> g(plan->mu);
  if (int rc = plan->flag.reserve(sizeof(int))) return rc;
  CYC_HIP(hipMemsetAsync(plan->flag.ptr, 0, sizeof(int), st));
  if (init) {
    const GlmArgs a = make_args(plan, nrows, y, w, off, nullptr, 0.0, geometry(nrows));
    hipLaunchKernelGGL(k_glm_init, dim3((unsigned)((nrows + 255) / 256)), dim3(256), 0, st, a, z,
                       wOut, (int*)plan->flag.ptr);
    CYC_LAUNCH_CHECK("k_glm_init");
  } else if (int rc = rows_pass(plan, r, nrows, y, w, off, coef, intercept, MODE_STEP, z, wOut,
                                st)) {
    return rc;
  }
  // the families' require on the label, once the kernel has run
  int bad = 0;
  CYC_HIP(hipMemcpyAsync(&bad, plan->flag.ptr, sizeof(int), hipMemcpyDeviceToHost, st));
  CYC_HIP(hipStreamSynchronize(st));
  CYC_REQUIRE(bad == 0, label_message(plan->spec));
  return CYC_OK;
}

int mean(cyc_glm_plan plan, const RowsArg& r, int64_t nrows, const double* off,
         const double* coef, double intercept, int linkPrediction, double* out, void* stream) {
  CYC_REQUIRE(plan != nullptr, "plan must not be null");
  CYC_REQUIRE(nrows >= 0, "nrows >= 0");
  if (nrows == 0) return CYC_OK;
  CYC_REQUIRE(out != nullptr, "out must not be null");
  hipStream_t st = cyc::as_stream(stream);
  if (int rc = check_rows(plan, r, coef, nrows, st)) return rc;
  std::lock_guard<std::mutex> g(plan->mu);
  return rows_pass(plan, r, nrows, nullptr, nullptr, off, coef, intercept,
                   linkPrediction ? MODE_ETA : MODE_MU, out, nullptr, st);
}

int stats(cyc_glm_plan plan, const RowsArg& r, int64_t nrows, const double* y, const double* w,
          const double* off, const double* coef, double intercept, int project,
          double dispersion, double* sums, void* stream) {
  CYC_REQUIRE(plan != nullptr, "plan must not be null");
  CYC_REQUIRE(nrows >= 0, "nrows >= 0");
  if (nrows == 0) return CYC_OK;
  CYC_REQUIRE(y != nullptr && sums != nullptr, "labels and sums must not be null");
  hipStream_t st = cyc::as_stream(stream);
  if (int rc = check_rows(plan, r, coef, nrows, st)) return rc;
  std::lock_guard<std::mutex> lock(plan->mu);
  const Geometry g = geometry(nrows);
  if (int rc = plan->slab.reserve(sizeof(double) * (size_t)g.waves * kSums)) return rc;
  const GlmArgs a = make_args(plan, nrows, y, w, off, coef, intercept, g);
  const size_t lds = coef ? sizeof(double) * (size_t)plan->p : 0;
  {
    cyc::KernelTimer timer("k_glm_stats", st);
    with_rows(r, coef, plan->p, [&](auto rows) {
      hipLaunchKernelGGL(k_glm_stats<decltype(rows)>, dim3((unsigned)g.blocks), dim3(256), lds, st,
                         rows, a, project, dispersion, (double*)plan->slab.ptr);
    });
    CYC_LAUNCH_CHECK("k_glm_stats");
  }
  hipLaunchKernelGGL(k_glm_fold, dim3(kSums), dim3(256), 0, st, (const double*)plan->slab.ptr,
                     g.waves, sums);
  CYC_LAUNCH_CHECK("k_glm_fold");
  return CYC_OK;
}

bool link_allowed(int family, int link) {
  switch (family) {
    case CYC_GLM_GAUSSIAN:
      return link == CYC_GLM_IDENTITY || link == CYC_GLM_LOG || link == CYC_GLM_INVERSE;
    case CYC_GLM_BINOMIAL:
      return link == CYC_GLM_LOGIT || link == CYC_GLM_PROBIT || link == CYC_GLM_CLOGLOG;
    case CYC_GLM_POISSON:
      return link == CYC_GLM_LOG || link == CYC_GLM_IDENTITY || link == CYC_GLM_SQRT;
    case CYC_GLM_GAMMA:
      return link == CYC_GLM_INVERSE || link == CYC_GLM_IDENTITY || link == CYC_GLM_LOG;
    default:
      return false;
  }
}

}  // namespace

extern "C" {

int cyc_glm_plan_create(int32_t family, int32_t link, double variancePower, double linkPower,
                        int32_t numFeatures, cyc_glm_plan* plan) {
  CYC_REQUIRE(plan != nullptr, "plan must not be null");
  CYC_REQUIRE(family >= CYC_GLM_GAUSSIAN && family <= CYC_GLM_TWEEDIE,
              "unsupported family code " + std::to_string(family));
  CYC_REQUIRE(link >= CYC_GLM_IDENTITY && link <= CYC_GLM_POWER,
              "unsupported link code " + std::to_string(link));
  GlmSpec s{family, link, 0.0, 0.0};
  if (family == CYC_GLM_TWEEDIE) {
    CYC_REQUIRE(link == CYC_GLM_POWER, "the tweedie family takes linkPower (CYC_GLM_POWER)");
    CYC_REQUIRE(variancePower == 0.0 || variancePower >= 1.0,
                "variancePower must be 0.0 or in [1, inf) but got " +
                    cyc::java_double(variancePower));
    CYC_REQUIRE(linkPower == linkPower, "linkPower must not be NaN");
    // Family.fromParams, Link.fromParams
    if (variancePower == 0.0) s.family = CYC_GLM_GAUSSIAN;
    else if (variancePower == 1.0) s.family = CYC_GLM_POISSON;
    else if (variancePower == 2.0) s.family = CYC_GLM_GAMMA;
    else s.vp = variancePower;
    if (linkPower == 0.0) s.link = CYC_GLM_LOG;
    else if (linkPower == 1.0) s.link = CYC_GLM_IDENTITY;
    else if (linkPower == -1.0) s.link = CYC_GLM_INVERSE;
    else if (linkPower == 0.5) s.link = CYC_GLM_SQRT;
    else s.lp = linkPower;
  } else {
    static const char* const kFamily[] = {"gaussian", "binomial", "poisson", "gamma"};
    static const char* const kLink[] = {"identity", "log", "inverse", "logit", "probit",
                                        "cloglog", "sqrt", "power"};
    CYC_REQUIRE(link_allowed(family, link),
                std::string("Generalized Linear Regression with ") + kFamily[family] +
                    " family does not support " + kLink[link] + " link function.");
  }
  CYC_REQUIRE(numFeatures >= 1 && numFeatures <= 4096,
              "numFeatures must be in 1..4096 but got " + std::to_string(numFeatures));
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    cyc::set_error("no HIP device visible");
    return CYC_ERR_NO_DEVICE;
  }
  auto* p = new cyc_glm_plan_s();
  p->p = numFeatures;
  p->spec = s;
  *plan = p;
  return CYC_OK;
}

int cyc_glm_plan_destroy(cyc_glm_plan plan) {
  delete plan;
  return CYC_OK;
}

int cyc_glm_reweight_dev(cyc_glm_plan plan, const double* X, int64_t nrows, const double* y,
                         const double* w, const double* offset, const double* coef,
                         double intercept, int32_t init, double* z, double* wOut, void* stream) {
  return reweight(plan, dense_rows(X), nrows, y, w, offset, coef, intercept, init, z, wOut,
                  stream);
}

int cyc_glm_reweight_csr_dev(cyc_glm_plan plan, const int64_t* rowptr, const int32_t* colidx,
                             const double* vals, int64_t nrows, const double* y, const double* w,
                             const double* offset, const double* coef, double intercept,
                             int32_t init, double* z, double* wOut, void* stream) {
  return reweight(plan, csr_rows(rowptr, colidx, vals), nrows, y, w, offset, coef, intercept,
                  init, z, wOut, stream);
}

int cyc_glm_mean_dev(cyc_glm_plan plan, const double* X, int64_t nrows, const double* offset,
                     const double* coef, double intercept, int32_t linkPrediction, double* out,
                     void* stream) {
  return mean(plan, dense_rows(X), nrows, offset, coef, intercept, linkPrediction, out, stream);
}

int cyc_glm_mean_csr_dev(cyc_glm_plan plan, const int64_t* rowptr, const int32_t* colidx,
                         const double* vals, int64_t nrows, const double* offset,
                         const double* coef, double intercept, int32_t linkPrediction,
                         double* out, void* stream) {
  return mean(plan, csr_rows(rowptr, colidx, vals), nrows, offset, coef, intercept,
              linkPrediction, out, stream);
}

int cyc_glm_stats_dev(cyc_glm_plan plan, const double* X, int64_t nrows, const double* y,
                      const double* w, const double* offset, const double* coef,
                      double intercept, int32_t project, double dispersion, double* sums,
                      void* stream) {
  return stats(plan, dense_rows(X), nrows, y, w, offset, coef, intercept, project, dispersion,
               sums, stream);
}

int cyc_glm_stats_csr_dev(cyc_glm_plan plan, const int64_t* rowptr, const int32_t* colidx,
                          const double* vals, int64_t nrows, const double* y, const double* w,
                          const double* offset, const double* coef, double intercept,
                          int32_t project, double dispersion, double* sums, void* stream) {
  return stats(plan, csr_rows(rowptr, colidx, vals), nrows, y, w, offset, coef, intercept,
               project, dispersion, sums, stream);
}

}  // extern "C"
