// linreg.hip -- the evaluate pass of a fitted linear model on gfx950 (MI355X):
// predictions, and the ten sums and extrema behind LinearRegressionSummary
// (ml/regression/LinearRegression.scala, RegressionMetrics), in one read of
// the rows.
//
// Kernels (HBM-bound: one read of the rows, no MFMA)
//   k_linreg_rows<Rows, Lds, Stats>
//                     the row walk of row_walk.hpp (shared with glm.hip): one
//                     wave per run of 64-row batches, lane i ending up with
//                     row i's dot product, then lane i runs row i's epilogue.
//                     Stats = false: pred[r] = x_r . coef + intercept.
//                     Stats = true: the row's terms of the ten outputs into
//                     per-lane accumulators (and pred[r] if asked for); at
//                     the end one fixed xor tree per output over the wave and
//                     one slab row per wave.
//   k_linreg_fold     the slab folded in wave order, one block per output
//                     (sums 0..7, min 8, max 9).  No floating-point atomics:
//                     two calls on the same input give the same bits.
// Lds: the coefficients are staged in LDS once per workgroup while they fit
// kLdsCoef doubles (64 KiB: what a launch gets without opting in to more, and
// two workgroups still fit a CU's 160 KiB); longer vectors (wide sparse rows)
// are gathered from global memory, i.e. from L2, which holds the 8 numFeatures
// bytes of any width this library is used at.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <limits>
#include <map>
#include <mutex>
#include <utility>

#include "common.hpp"
#include "row_walk.hpp"

namespace {

using namespace cyc::rowwalk;

constexpr int kOut = 10;    // the outputs of a stats call
constexpr int kSums = 8;    // the first kSums are sums, then min and max
constexpr int kLdsCoef = 8192;

struct LinArgs {
  const double* y;
  const double* w;
  const double* coef;
  double intercept;
  double center;
  int64_t n;
  int p;
  int64_t batchesPerWave;
};

template <class Rows, bool Lds, bool Stats>
__global__ __launch_bounds__(256) void k_linreg_rows(Rows rows, LinArgs a,
                                                     double* __restrict__ pred,
                                                     double* __restrict__ slab) {
  extern __shared__ double sh[];
  if constexpr (Lds) {
    for (int f = threadIdx.x; f < a.p; f += blockDim.x) sh[f] = a.coef[f];
    __syncthreads();
  }
  const int lane = threadIdx.x & 63;
  const int64_t gw = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t batches = (a.n + 63) / 64;
  const int64_t b0 = gw * a.batchesPerWave;
  const int64_t b1 = min<int64_t>(batches, b0 + a.batchesPerWave);
  double acc[kSums];
#pragma unroll
  for (int c = 0; c < kSums; ++c) acc[c] = 0.0;
  double lo = INFINITY, hi = -INFINITY;
  for (int64_t b = b0; b < b1; ++b) {
    const int64_t base = b * 64, r = base + lane;
    const bool in = r < a.n;
    double w = in ? 1.0 : 0.0;
    if (Stats && in && a.w) w = a.w[r];
    const bool live = in && w != 0.0;
    // a row of weight 0 is read only for its prediction
    const bool read = Stats ? (pred ? in : live) : in;
    double dot;
    if constexpr (Lds) dot = rows.dot(base, lane, read, a.p, sh);
    else dot = rows.dot(base, lane, read, a.p, a.coef);
    const double pr = dot + a.intercept;
    if (in && pred) pred[r] = pr;
    if (Stats && live) {
      const double y = a.y[r];
      const double e = y - pr;
      const double dy = y - a.center, dp = pr - a.center;
      acc[0] += w;
      acc[1] += w * y;
      acc[2] += w * y * y;
      acc[3] += w * dy * dy;
      acc[4] += w * e;
      acc[5] += w * e * e;
      acc[6] += w * fabs(e);
      acc[7] += w * dp * dp;
      if (w > 0.0) {
        const double s = sqrt(w) * e;
        lo = fmin(lo, s);
        hi = fmax(hi, s);
      }
    }
  }
  if constexpr (Stats) {
    // waves past the last batch write the identities, so the fold reads all
#pragma unroll
    for (int c = 0; c < kSums; ++c) {
      double v = acc[c];
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
      if (lane == 0) slab[gw * kOut + c] = v;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      lo = fmin(lo, __shfl_xor(lo, m));
      hi = fmax(hi, __shfl_xor(hi, m));
    }
    if (lane == 0) {
      slab[gw * kOut + 8] = lo;
      slab[gw * kOut + 9] = hi;
    }
  }
}

// out[c] over waves of slab[wave][c], c = blockIdx.x: each thread a
// contiguous run in wave order, then the 256 partials in thread order.
__global__ __launch_bounds__(256) void k_linreg_fold(const double* __restrict__ slab,
                                                     int64_t waves, double* __restrict__ out) {
  __shared__ double part[256];
  const int c = blockIdx.x;
  const int64_t per = (waves + 255) / 256;
  const int64_t w0 = threadIdx.x * per, w1 = min<int64_t>(waves, w0 + per);
  double v = c < kSums ? 0.0 : (c == 8 ? INFINITY : -INFINITY);
  for (int64_t w = w0; w < w1; ++w) {
    const double x = slab[w * kOut + c];
    v = c < kSums ? v + x : (c == 8 ? fmin(v, x) : fmax(v, x));
  }
  part[threadIdx.x] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = part[0];
    for (int i = 1; i < 256; ++i)
      t = c < kSums ? t + part[i] : (c == 8 ? fmin(t, part[i]) : fmax(t, part[i]));
    out[c] = t;
  }
}

// The per-wave slab of a stats call: one per (device, stream), since calls on
// one stream are ordered and calls on two may overlap.  Never destroyed: the
// HIP runtime may be gone when static destructors run.
std::mutex g_mu;
std::map<std::pair<int, hipStream_t>, cyc::DeviceBuffer>* g_slabs = nullptr;

int slab_for(hipStream_t st, size_t bytes, double** out) {
  int dev = 0;
  CYC_HIP(hipGetDevice(&dev));
  if (!g_slabs) g_slabs = new std::map<std::pair<int, hipStream_t>, cyc::DeviceBuffer>();
  cyc::DeviceBuffer& b = (*g_slabs)[std::make_pair(dev, st)];
  if (int rc = b.reserve(bytes)) return rc;
  *out = (double*)b.ptr;
  return CYC_OK;
}

template <bool Stats>
void launch(const RowsArg& r, const LinArgs& a, const Geometry& g, double* pred, double* slab,
            hipStream_t st) {
  with_rows(r, a.coef, a.p, [&](auto rows) {
    using R = decltype(rows);
    if (a.p <= kLdsCoef)
      hipLaunchKernelGGL((k_linreg_rows<R, true, Stats>), dim3((unsigned)g.blocks), dim3(256),
                         sizeof(double) * (size_t)a.p, st, rows, a, pred, slab);
    else
      hipLaunchKernelGGL((k_linreg_rows<R, false, Stats>), dim3((unsigned)g.blocks), dim3(256),
                         0, st, rows, a, pred, slab);
  });
}

int run(const RowsArg& r, int64_t nrows, int32_t numFeatures, const double* y, const double* w,
        const double* coef, double intercept, double center, double* out, double* pred,
        bool stats, void* stream) {
  CYC_REQUIRE(nrows >= 0, "nrows >= 0");
  CYC_REQUIRE(numFeatures >= 1, "numFeatures must be positive but got " +
                                    std::to_string(numFeatures));
  CYC_REQUIRE(coef != nullptr, "coefficients must not be null");
  if (stats) CYC_REQUIRE(out != nullptr, "out must not be null");
  hipStream_t st = cyc::as_stream(stream);
  if (nrows == 0) {
    if (stats) {
      const double inf = std::numeric_limits<double>::infinity();
      const double empty[kOut] = {0, 0, 0, 0, 0, 0, 0, 0, inf, -inf};
      CYC_HIP(hipMemcpyAsync(out, empty, sizeof(empty), hipMemcpyHostToDevice, st));
      CYC_HIP(hipStreamSynchronize(st));
    }
    return CYC_OK;
  }
  if (stats) CYC_REQUIRE(y != nullptr, "labels must not be null");
  else CYC_REQUIRE(pred != nullptr, "out must not be null");
  if (r.sparse) {
    CYC_REQUIRE(r.rowptr && r.colidx && r.vals, "non-null CSR arrays");
    if (int rc = cyc::check_csr_indices(r.rowptr, r.colidx, nrows, numFeatures, st)) return rc;
  } else {
    CYC_REQUIRE(r.X != nullptr, "non-null rows");
  }
  const Geometry g = geometry(nrows);
  LinArgs a;
  a.y = y;
  a.w = w;
  a.coef = coef;
  a.intercept = intercept;
  a.center = center;
  a.n = nrows;
  a.p = numFeatures;
  a.batchesPerWave = g.batchesPerWave;
  if (!stats) {
    cyc::KernelTimer timer("k_linreg_predict", st);
    launch<false>(r, a, g, pred, nullptr, st);
    CYC_LAUNCH_CHECK("k_linreg_rows");
    return CYC_OK;
  }
  std::lock_guard<std::mutex> lock(g_mu);
  double* slab = nullptr;
  if (int rc = slab_for(st, sizeof(double) * (size_t)g.waves * kOut, &slab)) return rc;
  {
    cyc::KernelTimer timer("k_linreg_stats", st);
    launch<true>(r, a, g, pred, slab, st);
    CYC_LAUNCH_CHECK("k_linreg_rows");
  }
  hipLaunchKernelGGL(k_linreg_fold, dim3(kOut), dim3(256), 0, st, (const double*)slab, g.waves,
                     out);
  CYC_LAUNCH_CHECK("k_linreg_fold");
  return CYC_OK;
}

}  // namespace

extern "C" {

int cyc_linreg_predict_dev(const double* X, int64_t nrows, int32_t numFeatures,
                           const double* coef, double intercept, double* out, void* stream) {
  return run(dense_rows(X), nrows, numFeatures, nullptr, nullptr, coef, intercept, 0.0, nullptr,
             out, false, stream);
}

int cyc_linreg_predict_csr_dev(const int64_t* rowptr, const int32_t* colidx, const double* vals,
                               int64_t nrows, int32_t numFeatures, const double* coef,
                               double intercept, double* out, void* stream) {
  return run(csr_rows(rowptr, colidx, vals), nrows, numFeatures, nullptr, nullptr, coef,
             intercept, 0.0, nullptr, out, false, stream);
}

int cyc_linreg_stats_dev(const double* X, int64_t nrows, int32_t numFeatures, const double* y,
                         const double* w, const double* coef, double intercept, double center,
                         double* out, double* pred, void* stream) {
  return run(dense_rows(X), nrows, numFeatures, y, w, coef, intercept, center, out, pred, true,
             stream);
}

int cyc_linreg_stats_csr_dev(const int64_t* rowptr, const int32_t* colidx, const double* vals,
                             int64_t nrows, int32_t numFeatures, const double* y,
                             const double* w, const double* coef, double intercept,
                             double center, double* out, double* pred, void* stream) {
  return run(csr_rows(rowptr, colidx, vals), nrows, numFeatures, y, w, coef, intercept, center,
             out, pred, true, stream);
}

}  // extern "C"
