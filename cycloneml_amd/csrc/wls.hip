// wls.hip -- the WeightedLeastSquares aggregate on gfx950 (MI355X): the
// normal-equation moments behind LinearRegression (linreg.hip,
// regression.py) and every IRLS step of GeneralizedLinearRegression
// (glm.hip).
//
// WeightedLeastSquares.Aggregator.add (ml/optim/WeightedLeastSquares.scala)
// as one weighted syrk: the staged tiles of syrk_tiles.hpp over the augmented
// row z_r = [a_r, b_r, 1.0] of width q = p + 2, U += sum_r w_r z_r z_r^T.
// The packed result holds every aggregator field: aaSum (leading p x p),
// abSum (column p), bbSum (p, p), aSum (column p + 1), bSum (p, p + 1), wSum
// (p + 1, p + 1).  Tiles, slabs, split sizing and the fold are the
// Gramian's (k_gram_tiles) with q for p.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include <mutex>
#include <string>

#include "common.hpp"
#include "syrk_tiles.hpp"

namespace {

// The augmented, weighted rows.  The i-side panel is scaled by w_r as it is
// staged (one dmul per element: spr's alpha x_i), the j-side panel is staged
// as it is.  A row of weight 0 stages zeros in both panels without reading
// its features (the reference's `if (w > 0.0)`: NaN or Inf features of such a
// row never reach an accumulator).  A negative or NaN weight raises *flag
// (the row stages zeros; the host fails the call).
struct WlsRows {
  const double* __restrict__ X;
  int p;
  const double* __restrict__ y;
  const double* __restrict__ w;
  int* __restrict__ flag;

  __device__ __forceinline__ void panel(const double* rowp, double yr, int c0, double* dst) const {
    if ((p & 1) == 0 && c0 + 8 <= p) {
      load8(rowp + c0, dst);
    } else {
      // ragged panels, odd p and the augmented columns: label, then ones
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int c = c0 + e;
        double v = 0.0;
        if (c < p) v = rowp[c];
        else if (c == p) v = yr;
        else if (c == p + 1) v = 1.0;
        dst[e] = v;
      }
    }
  }

  __device__ __forceinline__ bool fill(int64_t r, int ci, int cj, double* ri, double* rj) const {
    const double wr = w ? w[r] : 1.0;
    // once per row: the first tile pair's first staging thread of the row
    if (!(wr >= 0.0) && blockIdx.x == 0 && (threadIdx.x & 15) == 0) atomicOr(flag, 1);
    if (!(wr > 0.0)) return false;
    const double* rowp = X + r * p;
    const double yr = y[r];
    panel(rowp, yr, ci, ri);
    panel(rowp, yr, cj, rj);
#pragma unroll
    for (int e = 0; e < 8; ++e) ri[e] = dmul(wr, ri[e]);
    return true;
  }
};

__global__ __launch_bounds__(GT, 2) void k_wls_tiles(
    const double* __restrict__ X, int64_t nrows, int p, const double* __restrict__ y,
    const double* __restrict__ w, int tilesPerSide, int64_t rowsPerSplit,
    double* __restrict__ slab, int* __restrict__ flag) {
  staged_tiles(WlsRows{X, p, y, w, flag}, nrows, tilesPerSide, rowsPerSplit, slab);
}

}  // namespace

// The weighted syrk of width numFeatures + 2 (k_wls_tiles): its split-K slab,
// the densified CSR chunk and the bad-weight flag.
struct cyc_wls_plan_s {
  int p = 0;   // numFeatures
  std::mutex mu;
  cyc::DeviceBuffer slab;
  cyc::DeviceBuffer chunk;
  cyc::DeviceBuffer flag;
  int64_t lastSplits = 0;
};

namespace {

// U += the weighted syrk of the augmented rows (width q = p + 2)
int wls_locked(cyc_wls_plan plan, const double* X, int64_t nrows, const double* y,
               const double* w, double* U, hipStream_t st) {
  const int p = plan->p, q = p + 2;
  const int tps = tiles_per_side(q), pairs = tile_pairs(tps);
  const SplitK sk = split_rows(nrows, pairs, 2);
  plan->lastSplits = sk.splits;
  if (int rc = plan->slab.reserve(slab_bytes(sk.splits, pairs))) return rc;
  {
    cyc::KernelTimer timer("k_wls_tiles", st);
    hipLaunchKernelGGL(k_wls_tiles, dim3(pairs, (unsigned)sk.splits), dim3(GT), 0, st, X, nrows, p,
                       y, w, tps, sk.rowsPerSplit, (double*)plan->slab.ptr, (int*)plan->flag.ptr);
    CYC_LAUNCH_CHECK("k_wls_tiles");
  }
  return fold_slabs((const double*)plan->slab.ptr, sk.splits, tps, q, U, st);
}

// Aggregator.add's require on the instance weight, once the call's kernels
// have run: the flag read back on the call's stream.
int wls_check_weights(cyc_wls_plan plan, hipStream_t st) {
  int bad = 0;
  CYC_HIP(hipMemcpyAsync(&bad, plan->flag.ptr, sizeof(int), hipMemcpyDeviceToHost, st));
  CYC_HIP(hipStreamSynchronize(st));
  CYC_REQUIRE(bad == 0, "Negative weight: instance weights have to be >= 0.0");
  return CYC_OK;
}

}  // namespace

extern "C" {

int cyc_wls_plan_create(int32_t numFeatures, cyc_wls_plan* plan) {
  CYC_REQUIRE(plan != nullptr, "plan must not be null");
  // WeightedLeastSquares.MAX_NUM_FEATURES
  CYC_REQUIRE(numFeatures <= 4096,
              "In order to take the normal equation approach efficiently, we set the max "
              "number of features to 4096 but got " + std::to_string(numFeatures) + ".");
  CYC_REQUIRE(numFeatures > 0, "numFeatures must be positive");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    cyc::set_error("no HIP device visible");
    return CYC_ERR_NO_DEVICE;
  }
  auto* p = new cyc_wls_plan_s();
  p->p = numFeatures;
  *plan = p;
  return CYC_OK;
}

int cyc_wls_plan_destroy(cyc_wls_plan plan) {
  delete plan;
  return CYC_OK;
}

int cyc_wls_last_splits(cyc_wls_plan plan, int64_t* splits) {
  CYC_REQUIRE(plan != nullptr && splits != nullptr, "plan and splits must not be null");
  std::lock_guard<std::mutex> g(plan->mu);
  *splits = plan->lastSplits;
  return CYC_OK;
}

int cyc_wls_accumulate_dev(cyc_wls_plan plan, const double* X, int64_t nrows, const double* y,
                           const double* w, double* U, void* stream) {
  CYC_REQUIRE(plan != nullptr && U != nullptr, "plan and U must not be null");
  CYC_REQUIRE(nrows >= 0, "nrows >= 0");
  if (nrows == 0) return CYC_OK;
  CYC_REQUIRE(X != nullptr && y != nullptr, "non-null rows and labels");
  hipStream_t st = cyc::as_stream(stream);
  std::lock_guard<std::mutex> g(plan->mu);
  if (int rc = plan->flag.reserve(sizeof(int))) return rc;
  CYC_HIP(hipMemsetAsync(plan->flag.ptr, 0, sizeof(int), st));
  if (int rc = wls_locked(plan, X, nrows, y, w, U, st)) return rc;
  return wls_check_weights(plan, st);
}

int cyc_wls_accumulate_csr_dev(cyc_wls_plan plan, const int64_t* rowptr, const int32_t* colidx,
                               const double* vals, int64_t nrows, const double* y,
                               const double* w, double* U, void* stream) {
  CYC_REQUIRE(plan != nullptr && U != nullptr, "plan and U must not be null");
  CYC_REQUIRE(nrows >= 0, "nrows >= 0");
  if (nrows == 0) return CYC_OK;
  CYC_REQUIRE(rowptr && colidx && vals && y, "non-null CSR arrays and labels");
  hipStream_t st = cyc::as_stream(stream);
  if (int rc = cyc::check_csr_indices(rowptr, colidx, nrows, plan->p, st)) return rc;
  std::lock_guard<std::mutex> g(plan->mu);
  if (int rc = plan->flag.reserve(sizeof(int))) return rc;
  CYC_HIP(hipMemsetAsync(plan->flag.ptr, 0, sizeof(int), st));
  int64_t done = 0;   // the chunks come in row order
  int rc = over_csr_chunks(plan->chunk, plan->p, rowptr, colidx, vals, nrows, st,
                           [&](const double* D, int64_t nr) {
                             const int r = wls_locked(plan, D, nr, y + done, w ? w + done : nullptr,
                                                      U, st);
                             done += nr;
                             return r;
                           });
  if (rc) return rc;
  return wls_check_weights(plan, st);
}

}  // extern "C"
