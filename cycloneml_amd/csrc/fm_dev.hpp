// fm_dev.hpp -- what fm.hip (dense rows) and fm_csr.hip (CSR rows) share: the
// plan, the batch rule, the row epilogue (raw, loss and multiplier), the
// coefficients' split and the lowest-bad-label report.
#pragma once
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include <cmath>
#include <mutex>
#include <string>

#include "binary_rows.hpp"
#include "common.hpp"

struct cyc_fm_plan_s {
  std::mutex mu;
  int d = 0, k = 0;
  int fitIntercept = 0, fitLinear = 0, loss = 0;
  int64_t wsBytes = 0;
  cyc::DeviceBuffer dense, image, accum, ws, bad;
};

namespace cyc::fmdev {

constexpr int kFmRunRows = 1024;
constexpr int kMaxFactors = 64;
constexpr uint64_t kFmGolden = 0x9E3779B97F4A7C15ull;
constexpr uint64_t kNoBadRow = 0x7f7f7f7f7f7f7f7full;   // memset(0x7f)
constexpr int kLossSquared = 0, kLossLogistic = 1;

// forest.py's mix(), the batch rule: row r of iteration i is taken iff the top
// 53 bits of mix(42 + i, 0, 0, r) are >= floor((1 - fraction) 2^53)
__host__ __device__ __forceinline__ uint64_t fm_fin(uint64_t z) {
  z ^= z >> 30;
  z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27;
  z *= 0x94D049BB133111EBull;
  z ^= z >> 31;
  return z;
}
__device__ __forceinline__ bool fm_take(uint64_t h1, uint64_t thr, int64_t globalRow) {
  return (fm_fin(h1 + kFmGolden * ((uint64_t)globalRow + 1ull)) >> 11) >= thr;
}
// the two arguments of fm_take for iteration iter and fraction
inline uint64_t fm_seed(int64_t iter) {
  return fm_fin(fm_fin((uint64_t)(42 + iter) + kFmGolden) + kFmGolden);
}
inline uint64_t fm_threshold(double fraction) {
  return (uint64_t)std::floor((1.0 - fraction) * 9007199254740992.0);
}

// raw of one row from its finished products: S1 = x [V | w], S2 = x^2 V^2
__device__ __forceinline__ double fm_raw(const double* S1, const double* S2, int k, double b) {
  double raw = b + S1[k];
  for (int f = 0; f < k; ++f) {
    const double s = S1[f];
    raw += 0.5 * (s * s - S2[f]);
  }
  return raw;
}

// loss and multiplier; false: a classifier's label that is not 0 / 1
__device__ __forceinline__ bool fm_loss(int loss, double raw, double y, double* l, double* m) {
  if (loss == kLossSquared) {
    const double diff = raw - y;
    *l = diff * diff;
    *m = 2.0 * diff;
    return true;
  }
  if (!(y == 0.0 || y == 1.0)) return false;
  *l = y > 0 ? cyc::log1p_exp(-raw) : cyc::log1p_exp(raw);
  *m = 1.0 / (1.0 + exp(-raw)) - y;
  return true;
}

// the only atomic: the lowest global row whose label is not 0 / 1
__device__ __forceinline__ void fm_flag_bad(unsigned long long* bad, int64_t globalRow) {
  atomicMin(bad, (unsigned long long)globalRow);
}
inline int fm_clear_bad(cyc_fm_plan_s* p, hipStream_t st) {
  if (int rc = p->bad.reserve(sizeof(unsigned long long))) return rc;
  CYC_HIP(hipMemsetAsync(p->bad.ptr, 0x7f, sizeof(unsigned long long), st));
  return CYC_OK;
}
// a logistic plan's end of an evaluation: synchronizes, fails on a flagged row
inline int fm_report_bad(cyc_fm_plan_s* p, hipStream_t st) {
  if (p->loss != kLossLogistic) return CYC_OK;
  unsigned long long row = kNoBadRow;
  CYC_HIP(hipMemcpyAsync(&row, p->bad.ptr, sizeof(row), hipMemcpyDeviceToHost, st));
  CYC_HIP(hipStreamSynchronize(st));
  CYC_REQUIRE(row == kNoBadRow, "Classification labels should be 0 or 1 but row " +
                                    std::to_string(row) + " has another label");
  return CYC_OK;
}

struct Coef {
  const double *V, *w, *b;
};
inline Coef split_coef(const cyc_fm_plan_s* p, const double* coef) {
  const int64_t dk = (int64_t)p->d * p->k;
  Coef c{coef, nullptr, nullptr};
  if (p->fitLinear) c.w = coef + dk;
  if (p->fitIntercept) c.b = coef + dk + (p->fitLinear ? p->d : 0);
  return c;
}

// the argument checks both evaluate entry points make
inline int fm_check_evaluate(const void* plan, int64_t nrows, int64_t rowOffset, const void* coef,
                             const void* out, double fraction) {
  CYC_REQUIRE(plan != nullptr, "plan must not be null");
  CYC_REQUIRE(nrows >= 0 && rowOffset >= 0, "nrows >= 0 and rowOffset >= 0");
  CYC_REQUIRE(coef != nullptr && out != nullptr, "coef and out must not be null");
  CYC_REQUIRE(fraction > 0.0 && fraction <= 1.0,
              "miniBatchFraction must be in (0, 1] but got " + cyc::java_double(fraction));
  return CYC_OK;
}

}  // namespace cyc::fmdev
