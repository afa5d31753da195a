// logistic_plan.hpp -- the plan the block aggregators share (logistic.hip
// creates it; logistic_binary.hip and logistic_multinomial.hip run on it).
#pragma once

#include <hip/hip_runtime.h>

#include <mutex>

#include "common.hpp"

namespace cyc {

// A binary plan's aggregator: the `kind` of row_margin / bin_row
// (binary_rows.hpp) and of tiles_rows (tiles.hpp).
enum LossKind : int {
  kLogistic = 0,       // BinaryLogisticBlockAggregator (and every multinomial plan)
  kHinge = 1,          // HingeBlockAggregator (LinearSVC)
  kLeastSquares = 2,   // LeastSquaresBlockAggregator
  kHuber = 3,          // HuberBlockAggregator
  kAft = 4,            // AFTBlockAggregator
};

// Folds both families end with (kernels in logistic.hip).
// out[c] = sum over the `waves` partials slabS[w * width + c], in a fixed order.
int fold_scalars(const double* slabS, int64_t waves, int width, double* out, hipStream_t st);
// *lossSum += s2[0]; *weightSum += s2[1]
int add_scalars(const double* s2, double* lossSum, double* weightSum, hipStream_t st);

__device__ __forceinline__ double wave_sum_bcast(double s) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m);
  return __shfl(s, 0);  // every lane takes lane 0's association order
}

}  // namespace cyc

struct cyc_logistic_plan_s {
  int F = 0, C = 1, fitIntercept = 0, fitWithMean = 0;
  cyc::LossKind loss = cyc::kLogistic;
  double labelStd = 1.0, labelMean = 0.0;   // least squares
  double epsilon = 1.35;                     // Huber
  std::mutex mu;   // held over an add: the scratch below belongs to one call at a time
  cyc::DeviceBuffer effCoef;
  cyc::DeviceBuffer slabG, slabS, slabMS, gradAcc, scal, offset, multBuf, gslab, msTot;
  cyc::DeviceBuffer rowMult;
};

namespace cyc {

inline int check_common(cyc_logistic_plan p, const double* coef, const double* sm) {
  CYC_REQUIRE(p != nullptr && coef != nullptr, "plan and coefficients must not be null");
  if (p->fitWithMean) {
    CYC_REQUIRE(p->fitIntercept, "for training without intercept, should not center the vectors");
    CYC_REQUIRE(sm != nullptr, "scaled means is required when center the vectors");
  }
  return CYC_OK;
}

}  // namespace cyc
