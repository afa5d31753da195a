// logistic.hip -- the block aggregators' plan on gfx950 (MI355X): create and
// destroy for the six aggregator kinds, and the folds both families end with.
//
// Binary (logistic, hinge, least squares, Huber, AFT): logistic_binary.hip
// Multinomial:                                         logistic_multinomial.hip
// Merge: DifferentiableLossAggregator.scala:49-59 (gradientSum, lossSum,
//        weightSum add up; done in a fixed order, deterministic except the
//        plain-CSR binary gradient, see logistic_binary.hip).
//
// Kernels
//   k_fold_scalars   per-wave scalar partials summed in wave order
//   k_add_scalars    lossSum / weightSum += the folded pair
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include "logistic_plan.hpp"

namespace {

// Fold per-wave scalars in wave order: out[c] = sum_w slabS[w][c], c < width
// (binary: {loss, wsum, msum, sigmaGradSum}; multinomial: {loss, wsum}).
__global__ void k_fold_scalars(const double* __restrict__ slabS, int64_t waves, int width,
                               double* __restrict__ out) {
  __shared__ double sh[256];
  for (int c = 0; c < width; ++c) {
    double a = 0.0;
    const int64_t per = (waves + 255) / 256;
    const int64_t w0 = threadIdx.x * per, w1 = min<int64_t>(waves, w0 + per);
    for (int64_t w = w0; w < w1; ++w) a += slabS[w * width + c];
    sh[threadIdx.x] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
      double t = 0.0;
      for (int i = 0; i < 256; ++i) t += sh[i];
      out[c] = t;
    }
    __syncthreads();
  }
}

__global__ void k_add_scalars(const double* __restrict__ s2, double* __restrict__ lossSum,
                              double* __restrict__ weightSum) {
  *lossSum += s2[0];
  *weightSum += s2[1];
}

}  // namespace

namespace cyc {

int fold_scalars(const double* slabS, int64_t waves, int width, double* out, hipStream_t st) {
  hipLaunchKernelGGL(k_fold_scalars, dim3(1), dim3(256), 0, st, slabS, waves, width, out);
  CYC_LAUNCH_CHECK("k_fold_scalars");
  return CYC_OK;
}

int add_scalars(const double* s2, double* lossSum, double* weightSum, hipStream_t st) {
  hipLaunchKernelGGL(k_add_scalars, dim3(1), dim3(1), 0, st, s2, lossSum, weightSum);
  CYC_LAUNCH_CHECK("k_add_scalars");
  return CYC_OK;
}

}  // namespace cyc

extern "C" {

int cyc_logistic_plan_create(int32_t numFeatures, int32_t numClasses, int fitIntercept,
                             int fitWithMean, cyc_logistic_plan* plan) {
  CYC_REQUIRE(plan != nullptr, "plan must not be null");
  CYC_REQUIRE(numFeatures > 0, "numFeatures must be positive");
  CYC_REQUIRE(numClasses >= 1, "numClasses must be positive");
  if (fitWithMean)
    CYC_REQUIRE(fitIntercept, "for training without intercept, should not center the vectors");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    cyc::set_error("no HIP device visible");
    return CYC_ERR_NO_DEVICE;
  }
  auto* p = new cyc_logistic_plan_s();
  p->F = numFeatures;
  p->C = numClasses;
  p->fitIntercept = fitIntercept != 0;
  p->fitWithMean = fitWithMean != 0;
  *plan = p;
  return CYC_OK;
}

int cyc_logistic_plan_destroy(cyc_logistic_plan plan) {
  delete plan;
  return CYC_OK;
}

int cyc_hinge_plan_create(int32_t numFeatures, int fitIntercept, cyc_logistic_plan* plan) {
  // HingeBlockAggregator centers whenever it fits an intercept (:62-72, :133-141)
  int rc = cyc_logistic_plan_create(numFeatures, 1, fitIntercept, fitIntercept, plan);
  if (rc == CYC_OK) (*plan)->loss = cyc::kHinge;
  return rc;
}

int cyc_huber_plan_create(int32_t numFeatures, int fitIntercept, double epsilon,
                          cyc_logistic_plan* plan) {
  CYC_REQUIRE(epsilon > 1.0, "epsilon must be > 1.0");
  // centers whenever it fits an intercept (marginOffset :66-71, daxpy :131-134)
  int rc = cyc_logistic_plan_create(numFeatures, 1, fitIntercept, fitIntercept, plan);
  if (rc == CYC_OK) {
    (*plan)->loss = cyc::kHuber;
    (*plan)->epsilon = epsilon;
  }
  return rc;
}

int cyc_aft_plan_create(int32_t numFeatures, int fitIntercept, cyc_logistic_plan* plan) {
  // centers whenever it fits an intercept (marginOffset :52-58, daxpy :118-121)
  int rc = cyc_logistic_plan_create(numFeatures, 1, fitIntercept, fitIntercept, plan);
  if (rc == CYC_OK) (*plan)->loss = cyc::kAft;
  return rc;
}

int cyc_least_squares_plan_create(int32_t numFeatures, int fitIntercept, double labelStd,
                                  double labelMean, cyc_logistic_plan* plan) {
  CYC_REQUIRE(labelStd > 0.0, "LeastSquaresBlockAggregator requires the label standard "
                              "deviation to be positive.");
  int rc = cyc_logistic_plan_create(numFeatures, 1, fitIntercept, 0, plan);
  if (rc == CYC_OK) {
    (*plan)->loss = cyc::kLeastSquares;
    (*plan)->labelStd = labelStd;
    (*plan)->labelMean = labelMean;
  }
  return rc;
}

}  // extern "C"
