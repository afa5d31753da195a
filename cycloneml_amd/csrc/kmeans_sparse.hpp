// kmeans_sparse.hpp -- KMeans over sparse (CSR) points (kmeans_sparse.hip):
// the row norms and the Euclidean assignment, and the fixed-order per-cluster
// sums shared by the Euclidean and cosine KMeans plans.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace cyc {
namespace kmsparse {

// Vectors.norm(sparse, 2) of n CSR rows (k_row_norms_csr).
int row_norms(const int64_t* rowptr, const double* vals, int64_t n, double* norms, hipStream_t st);

// EuclideanDistanceMeasure.findClosest for n CSR rows against dense centers
// (k_assign_sparse): with the statistics' prunes, or, stats == nullptr,
// findClosest(centers, point).  cost may be null.
int sparse_assign(const int64_t* rowptr, const int32_t* colidx, const double* vals,
                  const double* xnorm, int64_t n, int d, const double* C, const double* cnorm,
                  int k, const double* stats, int32_t* assign, double* cost, hipStream_t st);

// updateClusterSum over CSR rows (DistanceMeasure.scala:189-191 / :466-469):
// sums(assign[r]) += a_r x_r with a_r = w_r (xnorm == nullptr) or w_r / xnorm[r]
// (cosine); wsum(assign[r]) += w_r; costSum[0] += sum of w_r cost[r].  All
// accumulate; every group of adds is folded in a fixed order (bitwise
// reproducible).  w may be null (unit weights).
int cluster_sums(const int64_t* rowptr, const int32_t* colidx, const double* vals,
                 const double* w, const double* xnorm, int64_t n, int d, int k,
                 const int32_t* assign, const double* cost, double* sums, double* wsum,
                 double* costSum, hipStream_t st);

}  // namespace kmsparse
}  // namespace cyc
