// kmeans_sums.hpp -- the per-cluster sums of a dense Lloyd call
// (kmeans_sums.hip): the stable counting sort of rows by cluster, the
// fixed-order chunk sums and folds, the incremental sums carried across the
// calls of one fit, and the center update.  Plain pointers and the two
// scratch structs below; no plan type here.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.hpp"

namespace cyc {
namespace kmsums {

constexpr int kChunkRows = 256;   // rows per deterministic partial sum
constexpr int kMaxK = 8192;       // LDS histogram bound for the sort

// Scratch of the sort and the chunk sums, owned by the plan: per-tile
// histograms, per-cluster totals, cluster and chunk offsets (k + 1 each),
// the row permutation, the chunks' partial sums / weights / costs, the
// per-cluster costs and the scan's segment sums; tickets: the arrival
// counters of the gated full pass (zero between calls).
struct SortScratch {
  DeviceBuffer hist, total, cstart, chunkStart, perm, part, pw, pc, ccost, segsum, tickets;
};

// Incremental cluster sums (k_inc_*; with the carried bounds, unit weights,
// no per-row costs), owned by the row image: the assignment the state refers
// to (prev), the per-cluster state S, P, W, Q, N, A, ES, EQ, and the scratch
// of the moved-row list and its sort by cluster.  cum: moved rows and calls
// that took the incremental path (two 64-bit counters).
struct IncState {
  bool enabled = true;   // cyc_kmeans_rows_set_incremental (CYC_KMEANS_INCR=0: off)
  bool valid = false;
  int k = 0;
  DeviceBuffer prev, tmpRow, tmpOld, bcount, count, gate, movedRow, movedNew, movedOld, S, P, W,
      Q, N, A, ES, EQ, cost, err, bad, tot, cum, pa, pds, psc;
};

// Counting sort of rows 0..n by assign[] into s.perm (stable: row order kept
// within a cluster), with cstart (k + 1 cluster offsets) and chunkStart
// (k + 1 offsets of kChunkRows-row chunks); part / pw / pc reserved for
// maxChunks chunks of d columns.  gate (optional, device): skipped when 0,
// and two launches instead of six.
int sort_clusters(SortScratch& s, const int32_t* assign, int64_t n, int d, int k, hipStream_t st,
                  int64_t& maxChunks, const int* gate = nullptr);

// The full pass: sort, chunk sums, the clusters' folds added into sums /
// wsum, the total cost added into cost_sum[0].  cost: per-row costs (null:
// computed by the chunk sums, d <= 1024; required beyond, and for cosine).
// cosine: sums of x / |x| with xnorm = |x|.  gate + inc (both or neither):
// the pass runs only when gate[0] != 0 and also resets inc's state from the
// clusters' sums (unit weights, no costs, d <= 1024; xnorm = |x|), in four
// launches that each end on a closed gate (nine ungated).
int full_pass(SortScratch& s, const double* X, int64_t n, int d, int k, const double* weights,
              const double* xnorm, bool cosine, const double* C, const int32_t* assign,
              double* cost, double* sums, double* wsum, double* cost_sum, hipStream_t st,
              const int* gate = nullptr, IncState* inc = nullptr);

// The Lloyd call's cluster sums, weights and cost through the incremental
// state or, when the device decides so, the full pass; both paths are
// enqueued and gated on the device (no host round trip).  The caller owns
// inc.valid / inc.k after the call's checks.
int inc_accumulate(SortScratch& s, IncState& inc, const double* X, const double* xnorm,
                   const int32_t* assign, int64_t n, int d, int k, const double* C, double* sums,
                   double* wsum, double* cost_sum, hipStream_t st);

// centroid = (1 / w) sum, its norm, and isCenterConverged (k_update_centers);
// the caller sets *converged = 1 first.
int update_centers(double* C, double* cnorm, const double* sums, const double* wsum, int k, int d,
                   double eps2, int32_t* converged, hipStream_t st);

}  // namespace kmsums
}  // namespace cyc
