// decision_tree.hpp -- what decision_tree.hip, random_forest.hip and gbt.hip
// share: the bounds of the binned image and of a histogram call, the number of
// statistics and the label rule; the device rules both families of kernels
// apply (the node of a slot, the route of a row, the run of a histogram
// workgroup, one row's statistics); and the host pieces that have one
// definition in decision_tree.hip: the checks of a plan, of a route table and
// of a tree a kernel may walk, and the driver of a histogram call.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <functional>
#include <string>

#include "common.hpp"
#include "kmeans_sums.hpp"

namespace cyc {
namespace dt {

constexpr int kMaxBins = 256;               // a bin is a byte
constexpr int kMaxSplits = kMaxBins - 1;    // thresholds per feature, the padded width
constexpr int kMaxClasses = 1024;
constexpr int kMaxFeatures = 65535 * 16;    // gridDim.y of k_dt_bin's panels
constexpr int kRunRows = 4096;              // rows per run of the histogram
constexpr int kLanes = 64;                  // lanes of a histogram workgroup (one wave)
constexpr int kWindow = 128;                // accumulators per lane: 64 KiB of LDS
constexpr int kMaxNodes = 4096;             // nodes per histogram call
constexpr int kMaxTreeNodes = 1 << 24;
constexpr int64_t kDefaultWorkspace = (int64_t)256 << 20;
static_assert(kMaxNodes + 1 <= cyc::kmsums::kMaxK, "nodes + the parked cluster are sorted");
static_assert(kWindow * kLanes * sizeof(double) <= 65536, "the accumulators fit a workgroup's LDS");

inline int num_stats(int C) { return C ? C + 1 : 4; }

// the runs whose partials (Q sub-runs of S B m doubles each) fit the workspace
inline int64_t runs_per_launch(int64_t wsBytes, int C, int m, int Q, int B) {
  return std::max<int64_t>(1, wsBytes / (8 * (int64_t)num_stats(C) * B * m * Q));
}

// the label of a row as a class index, or -1 (never an index)
__device__ __forceinline__ int dt_label(double y, int C) {
  if (!(y >= 0.0 && y < (double)C)) return -1;
  const int c = (int)y;
  return (double)c == y ? c : -1;
}

// the node 0 .. K - 1 slot s maps to in this call; K for a slot outside the
// table and for one whose node sits the call out
__device__ __forceinline__ int node_of_slot(int s, int numSlots,
                                            const int32_t* __restrict__ nodeOf, int K) {
  if ((unsigned)s < (unsigned)numSlots) {
    const int c = nodeOf[s];
    if ((unsigned)c < (unsigned)K) return c;
  }
  return K;
}

// the new slot of a row in slot s: its entry (feature, splitBin, leftNew,
// rightNew) sends the row's byte of the feature left when byte <= splitBin; a
// slot outside the table, and a parked one (feature < 0), give the skip slot
__device__ __forceinline__ int route_slot(int s, int numSlots, const int32_t* __restrict__ table,
                                          const uint8_t* __restrict__ row) {
  if ((unsigned)s >= (unsigned)numSlots) return -1;
  const int32_t* e = table + 4 * s;
  const int f = e[0];
  if (f < 0) return -1;
  return (int)row[f] <= e[1] ? e[2] : e[3];
}

// the node c of run `run` (the last c with runStart[c] <= run), the run's first
// entry of the permutation and its length
__device__ __forceinline__ void locate_run(int64_t run, const int64_t* __restrict__ runStart,
                                           const int64_t* __restrict__ cstart, int K, int& c,
                                           int64_t& first, int& cnt) {
  int lo = 0, hi = K;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (runStart[mid] <= run) lo = mid; else hi = mid;
  }
  c = lo;
  first = cstart[c] + (run - runStart[c]) * kRunRows;
  cnt = (int)(min<int64_t>(cstart[c + 1], first + kRunRows) - first);
}

// One row into its lane's accumulators acc[a kLanes + lane], a = stat B + bin -
// a0 when that lies in the window [0, W).  C > 0: stat label += iw, stat C +=
// cnt.  C == 0: iw, iw y, (iw y) y, cnt.  Each product rounded once.
__device__ __forceinline__ void add_row(double* acc, int lane, int bin, double y, double iw,
                                        double cnt, int a0, int W, int B, int C) {
  if (C) {
    const int lb = dt_label(y, C);
    // C B - a0 is uniform over the launch: written so that it is hoisted, which
    // keeps k_dt_hist's code what it was before the two kernels shared this
    const int a = lb * B + bin - a0, b = bin + (C * B - a0);
    if (lb >= 0 && (unsigned)a < (unsigned)W)
      acc[a * kLanes + lane] = dadd(acc[a * kLanes + lane], iw);
    if ((unsigned)b < (unsigned)W) acc[b * kLanes + lane] = dadd(acc[b * kLanes + lane], cnt);
  } else {
    const double wy = dmul(iw, y);
    const double v[4] = {iw, wy, dmul(wy, y), cnt};
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int a = s * B + bin - a0;
      if ((unsigned)a < (unsigned)W) acc[a * kLanes + lane] = dadd(acc[a * kLanes + lane], v[s]);
    }
  }
}

// ---- host, defined in decision_tree.hip.  Each returns CYC_OK or sets the error.

// 1 to kMaxFeatures features; `name` is the estimator's in the message
int check_features(const char* name, int32_t numFeatures);
// a HIP device is visible
int probe_device();
// what cyc_dt_plan_create and cyc_rf_plan_create ask of their arguments
int check_plan(const char* name, int32_t numFeatures, int32_t numClasses, int64_t workspaceBytes);

// a route table of numEntries x (feature, splitBin, leftNew, rightNew); `what`
// names an entry in the message ("slot", "slot entry")
int check_route_table(const int32_t* table, int numEntries, int d, const char* what);

// A tree a kernel may walk: the children of a node follow it and lie inside
// the nn nodes, and it splits a feature in [0, d); with splitBin at a bin in
// [0, kMaxSplits); with leafIndex a leaf's index is in [0, numLeaves).  ofTree
// follows the node in the message: "" or " of tree t".
int check_tree(int64_t nn, const int32_t* feature, const int32_t* firstChild,
               const int32_t* splitBin, const int32_t* leafIndex, int64_t numLeaves, int d,
               const std::string& ofTree);

// what a histogram call keeps between calls
struct HistScratch {
  cyc::kmsums::SortScratch sort;
  cyc::DeviceBuffer key, runStart, ws;
};

// the KernelTimer labels of the caller's launches
struct HistLabels {
  const char *runs, *hist, *fold;
};

// launches the caller's hist kernel over the runs [g0, g0 + gc) into scratch.ws
using HistLaunch = std::function<void(int64_t g0, int64_t gc, const int32_t* perm,
                                      const int64_t* cstart, const int64_t* runStart)>;

// The histogram of K nodes from scratch.key (one key 0 .. K per pair, K: not
// gathered): the stable sort by key, each node's pairs cut into runs of
// kRunRows, then per group of runs that fits wsBytes the caller's hist launch (Q
// partials of S B m doubles per run) and the fold of the partials, in (run,
// sub-run) order, onto hist (K x m x B x S, zeroed by the caller).
int histogram_runs(HistScratch& scratch, int64_t pairs, int K, int m, int Q, int B, int C,
                   int64_t wsBytes, double* hist, hipStream_t st, const HistLabels& labels,
                   const HistLaunch& launchHist);

}  // namespace dt
}  // namespace cyc
