// decision_tree.hpp -- what decision_tree.hip and random_forest.hip share: the
// bounds of the binned image and of a histogram call, the number of statistics
// and the label rule.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

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

// the label of a row as a class index, or -1 (never an index)
__device__ __forceinline__ int dt_label(double y, int C) {
  if (!(y >= 0.0 && y < (double)C)) return -1;
  const int c = (int)y;
  return (double)c == y ? c : -1;
}

}  // namespace dt
}  // namespace cyc
