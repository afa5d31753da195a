// decision_tree.hip -- DecisionTree on gfx950 (MI355X): the binned rows, the
// per-node histogram of one level, the routing of rows to the children, and the
// model's descent, for ml/tree/impl/RandomForest.scala's fit of one tree over
// dense fp64 rows with continuous features.  The split candidates, the split
// search over nodes x features x bins and the tree are host code
// (cycloneml_amd/tree.py).
//
// State.  The rows are binned once into a uint8 image (n x d): image[r][f] =
// the number of feature f's thresholds strictly below x[r][f] (TreePoint's
// Arrays.binarySearch).  Every row has an int32 slot, a compact id of the node
// it sits in; -1 is the skip slot of the parked rows (rows in leaves), which
// are never loaded again.  The host keeps the slot <-> node index map.
//
// Kernels
//   k_dt_check    the lowest row with a NaN feature (rule 1), a label that is
//                 no integer in [0, C) / is not finite (rule 2) or a weight that
//                 is not finite and >= 0 (rule 3): an integer atomicMin.
//   k_dt_bin      a workgroup takes kBinRows rows x kBinPanel features; the
//                 panel's thresholds sit in LDS (stride 255 doubles, odd: the
//                 16 lanes of a row hit 16 banks), 16 lanes read 128 contiguous
//                 bytes of a row and each finds its lower bound by bisection.
//   k_dt_route    newSlot from one byte of the image: bin <= splitBin goes
//                 left; a slot whose table entry is parked, and a slot outside
//                 the table, get the skip slot.
//   k_dt_key      the node (0 .. K - 1) a row's slot maps to in this call, K
//                 for every other row: the key of kmeans_sums.hpp's stable
//                 sort_clusters (cluster K is skipped).
//   k_dt_runs     runStart: a node's rows, in row order, are cut into runs of
//                 kRunRows rows.
//   k_dt_hist     a workgroup is one wave: one run x kLanes features x one
//                 window of kWindow accumulators.  A lane owns a feature; its
//                 accumulators acc[slot][lane] sit in LDS (a double per lane per
//                 slot: lane l is at bank 2 l whatever bin it hits, so the
//                 byte-indexed update never conflicts).  The accumulators of a
//                 feature are the flat index stat * bins + bin; when stats x
//                 bins is above kWindow the windows are passes (blockIdx.z).
//                 The run's rows are gathered through the permutation in row
//                 order, d contiguous bytes each, 8 rows' loads in flight.  The
//                 window goes to the workspace as part[run][flat][feature].
//   k_dt_fold     per node, the runs in order onto the histogram (zero at the
//                 start of the call), written as node x feature x bin x stat.
//                 The workspace holds a group of runs: a smaller one means more
//                 launches of the pair and the same chain, so the same bits.
//   k_dt_predict  a thread per row walks the tree (x[f] <= threshold goes to
//                 firstChild, else firstChild + 1) and writes the leaf index
//                 and, on request, the leaf's prediction, raw vector and
//                 probability.
// No atomics on doubles, every sum has one fixed order: two calls on the same
// inputs give the same bits.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <mutex>
#include <string>
#include <vector>

#include "common.hpp"
#include "decision_tree.hpp"
#include "kmeans_sums.hpp"

using namespace cyc::dt;

enum { DT_RULE_NONE = 0, DT_RULE_FEATURE = 1, DT_RULE_LABEL = 2, DT_RULE_WEIGHT = 3 };

struct cyc_dt_plan_s {
  std::mutex mu;
  int d = 0, C = 0;   // C = 0: variance
  int64_t wsBytes = 0;
  cyc::kmsums::SortScratch sort;
  cyc::DeviceBuffer table, key, ws, bad, runStart, thr, cnt, tree, leaf;
};

namespace {

// the bounds shared with random_forest.hip: decision_tree.hpp
constexpr int kBinPanel = 16;               // features whose thresholds are staged together
constexpr int kBinRows = 4096;              // rows per k_dt_bin workgroup
constexpr unsigned long long kNoBad = ~0ull;

__device__ __forceinline__ void dt_flag(unsigned long long* bad, int64_t row, int rule) {
  atomicMin(bad, (unsigned long long)row * 4ull + (unsigned long long)rule);
}

__global__ __launch_bounds__(256) void k_dt_check(const double* __restrict__ X,
                                                  const double* __restrict__ y,
                                                  const double* __restrict__ w, int64_t n, int d,
                                                  int C, unsigned long long* __restrict__ bad) {
  const int64_t stride = (int64_t)gridDim.x * 256, t0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  for (int64_t e = t0; e < n * d; e += stride) {
    const double x = X[e];
    if (x != x) dt_flag(bad, e / d, DT_RULE_FEATURE);
  }
  for (int64_t r = t0; r < n; r += stride) {
    const double yv = y[r];
    if (C ? dt_label(yv, C) < 0 : !(yv - yv == 0.0)) dt_flag(bad, r, DT_RULE_LABEL);
    if (w) {
      const double wv = w[r];
      if (!(wv >= 0.0 && wv - wv == 0.0)) dt_flag(bad, r, DT_RULE_WEIGHT);
    }
  }
}

// image[r][f] = #{s < cnt[f] : thr[f][s] < x[r][f]}
__global__ __launch_bounds__(256) void k_dt_bin(const double* __restrict__ X, int64_t n, int d,
                                                const double* __restrict__ thr,
                                                const int32_t* __restrict__ cnt,
                                                uint8_t* __restrict__ image) {
  __shared__ double thrS[kBinPanel * kMaxSplits];
  __shared__ int cntS[kBinPanel];
  const int tid = threadIdx.x, f0 = blockIdx.y * kBinPanel;
  const int pf = min(kBinPanel, d - f0);
  if (tid < kBinPanel) cntS[tid] = tid < pf ? min(max(cnt[f0 + tid], 0), kMaxSplits) : 0;
  for (int i = tid; i < pf * kMaxSplits; i += 256) thrS[i] = thr[(int64_t)f0 * kMaxSplits + i];
  __syncthreads();
  const int lf = tid % kBinPanel, f = f0 + lf;
  if (lf >= pf) return;
  const int64_t r0 = (int64_t)blockIdx.x * kBinRows, r1 = min<int64_t>(n, r0 + kBinRows);
  const double* t = thrS + lf * kMaxSplits;
  const int c = cntS[lf];
  for (int64_t r = r0 + tid / kBinPanel; r < r1; r += 256 / kBinPanel) {
    const double x = __builtin_nontemporal_load(&X[r * d + f]);
    int lo = 0, hi = c;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (t[mid] < x) lo = mid + 1; else hi = mid;
    }
    image[r * d + f] = (uint8_t)lo;
  }
}

// table: (feature, splitBin, leftNew, rightNew) per slot, feature < 0: parked
__global__ __launch_bounds__(256) void k_dt_route(const uint8_t* __restrict__ image, int64_t n,
                                                  int d, int numSlots,
                                                  const int32_t* __restrict__ table,
                                                  int32_t* __restrict__ slot) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  const int s = slot[r];
  int out = -1;
  if ((unsigned)s < (unsigned)numSlots) {
    const int f = table[4 * s];
    if (f >= 0) out = (int)image[r * d + f] <= table[4 * s + 1] ? table[4 * s + 2] : table[4 * s + 3];
  }
  if (out != s) slot[r] = out;
}

// slot: null = every row in slot 0
__global__ __launch_bounds__(256) void k_dt_key(const int32_t* __restrict__ slot, int64_t n,
                                                int numSlots, const int32_t* __restrict__ nodeOf,
                                                int K, int32_t* __restrict__ key) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  const int s = slot ? slot[r] : 0;
  int k = K;
  if ((unsigned)s < (unsigned)numSlots) {
    const int c = nodeOf[s];
    if ((unsigned)c < (unsigned)K) k = c;
  }
  key[r] = k;
}

__global__ void k_dt_runs(const int64_t* __restrict__ cstart, int K, int64_t* __restrict__ runStart) {
  if (blockIdx.x || threadIdx.x) return;
  int64_t s = 0;
  for (int c = 0; c < K; ++c) {
    runStart[c] = s;
    s += (cstart[c + 1] - cstart[c] + kRunRows - 1) / kRunRows;
  }
  runStart[K] = s;
}

// Run g0 + blockIdx.x, features blockIdx.y kLanes .., accumulators a0 = blockIdx.z
// kWindow .. of the flat index stat B + bin, into part[blockIdx.x][flat][feature].
// C > 0: stat label += w, stat C += 1.  C == 0: w, w y, (w y) y, 1.
__global__ __launch_bounds__(kLanes) void k_dt_hist(
    const uint8_t* __restrict__ image, int d, const double* __restrict__ y,
    const double* __restrict__ w, const int32_t* __restrict__ perm,
    const int64_t* __restrict__ cstart, const int64_t* __restrict__ runStart, int K, int64_t g0,
    int B, int C, double* __restrict__ part) {
  __shared__ double acc[kWindow][kLanes];
  const int64_t run = g0 + blockIdx.x;
  if (run >= runStart[K]) return;
  int lo = 0, hi = K;   // the node: the last c with runStart[c] <= run
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (runStart[mid] <= run) lo = mid; else hi = mid;
  }
  const int c = lo;
  const int64_t first = cstart[c] + (run - runStart[c]) * kRunRows;
  const int cnt = (int)(min<int64_t>(cstart[c + 1], first + kRunRows) - first);
  const int lane = threadIdx.x, f = blockIdx.y * kLanes + lane;
  const int S = C ? C + 1 : 4, flats = S * B;
  const int a0 = blockIdx.z * kWindow;
#pragma unroll 8
  for (int a = 0; a < kWindow; ++a) acc[a][lane] = 0.0;
  if (f < d) {
    for (int p0 = 0; p0 < cnt; p0 += 8) {
      int bin[8];
      double yv[8], wv[8];
      // the loads of 8 rows before their adds
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int64_t r = perm[first + min(p0 + u, cnt - 1)];
        bin[u] = image[r * d + f];
        yv[u] = y[r];
        wv[u] = w ? w[r] : 1.0;
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        // a byte outside the bins is never an index
        if (p0 + u >= cnt || bin[u] >= B) continue;
        if (C) {
          const int lb = dt_label(yv[u], C);
          const int a = lb * B + bin[u] - a0, b = C * B + bin[u] - a0;
          if (lb >= 0 && (unsigned)a < (unsigned)kWindow) acc[a][lane] = dadd(acc[a][lane], wv[u]);
          if ((unsigned)b < (unsigned)kWindow) acc[b][lane] = dadd(acc[b][lane], 1.0);
        } else {
          const double wy = dmul(wv[u], yv[u]);
          const double v[4] = {wv[u], wy, dmul(wy, yv[u]), 1.0};
#pragma unroll
          for (int s = 0; s < 4; ++s) {
            const int a = s * B + bin[u] - a0;
            if ((unsigned)a < (unsigned)kWindow) acc[a][lane] = dadd(acc[a][lane], v[s]);
          }
        }
      }
    }
    double* out = part + (int64_t)blockIdx.x * flats * d;
    for (int a = 0; a < kWindow && a0 + a < flats; ++a) out[(int64_t)(a0 + a) * d + f] = acc[a][lane];
  }
}

// hist[c] (d x B x S) += node c's runs of the group [g0, g0 + group), in order
__global__ __launch_bounds__(256) void k_dt_fold(const double* __restrict__ part,
                                                 const int64_t* __restrict__ runStart, int d,
                                                 int B, int S, int64_t g0, int64_t group,
                                                 double* __restrict__ hist) {
  const int c = blockIdx.x;
  const int64_t len = (int64_t)S * B * d;
  const int64_t a = max<int64_t>(runStart[c], g0), b = min<int64_t>(runStart[c + 1], g0 + group);
  if (a >= b) return;
  for (int64_t e = (int64_t)blockIdx.y * 256 + threadIdx.x; e < len; e += (int64_t)gridDim.y * 256) {
    const int f = (int)(e % d), flat = (int)(e / d);
    const int s = flat / B, bin = flat % B;
    double* dst = hist + (int64_t)c * len + ((int64_t)f * B + bin) * S + s;
    double v = *dst;
    for (int64_t run = a; run < b; ++run) v = dadd(v, part[(run - g0) * len + e]);
    *dst = v;
  }
}

// tree (int32): [feature | firstChild | leafIndex], numNodes each; thr: numNodes
__global__ __launch_bounds__(256) void k_dt_predict(
    const double* __restrict__ X, int64_t n, int d, int numNodes, const int32_t* __restrict__ tree,
    const double* __restrict__ thr, int C, const double* __restrict__ leafPred,
    const double* __restrict__ leafRaw, int32_t* __restrict__ leaf, double* __restrict__ pred,
    double* __restrict__ raw, double* __restrict__ prob) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  const int32_t* feature = tree;
  const int32_t* firstChild = tree + numNodes;
  const int32_t* leafIndex = tree + 2 * (int64_t)numNodes;
  int node = 0;
  // a child's index is above its parent's (checked by the host): it ends
  for (;;) {
    const int fc = firstChild[node];
    if (fc < 0) break;
    const double x = X[r * d + feature[node]];
    node = x <= thr[node] ? fc : fc + 1;
  }
  const int li = leafIndex[node];
  if (leaf) leaf[r] = li;
  if (pred) pred[r] = leafPred[li];
  if (raw)
    for (int c = 0; c < C; ++c) raw[r * C + c] = leafRaw[(int64_t)li * C + c];
  if (prob) {
    double s = 0.0;
    for (int c = 0; c < C; ++c) s = dadd(s, leafRaw[(int64_t)li * C + c]);
    for (int c = 0; c < C; ++c) {
      const double v = leafRaw[(int64_t)li * C + c];
      prob[r * C + c] = s != 0.0 ? v / s : v;
    }
  }
}

int reset_bad(cyc_dt_plan_s* p, hipStream_t st) {
  if (int rc = p->bad.reserve(sizeof(unsigned long long))) return rc;
  CYC_HIP(hipMemsetAsync(p->bad.ptr, 0xff, sizeof(unsigned long long), st));
  return CYC_OK;
}

int64_t runs_per_launch(const cyc_dt_plan_s* p, int B) {
  return std::max<int64_t>(1, p->wsBytes / (8 * (int64_t)num_stats(p->C) * B * p->d));
}

}  // namespace

extern "C" {

int cyc_dt_plan_create(int32_t numFeatures, int32_t numClasses, int64_t workspaceBytes,
                       cyc_dt_plan* plan) {
  CYC_REQUIRE(plan != nullptr, "plan must not be null");
  CYC_REQUIRE(numFeatures >= 1 && numFeatures <= kMaxFeatures,
              "DecisionTree supports 1 to " + std::to_string(kMaxFeatures) +
                  " features but got " + std::to_string(numFeatures));
  CYC_REQUIRE(numClasses >= 0 && numClasses <= kMaxClasses,
              "DecisionTree supports 1 to " + std::to_string(kMaxClasses) +
                  " classes (0: regression) but got " + std::to_string(numClasses));
  CYC_REQUIRE(workspaceBytes >= 0, "workspaceBytes must not be negative");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    cyc::set_error("no HIP device visible");
    return CYC_ERR_NO_DEVICE;
  }
  auto* p = new cyc_dt_plan_s();
  p->d = numFeatures;
  p->C = numClasses;
  p->wsBytes = workspaceBytes ? workspaceBytes : kDefaultWorkspace;
  *plan = p;
  return CYC_OK;
}

int cyc_dt_plan_destroy(cyc_dt_plan plan) {
  delete plan;
  return CYC_OK;
}

int64_t cyc_dt_max_features(void) { return kMaxFeatures; }
int64_t cyc_dt_max_nodes(void) { return kMaxNodes; }
int64_t cyc_dt_run_rows(void) { return kRunRows; }
int64_t cyc_dt_num_stats(cyc_dt_plan plan) { return plan ? num_stats(plan->C) : -1; }
int64_t cyc_dt_runs_per_launch(cyc_dt_plan plan, int32_t numBins) {
  return plan && numBins >= 1 && numBins <= kMaxBins ? runs_per_launch(plan, numBins) : -1;
}

int cyc_dt_check_dev(cyc_dt_plan plan, const double* X, const double* y, const double* w,
                     int64_t nrows, int64_t* badRow, int32_t* badRule, void* stream) {
  CYC_REQUIRE(plan != nullptr, "plan must not be null");
  CYC_REQUIRE(nrows >= 0 && nrows <= INT32_MAX, "0 <= nrows <= 2147483647");
  if (badRow) *badRow = -1;
  if (badRule) *badRule = DT_RULE_NONE;
  if (nrows == 0) return CYC_OK;
  CYC_REQUIRE(X != nullptr && y != nullptr, "non-null rows and labels");
  cyc_dt_plan_s* p = plan;
  hipStream_t st = cyc::as_stream(stream);
  std::lock_guard<std::mutex> g(p->mu);
  if (int rc = reset_bad(p, st)) return rc;
  {
    cyc::KernelTimer timer("k_dt_check", st);
    hipLaunchKernelGGL(k_dt_check,
                       dim3((unsigned)std::min<int64_t>((nrows * p->d + 255) / 256, 8192)),
                       dim3(256), 0, st, X, y, w, nrows, p->d, p->C,
                       (unsigned long long*)p->bad.ptr);
    CYC_LAUNCH_CHECK("k_dt_check");
  }
  unsigned long long v = 0;
  CYC_HIP(hipMemcpyAsync(&v, p->bad.ptr, sizeof(v), hipMemcpyDeviceToHost, st));
  CYC_HIP(hipStreamSynchronize(st));
  if (v == kNoBad) return CYC_OK;
  const int64_t row = (int64_t)(v >> 2);
  const int rule = (int)(v & 3);
  if (badRow) *badRow = row;
  if (badRule) *badRule = rule;
  const std::string at = " (row " + std::to_string(row) + ")";
  double x = 0.0;
  if (rule == DT_RULE_FEATURE) {
    cyc::set_error("requirement failed: DecisionTree requires feature values that are not NaN." +
                   at);
  } else if (rule == DT_RULE_LABEL) {
    CYC_HIP(hipMemcpy(&x, y + row, sizeof(x), hipMemcpyDeviceToHost));
    cyc::set_error(p->C ? "requirement failed: Classification labels should be integers in [0 to " +
                              std::to_string(p->C - 1) + "]. Found " + cyc::java_double(x) + "." +
                              at
                        : "requirement failed: Regression labels must be finite but got " +
                              cyc::java_double(x) + "." + at);
  } else {
    CYC_HIP(hipMemcpy(&x, w + row, sizeof(x), hipMemcpyDeviceToHost));
    cyc::set_error("requirement failed: illegal weight value: " + cyc::java_double(x) +
                   ". weight must be finite and >= 0.0." + at);
  }
  return CYC_ERR_INVALID_ARG;
}

int cyc_dt_bin_dev(cyc_dt_plan plan, const double* X, int64_t nrows, const double* thresholds,
                   const int32_t* numSplits, uint8_t* image, void* stream) {
  CYC_REQUIRE(plan != nullptr, "plan must not be null");
  CYC_REQUIRE(nrows >= 0 && nrows <= INT32_MAX, "0 <= nrows <= 2147483647");
  CYC_REQUIRE(thresholds != nullptr && numSplits != nullptr, "non-null thresholds and numSplits");
  cyc_dt_plan_s* p = plan;
  for (int f = 0; f < p->d; ++f)
    CYC_REQUIRE(numSplits[f] >= 0 && numSplits[f] <= kMaxSplits,
                "feature " + std::to_string(f) + " must have 0 to " + std::to_string(kMaxSplits) +
                    " splits but got " + std::to_string(numSplits[f]));
  if (nrows == 0) return CYC_OK;
  CYC_REQUIRE(X != nullptr && image != nullptr, "non-null rows and image");
  hipStream_t st = cyc::as_stream(stream);
  std::lock_guard<std::mutex> g(p->mu);
  const size_t tb = sizeof(double) * (size_t)p->d * kMaxSplits, cb = sizeof(int32_t) * (size_t)p->d;
  if (int rc = p->thr.reserve(tb)) return rc;
  if (int rc = p->cnt.reserve(cb)) return rc;
  // stream-ordered after the last call's kernels; the sources are pageable, so
  // the copies have left the caller's arrays when the call returns
  CYC_HIP(hipMemcpyAsync(p->thr.ptr, thresholds, tb, hipMemcpyHostToDevice, st));
  CYC_HIP(hipMemcpyAsync(p->cnt.ptr, numSplits, cb, hipMemcpyHostToDevice, st));
  cyc::KernelTimer timer("k_dt_bin", st);
  hipLaunchKernelGGL(k_dt_bin,
                     dim3((unsigned)((nrows + kBinRows - 1) / kBinRows),
                          (unsigned)((p->d + kBinPanel - 1) / kBinPanel)),
                     dim3(256), 0, st, X, nrows, p->d, (const double*)p->thr.ptr,
                     (const int32_t*)p->cnt.ptr, image);
  CYC_LAUNCH_CHECK("k_dt_bin");
  return CYC_OK;
}

int cyc_dt_route_dev(cyc_dt_plan plan, const uint8_t* image, int64_t nrows, int32_t* slot,
                     int32_t numSlots, const int32_t* table, void* stream) {
  CYC_REQUIRE(plan != nullptr, "plan must not be null");
  CYC_REQUIRE(nrows >= 0 && nrows <= INT32_MAX, "0 <= nrows <= 2147483647");
  CYC_REQUIRE(numSlots >= 1 && table != nullptr, "a table of at least one slot");
  cyc_dt_plan_s* p = plan;
  for (int s = 0; s < numSlots; ++s) {
    const int32_t f = table[4 * s], b = table[4 * s + 1];
    if (f < 0) continue;
    CYC_REQUIRE(f < p->d && b >= 0 && b < kMaxSplits,
                "slot " + std::to_string(s) + " must split a feature in [0, " +
                    std::to_string(p->d) + ") at a bin in [0, " + std::to_string(kMaxSplits) +
                    ")");
    CYC_REQUIRE(table[4 * s + 2] >= -1 && table[4 * s + 3] >= -1,
                "the new slots of slot " + std::to_string(s) + " must be -1 or a slot");
  }
  if (nrows == 0) return CYC_OK;
  CYC_REQUIRE(image != nullptr && slot != nullptr, "non-null image and slot");
  hipStream_t st = cyc::as_stream(stream);
  std::lock_guard<std::mutex> g(p->mu);
  const size_t tb = sizeof(int32_t) * 4 * (size_t)numSlots;
  if (int rc = p->table.reserve(tb)) return rc;
  CYC_HIP(hipMemcpyAsync(p->table.ptr, table, tb, hipMemcpyHostToDevice, st));
  cyc::KernelTimer timer("k_dt_route", st);
  hipLaunchKernelGGL(k_dt_route, dim3((unsigned)((nrows + 255) / 256)), dim3(256), 0, st, image,
                     nrows, p->d, numSlots, (const int32_t*)p->table.ptr, slot);
  CYC_LAUNCH_CHECK("k_dt_route");
  return CYC_OK;
}

int cyc_dt_histogram_dev(cyc_dt_plan plan, const uint8_t* image, const double* y, const double* w,
                         int64_t nrows, const int32_t* slot, int32_t numSlots,
                         const int32_t* nodeOf, int32_t numNodes, int32_t numBins, double* hist,
                         void* stream) {
  CYC_REQUIRE(plan != nullptr, "plan must not be null");
  CYC_REQUIRE(nrows >= 0 && nrows <= INT32_MAX, "0 <= nrows <= 2147483647");
  CYC_REQUIRE(numSlots >= 1 && nodeOf != nullptr, "a node per slot, at least one slot");
  CYC_REQUIRE(numNodes >= 1 && numNodes <= kMaxNodes,
              "1 to " + std::to_string(kMaxNodes) + " nodes but got " + std::to_string(numNodes));
  CYC_REQUIRE(numBins >= 1 && numBins <= kMaxBins,
              "1 to " + std::to_string(kMaxBins) + " bins but got " + std::to_string(numBins));
  CYC_REQUIRE(hist != nullptr, "hist must not be null");
  for (int s = 0; s < numSlots; ++s)
    CYC_REQUIRE(nodeOf[s] >= -1 && nodeOf[s] < numNodes,
                "the node of slot " + std::to_string(s) + " must be -1 or in [0, " +
                    std::to_string(numNodes) + ")");
  cyc_dt_plan_s* p = plan;
  const int d = p->d, K = numNodes, B = numBins, S = num_stats(p->C);
  const int64_t len = (int64_t)S * B * d;
  hipStream_t st = cyc::as_stream(stream);
  std::lock_guard<std::mutex> g(p->mu);
  CYC_HIP(hipMemsetAsync(hist, 0, sizeof(double) * (size_t)(K * len), st));
  if (nrows == 0) return CYC_OK;
  CYC_REQUIRE(image != nullptr && y != nullptr, "non-null image and labels");
  if (int rc = p->table.reserve(sizeof(int32_t) * (size_t)numSlots)) return rc;
  CYC_HIP(hipMemcpyAsync(p->table.ptr, nodeOf, sizeof(int32_t) * (size_t)numSlots,
                         hipMemcpyHostToDevice, st));
  if (int rc = p->key.reserve(sizeof(int32_t) * (size_t)nrows)) return rc;
  if (int rc = p->runStart.reserve(sizeof(int64_t) * (size_t)(K + 1))) return rc;
  int32_t* key = (int32_t*)p->key.ptr;
  {
    cyc::KernelTimer timer("k_dt_key", st);
    hipLaunchKernelGGL(k_dt_key, dim3((unsigned)((nrows + 255) / 256)), dim3(256), 0, st, slot,
                       nrows, numSlots, (const int32_t*)p->table.ptr, K, key);
    CYC_LAUNCH_CHECK("k_dt_key");
  }
  int64_t maxChunks = 0;
  // d = 0: the sort's own chunk buffers are not used here
  if (int rc = cyc::kmsums::sort_clusters(p->sort, key, nrows, 0, K + 1, st, maxChunks)) return rc;
  const int32_t* perm = (const int32_t*)p->sort.perm.ptr;
  const int64_t* cstart = (const int64_t*)p->sort.cstart.ptr;
  int64_t* runStart = (int64_t*)p->runStart.ptr;
  hipLaunchKernelGGL(k_dt_runs, dim3(1), dim3(64), 0, st, cstart, K, runStart);
  CYC_LAUNCH_CHECK("k_dt_runs");
  // the run count is on the device: the bound is launched, the surplus leaves
  const int64_t maxRuns = nrows / kRunRows + K;
  const int64_t group = std::min(maxRuns, runs_per_launch(p, B));
  if (int rc = p->ws.reserve(sizeof(double) * (size_t)(group * len))) return rc;
  const unsigned panels = (unsigned)((d + kLanes - 1) / kLanes);
  const unsigned passes = (unsigned)((S * B + kWindow - 1) / kWindow);
  const unsigned foldBlocks = (unsigned)std::min<int64_t>((len + 255) / 256, 1024);
  for (int64_t g0 = 0; g0 < maxRuns; g0 += group) {
    const int64_t gc = std::min(group, maxRuns - g0);
    {
      cyc::KernelTimer timer("k_dt_hist", st);
      hipLaunchKernelGGL(k_dt_hist, dim3((unsigned)gc, panels, passes), dim3(kLanes), 0, st, image,
                         d, y, w, perm, cstart, (const int64_t*)runStart, K, g0, B, p->C,
                         (double*)p->ws.ptr);
      CYC_LAUNCH_CHECK("k_dt_hist");
    }
    cyc::KernelTimer timer("k_dt_fold", st);
    hipLaunchKernelGGL(k_dt_fold, dim3((unsigned)K, foldBlocks), dim3(256), 0, st,
                       (const double*)p->ws.ptr, (const int64_t*)runStart, d, B, S, g0, gc, hist);
    CYC_LAUNCH_CHECK("k_dt_fold");
  }
  return CYC_OK;
}

int cyc_dt_predict_dev(cyc_dt_plan plan, const double* X, int64_t nrows, int32_t numNodes,
                       const int32_t* feature, const double* threshold, const int32_t* firstChild,
                       const int32_t* leafIndex, int32_t numLeaves, const double* leafPred,
                       const double* leafRaw, int32_t* leaf, double* pred, double* raw,
                       double* prob, void* stream) {
  CYC_REQUIRE(plan != nullptr, "plan must not be null");
  CYC_REQUIRE(nrows >= 0, "nrows >= 0");
  CYC_REQUIRE(numNodes >= 1 && numNodes <= kMaxTreeNodes,
              "1 to " + std::to_string(kMaxTreeNodes) + " nodes but got " +
                  std::to_string(numNodes));
  CYC_REQUIRE(feature != nullptr && threshold != nullptr && firstChild != nullptr &&
                  leafIndex != nullptr,
              "non-null node arrays");
  cyc_dt_plan_s* p = plan;
  CYC_REQUIRE(numLeaves >= 1 && numLeaves <= numNodes, "1 to numNodes leaves");
  for (int i = 0; i < numNodes; ++i) {
    const int32_t fc = firstChild[i];
    if (fc >= 0) {
      CYC_REQUIRE(fc > i && (int64_t)fc + 2 <= numNodes,
                  "the children of node " + std::to_string(i) +
                      " must follow it and lie inside the tree");
      CYC_REQUIRE(feature[i] >= 0 && feature[i] < p->d,
                  "node " + std::to_string(i) + " must split a feature in [0, " +
                      std::to_string(p->d) + ")");
    } else {
      CYC_REQUIRE(leafIndex[i] >= 0 && leafIndex[i] < numLeaves,
                  "leaf node " + std::to_string(i) + " needs a leaf index in [0, " +
                      std::to_string(numLeaves) + ")");
    }
  }
  CYC_REQUIRE((raw == nullptr && prob == nullptr) || (p->C > 0 && leafRaw != nullptr),
              "raw and prob need a classifier's plan and leafRaw");
  CYC_REQUIRE(pred == nullptr || leafPred != nullptr, "pred needs leafPred");
  if (nrows == 0) return CYC_OK;
  CYC_REQUIRE(X != nullptr, "rows must not be null");
  hipStream_t st = cyc::as_stream(stream);
  std::lock_guard<std::mutex> g(p->mu);
  const size_t nb = sizeof(int32_t) * (size_t)numNodes, tb = sizeof(double) * (size_t)numNodes;
  const size_t pb = sizeof(double) * (size_t)numLeaves, rb = pb * (size_t)std::max(p->C, 1);
  if (int rc = p->tree.reserve(3 * nb)) return rc;
  if (int rc = p->thr.reserve(tb)) return rc;
  if (int rc = p->leaf.reserve(pb + rb)) return rc;
  char* nd = (char*)p->tree.ptr;
  char* lf = (char*)p->leaf.ptr;
  CYC_HIP(hipMemcpyAsync(nd, feature, nb, hipMemcpyHostToDevice, st));
  CYC_HIP(hipMemcpyAsync(nd + nb, firstChild, nb, hipMemcpyHostToDevice, st));
  CYC_HIP(hipMemcpyAsync(nd + 2 * nb, leafIndex, nb, hipMemcpyHostToDevice, st));
  CYC_HIP(hipMemcpyAsync(p->thr.ptr, threshold, tb, hipMemcpyHostToDevice, st));
  if (leafPred) CYC_HIP(hipMemcpyAsync(lf, leafPred, pb, hipMemcpyHostToDevice, st));
  if (leafRaw) CYC_HIP(hipMemcpyAsync(lf + pb, leafRaw, rb, hipMemcpyHostToDevice, st));
  cyc::KernelTimer timer("k_dt_predict", st);
  hipLaunchKernelGGL(k_dt_predict, dim3((unsigned)((nrows + 255) / 256)), dim3(256), 0, st, X,
                     nrows, p->d, numNodes, (const int32_t*)p->tree.ptr, (const double*)p->thr.ptr,
                     p->C, leafPred ? (const double*)lf : nullptr,
                     leafRaw ? (const double*)(lf + pb) : nullptr, leaf, pred, raw, prob);
  CYC_LAUNCH_CHECK("k_dt_predict");
  return CYC_OK;
}

}  // extern "C"
