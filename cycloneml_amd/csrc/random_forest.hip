// random_forest.hip -- RandomForest on gfx950 (MI355X): the bag (per tree and
// row sample counts), one level's per-node histograms of a range of trees over
// each node's feature subset, the routing of every tree's rows, and the descent
// of a row through all trees with the votes or the mean, for
// ml/tree/impl/RandomForest.scala's fit of numTrees trees over dense fp64 rows
// with continuous features.  The rows' checks, the binned image and the descent
// of one tree are decision_tree.hip's (cyc_dt_check_dev, cyc_dt_bin_dev,
// cyc_dt_predict_dev); the image is binned once and shared by all trees.  The
// split candidates, the feature subsets, the split search and the trees are host
// code (cycloneml_amd/forest.py).
//
// State.  bag: T x n uint8, tree-major, the number of times tree t drew row r
// (null: all ones).  slot: T x n int32, tree-major, the compact id of the node
// row r sits in in tree t; -1 is the skip slot of parked rows.  The host keeps
// the (tree, slot) <-> node map: per-tree tables are concatenated and addressed
// through slotStart (one offset per tree, and the total).
//
// Randomness.  rf_mix(seed, stream, tree, index) = fin(fin(fin(seed + G) +
// G (2 tree + stream + 1)) + G (index + 1)) in uint64 arithmetic, fin =
// splitmix64's finaliser, G = 0x9E3779B97F4A7C15.  The bag is stream 0 with index
// = the GLOBAL row; its top 53 bits u are compared with a host-made ascending
// table of floor(cdf_k 2^53): the count is the number of entries <= u (integer
// compares only).  forest.py restates the mix in numpy (and uses stream 1 for
// the feature subsets, which never reach the device as anything but lists).
//
// Kernels
//   k_rf_bag      a thread per (tree, row): bag[t][r].
//   k_rf_route    a thread per (tree, row): k_dt_route's rule through the tree's
//                 piece of the concatenated table.
//   k_rf_key      a thread per pair (t, r) of a tree range [t0, t1): the node 0 ..
//                 K - 1 the pair's slot maps to, K when the slot sits out or the
//                 row was drawn 0 times: such a row is never gathered.  The key of
//                 kmeans_sums.hpp's stable sort_clusters, so a node's pairs stay
//                 in row order (a node belongs to one tree).
//   k_rf_hist     a workgroup is one wave: one run of kRunRows pairs of a node x
//                 one panel of the node's feature subset x one window of kWindow
//                 accumulators per lane in LDS, as k_dt_hist.  A lane owns a
//                 SUBSET feature nodeFeat[c][j].  With m subset features the
//                 panel is P = min(m, 64) features wide and the wave's lanes are
//                 P features x Q = floor(64 / P) sub-runs (lane = q P + j): sub-run
//                 q is the fixed slice [q L, (q + 1) L), L = ceil(kRunRows / Q), of
//                 the run's pairs, summed in row order by its own lanes, so Q rows
//                 are in flight per step.  64 - Q P lanes (fewer than P) have no
//                 sub-run and idle: none when m divides 64 (m = 16: 4 x 16), 1 at
//                 m = 3 (21 x 3), 4 at m = 5 or 10, but 64 - m for m in 33 .. 63,
//                 where Q = 1 and the wave is k_dt_hist's (m = 33: 31 lanes idle),
//                 and above 64 the last panel idles 64 - m mod 64 lanes as the
//                 tree's does.  Cost: the LDS stays min(S B, kWindow) x 64 doubles
//                 per wave (it is sized by the launch: 48 KiB at 3 x 32
//                 accumulators, so three waves share a CU's LDS where k_dt_hist's
//                 fixed 64 KiB lets two), and a run leaves Q partials of S B m
//                 doubles, at most S B 64 per run for m <= 64, what a tree's run
//                 leaves at d = 64.  The row is perm - (t - t0) n with the tree
//                 known per node; per row the gather is image[r d + f], y[r], w[r]
//                 and bag[t][r].
//   k_rf_fold     per node, the partials in (run, sub-run) order onto hist (K x m
//                 x B x S), zero at the start of the call.  An empty sub-run adds
//                 +0.0, which changes no bit.  A smaller workspace means more
//                 launches and the same chain.
//   k_rf_predict  a thread per row walks every tree in order (the trees
//                 concatenated breadth first, flatten_tree's form, with per-tree
//                 node and leaf offsets), writes the leaf matrix and adds the
//                 leaf's uploaded vote vector counts / total (classifier, in the
//                 raw output: up to 1024 classes never sit in registers) or
//                 prediction (regressor); the one division of the probability and
//                 of the mean is done here.
// Statistics, each product rounded once, unfused: classifier stat[label] +=
// numSamples w, stat[C] += numSamples; regressor iw = numSamples w: iw, iw y,
// (iw y) y, numSamples.  No atomics on doubles, every sum has one fixed order:
// two calls give the same bytes for every workspace size, tree range and node
// grouping.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <string>
#include <vector>

#include "common.hpp"
#include "decision_tree.hpp"
#include "kmeans_sums.hpp"

using namespace cyc::dt;

struct cyc_rf_plan_s {
  std::mutex mu;
  int d = 0, C = 0;   // C = 0: variance
  int64_t wsBytes = 0;
  cyc::kmsums::SortScratch sort;
  cyc::DeviceBuffer meta, key, ws, runStart, bagTable, tree, thr, leaf;
  std::vector<int32_t> nodeTree;   // the tree of every node of the last histogram call
};

namespace {

constexpr int kMaxTrees = 4096;
constexpr int kMaxBagTable = 255;           // a count fits a byte
constexpr uint64_t kGolden = 0x9E3779B97F4A7C15ull;

__host__ __device__ __forceinline__ uint64_t rf_fin(uint64_t z) {
  z ^= z >> 30;
  z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27;
  z *= 0x94D049BB133111EBull;
  z ^= z >> 31;
  return z;
}

__host__ __device__ __forceinline__ uint64_t rf_mix(uint64_t seed, uint64_t stream, uint64_t tree,
                                                    uint64_t index) {
  const uint64_t h1 = rf_fin(rf_fin(seed + kGolden) + kGolden * (2ull * tree + stream + 1ull));
  return rf_fin(h1 + kGolden * (index + 1ull));
}

// the panel width of m subset features; a wave holds kLanes / panel_width sub-runs
inline int panel_width(int m) { return std::min(m, (int)kLanes); }

// bag[t][r] = #{k : table[k] <= top 53 bits of rf_mix(seed, 0, t, rowOffset + r)}
__global__ __launch_bounds__(256) void k_rf_bag(int64_t n, int64_t rowOffset, uint64_t seed,
                                                const uint64_t* __restrict__ table, int len,
                                                uint8_t* __restrict__ bag) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  const int t = blockIdx.y;
  const uint64_t u = rf_mix(seed, 0ull, (uint64_t)t, (uint64_t)(rowOffset + r)) >> 11;
  int c = 0;
  for (int k = 0; k < len; ++k) c += table[k] <= u ? 1 : 0;
  bag[(int64_t)t * n + r] = (uint8_t)c;
}

// table: (feature, splitBin, leftNew, rightNew) per slot of every tree, tree t's
// slots at slotStart[t] .. slotStart[t + 1]; feature < 0: parked
__global__ __launch_bounds__(256) void k_rf_route(const uint8_t* __restrict__ image, int64_t n,
                                                  int d, const int32_t* __restrict__ slotStart,
                                                  const int32_t* __restrict__ table,
                                                  int32_t* __restrict__ slot) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  const int t = blockIdx.y;
  const int s0 = slotStart[t], numSlots = slotStart[t + 1] - s0;
  const int64_t at = (int64_t)t * n + r;
  const int s = slot[at];
  int out = -1;
  if ((unsigned)s < (unsigned)numSlots) {
    const int32_t* e = table + 4 * (int64_t)(s0 + s);
    const int f = e[0];
    if (f >= 0) out = (int)image[r * d + f] <= e[1] ? e[2] : e[3];
  }
  if (out != s) slot[at] = out;
}

// slot, bag: at the range's first tree; slot null = every pair in slot 0, bag
// null = every row drawn once
__global__ __launch_bounds__(256) void k_rf_key(const int32_t* __restrict__ slot,
                                                const uint8_t* __restrict__ bag, int64_t n,
                                                const int32_t* __restrict__ slotStart,
                                                const int32_t* __restrict__ nodeOf, int K,
                                                int32_t* __restrict__ key) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  const int tl = blockIdx.y;
  const int64_t pair = (int64_t)tl * n + r;
  const int s0 = slotStart[tl], numSlots = slotStart[tl + 1] - s0;
  const int s = slot ? slot[pair] : 0;
  int k = K;
  if ((unsigned)s < (unsigned)numSlots && (!bag || bag[pair] != 0)) {
    const int c = nodeOf[s0 + s];
    if ((unsigned)c < (unsigned)K) k = c;
  }
  key[pair] = k;
}

__global__ void k_rf_runs(const int64_t* __restrict__ cstart, int K, int64_t* __restrict__ runStart) {
  if (blockIdx.x || threadIdx.x) return;
  int64_t s = 0;
  for (int c = 0; c < K; ++c) {
    runStart[c] = s;
    s += (cstart[c + 1] - cstart[c] + kRunRows - 1) / kRunRows;
  }
  runStart[K] = s;
}

// Run g0 + blockIdx.x, subset features blockIdx.y P .. (lane % P), sub-run lane /
// P, accumulators a0 = blockIdx.z kWindow .. of the flat index stat B + bin, into
// part[blockIdx.x][sub-run][flat][subset feature].  acc: W x 64 doubles, W =
// min(S B, kWindow).
__global__ __launch_bounds__(kLanes) void k_rf_hist(
    const uint8_t* __restrict__ image, int64_t n, int d, const double* __restrict__ y,
    const double* __restrict__ w, const uint8_t* __restrict__ bag,
    const int32_t* __restrict__ perm, const int64_t* __restrict__ cstart,
    const int64_t* __restrict__ runStart, int K, int64_t g0, int B, int C, int m, int P, int W,
    const int32_t* __restrict__ nodeTree, const int32_t* __restrict__ nodeFeat,
    double* __restrict__ part) {
  extern __shared__ double acc[];   // [W][kLanes]
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
  const int lane = threadIdx.x, Q = kLanes / P, sub = (kRunRows + Q - 1) / Q;
  const int q = lane / P, jf = blockIdx.y * P + lane % P;
  const int S = C ? C + 1 : 4, flats = S * B;
  const int a0 = blockIdx.z * kWindow;
  // the lanes past the last sub-run, and past the subset in the last panel, idle
  if (q >= Q || jf >= m) return;
  for (int a = 0; a < W; ++a) acc[a * kLanes + lane] = 0.0;
  const int f = nodeFeat ? nodeFeat[(int64_t)c * m + jf] : jf;
  const int64_t pair0 = (int64_t)nodeTree[c] * n;   // the pairs of the node's tree start here
  const uint8_t* bagT = bag ? bag + pair0 : nullptr;
  const int p1 = min(cnt, (q + 1) * sub);
  for (int p0 = q * sub; p0 < p1; p0 += 8) {
    int bin[8], ns[8];
    double yv[8], wv[8];
    // the loads of 8 rows before their adds
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int64_t r = (int64_t)perm[first + min(p0 + u, p1 - 1)] - pair0;
      bin[u] = image[r * d + f];
      yv[u] = y[r];
      wv[u] = w ? w[r] : 1.0;
      ns[u] = bagT ? (int)bagT[r] : 1;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      // a byte outside the bins is never an index
      if (p0 + u >= p1 || bin[u] >= B) continue;
      const double cntv = (double)ns[u];
      const double iw = dmul(cntv, wv[u]);
      if (C) {
        const int lb = dt_label(yv[u], C);
        const int a = lb * B + bin[u] - a0, b = C * B + bin[u] - a0;
        if (lb >= 0 && (unsigned)a < (unsigned)W)
          acc[a * kLanes + lane] = dadd(acc[a * kLanes + lane], iw);
        if ((unsigned)b < (unsigned)W) acc[b * kLanes + lane] = dadd(acc[b * kLanes + lane], cntv);
      } else {
        const double wy = dmul(iw, yv[u]);
        const double v[4] = {iw, wy, dmul(wy, yv[u]), cntv};
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const int a = s * B + bin[u] - a0;
          if ((unsigned)a < (unsigned)W) acc[a * kLanes + lane] = dadd(acc[a * kLanes + lane], v[s]);
        }
      }
    }
  }
  double* out = part + ((int64_t)blockIdx.x * Q + q) * flats * m;
  for (int a = 0; a < W && a0 + a < flats; ++a) out[(int64_t)(a0 + a) * m + jf] = acc[a * kLanes + lane];
}

// hist[c] (m x B x S) += node c's partials of the runs [g0, g0 + group), in (run,
// sub-run) order
__global__ __launch_bounds__(256) void k_rf_fold(const double* __restrict__ part,
                                                 const int64_t* __restrict__ runStart, int m,
                                                 int B, int S, int Q, int64_t g0, int64_t group,
                                                 double* __restrict__ hist) {
  const int c = blockIdx.x;
  const int64_t len = (int64_t)S * B * m;
  const int64_t a = max<int64_t>(runStart[c], g0), b = min<int64_t>(runStart[c + 1], g0 + group);
  if (a >= b) return;
  for (int64_t e = (int64_t)blockIdx.y * 256 + threadIdx.x; e < len; e += (int64_t)gridDim.y * 256) {
    const int jf = (int)(e % m), flat = (int)(e / m);
    const int s = flat / B, bin = flat % B;
    double* dst = hist + (int64_t)c * len + ((int64_t)jf * B + bin) * S + s;
    double v = *dst;
    for (int64_t sr = (a - g0) * Q; sr < (b - g0) * Q; ++sr) v = dadd(v, part[sr * len + e]);
    *dst = v;
  }
}

// nodes (int32): [feature | firstChild | leafIndex], total nodes each, a tree's
// firstChild and leafIndex local to the tree; starts (int32): [nodeStart |
// leafStart], T + 1 each; leafValue: total leaves x max(C, 1)
__global__ __launch_bounds__(256) void k_rf_predict(
    const double* __restrict__ X, int64_t n, int d, int T, int totalNodes,
    const int32_t* __restrict__ nodes, const double* __restrict__ thr,
    const int32_t* __restrict__ starts, int C, const double* __restrict__ leafValue,
    int32_t* __restrict__ leaf, double* __restrict__ raw, double* __restrict__ prob,
    double* __restrict__ pred) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  const int32_t* feature = nodes;
  const int32_t* firstChild = nodes + totalNodes;
  const int32_t* leafIndex = nodes + 2 * (int64_t)totalNodes;
  const double* x = X + r * d;
  double sum = 0.0;
  for (int t = 0; t < T; ++t) {
    const int base = starts[t];
    int node = 0;
    // a child's index is above its parent's (checked by the host): it ends
    for (;;) {
      const int fc = firstChild[base + node];
      if (fc < 0) break;
      node = x[feature[base + node]] <= thr[base + node] ? fc : fc + 1;
    }
    const int li = leafIndex[base + node];
    if (leaf) leaf[r * T + t] = li;
    const int64_t gl = (int64_t)starts[T + 1 + t] + li;
    if (C) {
      if (raw)
        for (int c = 0; c < C; ++c) {
          const double v = leafValue[gl * C + c];
          raw[r * C + c] = t ? dadd(raw[r * C + c], v) : v;
        }
    } else {
      sum = dadd(sum, leafValue[gl]);
    }
  }
  if (!C) {
    if (pred) pred[r] = sum / (double)T;
    return;
  }
  if (prob) {
    double s = 0.0;
    for (int c = 0; c < C; ++c) s = dadd(s, raw[r * C + c]);
    for (int c = 0; c < C; ++c) {
      const double v = raw[r * C + c];
      prob[r * C + c] = s != 0.0 ? v / s : v;
    }
  }
  if (pred) {
    int best = 0;
    double bv = raw[r * C];
    for (int c = 1; c < C; ++c) {
      const double v = raw[r * C + c];
      if (v > bv) { bv = v; best = c; }
    }
    pred[r] = (double)best;
  }
}

int64_t runs_per_launch(const cyc_rf_plan_s* p, int m, int B) {
  const int Q = kLanes / panel_width(m);
  return std::max<int64_t>(1, p->wsBytes / (8 * (int64_t)num_stats(p->C) * B * m * Q));
}

}  // namespace

extern "C" {

int cyc_rf_plan_create(int32_t numFeatures, int32_t numClasses, int64_t workspaceBytes,
                       cyc_rf_plan* plan) {
  CYC_REQUIRE(plan != nullptr, "plan must not be null");
  CYC_REQUIRE(numFeatures >= 1 && numFeatures <= kMaxFeatures,
              "RandomForest supports 1 to " + std::to_string(kMaxFeatures) +
                  " features but got " + std::to_string(numFeatures));
  CYC_REQUIRE(numClasses >= 0 && numClasses <= kMaxClasses,
              "RandomForest supports 1 to " + std::to_string(kMaxClasses) +
                  " classes (0: regression) but got " + std::to_string(numClasses));
  CYC_REQUIRE(workspaceBytes >= 0, "workspaceBytes must not be negative");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    cyc::set_error("no HIP device visible");
    return CYC_ERR_NO_DEVICE;
  }
  auto* p = new cyc_rf_plan_s();
  p->d = numFeatures;
  p->C = numClasses;
  p->wsBytes = workspaceBytes ? workspaceBytes : kDefaultWorkspace;
  *plan = p;
  return CYC_OK;
}

int cyc_rf_plan_destroy(cyc_rf_plan plan) {
  delete plan;
  return CYC_OK;
}

int64_t cyc_rf_max_trees(void) { return kMaxTrees; }
int64_t cyc_rf_max_nodes(void) { return kMaxNodes; }
int64_t cyc_rf_run_rows(void) { return kRunRows; }
int64_t cyc_rf_num_stats(cyc_rf_plan plan) { return plan ? num_stats(plan->C) : -1; }
int64_t cyc_rf_sub_runs(int32_t numSubset) {
  return numSubset >= 1 ? kLanes / panel_width(numSubset) : -1;
}
int64_t cyc_rf_runs_per_launch(cyc_rf_plan plan, int32_t numSubset, int32_t numBins) {
  return plan && numSubset >= 1 && numSubset <= plan->d && numBins >= 1 && numBins <= kMaxBins
             ? runs_per_launch(plan, numSubset, numBins)
             : -1;
}

int cyc_rf_bag_dev(cyc_rf_plan plan, int64_t nrows, int32_t numTrees, int64_t rowOffset,
                   uint64_t seed, const uint64_t* table, int32_t tableLen, uint8_t* bag,
                   void* stream) {
  CYC_REQUIRE(plan != nullptr, "plan must not be null");
  CYC_REQUIRE(nrows >= 0 && nrows <= INT32_MAX, "0 <= nrows <= 2147483647");
  CYC_REQUIRE(numTrees >= 1 && numTrees <= kMaxTrees,
              "1 to " + std::to_string(kMaxTrees) + " trees but got " + std::to_string(numTrees));
  CYC_REQUIRE(rowOffset >= 0, "rowOffset must not be negative");
  CYC_REQUIRE(table != nullptr && tableLen >= 1 && tableLen <= kMaxBagTable,
              "a table of 1 to " + std::to_string(kMaxBagTable) + " entries");
  for (int k = 0; k < tableLen; ++k) {
    CYC_REQUIRE(table[k] <= (1ull << 53), "table entry " + std::to_string(k) + " must be at most 2^53");
    CYC_REQUIRE(k == 0 || table[k - 1] <= table[k], "the table must be ascending");
  }
  if (nrows == 0) return CYC_OK;
  CYC_REQUIRE(bag != nullptr, "bag must not be null");
  cyc_rf_plan_s* p = plan;
  hipStream_t st = cyc::as_stream(stream);
  std::lock_guard<std::mutex> g(p->mu);
  const size_t tb = sizeof(uint64_t) * (size_t)tableLen;
  if (int rc = p->bagTable.reserve(tb)) return rc;
  CYC_HIP(hipMemcpyAsync(p->bagTable.ptr, table, tb, hipMemcpyHostToDevice, st));
  cyc::KernelTimer timer("k_rf_bag", st);
  hipLaunchKernelGGL(k_rf_bag, dim3((unsigned)((nrows + 255) / 256), (unsigned)numTrees), dim3(256),
                     0, st, nrows, rowOffset, seed, (const uint64_t*)p->bagTable.ptr, tableLen, bag);
  CYC_LAUNCH_CHECK("k_rf_bag");
  return CYC_OK;
}

int cyc_rf_route_dev(cyc_rf_plan plan, const uint8_t* image, int64_t nrows, int32_t numTrees,
                     int32_t* slot, const int32_t* slotStart, const int32_t* table, void* stream) {
  CYC_REQUIRE(plan != nullptr, "plan must not be null");
  CYC_REQUIRE(nrows >= 0 && nrows <= INT32_MAX, "0 <= nrows <= 2147483647");
  CYC_REQUIRE(numTrees >= 1 && numTrees <= kMaxTrees,
              "1 to " + std::to_string(kMaxTrees) + " trees but got " + std::to_string(numTrees));
  CYC_REQUIRE(slotStart != nullptr && table != nullptr, "non-null slotStart and table");
  CYC_REQUIRE(slotStart[0] == 0, "slotStart must begin at 0");
  for (int t = 0; t < numTrees; ++t)
    CYC_REQUIRE(slotStart[t] <= slotStart[t + 1], "slotStart must not decrease");
  cyc_rf_plan_s* p = plan;
  const int total = slotStart[numTrees];
  CYC_REQUIRE(total >= 1, "a table of at least one slot");
  for (int s = 0; s < total; ++s) {
    const int32_t f = table[4 * s], b = table[4 * s + 1];
    if (f < 0) continue;
    CYC_REQUIRE(f < p->d && b >= 0 && b < kMaxSplits,
                "slot entry " + std::to_string(s) + " must split a feature in [0, " +
                    std::to_string(p->d) + ") at a bin in [0, " + std::to_string(kMaxSplits) +
                    ")");
    CYC_REQUIRE(table[4 * s + 2] >= -1 && table[4 * s + 3] >= -1,
                "the new slots of slot entry " + std::to_string(s) + " must be -1 or a slot");
  }
  if (nrows == 0) return CYC_OK;
  CYC_REQUIRE(image != nullptr && slot != nullptr, "non-null image and slot");
  hipStream_t st = cyc::as_stream(stream);
  std::lock_guard<std::mutex> g(p->mu);
  const size_t sb = sizeof(int32_t) * (size_t)(numTrees + 1), tb = sizeof(int32_t) * 4 * (size_t)total;
  if (int rc = p->meta.reserve(sb + tb)) return rc;
  char* md = (char*)p->meta.ptr;
  CYC_HIP(hipMemcpyAsync(md, slotStart, sb, hipMemcpyHostToDevice, st));
  CYC_HIP(hipMemcpyAsync(md + sb, table, tb, hipMemcpyHostToDevice, st));
  cyc::KernelTimer timer("k_rf_route", st);
  hipLaunchKernelGGL(k_rf_route, dim3((unsigned)((nrows + 255) / 256), (unsigned)numTrees),
                     dim3(256), 0, st, image, nrows, p->d, (const int32_t*)md,
                     (const int32_t*)(md + sb), slot);
  CYC_LAUNCH_CHECK("k_rf_route");
  return CYC_OK;
}

int cyc_rf_histogram_dev(cyc_rf_plan plan, const uint8_t* image, const double* y, const double* w,
                         const uint8_t* bag, int64_t nrows, const int32_t* slot, int32_t tree0,
                         int32_t tree1, const int32_t* slotStart, const int32_t* nodeOf,
                         int32_t numNodes, int32_t numSubset, const int32_t* nodeFeat,
                         int32_t numBins, double* hist, void* stream) {
  CYC_REQUIRE(plan != nullptr, "plan must not be null");
  cyc_rf_plan_s* p = plan;
  CYC_REQUIRE(nrows >= 0 && nrows <= INT32_MAX, "0 <= nrows <= 2147483647");
  CYC_REQUIRE(tree0 >= 0 && tree0 < tree1 && tree1 <= kMaxTrees,
              "a tree range inside [0, " + std::to_string(kMaxTrees) + ")");
  const int TR = tree1 - tree0;
  CYC_REQUIRE((int64_t)TR * nrows <= INT32_MAX,
              "the pairs of one call, (tree1 - tree0) nrows = " +
                  std::to_string((int64_t)TR * nrows) + ", must not exceed 2147483647");
  CYC_REQUIRE(numNodes >= 1 && numNodes <= kMaxNodes,
              "1 to " + std::to_string(kMaxNodes) + " nodes but got " + std::to_string(numNodes));
  CYC_REQUIRE(numBins >= 1 && numBins <= kMaxBins,
              "1 to " + std::to_string(kMaxBins) + " bins but got " + std::to_string(numBins));
  CYC_REQUIRE(numSubset >= 1 && numSubset <= p->d,
              "1 to " + std::to_string(p->d) + " features per node but got " +
                  std::to_string(numSubset));
  CYC_REQUIRE(nodeFeat != nullptr || numSubset == p->d,
              "nodeFeat may be null only when a node takes every feature");
  CYC_REQUIRE(slotStart != nullptr && nodeOf != nullptr, "non-null slotStart and nodeOf");
  CYC_REQUIRE(hist != nullptr, "hist must not be null");
  CYC_REQUIRE(slotStart[0] == 0, "slotStart must begin at 0");
  for (int t = 0; t < TR; ++t)
    CYC_REQUIRE(slotStart[t] <= slotStart[t + 1], "slotStart must not decrease");
  const int total = slotStart[TR];
  CYC_REQUIRE(total >= 1, "a node per slot, at least one slot");
  const int d = p->d, K = numNodes, B = numBins, S = num_stats(p->C), m = numSubset;
  hipStream_t st = cyc::as_stream(stream);
  std::lock_guard<std::mutex> g(p->mu);
  // the tree of every node, from the slots that name it: a node's pairs lie in one tree
  std::vector<int32_t>& nodeTree = p->nodeTree;
  nodeTree.assign((size_t)K, -1);
  for (int t = 0; t < TR; ++t)
    for (int s = slotStart[t]; s < slotStart[t + 1]; ++s) {
      const int32_t c = nodeOf[s];
      CYC_REQUIRE(c >= -1 && c < K,
                  "the node of slot entry " + std::to_string(s) + " must be -1 or in [0, " +
                      std::to_string(K) + ")");
      if (c < 0) continue;
      CYC_REQUIRE(nodeTree[c] < 0 || nodeTree[c] == t,
                  "node " + std::to_string(c) + " is named by slots of two trees");
      nodeTree[c] = t;
    }
  for (int c = 0; c < K; ++c)
    if (nodeTree[c] < 0) nodeTree[c] = 0;   // a node no slot names has no pairs
  if (nodeFeat)
    for (int64_t i = 0; i < (int64_t)K * m; ++i)
      CYC_REQUIRE(nodeFeat[i] >= 0 && nodeFeat[i] < d,
                  "nodeFeat entry " + std::to_string(i) + " must be a feature in [0, " +
                      std::to_string(d) + ") but is " + std::to_string(nodeFeat[i]));
  const int64_t len = (int64_t)S * B * m;
  CYC_HIP(hipMemsetAsync(hist, 0, sizeof(double) * (size_t)(K * len), st));
  if (nrows == 0) return CYC_OK;
  CYC_REQUIRE(image != nullptr && y != nullptr, "non-null image and labels");
  const int64_t pairs = (int64_t)TR * nrows;
  // meta (int32): slotStart | nodeOf | nodeTree | nodeFeat
  const size_t nSS = (size_t)TR + 1, nNO = (size_t)total, nNT = (size_t)K,
               nNF = nodeFeat ? (size_t)K * m : 0;
  if (int rc = p->meta.reserve(sizeof(int32_t) * (nSS + nNO + nNT + nNF))) return rc;
  int32_t* md = (int32_t*)p->meta.ptr;
  CYC_HIP(hipMemcpyAsync(md, slotStart, sizeof(int32_t) * nSS, hipMemcpyHostToDevice, st));
  CYC_HIP(hipMemcpyAsync(md + nSS, nodeOf, sizeof(int32_t) * nNO, hipMemcpyHostToDevice, st));
  CYC_HIP(hipMemcpyAsync(md + nSS + nNO, nodeTree.data(), sizeof(int32_t) * nNT,
                         hipMemcpyHostToDevice, st));
  if (nodeFeat)
    CYC_HIP(hipMemcpyAsync(md + nSS + nNO + nNT, nodeFeat, sizeof(int32_t) * nNF,
                           hipMemcpyHostToDevice, st));
  if (int rc = p->key.reserve(sizeof(int32_t) * (size_t)pairs)) return rc;
  if (int rc = p->runStart.reserve(sizeof(int64_t) * (size_t)(K + 1))) return rc;
  int32_t* key = (int32_t*)p->key.ptr;
  const int64_t off = (int64_t)tree0 * nrows;
  const uint8_t* bag0 = bag ? bag + off : nullptr;
  {
    cyc::KernelTimer timer("k_rf_key", st);
    hipLaunchKernelGGL(k_rf_key, dim3((unsigned)((nrows + 255) / 256), (unsigned)TR), dim3(256), 0,
                       st, slot ? slot + off : nullptr, bag0, nrows, (const int32_t*)md,
                       (const int32_t*)(md + nSS), K, key);
    CYC_LAUNCH_CHECK("k_rf_key");
  }
  int64_t maxChunks = 0;
  // d = 0: the sort's own chunk buffers are not used here
  if (int rc = cyc::kmsums::sort_clusters(p->sort, key, pairs, 0, K + 1, st, maxChunks)) return rc;
  const int32_t* perm = (const int32_t*)p->sort.perm.ptr;
  const int64_t* cstart = (const int64_t*)p->sort.cstart.ptr;
  int64_t* runStart = (int64_t*)p->runStart.ptr;
  hipLaunchKernelGGL(k_rf_runs, dim3(1), dim3(64), 0, st, cstart, K, runStart);
  CYC_LAUNCH_CHECK("k_rf_runs");
  // the run count is on the device: the bound is launched, the surplus leaves
  const int P = panel_width(m), Q = kLanes / P;
  const int64_t maxRuns = pairs / kRunRows + K;
  const int64_t group = std::min(maxRuns, runs_per_launch(p, m, B));
  if (int rc = p->ws.reserve(sizeof(double) * (size_t)(group * Q * len))) return rc;
  const int W = std::min(S * B, kWindow);
  const unsigned panels = (unsigned)((m + P - 1) / P);
  const unsigned passes = (unsigned)((S * B + kWindow - 1) / kWindow);
  const unsigned foldBlocks = (unsigned)std::min<int64_t>((len + 255) / 256, 1024);
  for (int64_t g0 = 0; g0 < maxRuns; g0 += group) {
    const int64_t gc = std::min(group, maxRuns - g0);
    {
      cyc::KernelTimer timer("k_rf_hist", st);
      hipLaunchKernelGGL(k_rf_hist, dim3((unsigned)gc, panels, passes), dim3(kLanes),
                         sizeof(double) * (size_t)W * kLanes, st, image, nrows, d, y, w, bag0, perm,
                         cstart, (const int64_t*)runStart, K, g0, B, p->C, m, P, W,
                         (const int32_t*)(md + nSS + nNO),
                         nodeFeat ? (const int32_t*)(md + nSS + nNO + nNT) : nullptr,
                         (double*)p->ws.ptr);
      CYC_LAUNCH_CHECK("k_rf_hist");
    }
    cyc::KernelTimer timer("k_rf_fold", st);
    hipLaunchKernelGGL(k_rf_fold, dim3((unsigned)K, foldBlocks), dim3(256), 0, st,
                       (const double*)p->ws.ptr, (const int64_t*)runStart, m, B, S, Q, g0, gc, hist);
    CYC_LAUNCH_CHECK("k_rf_fold");
  }
  return CYC_OK;
}

int cyc_rf_predict_dev(cyc_rf_plan plan, const double* X, int64_t nrows, int32_t numTrees,
                       const int32_t* nodeStart, const int32_t* leafStart, const int32_t* feature,
                       const double* threshold, const int32_t* firstChild,
                       const int32_t* leafIndex, const double* leafValue, int32_t* leaf,
                       double* raw, double* prob, double* pred, void* stream) {
  CYC_REQUIRE(plan != nullptr, "plan must not be null");
  cyc_rf_plan_s* p = plan;
  CYC_REQUIRE(nrows >= 0, "nrows >= 0");
  CYC_REQUIRE(numTrees >= 1 && numTrees <= kMaxTrees,
              "1 to " + std::to_string(kMaxTrees) + " trees but got " + std::to_string(numTrees));
  CYC_REQUIRE(nodeStart != nullptr && leafStart != nullptr, "non-null nodeStart and leafStart");
  CYC_REQUIRE(feature != nullptr && threshold != nullptr && firstChild != nullptr &&
                  leafIndex != nullptr && leafValue != nullptr,
              "non-null node arrays and leaf values");
  CYC_REQUIRE(nodeStart[0] == 0 && leafStart[0] == 0, "nodeStart and leafStart must begin at 0");
  for (int t = 0; t < numTrees; ++t) {
    const int64_t nn = (int64_t)nodeStart[t + 1] - nodeStart[t];
    const int64_t nl = (int64_t)leafStart[t + 1] - leafStart[t];
    CYC_REQUIRE(nn >= 1 && nn <= kMaxTreeNodes && nl >= 1 && nl <= nn,
                "tree " + std::to_string(t) + " needs 1 to " + std::to_string(kMaxTreeNodes) +
                    " nodes and 1 to as many leaves");
    CYC_REQUIRE(nodeStart[t + 1] > nodeStart[t], "nodeStart must increase");
    for (int64_t i = 0; i < nn; ++i) {
      const int64_t at = nodeStart[t] + i;
      const int32_t fc = firstChild[at];
      if (fc >= 0) {
        CYC_REQUIRE(fc > i && (int64_t)fc + 2 <= nn,
                    "the children of node " + std::to_string(i) + " of tree " + std::to_string(t) +
                        " must follow it and lie inside the tree");
        CYC_REQUIRE(feature[at] >= 0 && feature[at] < p->d,
                    "node " + std::to_string(i) + " of tree " + std::to_string(t) +
                        " must split a feature in [0, " + std::to_string(p->d) + ")");
      } else {
        CYC_REQUIRE(leafIndex[at] >= 0 && leafIndex[at] < nl,
                    "leaf node " + std::to_string(i) + " of tree " + std::to_string(t) +
                        " needs a leaf index in [0, " + std::to_string(nl) + ")");
      }
    }
  }
  CYC_REQUIRE(prob == nullptr || p->C > 0, "prob needs a classifier's plan");
  CYC_REQUIRE(raw == nullptr || p->C > 0, "raw needs a classifier's plan");
  CYC_REQUIRE(p->C == 0 || raw != nullptr || (prob == nullptr && pred == nullptr),
              "a classifier's prob and pred need raw: the votes are added there");
  if (nrows == 0) return CYC_OK;
  CYC_REQUIRE(X != nullptr, "rows must not be null");
  hipStream_t st = cyc::as_stream(stream);
  std::lock_guard<std::mutex> g(p->mu);
  const int totalNodes = nodeStart[numTrees], totalLeaves = leafStart[numTrees];
  const size_t nb = sizeof(int32_t) * (size_t)totalNodes, tb = sizeof(double) * (size_t)totalNodes;
  const size_t sb = sizeof(int32_t) * (size_t)(numTrees + 1);
  const size_t lb = sizeof(double) * (size_t)totalLeaves * (size_t)std::max(p->C, 1);
  if (int rc = p->tree.reserve(3 * nb + 2 * sb)) return rc;
  if (int rc = p->thr.reserve(tb)) return rc;
  if (int rc = p->leaf.reserve(lb)) return rc;
  char* nd = (char*)p->tree.ptr;
  CYC_HIP(hipMemcpyAsync(nd, feature, nb, hipMemcpyHostToDevice, st));
  CYC_HIP(hipMemcpyAsync(nd + nb, firstChild, nb, hipMemcpyHostToDevice, st));
  CYC_HIP(hipMemcpyAsync(nd + 2 * nb, leafIndex, nb, hipMemcpyHostToDevice, st));
  CYC_HIP(hipMemcpyAsync(nd + 3 * nb, nodeStart, sb, hipMemcpyHostToDevice, st));
  CYC_HIP(hipMemcpyAsync(nd + 3 * nb + sb, leafStart, sb, hipMemcpyHostToDevice, st));
  CYC_HIP(hipMemcpyAsync(p->thr.ptr, threshold, tb, hipMemcpyHostToDevice, st));
  CYC_HIP(hipMemcpyAsync(p->leaf.ptr, leafValue, lb, hipMemcpyHostToDevice, st));
  cyc::KernelTimer timer("k_rf_predict", st);
  hipLaunchKernelGGL(k_rf_predict, dim3((unsigned)((nrows + 255) / 256)), dim3(256), 0, st, X,
                     nrows, p->d, numTrees, totalNodes, (const int32_t*)nd,
                     (const double*)p->thr.ptr, (const int32_t*)(nd + 3 * nb), p->C,
                     (const double*)p->leaf.ptr, leaf, raw, prob, pred);
  CYC_LAUNCH_CHECK("k_rf_predict");
  return CYC_OK;
}

}  // extern "C"
