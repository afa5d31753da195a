// gbt.hip -- gradient-boosted trees on gfx950 (MI355X): the pass between two
// trees of ml/tree/impl/GradientBoostedTrees.scala's boost (updatePredictionError
// and computeWeightedError in one launch) and the ensemble's descent
// (GBTRegressionModel.predict, GBTClassificationModel's margin, raw and
// probability).  The trees themselves are grown by random_forest.hip's
// histogram and route over decision_tree.hip's binned image; the boosting loop,
// the losses' host form and the models are cycloneml_amd/gbt.py.
//
// A tree reaches the device as nodes of 16 bytes, breadth first, node 0 the
// root: (feature, firstChild, v).  firstChild < 0 is a leaf and v its value;
// otherwise the children are firstChild and firstChild + 1, both above the
// node's own index (checked on the host, so every walk ends inside the array),
// and v is the threshold (fp64 rows: x[feature] <= v goes to firstChild) or,
// in its low 32 bits, the split bin (image rows: byte <= bin goes to
// firstChild, the byte zero-extended, bins reach 255).
//
// Kernels
//   k_gbt_update   a thread per row, 256 rows per workgroup.  A tree of at most
//                  kLdsNodes nodes is staged in LDS (16 numNodes bytes, sized by
//                  the launch), a larger one is read from global memory.  The
//                  walk gathers the one byte (or double) per level of the row's
//                  own path.  Then, each operation rounded once, unfused:
//                    F = pred + leaf treeWeight            pred <- F
//                    squared   g = -2 (y - F)              e = (y - F)(y - F)
//                    absolute  g = y - F < 0 ? 1 : -1      e = |y - F|
//                    logistic  g = (-4 y) / (1 + exp((2 y) F))
//                              e = 2 log1pExp(-((2 y) F))
//                    resid <- -g (when asked for)
//                  and the workgroup's e w and w (1.0 without weights; rows past
//                  n add +0.0) go through one fixed binary tree in LDS (stride
//                  128, 64, .., 1) into part[2 block], part[2 block + 1].
//   k_gbt_fold     one workgroup: thread t adds the partials of the blocks t, t +
//                  256, t + 512, .. in block order from 0.0, the 256 sums go
//                  through the same tree, and sums[0], sums[1] are SET.
//   k_gbt_predict  a thread per row walks every tree in tree order over fp64
//                  rows.  The host cuts the trees, in order, into tiles of at
//                  most kLdsNodes nodes; a workgroup stages one tile after the
//                  other in LDS (a tree that is larger than a tile alone is a
//                  tile of its own and read from global memory) and a row's sum
//                  stays in its thread's register over all tiles:
//                    margin = 0.0; margin += leaf_t w_t   in tree order,
//                  whatever the tiling.  A leaf node carries its leaf index in
//                  the feature field.  p = 1 / (1 + exp(-2 margin)).
// exp and log1p are the device library's, the ones the binary logistic
// aggregator's epilogue calls (binary_rows.hpp's log1p_exp is used as it is).
// No atomics on doubles; every sum has one fixed order: two calls give the same
// bytes.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <mutex>
#include <string>
#include <vector>

#include "binary_rows.hpp"
#include "common.hpp"
#include "decision_tree.hpp"

using namespace cyc::dt;

namespace {

struct GbtNode {
  int32_t feature;      // a leaf of k_gbt_predict: its leaf index
  int32_t firstChild;   // -1: a leaf
  union {
    double v;           // the leaf's value, or the threshold
    int32_t bin;        // image rows: the split bin
  };
};
static_assert(sizeof(GbtNode) == 16, "a node is one 16-byte LDS slot");

constexpr int kBlock = 256;
constexpr int kLdsNodes = 2048;   // 32 KiB of nodes
constexpr int kMaxTrees = 4096;
constexpr int kLossSquared = 0, kLossAbsolute = 1, kLossLogistic = 2;

// the fixed tree over a workgroup's 256 pairs; the result is in a[0], b[0]
__device__ __forceinline__ void block_tree(double* a, double* b, int tid) {
  __syncthreads();
  for (int s = kBlock / 2; s > 0; s >>= 1) {
    if (tid < s) {
      a[tid] = dadd(a[tid], a[tid + s]);
      b[tid] = dadd(b[tid], b[tid + s]);
    }
    __syncthreads();
  }
}

template <bool IMAGE, typename Tree>
__device__ __forceinline__ int gbt_walk(Tree tree, const uint8_t* __restrict__ bytes,
                                        const double* __restrict__ x) {
  int node = 0;
  for (;;) {
    const int fc = tree[node].firstChild;
    if (fc < 0) return node;
    const int f = tree[node].feature;
    const bool left = IMAGE ? (int)bytes[f] <= tree[node].bin : x[f] <= tree[node].v;
    node = left ? fc : fc + 1;
  }
}

template <bool IMAGE, bool STAGED>
__global__ __launch_bounds__(kBlock) void k_gbt_update(
    const uint8_t* __restrict__ image, const double* __restrict__ X, int64_t n, int d,
    const GbtNode* __restrict__ nodes, int numNodes, double treeWeight, int loss,
    const double* __restrict__ y, const double* __restrict__ w, double* __restrict__ pred,
    double* __restrict__ resid, double* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) unsigned char dyn[];
  GbtNode* staged = reinterpret_cast<GbtNode*>(dyn);
  double* redE = reinterpret_cast<double*>(dyn + (STAGED ? sizeof(GbtNode) * (size_t)numNodes : 0));
  double* redW = redE + kBlock;
  const int tid = threadIdx.x;
  const int64_t r = (int64_t)blockIdx.x * kBlock + tid;
  if (STAGED) {
    for (int i = tid; i < numNodes; i += kBlock) staged[i] = nodes[i];
    __syncthreads();
  }
  double we = 0.0, ww = 0.0;
  if (r < n) {
    const uint8_t* bytes = IMAGE ? image + r * d : nullptr;
    const double* x = IMAGE ? nullptr : X + r * d;
    double leaf;
    if (STAGED) leaf = staged[gbt_walk<IMAGE>(staged, bytes, x)].v;
    else leaf = nodes[gbt_walk<IMAGE>(nodes, bytes, x)].v;
    const double F = dadd(pred[r], dmul(leaf, treeWeight));
    pred[r] = F;
    const double yy = y[r];
    double g, e;
    if (loss == kLossLogistic) {
      const double margin = dmul(dmul(2.0, yy), F);
      g = dmul(-4.0, yy) / dadd(1.0, exp(margin));
      e = dmul(2.0, cyc::log1p_exp(-margin));
    } else {
      const double diff = dsub(yy, F);
      if (loss == kLossAbsolute) {
        g = diff < 0.0 ? 1.0 : -1.0;
        e = fabs(diff);
      } else {
        g = dmul(-2.0, diff);
        e = dmul(diff, diff);
      }
    }
    if (resid) resid[r] = -g;
    ww = w ? w[r] : 1.0;
    we = dmul(e, ww);
  }
  redE[tid] = we;
  redW[tid] = ww;
  block_tree(redE, redW, tid);
  if (tid == 0) {
    part[2 * (int64_t)blockIdx.x] = redE[0];
    part[2 * (int64_t)blockIdx.x + 1] = redW[0];
  }
}

__global__ __launch_bounds__(kBlock) void k_gbt_fold(const double* __restrict__ part,
                                                     int64_t numBlocks,
                                                     double* __restrict__ sums) {
  __shared__ double redE[kBlock], redW[kBlock];
  const int tid = threadIdx.x;
  double a = 0.0, b = 0.0;
  for (int64_t i = tid; i < numBlocks; i += kBlock) {
    a = dadd(a, part[2 * i]);
    b = dadd(b, part[2 * i + 1]);
  }
  redE[tid] = a;
  redW[tid] = b;
  block_tree(redE, redW, tid);
  if (tid == 0) {
    sums[0] = redE[0];
    sums[1] = redW[0];
  }
}

// tiles (int32): [first tree of tile k | .. | numTrees] then per tile 1: staged;
// nodeStart: numTrees + 1
__global__ __launch_bounds__(kBlock) void k_gbt_predict(
    const double* __restrict__ X, int64_t n, int d, int T, const GbtNode* __restrict__ nodes,
    const int32_t* __restrict__ nodeStart, const double* __restrict__ treeWeights,
    const int32_t* __restrict__ tiles, int numTiles, int classifier, int32_t* __restrict__ leaf,
    double* __restrict__ margin, double* __restrict__ raw, double* __restrict__ prob,
    double* __restrict__ pred) {
  __shared__ GbtNode staged[kLdsNodes];
  const int tid = threadIdx.x;
  const int64_t r = (int64_t)blockIdx.x * kBlock + tid;
  const double* x = X + (r < n ? r : 0) * d;
  double sum = 0.0;
  for (int k = 0; k < numTiles; ++k) {
    const int ta = tiles[k], tb = tiles[k + 1];
    const bool inLds = tiles[numTiles + 1 + k] != 0;
    const int base = nodeStart[ta];
    if (inLds) {
      const int cnt = nodeStart[tb] - base;
      __syncthreads();   // the previous tile's walks are over
      for (int i = tid; i < cnt; i += kBlock) staged[i] = nodes[base + i];
      __syncthreads();
    }
    if (r >= n) continue;
    for (int t = ta; t < tb; ++t) {
      int li;
      double v;
      if (inLds) {
        const GbtNode* tree = staged + (nodeStart[t] - base);
        const int at = gbt_walk<false>(tree, nullptr, x);
        li = tree[at].feature;
        v = tree[at].v;
      } else {
        const GbtNode* tree = nodes + nodeStart[t];
        const int at = gbt_walk<false>(tree, nullptr, x);
        li = tree[at].feature;
        v = tree[at].v;
      }
      if (leaf) leaf[r * T + t] = li;
      sum = dadd(sum, dmul(v, treeWeights[t]));
    }
  }
  if (r >= n) return;
  if (margin) margin[r] = sum;
  if (raw) {
    raw[2 * r] = -sum;
    raw[2 * r + 1] = sum;
  }
  if (prob) {
    const double p = 1.0 / dadd(1.0, exp(dmul(-2.0, sum)));
    prob[2 * r] = dsub(1.0, p);
    prob[2 * r + 1] = p;
  }
  if (pred) pred[r] = classifier ? (sum > 0.0 ? 1.0 : 0.0) : sum;
}

// the checks every tree array gets before a kernel may walk it; nn nodes at `at`
int check_tree(int tree, int64_t nn, const int32_t* feature, const int32_t* firstChild,
               const int32_t* splitBin, int d) {
  for (int64_t i = 0; i < nn; ++i) {
    const int32_t fc = firstChild[i];
    if (fc < 0) continue;
    CYC_REQUIRE(fc > i && (int64_t)fc + 2 <= nn,
                "the children of node " + std::to_string(i) + " of tree " + std::to_string(tree) +
                    " must follow it and lie inside the tree");
    CYC_REQUIRE(feature[i] >= 0 && feature[i] < d,
                "node " + std::to_string(i) + " of tree " + std::to_string(tree) +
                    " must split a feature in [0, " + std::to_string(d) + ")");
    CYC_REQUIRE(!splitBin || (splitBin[i] >= 0 && splitBin[i] < kMaxSplits),
                "node " + std::to_string(i) + " of tree " + std::to_string(tree) +
                    " must split at a bin in [0, " + std::to_string(kMaxSplits) + ")");
  }
  return CYC_OK;
}

}  // namespace

struct cyc_gbt_plan_s {
  std::mutex mu;
  int d = 0;
  cyc::DeviceBuffer nodes, meta, part;
  std::vector<GbtNode> hostNodes;
  std::vector<int32_t> hostMeta;
};

extern "C" {

int cyc_gbt_plan_create(int32_t numFeatures, cyc_gbt_plan* plan) {
  CYC_REQUIRE(plan != nullptr, "plan must not be null");
  CYC_REQUIRE(numFeatures >= 1 && numFeatures <= kMaxFeatures,
              "GBT supports 1 to " + std::to_string(kMaxFeatures) + " features but got " +
                  std::to_string(numFeatures));
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    cyc::set_error("no HIP device visible");
    return CYC_ERR_NO_DEVICE;
  }
  auto* p = new cyc_gbt_plan_s();
  p->d = numFeatures;
  *plan = p;
  return CYC_OK;
}

int cyc_gbt_plan_destroy(cyc_gbt_plan plan) {
  delete plan;
  return CYC_OK;
}

int64_t cyc_gbt_lds_nodes(void) { return kLdsNodes; }
int64_t cyc_gbt_max_trees(void) { return kMaxTrees; }

int cyc_gbt_update_dev(cyc_gbt_plan plan, const uint8_t* image, const double* X, int64_t nrows,
                       int32_t numNodes, const int32_t* feature, const int32_t* splitBin,
                       const double* threshold, const int32_t* firstChild, const double* value,
                       double treeWeight, int32_t loss, const double* y, const double* w,
                       double* pred, double* resid, double* sums, void* stream) {
  CYC_REQUIRE(plan != nullptr, "plan must not be null");
  cyc_gbt_plan_s* p = plan;
  CYC_REQUIRE(nrows >= 0 && nrows <= INT32_MAX, "0 <= nrows <= 2147483647");
  CYC_REQUIRE(numNodes >= 1 && numNodes <= kMaxTreeNodes,
              "a tree of 1 to " + std::to_string(kMaxTreeNodes) + " nodes but got " +
                  std::to_string(numNodes));
  CYC_REQUIRE(loss >= kLossSquared && loss <= kLossLogistic,
              "loss must be 0 (squared), 1 (absolute) or 2 (logistic) but got " +
                  std::to_string(loss));
  CYC_REQUIRE(feature != nullptr && firstChild != nullptr && value != nullptr,
              "non-null node arrays and values");
  CYC_REQUIRE((image != nullptr) != (X != nullptr) || nrows == 0,
              "the rows come as the image or as fp64 rows, one of the two");
  const bool asImage = image != nullptr || (X == nullptr && splitBin != nullptr);
  CYC_REQUIRE(asImage ? splitBin != nullptr : threshold != nullptr,
              "image rows need splitBin, fp64 rows need threshold");
  CYC_REQUIRE(sums != nullptr, "sums must not be null");
  if (int rc = check_tree(0, numNodes, feature, firstChild, asImage ? splitBin : nullptr, p->d))
    return rc;
  hipStream_t st = cyc::as_stream(stream);
  if (nrows == 0) {
    CYC_HIP(hipMemsetAsync(sums, 0, 2 * sizeof(double), st));
    return CYC_OK;
  }
  CYC_REQUIRE(y != nullptr && pred != nullptr, "non-null labels and predictions");
  std::lock_guard<std::mutex> g(p->mu);
  std::vector<GbtNode>& hn = p->hostNodes;
  hn.assign((size_t)numNodes, GbtNode{});
  for (int i = 0; i < numNodes; ++i) {
    hn[i].feature = feature[i];
    hn[i].firstChild = firstChild[i] < 0 ? -1 : firstChild[i];
    if (firstChild[i] < 0) hn[i].v = value[i];
    else if (asImage) hn[i].bin = splitBin[i];
    else hn[i].v = threshold[i];
  }
  const int64_t blocks = (nrows + kBlock - 1) / kBlock;
  const size_t nb = sizeof(GbtNode) * (size_t)numNodes;
  if (int rc = p->nodes.reserve(nb)) return rc;
  if (int rc = p->part.reserve(sizeof(double) * 2 * (size_t)blocks)) return rc;
  CYC_HIP(hipMemcpyAsync(p->nodes.ptr, hn.data(), nb, hipMemcpyHostToDevice, st));
  // the upload reads hostNodes: the next call may not rewrite them before it is done
  CYC_HIP(hipStreamSynchronize(st));
  const bool inLds = numNodes <= kLdsNodes;
  const size_t lds = (inLds ? nb : 0) + sizeof(double) * 2 * kBlock;
  const GbtNode* dn = (const GbtNode*)p->nodes.ptr;
  double* part = (double*)p->part.ptr;
  {
    cyc::KernelTimer timer("k_gbt_update", st);
    auto launch = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(kBlock), lds, st, image, X, nrows,
                         p->d, dn, numNodes, treeWeight, loss, y, w, pred, resid, part);
    };
    if (asImage) {
      if (inLds) launch(k_gbt_update<true, true>);
      else launch(k_gbt_update<true, false>);
    } else {
      if (inLds) launch(k_gbt_update<false, true>);
      else launch(k_gbt_update<false, false>);
    }
    CYC_LAUNCH_CHECK("k_gbt_update");
  }
  cyc::KernelTimer timer("k_gbt_fold", st);
  hipLaunchKernelGGL(k_gbt_fold, dim3(1), dim3(kBlock), 0, st, (const double*)part, blocks, sums);
  CYC_LAUNCH_CHECK("k_gbt_fold");
  return CYC_OK;
}

int cyc_gbt_predict_dev(cyc_gbt_plan plan, const double* X, int64_t nrows, int32_t numTrees,
                        const int32_t* nodeStart, const int32_t* feature,
                        const double* threshold, const int32_t* firstChild,
                        const int32_t* leafIndex, const double* value, const double* treeWeights,
                        int32_t classifier, int32_t* leaf, double* margin, double* raw,
                        double* prob, double* pred, void* stream) {
  CYC_REQUIRE(plan != nullptr, "plan must not be null");
  cyc_gbt_plan_s* p = plan;
  CYC_REQUIRE(nrows >= 0 && nrows <= INT32_MAX, "0 <= nrows <= 2147483647");
  CYC_REQUIRE(numTrees >= 1 && numTrees <= kMaxTrees,
              "1 to " + std::to_string(kMaxTrees) + " trees but got " + std::to_string(numTrees));
  CYC_REQUIRE(nodeStart != nullptr && feature != nullptr && threshold != nullptr &&
                  firstChild != nullptr && leafIndex != nullptr && value != nullptr &&
                  treeWeights != nullptr,
              "non-null nodeStart, node arrays, values and treeWeights");
  CYC_REQUIRE(nodeStart[0] == 0, "nodeStart must begin at 0");
  CYC_REQUIRE(classifier != 0 || (raw == nullptr && prob == nullptr),
              "raw and prob need a classifier");
  for (int t = 0; t < numTrees; ++t) {
    const int64_t nn = (int64_t)nodeStart[t + 1] - nodeStart[t];
    CYC_REQUIRE(nn >= 1 && nn <= kMaxTreeNodes,
                "tree " + std::to_string(t) + " needs 1 to " + std::to_string(kMaxTreeNodes) +
                    " nodes");
    const int64_t at = nodeStart[t];
    if (int rc = check_tree(t, nn, feature + at, firstChild + at, nullptr, p->d)) return rc;
  }
  if (nrows == 0) return CYC_OK;
  CYC_REQUIRE(X != nullptr, "rows must not be null");
  hipStream_t st = cyc::as_stream(stream);
  std::lock_guard<std::mutex> g(p->mu);
  const int total = nodeStart[numTrees];
  std::vector<GbtNode>& hn = p->hostNodes;
  hn.assign((size_t)total, GbtNode{});
  for (int i = 0; i < total; ++i) {
    const bool isLeaf = firstChild[i] < 0;
    hn[i].feature = isLeaf ? leafIndex[i] : feature[i];
    hn[i].firstChild = isLeaf ? -1 : firstChild[i];
    hn[i].v = isLeaf ? value[i] : threshold[i];
  }
  // tiles: the trees in order, as many as fit kLdsNodes nodes; a larger tree alone
  std::vector<int32_t> first, inLds;
  for (int t = 0; t < numTrees;) {
    int tb = t + 1;
    const bool fits = nodeStart[tb] - nodeStart[t] <= kLdsNodes;
    while (fits && tb < numTrees && nodeStart[tb + 1] - nodeStart[t] <= kLdsNodes) ++tb;
    first.push_back(t);
    inLds.push_back(fits ? 1 : 0);
    t = tb;
  }
  const int numTiles = (int)first.size();
  // meta (int32): nodeStart | tiles' first trees, numTrees | staged flags
  std::vector<int32_t>& hm = p->hostMeta;
  hm.assign(nodeStart, nodeStart + numTrees + 1);
  hm.insert(hm.end(), first.begin(), first.end());
  hm.push_back(numTrees);
  hm.insert(hm.end(), inLds.begin(), inLds.end());
  const size_t nb = sizeof(GbtNode) * (size_t)total, mb = sizeof(int32_t) * hm.size();
  const size_t wb = sizeof(double) * (size_t)numTrees;
  if (int rc = p->nodes.reserve(nb)) return rc;
  if (int rc = p->meta.reserve(mb)) return rc;
  if (int rc = p->part.reserve(wb)) return rc;
  CYC_HIP(hipMemcpyAsync(p->nodes.ptr, hn.data(), nb, hipMemcpyHostToDevice, st));
  CYC_HIP(hipMemcpyAsync(p->meta.ptr, hm.data(), mb, hipMemcpyHostToDevice, st));
  CYC_HIP(hipMemcpyAsync(p->part.ptr, treeWeights, wb, hipMemcpyHostToDevice, st));
  CYC_HIP(hipStreamSynchronize(st));   // the uploads read the plan's host vectors
  const int32_t* md = (const int32_t*)p->meta.ptr;
  cyc::KernelTimer timer("k_gbt_predict", st);
  hipLaunchKernelGGL(k_gbt_predict, dim3((unsigned)((nrows + kBlock - 1) / kBlock)), dim3(kBlock),
                     0, st, X, nrows, p->d, numTrees, (const GbtNode*)p->nodes.ptr, md,
                     (const double*)p->part.ptr, md + numTrees + 1, numTiles, classifier, leaf,
                     margin, raw, prob, pred);
  CYC_LAUNCH_CHECK("k_gbt_predict");
  return CYC_OK;
}

}  // extern "C"
