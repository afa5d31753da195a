// bisecting_kmeans.hip -- BisectingKMeans on gfx950 (MI355X): one inner
// iteration of mllib/clustering/BisectingKMeans.scala's level loop over dense
// fp64 rows, and BisectingKMeansModel's tree descent.  The level logic (which
// clusters divide, the random children, the tree) is host code
// (cycloneml_amd/bisecting_kmeans.py).
//
// State.  Every row has an int32 slot, a compact id of the cluster it sits in;
// the host keeps the slot <-> node index map.  A step reads slot[] and a table
// of (leftNew, rightNew, keepNew) per slot and writes newSlot[]: new slots 0 ..
// K - 1 are the children on offer (the rows of `centers`), new slots >= K hold
// the rows that take no part.
//
// Kernels
//   k_bkm_check    the lowest row whose norm is not finite (rule 1) or whose
//                  weight is not finite and positive (rule 2): an integer
//                  atomicMin.
//   k_bkm_assign   one thread per row, a workgroup per tile of kTileRows rows.
//                  The tile's rows go through LDS kPanel columns at a time
//                  (16 lanes read 128 contiguous bytes of a row, the next
//                  panel's loads are in flight while this one is summed), and
//                  each thread walks its row's columns in order with the two
//                  sequential sums of Vectors.sqdist, one per child, unfused.
//                  findClosest's bound skip decides only whether a distance is
//                  looked at, so both are formed and the reference's
//                  comparisons are then made as written: the same pick.  A row
//                  whose slot offers one child takes it (findClosest over one
//                  center returns index 0 whatever the distance); a row that
//                  offers none keeps keepNew.  Neither row is loaded, and a
//                  tile without a two-child row loads nothing.
//   k_bkm_chunk    after the stable sort of rows by new slot (kmeans_sums.hpp's
//                  sort_clusters; the rows that take no part are cluster K and
//                  are skipped): per chunk of kChunkRows rows of one child, in
//                  row order, sum of w x per column (axpy order); the chunk's
//                  sum of w and of (norm norm) w by one fixed tree over the
//                  chunk's rows.
//   k_bkm_fold     per child, the chunks in order onto an accumulator that
//                  starts at zero; the last group adds the accumulator into
//                  the caller's sums and the row count into count.  The
//                  workspace holds a group of chunks: a smaller one means more
//                  launches of the pair and the same chain, so the same bits.
//   k_bkm_predict  the descent: lanes sit at their own nodes; per level the
//                  tile goes through LDS as in k_bkm_assign against the two
//                  children (right only under <: Scala's minBy keeps the first
//                  minimum), until every row of the tile is at a leaf.
// No atomics on doubles, every sum has one fixed order: two calls on the same
// inputs give the same bits.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "common.hpp"
#include "kmeans_sums.hpp"

enum { BKM_RULE_NONE = 0, BKM_RULE_NORM = 1, BKM_RULE_WEIGHT = 2, BKM_RULE_SLOT = 3 };

struct cyc_bkm_plan_s {
  std::mutex mu;
  int d = 0;
  int64_t wsBytes = 0;
  cyc::kmsums::SortScratch sort;
  cyc::DeviceBuffer table, key, ws, acc, bad, nodes;
};

namespace {

using cyc::kmsums::kChunkRows;

constexpr int kTileRows = 256;              // rows per k_bkm_assign / k_bkm_predict workgroup
constexpr int kPanel = 16;                  // columns of the tile staged in LDS at a time
constexpr int kPanelStride = kPanel + 1;    // doubles per staged row (odd: no bank conflict)
constexpr int kColsPerBlock = 1024;         // columns per k_bkm_chunk workgroup (4 per thread)
constexpr int kMaxChildren = 4096;          // K, below the sort's LDS histogram bound
constexpr int kMaxNodes = 1 << 20;
constexpr int64_t kDefaultWorkspace = (int64_t)256 << 20;
constexpr unsigned long long kNoBad = ~0ull;
static_assert(kMaxChildren + 1 <= cyc::kmsums::kMaxK, "children + the parked cluster are sorted");
static_assert(kTileRows * kPanel % 256 == 0, "a panel is a whole number of loads per thread");

__device__ __forceinline__ void bkm_flag(unsigned long long* bad, int64_t row, int rule) {
  atomicMin(bad, (unsigned long long)row * 4ull + (unsigned long long)rule);
}

__global__ __launch_bounds__(256) void k_bkm_check(const double* __restrict__ xnorm,
                                                   const double* __restrict__ w, int64_t n,
                                                   unsigned long long* __restrict__ bad) {
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < n; r += (int64_t)gridDim.x * 256) {
    const double xn = xnorm[r];
    if (!(xn - xn == 0.0)) bkm_flag(bad, r, BKM_RULE_NORM);
    if (w) {
      const double wv = w[r];
      if (!(wv > 0.0 && wv - wv == 0.0)) bkm_flag(bad, r, BKM_RULE_WEIGHT);
    }
  }
}

// The sequential sqdist of this thread's row (r0 + threadIdx.x) to the centers
// pl and pr, columns ascending: dl, dr.  Every thread of the workgroup calls
// it; live: the row is loaded and summed (a row that is not live is in no
// bounds relation to n, and its pl / pr are not read).
__device__ __forceinline__ void tile_sqdist(const double* __restrict__ X, int64_t r0, int d,
                                            bool live, const double* __restrict__ pl,
                                            const double* __restrict__ pr, double* tile,
                                            int* liveS, double& dl, double& dr) {
  constexpr int PER = kTileRows * kPanel / 256;
  const int tid = threadIdx.x;
  liveS[tid] = live ? 1 : 0;
  __syncthreads();
  double v[PER];
  auto load = [&](int j0) {
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const int e = tid + 256 * u, row = e / kPanel, j = j0 + e % kPanel;
      v[u] = 0.0;
      // nontemporal: a row is read once per pass
      if (liveS[row] && j < d) v[u] = __builtin_nontemporal_load(&X[(r0 + row) * d + j]);
    }
  };
  load(0);
  dl = dr = 0.0;
  for (int j0 = 0; j0 < d; j0 += kPanel) {
    __syncthreads();   // the previous panel is consumed
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const int e = tid + 256 * u;
      tile[(e / kPanel) * kPanelStride + e % kPanel] = v[u];
    }
    __syncthreads();
    if (j0 + kPanel < d) load(j0 + kPanel);
    if (!live) continue;
    const double* row = tile + tid * kPanelStride;
    if (j0 + kPanel <= d) {
#pragma unroll
      for (int c = 0; c < kPanel; ++c) {
        const double x = row[c];
        const double a = dsub(pl[j0 + c], x), b = dsub(pr[j0 + c], x);
        dl = dadd(dl, dmul(a, a));
        dr = dadd(dr, dmul(b, b));
      }
    } else {
      for (int c = 0; j0 + c < d; ++c) {
        const double x = row[c];
        const double a = dsub(pl[j0 + c], x), b = dsub(pr[j0 + c], x);
        dl = dadd(dl, dmul(a, a));
        dr = dadd(dr, dmul(b, b));
      }
    }
  }
}

// slot (null: every row in slot 0) and newSlot may be the same array.
__global__ __launch_bounds__(256) void k_bkm_assign(
    const double* __restrict__ X, const double* __restrict__ xnorm, const int32_t* slot, int64_t n,
    int d, int numSlots, const int32_t* __restrict__ table, int K, const double* __restrict__ C,
    const double* __restrict__ cnorm, int32_t* newSlot, int32_t* __restrict__ key,
    unsigned long long* __restrict__ bad) {
  __shared__ double tile[kTileRows * kPanelStride];
  __shared__ int liveS[kTileRows];
  const int64_t r0 = (int64_t)blockIdx.x * kTileRows, r = r0 + threadIdx.x;
  int cl = -1, cr = -1, keep = -1;
  if (r < n) {
    const int s = slot ? slot[r] : 0;
    if ((unsigned)s < (unsigned)numSlots) {
      cl = table[3 * s];
      cr = table[3 * s + 1];
      keep = table[3 * s + 2];
    } else {
      // never an index: the row stays where it is and the call fails
      bkm_flag(bad, r, BKM_RULE_SLOT);
      keep = s;
    }
  }
  const bool two = cl >= 0 && cr >= 0;
  if (!__syncthreads_or(two)) {
    // no row of the tile has two children on offer: nothing is loaded
    if (r < n) {
      const int pick = cl >= 0 ? cl : cr >= 0 ? cr : keep;
      newSlot[r] = pick;
      if (key) key[r] = (pick >= 0 && pick < K) ? pick : K;
    }
    return;
  }
  double dl, dr;
  tile_sqdist(X, r0, d, two, C + (int64_t)(two ? cl : 0) * d, C + (int64_t)(two ? cr : 0) * d,
              tile, liveS, dl, dr);
  if (r >= n) return;
  int pick = cl >= 0 ? cl : cr >= 0 ? cr : keep;
  if (two) {
    // DistanceMeasure.scala:318-340 over [left, right]
    const double xn = xnorm[r];
    double best = INFINITY;
    int idx = 0;
    double lb = dsub(cnorm[cl], xn);
    lb = dmul(lb, lb);
    if (lb < best && dl < best) {
      best = dl;
      idx = 0;
    }
    lb = dsub(cnorm[cr], xn);
    lb = dmul(lb, lb);
    if (lb < best && dr < best) {
      best = dr;
      idx = 1;
    }
    pick = idx ? cr : cl;
  }
  newSlot[r] = pick;
  if (key) key[r] = (pick >= 0 && pick < K) ? pick : K;
}

// Chunk ch of the sorted rows (a child's, ch < chunkStart[K]) into
// part[(ch - g0) (d + 2)]: [sum of w | sum of (norm norm) w | sum of w x (d)].
template <int NJ>
__global__ __launch_bounds__(256) void k_bkm_chunk(
    const double* __restrict__ X, int d, const double* __restrict__ w,
    const double* __restrict__ xnorm, const int32_t* __restrict__ perm,
    const int64_t* __restrict__ cstart, const int64_t* __restrict__ chunkStart, int K, int64_t g0,
    double* __restrict__ part) {
  __shared__ int32_t rowsS[kChunkRows];
  __shared__ double redW[256], redQ[256];
  const int64_t ch = g0 + blockIdx.x;
  if (ch >= chunkStart[K]) return;
  int lo = 0, hi = K;   // the child: the last c with chunkStart[c] <= ch
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (chunkStart[mid] <= ch) lo = mid; else hi = mid;
  }
  const int c = lo;
  const int64_t first = cstart[c] + (ch - chunkStart[c]) * kChunkRows;
  const int cnt = (int)(min<int64_t>(cstart[c + 1], first + kChunkRows) - first);
  const int tid = threadIdx.x;
  for (int i = tid; i < cnt; i += 256) rowsS[i] = perm[first + i];
  __syncthreads();
  const int jb = blockIdx.y * kColsPerBlock;
  double* out = part + (int64_t)blockIdx.x * (d + 2);
  double s[NJ];
#pragma unroll
  for (int u = 0; u < NJ; ++u) s[u] = 0.0;
  for (int p0 = 0; p0 < cnt; p0 += 8) {
    double xv[8][NJ];
#pragma unroll
    for (int v = 0; v < 8; ++v) {
      const int64_t r = rowsS[min(p0 + v, cnt - 1)];
#pragma unroll
      for (int u = 0; u < NJ; ++u) {
        const int j = jb + tid + 256 * u;
        xv[v][u] = j < d ? __builtin_nontemporal_load(&X[r * d + j]) : 0.0;
      }
    }
#pragma unroll
    for (int v = 0; v < 8; ++v) {
      if (p0 + v < cnt) {
        const double wr = w ? w[rowsS[p0 + v]] : 1.0;
#pragma unroll
        for (int u = 0; u < NJ; ++u)
          s[u] = w ? dadd(s[u], dmul(wr, xv[v][u])) : dadd(s[u], xv[v][u]);
      }
    }
  }
#pragma unroll
  for (int u = 0; u < NJ; ++u) {
    const int j = jb + tid + 256 * u;
    if (j < d) out[2 + j] = s[u];
  }
  if (blockIdx.y != 0) return;
  double wv = 0.0, qv = 0.0;
  if (tid < cnt) {
    const int64_t r = rowsS[tid];
    const double xn = xnorm[r];
    wv = w ? w[r] : 1.0;
    qv = dmul(dmul(xn, xn), wv);
  }
  redW[tid] = wv;
  redQ[tid] = qv;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (tid < off) {
      redW[tid] = dadd(redW[tid], redW[tid + off]);
      redQ[tid] = dadd(redQ[tid], redQ[tid + off]);
    }
    __syncthreads();
  }
  if (tid == 0) {
    out[0] = redW[0];
    out[1] = redQ[0];
  }
}

// acc [wsum (K) | sumSq (K) | sums (K x d)] += child blockIdx.x's chunks of the
// group [g0, g0 + group), in order; last: sums += acc, count += the rows.
__global__ __launch_bounds__(256) void k_bkm_fold(const double* __restrict__ part,
                                                  const int64_t* __restrict__ cstart,
                                                  const int64_t* __restrict__ chunkStart, int K,
                                                  int d, int64_t g0, int64_t group, int last,
                                                  double* __restrict__ acc,
                                                  double* __restrict__ sums,
                                                  int64_t* __restrict__ count) {
  const int c = blockIdx.x;
  const int e = blockIdx.y * 256 + threadIdx.x;
  const int64_t len = d + 2;
  if (e >= len) return;
  const int64_t a = max<int64_t>(chunkStart[c], g0), b = min<int64_t>(chunkStart[c + 1], g0 + group);
  const int64_t at = e == 0 ? c : e == 1 ? (int64_t)K + c : 2 * (int64_t)K + (int64_t)c * d + (e - 2);
  double s = acc[at];
  int64_t ch = a;
  // chunk order kept; 16 chunks' loads in flight per step
  for (; ch + 16 <= b; ch += 16) {
    double v[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) v[u] = part[(ch - g0 + u) * len + e];
#pragma unroll
    for (int u = 0; u < 16; ++u) s = dadd(s, v[u]);
  }
  for (; ch < b; ++ch) s = dadd(s, part[(ch - g0) * len + e]);
  acc[at] = s;
  if (!last) return;
  sums[at] = dadd(sums[at], s);
  if (e == 0) count[c] += cstart[c + 1] - cstart[c];
}

// nodes: [firstChild | numChildren | leafIndex], numNodes each; the children
// of a node are firstChild, firstChild + 1.  rootLeaf: the tree is one leaf.
__global__ __launch_bounds__(256) void k_bkm_predict(
    const double* __restrict__ X, int64_t n, int d, int numNodes,
    const int32_t* __restrict__ nodes, const double* __restrict__ C, int rootLeaf,
    int32_t* __restrict__ pred, double* __restrict__ cost) {
  __shared__ double tile[kTileRows * kPanelStride];
  __shared__ int liveS[kTileRows];
  const int32_t* firstChild = nodes;
  const int32_t* numChildren = nodes + numNodes;
  const int32_t* leafIndex = nodes + 2 * (int64_t)numNodes;
  const int64_t r0 = (int64_t)blockIdx.x * kTileRows, r = r0 + threadIdx.x;
  int node = 0;
  double cst = 0.0, dl, dr;
  if (rootLeaf) {
    tile_sqdist(X, r0, d, r < n, C, C, tile, liveS, dl, dr);
    cst = dl;
  } else {
    // a child's index is above its parent's (checked by the host): it ends
    for (;;) {
      const int nc = r < n ? numChildren[node] : 0;
      if (!__syncthreads_or(nc > 0)) break;
      const int cl = nc > 0 ? firstChild[node] : 0, cr = nc > 1 ? cl + 1 : cl;
      tile_sqdist(X, r0, d, nc > 0, C + (int64_t)cl * d, C + (int64_t)cr * d, tile, liveS, dl, dr);
      if (nc > 0) {
        const bool right = nc > 1 && dr < dl;
        node = right ? cr : cl;
        cst = right ? dr : dl;
      }
    }
  }
  if (r >= n) return;
  pred[r] = leafIndex[node];
  if (cost) cost[r] = cst;
}

int reset_bad(cyc_bkm_plan_s* p, hipStream_t st) {
  if (int rc = p->bad.reserve(sizeof(unsigned long long))) return rc;
  CYC_HIP(hipMemsetAsync(p->bad.ptr, 0xff, sizeof(unsigned long long), st));
  return CYC_OK;
}

int read_bad(cyc_bkm_plan_s* p, hipStream_t st, int64_t* row, int* rule) {
  unsigned long long v = 0;
  CYC_HIP(hipMemcpyAsync(&v, p->bad.ptr, sizeof(v), hipMemcpyDeviceToHost, st));
  CYC_HIP(hipStreamSynchronize(st));
  *row = v == kNoBad ? -1 : (int64_t)(v >> 2);
  *rule = v == kNoBad ? BKM_RULE_NONE : (int)(v & 3);
  return CYC_OK;
}

int refuse(int64_t row, int rule, const double* xnorm, const double* w, const int32_t* slot,
           int numSlots) {
  const std::string at = " (row " + std::to_string(row) + ")";
  double v = 0.0;
  if (rule == BKM_RULE_NORM) {
    CYC_HIP(hipMemcpy(&v, xnorm + row, sizeof(v), hipMemcpyDeviceToHost));
    cyc::set_error("requirement failed: the norm of a row must be finite but got " +
                   cyc::java_double(v) + "." + at);
  } else if (rule == BKM_RULE_WEIGHT) {
    CYC_HIP(hipMemcpy(&v, w + row, sizeof(v), hipMemcpyDeviceToHost));
    cyc::set_error("requirement failed: illegal weight value: " + cyc::java_double(v) +
                   ". weight must be finite and > 0.0." + at);
  } else {
    int32_t s = 0;
    if (slot) CYC_HIP(hipMemcpy(&s, slot + row, sizeof(s), hipMemcpyDeviceToHost));
    cyc::set_error("requirement failed: slot " + std::to_string(s) + " is outside [0, " +
                   std::to_string(numSlots) + ")." + at);
  }
  return CYC_ERR_INVALID_ARG;
}

template <class F>
void with_nj(int nj, F&& f) {
  if (nj <= 1) f(std::integral_constant<int, 1>{});
  else if (nj == 2) f(std::integral_constant<int, 2>{});
  else f(std::integral_constant<int, 4>{});
}

int64_t chunks_per_launch(const cyc_bkm_plan_s* p) {
  return std::max<int64_t>(1, p->wsBytes / (8 * ((int64_t)p->d + 2)));
}

// count / sums += the summary of the children among key[] (0 .. K - 1; K: the
// rows that take no part)
int summarize(cyc_bkm_plan_s* p, const double* X, const double* xnorm, const double* w, int64_t n,
              int K, const int32_t* key, int64_t* count, double* sums, hipStream_t st) {
  const int d = p->d;
  int64_t maxChunks = 0;
  // d = 0: the sort's own chunk buffers are not used here
  if (int rc = cyc::kmsums::sort_clusters(p->sort, key, n, 0, K + 1, st, maxChunks)) return rc;
  const int64_t group = std::min(maxChunks, chunks_per_launch(p));
  const int64_t len = (int64_t)d + 2, accLen = (int64_t)K * len;
  if (int rc = p->ws.reserve(sizeof(double) * (size_t)(group * len))) return rc;
  if (int rc = p->acc.reserve(sizeof(double) * (size_t)accLen)) return rc;
  CYC_HIP(hipMemsetAsync(p->acc.ptr, 0, sizeof(double) * (size_t)accLen, st));
  const int32_t* perm = (const int32_t*)p->sort.perm.ptr;
  const int64_t* cstart = (const int64_t*)p->sort.cstart.ptr;
  const int64_t* chunkStart = (const int64_t*)p->sort.chunkStart.ptr;
  const int colBlocks = (d + kColsPerBlock - 1) / kColsPerBlock;
  const int nj = (std::min(d, kColsPerBlock) + 255) / 256;
  // the chunk count is on the device: the bound is launched, the surplus leaves
  for (int64_t g0 = 0; g0 < maxChunks; g0 += group) {
    const int64_t gc = std::min(group, maxChunks - g0);
    {
      cyc::KernelTimer timer("k_bkm_chunk", st);
      with_nj(nj, [&](auto NJ) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_bkm_chunk<decltype(NJ)::value>),
                           dim3((unsigned)gc, (unsigned)colBlocks), dim3(256), 0, st, X, d, w,
                           xnorm, perm, cstart, chunkStart, K, g0, (double*)p->ws.ptr);
      });
      CYC_LAUNCH_CHECK("k_bkm_chunk");
    }
    cyc::KernelTimer timer("k_bkm_fold", st);
    hipLaunchKernelGGL(k_bkm_fold, dim3((unsigned)K, (unsigned)((len + 255) / 256)), dim3(256), 0,
                       st, (const double*)p->ws.ptr, cstart, chunkStart, K, d, g0, gc,
                       g0 + gc >= maxChunks ? 1 : 0, (double*)p->acc.ptr, sums, count);
    CYC_LAUNCH_CHECK("k_bkm_fold");
  }
  return CYC_OK;
}

}  // namespace

extern "C" {

int cyc_bkm_plan_create(int32_t numFeatures, int64_t workspaceBytes, cyc_bkm_plan* plan) {
  CYC_REQUIRE(plan != nullptr, "plan must not be null");
  CYC_REQUIRE(numFeatures >= 1,
              "numFeatures must be positive but got " + std::to_string(numFeatures));
  CYC_REQUIRE((int64_t)numFeatures <= (int64_t)65535 * kColsPerBlock,
              "BisectingKMeans supports up to " + std::to_string((int64_t)65535 * kColsPerBlock) +
                  " features but got " + std::to_string(numFeatures));
  CYC_REQUIRE(workspaceBytes >= 0, "workspaceBytes must not be negative");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    cyc::set_error("no HIP device visible");
    return CYC_ERR_NO_DEVICE;
  }
  auto* p = new cyc_bkm_plan_s();
  p->d = numFeatures;
  p->wsBytes = workspaceBytes ? workspaceBytes : kDefaultWorkspace;
  *plan = p;
  return CYC_OK;
}

int cyc_bkm_plan_destroy(cyc_bkm_plan plan) {
  delete plan;
  return CYC_OK;
}

int64_t cyc_bkm_tile_rows(cyc_bkm_plan plan) { return plan ? kTileRows : -1; }
int64_t cyc_bkm_panel_cols(cyc_bkm_plan plan) { return plan ? kPanel : -1; }
int64_t cyc_bkm_chunk_rows(cyc_bkm_plan plan) { return plan ? kChunkRows : -1; }
int64_t cyc_bkm_chunks_per_launch(cyc_bkm_plan plan) {
  return plan ? chunks_per_launch(plan) : -1;
}
int64_t cyc_bkm_max_children(cyc_bkm_plan plan) { return plan ? kMaxChildren : -1; }

int cyc_bkm_step_dev(cyc_bkm_plan plan, const double* X, const double* xnorm, const double* w,
                     int64_t nrows, const int32_t* slot, int32_t numSlots, const int32_t* table,
                     int32_t numChildren, const double* centers, const double* cnorm,
                     int32_t* newSlot, int64_t* count, double* sums, int32_t check,
                     int64_t* badRow, int32_t* badRule, void* stream) {
  CYC_REQUIRE(plan != nullptr, "plan must not be null");
  CYC_REQUIRE(nrows >= 0 && nrows <= INT32_MAX, "0 <= nrows <= 2147483647");
  CYC_REQUIRE(numSlots >= 1 && table != nullptr, "a table of at least one slot");
  CYC_REQUIRE(numChildren >= 1 && numChildren <= kMaxChildren,
              "1 to " + std::to_string(kMaxChildren) + " children but got " +
                  std::to_string(numChildren));
  CYC_REQUIRE((count == nullptr) == (sums == nullptr), "count and sums: both or neither");
  const int K = numChildren;
  for (int s = 0; s < numSlots; ++s) {
    const int32_t l = table[3 * s], r = table[3 * s + 1], keep = table[3 * s + 2];
    CYC_REQUIRE(l >= -1 && l < K && r >= -1 && r < K,
                "the children of slot " + std::to_string(s) + " must be -1 or in [0, " +
                    std::to_string(K) + ")");
    CYC_REQUIRE(keep == -1 || keep >= K,
                "keepNew of slot " + std::to_string(s) + " must be -1 or at least " +
                    std::to_string(K));
    CYC_REQUIRE(l >= 0 || r >= 0 || keep >= 0,
                "slot " + std::to_string(s) + " offers no child and no keepNew");
  }
  if (badRow) *badRow = -1;
  if (badRule) *badRule = BKM_RULE_NONE;
  if (nrows == 0) return CYC_OK;
  CYC_REQUIRE(X != nullptr && xnorm != nullptr && centers != nullptr && cnorm != nullptr &&
                  newSlot != nullptr,
              "non-null rows, norms, centers, center norms and newSlot");
  cyc_bkm_plan_s* p = plan;
  hipStream_t st = cyc::as_stream(stream);
  std::lock_guard<std::mutex> g(p->mu);
  if (int rc = reset_bad(p, st)) return rc;
  if (int rc = p->table.reserve(sizeof(int32_t) * 3 * (size_t)numSlots)) return rc;
  // stream-ordered after the last call's kernels; the source is pageable, so
  // the copy has left the caller's array when the call returns
  CYC_HIP(hipMemcpyAsync(p->table.ptr, table, sizeof(int32_t) * 3 * (size_t)numSlots,
                         hipMemcpyHostToDevice, st));
  int32_t* key = nullptr;
  if (sums) {
    if (int rc = p->key.reserve(sizeof(int32_t) * (size_t)nrows)) return rc;
    key = (int32_t*)p->key.ptr;
  }
  if (check) {
    cyc::KernelTimer timer("k_bkm_check", st);
    hipLaunchKernelGGL(k_bkm_check, dim3((unsigned)std::min<int64_t>((nrows + 255) / 256, 4096)),
                       dim3(256), 0, st, xnorm, w, nrows, (unsigned long long*)p->bad.ptr);
    CYC_LAUNCH_CHECK("k_bkm_check");
  }
  {
    cyc::KernelTimer timer("k_bkm_assign", st);
    hipLaunchKernelGGL(k_bkm_assign, dim3((unsigned)((nrows + kTileRows - 1) / kTileRows)),
                       dim3(256), 0, st, X, xnorm, slot, nrows, p->d, numSlots,
                       (const int32_t*)p->table.ptr, K, centers, cnorm, newSlot, key,
                       (unsigned long long*)p->bad.ptr);
    CYC_LAUNCH_CHECK("k_bkm_assign");
  }
  if (sums)
    if (int rc = summarize(p, X, xnorm, w, nrows, K, key, count, sums, st)) return rc;
  int64_t row = -1;
  int rule = 0;
  if (int rc = read_bad(p, st, &row, &rule)) return rc;
  if (rule == BKM_RULE_NONE) return CYC_OK;
  if (badRow) *badRow = row;
  if (badRule) *badRule = rule;
  return refuse(row, rule, xnorm, w, slot, numSlots);
}

int cyc_bkm_predict_dev(cyc_bkm_plan plan, const double* X, int64_t nrows, int32_t numNodes,
                        const int32_t* firstChild, const int32_t* numChildren,
                        const int32_t* leafIndex, const double* centers, int32_t* pred,
                        double* cost, void* stream) {
  CYC_REQUIRE(plan != nullptr, "plan must not be null");
  CYC_REQUIRE(nrows >= 0, "nrows >= 0");
  CYC_REQUIRE(numNodes >= 1 && numNodes <= kMaxNodes,
              "1 to " + std::to_string(kMaxNodes) + " nodes but got " + std::to_string(numNodes));
  CYC_REQUIRE(firstChild != nullptr && numChildren != nullptr && leafIndex != nullptr,
              "non-null node arrays");
  for (int i = 0; i < numNodes; ++i) {
    const int32_t nc = numChildren[i], fc = firstChild[i];
    CYC_REQUIRE(nc >= 0 && nc <= 2, "node " + std::to_string(i) + " must have 0, 1 or 2 children");
    if (nc > 0)
      CYC_REQUIRE(fc > i && (int64_t)fc + nc <= numNodes,
                  "the children of node " + std::to_string(i) +
                      " must follow it and lie inside the tree");
    else
      CYC_REQUIRE(leafIndex[i] >= 0, "leaf node " + std::to_string(i) + " needs a leaf index");
  }
  if (nrows == 0) return CYC_OK;
  CYC_REQUIRE(X != nullptr && centers != nullptr && pred != nullptr,
              "non-null rows, centers and pred");
  cyc_bkm_plan_s* p = plan;
  hipStream_t st = cyc::as_stream(stream);
  std::lock_guard<std::mutex> g(p->mu);
  const size_t nb = sizeof(int32_t) * (size_t)numNodes;
  if (int rc = p->nodes.reserve(3 * nb)) return rc;
  char* nd = (char*)p->nodes.ptr;
  CYC_HIP(hipMemcpyAsync(nd, firstChild, nb, hipMemcpyHostToDevice, st));
  CYC_HIP(hipMemcpyAsync(nd + nb, numChildren, nb, hipMemcpyHostToDevice, st));
  CYC_HIP(hipMemcpyAsync(nd + 2 * nb, leafIndex, nb, hipMemcpyHostToDevice, st));
  cyc::KernelTimer timer("k_bkm_predict", st);
  hipLaunchKernelGGL(k_bkm_predict, dim3((unsigned)((nrows + kTileRows - 1) / kTileRows)),
                     dim3(256), 0, st, X, nrows, p->d, numNodes, (const int32_t*)p->nodes.ptr,
                     centers, numChildren[0] == 0 ? 1 : 0, pred, cost);
  CYC_LAUNCH_CHECK("k_bkm_predict");
  return CYC_OK;
}

}  // extern "C"
