// kmeans.hip -- the KMeans plan on gfx950 (MI355X): the C ABI of the Lloyd
// iteration body, its checks, and the host logic that strings the tiers
// together.  The kernels of each tier live in a unit of their own.
//
// Replaces mllib/clustering/KMeans.scala:275-334 (the mapPartitions body and
// its reduceByKey merge) and DistanceMeasure.scala:48-118, 189-203, 282-350.
//
// What a Euclidean Lloyd call (cyc_kmeans_accumulate_dev) runs, in order, all
// device-resident on one stream:
//   1. Center preparation (prep_all here; cyc::km8::centers_prepare_all,
//      kmeans_i8_centers.hip): the require(norm >= 0) check, computeStatistics
//      (0.25*dist^2 packed upper + row minima, bit-exact), the transposed
//      centers Ct (the fp64 MFMA B operand), the carried bounds' center drift
//      and neighbourhoods, the i8 center image and the screens' zeroed
//      counters, as three fused launches.  CYC_KMEANS_PREP=0, a row image of
//      d > 256 and the other entry points run the same bodies as separate
//      launches (require_enqueue, do_stats, bounds_prepare, do_assign).
//   2. Carried bounds (bounds_* here; kernels in kmeans_i8_lists.hip, the
//      re-check in kmeans_i8_cands.hip): with a row
//      image, rows whose bounds of the last call still certify their center
//      are kept; the others are listed for re-check or for the screens.
//   3. i8 exact-integer screens over the row image (cyc::km8::screen,
//      kmeans_i8.hip): one-limb pass and two-limb refinement, candidate
//      pass, three-limb candidate tier (kmeans_i8_cands.hip); screen_setup
//      here builds their arguments once per call.  Without a row image: the bf16x3 screen
//      (kmeans_fp64.hip) or none.
//   4. fp64 MFMA screen (cyc::kmfp64::launch_assign, kmeans_fp64.hip) over
//      the rows the screens before it queued, or over every row: a row whose
//      best center is separated from every other by more than a rigorous
//      error margin is decided; the rest are queued.
//   5. Exact tier (cyc::kmfp64::launch_exact, kmeans_fp64.hip): the
//      reference's findClosest-with-statistics loop restated instruction for
//      instruction for the queued rows (ties, near ties, NaN/Inf).
//   6. Cluster sums (kmeans_sums.hip): the incremental sums of the rows that
//      changed cluster (inc_accumulate; with carried bounds, unit weights, no
//      per-row costs) or the full pass (full_pass: stable counting sort,
//      fixed-order chunk sums and folds; deterministic run to run).
//   7. cyc_kmeans_update_dev (cyc::kmsums::update_centers): centroid =
//      (1/w)*sum, new norm, convergence flag.
// do_assign runs 3-5 for every dense entry point.  The cosine plan's tiers are
// in kmeans_cos.hip (cos_* here), sparse rows' in kmeans_sparse.hip, the
// silhouette's in silhouette.hip.
//
// State carried from one call of a fit to the next lives in the row image
// (cyc_kmeans_rows_s): the bounds and candidate sets (b*) and the incremental
// sums (inc).  The plan (cyc_kmeans_plan_s) holds sizes and scratch only.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <mutex>
#include <utility>
#include <vector>

#include "common.hpp"
#include "kmeans_centers.hpp"
#include "kmeans_i8.hpp"
#include "kmeans_cos.hpp"
#include "kmeans_fp64.hpp"
#include "kmeans_sparse.hpp"
#include "kmeans_sums.hpp"
#include "silhouette.hpp"

namespace {

using cyc::kmsums::kChunkRows;
using cyc::kmsums::kMaxK;

// --------------------------------------------------------------- switches
// Every environment switch this file reads, with its default and when it is
// read.  (CYC_KMEANS_DUMP and CYCLONE_STRICT_PARITY are read in common.hpp;
// the i8 screen's own switches, each through one accessor of kmeans_i8.hpp:
//   CYC_KMEANS_PREP     on     kmeans_i8_centers.hip  prep_fused(); 0: the separate launches
//   CYC_KMEANS_RECHECK  unset  kmeans_i8_lists.hip    recheck_two_phase(); 1: one-phase re-check
//   CYC_KMEANS_SIDE     unset  kmeans_i8.hip          screen_side_stream(); 1: the three-limb
//                                                     pass beside the candidate pass
//   CYC_QUANT_PF        on     kmeans_i8_rows.hip     rows_quantize(); 0: the row-at-a-time
//                                                     image kernel
// all read once.)
//   name                    default  read          meaning
//   CYC_KMEANS_ASSIGN       unset    plan create   1/2/3: the screen tier of a plan without
//                                                  a row image (test hook, Sizing::variant)
//   CYC_KMEANS_CANDS3       on       per call      0: no three-limb candidate tier
//   CYC_KMEANS_NO_REFINE    unset    per call      set: no one-limb pass + refinement, and
//                                                  so no carried bounds
//   CYC_KMEANS_NO_STAGE     unset    per call      set: the screens append straight to
//                                                  their lists (no sharded stage)
//   CYC_KMEANS_BOUNDS       on       once          0: no carried bounds
//   CYC_KMEANS_NBR          on       once          0: no neighbourhood re-checks (state 3)
//   CYC_KMEANS_INCR         on       once          0: no incremental cluster sums
//   CYC_KMEANS_EXACT_SPLIT  on       once          0: k_assign_exact alone in the exact tier
//   CYC_KMEANS_LIST_BM      on       once          0: queued rows in the plan's tile, not 16
//   CYC_KMEANS_DUMP_CALL    10       once          the bounded call whose state is dumped
bool env_is0(const char* name) {
  const char* e = std::getenv(name);
  return e && e[0] == '0';
}
int sw_assign_variant() {
  const char* v = std::getenv("CYC_KMEANS_ASSIGN");
  return v ? std::atoi(v) : 0;
}
bool sw_cands3() { return !env_is0("CYC_KMEANS_CANDS3"); }
bool sw_refine() { return std::getenv("CYC_KMEANS_NO_REFINE") == nullptr; }
bool sw_stage() { return std::getenv("CYC_KMEANS_NO_STAGE") == nullptr; }
bool sw_bounds() {
  static const bool on = !env_is0("CYC_KMEANS_BOUNDS");
  return on;
}
bool sw_nbr() {
  static const bool on = !env_is0("CYC_KMEANS_NBR");
  return on;
}
bool sw_incr() {
  static const bool on = !env_is0("CYC_KMEANS_INCR");
  return on;
}
bool sw_exact_split() {
  static const bool on = !env_is0("CYC_KMEANS_EXACT_SPLIT");
  return on;
}
bool sw_list16() {
  static const bool on = !env_is0("CYC_KMEANS_LIST_BM");
  return on;
}
int sw_dump_call() {
  static const int call = [] {
    const char* e = std::getenv("CYC_KMEANS_DUMP_CALL");
    return e ? std::atoi(e) : 10;
  }();
  return call;
}

// ---------------------------------------------------------------- helpers
// Vectors.norm(dense, 2) (Vectors.scala:489-514): one thread per row, the
// squares summed in column order.  256 rows per block; 16-column slices of
// them staged through two LDS buffers (row stride 17 doubles: the row-wise
// reads hit distinct banks), loaded coalesced (16 consecutive threads read
// one row's 128 bytes) one slice ahead in registers: one barrier per slice.
constexpr int kNormRows = 256, kNormCols = 16, kNormStride = kNormCols + 1;
__global__ __launch_bounds__(kNormRows) void k_row_norms(const double* __restrict__ X, int64_t n,
                                                         int d, double* __restrict__ norms) {
  __shared__ double tile[2][kNormRows * kNormStride];
  const int t = threadIdx.x;
  const int64_t row0 = (int64_t)blockIdx.x * kNormRows;
  constexpr int PER = kNormRows * kNormCols / kNormRows;   // loads per thread per slice
  double v[PER];
  // element e = t + 256 i of a slice: row e / 16, column e % 16
  auto load = [&](int c0) {
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int e = t + kNormRows * i, r = e / kNormCols, c = c0 + e % kNormCols;
      const int64_t gr = row0 + r;
      v[i] = (gr < n && c < d) ? __builtin_nontemporal_load(&X[gr * d + c]) : 0.0;
    }
  };
  auto store = [&](double* b) {
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int e = t + kNormRows * i;
      b[(e / kNormCols) * kNormStride + e % kNormCols] = v[i];
    }
  };
  double s = 0.0;
  load(0);
  store(tile[0]);
  int buf = 0;
  for (int c0 = 0; c0 < d; c0 += kNormCols) {
    if (c0 + kNormCols < d) load(c0 + kNormCols);
    __syncthreads();   // slice c0 in tile[buf]; every thread done with tile[buf ^ 1]
    const double* row = tile[buf] + t * kNormStride;
    const int lim = min(kNormCols, d - c0);
    for (int c = 0; c < lim; ++c) s = dadd(s, dmul(row[c], row[c]));
    if (c0 + kNormCols < d) store(tile[buf ^ 1]);
    buf ^= 1;
  }
  const int64_t gr = row0 + t;
  if (gr < n) norms[gr] = __builtin_sqrt(s);
}

__global__ void k_center_transpose(const double* __restrict__ C, int k, int d, int d4, int kpad,
                                   double* __restrict__ Ct) {
  int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t total = (int64_t)d4 * kpad;
  if (idx >= total) return;
  int j = (int)(idx / kpad), i = (int)(idx % kpad);
  Ct[idx] = (i < k && j < d) ? C[(int64_t)i * d + j] : 0.0;
}

// kInfBits, the statistics' tile sizes and the bodies of the center kernels
// below live in kmeans_centers.hpp (cyc::kmc): centers_prepare_all
// (kmeans_i8_centers.hip) runs the same bodies as jobs of its fused launches.
using cyc::kmc::kInfBits;
using cyc::kmc::kStT;
using cyc::kmc::kStC;

__global__ void k_fill_u64(unsigned long long* __restrict__ p, int n, unsigned long long v) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}
// k_center_transpose and the statistics' dmin fill in one launch
__global__ void k_center_transpose_fill(const double* __restrict__ C, int k, int d, int d4,
                                        int kpad, double* __restrict__ Ct,
                                        unsigned long long* __restrict__ p, unsigned long long v) {
  cyc::kmc::center_transpose_fill(C, k, d, d4, kpad, Ct, p, v, blockIdx.x, threadIdx.x);
}
// two counters zeroed by one launch (two fills before)
__global__ void k_zero2(unsigned int* __restrict__ a, unsigned int* __restrict__ b) {
  cyc::kmc::zero2(a, b, threadIdx.x);
}

// computeStatistics pairs and diagonal (cyc::kmc::stats_pairs / stats_diag)
__global__ __launch_bounds__(256) void k_stats_pairs(const double* __restrict__ C, int k, int d,
                                                     int tps, double* __restrict__ packed,
                                                     unsigned long long* __restrict__ dmin) {
  cyc::kmc::stats_pairs(C, k, d, tps, packed, dmin, blockIdx.x, threadIdx.x);
}

__global__ void k_stats_diag(int k, double* __restrict__ packed,
                             const unsigned long long* __restrict__ dmin) {
  cyc::kmc::stats_diag(k, packed, dmin, kInfBits, blockIdx.x, threadIdx.x);
}

// pointCost of a row no center reaches (NaN/Inf coordinates): findClosest
// without statistics keeps bestDistance = +Infinity (:321-337), while the
// recomputed sqdist to center 0 is NaN or +Infinity.
__global__ void k_nostats_cost_fix(int64_t n, double* __restrict__ cost) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r < n && __builtin_isnan(cost[r])) cost[r] = __builtin_inf();
}

// MLUtils.fastSquaredDistance's require(norm1 >= 0.0 && norm2 >= 0.0,
// "Both norms should be greater or equal to 0.0, ...") (mllib/util/
// MLUtils.scala:542-543), as a with-statistics Lloyd step meets it:
// computeStatistics (DistanceMeasure.scala:48-76) measures every center pair,
// so a center with a NaN norm fails (k >= 2), and findClosest (:282-287)
// measures (center 0, point) first for every point.  Other centers are only
// measured behind `lowerBound < bestDistance` (:295-297), which a NaN norm
// never passes; findClosest WITHOUT statistics (:318-340) therefore never
// fails.  A norm is NaN iff the vector holds a NaN (Vectors.scala:500-507).
// req[0]: lowest center holding a NaN, req[1]: lowest row with a NaN norm
// (~0 when none; set by the caller); req[2..4] as doubles: norm(c0),
// norm(c1), xnorm[0] -- the values the reference's message interpolates.
__global__ void k_require_norms(const double* __restrict__ C, int k, int d,
                                const double* __restrict__ xnorm, int64_t n,
                                unsigned long long* __restrict__ req) {
  cyc::kmc::require_norms(C, k, d, xnorm, n, req, gridDim.x, blockIdx.x, threadIdx.x);
}

// cost[r] = Vectors.sqdist(C[assign[r]], X[r]) (Vectors.scala:580-587): the
// distance findClosest returns for the chosen center.  One thread per row,
// the rows staged as in k_row_norms (256 rows, 16-column slices through two
// padded LDS buffers one slice ahead); the centers (L2-resident) read per
// thread.
__global__ __launch_bounds__(kNormRows) void k_row_cost(const double* __restrict__ X, int64_t n,
                                                        int d, const double* __restrict__ C,
                                                        const int32_t* __restrict__ assign,
                                                        double* __restrict__ cost) {
  __shared__ double tile[2][kNormRows * kNormStride];
  const int t = threadIdx.x;
  const int64_t row0 = (int64_t)blockIdx.x * kNormRows;
  const int64_t myr = row0 + t;
  const double* crow = myr < n ? C + (int64_t)assign[myr] * d : C;
  constexpr int PER = kNormCols;   // loads per thread per slice
  double v[PER];
  auto load = [&](int c0) {
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int e = t + kNormRows * i, r = e / kNormCols, c = c0 + e % kNormCols;
      const int64_t gr = row0 + r;
      v[i] = (gr < n && c < d) ? __builtin_nontemporal_load(&X[gr * d + c]) : 0.0;
    }
  };
  auto store = [&](double* b) {
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int e = t + kNormRows * i;
      b[(e / kNormCols) * kNormStride + e % kNormCols] = v[i];
    }
  };
  double s = 0.0;
  load(0);
  store(tile[0]);
  int buf = 0;
  for (int c0 = 0; c0 < d; c0 += kNormCols) {
    if (c0 + kNormCols < d) load(c0 + kNormCols);
    __syncthreads();   // slice c0 in tile[buf]; every thread done with tile[buf ^ 1]
    const double* row = tile[buf] + t * kNormStride;
    const int lim = min(kNormCols, d - c0);
    for (int c = 0; c < lim; ++c) {
      const double df = dsub(crow[c0 + c], row[c]);
      s = dadd(s, dmul(df, df));
    }
    if (c0 + kNormCols < d) store(tile[buf ^ 1]);
    buf ^= 1;
  }
  if (myr < n) cost[myr] = s;
}

}  // namespace

// ------------------------------------------------------------------ plan
struct cyc_kmeans_plan_s {
  int d = 0, k = 0;
  int measure = CYC_DISTANCE_EUCLIDEAN;   // DistanceMeasure of the plan
  // cosine: unit center directions for the screen, their norms, computed
  // center norms (statistics without given norms)
  cyc::DeviceBuffer cosV, cosVn, cosCn;
  bool dense_ok = true;     // d fits the LDS-resident dense assign kernels (d <= 1216)
  cyc::kmfp64::Sizing fp;   // the fp64 / bf16x3 screens' tiles and constants (kmeans_fp64.hpp)
  int64_t lastTier2 = 0;    // rows the bf16 screen queued (last counted call)
  int64_t lastExact = 0;    // rows the fp64 screen queued (last counted call)
  int64_t lastLimb3 = -1;   // rows the two-limb i8 pass left to the three-limb pass (-1: none)
  int64_t lastCands = -1;   // rows the two-limb i8 pass left to the candidate pass
  int64_t lastCands2 = -1;  // rows the three-limb candidate tier left to the fp64 pass
  bool cands3 = false;      // the last cand_args enabled the three-limb candidate tier
  cyc::DeviceBuffer cb3, cq3, ok3, list3, list3Count;
  // i8 exact-integer screen (kmeans_i8.hip), used with a row image
  int ktp8 = 0;
  // cb8: the center image (fragments, then the center-major copy, d <= 256)
  cyc::DeviceBuffer cb8, cq8, g8, prm8, scr8, list8Count;   // list8 = slowList (idle then)
  // candidate pass of the d <= 256 screen (kmeans_i8.hpp CandArgs)
  cyc::DeviceBuffer candRows, cands, candCount;
  // the rows the three-limb candidate tier leaves to the fp64 pass
  cyc::DeviceBuffer candRows2, cands2, candCount2;
  // the one-limb pass + two-limb refinement (kmeans_i8.hpp RefineArgs)
  cyc::DeviceBuffer cand1Rows, cand1, cand1Count, fullList, fullCount;
  // the screens' sharded append stage (kmeans_i8.hpp AppendStage)
  cyc::DeviceBuffer stgRowsA, stgRowsB, stgCandRows, stgCands, stgCounts;
  bool lastRefined = false;  // the last i8 screen ran the refinement path
  int64_t max_rows = 0;
  std::mutex mu;
  cyc::DeviceBuffer ct, stats, dmin, slowList, slowCount, assignTmp, costTmp;
  cyc::kmsums::SortScratch sort;   // the counting sort and the chunk sums (kmeans_sums.hpp)
  cyc::DeviceBuffer exactDist;   // k_exact_dist's distances (kmeans_fp64.hip)
  // require(norm1 >= 0.0 && norm2 >= 0.0) check (k_require_norms): device
  // result, its pinned host copy and the event that marks the copy landed
  cyc::DeviceBuffer req;
  // ClusteringEvaluator's Silhouette (silhouette.hpp): check flags, row
  // norms, per-block score partials
  cyc::DeviceBuffer silFlags, silNorms, silPart;
  unsigned long long* reqHost = nullptr;
  hipEvent_t reqEv = nullptr;
  ~cyc_kmeans_plan_s() {
    if (reqHost) (void)hipHostFree(reqHost);
    if (reqEv) (void)hipEventDestroy(reqEv);
  }
};

// Per-fit row image for the i8 screen (cyc_kmeans_rows_create).
struct cyc_kmeans_rows_s {
  const double* X = nullptr;
  int64_t n = 0;
  int d = 0;
  bool usable = false;     // d <= 512
  bool cosine = false;     // image of the unit directions x / |x|
  cyc::DeviceBuffer img, meta, unorm;   // unorm: |x / |x|| per row (cosine); |x| (Euclidean:
                                        // any summation order, the screens' margins)
  // Carried bounds of one fit's Lloyd iterations (kmeans_i8.hpp Bounds):
  // cyc_kmeans_accumulate_dev screens only the rows they cannot certify.
  // State: per row (ub, lb) and the assignment they certify (bAssign), the
  // centers they refer to (bCp, k x d); valid once a call has written them.
  bool bEnabled = true;    // cyc_kmeans_rows_set_bounds (CYC_KMEANS_BOUNDS=0: off by default)
  bool bValid = false;
  int bk = 0;
  cyc::DeviceBuffer bnd, bAssign, bCp, bDelta, bCcs, bPrm, bTmp, bCount, bList, bListCount, bCum;
  cyc::DeviceBuffer bTmp2, bCount2;   // the filter's state-1 list (k8::Bounds::collected)
  // carried candidate sets (kmeans_i8.hpp Bounds): outside bound, sets,
  // per-row state, the re-check list, its count and running total
  cyc::DeviceBuffer bLnc, bSets, bState, bRc, bRcCount, bRcCum;
  // the centers' neighbourhoods for the state-3 re-checks (k_center_nbrs)
  cyc::DeviceBuffer bNbr, bNbrR;
  int64_t bCalls = 0, bFullRows = 0;   // bounded calls; rows of their full (first) screens
  cyc::kmsums::IncState inc;   // incremental cluster sums (kmeans_sums.hpp)
  // The row half of the require(norm >= 0) check, kept with the image: the
  // rows and the norms passed with them are fixed for its lifetime, so the
  // first Lloyd call's result for (xnorm, n) -- req[1], the lowest row with a
  // NaN norm (~0: none), and req[4], the bits of xnorm[0] -- stands for the
  // later calls, which run the centers' half alone (require_check).
  struct RowVerdict {
    bool valid = false;
    const double* xnorm = nullptr;
    int64_t n = 0;
    unsigned long long rbad = ~0ull, x0 = 0;
    bool holds(const double* xn, int64_t rows) const { return valid && xnorm == xn && n == rows; }
  } verdict;
};

namespace {

// computeStatistics as three launches (k_center_transpose_fill, k_stats_pairs,
// k_stats_diag): cyc_kmeans_stats_dev, the silhouette and CYC_KMEANS_PREP=0;
// a Lloyd call runs the same bodies as jobs of prep_all.
int do_stats(cyc_kmeans_plan p, const double* C, hipStream_t st) {
  const int k = p->k, d = p->d;
  const int tps = (k + kStT - 1) / kStT;
  unsigned long long* dmin = (unsigned long long*)p->dmin.ptr;
  if (p->dense_ok) {
    const int64_t total = std::max<int64_t>((int64_t)p->fp.d4 * p->fp.kpad, k);
    hipLaunchKernelGGL(k_center_transpose_fill, dim3((unsigned)((total + 255) / 256)), dim3(256),
                       0, st, C, k, d, p->fp.d4, p->fp.kpad, (double*)p->ct.ptr, dmin, kInfBits);
    CYC_LAUNCH_CHECK("k_center_transpose_fill");
  } else {
    hipLaunchKernelGGL(k_fill_u64, dim3((k + 255) / 256), dim3(256), 0, st, dmin, k, kInfBits);
    CYC_LAUNCH_CHECK("k_fill_u64");
  }
  hipLaunchKernelGGL(k_stats_pairs, dim3((unsigned)(tps * (tps + 1) / 2)), dim3(256), 0, st, C, k,
                     d, tps, (double*)p->stats.ptr, dmin);
  CYC_LAUNCH_CHECK("k_stats_pairs");
  hipLaunchKernelGGL(k_stats_diag, dim3((k + 255) / 256), dim3(256), 0, st, k,
                     (double*)p->stats.ptr, (const unsigned long long*)dmin);
  CYC_LAUNCH_CHECK("k_stats_diag");
  return CYC_OK;
}

// The candidate pass's buffers and arguments (d <= 256 screens only).
int cand_args(cyc_kmeans_plan p, int64_t n, const double* X, const double* xnorm,
              const double* C, const double* cnorm, bool unit, cyc::km8::CandArgs& ca,
              bool& use) {
  use = cyc::km8::uses32(p->d);
  if (!use) return CYC_OK;
  int rc;
  if ((rc = p->candRows.reserve(sizeof(int32_t) * (size_t)n)) ||
      (rc = p->cands.reserve(sizeof(int32_t) * (size_t)n * cyc::km8::kCandMax)) ||
      (rc = p->candCount.reserve(64)))
    return rc;
  // Euclidean: a 2^-30 relative gap is far above fp64 rounding; the cosine
  // plan keeps the screen's own 2^-19 (the statistic's sqrt, kmeans_cos.hip)
  ca = cyc::km8::CandArgs{X, xnorm, C, cnorm, p->k, unit, unit ? 0x1p-19 : 0x1p-30,
                          (int32_t*)p->candRows.ptr, (int32_t*)p->cands.ptr,
                          (unsigned int*)p->candCount.ptr};
  // the three-limb candidate tier (CYC_KMEANS_CANDS3=0: every candidate row
  // straight to the fp64 pass)
  p->cands3 = sw_cands3();
  if (p->cands3) {
    if ((rc = p->candRows2.reserve(sizeof(int32_t) * (size_t)n)) ||
        (rc = p->cands2.reserve(sizeof(int32_t) * (size_t)n * cyc::km8::kCandMax)) ||
        (rc = p->candCount2.reserve(64)))
      return rc;
    ca.candRows2 = (int32_t*)p->candRows2.ptr;
    ca.cands2 = (int32_t*)p->cands2.ptr;
    ca.candCount2 = (unsigned int*)p->candCount2.ptr;
  }
  return CYC_OK;
}

// The one-limb pass + two-limb refinement of the d <= 256 screen, for k >
// 96 (below that the two-limb pass over every center is as cheap) and k <=
// 4096 (the refinement's union bitmap): whether a plan's screen runs it.
bool refine_on(cyc_kmeans_plan p) {
  return cyc::km8::uses32(p->d) && p->k > 96 && cyc::km8::tiles32(p->k) * 32 <= 4096 &&
         sw_refine();
}

int refine_args(cyc_kmeans_plan p, int64_t n, bool useCa, cyc::km8::RefineArgs& ra, bool& use) {
  const int kstride = cyc::km8::tiles32(p->k) * 32;
  use = useCa && refine_on(p);
  p->lastRefined = use;
  if (!use) return CYC_OK;
  int rc;
  if ((rc = p->cand1Rows.reserve(sizeof(int32_t) * (size_t)n)) ||
      (rc = p->cand1.reserve(sizeof(int32_t) * (size_t)n * cyc::km8::kCand1)) ||
      (rc = p->cand1Count.reserve(64)) ||
      (rc = p->fullList.reserve(sizeof(int32_t) * (size_t)n)) ||
      (rc = p->fullCount.reserve(64)))
    return rc;
  ra = cyc::km8::RefineArgs{kstride, (int32_t*)p->cand1Rows.ptr, (int32_t*)p->cand1.ptr,
                            (unsigned int*)p->cand1Count.ptr, (int32_t*)p->fullList.ptr,
                            (unsigned int*)p->fullCount.ptr};
  return CYC_OK;
}

// Carried bounds for a Lloyd call (cyc_kmeans_accumulate_dev): Euclidean
// rows with an image whose screen runs the one-limb pass (refine_args).
bool bounds_on(cyc_kmeans_plan p, cyc_kmeans_rows rows) {
  return rows && rows->usable && !rows->cosine && rows->bEnabled && sw_bounds() &&
         !cyc::strict_parity() && p->measure == CYC_DISTANCE_EUCLIDEAN && refine_on(p);
}

// no neighbourhood re-checks (state 3)
bool nbrOff() { return !sw_nbr() || cyc::strict_parity(); }

// Moves the bounds to the centers C (the drift against the last call's,
// then Cp = C) and lists the rows they cannot certify; bd for the screen.
// The first call of a fit (or after a change of k) screens every row.
// Three steps: bounds_reserve (buffers; carry: the state of the last call
// is usable), the center side (k_center_drift, k_drift_top and, inside
// bounds_filter, k_center_nbrs: separate launches here, jobs of prep_all's
// three launches in the fused form), bounds_lists (the row side).
int bounds_reserve(cyc_kmeans_plan p, cyc_kmeans_rows rows, int64_t n, hipStream_t st,
                   bool& carry) {
  namespace k8 = cyc::km8;
  const int k = p->k, d = p->d;
  int rc;
  if ((rc = rows->bnd.reserve(sizeof(float2) * (size_t)n)) ||
      (rc = rows->bAssign.reserve(sizeof(int32_t) * (size_t)n)) ||
      (rc = rows->bCp.reserve(sizeof(double) * (size_t)k * d)) ||
      (rc = rows->bDelta.reserve(sizeof(double) * (size_t)k)) ||
      (rc = rows->bCcs.reserve(sizeof(double) * (size_t)k)) ||
      (rc = rows->bPrm.reserve(sizeof(k8::DriftParams))) ||
      (rc = rows->bTmp.reserve(sizeof(int32_t) * (size_t)n)) ||
      (rc = rows->bCount.reserve(sizeof(unsigned int) * (size_t)(k8::bounds_blocks(n) + 1))) ||
      (rc = rows->bTmp2.reserve(sizeof(int32_t) * (size_t)n)) ||
      (rc = rows->bCount2.reserve(sizeof(unsigned int) * (size_t)(k8::bounds_blocks(n) + 1))) ||
      (rc = rows->bList.reserve(sizeof(int32_t) * (size_t)n)) ||
      (rc = rows->bListCount.reserve(64)) ||
      (rc = rows->bLnc.reserve(sizeof(float) * (size_t)n)) ||
      (rc = rows->bSets.reserve(sizeof(int32_t) * (size_t)n * k8::kCandMax)) ||
      (rc = rows->bState.reserve((size_t)n)) ||
      (rc = rows->bRc.reserve(sizeof(int32_t) * (size_t)n)) ||
      (rc = rows->bRcCount.reserve(64)) ||
      (rc = rows->bNbr.reserve(sizeof(int32_t) * (size_t)k * k8::kCandMax)) ||
      (rc = rows->bNbrR.reserve(sizeof(float) * (size_t)k)))
    return rc;
  if (!rows->bCum.ptr) {
    if ((rc = rows->bCum.reserve(64)) || (rc = rows->bRcCum.reserve(64))) return rc;
    CYC_HIP(hipMemsetAsync(rows->bCum.ptr, 0, 8, st));
    CYC_HIP(hipMemsetAsync(rows->bRcCum.ptr, 0, 8, st));
  }
  carry = rows->bValid && rows->bk == k;
  rows->bValid = false;   // until the screen has written the bounds
  return CYC_OK;
}

// nbrsReady: the neighbourhoods were built with the centers' preparation
int bounds_lists(cyc_kmeans_plan p, cyc_kmeans_rows rows, const double* xnorm, int64_t n,
                 hipStream_t st, cyc::km8::Bounds& bd, bool carry, bool nbrsReady) {
  namespace k8 = cyc::km8;
  const int k = p->k;
  int rc;
  bd = k8::Bounds{(float2*)rows->bnd.ptr, nullptr, nullptr};
  bd.lnc = (float*)rows->bLnc.ptr;
  bd.sets = (int32_t*)rows->bSets.ptr;
  bd.state = (unsigned char*)rows->bState.ptr;
  bd.dp = (const k8::DriftParams*)rows->bPrm.ptr;
  bd.tmp = (int32_t*)rows->bTmp.ptr;
  bd.bcount = (unsigned int*)rows->bCount.ptr;
  bd.list = (int32_t*)rows->bList.ptr;
  bd.listCount = (unsigned int*)rows->bListCount.ptr;
  bd.cum = (unsigned long long*)rows->bCum.ptr;
  bd.n = n;
  if (carry) {
    // kept rows, the re-check list (screen: the re-check, then the state-1
    // rows collected into bList for the one-limb pass; with the two-phase
    // re-check the filter lists its state-1 rows there itself and the
    // re-check appends its failures)
    const bool two = k8::recheck_two_phase();
    k8::FilterArgs fa{(const int32_t*)rows->bAssign.ptr, xnorm, k,
                      (const double*)rows->bDelta.ptr, (int32_t*)rows->bRc.ptr,
                      (unsigned int*)rows->bRcCount.ptr, (unsigned long long*)rows->bRcCum.ptr};
    fa.stats = nbrOff() ? nullptr : (const double*)p->stats.ptr;
    fa.nbr = (int32_t*)rows->bNbr.ptr;
    fa.nbrR = (float*)rows->bNbrR.ptr;
    fa.nbrsReady = nbrsReady;
    if (two) {
      fa.tmp2 = (int32_t*)rows->bTmp2.ptr;
      fa.bcount2 = (unsigned int*)rows->bCount2.ptr;
    }
    if ((rc = k8::bounds_filter(bd, fa, st))) return rc;
    bd.collected = two;
    if (!nbrOff()) {
      bd.nbr = (const int32_t*)rows->bNbr.ptr;
      bd.nbrR = (const float*)rows->bNbrR.ptr;
    }
    if (cyc::dump_dir() && rows->bCalls == sw_dump_call()) {
      bd.dump = 1;
      cyc::dump_dev("state_filter", rows->bState.ptr, (size_t)n, st);
      cyc::dump_dev("bnd", rows->bnd.ptr, sizeof(float2) * (size_t)n, st);
      cyc::dump_dev("lnc", rows->bLnc.ptr, sizeof(float) * (size_t)n, st);
      cyc::dump_dev("assign", rows->bAssign.ptr, sizeof(int32_t) * (size_t)n, st);
      cyc::dump_dev("nbrR", rows->bNbrR.ptr, sizeof(float) * (size_t)k, st);
      cyc::dump_dev("nbr", rows->bNbr.ptr, sizeof(int32_t) * (size_t)k * k8::kCandMax, st);
      cyc::dump_dev("delta", rows->bDelta.ptr, sizeof(double) * (size_t)k, st);
      cyc::dump_dev("prm", rows->bPrm.ptr, sizeof(k8::DriftParams), st);
    }
    bd.rcRows = (const int32_t*)rows->bRc.ptr;
    bd.rcCount = (const unsigned int*)rows->bRcCount.ptr;
    bd.rowsIn = bd.list;
    bd.rowsInCount = bd.listCount;
  } else {
    // a full screen: no carried sets yet (NaN outside bounds)
    CYC_HIP(hipMemsetAsync(bd.lnc, 0xff, sizeof(float) * (size_t)n, st));
    rows->bFullRows += n;
  }
  return CYC_OK;
}

int bounds_prepare(cyc_kmeans_plan p, cyc_kmeans_rows rows, const double* C,
                   const double* xnorm, int64_t n, hipStream_t st, cyc::km8::Bounds& bd) {
  namespace k8 = cyc::km8;
  bool carry = false;
  int rc;
  if ((rc = bounds_reserve(p, rows, n, st, carry)) ||
      (rc = k8::centers_drift(C, (double*)rows->bCp.ptr, p->k, p->d, (double*)rows->bDelta.ptr,
                              (double*)rows->bCcs.ptr, (k8::DriftParams*)rows->bPrm.ptr, st)))
    return rc;
  return bounds_lists(p, rows, xnorm, n, st, bd, carry, false);
}

// The screens' sharded append stage for n rows (with the candidate pass);
// CYC_KMEANS_NO_STAGE=1 appends straight to the lists (one counter each).
int stage_args(cyc_kmeans_plan p, int64_t n, bool useCa, cyc::km8::AppendStage& sg, bool& use) {
  use = useCa && sw_stage();
  if (!use) return CYC_OK;
  namespace k8 = cyc::km8;
  const unsigned cap = k8::shard_cap(n);
  const size_t ent = (size_t)cap * k8::kShards;
  const size_t cbytes = sizeof(unsigned int) * k8::kSets * k8::kShards * k8::kShardStride;
  int rc;
  if ((rc = p->stgRowsA.reserve(sizeof(int32_t) * ent)) ||
      (rc = p->stgRowsB.reserve(sizeof(int32_t) * ent)) ||
      (rc = p->stgCandRows.reserve(sizeof(int32_t) * ent)) ||
      (rc = p->stgCands.reserve(sizeof(int32_t) * ent * k8::kCand1)) ||
      (rc = p->stgCounts.reserve(cbytes)))
    return rc;
  sg = k8::AppendStage{(int32_t*)p->stgRowsA.ptr, (int32_t*)p->stgRowsB.ptr,
                       (int32_t*)p->stgCandRows.ptr, (int32_t*)p->stgCands.ptr,
                       (unsigned int*)p->stgCounts.ptr, cap};
  return CYC_OK;
}

// The i8 screens' optional arguments for one call: the candidate pass, the
// one-limb pass + refinement and the append stage, each with whether this
// call uses it, and what every launch of the screen shares (call; its
// xnorm, assign and st are the entry point's, set by do_assign / cos_assign).
// Built once per call (screen_setup), read by prep_all for the counters its
// fused launch zeroes and by the screen itself.
struct ScreenSetup {
  cyc::km8::ScreenCall call;
  cyc::km8::CandArgs ca;
  cyc::km8::RefineArgs ra;
  cyc::km8::AppendStage sg;
  bool useCa = false, useRa = false, useSg = false;
  const cyc::km8::CandArgs* cand() const { return useCa ? &ca : nullptr; }
  const cyc::km8::RefineArgs* refine() const { return useRa ? &ra : nullptr; }
  const cyc::km8::AppendStage* stage() const { return useSg ? &sg : nullptr; }
};

// Reserves the buffers and reads the per-call switches (CANDS3, NO_REFINE,
// NO_STAGE).  Nothing without a usable row image.  unit: the cosine plan's
// screen on unit directions (C, cnorm: the unit centers; no refinement).
int screen_setup(cyc_kmeans_plan p, cyc_kmeans_rows rows, int64_t n, const double* X,
                 const double* xnorm, const double* C, const double* cnorm, bool unit,
                 ScreenSetup& ss) {
  ss = ScreenSetup{};
  if (!(rows && rows->usable)) return CYC_OK;
  int rc;
  if ((rc = cand_args(p, n, X, xnorm, C, cnorm, unit, ss.ca, ss.useCa)) ||
      (!unit && (rc = refine_args(p, n, ss.useCa, ss.ra, ss.useRa))) ||
      (rc = stage_args(p, n, ss.useCa, ss.sg, ss.useSg)))
    return rc;
  ss.call = cyc::km8::ScreenCall{rows->img.ptr, (const int2*)rows->meta.ptr, nullptr, n, p->d,
                                 p->cb8.ptr, (const float*)p->cq8.ptr, (const double*)p->g8.ptr,
                                 cnorm, (const cyc::km8::CenterParams*)p->prm8.ptr, p->ktp8,
                                 nullptr, nullptr};
  return CYC_OK;
}

// One dense Euclidean assignment (tiers 3-5 of the header) as its entry
// point describes it.
struct AssignCall {
  // rows: X (n x d), their norms, the row image (or null)
  const double* X = nullptr;
  const double* xnorm = nullptr;
  cyc_kmeans_rows rows = nullptr;
  int64_t n = 0;
  // centers and their norms
  const double* C = nullptr;
  const double* cnorm = nullptr;
  // outputs: cost may be null; n_exact_out (optional) reads the tiers'
  // queue lengths back (a host sync) and records them in the plan
  int32_t* assign = nullptr;
  double* cost = nullptr;
  int64_t* n_exact_out = nullptr;
  // nostats: findClosest(centers, point) (DistanceMeasure.scala:318-340); the
  // screens certify only rows whose winner both loops return, so only the
  // exact tier differs (no statistics prunes, best starts at +inf)
  bool nostats = false;
  const cyc::km8::Bounds* bounds = nullptr;   // carried bounds (bounds_lists)
  bool approxNorm = false;   // xnorm is the row image's (any summation order)
  bool prepared = false;     // prep_all already zeroed the counters and built the center image
};

int do_assign(cyc_kmeans_plan p, const AssignCall& a, const ScreenSetup& ss, hipStream_t st) {
  const double *X = a.X, *xnorm = a.xnorm, *C = a.C, *cnorm = a.cnorm;
  const int64_t n = a.n;
  const cyc::kmfp64::Sizing& fp = p->fp;
  const double* ct = (const double*)p->ct.ptr;
  int32_t* slowList = (int32_t*)p->slowList.ptr;
  unsigned int* slowCount = (unsigned int*)p->slowCount.ptr;
  const double* statsArg = a.nostats ? nullptr : (const double*)p->stats.ptr;
  const bool i8 = a.rows && a.rows->usable;
  // slowCount (and list3Count for the i8 tier) zeroed by one launch
  if (!a.prepared) {
    hipLaunchKernelGGL(k_zero2, dim3(1), dim3(64), 0, st, slowCount,
                       i8 ? (unsigned int*)p->list3Count.ptr : nullptr);
    CYC_LAUNCH_CHECK("k_zero2");
  }
  int rc = CYC_OK;
  const int32_t* rowList = nullptr;
  const unsigned int* rowCount = nullptr;
  if (i8) {
    // tier 1: exact-integer i8 screen over every row; undecided rows -> list3
    // centers_prepare: k_centers_scan, k_centers_params, k_centers_pack32
    // (or k_centers_pack), three launches; jobs of prep_all's when prepared
    if (!a.prepared &&
        (rc = cyc::km8::centers_prepare(C, cnorm, p->k, p->d, p->ktp8, p->cb8.ptr,
                                        (float*)p->cq8.ptr, (double*)p->g8.ptr,
                                        (cyc::km8::CenterParams*)p->prm8.ptr,
                                        (double*)p->scr8.ptr, st)))
      return rc;
    cyc::km8::ScreenCall sc = ss.call;
    sc.xnorm = xnorm;
    sc.assign = a.assign;
    sc.st = st;
    if ((rc = cyc::km8::screen(sc, (int32_t*)p->list3.ptr, (unsigned int*)p->list3Count.ptr,
                               slowList, (unsigned int*)p->list8Count.ptr, ss.cand(),
                               ss.refine(), ss.stage(), a.bounds, a.prepared)))
      return rc;
    rowList = (const int32_t*)p->list3.ptr;
    rowCount = (const unsigned int*)p->list3Count.ptr;
  } else if (fp.variant == 3) {
    // tier 1: bf16x3 screen over every row; undecided rows -> list3
    if ((rc = cyc::kmfp64::launch_assign3(fp, X, xnorm, n, C, cnorm, p->cb3.ptr,
                                          (float*)p->cq3.ptr, (int*)p->ok3.ptr, a.assign, a.cost,
                                          (int32_t*)p->list3.ptr,
                                          (unsigned int*)p->list3Count.ptr, st)))
      return rc;
    rowList = (const int32_t*)p->list3.ptr;
    rowCount = (const unsigned int*)p->list3Count.ptr;
  }
  // tier 2: fp64 MFMA screen (every row, or the queued ones).  Queued rows
  // (a few thousand after the i8 tiers) go 16 to a workgroup: a 64-row
  // tile kept ~50 CUs busy for ~110 us each (CYC_KMEANS_LIST_BM=0: the
  // plan's tile); the dynamic LDS stays the plan's (64-row) size, which
  // covers 16 rows
  const int bm = rowList && sw_list16() && fp.bm >= 16 ? 16 : fp.bm;
  if ((rc = cyc::kmfp64::launch_assign(fp, bm, X, xnorm, n, C, cnorm, ct, a.assign, a.cost,
                                       slowList, slowCount, st, rowList, rowCount)))
    return rc;
  // Exact emulation of the reference loop for undecided rows.  The queue
  // length is read back only when the caller asks for it; otherwise a
  // grid-stride launch drains whatever the queue holds without a host sync.
  int64_t known = -1;
  if (a.n_exact_out) {
    unsigned int h_slow = 0, h_tier2 = 0, h_limb3 = 0, h_cand = 0, h_cand2 = 0;
    const bool twoPass = i8 && cyc::km8::uses32(p->d);
    CYC_HIP(hipMemcpyAsync(&h_slow, slowCount, sizeof(unsigned), hipMemcpyDeviceToHost, st));
    if (rowCount)
      CYC_HIP(hipMemcpyAsync(&h_tier2, rowCount, sizeof(unsigned), hipMemcpyDeviceToHost, st));
    if (twoPass) {
      CYC_HIP(hipMemcpyAsync(&h_limb3, p->list8Count.ptr, sizeof(unsigned), hipMemcpyDeviceToHost, st));
      CYC_HIP(hipMemcpyAsync(&h_cand, p->candCount.ptr, sizeof(unsigned), hipMemcpyDeviceToHost, st));
      if (p->cands3)
        CYC_HIP(hipMemcpyAsync(&h_cand2, p->candCount2.ptr, sizeof(unsigned), hipMemcpyDeviceToHost, st));
    }
    CYC_HIP(hipStreamSynchronize(st));
    *a.n_exact_out = h_slow;
    p->lastTier2 = rowCount ? (int64_t)h_tier2 : n;
    p->lastExact = h_slow;
    p->lastLimb3 = twoPass ? (int64_t)h_limb3 : -1;
    p->lastCands = twoPass ? (int64_t)h_cand : -1;
    p->lastCands2 = twoPass && p->cands3 ? (int64_t)h_cand2 : -1;
    if (!h_slow) return CYC_OK;
    known = h_slow;
  }
  return cyc::kmfp64::launch_exact(fp, X, xnorm, n, C, cnorm, ct, statsArg, slowList, slowCount,
                                   p->exactDist, a.assign, a.cost, a.approxNorm, known,
                                   sw_exact_split(), st);
}

// The checks' device result (bytes), its pinned host copy (5 words) and the
// event that marks the copy landed, created on first use.
int req_reserve(cyc_kmeans_plan p, size_t bytes) {
  int rc;
  if ((rc = p->req.reserve(bytes))) return rc;
  if (!p->reqHost) CYC_HIP(hipHostMalloc((void**)&p->reqHost, 5 * sizeof(unsigned long long)));
  if (!p->reqEv) CYC_HIP(hipEventCreateWithFlags(&p->reqEv, hipEventDisableTiming));
  return CYC_OK;
}

// Enqueue k_require_norms and the copy of its result; require_check reads it
// after the rest of the call is enqueued, so the host waits only for this
// early, short kernel (its result lands long before the assign finishes).
// (The separate-launch form: cyc_kmeans_accumulate_dev runs the check as a
// level-0 job of prep_all, with the same fill before and copy + event after.)
int require_enqueue(cyc_kmeans_plan p, const double* C, const double* xnorm, int64_t n,
                    hipStream_t st) {
  int rc;
  if ((rc = req_reserve(p, 5 * sizeof(unsigned long long)))) return rc;
  CYC_HIP(hipMemsetAsync(p->req.ptr, 0xff, 2 * sizeof(unsigned long long), st));
  const int64_t work = std::max<int64_t>(n, (int64_t)p->k * p->d);
  const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((work + 255) / 256, 2048));
  hipLaunchKernelGGL(k_require_norms, dim3(grid), dim3(256), 0, st, C, p->k, p->d, xnorm, n,
                     (unsigned long long*)p->req.ptr);
  CYC_LAUNCH_CHECK("k_require_norms");
  CYC_HIP(hipMemcpyAsync(p->reqHost, p->req.ptr, 5 * sizeof(unsigned long long),
                         hipMemcpyDeviceToHost, st));
  CYC_HIP(hipEventRecord(p->reqEv, st));
  return CYC_OK;
}

// The fused form of a Lloyd call's center-only work (cyc::km8::
// centers_prepare_all): what require_enqueue, do_stats, the center side of
// bounds_prepare, do_assign's k_zero2 and centers_prepare and the screen's
// k_zero_counters enqueue as twelve launches, as three.  The req buffer
// holds the 5 req words, padding to 8, then the statistics' k row minima:
// ONE 0xff byte fill presets req[0..1] and the minima (the pairs job's
// atomicMin runs beside the transpose job in level 0, so the minima cannot
// be preset by that job as k_center_transpose_fill does; ~0 is above every
// statistic's bit pattern and stats_diag reads it as +Infinity).
// useBnd / carry: bounds_on and bounds_reserve's carry.  ss: the call's
// screen setup, whose counters the launches zero; null (cyc_kmeans_stats_dev):
// the check, the statistics and the transpose alone.
int prep_all(cyc_kmeans_plan p, cyc_kmeans_rows rows, const double* xnorm, int64_t n,
             const double* C, const double* cnorm, bool useBnd, bool carry,
             const ScreenSetup* ss, hipStream_t st) {
  namespace k8 = cyc::km8;
  const int k = p->k, d = p->d;
  int rc;
  const size_t reqBytes = sizeof(unsigned long long) * (8 + (size_t)k);
  if ((rc = req_reserve(p, reqBytes))) return rc;
  CYC_HIP(hipMemsetAsync(p->req.ptr, 0xff, reqBytes, st));
  k8::PrepJobs J;
  J.C = C;
  J.cnorm = cnorm;
  J.k = k;
  J.d = d;
  J.stats = (double*)p->stats.ptr;
  J.dmin = (unsigned long long*)p->req.ptr + 8;
  J.ct = p->dense_ok ? (double*)p->ct.ptr : nullptr;
  J.d4 = p->fp.d4;
  J.kpad = p->fp.kpad;
  J.xnorm = xnorm;
  J.n = n;
  J.req = (unsigned long long*)p->req.ptr;
  const int64_t work = std::max<int64_t>(n, (int64_t)k * d);
  J.reqBlocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>((work + 255) / 256, 2048));
  if (useBnd) {
    J.Cp = (double*)rows->bCp.ptr;
    J.delta = (double*)rows->bDelta.ptr;
    J.ccs = (double*)rows->bCcs.ptr;
    J.dprm = (k8::DriftParams*)rows->bPrm.ptr;
    if (carry && !nbrOff()) {
      J.nbr = (int32_t*)rows->bNbr.ptr;
      J.nbrR = (float*)rows->bNbrR.ptr;
    }
  }
  const bool i8 = rows && rows->usable;
  if (ss) {
    J.zeroA = (unsigned int*)p->slowCount.ptr;
    J.zeroB = i8 ? (unsigned int*)p->list3Count.ptr : nullptr;
  }
  if (i8 && ss) {
    J.ktp = p->ktp8;
    J.Cb = p->cb8.ptr;
    J.cq = (float*)p->cq8.ptr;
    J.g = (double*)p->g8.ptr;
    J.cprm = (k8::CenterParams*)p->prm8.ptr;
    J.scratch = (double*)p->scr8.ptr;
    // the screen's counters, for the arguments do_assign passes it
    J.zero = k8::screen_zero_args((unsigned int*)p->list8Count.ptr, ss->cand(), ss->refine(),
                                  ss->stage());
  }
  return k8::centers_prepare_all(J, st, p->reqHost, p->reqEv);
}

// The IllegalArgumentException the reference raises first, if any:
// computeStatistics' pair loop (i < j, DistanceMeasure.scala:55-66) meets
// (0, m) for the lowest NaN center m > 0, or (0, 1) when center 0 is NaN;
// with k == 1 there are no statistics and the first point meets center 0;
// otherwise the first NaN-norm point meets center 0 (norm2 = NaN).
// verdict (a Lloyd call with a row image): the image's stored row result put
// in place of the words a call without the row half left at their presets,
// or, when it does not hold for (xnorm, n), this call's row result stored.
int require_check(cyc_kmeans_plan p, int64_t n, const double* Xrow0 = nullptr,
                  cyc_kmeans_rows_s::RowVerdict* verdict = nullptr,
                  const double* xnorm = nullptr) {
  CYC_HIP(hipEventSynchronize(p->reqEv));
  if (verdict) {
    if (verdict->holds(xnorm, n)) {
      p->reqHost[1] = verdict->rbad;
      p->reqHost[4] = verdict->x0;
    } else {
      *verdict = {true, xnorm, n, p->reqHost[1], p->reqHost[4]};
    }
  }
  const unsigned long long cbad = p->reqHost[0], rbad = p->reqHost[1];
  double* v = reinterpret_cast<double*>(p->reqHost + 2);
  if (Xrow0 && n > 0 && cbad == 0 && !(p->k >= 2)) {
    // the message's norm2 is row 0's Vectors.norm: the image's norms (in
    // another summation order) stand in for the caller's, so recompute it
    std::vector<double> x0((size_t)p->d);
    CYC_HIP(hipMemcpy(x0.data(), Xrow0, sizeof(double) * (size_t)p->d, hipMemcpyDeviceToHost));
    double sq = 0.0;
    for (int j = 0; j < p->d; ++j) sq = sq + x0[j] * x0[j];
    v[2] = std::sqrt(sq);
  }
  const double nan = __builtin_nan("");
  auto fail = [](double n1, double n2) {
    cyc::set_error("requirement failed: Both norms should be greater or equal to 0.0, found "
                   "norm1=" + cyc::java_double(n1) + ", norm2=" + cyc::java_double(n2));
    return CYC_ERR_INVALID_ARG;
  };
  if (p->k >= 2 && cbad < (unsigned long long)p->k) return cbad == 0 ? fail(nan, v[1]) : fail(v[0], nan);
  if (n > 0 && cbad == 0) return fail(nan, v[2]);
  if (rbad < (unsigned long long)n) return fail(v[0], nan);
  return CYC_OK;
}

int ensure_rows(cyc_kmeans_plan p, int64_t n) {
  if (n <= p->max_rows && p->slowList.ptr) return CYC_OK;
  int rc;
  if ((rc = p->slowList.reserve(sizeof(int32_t) * (size_t)std::max<int64_t>(n, 1)))) return rc;
  if ((rc = p->list3.reserve(sizeof(int32_t) * (size_t)std::max<int64_t>(n, 1)))) return rc;
  p->max_rows = std::max(p->max_rows, n);
  return CYC_OK;
}

// ------------------------------------------------------------ cosine plan
bool is_cos(cyc_kmeans_plan p) { return p->measure == CYC_DISTANCE_COSINE; }

// The zero-length assert of CosineDistanceMeasure.distance (DistanceMeasure.
// scala:453-456): enqueued first, read by cos_check at the end of the call.
// Every center norm is checked when checkCenters (computeStatistics measures
// every pair for k >= 2; findClosest measures center 0, and without
// statistics every center, for each point), every row norm when n > 0.
int cos_enqueue(cyc_kmeans_plan p, const double* cnorm, bool checkCenters, const double* xnorm,
                int64_t n, hipStream_t st) {
  int rc;
  if ((rc = req_reserve(p, 5 * sizeof(unsigned long long)))) return rc;
  if ((rc = cyc::kmcos::assert_norms(cnorm, p->k, checkCenters, xnorm, n,
                                     (unsigned long long*)p->req.ptr, st)))
    return rc;
  CYC_HIP(hipMemcpyAsync(p->reqHost, p->req.ptr, sizeof(unsigned long long),
                         hipMemcpyDeviceToHost, st));
  CYC_HIP(hipEventRecord(p->reqEv, st));
  return CYC_OK;
}

int cos_check(cyc_kmeans_plan p) {
  CYC_HIP(hipEventSynchronize(p->reqEv));
  if (p->reqHost[0]) {
    cyc::set_error("assertion failed: Cosine distance is not defined for zero-length vectors.");
    return CYC_ERR_ASSERTION;
  }
  return CYC_OK;
}

int cos_transpose(cyc_kmeans_plan p, const double* C, hipStream_t st) {
  const int64_t total = (int64_t)p->fp.d4 * p->fp.kpad;
  hipLaunchKernelGGL(k_center_transpose, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st,
                     C, p->k, p->d, p->fp.d4, p->fp.kpad, (double*)p->ct.ptr);
  CYC_LAUNCH_CHECK("k_center_transpose");
  return CYC_OK;
}

int cos_stats(cyc_kmeans_plan p, const double* C, const double* cnorm, hipStream_t st) {
  return cyc::kmcos::stats(C, cnorm, p->k, p->d, (double*)p->stats.ptr,
                           (unsigned long long*)p->dmin.ptr, st);
}

// CosineDistanceMeasure.findClosest for n dense rows: the i8 screen on the
// unit directions (row image built for cosine), then the reference loop for
// every row it leaves (every row without an image).
int cos_assign(cyc_kmeans_plan p, const double* X, const double* xnorm, cyc_kmeans_rows rows,
               int64_t n, const double* C, const double* cnorm, int32_t* assign, double* cost,
               int64_t* n_exact_out, hipStream_t st, bool nostats) {
  int rc;
  if ((rc = cos_transpose(p, C, st))) return rc;
  int32_t* list = (int32_t*)p->list3.ptr;
  unsigned int* count = (unsigned int*)p->list3Count.ptr;
  const bool screen = rows && rows->usable && p->ktp8 > 0;
  if (screen) {
    if ((rc = p->cosV.reserve(sizeof(double) * (size_t)p->k * p->d)) ||
        (rc = p->cosVn.reserve(sizeof(double) * (size_t)p->k)))
      return rc;
    double* V = (double*)p->cosV.ptr;
    double* Vn = (double*)p->cosVn.ptr;
    if ((rc = cyc::kmcos::centers_unit(C, cnorm, p->k, p->d, V, Vn, st))) return rc;
    CYC_HIP(hipMemsetAsync(count, 0, sizeof(unsigned int), st));
    ScreenSetup ss;
    if ((rc = screen_setup(p, rows, n, X, xnorm, V, Vn, true, ss))) return rc;
    cyc::km8::ScreenCall sc = ss.call;
    sc.xnorm = (const double*)rows->unorm.ptr;   // the unit directions' norms
    sc.assign = assign;
    sc.st = st;
    if ((rc = cyc::km8::centers_prepare(V, Vn, p->k, p->d, p->ktp8, p->cb8.ptr,
                                        (float*)p->cq8.ptr, (double*)p->g8.ptr,
                                        (cyc::km8::CenterParams*)p->prm8.ptr,
                                        (double*)p->scr8.ptr, st)) ||
        (rc = cyc::km8::screen(sc, list, count, (int32_t*)p->slowList.ptr,
                               (unsigned int*)p->list8Count.ptr, ss.cand(), nullptr,
                               ss.stage())))
      return rc;
  } else if ((rc = cyc::kmcos::list_all(list, count, n, st))) {
    return rc;
  }
  int64_t maxRows = n;
  if (n_exact_out) {
    unsigned int h = 0, h3 = 0, hc = 0, hc2 = 0;
    const bool twoPass = screen && cyc::km8::uses32(p->d);
    CYC_HIP(hipMemcpyAsync(&h, count, sizeof(unsigned), hipMemcpyDeviceToHost, st));
    if (twoPass) {
      CYC_HIP(hipMemcpyAsync(&h3, p->list8Count.ptr, sizeof(unsigned), hipMemcpyDeviceToHost, st));
      CYC_HIP(hipMemcpyAsync(&hc, p->candCount.ptr, sizeof(unsigned), hipMemcpyDeviceToHost, st));
      if (p->cands3)
        CYC_HIP(hipMemcpyAsync(&hc2, p->candCount2.ptr, sizeof(unsigned), hipMemcpyDeviceToHost, st));
    }
    CYC_HIP(hipStreamSynchronize(st));
    *n_exact_out = h;
    p->lastTier2 = h;   // no fp64 screen tier: the screen's leftovers are exact
    p->lastExact = h;
    p->lastLimb3 = twoPass ? (int64_t)h3 : -1;
    p->lastCands = twoPass ? (int64_t)hc : -1;
    p->lastCands2 = twoPass && p->cands3 ? (int64_t)hc2 : -1;
    maxRows = h;
  }
  if (maxRows == 0) return CYC_OK;
  return cyc::kmcos::assign_exact(X, xnorm, p->d, C, (const double*)p->ct.ptr, p->fp.kpad, cnorm,
                                  p->k, nostats ? nullptr : (const double*)p->stats.ptr, list,
                                  count, maxRows, assign, cost, st);
}

bool inc_on(cyc_kmeans_rows rows) {
  return rows->inc.enabled && sw_incr() && !cyc::strict_parity();
}

}  // namespace

extern "C" {

int cyc_row_norms_dev(const double* X, int64_t n, int32_t d, double* norms, void* stream) {
  CYC_REQUIRE(n >= 0 && d > 0, "n >= 0 and d > 0");
  if (n == 0) return CYC_OK;
  hipLaunchKernelGGL(k_row_norms, dim3((unsigned)((n + kNormRows - 1) / kNormRows)),
                     dim3(kNormRows), 0, cyc::as_stream(stream), X, n, d, norms);
  CYC_LAUNCH_CHECK("k_row_norms");
  return CYC_OK;
}

int cyc_kmeans_plan_create(int32_t d, int32_t k, int64_t max_rows, cyc_kmeans_plan* plan) {
  CYC_REQUIRE(plan != nullptr, "plan must not be null");
  CYC_REQUIRE(d > 0, "Number of features must be positive");
  CYC_REQUIRE(k >= 1, "Number of clusters must be positive but got " + std::to_string(k));
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    cyc::set_error("no HIP device visible");
    return CYC_ERR_NO_DEVICE;
  }
  if (k > kMaxK) {
    cyc::set_error("k > 8192 is not supported by the device counting sort");
    return CYC_ERR_UNSUPPORTED;
  }
  auto* p = new cyc_kmeans_plan_s();
  p->d = d;
  p->k = k;
  p->fp = cyc::kmfp64::sizing(d, k, sw_assign_variant());
  // d > 1216: no LDS-resident dense assign; the plan still serves sparse rows
  p->dense_ok = p->fp.bm != 0;
  int rc;
  if (p->fp.variant == 3 &&
      ((rc = p->cb3.reserve((size_t)p->fp.ktp3 * p->fp.ks3 * 2 * 64 * 16)) ||
       (rc = p->cq3.reserve(sizeof(float) * (size_t)p->fp.ktp3 * 16)) ||
       (rc = p->ok3.reserve(64)))) {
    delete p;
    return rc;
  }
  if ((rc = p->list3Count.reserve(64))) {
    delete p;
    return rc;
  }
  if (d <= cyc::km8::kMaxD) {
    const int ks8 = cyc::km8::ksteps(d);
    p->ktp8 = (int)cyc::round_up((k + 15) / 16, cyc::km8::kWaves);
    if ((rc = p->cb8.reserve((size_t)p->ktp8 * ks8 * 3 * 64 * 16 * 2)) ||
        (rc = p->cq8.reserve(sizeof(float) * (size_t)p->ktp8 * 48)) ||
        (rc = p->g8.reserve(sizeof(double) * (size_t)p->ktp8 * 48)) ||
        (rc = p->list8Count.reserve(64)) ||
        (rc = p->prm8.reserve(sizeof(cyc::km8::CenterParams))) ||
        (rc = p->scr8.reserve(sizeof(double) * 2 * (size_t)k))) {
      delete p;
      return rc;
    }
  }
  if ((p->dense_ok && (rc = p->ct.reserve(sizeof(double) * (size_t)p->fp.d4 * p->fp.kpad))) ||
      (rc = p->stats.reserve(sizeof(double) * ((size_t)k * (k + 1) / 2))) ||
      (rc = p->dmin.reserve(sizeof(unsigned long long) * (size_t)k)) ||
      (rc = p->slowCount.reserve(64)) || (rc = ensure_rows(p, std::max<int64_t>(max_rows, 1)))) {
    delete p;
    return rc;
  }
  *plan = p;
  return CYC_OK;
}

int cyc_kmeans_last_tiers(cyc_kmeans_plan p, int64_t* fp64_screen_rows, int64_t* exact_rows) {
  CYC_REQUIRE(p != nullptr && fp64_screen_rows && exact_rows, "arguments must not be null");
  std::lock_guard<std::mutex> g(p->mu);
  *fp64_screen_rows = p->lastTier2;
  *exact_rows = p->lastExact;
  return CYC_OK;
}

int cyc_kmeans_last_screen(cyc_kmeans_plan p, int64_t* three_limb_rows) {
  CYC_REQUIRE(p != nullptr && three_limb_rows, "arguments must not be null");
  std::lock_guard<std::mutex> g(p->mu);
  *three_limb_rows = p->lastLimb3;
  return CYC_OK;
}

int cyc_kmeans_last_candidates(cyc_kmeans_plan p, int64_t* candidate_rows) {
  CYC_REQUIRE(p != nullptr && candidate_rows, "arguments must not be null");
  std::lock_guard<std::mutex> g(p->mu);
  *candidate_rows = p->lastCands;
  return CYC_OK;
}

int cyc_kmeans_last_candidates3(cyc_kmeans_plan p, int64_t* fp64_rows) {
  CYC_REQUIRE(p != nullptr && fp64_rows, "arguments must not be null");
  std::lock_guard<std::mutex> g(p->mu);
  *fp64_rows = p->lastCands2;
  return CYC_OK;
}

int cyc_kmeans_last_refine(cyc_kmeans_plan p, int64_t* listed_rows, int64_t* full_rows,
                           int64_t* union_centers) {
  CYC_REQUIRE(p != nullptr && listed_rows && full_rows && union_centers,
              "arguments must not be null");
  std::lock_guard<std::mutex> g(p->mu);
  *listed_rows = *full_rows = *union_centers = -1;
  if (!p->lastRefined) return CYC_OK;
  unsigned int h[3] = {0, 0, 0};
  CYC_HIP(hipMemcpy(h, p->cand1Count.ptr, sizeof(unsigned int), hipMemcpyDeviceToHost));
  CYC_HIP(hipMemcpy(h + 1, p->fullCount.ptr, 2 * sizeof(unsigned int), hipMemcpyDeviceToHost));
  *listed_rows = h[0];
  *full_rows = h[1];
  *union_centers = h[2];
  return CYC_OK;
}

int cyc_kmeans_plan_destroy(cyc_kmeans_plan plan) {
  delete plan;
  return CYC_OK;
}

int cyc_kmeans_plan_set_distance_measure(cyc_kmeans_plan p, int32_t measure) {
  CYC_REQUIRE(p != nullptr, "plan must not be null");
  // DistanceMeasure.decodeFromString (DistanceMeasure.scala:241-247)
  CYC_REQUIRE(measure == CYC_DISTANCE_EUCLIDEAN || measure == CYC_DISTANCE_COSINE,
              "distanceMeasure must be one of: euclidean, cosine. " + std::to_string(measure) +
                  " provided.");
  std::lock_guard<std::mutex> g(p->mu);
  p->measure = measure;
  return CYC_OK;
}

int cyc_kmeans_stats_dev(cyc_kmeans_plan p, const double* C, double* stats_out, void* stream) {
  CYC_REQUIRE(p != nullptr && C != nullptr, "plan and centers must not be null");
  std::lock_guard<std::mutex> g(p->mu);
  hipStream_t st = cyc::as_stream(stream);
  int rc;
  if (is_cos(p)) {
    // new VectorWithNorm(center): norms computed here (KMeansModel.scala:47-56)
    if ((rc = p->cosCn.reserve(sizeof(double) * (size_t)p->k))) return rc;
    const double* cn = (const double*)p->cosCn.ptr;
    hipLaunchKernelGGL(k_row_norms, dim3((unsigned)((p->k + kNormRows - 1) / kNormRows)),
                       dim3(kNormRows), 0, st, C, (int64_t)p->k, p->d, (double*)p->cosCn.ptr);
    CYC_LAUNCH_CHECK("k_row_norms");
    if ((rc = cos_enqueue(p, cn, p->k >= 2, nullptr, 0, st))) return rc;
    if (p->dense_ok && (rc = cos_transpose(p, C, st))) return rc;
    if ((rc = cos_stats(p, C, cn, st))) return rc;
  } else if (cyc::km8::prep_fused()) {
    if ((rc = prep_all(p, nullptr, nullptr, 0, C, nullptr, false, false, nullptr, st)))
      return rc;
  } else {
    if ((rc = require_enqueue(p, C, nullptr, 0, st))) return rc;
    if ((rc = do_stats(p, C, st))) return rc;
  }
  if (stats_out)
    CYC_HIP(hipMemcpyAsync(stats_out, p->stats.ptr, sizeof(double) * ((size_t)p->k * (p->k + 1) / 2),
                           hipMemcpyDeviceToDevice, st));
  return is_cos(p) ? cos_check(p) : require_check(p, 0);
}

int cyc_kmeans_rows_create(cyc_kmeans_plan p, const double* X, int64_t n, void* stream,
                           cyc_kmeans_rows* out) {
  CYC_REQUIRE(p != nullptr && out != nullptr, "plan and out must not be null");
  CYC_REQUIRE(n >= 0, "n >= 0");
  CYC_REQUIRE(X != nullptr || n == 0, "X must not be null");
  auto* r = new cyc_kmeans_rows_s();
  r->X = X;
  r->n = n;
  r->d = p->d;
  r->usable = p->d <= cyc::km8::kMaxD && p->ktp8 > 0;
  r->cosine = is_cos(p);
  if (r->usable && n > 0) {
    int rc;
    hipStream_t st = cyc::as_stream(stream);
    if ((rc = r->img.reserve((size_t)n * cyc::km8::image_row_bytes(p->d))) ||
        (rc = r->meta.reserve(sizeof(int2) * (size_t)n))) {
      delete r;
      return rc;
    }
    if (r->cosine) {
      // the image of x / |x|, and |x / |x|| for the screen's margins
      cyc::DeviceBuffer xn;
      if ((rc = r->unorm.reserve(sizeof(double) * (size_t)n)) ||
          (rc = xn.reserve(sizeof(double) * (size_t)n))) {
        delete r;
        return rc;
      }
      hipLaunchKernelGGL(k_row_norms, dim3((unsigned)((n + kNormRows - 1) / kNormRows)),
                         dim3(kNormRows), 0, st, X, n, p->d, (double*)xn.ptr);
      CYC_LAUNCH_CHECK("k_row_norms");
      rc = cyc::km8::rows_quantize(X, n, p->d, r->img.ptr, (int2*)r->meta.ptr, st,
                                   (const double*)xn.ptr, (double*)r->unorm.ptr);
      if (!rc && hipStreamSynchronize(st) != hipSuccess) rc = CYC_ERR_HIP;   // xn freed here
    } else {
      // with the image, the norms in any summation order (a wave sum): what
      // the screens need when the caller passes no norms (accumulate_dev)
      if ((rc = r->unorm.reserve(sizeof(double) * (size_t)n))) {
        delete r;
        return rc;
      }
      rc = cyc::km8::rows_quantize(X, n, p->d, r->img.ptr, (int2*)r->meta.ptr, st, nullptr,
                                   (double*)r->unorm.ptr);
    }
    if (rc) {
      delete r;
      return rc;
    }
  }
  *out = r;
  return CYC_OK;
}

int cyc_kmeans_rows_destroy(cyc_kmeans_rows rows) {
  delete rows;
  return CYC_OK;
}

int64_t cyc_kmeans_rows_bytes(cyc_kmeans_rows rows) {
  return rows ? (int64_t)(rows->img.bytes + rows->meta.bytes) : 0;
}

int cyc_kmeans_rows_set_bounds(cyc_kmeans_rows rows, int32_t enable) {
  CYC_REQUIRE(rows != nullptr, "rows must not be null");
  rows->bEnabled = enable != 0;
  rows->bValid = false;   // a re-enabled fit starts from a full screen
  return CYC_OK;
}

int cyc_kmeans_rows_set_incremental(cyc_kmeans_rows rows, int32_t enable) {
  CYC_REQUIRE(rows != nullptr, "rows must not be null");
  rows->inc.enabled = enable != 0;
  rows->inc.valid = false;   // the next call runs the full pass
  return CYC_OK;
}

int cyc_kmeans_rows_incremental_info(cyc_kmeans_rows rows, int64_t* incremental_calls,
                                     int64_t* moved_rows) {
  CYC_REQUIRE(rows != nullptr && incremental_calls != nullptr && moved_rows != nullptr,
              "arguments must not be null");
  unsigned long long cum[2] = {0, 0};
  if (rows->inc.cum.ptr) {
    CYC_HIP(hipDeviceSynchronize());
    CYC_HIP(hipMemcpy(cum, rows->inc.cum.ptr, sizeof(cum), hipMemcpyDeviceToHost));
  }
  *incremental_calls = (int64_t)cum[1];
  *moved_rows = (int64_t)cum[0];
  return CYC_OK;
}

int cyc_kmeans_rows_bounds_rechecked(cyc_kmeans_rows rows, int64_t* rechecked_rows) {
  CYC_REQUIRE(rows != nullptr && rechecked_rows != nullptr, "arguments must not be null");
  unsigned long long cum = 0;
  if (rows->bRcCum.ptr) {
    CYC_HIP(hipDeviceSynchronize());
    CYC_HIP(hipMemcpy(&cum, rows->bRcCum.ptr, sizeof(cum), hipMemcpyDeviceToHost));
  }
  *rechecked_rows = (int64_t)cum;
  return CYC_OK;
}

int cyc_kmeans_rows_bounds_info(cyc_kmeans_rows rows, int64_t* calls, int64_t* screened_rows) {
  CYC_REQUIRE(rows != nullptr && calls != nullptr && screened_rows != nullptr,
              "arguments must not be null");
  unsigned long long cum = 0;
  if (rows->bCum.ptr) {
    CYC_HIP(hipDeviceSynchronize());   // the counter is added on the callers' streams
    CYC_HIP(hipMemcpy(&cum, rows->bCum.ptr, sizeof(cum), hipMemcpyDeviceToHost));
  }
  *calls = rows->bCalls;
  *screened_rows = rows->bFullRows + (int64_t)cum;
  return CYC_OK;
}

namespace {
int check_rows(cyc_kmeans_plan p, cyc_kmeans_rows rows, const double* X, int64_t n) {
  CYC_REQUIRE(rows == nullptr || (rows->X == X && rows->n == n && rows->d == p->d),
              "the row image was built for other rows (cyc_kmeans_rows_create)");
  CYC_REQUIRE(rows == nullptr || rows->cosine == is_cos(p),
              "the row image was built for another distance measure");
  return CYC_OK;
}

// What the three dense entry points do after their own argument checks: the
// row image's checks, the d <= 1216 requirement, then the plan's lock (held
// by the caller's lk until it returns) and the per-row queues.
int dense_enter(cyc_kmeans_plan p, cyc_kmeans_rows rows, const double* X, int64_t n,
                std::unique_lock<std::mutex>& lk) {
  if (int rc = check_rows(p, rows, X, n)) return rc;
  if (!p->dense_ok) {
    cyc::set_error("d > 1216 is not supported by the LDS-resident assign kernel (dense rows)");
    return CYC_ERR_UNSUPPORTED;
  }
  lk = std::unique_lock<std::mutex>(p->mu);
  return ensure_rows(p, n);
}
}  // namespace

int cyc_kmeans_assign_dev(cyc_kmeans_plan p, const double* X, const double* xnorm,
                          cyc_kmeans_rows rows, int64_t n, const double* C, const double* cnorm,
                          int32_t* assign, double* cost, int64_t* n_exact_out, void* stream) {
  CYC_REQUIRE(p != nullptr, "plan must not be null");
  CYC_REQUIRE(n >= 0, "n >= 0");
  CYC_REQUIRE(assign != nullptr && cost != nullptr, "assign and cost must not be null");
  if (n_exact_out) *n_exact_out = 0;
  if (n == 0) return CYC_OK;
  std::unique_lock<std::mutex> lk;
  int rc = dense_enter(p, rows, X, n, lk);
  if (rc) return rc;
  hipStream_t st = cyc::as_stream(stream);
  if (is_cos(p)) {
    if ((rc = cos_enqueue(p, cnorm, true, xnorm, n, st)) ||
        (rc = cos_assign(p, X, xnorm, rows, n, C, cnorm, assign, nullptr, n_exact_out, st, false)) ||
        (rc = cyc::kmcos::row_cost(X, n, p->d, C, cnorm, xnorm, assign, cost, st)))
      return rc;
    return cos_check(p);
  }
  ScreenSetup ss;
  AssignCall call{X, xnorm, rows, n, C, cnorm, assign};
  call.n_exact_out = n_exact_out;
  if ((rc = require_enqueue(p, C, xnorm, n, st)) ||
      (rc = screen_setup(p, rows, n, X, nullptr, C, cnorm, false, ss)) ||
      (rc = do_assign(p, call, ss, st)))
    return rc;
  hipLaunchKernelGGL(k_row_cost, dim3((unsigned)((n + kNormRows - 1) / kNormRows)),
                     dim3(kNormRows), 0, st, X, n, p->d, C,
                     (const int32_t*)assign, cost);
  CYC_LAUNCH_CHECK("k_row_cost");
  return require_check(p, n);
}

int cyc_kmeans_point_cost_dev(cyc_kmeans_plan p, const double* X, const double* xnorm,
                              cyc_kmeans_rows rows, int64_t n, const double* C,
                              const double* cnorm, int32_t* assign, double* cost, void* stream) {
  CYC_REQUIRE(p != nullptr, "plan must not be null");
  CYC_REQUIRE(n >= 0, "n >= 0");
  CYC_REQUIRE(assign != nullptr && cost != nullptr, "assign and cost must not be null");
  if (n == 0) return CYC_OK;
  std::unique_lock<std::mutex> lk;
  int rc = dense_enter(p, rows, X, n, lk);
  if (rc) return rc;
  hipStream_t st = cyc::as_stream(stream);
  if (is_cos(p)) {
    if ((rc = cos_enqueue(p, cnorm, true, xnorm, n, st)) ||
        (rc = cos_assign(p, X, xnorm, rows, n, C, cnorm, assign, nullptr, nullptr, st, true)) ||
        (rc = cyc::kmcos::row_cost(X, n, p->d, C, cnorm, xnorm, assign, cost, st)))
      return rc;
    // a row no center beats +Infinity for keeps it (:136-148)
    hipLaunchKernelGGL(k_nostats_cost_fix, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n,
                       cost);
    CYC_LAUNCH_CHECK("k_nostats_cost_fix");
    return cos_check(p);
  }
  // the fp64 screen reads the transposed centers, which cyc_kmeans_stats_dev
  // would otherwise build: no statistics are needed here
  const int64_t total = (int64_t)p->fp.d4 * p->fp.kpad;
  hipLaunchKernelGGL(k_center_transpose, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st,
                     C, p->k, p->d, p->fp.d4, p->fp.kpad, (double*)p->ct.ptr);
  CYC_LAUNCH_CHECK("k_center_transpose");
  ScreenSetup ss;
  AssignCall call{X, xnorm, rows, n, C, cnorm, assign};
  call.nostats = true;
  if ((rc = screen_setup(p, rows, n, X, nullptr, C, cnorm, false, ss)) ||
      (rc = do_assign(p, call, ss, st)))
    return rc;
  hipLaunchKernelGGL(k_row_cost, dim3((unsigned)((n + kNormRows - 1) / kNormRows)),
                     dim3(kNormRows), 0, st, X, n, p->d, C,
                     (const int32_t*)assign, cost);
  CYC_LAUNCH_CHECK("k_row_cost");
  hipLaunchKernelGGL(k_nostats_cost_fix, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n,
                     cost);
  CYC_LAUNCH_CHECK("k_nostats_cost_fix");
  return CYC_OK;
}

int cyc_kmeans_accumulate_dev(cyc_kmeans_plan p, const double* X, const double* xnorm,
                              cyc_kmeans_rows rows, const double* weights, int64_t n,
                              const double* C, const double* cnorm, double* sums, double* wsum,
                              double* cost_sum, int32_t* assign, double* cost, void* stream) {
  CYC_REQUIRE(p != nullptr, "plan must not be null");
  CYC_REQUIRE(n >= 0, "n >= 0");
  CYC_REQUIRE(sums && wsum && cost_sum, "sums, wsum and cost_sum must not be null");
  if (n == 0) return CYC_OK;
  std::unique_lock<std::mutex> lk;
  int rc = dense_enter(p, rows, X, n, lk);
  if (rc) return rc;
  // xnorm == NULL: the row image's norms for the screens (Euclidean), the
  // reference's own norms computed where its loop needs them (k_assign_exact)
  const bool approxNorm = xnorm == nullptr;
  CYC_REQUIRE(!approxNorm || (rows && rows->usable && !rows->cosine && rows->unorm.ptr),
              "xnorm may be null only with a Euclidean row image (cyc_kmeans_rows_create)");
  if (approxNorm) xnorm = (const double*)rows->unorm.ptr;
  hipStream_t st = cyc::as_stream(stream);
  const int k = p->k, d = p->d;
  // carried bounds: the assignment lives in the row image's state and is
  // copied to the caller's array after the screen
  const bool useBnd = bounds_on(p, rows);
  int32_t* const userAssign = assign;
  if (useBnd) {
    assign = (int32_t*)nullptr;
  } else if (!assign) {
    if ((rc = p->assignTmp.reserve(sizeof(int32_t) * (size_t)n))) return rc;
    assign = (int32_t*)p->assignTmp.ptr;
  }
  const bool cosm = is_cos(p);
  if (cosm) {
    if ((rc = cos_enqueue(p, cnorm, true, xnorm, n, st)) || (rc = cos_stats(p, C, cnorm, st)) ||
        (rc = cos_assign(p, X, xnorm, rows, n, C, cnorm, assign, nullptr, nullptr, st, false)))
      return rc;
  } else {
    // the center-only work in three launches (prep_all), or as the separate
    // launches (CYC_KMEANS_PREP=0; an image of d > 256, whose screen packs
    // another center image)
    const bool fused = cyc::km8::prep_fused() &&
                       (!(rows && rows->usable) || cyc::km8::uses32(d));
    cyc::km8::Bounds bd{};
    // the one screen setup of the call: prep_all zeroes its counters, the
    // screen uses them
    ScreenSetup ss;
    if ((rc = screen_setup(p, rows, n, X, nullptr, C, cnorm, false, ss))) return rc;
    // the rows' half of the require check: once per image (RowVerdict)
    const bool rowsChecked = rows && rows->verdict.holds(xnorm, n);
    const double* reqNorm = rowsChecked ? nullptr : xnorm;
    const int64_t reqRows = rowsChecked ? 0 : n;
    if (fused) {
      bool carry = false;
      if (useBnd && (rc = bounds_reserve(p, rows, n, st, carry))) return rc;
      if ((rc = prep_all(p, rows, reqNorm, reqRows, C, cnorm, useBnd, carry, &ss, st))) return rc;
      if (useBnd) {
        if ((rc = bounds_lists(p, rows, xnorm, n, st, bd, carry, true))) return rc;
        assign = (int32_t*)rows->bAssign.ptr;
      }
    } else {
      if ((rc = require_enqueue(p, C, reqNorm, reqRows, st))) return rc;
      if ((rc = do_stats(p, C, st))) return rc;
      if (useBnd) {
        if ((rc = bounds_prepare(p, rows, C, xnorm, n, st, bd))) return rc;
        assign = (int32_t*)rows->bAssign.ptr;
      }
    }
    AssignCall call{X, xnorm, rows, n, C, cnorm, assign};
    call.bounds = useBnd ? &bd : nullptr;
    call.approxNorm = approxNorm;
    call.prepared = fused;
    if ((rc = do_assign(p, call, ss, st))) return rc;
    if (useBnd) {
      rows->bValid = true;
      rows->bk = k;
      ++rows->bCalls;
      if (userAssign)
        CYC_HIP(hipMemcpyAsync(userAssign, assign, sizeof(int32_t) * (size_t)n,
                               hipMemcpyDeviceToDevice, st));
    }
  }
  const int nj = (d + 255) / 256;
  // incremental cluster sums (k_inc_*): with the carried bounds, unit
  // weights and no per-row costs asked for
  const bool useInc = useBnd && inc_on(rows) && !cost && !weights && nj <= 4;
  if (rows && !useInc) rows->inc.valid = false;
  if (useInc) {
    if ((rc = cyc::kmsums::inc_accumulate(p->sort, rows->inc, X, xnorm, assign, n, d, k, C, sums,
                                          wsum, cost_sum, st)))
      return rc;
    rc = require_check(p, n, approxNorm ? X : nullptr, &rows->verdict, xnorm);
    rows->inc.valid = rc == CYC_OK;
    rows->inc.k = k;
    return rc;
  }
  // d > 1024: per-row costs first (k_chunk_sums fuses them for d <= 1024);
  // cosine: always (the cost is a ddot, summed per row)
  if (cosm) {
    if (!cost) {
      if ((rc = p->costTmp.reserve(sizeof(double) * (size_t)n))) return rc;
      cost = (double*)p->costTmp.ptr;
    }
    if ((rc = cyc::kmcos::row_cost(X, n, d, C, cnorm, xnorm, assign, cost, st))) return rc;
  } else if (nj > 4) {
    if (!cost) {
      if ((rc = p->costTmp.reserve(sizeof(double) * (size_t)n))) return rc;
      cost = (double*)p->costTmp.ptr;
    }
    hipLaunchKernelGGL(k_row_cost, dim3((unsigned)((n + kNormRows - 1) / kNormRows)),
                     dim3(kNormRows), 0, st, X, n, d, C,
                       (const int32_t*)assign, cost);
    CYC_LAUNCH_CHECK("k_row_cost");
  }

  if ((rc = cyc::kmsums::full_pass(p->sort, X, n, d, k, weights, xnorm, cosm, C, assign, cost, sums,
                                   wsum, cost_sum, st)))
    return rc;
  return cosm ? cos_check(p)
              : require_check(p, n, approxNorm ? X : nullptr, rows ? &rows->verdict : nullptr,
                              xnorm);
}

int cyc_kmeans_update_dev(cyc_kmeans_plan p, double* C, double* cnorm, const double* sums,
                          const double* wsum, double epsilon, int32_t* converged_out,
                          void* stream) {
  CYC_REQUIRE(p != nullptr, "plan must not be null");
  CYC_REQUIRE(epsilon >= 0, "epsilon must be nonnegative");
  std::lock_guard<std::mutex> g(p->mu);
  hipStream_t st = cyc::as_stream(stream);
  if (converged_out) CYC_HIP(hipMemsetD32Async((hipDeviceptr_t)converged_out, 1, 1, st));
  if (is_cos(p))
    return cyc::kmcos::update(C, cnorm, sums, wsum, p->k, p->d, epsilon, converged_out, st);
  return cyc::kmsums::update_centers(C, cnorm, sums, wsum, p->k, p->d, epsilon * epsilon,
                                     converged_out, st);
}


// ---------------------------------------------------------------------------
// ClusteringEvaluator's Silhouette (ml/evaluation/ClusteringMetrics.scala,
// silhouette.hpp): the plan's measure picks SquaredEuclideanSilhouette
// (CYC_DISTANCE_EUCLIDEAN) or CosineSilhouette.
// ---------------------------------------------------------------------------
namespace {

// pred in [0, k) and checkNonNegativeWeight over the rows (host sync).
int sil_check(cyc_kmeans_plan p, const int32_t* pred, const double* w, int64_t n,
              hipStream_t st) {
  int rc;
  if ((rc = p->silFlags.reserve(16))) return rc;
  unsigned int* bad = (unsigned int*)p->silFlags.ptr;
  unsigned long long* badW = (unsigned long long*)((char*)p->silFlags.ptr + 8);
  CYC_HIP(hipMemsetAsync(bad, 0, 8, st));
  CYC_HIP(hipMemsetAsync(badW, 0xff, 8, st));
  if ((rc = cyc::silh::check_pred(pred, w, n, p->k, bad, badW, st))) return rc;
  unsigned long long h[2] = {0, 0};
  CYC_HIP(hipMemcpyAsync(h, p->silFlags.ptr, 16, hipMemcpyDeviceToHost, st));
  CYC_HIP(hipStreamSynchronize(st));
  if ((unsigned int)h[0] != 0u) {
    cyc::set_error("requirement failed: predictions must lie in [0, k) for k = " +
                   std::to_string(p->k));
    return CYC_ERR_INVALID_ARG;
  }
  if (h[1] != ~0ull) {
    double v = 0.0;
    CYC_HIP(hipMemcpy(&v, w + h[1], sizeof(double), hipMemcpyDeviceToHost));
    // ml/functions.scala:91
    cyc::set_error("requirement failed: illegal weight value: " + cyc::java_double(v) +
                   ". weight must be >= 0.0.");
    return CYC_ERR_INVALID_ARG;
  }
  return CYC_OK;
}

// Vectors.norm(features, 2.0) per row (given, or into the plan's buffer).
int sil_norms(cyc_kmeans_plan p, const double* X, const double* xnorm, int64_t n, hipStream_t st,
              const double*& out) {
  if (xnorm) {
    out = xnorm;
    return CYC_OK;
  }
  int rc;
  if ((rc = p->silNorms.reserve(sizeof(double) * (size_t)n))) return rc;
  if ((rc = cyc_row_norms_dev(X, n, p->d, (double*)p->silNorms.ptr, st))) return rc;
  out = (const double*)p->silNorms.ptr;
  return CYC_OK;
}

}  // namespace

int cyc_kmeans_silhouette_stats_dev(cyc_kmeans_plan p, const double* X, const double* xnorm,
                                    int64_t n, const int32_t* pred, const double* weights,
                                    double* stats, void* stream) {
  CYC_REQUIRE(p != nullptr, "plan must not be null");
  CYC_REQUIRE(n >= 0, "n >= 0");
  CYC_REQUIRE(stats != nullptr, "stats must not be null");
  if (n == 0) return CYC_OK;
  CYC_REQUIRE(X != nullptr && pred != nullptr, "X and pred must not be null");
  std::lock_guard<std::mutex> g(p->mu);
  hipStream_t st = cyc::as_stream(stream);
  int rc;
  const double* xn = nullptr;
  if ((rc = sil_check(p, pred, weights, n, st)) || (rc = sil_norms(p, X, xnorm, n, st, xn)))
    return rc;
  int64_t maxChunks = 0;
  if ((rc = cyc::kmsums::sort_clusters(p->sort, pred, n, p->d, p->k, st, maxChunks))) return rc;
  if ((rc = cyc::silh::chunk_sums(X, p->d, weights, xn, is_cos(p), (const int32_t*)p->sort.perm.ptr,
                                  (const int64_t*)p->sort.cstart.ptr,
                                  (const int64_t*)p->sort.chunkStart.ptr, p->k, maxChunks, kChunkRows,
                                  (double*)p->sort.part.ptr, (double*)p->sort.pw.ptr, (double*)p->sort.pc.ptr,
                                  st)))
    return rc;
  return cyc::silh::fold((const double*)p->sort.part.ptr, (const double*)p->sort.pw.ptr,
                         (const double*)p->sort.pc.ptr, (const int64_t*)p->sort.cstart.ptr,
                         (const int64_t*)p->sort.chunkStart.ptr, p->d, p->k, stats, st);
}

int cyc_kmeans_silhouette_score_dev(cyc_kmeans_plan p, const double* X, const double* xnorm,
                                    int64_t n, const int32_t* pred, const double* weights,
                                    const double* stats, double* partial, void* stream) {
  CYC_REQUIRE(p != nullptr, "plan must not be null");
  CYC_REQUIRE(n >= 0, "n >= 0");
  CYC_REQUIRE(stats != nullptr && partial != nullptr, "stats and partial must not be null");
  std::lock_guard<std::mutex> g(p->mu);
  hipStream_t st = cyc::as_stream(stream);
  const int k = p->k, d = p->d;
  // clustersStatsMap.size > 1 (ClusteringMetrics.scala:391 / :532): the
  // clusters with rows, over every rank's rows once stats are merged
  std::vector<double> cnt((size_t)k);
  CYC_HIP(hipMemcpyAsync(cnt.data(), stats + (int64_t)k * d + 2 * (int64_t)k,
                         sizeof(double) * (size_t)k, hipMemcpyDeviceToHost, st));
  CYC_HIP(hipStreamSynchronize(st));
  int present = 0;
  for (int c = 0; c < k; ++c) present += cnt[(size_t)c] > 0.0 ? 1 : 0;
  if (present <= 1) {
    cyc::set_error("assertion failed: Number of clusters must be greater than one.");
    return CYC_ERR_ASSERTION;
  }
  if (n == 0) return CYC_OK;
  CYC_REQUIRE(X != nullptr && pred != nullptr, "X and pred must not be null");
  int rc;
  const double* xn = nullptr;
  if ((rc = sil_check(p, pred, weights, n, st)) || (rc = sil_norms(p, X, xnorm, n, st, xn)))
    return rc;
  if ((rc = p->silPart.reserve(sizeof(double) * 2 * (size_t)((n + 63) / 64)))) return rc;
  return cyc::silh::score(X, xn, n, d, pred, weights, k, is_cos(p), stats,
                          (double*)p->silPart.ptr, partial, st);
}


int cyc_row_norms_csr_dev(const int64_t* rowptr, const double* vals, int64_t n, double* norms,
                          void* stream) {
  CYC_REQUIRE(n >= 0 && (n == 0 || (rowptr && norms)), "n >= 0 and non-null buffers");
  if (n == 0) return CYC_OK;
  return cyc::kmsparse::row_norms(rowptr, vals, n, norms, cyc::as_stream(stream));
}

namespace {
// findClosest for CSR rows with the plan's statistics (nostats: without)
int sparse_assign(cyc_kmeans_plan p, const int64_t* rowptr, const int32_t* colidx,
                  const double* vals, const double* xnorm, int64_t n, const double* C,
                  const double* cnorm, int32_t* assign, double* cost, hipStream_t st,
                  bool nostats = false) {
  return cyc::kmsparse::sparse_assign(rowptr, colidx, vals, xnorm, n, p->d, C, cnorm, p->k,
                                      nostats ? nullptr : (const double*)p->stats.ptr, assign,
                                      cost, st);
}
}  // namespace

int cyc_kmeans_assign_csr_dev(cyc_kmeans_plan p, const int64_t* rowptr, const int32_t* colidx,
                              const double* vals, const double* xnorm, int64_t n, const double* C,
                              const double* cnorm, int32_t* assign, double* cost, void* stream) {
  CYC_REQUIRE(p != nullptr, "plan must not be null");
  CYC_REQUIRE(n >= 0, "n >= 0");
  CYC_REQUIRE(assign != nullptr && cost != nullptr, "assign and cost must not be null");
  if (n == 0) return CYC_OK;
  std::lock_guard<std::mutex> g(p->mu);
  hipStream_t st = cyc::as_stream(stream);
  int rc;
  if (is_cos(p)) {
    if ((rc = cos_enqueue(p, cnorm, true, xnorm, n, st)) ||
        (rc = cyc::kmcos::assign_sparse(rowptr, colidx, vals, xnorm, n, p->d, C, cnorm, p->k,
                                        (const double*)p->stats.ptr, assign, cost, st)))
      return rc;
    return cos_check(p);
  }
  if ((rc = require_enqueue(p, C, xnorm, n, st))) return rc;
  if ((rc = sparse_assign(p, rowptr, colidx, vals, xnorm, n, C, cnorm, assign, cost, st)))
    return rc;
  return require_check(p, n);
}

int cyc_kmeans_point_cost_csr_dev(cyc_kmeans_plan p, const int64_t* rowptr,
                                  const int32_t* colidx, const double* vals, const double* xnorm,
                                  int64_t n, const double* C, const double* cnorm,
                                  int32_t* assign, double* cost, void* stream) {
  CYC_REQUIRE(p != nullptr, "plan must not be null");
  CYC_REQUIRE(n >= 0, "n >= 0");
  CYC_REQUIRE(assign != nullptr && cost != nullptr, "assign and cost must not be null");
  if (n == 0) return CYC_OK;
  std::lock_guard<std::mutex> g(p->mu);
  hipStream_t st = cyc::as_stream(stream);
  if (is_cos(p)) {
    int rc;
    if ((rc = cos_enqueue(p, cnorm, true, xnorm, n, st)) ||
        (rc = cyc::kmcos::assign_sparse(rowptr, colidx, vals, xnorm, n, p->d, C, cnorm, p->k,
                                        nullptr, assign, cost, st)))
      return rc;
    hipLaunchKernelGGL(k_nostats_cost_fix, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n,
                       cost);
    CYC_LAUNCH_CHECK("k_nostats_cost_fix");
    return cos_check(p);
  }
  return sparse_assign(p, rowptr, colidx, vals, xnorm, n, C, cnorm, assign, cost, st, true);
}

int cyc_kmeans_accumulate_csr_dev(cyc_kmeans_plan p, const int64_t* rowptr,
                                  const int32_t* colidx, const double* vals, const double* xnorm,
                                  const double* weights, int64_t n, const double* C,
                                  const double* cnorm, double* sums, double* wsum,
                                  double* cost_sum, int32_t* assign, double* cost, void* stream) {
  CYC_REQUIRE(p != nullptr, "plan must not be null");
  CYC_REQUIRE(n >= 0, "n >= 0");
  CYC_REQUIRE(sums && wsum && cost_sum, "sums, wsum and cost_sum must not be null");
  if (n == 0) return CYC_OK;
  std::lock_guard<std::mutex> g(p->mu);
  hipStream_t st = cyc::as_stream(stream);
  int rc;
  if (!assign) {
    if ((rc = p->assignTmp.reserve(sizeof(int32_t) * (size_t)n))) return rc;
    assign = (int32_t*)p->assignTmp.ptr;
  }
  if (!cost) {
    if ((rc = p->costTmp.reserve(sizeof(double) * (size_t)n))) return rc;
    cost = (double*)p->costTmp.ptr;
  }
  if (is_cos(p)) {
    if ((rc = cos_enqueue(p, cnorm, true, xnorm, n, st)) || (rc = cos_stats(p, C, cnorm, st)) ||
        (rc = cyc::kmcos::assign_sparse(rowptr, colidx, vals, xnorm, n, p->d, C, cnorm, p->k,
                                        (const double*)p->stats.ptr, assign, cost, st)) ||
        (rc = cyc::kmsparse::cluster_sums(rowptr, colidx, vals, weights, xnorm, n, p->d, p->k,
                                          assign, cost, sums, wsum, cost_sum, st)))
      return rc;
    return cos_check(p);
  }
  if ((rc = require_enqueue(p, C, xnorm, n, st))) return rc;
  if ((rc = do_stats(p, C, st))) return rc;
  if ((rc = sparse_assign(p, rowptr, colidx, vals, xnorm, n, C, cnorm, assign, cost, st)))
    return rc;
  if ((rc = cyc::kmsparse::cluster_sums(rowptr, colidx, vals, weights, nullptr, n, p->d, p->k,
                                        assign, cost, sums, wsum, cost_sum, st)))
    return rc;
  return require_check(p, n);
}

}  // extern "C"
