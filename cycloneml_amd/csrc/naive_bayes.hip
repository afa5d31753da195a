// naive_bayes.hip -- NaiveBayes on gfx950 (MI355X): the per-class aggregate of
// ml/classification/NaiveBayes.scala over dense fp64 rows for the four model
// types (multinomial, complement, bernoulli, gaussian).  The model comes from
// the aggregate in closed form on the host (cycloneml_amd/naive_bayes.py).
//
// Aggregate.  sums is one fp64 buffer [W (C) | S (C x d, row-major) | Q (C x d,
// gaussian only)]: W_c = sum of w_i, S_c[j] = sum of w_i x_ij, Q_c[j] = sum of
// w_i (x_ij x_ij) over the rows of label c.  Calls ADD into it.
//
// Kernels
//   k_nb_agg<GAUSS>  dense rows.  The d + 1 columns of a row are its features
//                    and a column of ones (whose sum is W_c).  A run is
//                    kRunRows consecutive rows; T = col_tile lanes, one per
//                    column, own one run x T columns, and a workgroup of 256
//                    lanes holds 256 / T consecutive runs.  Labels and weights
//                    are staged in LDS kStage rows at a time (checked there: a
//                    bad label becomes -1 and is never used as an index).  The
//                    per-class accumulators live in LDS, acc[class][lane]: a
//                    lane alone owns its column, so a run's rows are added in
//                    row order with no conflict.  classes_per_pass classes fit
//                    (16, gaussian 8 + 8); blockIdx.z walks the passes, and a
//                    row outside the pass is not loaded, so X is streamed
//                    once whatever C is.  Every (run, class, column) partial
//                    goes to the workspace.
//   k_nb_fold        sums[e] = (..((sums[e] + run 0) + run 1) ..): one thread
//                    per entry, the runs in order.  The workspace holds
//                    `group` runs; a smaller workspace means more launches of
//                    the pair, and since the fold is one chain in run order
//                    the sums do not depend on the grouping.
// No atomics on doubles: every sum has one fixed order, so two calls on the
// same inputs give the same bits.  (The lowest offending row is an integer
// atomicMin.)
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <string>
#include <vector>

#include "common.hpp"

enum { NB_MULTINOMIAL = 0, NB_COMPLEMENT = 1, NB_BERNOULLI = 2, NB_GAUSSIAN = 3 };
enum { NB_RULE_NONE = 0, NB_RULE_LABEL = 1, NB_RULE_WEIGHT = 2, NB_RULE_VALUE = 3 };

struct cyc_nb_plan_s {
  std::mutex mu;
  int C = 0, d = 0, type = 0;
  int64_t wsBytes = 0;
  cyc::DeviceBuffer ws, bad;
};

namespace {

constexpr int kMaxClasses = 1024;
constexpr int kRunRows = 1024;              // rows per run of the dense aggregate
constexpr int kStage = 64;                  // rows of labels / weights staged at a time
constexpr int kAccSlots = 16;               // LDS accumulator rows of 256 doubles
constexpr int kMinTile = 16, kMaxTile = 256;
constexpr int kMaxColBlocks = 65535;        // gridDim.y
constexpr int64_t kDefaultWorkspace = (int64_t)256 << 20;
constexpr unsigned long long kNoBad = ~0ull;

inline int col_tile(int d) {
  int t = kMinTile;
  while (t < kMaxTile && t < d + 1) t <<= 1;
  return t;
}
inline int classes_per_pass(int type) { return type == NB_GAUSSIAN ? kAccSlots / 2 : kAccSlots; }

__device__ __forceinline__ void nb_flag(unsigned long long* bad, int64_t row, int rule) {
  atomicMin(bad, (unsigned long long)row * 8ull + (unsigned long long)rule);
}

// the label of a row as a class index, or -1 (never an index)
__device__ __forceinline__ int nb_label(double y, int C) {
  if (!(y >= 0.0 && y < (double)C)) return -1;
  const int c = (int)y;
  return (double)c == y ? c : -1;
}

// ws[(run len) + (gauss C (d + 1)) + c (d + 1) + col], col == d: the ones
template <bool GAUSS>
__global__ __launch_bounds__(256) void k_nb_agg(
    const double* __restrict__ X, const double* __restrict__ y, const double* __restrict__ w,
    int64_t n, int64_t row0, int64_t runs, int d, int C, int T, int type,
    double* __restrict__ ws, int64_t len, unsigned long long* __restrict__ bad) {
  constexpr int P = GAUSS ? kAccSlots / 2 : kAccSlots;
  __shared__ double acc[kAccSlots][256];
  __shared__ double wS[256 / kMinTile][kStage];
  __shared__ int labS[256 / kMinTile][kStage];
  const int tid = threadIdx.x;
  const int slots = 256 / T, slot = tid / T, lc = tid % T;
  const int col = blockIdx.y * T + lc;
  const int64_t run = (int64_t)blockIdx.x * slots + slot;
  const bool runOk = run < runs;
  const int64_t r0 = runOk ? std::min<int64_t>(n, row0 + run * kRunRows) : n;
  const int64_t r1 = std::min<int64_t>(n, r0 + kRunRows);
  const int c0 = blockIdx.z * P;
  const bool checks = blockIdx.y == 0 && blockIdx.z == 0;
#pragma unroll
  for (int s = 0; s < kAccSlots; ++s) acc[s][tid] = 0.0;
  for (int base = 0; base < kRunRows; base += kStage) {
    __syncthreads();   // the previous stage is consumed
    for (int i = lc; i < kStage; i += T) {
      const int64_t row = r0 + base + i;
      int lb = -1;
      double wv = 0.0;
      if (row < r1) {
        const double yv = y[row];
        wv = w ? w[row] : 1.0;
        lb = nb_label(yv, C);
        if (lb < 0) {
          if (checks) nb_flag(bad, row, NB_RULE_LABEL);
        } else if (!(wv >= 0.0)) {
          if (checks) nb_flag(bad, row, NB_RULE_WEIGHT);
          lb = -1;
        }
      }
      labS[slot][i] = lb;
      wS[slot][i] = wv;
    }
    __syncthreads();
    if (!runOk || col > d) continue;
    for (int i0 = 0; i0 < kStage; i0 += 8) {
      double xv[8];
      int lb[8];
      // the loads of 8 rows before their adds
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        lb[u] = labS[slot][i0 + u];
        const bool in = lb[u] >= c0 && lb[u] < c0 + P;
        lb[u] = in ? lb[u] - c0 : -1;
        xv[u] = 1.0;
        if (in && col < d) xv[u] = X[(r0 + base + i0 + u) * d + col];
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        if (lb[u] < 0) continue;
        const double x = xv[u], wv = wS[slot][i0 + u];
        if (col < d) {
          const bool okv = type == NB_GAUSSIAN ? true
                           : type == NB_BERNOULLI ? (x == 0.0 || x == 1.0)
                                                  : (x >= 0.0);
          if (!okv) nb_flag(bad, r0 + base + i0 + u, NB_RULE_VALUE);
        }
        acc[lb[u]][tid] += wv * x;
        if constexpr (GAUSS) acc[P + lb[u]][tid] += wv * (x * x);
      }
    }
  }
  if (!runOk || col > d) return;
  double* out = ws + run * len;
  const int64_t cd = (int64_t)C * (d + 1);
  for (int c = 0; c < P && c0 + c < C; ++c) {
    out[(int64_t)(c0 + c) * (d + 1) + col] = acc[c][tid];
    if constexpr (GAUSS) out[cd + (int64_t)(c0 + c) * (d + 1) + col] = acc[P + c][tid];
  }
}

// entry e of a run's part [S' (C x (d + 1)) | Q' (C x (d + 1))] -> its place
// in [W | S (C x d) | Q (C x d)], or -1 (the ones column of Q')
__device__ __forceinline__ int64_t nb_dest(int64_t e, int C, int d) {
  const int64_t cd = (int64_t)C * (d + 1);
  const bool q = e >= cd;
  if (q) e -= cd;
  const int64_t c = e / (d + 1);
  const int col = (int)(e % (d + 1));
  if (col == d) return q ? -1 : c;
  return C + (q ? (int64_t)C * d : 0) + c * d + col;
}

// sums += the parts in order
__global__ __launch_bounds__(256) void k_nb_fold(const double* __restrict__ ws, int64_t parts,
                                                 int64_t len, int C, int d,
                                                 double* __restrict__ sums) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < len;
       e += (int64_t)gridDim.x * 256) {
    const int64_t dst = nb_dest(e, C, d);
    if (dst < 0) continue;
    double s = sums[dst];
    for (int64_t r = 0; r < parts; ++r) s += ws[r * len + e];
    sums[dst] = s;
  }
}

int reset_bad(cyc_nb_plan_s* p, hipStream_t st) {
  if (int rc = p->bad.reserve(sizeof(unsigned long long))) return rc;
  CYC_HIP(hipMemsetAsync(p->bad.ptr, 0xff, sizeof(unsigned long long), st));
  return CYC_OK;
}

int read_bad(cyc_nb_plan_s* p, hipStream_t st, int64_t* row, int* rule) {
  unsigned long long v = 0;
  CYC_HIP(hipMemcpyAsync(&v, p->bad.ptr, sizeof(v), hipMemcpyDeviceToHost, st));
  CYC_HIP(hipStreamSynchronize(st));
  *row = v == kNoBad ? -1 : (int64_t)(v >> 3);
  *rule = v == kNoBad ? NB_RULE_NONE : (int)(v & 7);
  return CYC_OK;
}

bool value_ok(int type, double x) {
  if (type == NB_GAUSSIAN) return true;
  if (type == NB_BERNOULLI) return x == 0.0 || x == 1.0;
  return x >= 0.0;
}

// the message of the lowest offending row; vals: the row's nv values
int refuse(cyc_nb_plan_s* p, int64_t row, int rule, const double* y, const double* w,
           const double* vals, int64_t nv) {
  std::string at = " (row " + std::to_string(row) + ")";
  double v = 0.0;
  if (rule == NB_RULE_LABEL) {
    CYC_HIP(hipMemcpy(&v, y + row, sizeof(v), hipMemcpyDeviceToHost));
    cyc::set_error("requirement failed: Classification labels should be integers in [0 to " +
                   std::to_string(p->C - 1) + "]. Found " + cyc::java_double(v) + "." + at);
    return CYC_ERR_INVALID_ARG;
  }
  if (rule == NB_RULE_WEIGHT) {
    CYC_HIP(hipMemcpy(&v, w + row, sizeof(v), hipMemcpyDeviceToHost));
    cyc::set_error("requirement failed: illegal weight value: " + cyc::java_double(v) +
                   ". weight must be >= 0.0." + at);
    return CYC_ERR_INVALID_ARG;
  }
  std::vector<double> h((size_t)nv);
  if (nv) CYC_HIP(hipMemcpy(h.data(), vals, sizeof(double) * (size_t)nv, hipMemcpyDeviceToHost));
  for (double x : h)
    if (!value_ok(p->type, x)) {
      v = x;
      break;
    }
  cyc::set_error(std::string("requirement failed: ") +
                 (p->type == NB_BERNOULLI
                      ? "Bernoulli naive Bayes requires 0 or 1 feature values but found "
                      : "Naive Bayes requires nonnegative feature values but found ") +
                 cyc::java_double(v) + "." + at);
  return CYC_ERR_INVALID_ARG;
}

// sums += the aggregate of n rows, the runs in groups the workspace holds
int aggregate_runs(cyc_nb_plan_s* p, const double* X, const double* y, const double* w,
                   int64_t n, double* sums, hipStream_t st) {
  const int dw = p->d;
  const bool gauss = p->type == NB_GAUSSIAN;
  const int64_t len = (int64_t)p->C * (dw + 1) * (gauss ? 2 : 1);
  const int64_t runs = (n + kRunRows - 1) / kRunRows;
  const int64_t group = std::min(runs, std::max<int64_t>(1, p->wsBytes / (8 * len)));
  if (int rc = p->ws.reserve(sizeof(double) * (size_t)(group * len))) return rc;
  const int T = col_tile(dw), slots = 256 / T;
  const int P = gauss ? kAccSlots / 2 : kAccSlots;
  const unsigned colBlocks = (unsigned)((dw + T) / T), passes = (unsigned)((p->C + P - 1) / P);
  for (int64_t g0 = 0; g0 < runs; g0 += group) {
    const int64_t gr = std::min(group, runs - g0);
    const dim3 grid((unsigned)((gr + slots - 1) / slots), colBlocks, passes);
    {
      cyc::KernelTimer timer("k_nb_agg", st);
      if (gauss)
        hipLaunchKernelGGL(k_nb_agg<true>, grid, dim3(256), 0, st, X, y, w, n, g0 * kRunRows, gr,
                           dw, p->C, T, p->type, (double*)p->ws.ptr, len,
                           (unsigned long long*)p->bad.ptr);
      else
        hipLaunchKernelGGL(k_nb_agg<false>, grid, dim3(256), 0, st, X, y, w, n, g0 * kRunRows, gr,
                           dw, p->C, T, p->type, (double*)p->ws.ptr, len,
                           (unsigned long long*)p->bad.ptr);
      CYC_LAUNCH_CHECK("k_nb_agg");
    }
    cyc::KernelTimer timer("k_nb_fold", st);
    hipLaunchKernelGGL(k_nb_fold, dim3((unsigned)std::min<int64_t>((len + 255) / 256, 4096)),
                       dim3(256), 0, st, (const double*)p->ws.ptr, gr, len, p->C, dw, sums);
    CYC_LAUNCH_CHECK("k_nb_fold");
  }
  return CYC_OK;
}

}  // namespace

extern "C" {

int cyc_nb_plan_create(int32_t numClasses, int32_t numFeatures, int32_t modelType,
                       int64_t workspaceBytes, cyc_nb_plan* plan) {
  CYC_REQUIRE(plan != nullptr, "plan must not be null");
  CYC_REQUIRE(numClasses >= 1 && numClasses <= kMaxClasses,
              "NaiveBayes supports 1 to " + std::to_string(kMaxClasses) + " classes but got " +
                  std::to_string(numClasses));
  CYC_REQUIRE(numFeatures >= 1,
              "numFeatures must be positive but got " + std::to_string(numFeatures));
  // the column blocks of the d + 1 columns are the grid's y extent
  CYC_REQUIRE((int64_t)numFeatures + 1 <= (int64_t)kMaxColBlocks * kMaxTile,
              "NaiveBayes supports up to " +
                  std::to_string((int64_t)kMaxColBlocks * kMaxTile - 1) +
                  " features but got " + std::to_string(numFeatures));
  CYC_REQUIRE(modelType >= NB_MULTINOMIAL && modelType <= NB_GAUSSIAN,
              "modelType must be 0 (multinomial), 1 (complement), 2 (bernoulli) or 3 (gaussian) "
              "but got " + std::to_string(modelType));
  CYC_REQUIRE(workspaceBytes >= 0, "workspaceBytes must not be negative");
  CYC_REQUIRE((int64_t)numClasses * ((int64_t)numFeatures + 1) <= INT32_MAX / 2,
              std::to_string(numClasses) + " x " + std::to_string(numFeatures) +
                  " dense matrix is too large to allocate");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    cyc::set_error("no HIP device visible");
    return CYC_ERR_NO_DEVICE;
  }
  auto* p = new cyc_nb_plan_s();
  p->C = numClasses;
  p->d = numFeatures;
  p->type = modelType;
  p->wsBytes = workspaceBytes ? workspaceBytes : kDefaultWorkspace;
  *plan = p;
  return CYC_OK;
}

int cyc_nb_plan_destroy(cyc_nb_plan plan) {
  delete plan;
  return CYC_OK;
}

int64_t cyc_nb_col_tile(cyc_nb_plan plan) { return plan ? col_tile(plan->d) : -1; }
int64_t cyc_nb_rows_per_run(cyc_nb_plan plan) { return plan ? kRunRows : -1; }
int64_t cyc_nb_classes_per_pass(cyc_nb_plan plan) {
  return plan ? classes_per_pass(plan->type) : -1;
}

int cyc_nb_aggregate_dev(cyc_nb_plan plan, const double* X, int64_t nrows, const double* y,
                         const double* w, double* sums, int64_t* badRow, int32_t* badRule,
                         void* stream) {
  CYC_REQUIRE(plan != nullptr, "plan must not be null");
  CYC_REQUIRE(nrows >= 0, "nrows >= 0");
  CYC_REQUIRE(sums != nullptr, "sums must not be null");
  if (badRow) *badRow = -1;
  if (badRule) *badRule = NB_RULE_NONE;
  if (nrows == 0) return CYC_OK;
  CYC_REQUIRE(X != nullptr && y != nullptr, "non-null rows and labels");
  cyc_nb_plan_s* p = plan;
  hipStream_t st = cyc::as_stream(stream);
  std::lock_guard<std::mutex> g(p->mu);
  if (int rc = reset_bad(p, st)) return rc;
  if (int rc = aggregate_runs(p, X, y, w, nrows, sums, st)) return rc;
  int64_t row = -1;
  int rule = 0;
  if (int rc = read_bad(p, st, &row, &rule)) return rc;
  if (rule == NB_RULE_NONE) return CYC_OK;
  if (badRow) *badRow = row;
  if (badRule) *badRule = rule;
  return refuse(p, row, rule, y, w, X + row * p->d, p->d);
}

}  // extern "C"
