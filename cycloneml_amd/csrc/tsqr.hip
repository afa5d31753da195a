// tsqr.hip -- R of X = Q R on gfx950 (MI355X) for a tall X (m x n, row-major
// fp64, n <= 1024): RowMatrix.tallSkinnyQR (mllib/linalg/distributed/
// RowMatrix.scala, tallSkinnyQR: qr.reduced per partition, the stacked R's
// reduced pairwise).  Householder reflectors throughout, never the Gramian:
// the error of R follows cond(X), not cond(X)^2.
//
// Layout.  NP = n rounded up to 16, NB = NP / 16 panels.  A running R is an
// NP x NP row-major slab in the plan's workspace (zeros below the diagonal and
// in the padding), private to one workgroup.  The shard is cut into runs of
// kRunRows rows counted from row 0, whatever the device or the workspace.
//
// Kernels
//   k_tsqr_run     one workgroup (8 waves) per run: folds the run's rows,
//                  tile after tile, into its slab (feed_rows below).
//   k_tsqr_fold    one workgroup: feeds `count` triangles, in index order and
//                  one at a time, into one slab through the same feed_rows.
//                  Serves the runs of a launch and the ranks' R's.  A tile
//                  of triangle rows [t0, t0 + T) is zero left of column t0:
//                  panels left of it are skipped.
//   k_tsqr_copy    slab -> n x n row-major, explicit zeros below the diagonal.
//   k_tsqr_finish  the sign rule: rows with a negative diagonal are negated.
//
// feed_rows: the triangle-on-top-of-rectangle update.  A tile of T =
// tile_rows(n) rows is staged in LDS with row stride LD = NP + 8 (rows 8 or 24
// doubles apart modulo 32: the four rows of an MFMA operand read fall on
// different banks).  Every thread keeps 32 slots of the NEXT tile in
// registers, loaded (coalesced, once) before the update of the current one
// starts; a slot is (row, column) of a grid 2^sh columns wide, 2^sh the power
// of two >= NP, so T = min(64, 16384 >> sh): 64 rows up to n = 256, 32 up to
// 512, 16 up to 1024 (128 KiB of rows, 140 KiB of LDS with padding and panel
// scratch).  Per panel p of 16 columns, left to right:
//   factor  (wave 0)  Householder QR of the stack [R_pp ; A_p].  R_pp is
//           upper triangular, so reflector j is e_j plus a vector v_j on the
//           tile rows only; V (T x 16) overwrites A_p.  Lane (c, q) = (lane &
//           15, lane >> 4) owns column c of rows [q T/4, (q + 1) T/4): one
//           sweep gives a_j . a_c for all c (its four quarters added in a fixed
//           order by two xor-shuffles), i.e. the norm (c == j), the
//           projections (c > j) and v_j . v_c for the compact-WY factor Tf
//           (c < j).  norm == 0: tau = 0, the column is left as it is.
//   update  (all waves, 16-column blocks b > p round-robin) on
//           v_mfma_f64_16x16x4_f64:
//             S = R_pb + V^T A_b      T / 4 MFMAs, both operands from LDS
//             W = Tf^T S              4 MFMAs; S goes in as the B operand
//                                     straight from its accumulator registers
//                                     (k-step kk takes rows g + 4 kk)
//             R_pb -= W
//             A_b -= V W              4 MFMAs per 16 rows, W from registers
// No atomics, every sum in a fixed order: the same bytes on every call and for
// every workspace size.  NaN / Inf propagate; nothing is indexed by data.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <string>

#include "common.hpp"

namespace {

constexpr int kPanel = 16;
constexpr int kWaves = 8;
constexpr int kThreads = 64 * kWaves;
constexpr int kRunRows = 16384;
constexpr int kTileDoubles = 16384;            // 128 KiB of rows per tile
constexpr int kPf = kTileDoubles / kThreads;   // doubles of the next tile per thread
constexpr int kLdPad = 8;
constexpr int kMaxCols = 1024;
constexpr int kDefaultRunsPerLaunch = 512;

inline int pad16(int n) { return (n + kPanel - 1) / kPanel * kPanel; }
inline int log2_cols(int n) {
  int sh = 4;
  while ((1 << sh) < n) ++sh;
  return sh;
}
// the rows of kTileDoubles slots of 2^sh columns, at most 64
inline int tile_rows(int n) { return std::min(64, kTileDoubles >> log2_cols(n)); }
inline size_t lds_bytes(int n) {
  return sizeof(double) * ((size_t)tile_rows(n) * (pad16(n) + kLdPad) + 2 * kPanel * kPanel);
}
inline size_t slab_doubles(int n) { return (size_t)pad16(n) * pad16(n); }

struct Geom {
  int n, NP, T, LD, sh;   // 2^sh: the power of two >= NP
};

// Householder QR of [R_pp ; A_p] by one wave.  A = the tile at column 16 p,
// rpp / tf = 16 x 16 LDS scratch, Rp = the slab at (16 p, 16 p).
__device__ __forceinline__ void factor_panel(double* __restrict__ A, int T, int LD,
                                             double* __restrict__ rpp, double* __restrict__ tf,
                                             double* __restrict__ Rp, int NP, int lane) {
  const int c = lane & 15, q = lane >> 4;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int e = lane + 64 * k;
    rpp[e] = Rp[(e >> 4) * NP + (e & 15)];
    tf[e] = 0.0;
  }
  __builtin_amdgcn_wave_barrier();
  const int i0 = q * (T / 4), i1 = i0 + T / 4;
  for (int j = 0; j < kPanel; ++j) {
    double d = 0.0;
    for (int i = i0; i < i1; ++i) d += A[i * LD + j] * A[i * LD + c];
    d = d + __shfl_xor(d, 16);
    d = d + __shfl_xor(d, 32);
    const double sigma = __shfl(d, j);
    if (sigma == 0.0) continue;   // tau = 0 (uniform over the wave): column and Tf untouched
    const double alpha = rpp[j * 16 + j];
    const double norm = __builtin_sqrt(alpha * alpha + sigma);
    const double beta = alpha > 0.0 ? -norm : norm;
    const double tau = (beta - alpha) / beta;
    const double scale = 1.0 / (alpha - beta);
    const double rjc = rpp[j * 16 + c];
    const double z = d * scale;                       // v_j . a_c (c > j), v_j . v_c (c < j)
    const double w = tau * (rjc + z);
    for (int i = i0; i < i1; ++i) {
      const double v = A[i * LD + j] * scale;
      if (c > j) A[i * LD + c] -= v * w;
      else if (c == j) A[i * LD + j] = v;
    }
    // Tf(0:j, j) = -tau Tf(0:j, 0:j) (V(:, 0:j)^T v_j), Tf(j, j) = tau; lane c holds row c
    double s = 0.0;
    for (int k = 0; k < j; ++k) {
      const double zk = __shfl(z, k);
      if (k >= c) s += tf[c * 16 + k] * zk;
    }
    if (q == 0) {
      if (c > j) rpp[j * 16 + c] = rjc - w;
      else if (c == j) {
        rpp[j * 16 + j] = beta;
        tf[j * 16 + j] = tau;
      } else {
        tf[c * 16 + j] = -tau * s;
      }
    }
    __builtin_amdgcn_wave_barrier();
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int e = lane + 64 * k;
    Rp[(e >> 4) * NP + (e & 15)] = (e & 15) >= (e >> 4) ? rpp[e] : 0.0;
  }
}

// Block b of the trailing update of panel p, by one wave.
__device__ __forceinline__ void update_block(double* __restrict__ tile, const Geom& G, int p,
                                             int b, const double* __restrict__ tf,
                                             double* __restrict__ R, int lane) {
  const int c = lane & 15, g = lane >> 4, LD = G.LD;
  const double* V = tile + 16 * p;
  double* Ab = tile + 16 * b;
  double* Rpb = R + (size_t)(16 * p) * G.NP + 16 * b;
  double rold[4];
  cyc_double4 S, W = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int r = 0; r < 4; ++r) S[r] = rold[r] = Rpb[(g + 4 * r) * G.NP + c];
  for (int k0 = 0; k0 < G.T; k0 += 4)
    S = __builtin_amdgcn_mfma_f64_16x16x4f64(V[(k0 + g) * LD + c], Ab[(k0 + g) * LD + c], S, 0, 0,
                                             0);
#pragma unroll
  for (int kk = 0; kk < 4; ++kk)
    W = __builtin_amdgcn_mfma_f64_16x16x4f64(tf[(g + 4 * kk) * 16 + c], S[kk], W, 0, 0, 0);
#pragma unroll
  for (int r = 0; r < 4; ++r) Rpb[(g + 4 * r) * G.NP + c] = rold[r] - W[r];
  for (int t = 0; t < G.T; t += 16) {
    cyc_double4 acc;
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] = Ab[(t + g + 4 * r) * LD + c];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk)
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(-V[(t + c) * LD + g + 4 * kk], W[kk], acc, 0, 0,
                                                 0);
#pragma unroll
    for (int r = 0; r < 4; ++r) Ab[(t + g + 4 * r) * LD + c] = acc[r];
  }
}

// Folds rows [0, nrows) of src (row r at src + r ld, n columns) into the slab
// R.  tri: the rows are an upper triangle (entries left of the diagonal are
// taken as zero, panels left of a tile skipped).  Called by the whole
// workgroup; R's earlier writes need no barrier before the call.
__device__ void feed_rows(const double* __restrict__ src, int64_t nrows, int ld, bool tri,
                          const Geom& G, double* __restrict__ R, double* __restrict__ lds) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int NB = G.NP / kPanel;
  double* tile = lds;
  double* rpp = lds + (size_t)G.T * G.LD;
  double* tf = rpp + kPanel * kPanel;
  // Slot idx = tid + 512 k of the next tile is row idx >> sh, column idx &
  // (2^sh - 1), 2^sh the power of two >= NP: shifts only, nothing kept per
  // slot but its double.  An absent slot (past the rows, past column n, left
  // of a triangle's diagonal) reads offset 0 and is stored as zero.
  double pf[kPf];
  unsigned present = 0;
  const int sh = G.sh, cmask = (1 << sh) - 1;
  // slot indices are rebuilt from an opaque copy of tid at every use: hoisted
  // out of the tile loop they would hold ~100 registers across the update
  auto opaque_tid = [&]() {
    int t = tid;
    asm volatile("" : "+v"(t));
    return t;
  };
  auto load = [&](int64_t r0) {
    const int t0 = opaque_tid();
    const int rows = (int)std::min<int64_t>(G.T, nrows - r0);
    const int d0 = tri ? (int)r0 : -(1 << 20);   // column of row 0's diagonal
    const double* base = src + r0 * ld;
    present = 0;
#pragma unroll
    for (int k = 0; k < kPf; ++k) {
      const int idx = t0 + k * kThreads, row = idx >> sh, col = idx & cmask;
      const bool in = row < rows && col < G.n && col >= d0 + row;
      pf[k] = base[in ? row * ld + col : 0];
      present |= (unsigned)in << k;
    }
  };
  load(0);
  for (int64_t r0 = 0; r0 < nrows; r0 += G.T) {
    __syncthreads();   // the previous tile is done with, R's writes are visible
    const int t0 = opaque_tid();
#pragma unroll
    for (int k = 0; k < kPf; ++k) {
      const int idx = t0 + k * kThreads, row = idx >> sh, col = idx & cmask;
      if (row < G.T && col < G.NP) tile[row * G.LD + col] = (present >> k & 1) ? pf[k] : 0.0;
    }
    if (r0 + G.T < nrows) load(r0 + G.T);
    for (int p = tri ? (int)(r0 / kPanel) : 0; p < NB; ++p) {
      __syncthreads();
      if (wave == 0)
        factor_panel(tile + 16 * p, G.T, G.LD, rpp, tf, R + (size_t)(16 * p) * G.NP + 16 * p,
                     G.NP, lane);
      __syncthreads();
      for (int b = p + 1 + wave; b < NB; b += kWaves) update_block(tile, G, p, b, tf, R, lane);
    }
  }
  __syncthreads();
}

__device__ __forceinline__ void zero_slab(double* __restrict__ R, int NP) {
  for (int e = threadIdx.x; e < NP * NP; e += kThreads) R[e] = 0.0;
}

__global__ __launch_bounds__(kThreads) void k_tsqr_run(const double* __restrict__ X, int64_t m,
                                                       Geom G, int64_t run0,
                                                       double* __restrict__ slabs) {
  extern __shared__ double lds[];
  double* R = slabs + (size_t)blockIdx.x * G.NP * G.NP;
  zero_slab(R, G.NP);
  const int64_t r0 = (run0 + blockIdx.x) * kRunRows;
  feed_rows(X + r0 * G.n, std::min<int64_t>(kRunRows, m - r0), G.n, false, G, R, lds);
}

// triangle i: rows [0, n) at src + i triStride, row stride ld
__global__ __launch_bounds__(kThreads) void k_tsqr_fold(const double* __restrict__ src,
                                                        int64_t count, int64_t triStride,
                                                        int ld, Geom G, int init,
                                                        double* __restrict__ R) {
  extern __shared__ double lds[];
  if (init) zero_slab(R, G.NP);
  for (int64_t i = 0; i < count; ++i) feed_rows(src + i * triStride, G.n, ld, true, G, R, lds);
}

__global__ __launch_bounds__(256) void k_tsqr_copy(const double* __restrict__ R, int n, int NP,
                                                   double* __restrict__ out) {
  for (int e = blockIdx.x * 256 + threadIdx.x; e < n * n; e += gridDim.x * 256) {
    const int i = e / n, j = e - i * n;
    out[e] = j >= i ? R[i * NP + j] : 0.0;
  }
}

// row blockIdx.x: every thread reads the diagonal before any of them writes
__global__ __launch_bounds__(256) void k_tsqr_finish(double* __restrict__ R, int n) {
  const int i = blockIdx.x;
  const double d = R[(size_t)i * n + i];
  __syncthreads();
  if (d < 0.0)
    for (int j = i + threadIdx.x; j < n; j += 256) R[(size_t)i * n + j] = -R[(size_t)i * n + j];
}

}  // namespace

struct cyc_tsqr_plan_s {
  Geom G;
  size_t workspaceBytes = 0;   // 0: sized per call
  std::mutex mu;
  cyc::DeviceBuffer ws;        // slab 0: the running R; slabs 1..: the runs of a launch
};

namespace {

int allow_lds(const cyc_tsqr_plan_s* p) {
  const int bytes = (int)lds_bytes(p->G.n);
  CYC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_tsqr_run),
                              hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
  CYC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_tsqr_fold),
                              hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
  return CYC_OK;
}

int copy_out(const cyc_tsqr_plan_s* p, double* R_out, hipStream_t st) {
  const int n = p->G.n;
  hipLaunchKernelGGL(k_tsqr_copy, dim3((unsigned)std::min((n * n + 255) / 256, 4096)), dim3(256),
                     0, st, (const double*)p->ws.ptr, n, p->G.NP, R_out);
  CYC_LAUNCH_CHECK("k_tsqr_copy");
  return CYC_OK;
}

}  // namespace

extern "C" {

int cyc_tsqr_run_rows(void) { return kRunRows; }
int cyc_tsqr_panel_cols(void) { return kPanel; }
int cyc_tsqr_tile_rows(int32_t ncols) {
  return ncols >= 1 && ncols <= kMaxCols ? tile_rows(ncols) : 0;
}

int cyc_tsqr_plan_create(int32_t ncols, int64_t workspaceBytes, cyc_tsqr_plan* plan) {
  CYC_REQUIRE(plan != nullptr, "plan must not be null");
  CYC_REQUIRE(ncols >= 1 && ncols <= kMaxCols,
              "tallSkinnyQR supports 1 to " + std::to_string(kMaxCols) + " columns but got " +
                  std::to_string(ncols));
  const size_t slab = sizeof(double) * slab_doubles(ncols);
  CYC_REQUIRE(workspaceBytes == 0 || (workspaceBytes > 0 && (size_t)workspaceBytes >= 2 * slab),
              "workspaceBytes must be 0 or at least " + std::to_string(2 * slab) +
                  " (the running R and one run) but got " + std::to_string(workspaceBytes));
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    cyc::set_error("no HIP device visible");
    return CYC_ERR_NO_DEVICE;
  }
  auto* p = new cyc_tsqr_plan_s();
  p->G = Geom{ncols, pad16(ncols), tile_rows(ncols), pad16(ncols) + kLdPad, log2_cols(ncols)};
  p->workspaceBytes = (size_t)workspaceBytes;
  *plan = p;
  return CYC_OK;
}

int cyc_tsqr_plan_destroy(cyc_tsqr_plan plan) {
  delete plan;
  return CYC_OK;
}

int cyc_tsqr_factor_dev(cyc_tsqr_plan plan, const double* X, int64_t nrows, double* R_out,
                        void* stream) {
  CYC_REQUIRE(plan != nullptr && R_out != nullptr, "plan and R_out must not be null");
  CYC_REQUIRE(nrows >= 0, "nrows >= 0");
  CYC_REQUIRE(nrows == 0 || X != nullptr, "non-null rows");
  hipStream_t st = cyc::as_stream(stream);
  std::lock_guard<std::mutex> g(plan->mu);
  const Geom G = plan->G;
  const size_t slab = slab_doubles(G.n);
  const int64_t runs = (nrows + kRunRows - 1) / kRunRows;
  const int64_t perLaunch =
      plan->workspaceBytes ? (int64_t)(plan->workspaceBytes / (sizeof(double) * slab)) - 1
                           : std::max<int64_t>(1, std::min<int64_t>(runs, kDefaultRunsPerLaunch));
  if (int rc = plan->ws.reserve(sizeof(double) * slab * (size_t)(perLaunch + 1))) return rc;
  if (int rc = allow_lds(plan)) return rc;
  double* acc = (double*)plan->ws.ptr;
  double* slabs = acc + slab;
  const size_t lds = lds_bytes(G.n);
  for (int64_t run0 = 0; run0 < std::max<int64_t>(runs, 1); run0 += perLaunch) {
    const int64_t nb = std::min(perLaunch, runs - run0);
    if (nb > 0) {
      cyc::KernelTimer timer("k_tsqr_run", st);
      hipLaunchKernelGGL(k_tsqr_run, dim3((unsigned)nb), dim3(kThreads), lds, st, X, nrows, G,
                         run0, slabs);
      CYC_LAUNCH_CHECK("k_tsqr_run");
    }
    cyc::KernelTimer timer("k_tsqr_fold", st);
    hipLaunchKernelGGL(k_tsqr_fold, dim3(1), dim3(kThreads), lds, st, (const double*)slabs,
                       std::max<int64_t>(nb, 0), (int64_t)slab, G.NP, G,
                       (int)(run0 == 0), acc);
    CYC_LAUNCH_CHECK("k_tsqr_fold");
  }
  return copy_out(plan, R_out, st);
}

int cyc_tsqr_fold_dev(cyc_tsqr_plan plan, const double* Rs, int64_t count, double* R_out,
                      void* stream) {
  CYC_REQUIRE(plan != nullptr && R_out != nullptr, "plan and R_out must not be null");
  CYC_REQUIRE(count >= 0, "count >= 0");
  CYC_REQUIRE(count == 0 || Rs != nullptr, "non-null triangles");
  hipStream_t st = cyc::as_stream(stream);
  std::lock_guard<std::mutex> g(plan->mu);
  const Geom G = plan->G;
  if (int rc = plan->ws.reserve(sizeof(double) * slab_doubles(G.n))) return rc;
  if (int rc = allow_lds(plan)) return rc;
  {
    cyc::KernelTimer timer("k_tsqr_fold", st);
    hipLaunchKernelGGL(k_tsqr_fold, dim3(1), dim3(kThreads), lds_bytes(G.n), st, Rs, count,
                       (int64_t)G.n * G.n, G.n, G, 1, (double*)plan->ws.ptr);
    CYC_LAUNCH_CHECK("k_tsqr_fold");
  }
  return copy_out(plan, R_out, st);
}

int cyc_tsqr_finish_dev(cyc_tsqr_plan plan, double* R, void* stream) {
  CYC_REQUIRE(plan != nullptr && R != nullptr, "plan and R must not be null");
  hipLaunchKernelGGL(k_tsqr_finish, dim3((unsigned)plan->G.n), dim3(256), 0,
                     cyc::as_stream(stream), R, plan->G.n);
  CYC_LAUNCH_CHECK("k_tsqr_finish");
  return CYC_OK;
}

}  // extern "C"
