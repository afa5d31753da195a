// als.hip -- ALS (ml/recommendation/ALS.scala) on gfx950 (MI355X): one
// half-step of computeFactors (NormalEquation.add per rating, CholeskySolver
// .solve per destination id) and the model's predict.  The Scala is cited from
// memory; the arithmetic below is the contract.
//
// One side is the ratings grouped by destination id in CSR form: rowptr (int64,
// m + 1), colidx (int32 source ids), values (float32 ratings); duplicates of a
// (user, item) pair stay separate entries.  Y is the source factors (nsrc x
// rank float32, row-major), X the destination factors (m x rank float32).
//
// Row u, each of its ratings (i, r) in order: da = (double) Y[i]; ata += c da
// da^T (dspr on the packed upper triangle), atb += b da (daxpy), all fp64.
//   explicit       c = 1, b = r, numExplicits = n_u (the row's rating count)
//   implicitPrefs  c1 = alpha |r|, c = c1, b = 1 + c1 if r > 0 else 0 (atb takes
//                  b, not c b), numExplicits = #{r > 0}, and ata starts from
//                  YtY = sum_i da_i da_i^T over ALL source rows
// then ata's diagonal += regParam numExplicits, a Cholesky solve (dppsv) in
// fp64, X[u] = (float) solution.  A row without ratings gets an all-zero factor
// and present[u] = 0.  A non-positive (or NaN) pivot stores a zero factor and
// leaves the lowest such row in *info (-1: none); nothing faults and no NaN is
// written.
//
// Kernels
//   k_als_check       rowptr[0] == 0, rowptr non-decreasing, rowptr[m] == nnz,
//                     0 <= colidx < nsrc, before anything gathers through them.
//   k_als_count_pos   #{r > 0} per row (a wave per row, integer adds).
//   k_als_normal      a workgroup (4 waves) owns one segment: at most kSegment
//                     ratings of one row.  Chunks of kChunk ratings are gathered
//                     into LDS as fp64 rows z = [y | b | 0 ..] of 16 W columns, W
//                     = ceil((rank + 1) / 16) (the next chunk's loads are in
//                     flight while this one multiplies).  Wave w takes ratings
//                     8 w .. 8 w + 7 of the chunk and every upper tile pair (ti <=
//                     tj): v_mfma_f64_16x16x4_f64 with A = y (lane l: row l & 15
//                     of tile ti, rating l >> 4; the b position reads as 0) and B
//                     = [c y | b] (column l & 15 of tile tj), so atb is column
//                     `rank` of the product, as M_j rides k_gmm_mstep's [x, 1].
//                     The four waves' accumulators are added into the LDS system
//                     in wave order.  TEMPLATE ARGUMENT YTY: the same walk over
//                     a split of consecutive rows of Y with c = 1, b = 0.
//                     A row of one segment is solved in the same kernel; a
//                     longer row's segment stores its [ata | atb] in the
//                     workspace.
//   k_als_fold_solve  a long row's partials added in segment order, then the
//                     solve.
//   k_als_fold_yty    YtY = the splits' partials in split order (full
//                     symmetric rank x rank, row-major).
//   k_als_mark        present[u] = n_u > 0; a zero factor where it is not.
//   k_als_predict     out[p] = sdot(rank, U[users[p]], V[items[p]]) in fp32,
//                     products added left to right, unfused; NaN where an id is
//                     negative, past the count or absent.
// The solve (als_solve) works on the LDS copy: upper Cholesky A = U^T U, right-
// looking, with atb carried as one more column (which is the forward solve),
// then the back substitution column by column.  Only entries with row <= col
// are ever read.
// Every sum has one fixed order and there is no floating-point atomic: two
// calls on the same inputs give the same bits.
//
// LDS at rank 64 (T = 4, W = 5): chunk 32 x 80 doubles (20 KB) + the 64 x 80
// system (40 KB) + 160 doubles: under 64 KB.  At that rank the kernel's 256
// VGPRs, not its LDS, keep a CU to one workgroup.
//
// Cost per rating: rank (rank + 1) fp64 flop for the triangle (the padded
// tiles issue 512 flop each: 1 tile at rank 10, 14 at rank 64) against 4 rank
// gathered bytes; per row rank^3 / 3 flop for the solve.  Rank 10 sits on the
// bandwidth side of the roofline, rank 64 on the MFMA side: DESIGN.md 5g, with
// the measured times.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include <algorithm>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "common.hpp"

struct cyc_als_side_s {
  std::mutex mu;
  int64_t m = 0, nnz = 0, nsrc = 0;
  int rank = 0;
  const int64_t* rowptr = nullptr;   // borrowed: the caller keeps them alive
  const int32_t* colidx = nullptr;
  const float* values = nullptr;
  int64_t nseg = 0, nlong = 0, nslots = 0;
  cyc::DeviceBuffer segRow, segOff, segSlot, longRow, longSlot, npos;
  cyc::DeviceBuffer ws, slab, yty, bad;
};

namespace {

constexpr int kSegment = 1024;    // L: ratings of one row per workgroup
constexpr int kChunk = 32;        // ratings per LDS chunk
constexpr int kThreads = 256;
constexpr int kMaxRank = 64;
constexpr int64_t kMaxGrid = (int64_t)1 << 20;
constexpr int64_t kYtyRows = 1024;   // rows of Y per YtY split (at least)
constexpr int64_t kYtySplits = 1024;

inline int tiles16(int x) { return x / 16 + (x % 16 != 0); }
// chunk row stride: rows k, k + 1 on disjoint LDS banks (16 mod 32 doubles)
inline int chunk_ld(int W) { return (W & 1) ? 16 * W : 16 * W + 16; }
inline size_t lds_doubles(int T, int W, bool chunk) {
  return (chunk ? (size_t)kChunk * chunk_ld(W) + kChunk : 0) + (size_t)256 * T * W + 32 * T;
}

__global__ __launch_bounds__(256) void k_als_check(const int64_t* __restrict__ rowptr,
                                                   const int32_t* __restrict__ colidx, int64_t m,
                                                   int64_t nnz, int64_t nsrc,
                                                   unsigned long long* __restrict__ bad) {
  const int64_t n = m + 1 > nnz ? m + 1 : nnz;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    if (i == 0 && rowptr[0] != 0) atomicMin(&bad[0], 0ull);
    if (i < m && rowptr[i] > rowptr[i + 1]) atomicMin(&bad[1], (unsigned long long)i);
    if (i == m && rowptr[m] != nnz) atomicMin(&bad[2], 0ull);
    if (i < nnz && (colidx[i] < 0 || colidx[i] >= nsrc)) atomicMin(&bad[3], (unsigned long long)i);
  }
}

__global__ __launch_bounds__(256) void k_als_count_pos(const int64_t* __restrict__ rowptr,
                                                       const float* __restrict__ values, int64_t m,
                                                       int32_t* __restrict__ npos) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  for (int64_t u = wave; u < m; u += (int64_t)gridDim.x * 4) {
    int cnt = 0;
    for (int64_t e = rowptr[u] + lane; e < rowptr[u + 1]; e += 64) cnt += values[e] > 0.0f;
#pragma unroll
    for (int sh = 1; sh < 64; sh <<= 1) cnt += __shfl_xor(cnt, sh);
    if (lane == 0) npos[u] = cnt;
  }
}

__global__ __launch_bounds__(256) void k_als_mark(const int64_t* __restrict__ rowptr, int64_t m,
                                                  int rank, float* __restrict__ X,
                                                  uint8_t* __restrict__ present) {
  for (int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x; u < m; u += (int64_t)gridDim.x * 256) {
    const bool has = rowptr[u + 1] > rowptr[u];
    present[u] = has ? 1 : 0;
    if (!has)
      for (int f = 0; f < rank; ++f) X[u * rank + f] = 0.0f;
  }
}

// acc += over ratings k in [0, n): z_k z'_k^T, z = y of src(k) (A operand), z'
// = [c y | b] (B operand).  src(k, i, c, b) names the k-th source row and its
// weights.  Zs: kChunk x LD doubles, cs: kChunk doubles.
template <int T, int W, class Src>
__device__ __forceinline__ void als_accumulate(const float* __restrict__ Y, int rank, int64_t n,
                                               Src src, double* Zs, double* cs,
                                               cyc_double4 (&acc)[T][W]) {
  constexpr int RW = 16 * W, LD = (W & 1) ? RW : RW + 16;
  constexpr int PT = kChunk * RW / kThreads;   // 2 W staged values per thread
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, c = lane & 15;
  double v[PT], cv[PT];
  auto load = [&](int64_t k0) {
#pragma unroll
    for (int q = 0; q < PT; ++q) {
      const int e = tid + q * kThreads;
      const int64_t k = k0 + e / RW;
      const int col = e % RW;
      double val = 0.0, cc = 0.0;
      if (k < n) {
        int64_t i;
        double b;
        src(k, i, cc, b);
        if (col < rank) val = (double)Y[i * rank + col];
        else if (col == rank) val = b;
      }
      v[q] = val;
      cv[q] = cc;
    }
  };
  if (n > 0) load(0);
  for (int64_t k0 = 0; k0 < n; k0 += kChunk) {
    __syncthreads();   // the previous chunk is read
#pragma unroll
    for (int q = 0; q < PT; ++q) {
      const int e = tid + q * kThreads;
      Zs[(e / RW) * LD + e % RW] = v[q];
      if (e % RW == 0) cs[e / RW] = cv[q];
    }
    __syncthreads();
    if (k0 + kChunk < n) load(k0 + kChunk);
#pragma unroll
    for (int ks = 0; ks < kChunk / 16; ++ks) {
      const int kr = wave * (kChunk / 4) + ks * 4 + g;
      const double ck = cs[kr];
      double a[T], b[W];
#pragma unroll
      for (int t = 0; t < W; ++t) {
        const double z = Zs[kr * LD + t * 16 + c];
        const bool isb = t * 16 + c == rank;
        if (t < T) a[t < T ? t : 0] = isb ? 0.0 : z;
        b[t] = isb ? z : ck * z;
      }
#pragma unroll
      for (int ti = 0; ti < T; ++ti)
#pragma unroll
        for (int tj = ti; tj < W; ++tj)
          acc[ti][tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ti], b[tj], acc[ti][tj], 0, 0, 0);
    }
  }
}

// S (16 T x 16 W) = the four waves' accumulators in wave order; tiles below
// the diagonal are never written (and never read).
template <int T, int W>
__device__ __forceinline__ void als_reduce(const cyc_double4 (&acc)[T][W], double* S) {
  constexpr int RW = 16 * W;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, c = lane & 15;
  __syncthreads();   // S's previous user is done
  for (int w = 0; w < 4; ++w) {
    if (wave == w) {
#pragma unroll
      for (int ti = 0; ti < T; ++ti)
#pragma unroll
        for (int tj = ti; tj < W; ++tj)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            double* p = S + (ti * 16 + g + 4 * r) * RW + tj * 16 + c;
            *p = w == 0 ? acc[ti][tj][r] : *p + acc[ti][tj][r];
          }
    }
    __syncthreads();
  }
}

// S holds [ata | atb] (row <= col <= rank valid, stride RW).  ata += yty (or
// nothing), diagonal += lambda, Cholesky, both triangular solves; xs[0 ..
// rank) is the solution.  false (for every thread) at a pivot that is not > 0.
__device__ __forceinline__ bool als_solve(double* S, int RW, int rank, double lambda,
                                          const double* __restrict__ yty, double* diag,
                                          double* xs) {
  const int tid = threadIdx.x;
  for (int e = tid; e < rank * rank; e += kThreads) {
    const int i = e / rank, j = e % rank;
    if (i <= j) {
      double v = S[i * RW + j];
      if (yty) v = yty[e] + v;
      if (i == j) v += lambda;
      S[i * RW + j] = v;
    }
  }
  __syncthreads();
  for (int j = 0; j < rank; ++j) {
    const double piv = S[j * RW + j];
    if (!(piv > 0.0)) return false;
    const double d = __builtin_sqrt(piv);
    if (tid == 0) diag[j] = d;
    for (int cidx = j + 1 + tid; cidx <= rank; cidx += kThreads) S[j * RW + cidx] /= d;
    __syncthreads();
    // rows j + 1 .. rank - 1 over the waves, columns r .. rank over the lanes
    for (int r = j + 1 + (tid >> 6); r < rank; r += kThreads / 64) {
      const double f = S[j * RW + r];
      for (int cidx = r + (tid & 63); cidx <= rank; cidx += 64)
        S[r * RW + cidx] -= f * S[j * RW + cidx];
    }
    __syncthreads();
  }
  for (int j = rank - 1; j >= 0; --j) {
    const double x = S[j * RW + rank] / diag[j];
    if (tid == 0) xs[j] = x;
    for (int r = tid; r < j; r += kThreads) S[r * RW + rank] -= S[r * RW + j] * x;
    __syncthreads();
  }
  return true;
}

__device__ __forceinline__ void als_store(bool ok, int64_t row, int rank, const double* xs,
                                          float* __restrict__ X,
                                          unsigned long long* __restrict__ info) {
  const int tid = threadIdx.x;
  if (tid < rank) X[row * rank + tid] = ok ? (float)xs[tid] : 0.0f;
  if (!ok && tid == 0) atomicMin(info, (unsigned long long)row);
}

struct AlsArgs {
  const int64_t* rowptr;
  const int32_t* colidx;
  const float* values;
  const float* Y;
  const int32_t* segRow;
  const int64_t* segOff;
  const int64_t* segSlot;
  const int32_t* npos;
  const double* yty;
  double* ws;
  float* X;
  unsigned long long* info;
  int64_t nseg, nsrc, rowsPerSplit;
  double regParam, alpha;
  int rank, implicitPrefs;
};

// YTY: segment s is the split [s rowsPerSplit, ..) of Y's rows, its partial
// goes to ws slot s.
template <int T, int W, bool YTY>
__global__ __launch_bounds__(kThreads) void k_als_normal(AlsArgs p) {
  extern __shared__ double smem[];
  constexpr int RW = 16 * W, LD = (W & 1) ? RW : RW + 16;
  double* Zs = smem;
  double* cs = Zs + kChunk * LD;
  double* S = cs + kChunk;
  double* diag = S + 256 * T * W;
  double* xs = diag + 16 * T;
  const int tid = threadIdx.x, rank = p.rank;
  for (int64_t s = blockIdx.x; s < p.nseg; s += gridDim.x) {
    cyc_double4 acc[T][W];
#pragma unroll
    for (int ti = 0; ti < T; ++ti)
#pragma unroll
      for (int tj = 0; tj < W; ++tj) acc[ti][tj] = cyc_double4{0.0, 0.0, 0.0, 0.0};
    int64_t row = 0, slot = s;
    if constexpr (YTY) {
      const int64_t r0 = s * p.rowsPerSplit;
      const int64_t n = min(p.rowsPerSplit, p.nsrc - r0);
      als_accumulate<T, W>(p.Y, rank, n,
                           [&](int64_t k, int64_t& i, double& c, double& b) {
                             i = r0 + k;
                             c = 1.0;
                             b = 0.0;
                           },
                           Zs, cs, acc);
    } else {
      row = p.segRow[s];
      slot = p.segSlot[s];
      const int64_t off = p.segOff[s];
      const int64_t n = min<int64_t>(kSegment, p.rowptr[row + 1] - off);
      const int32_t* ci = p.colidx + off;
      const float* rv = p.values + off;
      const bool imp = p.implicitPrefs != 0;
      const double alpha = p.alpha;
      als_accumulate<T, W>(p.Y, rank, n,
                           [&](int64_t k, int64_t& i, double& c, double& b) {
                             i = ci[k];
                             const double r = (double)rv[k];
                             if (imp) {
                               const double c1 = alpha * __builtin_fabs(r);
                               c = c1;
                               b = r > 0.0 ? 1.0 + c1 : 0.0;
                             } else {
                               c = 1.0;
                               b = r;
                             }
                           },
                           Zs, cs, acc);
    }
    als_reduce<T, W>(acc, S);
    if (slot >= 0) {
      double* out = p.ws + slot * (256 * T * W);
      for (int e = tid; e < 16 * T * RW; e += kThreads) {
        const int r = e / RW, cidx = e % RW;
        if (r <= cidx && cidx <= rank) out[e] = S[e];
      }
    } else {
      const int64_t nexp = p.implicitPrefs ? p.npos[row] : p.rowptr[row + 1] - p.rowptr[row];
      const bool ok = als_solve(S, RW, rank, p.regParam * (double)nexp, p.yty, diag, xs);
      als_store(ok, row, rank, xs, p.X, p.info);
    }
  }
}

template <int T, int W>
__global__ __launch_bounds__(kThreads) void k_als_fold_solve(AlsArgs p,
                                                             const int32_t* __restrict__ longRow,
                                                             const int64_t* __restrict__ longSlot,
                                                             int64_t nlong) {
  extern __shared__ double smem[];
  constexpr int RW = 16 * W;
  double* S = smem;
  double* diag = S + 256 * T * W;
  double* xs = diag + 16 * T;
  const int tid = threadIdx.x, rank = p.rank;
  for (int64_t l = blockIdx.x; l < nlong; l += gridDim.x) {
    const int64_t row = longRow[l];
    const int64_t n = p.rowptr[row + 1] - p.rowptr[row];
    const int64_t cnt = (n + kSegment - 1) / kSegment;
    const double* src = p.ws + longSlot[l] * (256 * T * W);
    __syncthreads();   // the previous row's solution is stored
    for (int e = tid; e < 16 * T * RW; e += kThreads) {
      const int r = e / RW, cidx = e % RW;
      if (r <= cidx && cidx <= rank) {
        double s = 0.0;
        for (int64_t q = 0; q < cnt; ++q) s += src[q * (256 * T * W) + e];
        S[e] = s;
      }
    }
    __syncthreads();
    const int64_t nexp = p.implicitPrefs ? p.npos[row] : n;
    const bool ok = als_solve(S, RW, rank, p.regParam * (double)nexp, p.yty, diag, xs);
    als_store(ok, row, rank, xs, p.X, p.info);
  }
}

// yty[i rank + j] = yty[j rank + i] = the splits' entries (i, j), i <= j, in
// split order.
__global__ __launch_bounds__(256) void k_als_fold_yty(const double* __restrict__ slab,
                                                      int64_t splits, int64_t stride, int RW,
                                                      int rank, double* __restrict__ yty) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= rank * rank) return;
  const int i = e / rank, j = e % rank;
  if (i > j) return;
  double s = 0.0;
  for (int64_t q = 0; q < splits; ++q) s += slab[q * stride + i * RW + j];
  yty[i * rank + j] = s;
  yty[j * rank + i] = s;
}

__global__ __launch_bounds__(256) void k_als_predict(
    const float* __restrict__ U, const uint8_t* __restrict__ up, int64_t nu,
    const float* __restrict__ V, const uint8_t* __restrict__ vp, int64_t nv, int rank,
    const int32_t* __restrict__ users, const int32_t* __restrict__ items, int64_t n,
    float* __restrict__ out) {
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < n; q += (int64_t)gridDim.x * 256) {
    const int64_t u = users[q], i = items[q];
    float s = __builtin_nanf("");
    if (u >= 0 && u < nu && i >= 0 && i < nv && (!up || up[u]) && (!vp || vp[i])) {
      const float* a = U + u * rank;
      const float* b = V + i * rank;
      s = 0.0f;
      for (int f = 0; f < rank; ++f) s = s + a[f] * b[f];
    }
    out[q] = s;
  }
}

inline unsigned grid_for(int64_t items, int per) {
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>((items + per - 1) / per, kMaxGrid));
}

// the (T, W) instantiation of rank: T = ceil(rank / 16), W = ceil((rank + 1) / 16)
#define ALS_DISPATCH(rank, CALL)                          \
  do {                                                    \
    const int _T = tiles16(rank), _W = tiles16(rank + 1); \
    if (_T == 1 && _W == 1) { CALL(1, 1); }               \
    else if (_T == 1) { CALL(1, 2); }                     \
    else if (_T == 2 && _W == 2) { CALL(2, 2); }          \
    else if (_T == 2) { CALL(2, 3); }                     \
    else if (_T == 3 && _W == 3) { CALL(3, 3); }          \
    else if (_T == 3) { CALL(3, 4); }                     \
    else if (_T == 4 && _W == 4) { CALL(4, 4); }          \
    else { CALL(4, 5); }                                  \
  } while (0)

int yty(cyc_als_side_s* s, const float* Y, double* out, hipStream_t st) {
  const int rank = s->rank, T = tiles16(rank), W = tiles16(rank + 1);
  // a fixed function of nsrc alone: the same bits on every device
  int64_t splits = std::max<int64_t>(1, std::min(kYtySplits, (s->nsrc + kYtyRows - 1) / kYtyRows));
  const int64_t rps = cyc::round_up((s->nsrc + splits - 1) / splits, kChunk);
  splits = (s->nsrc + rps - 1) / rps;
  const int64_t stride = (int64_t)256 * T * W;
  if (int rc = s->slab.reserve(sizeof(double) * (size_t)(splits * stride))) return rc;
  AlsArgs a{};
  a.Y = Y;
  a.ws = (double*)s->slab.ptr;
  a.nseg = splits;
  a.nsrc = s->nsrc;
  a.rowsPerSplit = rps;
  a.rank = rank;
  const size_t lds = sizeof(double) * lds_doubles(T, W, true);
  {
    cyc::KernelTimer timer("k_als_yty", st);
#define ALS_YTY(TT, WW)                                                                        \
  hipLaunchKernelGGL((k_als_normal<TT, WW, true>), dim3((unsigned)splits), dim3(kThreads), lds, \
                     st, a)
    ALS_DISPATCH(rank, ALS_YTY);
#undef ALS_YTY
    CYC_LAUNCH_CHECK("k_als_yty");
  }
  hipLaunchKernelGGL(k_als_fold_yty, dim3((rank * rank + 255) / 256), dim3(256), 0, st,
                     (const double*)s->slab.ptr, splits, stride, 16 * W, rank, out);
  CYC_LAUNCH_CHECK("k_als_fold_yty");
  return CYC_OK;
}

}  // namespace

extern "C" {

int cyc_als_segment(void) { return kSegment; }

int cyc_als_side_create(const int64_t* rowptr, const int32_t* colidx, const float* values,
                        int64_t m, int64_t nnz, int64_t nsrc, int32_t rank, void* stream,
                        cyc_als_side* side) {
  CYC_REQUIRE(side != nullptr, "side must not be null");
  CYC_REQUIRE(rank >= 1 && rank <= kMaxRank,
              "ALS supports rank 1 to " + std::to_string(kMaxRank) + " but got " +
                  std::to_string(rank));
  CYC_REQUIRE(m >= 1, "the number of destination ids must be positive but got " +
                          std::to_string(m));
  CYC_REQUIRE(nsrc >= 1, "the number of source ids must be positive but got " +
                             std::to_string(nsrc));
  CYC_REQUIRE(m <= 0x7fffffff && nsrc <= 0x7fffffff, "ids are int32");
  CYC_REQUIRE(nnz >= 0, "nnz >= 0");
  CYC_REQUIRE(rowptr != nullptr, "rowptr must not be null");
  CYC_REQUIRE(nnz == 0 || (colidx != nullptr && values != nullptr),
              "colidx and values must not be null");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    cyc::set_error("no HIP device visible");
    return CYC_ERR_NO_DEVICE;
  }
  hipStream_t st = cyc::as_stream(stream);
  std::unique_ptr<cyc_als_side_s> s(new cyc_als_side_s());
  s->m = m;
  s->nnz = nnz;
  s->nsrc = nsrc;
  s->rank = rank;
  s->rowptr = rowptr;
  s->colidx = colidx;
  s->values = values;

  // the structure, on the device, before anything gathers through it
  unsigned long long bad[4];
  std::fill(bad, bad + 4, ~0ull);
  if (int rc = s->bad.reserve(sizeof(bad))) return rc;
  CYC_HIP(hipMemcpyAsync(s->bad.ptr, bad, sizeof(bad), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_als_check, dim3(grid_for(std::max(m + 1, nnz), 256)), dim3(256), 0, st,
                     rowptr, colidx, m, nnz, nsrc, (unsigned long long*)s->bad.ptr);
  CYC_LAUNCH_CHECK("k_als_check");
  CYC_HIP(hipMemcpyAsync(bad, s->bad.ptr, sizeof(bad), hipMemcpyDeviceToHost, st));
  CYC_HIP(hipStreamSynchronize(st));
  CYC_REQUIRE(bad[0] == ~0ull, "rowptr must start at 0");
  CYC_REQUIRE(bad[1] == ~0ull,
              "rowptr must be non-decreasing but decreases after row " + std::to_string(bad[1]));
  CYC_REQUIRE(bad[2] == ~0ull, "rowptr must end at nnz = " + std::to_string(nnz));
  CYC_REQUIRE(bad[3] == ~0ull, "source ids must be in [0, " + std::to_string(nsrc) +
                                   ") but entry " + std::to_string(bad[3]) + " is not");

  // the segment table, once: the ratings do not change during a fit
  std::vector<int64_t> rp((size_t)m + 1);
  CYC_HIP(hipMemcpyAsync(rp.data(), rowptr, sizeof(int64_t) * (m + 1), hipMemcpyDeviceToHost, st));
  CYC_HIP(hipStreamSynchronize(st));
  std::vector<int32_t> segRow, longRow;
  std::vector<int64_t> segOff, segSlot, longSlot;
  int64_t slots = 0;
  for (int64_t u = 0; u < m; ++u) {
    const int64_t n = rp[u + 1] - rp[u];
    const int64_t cnt = (n + kSegment - 1) / kSegment;
    if (cnt > 1) {
      longRow.push_back((int32_t)u);
      longSlot.push_back(slots);
    }
    for (int64_t q = 0; q < cnt; ++q) {
      segRow.push_back((int32_t)u);
      segOff.push_back(rp[u] + q * kSegment);
      segSlot.push_back(cnt > 1 ? slots++ : -1);
    }
  }
  s->nseg = (int64_t)segRow.size();
  s->nlong = (int64_t)longRow.size();
  s->nslots = slots;
  auto upload = [&](cyc::DeviceBuffer& b, const void* src, size_t bytes) -> int {
    if (int rc = b.reserve(bytes)) return rc;
    if (bytes) CYC_HIP(hipMemcpyAsync(b.ptr, src, bytes, hipMemcpyHostToDevice, st));
    return CYC_OK;
  };
  if (int rc = upload(s->segRow, segRow.data(), sizeof(int32_t) * segRow.size())) return rc;
  if (int rc = upload(s->segOff, segOff.data(), sizeof(int64_t) * segOff.size())) return rc;
  if (int rc = upload(s->segSlot, segSlot.data(), sizeof(int64_t) * segSlot.size())) return rc;
  if (int rc = upload(s->longRow, longRow.data(), sizeof(int32_t) * longRow.size())) return rc;
  if (int rc = upload(s->longSlot, longSlot.data(), sizeof(int64_t) * longSlot.size())) return rc;
  if (int rc = s->npos.reserve(sizeof(int32_t) * (size_t)m)) return rc;
  hipLaunchKernelGGL(k_als_count_pos, dim3(grid_for(m, 4)), dim3(256), 0, st, rowptr, values, m,
                     (int32_t*)s->npos.ptr);
  CYC_LAUNCH_CHECK("k_als_count_pos");
  CYC_HIP(hipStreamSynchronize(st));   // the host tables are consumed
  *side = s.release();
  return CYC_OK;
}

int cyc_als_side_destroy(cyc_als_side side) {
  delete side;
  return CYC_OK;
}

int cyc_als_yty_dev(cyc_als_side side, const float* Y, double* yty_out, void* stream) {
  CYC_REQUIRE(side != nullptr, "side must not be null");
  CYC_REQUIRE(Y != nullptr && yty_out != nullptr, "Y and yty must not be null");
  std::lock_guard<std::mutex> g(side->mu);
  return yty(side, Y, yty_out, cyc::as_stream(stream));
}

int cyc_als_solve_dev(cyc_als_side side, const float* Y, double regParam, int32_t implicitPrefs,
                      double alpha, const double* yty_in, float* X, uint8_t* present,
                      int64_t* info, void* stream) {
  CYC_REQUIRE(side != nullptr, "side must not be null");
  CYC_REQUIRE(Y != nullptr && X != nullptr && present != nullptr && info != nullptr,
              "Y, X, present and info must not be null");
  CYC_REQUIRE(regParam >= 0.0, "regParam must be >= 0 but got " + cyc::java_double(regParam));
  CYC_REQUIRE(!implicitPrefs || alpha >= 0.0,
              "alpha must be >= 0 but got " + cyc::java_double(alpha));
  cyc_als_side_s* s = side;
  hipStream_t st = cyc::as_stream(stream);
  std::lock_guard<std::mutex> g(s->mu);
  const int rank = s->rank, T = tiles16(rank), W = tiles16(rank + 1);
  if (implicitPrefs && !yty_in) {
    if (int rc = s->yty.reserve(sizeof(double) * (size_t)rank * rank)) return rc;
    if (int rc = yty(s, Y, (double*)s->yty.ptr, st)) return rc;
    yty_in = (const double*)s->yty.ptr;
  }
  if (int rc = s->ws.reserve(sizeof(double) * (size_t)s->nslots * 256 * T * W)) return rc;
  CYC_HIP(hipMemsetAsync(info, 0xff, sizeof(int64_t), st));
  hipLaunchKernelGGL(k_als_mark, dim3(grid_for(s->m, 256)), dim3(256), 0, st, s->rowptr, s->m,
                     rank, X, present);
  CYC_LAUNCH_CHECK("k_als_mark");
  if (s->nseg == 0) return CYC_OK;
  AlsArgs a{};
  a.rowptr = s->rowptr;
  a.colidx = s->colidx;
  a.values = s->values;
  a.Y = Y;
  a.segRow = (const int32_t*)s->segRow.ptr;
  a.segOff = (const int64_t*)s->segOff.ptr;
  a.segSlot = (const int64_t*)s->segSlot.ptr;
  a.npos = (const int32_t*)s->npos.ptr;
  a.yty = implicitPrefs ? yty_in : nullptr;
  a.ws = (double*)s->ws.ptr;
  a.X = X;
  a.info = (unsigned long long*)info;
  a.nseg = s->nseg;
  a.nsrc = s->nsrc;
  a.regParam = regParam;
  a.alpha = alpha;
  a.rank = rank;
  a.implicitPrefs = implicitPrefs ? 1 : 0;
  {
    cyc::KernelTimer timer("k_als_normal", st);
    const size_t lds = sizeof(double) * lds_doubles(T, W, true);
#define ALS_NORMAL(TT, WW)                                                                   \
  hipLaunchKernelGGL((k_als_normal<TT, WW, false>), dim3(grid_for(s->nseg, 1)), dim3(kThreads), \
                     lds, st, a)
    ALS_DISPATCH(rank, ALS_NORMAL);
#undef ALS_NORMAL
    CYC_LAUNCH_CHECK("k_als_normal");
  }
  if (s->nlong > 0) {
    cyc::KernelTimer timer("k_als_fold_solve", st);
    const size_t lds = sizeof(double) * lds_doubles(T, W, false);
#define ALS_FOLD(TT, WW)                                                                        \
  hipLaunchKernelGGL((k_als_fold_solve<TT, WW>), dim3(grid_for(s->nlong, 1)), dim3(kThreads), lds, \
                     st, a, (const int32_t*)s->longRow.ptr, (const int64_t*)s->longSlot.ptr,    \
                     s->nlong)
    ALS_DISPATCH(rank, ALS_FOLD);
#undef ALS_FOLD
    CYC_LAUNCH_CHECK("k_als_fold_solve");
  }
  return CYC_OK;
}

int cyc_als_predict_dev(const float* U, const uint8_t* userPresent, int64_t numUsers,
                        const float* V, const uint8_t* itemPresent, int64_t numItems, int32_t rank,
                        const int32_t* users, const int32_t* items, int64_t n, float* out,
                        void* stream) {
  CYC_REQUIRE(rank >= 1, "rank must be positive but got " + std::to_string(rank));
  CYC_REQUIRE(numUsers >= 0 && numItems >= 0 && n >= 0, "counts must not be negative");
  if (n == 0) return CYC_OK;
  CYC_REQUIRE(users != nullptr && items != nullptr && out != nullptr,
              "users, items and out must not be null");
  CYC_REQUIRE((U != nullptr || numUsers == 0) && (V != nullptr || numItems == 0),
              "factors must not be null");
  hipStream_t st = cyc::as_stream(stream);
  hipLaunchKernelGGL(k_als_predict, dim3(grid_for(n, 256)), dim3(256), 0, st, U, userPresent,
                     numUsers, V, itemPresent, numItems, rank, users, items, n, out);
  CYC_LAUNCH_CHECK("k_als_predict");
  return CYC_OK;
}

}  // extern "C"
