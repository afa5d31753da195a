// syrk_tiles.hpp -- the 128 x 128 split-K fp64 MFMA syrk tile shared by the
// RowMatrix Gramian (gramian.hip: k_gram_tiles, k_gram_dma) and the WLS
// aggregate (wls.hip: k_wls_tiles).  Kernels and helpers here sit in an
// anonymous namespace: every translation unit that includes this file gets
// its own copy.
//
// U (packed upper, column-major: U[j(j+1)/2 + i], i <= j) += sum_r z_r z_r^T
// is a syrk with a huge contraction dimension (rows).  Layout / schedule:
//   - output split in 128 x 128 tiles, only the upper block triangle (a
//     "tile pair" ti <= tj, numbered row by row);
//   - rows split in S contiguous ranges (split-K, split_rows) so that tile
//     pairs x S >> 256 CUs; each workgroup accumulates its tile over its
//     range with v_mfma_f64_16x16x4f64 (4 waves, 64 x 64 per wave = 16
//     accumulators);
//   - chunks of rows of the two 128-column panels go through LDS (row stride
//     144 doubles: the two 16-lane halves of a ds_read_b64 hit disjoint
//     banks).  staged_tiles stages 16-row chunks through registers, the next
//     chunk prefetched while this one multiplies; a row source prepares the
//     values (the mean subtracted, the weight applied) on the way;
//   - partial tiles go to slabs [split][tile pair][i (128)][j (128)];
//     k_gram_fold adds the S slabs in fixed order into U (deterministic, no
//     atomics).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>

#include "common.hpp"

namespace {

constexpr int TILE = 128;
constexpr int KC = 16;             // rows per staged LDS chunk; a split's rows are a multiple
constexpr int LDSW = TILE + 16;    // LDS row stride (doubles)
constexpr int GT = 256;            // threads per workgroup

// tile pair number -> (ti <= tj), pairs numbered along the rows of the upper
// block triangle
__device__ __forceinline__ void tile_pair(int pair, int tilesPerSide, int& ti, int& tj) {
  int t = pair;
  ti = 0;
  while (t >= tilesPerSide - ti) { t -= tilesPerSide - ti; ++ti; }
  tj = ti + t;
}

__device__ __forceinline__ void zero_acc(cyc_double4 (&acc)[4][4]) {
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = cyc_double4{0.0, 0.0, 0.0, 0.0};
}

// The MFMA operands of one k-step (4 rows: this lane's is krow) of wave
// (wy, wx)'s 64 x 64 block, from the chunk's two LDS panels.
__device__ __forceinline__ void fetch_operands(const double* Ai, const double* Aj, int krow, int wy,
                                               int wx, int lane, double (&a)[4], double (&b)[4]) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    a[q] = Ai[krow * LDSW + wy * 64 + q * 16 + (lane & 15)];
    b[q] = Aj[krow * LDSW + wx * 64 + q * 16 + (lane & 15)];
  }
}

__device__ __forceinline__ void mfma_step(const double (&a)[4], const double (&b)[4],
                                          cyc_double4 (&acc)[4][4]) {
#pragma unroll
  for (int qa = 0; qa < 4; ++qa)
#pragma unroll
    for (int qb = 0; qb < 4; ++qb)
      acc[qa][qb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[qa], b[qb], acc[qa][qb], 0, 0, 0);
}

// wave (wy, wx)'s accumulators into the workgroup's 128 x 128 slab tile
__device__ __forceinline__ void store_tile(double* out, int wy, int wx, int lane,
                                           const cyc_double4 (&acc)[4][4]) {
#pragma unroll
  for (int qa = 0; qa < 4; ++qa)
#pragma unroll
    for (int qb = 0; qb < 4; ++qb)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = wy * 64 + qa * 16 + (lane >> 4) + 4 * r;
        const int j = wx * 64 + qb * 16 + (lane & 15);
        out[i * TILE + j] = acc[qa][qb][r];
      }
}

// 8 consecutive doubles of a row whose address is a multiple of 16 bytes:
// 64 contiguous bytes per thread, 4 x 16-byte loads
__device__ __forceinline__ void load8(const double* src, double* dst) {
  const double2* v = reinterpret_cast<const double2*>(src);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    double2 t2 = v[e];
    dst[2 * e] = t2.x;
    dst[2 * e + 1] = t2.y;
  }
}

// The register-staged tile: blockIdx.x -> tile pair, blockIdx.y -> row split
// (rows [y rowsPerSplit, ...)), GT threads.  Staging map: KC rows x 128 cols
// per panel = 2048 doubles, 256 threads x 8: thread -> row sr = tid >> 4,
// cols sc .. sc + 7 (sc = (tid & 15) * 8).  rows.fill(r, ci, cj, ri, rj)
// gives that thread's 8 values of row r in the i-side panel (columns ci ..)
// and the j-side panel (cj ..), or returns false for a row that stages zeros.
template <class Rows>
__device__ __forceinline__ void staged_tiles(const Rows& rows, int64_t nrows, int tilesPerSide,
                                             int64_t rowsPerSplit, double* __restrict__ slab) {
  __shared__ __attribute__((aligned(16))) double Ai[KC * LDSW];
  __shared__ __attribute__((aligned(16))) double Aj[KC * LDSW];
  int ti, tj;
  tile_pair(blockIdx.x, tilesPerSide, ti, tj);
  const int I0 = ti * TILE, J0 = tj * TILE;
  const int64_t r0 = (int64_t)blockIdx.y * rowsPerSplit;
  const int64_t r1 = min<int64_t>(nrows, r0 + rowsPerSplit);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wy = wave >> 1, wx = wave & 1;

  cyc_double4 acc[4][4];
  zero_acc(acc);

  const int sr = tid >> 4, sc = (tid & 15) * 8;
  double ri[8], rj[8];
  auto load = [&](int64_t rb) {
    const int64_t r = rb + sr;
    if (!(r < r1 && rows.fill(r, I0 + sc, J0 + sc, ri, rj))) {
#pragma unroll
      for (int e = 0; e < 8; ++e) ri[e] = rj[e] = 0.0;
    }
  };
  auto store = [&]() {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      Ai[sr * LDSW + sc + e] = ri[e];
      Aj[sr * LDSW + sc + e] = rj[e];
    }
  };

  if (r0 < r1) load(r0);
  for (int64_t rb = r0; rb < r1; rb += KC) {
    __syncthreads();
    store();
    __syncthreads();
    if (rb + KC < r1) load(rb + KC);
#pragma unroll
    for (int kk = 0; kk < KC; kk += 4) {
      double a[4], b[4];
      fetch_operands(Ai, Aj, kk + (lane >> 4), wy, wx, lane, a, b);
      mfma_step(a, b, acc);
    }
  }

  const int pairs = tilesPerSide * (tilesPerSide + 1) / 2;
  store_tile(slab + ((size_t)blockIdx.y * pairs + blockIdx.x) * TILE * TILE, wy, wx, lane, acc);
}

// U[iut(I0+i, J0+j)] += sum over splits (fixed order), upper triangle only.
__global__ void k_gram_fold(const double* __restrict__ slab, int splits, int tilesPerSide, int p,
                            double* __restrict__ U) {
  const int pair = blockIdx.y;
  int ti, tj;
  tile_pair(pair, tilesPerSide, ti, tj);
  const int pairs = tilesPerSide * (tilesPerSide + 1) / 2;
  const int e = blockIdx.x * blockDim.x + threadIdx.x;   // i * 128 + j
  if (e >= TILE * TILE) return;
  const int i = e / TILE, j = e % TILE;
  const int gi = ti * TILE + i, gj = tj * TILE + j;
  if (gi >= p || gj >= p || gi > gj) return;
  double s = 0.0;
  for (int sp = 0; sp < splits; ++sp) s = dadd(s, slab[((size_t)sp * pairs + pair) * TILE * TILE + e]);
  const int64_t idx = (int64_t)gj * (gj + 1) / 2 + gi;
  U[idx] = dadd(U[idx], s);
}

inline int tiles_per_side(int width) { return (width + TILE - 1) / TILE; }
inline int tile_pairs(int tilesPerSide) { return tilesPerSide * (tilesPerSide + 1) / 2; }

struct SplitK {
  int64_t splits, rowsPerSplit;
};

// split-K for a kernel that runs wgPerCu workgroups per CU: at least 4 rounds
// of workgroups and at least 64 rows per split, with the split count whose
// last round is fullest (36 tile pairs x 57 splits = 2052 workgroups ran 5
// rounds, the 5th holding 4; 36 x 71 = 2556 fill 4.99 rounds); a split's rows
// a multiple of KC.
inline SplitK split_rows(int64_t nrows, int pairs, int wgPerCu) {
  const int64_t slots = wgPerCu * (int64_t)cyc::device_cus();
  const int64_t lo = std::max<int64_t>(1, (4 * slots + pairs - 1) / pairs);
  int64_t splits = cyc::balanced_splits(pairs, lo, 2 * lo, slots);
  splits = std::min<int64_t>(splits, std::max<int64_t>(1, nrows / 64));
  const int64_t rps = cyc::round_up((nrows + splits - 1) / splits, KC);
  return {(nrows + rps - 1) / rps, rps};
}

inline size_t slab_bytes(int64_t splits, int pairs) {
  return sizeof(double) * (size_t)splits * pairs * TILE * TILE;
}

// U (order `width`) += the splits' slabs
inline int fold_slabs(const double* slab, int64_t splits, int tilesPerSide, int width, double* U,
                      hipStream_t st) {
  hipLaunchKernelGGL(k_gram_fold, dim3(TILE * TILE / 256, tile_pairs(tilesPerSide)), dim3(256), 0,
                     st, slab, (int)splits, tilesPerSide, width, U);
  CYC_LAUNCH_CHECK("k_gram_fold");
  return CYC_OK;
}

// CSR rows [r0, r0 + rows) scattered into a zeroed dense row-major chunk
// (one wave per row): the sparse rows of a RowMatrix reach the same syrk.
// For a nonzero x_j the sparse spr branch (mllib/linalg/BLAS.scala:269-298)
// adds (alpha x_j) x_i exactly as dspr does, so the densified rows give the
// reference's per-row products.
__global__ __launch_bounds__(256) void k_csr_densify(const int64_t* __restrict__ rowptr,
                                                     const int32_t* __restrict__ colidx,
                                                     const double* __restrict__ vals, int64_t r0,
                                                     int64_t rows, int p,
                                                     double* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  double* o = out + r * p;
  const int64_t a = rowptr[r0 + r], b = rowptr[r0 + r + 1];
  for (int64_t k = a + lane; k < b; k += 64) o[colidx[k]] = vals[k];
}

// CSR rows of width p in chunks of about 1 GiB of dense rows: densify into
// `chunk`, then `dense`.
template <class F>
int over_csr_chunks(cyc::DeviceBuffer& chunk, int p, const int64_t* rowptr,
                    const int32_t* colidx, const double* vals, int64_t nrows, hipStream_t st,
                    F dense) {
  const int64_t R = std::max<int64_t>(256, ((int64_t)1 << 30) / (8 * (int64_t)p)) / 256 * 256;
  const int64_t rows = std::min<int64_t>(R, nrows);
  if (int rc = chunk.reserve(sizeof(double) * (size_t)rows * p)) return rc;
  double* buf = (double*)chunk.ptr;
  for (int64_t r0 = 0; r0 < nrows; r0 += R) {
    const int64_t nr = std::min<int64_t>(R, nrows - r0);
    CYC_HIP(hipMemsetAsync(buf, 0, sizeof(double) * (size_t)nr * p, st));
    hipLaunchKernelGGL(k_csr_densify, dim3((unsigned)((nr + 3) / 4)), dim3(256), 0, st, rowptr,
                       colidx, vals, r0, nr, p, buf);
    CYC_LAUNCH_CHECK("k_csr_densify");
    if (int rc = dense((const double*)buf, nr)) return rc;
  }
  return CYC_OK;
}

}  // namespace
