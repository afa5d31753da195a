// kmeans_sums.hip -- the per-cluster sums of a dense KMeans Lloyd call on
// gfx950 (MI355X): KMeans.scala:296-311's updateClusterSum / clusterWeightSum
// / costAccum over the rows of a call, and the center update after it.
//
//   k_hist / k_scan_* / k_scatter   stable counting sort of rows by cluster.
//   k_chunk_sums* / k_reduce_clusters / k_cost_total   per-cluster sum of
//       w*x, w, w*cost in a fixed order (deterministic run to run): partial
//       sums of 256-row chunks, folded per cluster in chunk order.
//   k_inc_*   the incremental sums of a fit with carried bounds: the state of
//       the last call updated by the rows that changed cluster, with a device
//       side check that falls back to the full pass above (the gate).
//   k_*_gated   the full pass behind the incremental sums' gate as four
//       launches (nine ungated): the small single-workgroup stages run in the
//       last workgroup to finish the stage before them (last_arrival).
//   k_update_centers   centroid = (1/w)*sum, new norm, convergence flag.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "common.hpp"
#include "kmeans_cos.hpp"
#include "kmeans_sums.hpp"

namespace {

constexpr int kSortTile = 4096;           // rows per counting-sort tile
using cyc::kmsums::kChunkRows;

// ------------------------------------------------------- counting sort
__global__ void k_hist(const int32_t* __restrict__ assign, int64_t n, int k,
                       int32_t* __restrict__ hist, const int* __restrict__ gate) {
  if (gate && !*gate) return;
  extern __shared__ int32_t cnt[];
  for (int c = threadIdx.x; c < k; c += blockDim.x) cnt[c] = 0;
  __syncthreads();
  const int64_t r0 = (int64_t)blockIdx.x * kSortTile;
  const int64_t r1 = min<int64_t>(n, r0 + kSortTile);
  for (int64_t r = r0 + threadIdx.x; r < r1; r += blockDim.x) atomicAdd(&cnt[assign[r]], 1);
  __syncthreads();
  for (int c = threadIdx.x; c < k; c += blockDim.x) hist[(int64_t)blockIdx.x * k + c] = cnt[c];
}

// Per cluster: exclusive running offset over the tiles (in place) and the
// total, as a segmented scan (integer sums: any grouping gives the same
// offsets).  1. per (tile segment, cluster) sums; 2. per cluster, the
// segments' exclusive offsets and the total; 3. the offsets inside segments.
constexpr int kScanSegs = 64;

__global__ void k_scan_seg(const int32_t* __restrict__ hist, int tiles, int k, int segT,
                           int32_t* __restrict__ segsum, const int* __restrict__ gate) {
  if (gate && !*gate) return;
  const int c = blockIdx.x * 64 + threadIdx.x, s = blockIdx.y;
  if (c >= k) return;
  const int t0 = s * segT, t1 = min(tiles, t0 + segT);
  int sum = 0;
#pragma unroll 8
  for (int t = t0; t < t1; ++t) sum += hist[(int64_t)t * k + c];
  segsum[(int64_t)s * k + c] = sum;
}

__global__ void k_scan_segoff(int32_t* __restrict__ segsum, int segs, int k,
                              int64_t* __restrict__ total, const int* __restrict__ gate) {
  if (gate && !*gate) return;
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= k) return;
  int64_t run = 0;
  for (int s = 0; s < segs; ++s) {
    const int32_t h = segsum[(int64_t)s * k + c];
    segsum[(int64_t)s * k + c] = (int32_t)run;
    run += h;
  }
  total[c] = run;
}

__global__ void k_scan_apply(int32_t* __restrict__ hist, int tiles, int k, int segT,
                             const int32_t* __restrict__ segoff, const int* __restrict__ gate) {
  if (gate && !*gate) return;
  const int c = blockIdx.x * 64 + threadIdx.x, s = blockIdx.y;
  if (c >= k) return;
  const int t0 = s * segT, t1 = min(tiles, t0 + segT);
  int32_t run = segoff[(int64_t)s * k + c];
  for (int t = t0; t < t1; ++t) {
    const int32_t h = hist[(int64_t)t * k + c];
    hist[(int64_t)t * k + c] = run;
    run += h;
  }
}

// Single block: cluster start offsets and chunk start offsets (exclusive scans).
__global__ void k_scan_clusters(const int64_t* __restrict__ total, int k,
                                int64_t* __restrict__ cstart, int64_t* __restrict__ chunkStart,
                                const int* __restrict__ gate) {
  if (gate && !*gate) return;
  __shared__ int64_t s_rows[1024], s_chunks[1024];
  const int tid = threadIdx.x;
  const int per = (k + 1023) / 1024;
  int64_t rows = 0, chunks = 0;
  for (int q = 0; q < per; ++q) {
    int c = tid * per + q;
    if (c < k) {
      rows += total[c];
      chunks += (total[c] + kChunkRows - 1) / kChunkRows;
    }
  }
  s_rows[tid] = rows;
  s_chunks[tid] = chunks;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {
    int64_t a = tid >= off ? s_rows[tid - off] : 0, b = tid >= off ? s_chunks[tid - off] : 0;
    __syncthreads();
    s_rows[tid] += a;
    s_chunks[tid] += b;
    __syncthreads();
  }
  int64_t rbase = tid ? s_rows[tid - 1] : 0, cbase = tid ? s_chunks[tid - 1] : 0;
  for (int q = 0; q < per; ++q) {
    int c = tid * per + q;
    if (c < k) {
      cstart[c] = rbase;
      chunkStart[c] = cbase;
      rbase += total[c];
      cbase += (total[c] + kChunkRows - 1) / kChunkRows;
    }
  }
  if (tid == 1023) {
    cstart[k] = s_rows[1023];
    chunkStart[k] = s_chunks[1023];
  }
}

// One wave per tile, rows in order: perm[cstart[c] + tileOffset[c] + rank] = row.
// Tiles by XCD: block b runs on XCD b % 8 and takes tile (b % 8) * per +
// b / 8, so each XCD walks a contiguous range of tiles.  A cluster's rows
// from consecutive tiles land side by side in perm; with consecutive tiles
// on one XCD their 4-byte writes meet in that XCD's L2 instead of partial
// lines from eight L2s (the grid is 8 * per blocks; the spare ones leave).
// segOff (the gated form, else null): tileOff holds the offsets inside
// segments of segT tiles and segOff the segments' own (k_hist_scan_gated).
__device__ __forceinline__ void scatter_tile(const int32_t* __restrict__ assign, int64_t n, int k,
                                             const int32_t* __restrict__ tileOff,
                                             const int64_t* __restrict__ cstart,
                                             int32_t* __restrict__ perm, int64_t tiles,
                                             const int32_t* __restrict__ segOff, int segT) {
  extern __shared__ int64_t pos[];
  const int64_t per = ((int64_t)gridDim.x + 7) / 8;
  const int64_t tile = (int64_t)(blockIdx.x & 7) * per + (blockIdx.x >> 3);
  if (tile >= tiles) return;
  const int lane = threadIdx.x;
  const int kb = 32 - __builtin_clz((unsigned)max(k - 1, 1));   // bits of a cluster index
  if (segOff) {
    const int64_t seg = tile / segT;
    for (int c = lane; c < k; c += 64)
      pos[c] = cstart[c] + segOff[seg * k + c] + tileOff[tile * k + c];
  } else {
    for (int c = lane; c < k; c += 64) pos[c] = cstart[c] + tileOff[tile * k + c];
  }
  __syncthreads();
  const int64_t r0 = tile * kSortTile;
  const int64_t r1 = min<int64_t>(n, r0 + kSortTile);
  // the tile's assignments loaded up front (one latency, not one per 64
  // rows: 124 -> ~30 us at 10M rows), then the stable in-order walk
  constexpr int PER = kSortTile / 64;
  int cv[PER];
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int64_t r = r0 + i * 64 + lane;
    cv[i] = (r < r1) ? assign[r] : -1;
  }
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int64_t r = r0 + i * 64 + lane;
    const int c = cv[i];
    // the lanes holding the same cluster: one ballot per bit of the index
    unsigned long long m = __ballot(c >= 0);
    for (int b = 0; b < kb; ++b) {
      const bool bit = (c >> b) & 1;
      const unsigned long long bal = __ballot(bit);
      m &= bit ? bal : ~bal;
    }
    const int prior = __popcll(m & ((1ull << lane) - 1));
    const int last = 63 - __clzll(m);
    int64_t p = (c >= 0) ? pos[c] + prior : 0;
    __builtin_amdgcn_wave_barrier();
    if (c >= 0) {
      perm[p] = (int32_t)r;
      if (last == lane) pos[c] = p + 1;
    }
    __builtin_amdgcn_wave_barrier();
  }
}

__global__ void k_scatter(const int32_t* __restrict__ assign, int64_t n, int k,
                          const int32_t* __restrict__ tileOff, const int64_t* __restrict__ cstart,
                          int32_t* __restrict__ perm, int64_t tiles, const int* __restrict__ gate) {
  if (gate && !*gate) return;
  scatter_tile(assign, n, k, tileOff, cstart, perm, tiles, nullptr, 0);
}

// Partial sums of up to kChunkRows rows of one cluster, rows in index order
// (updateClusterSum, DistanceMeasure.scala:189-191: axpy(w, x, sum)), their
// weights, and each row's cost = fastSquaredDistance(center, row) = the
// sequential Vectors.sqdist (Vectors.scala:580-587) that findClosest returns
// for the chosen center, summed as w * cost (KMeans.scala:302) in row order.
// The cost is fused here because the rows are read anyway: thread j holds
// dims j, j+256, ... (NJ of them) and writes (c_j - x_j)^2 of G rows to LDS;
// G threads then run the G sequential sums.  costOut (may be NULL) receives
// the per-row costs.
template <int NJ>
__global__ __launch_bounds__(256) void k_chunk_sums(
    const double* __restrict__ X, int d, const double* __restrict__ w,
    const double* __restrict__ C, const int32_t* __restrict__ perm,
    const int64_t* __restrict__ cstart, const int64_t* __restrict__ chunkStart, int k,
    double* __restrict__ part, double* __restrict__ pw, double* __restrict__ pc,
    double* __restrict__ costOut) {
  constexpr int G = 16;
  __shared__ double sq[G * (NJ * 256 + 1)];
  __shared__ double rcost[G];
  const int64_t ch = blockIdx.x;
  if (ch >= chunkStart[k]) return;
  int lo = 0, hi = k;   // cluster = last c with chunkStart[c] <= ch
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (chunkStart[mid] <= ch) lo = mid; else hi = mid;
  }
  const int c = lo;
  const int64_t first = cstart[c] + (ch - chunkStart[c]) * kChunkRows;
  const int64_t last = min<int64_t>(cstart[c + 1], first + kChunkRows);
  const int tid = threadIdx.x;
  constexpr int SQS = NJ * 256 + 1;
  double s[NJ], cj[NJ];
#pragma unroll
  for (int q = 0; q < NJ; ++q) {
    const int j = tid + 256 * q;
    s[q] = 0.0;
    cj[q] = j < d ? C[(int64_t)c * d + j] : 0.0;
  }
  double sw = 0.0, sc = 0.0;
  for (int64_t g0 = first; g0 < last; g0 += G) {
    const int gn = (int)min<int64_t>(G, last - g0);
    for (int pp = 0; pp < gn; ++pp) {
      const int64_t r = perm[g0 + pp];
      const double wr = w ? w[r] : 1.0;
#pragma unroll
      for (int q = 0; q < NJ; ++q) {
        const int j = tid + 256 * q;
        if (j < d) {
          const double x = X[r * d + j];
          s[q] = w ? dadd(s[q], dmul(wr, x)) : dadd(s[q], x);
          const double df = dsub(cj[q], x);
          sq[pp * SQS + j] = dmul(df, df);
        }
      }
    }
    __syncthreads();
    if (tid < gn) {
      double t = 0.0;
      for (int j = 0; j < d; ++j) t = dadd(t, sq[tid * SQS + j]);
      rcost[tid] = t;
      if (costOut) costOut[perm[g0 + tid]] = t;
    }
    __syncthreads();
    if (tid == 0) {
      for (int pp = 0; pp < gn; ++pp) {
        const double wt = w ? w[perm[g0 + pp]] : 1.0;
        sw = dadd(sw, wt);
        sc = dadd(sc, dmul(rcost[pp], wt));
      }
    }
  }
#pragma unroll
  for (int q = 0; q < NJ; ++q) {
    const int j = tid + 256 * q;
    if (j < d) part[ch * d + j] = s[q];
  }
  if (tid == 0) {
    pw[ch] = sw;
    pc[ch] = sc;
  }
}

// The Lloyd path when no per-row costs are requested: thread j accumulates
// both sum_r w x_rj and sum_r w (c_j - x_rj)^2 over the chunk's rows, and the
// chunk's cost is one fixed-order block reduction of the latter.  The cost
// total then differs from summing the rows' sequential sqdist values only
// in rounding order (all terms positive, ~1e-16 relative; the bar is 1e-10),
// and the pass is a plain HBM stream: 8 rows' loads in flight per thread.
// One chunk ch < chunkStart[k]; rowsS / red / reda: the workgroup's LDS.
template <int NJ>
__device__ __forceinline__ void chunk_sums_fast_one(
    const double* __restrict__ X, int d, const double* __restrict__ w,
    const double* __restrict__ C, const int32_t* __restrict__ perm,
    const int64_t* __restrict__ cstart, const int64_t* __restrict__ chunkStart, int k,
    double* __restrict__ part, double* __restrict__ pw, double* __restrict__ pc,
    const double* __restrict__ xnorm, double* __restrict__ pa, const int64_t ch, int32_t* rowsS,
    double* red, double* reda) {
  int lo = 0, hi = k;
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
  double s[NJ], q[NJ], cj[NJ];
#pragma unroll
  for (int u = 0; u < NJ; ++u) {
    const int j = tid + 256 * u;
    s[u] = q[u] = 0.0;
    cj[u] = j < d ? C[(int64_t)c * d + j] : 0.0;
  }
  for (int p0 = 0; p0 < cnt; p0 += 8) {
    double xv[8][NJ];
#pragma unroll
    for (int v = 0; v < 8; ++v) {
      const int64_t r = rowsS[min(p0 + v, cnt - 1)];
#pragma unroll
      for (int u = 0; u < NJ; ++u) {
        const int j = tid + 256 * u;
        // nontemporal: the rows are read once per iteration
        xv[v][u] = j < d ? __builtin_nontemporal_load(&X[r * d + j]) : 0.0;
      }
    }
#pragma unroll
    for (int v = 0; v < 8; ++v) {
      if (p0 + v < cnt) {
        const double wr = w ? w[rowsS[p0 + v]] : 1.0;
#pragma unroll
        for (int u = 0; u < NJ; ++u) {
          const double x = xv[v][u];
          const double df = dsub(cj[u], x);
          if (w) {
            s[u] = dadd(s[u], dmul(wr, x));
            q[u] = dadd(q[u], dmul(wr, dmul(df, df)));
          } else {
            s[u] = dadd(s[u], x);
            q[u] = dadd(q[u], dmul(df, df));
          }
        }
      }
    }
  }
  double qt = 0.0;
#pragma unroll
  for (int u = 0; u < NJ; ++u) {
    const int j = tid + 256 * u;
    if (j < d) part[ch * d + j] = s[u];
    qt = dadd(qt, q[u]);
  }
  red[tid] = qt;
  // pa (incremental sums' error scale): the chunk's sum of w |x| (wave-order
  // norms are enough, it only sizes a bound)
  if (pa) reda[tid] = tid < cnt ? (w ? dmul(w[rowsS[tid]], xnorm[rowsS[tid]]) : xnorm[rowsS[tid]])
                                : 0.0;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (tid < off) {
      red[tid] = dadd(red[tid], red[tid + off]);
      if (pa) reda[tid] = dadd(reda[tid], reda[tid + off]);
    }
    __syncthreads();
  }
  if (tid == 0) {
    double sw = 0.0;
    if (w) {
      for (int i = 0; i < cnt; ++i) sw = dadd(sw, w[rowsS[i]]);
    } else {
      sw = (double)cnt;
    }
    pw[ch] = sw;
    pc[ch] = red[0];
    if (pa) pa[ch] = reda[0];
  }
}

template <int NJ>
__global__ __launch_bounds__(256) void k_chunk_sums_fast(
    const double* __restrict__ X, int d, const double* __restrict__ w,
    const double* __restrict__ C, const int32_t* __restrict__ perm,
    const int64_t* __restrict__ cstart, const int64_t* __restrict__ chunkStart, int k,
    double* __restrict__ part, double* __restrict__ pw, double* __restrict__ pc,
    const double* __restrict__ xnorm, double* __restrict__ pa, const int* __restrict__ gate) {
  __shared__ int32_t rowsS[kChunkRows];
  __shared__ double red[256], reda[256];
  if (gate && !*gate) return;
  const int64_t ch = blockIdx.x;
  if (ch >= chunkStart[k]) return;
  chunk_sums_fast_one<NJ>(X, d, w, C, perm, cstart, chunkStart, k, part, pw, pc, xnorm, pa, ch,
                          rowsS, red, reda);
}

// The gated form: a grid bounded by the device strides over the chunks, so a
// closed gate costs the same at every n.  Each chunk writes its own part /
// pw / pc / pa slot as above, whichever workgroup computes it.
template <int NJ>
__global__ __launch_bounds__(256) void k_chunk_sums_fast_gated(
    const double* __restrict__ X, int d, const double* __restrict__ C,
    const int32_t* __restrict__ perm, const int64_t* __restrict__ cstart,
    const int64_t* __restrict__ chunkStart, int k, double* __restrict__ part,
    double* __restrict__ pw, double* __restrict__ pc, const double* __restrict__ xnorm,
    double* __restrict__ pa, const int* __restrict__ gate) {
  __shared__ int32_t rowsS[kChunkRows];
  __shared__ double red[256], reda[256];
  if (!*gate) return;
  const int64_t chunks = chunkStart[k];
  for (int64_t ch = blockIdx.x; ch < chunks; ch += gridDim.x) {
    chunk_sums_fast_one<NJ>(X, d, nullptr, C, perm, cstart, chunkStart, k, part, pw, pc, xnorm, pa,
                            ch, rowsS, red, reda);
    __syncthreads();   // thread 0 has read red / reda / rowsS
  }
}

// Same without the fused cost (d > 1024): costs come from k_row_cost.
__global__ void k_chunk_sums_nocost(const double* __restrict__ X, int d,
                                    const double* __restrict__ w,
                                    const double* __restrict__ cost,
                                    const int32_t* __restrict__ perm,
                                    const int64_t* __restrict__ cstart,
                                    const int64_t* __restrict__ chunkStart, int k,
                                    double* __restrict__ part, double* __restrict__ pw,
                                    double* __restrict__ pc) {
  const int64_t ch = blockIdx.x;
  if (ch >= chunkStart[k]) return;
  int lo = 0, hi = k;
  while (hi - lo > 1) {
    int mid = (lo + hi) >> 1;
    if (chunkStart[mid] <= ch) lo = mid; else hi = mid;
  }
  const int c = lo;
  const int64_t first = cstart[c] + (ch - chunkStart[c]) * kChunkRows;
  const int64_t last = min<int64_t>(cstart[c + 1], first + kChunkRows);
  for (int j = threadIdx.x; j < d; j += blockDim.x) {
    double s = 0.0;
    if (w) {
      for (int64_t p = first; p < last; ++p) {
        const int64_t r = perm[p];
        s = dadd(s, dmul(w[r], X[r * d + j]));
      }
    } else {
      for (int64_t p = first; p < last; ++p) s = dadd(s, X[(int64_t)perm[p] * d + j]);
    }
    part[ch * d + j] = s;
  }
  if (threadIdx.x == 0) {
    double sw = 0.0, sc = 0.0;
    for (int64_t p = first; p < last; ++p) {
      const int64_t r = perm[p];
      const double wt = w ? w[r] : 1.0;
      sw = dadd(sw, wt);
      sc = dadd(sc, dmul(cost[r], wt));
    }
    pw[ch] = sw;
    pc[ch] = sc;
  }
}

// Fold a cluster's chunks in chunk order and add into the caller's sums.
// fS / fW / fA (optional, the incremental sums' state): the cluster's own
// sums, weight and sum of w |x| (from pa) stored besides.
__device__ __forceinline__ void reduce_cluster(const double* __restrict__ part,
                                               const double* __restrict__ pw,
                                               const double* __restrict__ pc,
                                               const int64_t* __restrict__ chunkStart, int d,
                                               double* __restrict__ sums,
                                               double* __restrict__ wsum, double* ccost,
                                               const double* __restrict__ pa,
                                               double* __restrict__ fS, double* __restrict__ fW,
                                               double* __restrict__ fA) {
  const int c = blockIdx.x;
  const int64_t a = chunkStart[c], b = chunkStart[c + 1];
  if (a == b) {
    if (threadIdx.x == 0) ccost[c] = 0.0;
    if (fS) {
      for (int j = threadIdx.x; j < d; j += blockDim.x) fS[(int64_t)c * d + j] = 0.0;
      if (threadIdx.x == 0) fW[c] = fA[c] = 0.0;
    }
    return;
  }
  // chunk order kept; 16 chunks' loads in flight per step
  for (int j = threadIdx.x; j < d; j += blockDim.x) {
    double s = 0.0;
    int64_t ch = a;
    for (; ch + 16 <= b; ch += 16) {
      double v[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) v[u] = part[(ch + u) * d + j];
#pragma unroll
      for (int u = 0; u < 16; ++u) s = dadd(s, v[u]);
    }
    for (; ch < b; ++ch) s = dadd(s, part[ch * d + j]);
    sums[(int64_t)c * d + j] = dadd(sums[(int64_t)c * d + j], s);
    if (fS) fS[(int64_t)c * d + j] = s;
  }
  // the weight and cost folds on two other waves (pa on a third)
  const int tw = 64 % blockDim.x, tc = 128 % blockDim.x, ta = 192 % blockDim.x;
  if (fS && threadIdx.x == ta && ta != tw && ta != tc) {
    double s = 0.0;
    for (int64_t ch = a; ch < b; ++ch) s = dadd(s, pa[ch]);
    fA[c] = s;
  }
  if (threadIdx.x == tw || threadIdx.x == tc) {
    const double* src = threadIdx.x == tw ? pw : pc;
    double s = 0.0;
    int64_t ch = a;
    for (; ch + 8 <= b; ch += 8) {
      double v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = src[ch + u];
#pragma unroll
      for (int u = 0; u < 8; ++u) s = dadd(s, v[u]);
    }
    for (; ch < b; ++ch) s = dadd(s, src[ch]);
    if (threadIdx.x == tw) {
      wsum[c] = dadd(wsum[c], s);
      if (fS) fW[c] = s;
    } else {
      ccost[c] = s;
    }
  }
}

__global__ void k_reduce_clusters(const double* __restrict__ part, const double* __restrict__ pw,
                                  const double* __restrict__ pc,
                                  const int64_t* __restrict__ chunkStart, int d,
                                  double* __restrict__ sums, double* __restrict__ wsum,
                                  double* __restrict__ ccost, const double* __restrict__ pa,
                                  double* __restrict__ fS, double* __restrict__ fW,
                                  double* __restrict__ fA, const int* __restrict__ gate) {
  if (gate && !*gate) return;
  reduce_cluster(part, pw, pc, chunkStart, d, sums, wsum, ccost, pa, fS, fW, fA);
}

// Fixed-shape tree over 256 threads: cost_sum += sum_c ccost[c].
__device__ __forceinline__ void cost_total(const double* ccost, int k, double* __restrict__ out) {
  __shared__ double s[256];
  double a = 0.0;
  for (int c = threadIdx.x; c < k; c += 256) a = dadd(a, ccost[c]);
  s[threadIdx.x] = a;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (threadIdx.x < off) s[threadIdx.x] = dadd(s[threadIdx.x], s[threadIdx.x + off]);
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = dadd(out[0], s[0]);
}

// Single block.
__global__ void k_cost_total(const double* __restrict__ ccost, int k, double* __restrict__ out,
                             const int* __restrict__ gate) {
  if (gate && !*gate) return;
  cost_total(ccost, k, out);
}

// ------------------------------------------------ the gated full pass
// The full pass behind inc_accumulate's gate runs in few of a fit's calls,
// but its launches are enqueued in all of them (the host cannot read the
// gate without draining the stream), so it is four launches there, each of
// which ends on a closed gate: k_hist_scan_gated, k_scatter_gated,
// k_chunk_sums_fast_gated, k_reduce_cost_gated.  The single-workgroup stages
// between the ungated pass's kernels run in the last workgroup to finish the
// stage before them; no workgroup waits for another.  Same results as the
// ungated pass: the integer stages are exact in any grouping, every fp64
// fold keeps its operands' order.

// True (in every thread) in the last of `total` workgroups to arrive at
// *ticket, which it zeroes again for the next call; that workgroup then sees
// what the others stored before arriving (an agent-scope release before the
// ticket, an acquire after it: the XCDs' L2s are not coherent).  Data handed
// over this way is read through pointers that are not const __restrict__.
__device__ __forceinline__ bool last_arrival(unsigned int* ticket, unsigned int total,
                                             int* lastLds) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned int t =
        __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int last = t + 1 == total;
    if (last) {
      __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    *lastLds = last;
  }
  __syncthreads();
  return *lastLds != 0;
}

// Rows t0..t1 of a[t * k + c] replaced by their exclusive running sums down
// each column c (256 threads over the columns), done(c, the column's sum).
// Four columns by eight rows of loads in flight per thread.
template <class T, class F>
__device__ __forceinline__ void scan_columns(int32_t* a, int t0, int t1, int k, F&& done) {
  constexpr int CQ = 4, TB = 8;
  for (int cb = threadIdx.x; cb < k; cb += 256 * CQ) {
    T run[CQ];
#pragma unroll
    for (int u = 0; u < CQ; ++u) run[u] = 0;
    for (int t = t0; t < t1; t += TB) {
      int32_t h[CQ][TB];
#pragma unroll
      for (int u = 0; u < CQ; ++u)
#pragma unroll
        for (int v = 0; v < TB; ++v) {
          const int c = cb + 256 * u;
          h[u][v] = (c < k && t + v < t1) ? a[(int64_t)(t + v) * k + c] : 0;
        }
#pragma unroll
      for (int u = 0; u < CQ; ++u)
#pragma unroll
        for (int v = 0; v < TB; ++v) {
          const int c = cb + 256 * u;
          if (c < k && t + v < t1) {
            a[(int64_t)(t + v) * k + c] = (int32_t)run[u];
            run[u] += h[u][v];
          }
        }
    }
#pragma unroll
    for (int u = 0; u < CQ; ++u)
      if (cb + 256 * u < k) done(cb + 256 * u, run[u]);
  }
}

constexpr int kTicketWords = 128;  // [0] the segments', [1 + s] segment s's tiles', [127] the folds'
static_assert(kScanSegs + 1 < kTicketWords - 1, "one ticket per scan segment");

// k_hist, then per segment of segT tiles (the last of its tiles' workgroups)
// k_scan_seg and k_scan_apply's walk in one -- the tiles' offsets inside the
// segment, in place, and the segment's sums; k_scatter_gated adds the
// segment's own offset -- then (the last segment's workgroup) k_scan_segoff
// and k_scan_clusters.
__global__ __launch_bounds__(256) void k_hist_scan_gated(
    const int32_t* __restrict__ assign, int64_t n, int k, int tiles, int segT, int segs,
    int32_t* hist, int32_t* segsum, int64_t* total, int64_t* __restrict__ cstart,
    int64_t* __restrict__ chunkStart, unsigned int* tickets, const int* __restrict__ gate) {
  if (!*gate) return;
  extern __shared__ int32_t cnt[];
  __shared__ int lastS;
  __shared__ int64_t s_rows[256], s_chunks[256];
  const int tid = threadIdx.x;
  for (int c = tid; c < k; c += 256) cnt[c] = 0;
  __syncthreads();
  const int64_t r0 = (int64_t)blockIdx.x * kSortTile;
  const int64_t r1 = min<int64_t>(n, r0 + kSortTile);
  for (int64_t r = r0 + tid; r < r1; r += 256) atomicAdd(&cnt[assign[r]], 1);
  __syncthreads();
  for (int c = tid; c < k; c += 256) hist[(int64_t)blockIdx.x * k + c] = cnt[c];
  const int seg = (int)blockIdx.x / segT;
  const int t0 = seg * segT, t1 = min(tiles, t0 + segT);
  if (!last_arrival(&tickets[1 + seg], (unsigned)(t1 - t0), &lastS)) return;
  scan_columns<int32_t>(hist, t0, t1, k,
                        [&](int c, int32_t sum) { segsum[(int64_t)seg * k + c] = sum; });
  if (!last_arrival(&tickets[0], (unsigned)segs, &lastS)) return;
  scan_columns<int64_t>(segsum, 0, segs, k, [&](int c, int64_t sum) { total[c] = sum; });
  __syncthreads();
  // k_scan_clusters over 256 threads
  const int per = (k + 255) / 256;
  int64_t rows = 0, chunks = 0;
  for (int q = 0; q < per; ++q) {
    const int c = tid * per + q;
    if (c < k) {
      rows += total[c];
      chunks += (total[c] + kChunkRows - 1) / kChunkRows;
    }
  }
  s_rows[tid] = rows;
  s_chunks[tid] = chunks;
  __syncthreads();
  for (int off = 1; off < 256; off <<= 1) {
    const int64_t a = tid >= off ? s_rows[tid - off] : 0, b = tid >= off ? s_chunks[tid - off] : 0;
    __syncthreads();
    s_rows[tid] += a;
    s_chunks[tid] += b;
    __syncthreads();
  }
  int64_t rbase = tid ? s_rows[tid - 1] : 0, cbase = tid ? s_chunks[tid - 1] : 0;
  for (int q = 0; q < per; ++q) {
    const int c = tid * per + q;
    if (c < k) {
      cstart[c] = rbase;
      chunkStart[c] = cbase;
      rbase += total[c];
      cbase += (total[c] + kChunkRows - 1) / kChunkRows;
    }
  }
  if (tid == 255) {
    cstart[k] = s_rows[255];
    chunkStart[k] = s_chunks[255];
  }
}

__global__ void k_scatter_gated(const int32_t* __restrict__ assign, int64_t n, int k,
                                const int32_t* __restrict__ tileOff,
                                const int64_t* __restrict__ cstart, int32_t* __restrict__ perm,
                                int64_t tiles, const int32_t* __restrict__ segOff, int segT,
                                const int* __restrict__ gate) {
  if (!*gate) return;
  scatter_tile(assign, n, k, tileOff, cstart, perm, tiles, segOff, segT);
}

// k_reduce_clusters, then k_cost_total in the last cluster's workgroup to finish.
__global__ __launch_bounds__(256) void k_reduce_cost_gated(
    const double* __restrict__ part, const double* __restrict__ pw, const double* __restrict__ pc,
    const int64_t* __restrict__ chunkStart, int d, int k, double* __restrict__ sums,
    double* __restrict__ wsum, double* ccost, const double* __restrict__ pa,
    double* __restrict__ fS, double* __restrict__ fW, double* __restrict__ fA,
    double* __restrict__ costSum, unsigned int* ticket, const int* __restrict__ gate) {
  if (!*gate) return;
  __shared__ int lastS;
  reduce_cluster(part, pw, pc, chunkStart, d, sums, wsum, ccost, pa, fS, fW, fA);
  if (!last_arrival(ticket, (unsigned)k, &lastS)) return;
  cost_total(ccost, k, costSum);
}

// ------------------------------------------------- incremental cluster sums
// (round 6) With the carried bounds most rows keep their center from one
// Lloyd call of a fit to the next, so the cluster sums change only by the
// rows that moved.  The row image's owner keeps, per cluster c, the sums S_c,
// weight W_c (unit weights: the count), member count N_c, a reference point
// P_c (the centers of the last full pass) with Q_c = sum |x - P_c|^2 over the
// members, and A_c = sum |x| (error scale).  A call with few moved rows
// (<= n / kIncMovedFrac) updates them by the moved rows alone (subtracted
// from the old cluster, added to the new, in row order: each cluster's
// workgroup picks its entries from the row-ordered moved list) and takes the cost
// for the call's centers c from
//   sum_x |x - c|^2 = Q_c + 2 (P_c - c).(S_c - W_c P_c) + W_c |P_c - c|^2,
// which is exact algebra; the rounding of every term is bounded on the device
// (ES_c, EQ_c and the correction's own).  When the bound
// exceeds 2^-40 of the cost, a moved count is too large, or no state exists,
// the call runs the full pass over every row instead (the sort by cluster and
// k_chunk_sums_fast), which resets the state.  Gates: gate[0] = 1 runs the
// full pass, gate[1] = 1 the incremental one; exactly one is set.
constexpr int kIncRows = 2048;       // rows per k_inc_moved workgroup
constexpr int kIncMovedFrac = 16;    // at most n / 16 moved rows take the incremental path
                                     // (kIncSplit workgroups fold a cluster's entries: a large
                                     // churn concentrates on a few clusters)

// The rows whose assignment differs from prev (then prev = assign): per
// kIncRows-row block, in row order, into tmpRow / tmpOld at the block's base;
// the block's count in bcount[block].
__global__ __launch_bounds__(256) void k_inc_moved(const int32_t* __restrict__ assign,
                                                   int32_t* __restrict__ prev, int64_t n,
                                                   int32_t* __restrict__ tmpRow,
                                                   int32_t* __restrict__ tmpOld,
                                                   unsigned int* __restrict__ bcount) {
  constexpr int IT = kIncRows / 256;
  __shared__ unsigned wc[IT * 4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t base = (int64_t)blockIdx.x * kIncRows;
  unsigned long long masks[IT];
  int32_t olds[IT];
#pragma unroll
  for (int it = 0; it < IT; ++it) {
    const int64_t r = base + it * 256 + tid;
    bool moved = false;
    olds[it] = -1;
    if (r < n) {
      const int32_t a = assign[r], b = prev[r];
      moved = a != b;
      olds[it] = b;
      if (moved) prev[r] = a;
    }
    masks[it] = __builtin_amdgcn_ballot_w64(moved);
    if (lane == 0) wc[it * 4 + wave] = (unsigned)__builtin_popcountll(masks[it]);
  }
  __syncthreads();
  const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
  for (int it = 0; it < IT; ++it) {
    unsigned before = 0;
    for (int j = 0; j < it * 4 + wave; ++j) before += wc[j];
    if ((masks[it] >> lane) & 1ull) {
      const int64_t pos = base + before + (unsigned)__builtin_popcountll(masks[it] & below);
      tmpRow[pos] = (int32_t)(base + it * 256 + tid);
      tmpOld[pos] = olds[it];
    }
  }
  if (tid == 0) {
    unsigned total = 0;
    for (int j = 0; j < IT * 4; ++j) total += wc[j];
    bcount[blockIdx.x] = total;
  }
}

// Single block: bcount[0..nb) -> exclusive offsets, bcount[nb] = *count = the
// moved rows; the gates (incremental when valid and count <= mcap); *movedCum
// += count on the incremental path.
__global__ __launch_bounds__(1024) void k_inc_scan(unsigned int* __restrict__ bcount, int64_t nb,
                                                   unsigned int* __restrict__ count, int valid,
                                                   int64_t mcap, int* __restrict__ gate,
                                                   unsigned long long* __restrict__ movedCum) {
  __shared__ unsigned part[1024];
  const int t = threadIdx.x;
  const int64_t per = (nb + 1023) / 1024;
  const int64_t a = min<int64_t>(nb, t * per), e = min<int64_t>(nb, a + per);
  unsigned s = 0;
  for (int64_t i = a; i < e; ++i) s += bcount[i];
  part[t] = s;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {
    const unsigned v = t >= off ? part[t - off] : 0u;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  unsigned run = t ? part[t - 1] : 0u;
  for (int64_t i = a; i < e; ++i) {
    const unsigned c = bcount[i];
    bcount[i] = run;
    run += c;
  }
  if (t == 1023) {
    const unsigned total = part[1023];
    bcount[nb] = total;
    *count = total;
    const int inc = valid && (int64_t)total <= mcap;
    gate[0] = inc ? 0 : 1;
    gate[1] = inc ? 1 : 0;
    if (inc) *movedCum += (unsigned long long)total;
  }
}

// The blocks' moved rows behind their offsets, with their new and old
// clusters (incremental path only).
__global__ __launch_bounds__(256) void k_inc_gather(const int32_t* __restrict__ tmpRow,
                                                    const int32_t* __restrict__ tmpOld,
                                                    const unsigned int* __restrict__ bcount,
                                                    const int32_t* __restrict__ assign,
                                                    int32_t* __restrict__ movedRow,
                                                    int32_t* __restrict__ movedNew,
                                                    int32_t* __restrict__ movedOld,
                                                    const int* __restrict__ gate) {
  if (!gate[1]) return;
  const int64_t b = blockIdx.x, base = b * kIncRows;
  const unsigned off = bcount[b], cnt = bcount[b + 1] - off;
  for (unsigned i = threadIdx.x; i < cnt; i += 256) {
    const int32_t r = tmpRow[base + i];
    movedRow[off + i] = r;
    movedNew[off + i] = assign[r];
    movedOld[off + i] = tmpOld[base + i];
  }
}

// Block sum of NV doubles per thread (fixed tree, results in every thread).
template <int NV>
__device__ __forceinline__ void inc_block_sum(double (&v)[NV], double* red) {
  const int tid = threadIdx.x;
  __syncthreads();
#pragma unroll
  for (int i = 0; i < NV; ++i) red[i * 256 + tid] = v[i];
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (tid < off) {
#pragma unroll
      for (int i = 0; i < NV; ++i) red[i * 256 + tid] = dadd(red[i * 256 + tid], red[i * 256 + tid + off]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < NV; ++i) v[i] = red[i * 256];
}

// kIncSplit workgroups per cluster, each over one contiguous slice of the
// moved list: the cluster's entries there (the moved rows that left or
// joined it) picked in list order -- kIncScan entries per thread per step,
// compacted in order through LDS -- and folded into a partial (sums per
// dimension; the cost terms, count and norm sums as scalars).  Unit weights.
constexpr int kIncScan = 8;
constexpr int kIncSplit = 8;
constexpr int kIncPs = 6;   // scalars per partial: dq, |dq|, count, sum |x| signed, sum |x|, entries
template <int NJ>
__global__ __launch_bounds__(256) void k_inc_part(
    const double* __restrict__ X, int d, const double* __restrict__ xnorm,
    const int32_t* __restrict__ movedRow, const int32_t* __restrict__ movedNew,
    const int32_t* __restrict__ movedOld, const unsigned int* __restrict__ count,
    const double* __restrict__ P, double* __restrict__ pds, double* __restrict__ psc,
    const int* __restrict__ gate) {
  if (!gate[1]) return;
  constexpr int B = 256 * kIncScan;
  __shared__ int32_t rowsS[B];
  __shared__ float sgS[B];
  __shared__ unsigned wcS[kIncScan * 4];
  __shared__ double red[5 * 256];
  const int c = blockIdx.x, g = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned m = *count;
  const unsigned s0 = (unsigned)((uint64_t)m * g / kIncSplit);
  const unsigned s1 = (unsigned)((uint64_t)m * (g + 1) / kIncSplit);
  int64_t ent = 0;
  double ds[NJ], dq[NJ], dqa[NJ], pj[NJ];
#pragma unroll
  for (int u = 0; u < NJ; ++u) {
    const int j = tid + 256 * u;
    ds[u] = dq[u] = dqa[u] = 0.0;
    pj[u] = j < d ? P[(int64_t)c * d + j] : 0.0;
  }
  double tN = 0.0, tA = 0.0, tAbs = 0.0;   // this thread's entries: count, sum |x|
  const unsigned long long below = (1ull << lane) - 1ull;
  for (unsigned base = s0; base < s1; base += B) {
    int nw[kIncScan], ol[kIncScan];
#pragma unroll
    for (int q = 0; q < kIncScan; ++q) {
      const unsigned i = base + q * 256 + tid;
      nw[q] = i < s1 ? movedNew[i] : -1;
      ol[q] = i < s1 ? movedOld[i] : -1;
    }
    unsigned long long mk[kIncScan];
    __syncthreads();   // the previous batch's entries are folded
#pragma unroll
    for (int q = 0; q < kIncScan; ++q) {
      mk[q] = __builtin_amdgcn_ballot_w64(nw[q] == c || ol[q] == c);
      if (lane == 0) wcS[q * 4 + wave] = (unsigned)__builtin_popcountll(mk[q]);
    }
    __syncthreads();
    int cnt = 0;
#pragma unroll
    for (int q = 0; q < kIncScan; ++q) {
      unsigned before = 0;
      for (int j = 0; j < q * 4 + wave; ++j) before += wcS[j];
      if ((mk[q] >> lane) & 1ull) {
        const unsigned pos = before + (unsigned)__builtin_popcountll(mk[q] & below);
        rowsS[pos] = movedRow[base + q * 256 + tid];
        sgS[pos] = nw[q] == c ? 1.0f : -1.0f;
      }
    }
    for (int j = 0; j < kIncScan * 4; ++j) cnt += (int)wcS[j];
    __syncthreads();
    ent += cnt;
    for (int e = tid; e < cnt; e += 256) {
      const bool add = sgS[e] > 0.0f;
      const double xn = xnorm[rowsS[e]];
      tN += add ? 1.0 : -1.0;
      tA = add ? dadd(tA, xn) : dsub(tA, xn);
      tAbs = dadd(tAbs, xn);
    }
    for (int p0 = 0; p0 < cnt; p0 += 8) {
      double xv[8][NJ];
#pragma unroll
      for (int v = 0; v < 8; ++v) {
        const int64_t r = rowsS[min(p0 + v, cnt - 1)];
#pragma unroll
        for (int u = 0; u < NJ; ++u) {
          const int j = tid + 256 * u;
          xv[v][u] = j < d ? X[r * d + j] : 0.0;
        }
      }
#pragma unroll
      for (int v = 0; v < 8; ++v) {
        if (p0 + v < cnt) {
          const bool add = sgS[p0 + v] > 0.0f;
#pragma unroll
          for (int u = 0; u < NJ; ++u) {
            const double x = xv[v][u];
            const double df = dsub(pj[u], x);
            const double t = dmul(df, df);
            ds[u] = add ? dadd(ds[u], x) : dsub(ds[u], x);
            dq[u] = add ? dadd(dq[u], t) : dsub(dq[u], t);
            dqa[u] = dadd(dqa[u], t);
          }
        }
      }
    }
  }
  double r1[5] = {0.0, 0.0, tN, tA, tAbs};
#pragma unroll
  for (int u = 0; u < NJ; ++u) {
    r1[0] = dadd(r1[0], dq[u]);
    r1[1] = dadd(r1[1], dqa[u]);
  }
  inc_block_sum<5>(r1, red);
  const int64_t slot = (int64_t)c * kIncSplit + g;
#pragma unroll
  for (int u = 0; u < NJ; ++u) {
    const int j = tid + 256 * u;
    if (j < d) pds[slot * d + j] = ds[u];
  }
  if (tid < 5) psc[slot * kIncPs + tid] = r1[tid];
  if (tid == 5) psc[slot * kIncPs + 5] = (double)ent;
}

// One workgroup per cluster: its partials summed in slice order, folded into
// the state; then its cost for the call's centers C and the bound of that
// cost's rounding (cerr), cbad = 1 when the state's error grew past 2^-38 of
// the sum of the members' norms.
template <int NJ>
__global__ __launch_bounds__(256) void k_inc_combine(
    int d, const double* __restrict__ C, const double* __restrict__ pds,
    const double* __restrict__ psc, double* __restrict__ S, const double* __restrict__ P,
    double* __restrict__ W, double* __restrict__ Q, int64_t* __restrict__ N,
    double* __restrict__ A, double* __restrict__ ES, double* __restrict__ EQ,
    double* __restrict__ ccost, double* __restrict__ cerr, int* __restrict__ cbad,
    const int* __restrict__ gate) {
  if (!gate[1]) return;
  __shared__ double red[4 * 256];
  const int c = blockIdx.x, tid = threadIdx.x;
  double r1[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  int64_t ent = 0;
  double ds[NJ], pj[NJ];
#pragma unroll
  for (int u = 0; u < NJ; ++u) {
    const int j = tid + 256 * u;
    ds[u] = 0.0;
    pj[u] = j < d ? P[(int64_t)c * d + j] : 0.0;
  }
  for (int g = 0; g < kIncSplit; ++g) {
    const int64_t slot = (int64_t)c * kIncSplit + g;
#pragma unroll
    for (int u = 0; u < NJ; ++u) {
      const int j = tid + 256 * u;
      if (j < d) ds[u] = dadd(ds[u], pds[slot * d + j]);
    }
#pragma unroll
    for (int i = 0; i < 5; ++i) r1[i] = dadd(r1[i], psc[slot * kIncPs + i]);
    ent += (int64_t)psc[slot * kIncPs + 5];
  }
  const int64_t nNew = N[c] + (int64_t)r1[2];
  const bool empty = nNew <= 0;
  const double wNew = empty ? 0.0 : (double)nNew;    // unit weights: the count
  double sv[NJ];
#pragma unroll
  for (int u = 0; u < NJ; ++u) {
    const int j = tid + 256 * u;
    const double s0 = j < d ? S[(int64_t)c * d + j] : 0.0;
    sv[u] = empty ? 0.0 : (ent ? dadd(s0, ds[u]) : s0);
    if (j < d && ent) S[(int64_t)c * d + j] = sv[u];
  }
  // the cost's terms for the call's centers
  double r2[4] = {0.0, 0.0, 0.0, 0.0};   // |S|^2, D.V, |D|^2, |P|^2
#pragma unroll
  for (int u = 0; u < NJ; ++u) {
    const int j = tid + 256 * u;
    if (j < d) {
      const double D = dsub(pj[u], C[(int64_t)c * d + j]);
      const double V = dsub(sv[u], dmul(wNew, pj[u]));
      r2[0] = dadd(r2[0], dmul(sv[u], sv[u]));
      r2[1] = dadd(r2[1], dmul(D, V));
      r2[2] = dadd(r2[2], dmul(D, D));
      r2[3] = dadd(r2[3], dmul(pj[u], pj[u]));
    }
  }
  inc_block_sum<4>(r2, red);
  if (tid == 0) {
    double q = Q[c], a = A[c], es = ES[c], eq = EQ[c];
    if (empty) {
      q = a = es = eq = 0.0;
    } else if (ent) {
      const double nS = sqrt(r2[0]) * (1.0 + 0x1p-50);
      q = dadd(q, r1[0]);
      a = dadd(a, r1[3]);
      // a slice's entries sum sequentially, then the slices and (for the
      // cost terms) the dimensions and the block tree: <= ent + kIncSplit
      // + 16 roundings per term
      es += 0x1p-52 * ((double)(ent + kIncSplit + 1) * r1[4] + nS);
      eq += 0x1p-52 * ((double)(ent + kIncSplit + 16) * r1[1] + fabs(q));
    }
    N[c] = empty ? 0 : nNew;
    W[c] = wNew;
    Q[c] = q;
    A[c] = a;
    ES[c] = es;
    EQ[c] = eq;
    double cost = 0.0, err = 0.0;
    int bad = 0;
    if (!empty) {
      const double nS = sqrt(r2[0]) * (1.0 + 0x1p-50), nD = sqrt(r2[2]) * (1.0 + 0x1p-50),
                   nP = sqrt(r2[3]) * (1.0 + 0x1p-50);
      cost = dadd(q, dadd(dmul(2.0, r2[1]), dmul(wNew, r2[2])));
      const double sv2 = nS + wNew * nP;
      // the correction's own rounding: D and V (one rounding each, the
      // 2^-51 term), the dot's and |D|^2's sums (<= NJ + 8 + 2 <= 14
      // roundings of terms bounded by |D| |V|, |D|^2: 2 x 16 x 2^-53 <=
      // 2^-47, taken as 2^-46)
      err = eq + 2.0 * nD * (es + 0x1p-51 * sv2) + 0x1p-46 * (nD * sv2 + wNew * r2[2]) +
            0x1p-50 * fabs(cost);
      bad = !(es <= 0x1p-38 * a) || !(fabs(cost) < INFINITY) || !(err < INFINITY);
    }
    ccost[c] = cost;
    cerr[c] = err;
    cbad[c] = bad;
  }
}

// Single block: the clusters' costs and error bounds summed in a fixed
// tree; the incremental result stands when no cluster is flagged and the
// bound is within 2^-40 of the cost, else the gates switch to the full pass.
__global__ __launch_bounds__(256) void k_inc_check(const double* __restrict__ ccost,
                                                   const double* __restrict__ cerr,
                                                   const int* __restrict__ cbad, int k,
                                                   int* __restrict__ gate,
                                                   double* __restrict__ tot,
                                                   unsigned long long* __restrict__ incCum) {
  if (!gate[1]) return;
  __shared__ double red[3 * 256];
  double v[3] = {0.0, 0.0, 0.0};
  for (int c = threadIdx.x; c < k; c += 256) {
    v[0] = dadd(v[0], ccost[c]);
    v[1] += cerr[c];
    v[2] += cbad[c] ? 1.0 : 0.0;
  }
  inc_block_sum<3>(v, red);
  if (threadIdx.x == 0) {
    const bool ok = v[2] == 0.0 && v[1] <= 0x1p-40 * fabs(v[0]) && fabs(v[0]) < INFINITY;
    tot[0] = v[0];
    tot[1] = v[1];
    if (ok) {
      *incCum += 1ull;
    } else {
      gate[0] = 1;
      gate[1] = 0;
    }
  }
}

// After the check (one launch, k_inc_finish): the incremental result into
// the caller's buffers (gate[1]: sums += S, wsum += W, cost_sum += the
// checked total); after a full pass (gate[0]) its fresh sums are the state
// (written by k_reduce_clusters), P = C, Q = the clusters' costs, N = the
// counts, and the error bounds of the full pass's own summation (<= 256
// rows per chunk partial, the block tree, then the chunk fold).  The two
// read and write disjoint buffers, so one after the other or side by side
// is the same.
__global__ __launch_bounds__(256) void k_inc_finish(
    const double* __restrict__ C, int d, double* __restrict__ P, const double* __restrict__ ccost,
    const int64_t* __restrict__ total, const int64_t* __restrict__ chunkStart,
    double* __restrict__ Q, int64_t* __restrict__ N, const double* __restrict__ A,
    double* __restrict__ ES, double* __restrict__ EQ, const double* __restrict__ S,
    const double* __restrict__ W, const double* __restrict__ tot, double* __restrict__ sums,
    double* __restrict__ wsum, double* __restrict__ costSum, const int* __restrict__ gate) {
  const int c = blockIdx.x;
  if (gate[0]) {
    for (int j = threadIdx.x; j < d; j += 256) P[(int64_t)c * d + j] = C[(int64_t)c * d + j];
    if (threadIdx.x == 0) {
      const double f = 0x1p-52 * (double)(300 + (chunkStart[c + 1] - chunkStart[c]));
      Q[c] = ccost[c];
      N[c] = total[c];
      ES[c] = f * A[c];
      EQ[c] = f * fabs(ccost[c]);
    }
  }
  if (gate[1]) {
    for (int j = threadIdx.x; j < d; j += 256)
      sums[(int64_t)c * d + j] = dadd(sums[(int64_t)c * d + j], S[(int64_t)c * d + j]);
    if (threadIdx.x == 0) {
      wsum[c] = dadd(wsum[c], W[c]);
      if (c == 0) costSum[0] = dadd(costSum[0], tot[0]);
    }
  }
}

constexpr int kUpdLds = 3072;   // widest center staged in LDS by k_update_centers

// centroid (DistanceMeasure.scala:200-203: scal(1/w, sum); new VectorWithNorm)
// and isCenterConverged (:345-350).  One 64-lane workgroup per center: the
// elementwise part in parallel, then lane 0 runs the two sequential sums (the
// moved distance and the new norm, in index order) from LDS.  The caller sets
// *converged = 1 first; a center that moved clears it.
__global__ __launch_bounds__(64) void k_update_centers(
    double* __restrict__ C, double* __restrict__ cnorm, const double* __restrict__ sums,
    const double* __restrict__ wsum, int k, int d, double eps2, int32_t* __restrict__ converged) {
  extern __shared__ double upd[];   // 2 d (d <= kUpdLds)
  const int c = blockIdx.x, lane = threadIdx.x;
  const double w = wsum[c];
  if (!(w > 0)) return;
  const double a = 1.0 / w;
  double* crow = C + (int64_t)c * d;
  const double* srow = sums + (int64_t)c * d;
  if (d > kUpdLds) {
    // wide (sparse-input) centers: lane 0 reads both rows in order first
    if (lane == 0) {
      double moved = 0.0, nn = 0.0;
      for (int j = 0; j < d; ++j) {
        const double v = dmul(a, srow[j]);
        const double sc = dsub(v, crow[j]);
        moved = dadd(moved, dmul(sc, sc));
        nn = dadd(nn, dmul(v, v));
      }
      cnorm[c] = __builtin_sqrt(nn);
      if (!(moved <= eps2) && converged) atomicAnd(converged, 0);
    }
    __syncthreads();
    for (int j = lane; j < d; j += 64) crow[j] = dmul(a, srow[j]);
    return;
  }
  for (int j = lane; j < d; j += 64) {
    const double v = dmul(a, srow[j]);
    const double sc = dsub(v, crow[j]);
    upd[j] = dmul(sc, sc);
    upd[d + j] = dmul(v, v);
    crow[j] = v;
  }
  __syncthreads();
  if (lane == 0) {
    double moved = 0.0, nn = 0.0;
    for (int j = 0; j < d; ++j) {
      moved = dadd(moved, upd[j]);
      nn = dadd(nn, upd[d + j]);
    }
    cnorm[c] = __builtin_sqrt(nn);
    if (!(moved <= eps2) && converged) atomicAnd(converged, 0);
  }
}

// The chunk-sum and incremental kernels are instantiated per NJ = 1, 2, 4
// column groups of 256 (d <= 1024): f(integral_constant<NJ>) for nj groups.
template <class F>
void with_nj(int nj, F&& f) {
  if (nj == 1) f(std::integral_constant<int, 1>{});
  else if (nj == 2) f(std::integral_constant<int, 2>{});
  else f(std::integral_constant<int, 4>{});
}

}  // namespace

namespace cyc {
namespace kmsums {

int sort_clusters(SortScratch& s, const int32_t* assign, int64_t n, int d, int k, hipStream_t st,
                  int64_t& maxChunks, const int* gate) {
  int rc;
  const int tiles = (int)((n + kSortTile - 1) / kSortTile);
  maxChunks = (n + kChunkRows - 1) / kChunkRows + k;
  if ((rc = s.hist.reserve(sizeof(int32_t) * (size_t)tiles * k)) ||
      (rc = s.total.reserve(sizeof(int64_t) * (size_t)k)) ||
      (rc = s.cstart.reserve(sizeof(int64_t) * (size_t)(k + 1))) ||
      (rc = s.chunkStart.reserve(sizeof(int64_t) * (size_t)(k + 1))) ||
      (rc = s.perm.reserve(sizeof(int32_t) * (size_t)n)) ||
      (rc = s.part.reserve(sizeof(double) * (size_t)maxChunks * d)) ||
      (rc = s.pw.reserve(sizeof(double) * (size_t)maxChunks)) ||
      (rc = s.pc.reserve(sizeof(double) * (size_t)maxChunks)) ||
      (rc = s.ccost.reserve(sizeof(double) * (size_t)k)))
    return rc;
  int32_t* hist = (int32_t*)s.hist.ptr;
  const int segT = (tiles + std::min(kScanSegs, tiles) - 1) / std::min(kScanSegs, tiles);
  const int segs = (tiles + segT - 1) / segT;
  if ((rc = s.segsum.reserve(sizeof(int32_t) * (size_t)segs * k))) return rc;
  int32_t* segsum = (int32_t*)s.segsum.ptr;
  if (gate) {
    // two launches (the gated full pass above); the tickets are zero between
    // calls: zeroed when allocated, then by their last arrivals
    const void* had = s.tickets.ptr;
    const int hadDev = s.tickets.device;
    if ((rc = s.tickets.reserve(sizeof(unsigned int) * kTicketWords))) return rc;
    if (s.tickets.ptr != had || s.tickets.device != hadDev)
      CYC_HIP(hipMemsetAsync(s.tickets.ptr, 0, sizeof(unsigned int) * kTicketWords, st));
    hipLaunchKernelGGL(k_hist_scan_gated, dim3(tiles), dim3(256), sizeof(int32_t) * k, st, assign,
                       n, k, tiles, segT, segs, hist, segsum, (int64_t*)s.total.ptr,
                       (int64_t*)s.cstart.ptr, (int64_t*)s.chunkStart.ptr,
                       (unsigned int*)s.tickets.ptr, gate);
    CYC_LAUNCH_CHECK("k_hist_scan_gated");
    hipLaunchKernelGGL(k_scatter_gated, dim3((unsigned)(8 * (((int64_t)tiles + 7) / 8))), dim3(64),
                       sizeof(int64_t) * k, st, assign, n, k, (const int32_t*)hist,
                       (const int64_t*)s.cstart.ptr, (int32_t*)s.perm.ptr, (int64_t)tiles,
                       (const int32_t*)segsum, segT, gate);
    CYC_LAUNCH_CHECK("k_scatter_gated");
    return CYC_OK;
  }
  hipLaunchKernelGGL(k_hist, dim3(tiles), dim3(256), sizeof(int32_t) * k, st, assign, n, k, hist,
                     gate);
  CYC_LAUNCH_CHECK("k_hist");
  {
    hipLaunchKernelGGL(k_scan_seg, dim3((unsigned)((k + 63) / 64), (unsigned)segs), dim3(64), 0, st,
                       (const int32_t*)hist, tiles, k, segT, segsum, gate);
    CYC_LAUNCH_CHECK("k_scan_seg");
    hipLaunchKernelGGL(k_scan_segoff, dim3((unsigned)((k + 255) / 256)), dim3(256), 0, st, segsum,
                       segs, k, (int64_t*)s.total.ptr, gate);
    CYC_LAUNCH_CHECK("k_scan_segoff");
    hipLaunchKernelGGL(k_scan_apply, dim3((unsigned)((k + 63) / 64), (unsigned)segs), dim3(64), 0,
                       st, hist, tiles, k, segT, (const int32_t*)segsum, gate);
    CYC_LAUNCH_CHECK("k_scan_apply");
  }
  hipLaunchKernelGGL(k_scan_clusters, dim3(1), dim3(1024), 0, st, (const int64_t*)s.total.ptr, k,
                     (int64_t*)s.cstart.ptr, (int64_t*)s.chunkStart.ptr, gate);
  CYC_LAUNCH_CHECK("k_scan_clusters");
  hipLaunchKernelGGL(k_scatter, dim3((unsigned)(8 * (((int64_t)tiles + 7) / 8))), dim3(64),
                     sizeof(int64_t) * k, st, assign, n, k, hist, (const int64_t*)s.cstart.ptr,
                     (int32_t*)s.perm.ptr, (int64_t)tiles, gate);
  CYC_LAUNCH_CHECK("k_scatter");
  return CYC_OK;
}

int full_pass(SortScratch& s, const double* X, int64_t n, int d, int k, const double* weights,
              const double* xnorm, bool cosine, const double* C, const int32_t* assign,
              double* cost, double* sums, double* wsum, double* cost_sum, hipStream_t st,
              const int* gate, IncState* inc) {
  const int nj = (d + 255) / 256;
  int rc;
  int64_t maxChunks = 0;
  if ((rc = sort_clusters(s, assign, n, d, k, st, maxChunks, gate))) return rc;
  if (inc && (rc = inc->pa.reserve(sizeof(double) * (size_t)maxChunks))) return rc;
  const int32_t* perm = (const int32_t*)s.perm.ptr;
  const int64_t* cstart = (const int64_t*)s.cstart.ptr;
  const int64_t* chunkStart = (const int64_t*)s.chunkStart.ptr;
  double *part = (double*)s.part.ptr, *pw = (double*)s.pw.ptr, *pc = (double*)s.pc.ptr;
  double* pa = inc ? (double*)inc->pa.ptr : nullptr;
  // Number of chunks is data dependent; launch the upper bound and let the
  // surplus blocks (ch >= chunkStart[k]) exit.
  if (cosine) {
    if ((rc = cyc::kmcos::chunk_sums(X, d, weights, xnorm, cost, perm, cstart, chunkStart, k,
                                     maxChunks, part, pw, pc, st)))
      return rc;
  } else {
    cyc::KernelTimer timer("k_chunk_sums", st);
    const dim3 grid((unsigned)maxChunks);
    // no per-row costs, d <= 1024: k_chunk_sums_fast (and the incremental
    // state's sum of w |x| into pa); per-row costs wanted: k_chunk_sums;
    // d > 1024: the costs were computed first (k_row_cost)
    if (gate && inc && !cost && !weights && nj <= 4)
      with_nj(nj, [&](auto NJ) {
        // the gated form: a grid of 8 workgroups per CU strides over the chunks
        const dim3 bounded((unsigned)std::min<int64_t>(maxChunks, 8 * (int64_t)cyc::device_cus()));
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_chunk_sums_fast_gated<decltype(NJ)::value>), bounded,
                           dim3(256), 0, st, X, d, C, perm, cstart, chunkStart, k, part, pw, pc,
                           xnorm, pa, gate);
      });
    else if (!cost && nj <= 4)
      with_nj(nj, [&](auto NJ) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_chunk_sums_fast<decltype(NJ)::value>), grid,
                           dim3(256), 0, st, X, d, weights, C, perm, cstart, chunkStart, k, part,
                           pw, pc, inc ? xnorm : (const double*)nullptr, pa, gate);
      });
    else if (nj <= 4)
      with_nj(nj, [&](auto NJ) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_chunk_sums<decltype(NJ)::value>), grid, dim3(256), 0,
                           st, X, d, weights, C, perm, cstart, chunkStart, k, part, pw, pc,
                           cost);
      });
    else
      hipLaunchKernelGGL(k_chunk_sums_nocost, grid, dim3(256), 0, st, X, d, weights,
                         (const double*)cost, perm, cstart, chunkStart, k, part, pw, pc);
    CYC_LAUNCH_CHECK("k_chunk_sums");
  }
  if (gate && inc && !cosine) {
    hipLaunchKernelGGL(k_reduce_cost_gated, dim3(k), dim3(256), 0, st, (const double*)part,
                       (const double*)pw, (const double*)pc, chunkStart, d, k, sums, wsum,
                       (double*)s.ccost.ptr, (const double*)pa, (double*)inc->S.ptr,
                       (double*)inc->W.ptr, (double*)inc->A.ptr, cost_sum,
                       (unsigned int*)s.tickets.ptr + (kTicketWords - 1), gate);
    CYC_LAUNCH_CHECK("k_reduce_cost_gated");
    return CYC_OK;
  }
  hipLaunchKernelGGL(k_reduce_clusters, dim3(k), dim3(256), 0, st, (const double*)part,
                     (const double*)pw, (const double*)pc, chunkStart, d, sums, wsum,
                     (double*)s.ccost.ptr, (const double*)pa,
                     inc ? (double*)inc->S.ptr : nullptr, inc ? (double*)inc->W.ptr : nullptr,
                     inc ? (double*)inc->A.ptr : nullptr, gate);
  CYC_LAUNCH_CHECK("k_reduce_clusters");
  hipLaunchKernelGGL(k_cost_total, dim3(1), dim3(256), 0, st, (const double*)s.ccost.ptr, k,
                     cost_sum, gate);
  CYC_LAUNCH_CHECK("k_cost_total");
  return CYC_OK;
}

int inc_accumulate(SortScratch& s, IncState& inc, const double* X, const double* xnorm,
                   const int32_t* assign, int64_t n, int d, int k, const double* C, double* sums,
                   double* wsum, double* cost_sum, hipStream_t st) {
  const int nj = (d + 255) / 256;
  const int64_t nb = (n + kIncRows - 1) / kIncRows;
  const int64_t mcap = n / kIncMovedFrac;
  const size_t kd = (size_t)k * d;
  int rc;
  const bool fresh = inc.prev.ptr == nullptr;
  if ((rc = inc.prev.reserve(sizeof(int32_t) * (size_t)n)) ||
      (rc = inc.tmpRow.reserve(sizeof(int32_t) * (size_t)n)) ||
      (rc = inc.tmpOld.reserve(sizeof(int32_t) * (size_t)n)) ||
      (rc = inc.bcount.reserve(sizeof(unsigned int) * (size_t)(nb + 1))) ||
      (rc = inc.count.reserve(64)) || (rc = inc.gate.reserve(64)) ||
      (rc = inc.movedRow.reserve(sizeof(int32_t) * (size_t)std::max<int64_t>(mcap, 1))) ||
      (rc = inc.movedNew.reserve(sizeof(int32_t) * (size_t)std::max<int64_t>(mcap, 1))) ||
      (rc = inc.movedOld.reserve(sizeof(int32_t) * (size_t)std::max<int64_t>(mcap, 1))) ||
      (rc = inc.S.reserve(sizeof(double) * kd)) || (rc = inc.P.reserve(sizeof(double) * kd)) ||
      (rc = inc.pds.reserve(sizeof(double) * kd * kIncSplit)) ||
      (rc = inc.psc.reserve(sizeof(double) * (size_t)k * kIncSplit * kIncPs)) ||
      (rc = inc.W.reserve(sizeof(double) * (size_t)k)) ||
      (rc = inc.Q.reserve(sizeof(double) * (size_t)k)) ||
      (rc = inc.N.reserve(sizeof(int64_t) * (size_t)k)) ||
      (rc = inc.A.reserve(sizeof(double) * (size_t)k)) ||
      (rc = inc.ES.reserve(sizeof(double) * (size_t)k)) ||
      (rc = inc.EQ.reserve(sizeof(double) * (size_t)k)) ||
      (rc = inc.cost.reserve(sizeof(double) * (size_t)k)) ||
      (rc = inc.err.reserve(sizeof(double) * (size_t)k)) ||
      (rc = inc.bad.reserve(sizeof(int) * (size_t)k)) || (rc = inc.tot.reserve(64)) ||
      (rc = inc.cum.reserve(64)))
    return rc;
  if (fresh) {
    CYC_HIP(hipMemsetAsync(inc.prev.ptr, 0xff, sizeof(int32_t) * (size_t)n, st));
    CYC_HIP(hipMemsetAsync(inc.cum.ptr, 0, 16, st));
  }
  const int valid = inc.valid && inc.k == k ? 1 : 0;
  inc.valid = false;   // until this call has completed
  int* gate = (int*)inc.gate.ptr;
  unsigned long long* cum = (unsigned long long*)inc.cum.ptr;
  const unsigned int* cnt = (const unsigned int*)inc.count.ptr;
  {
    cyc::KernelTimer timer("k_kmeans_inc", st);
    hipLaunchKernelGGL(k_inc_moved, dim3((unsigned)nb), dim3(256), 0, st, assign,
                       (int32_t*)inc.prev.ptr, n, (int32_t*)inc.tmpRow.ptr,
                       (int32_t*)inc.tmpOld.ptr, (unsigned int*)inc.bcount.ptr);
    CYC_LAUNCH_CHECK("k_inc_moved");
    hipLaunchKernelGGL(k_inc_scan, dim3(1), dim3(1024), 0, st, (unsigned int*)inc.bcount.ptr,
                       nb, (unsigned int*)inc.count.ptr, valid, mcap, gate, cum);
    CYC_LAUNCH_CHECK("k_inc_scan");
    hipLaunchKernelGGL(k_inc_gather, dim3((unsigned)nb), dim3(256), 0, st,
                       (const int32_t*)inc.tmpRow.ptr, (const int32_t*)inc.tmpOld.ptr,
                       (const unsigned int*)inc.bcount.ptr, assign,
                       (int32_t*)inc.movedRow.ptr, (int32_t*)inc.movedNew.ptr,
                       (int32_t*)inc.movedOld.ptr, (const int*)gate);
    CYC_LAUNCH_CHECK("k_inc_gather");
    with_nj(nj, [&](auto NJ) {
      constexpr int J = decltype(NJ)::value;
      hipLaunchKernelGGL(HIP_KERNEL_NAME(k_inc_part<J>), dim3((unsigned)k, kIncSplit), dim3(256),
                         0, st, X, d, xnorm, (const int32_t*)inc.movedRow.ptr,
                         (const int32_t*)inc.movedNew.ptr, (const int32_t*)inc.movedOld.ptr, cnt,
                         (const double*)inc.P.ptr, (double*)inc.pds.ptr, (double*)inc.psc.ptr,
                         (const int*)gate);
      hipLaunchKernelGGL(HIP_KERNEL_NAME(k_inc_combine<J>), dim3((unsigned)k), dim3(256), 0, st,
                         d, C, (const double*)inc.pds.ptr, (const double*)inc.psc.ptr,
                         (double*)inc.S.ptr, (const double*)inc.P.ptr, (double*)inc.W.ptr,
                         (double*)inc.Q.ptr, (int64_t*)inc.N.ptr, (double*)inc.A.ptr,
                         (double*)inc.ES.ptr, (double*)inc.EQ.ptr, (double*)inc.cost.ptr,
                         (double*)inc.err.ptr, (int*)inc.bad.ptr, (const int*)gate);
    });
    CYC_LAUNCH_CHECK("k_inc_part / k_inc_combine");
    hipLaunchKernelGGL(k_inc_check, dim3(1), dim3(256), 0, st, (const double*)inc.cost.ptr,
                       (const double*)inc.err.ptr, (const int*)inc.bad.ptr, k, gate,
                       (double*)inc.tot.ptr, cum + 1);
    CYC_LAUNCH_CHECK("k_inc_check");
  }
  // the full pass (gate[0]): the counting sort, chunk sums, cluster folds,
  // and the state reset from them
  if ((rc = full_pass(s, X, n, d, k, nullptr, xnorm, false, C, assign, nullptr, sums, wsum,
                      cost_sum, st, gate, &inc)))
    return rc;
  hipLaunchKernelGGL(k_inc_finish, dim3(k), dim3(256), 0, st, C, d, (double*)inc.P.ptr,
                     (const double*)s.ccost.ptr, (const int64_t*)s.total.ptr,
                     (const int64_t*)s.chunkStart.ptr, (double*)inc.Q.ptr,
                     (int64_t*)inc.N.ptr, (const double*)inc.A.ptr, (double*)inc.ES.ptr,
                     (double*)inc.EQ.ptr, (const double*)inc.S.ptr,
                     (const double*)inc.W.ptr, (const double*)inc.tot.ptr, sums, wsum,
                     cost_sum, (const int*)gate);
  CYC_LAUNCH_CHECK("k_inc_finish");
  return CYC_OK;
}

int update_centers(double* C, double* cnorm, const double* sums, const double* wsum, int k, int d,
                   double eps2, int32_t* converged, hipStream_t st) {
  hipLaunchKernelGGL(k_update_centers, dim3((unsigned)k), dim3(64),
                     d <= kUpdLds ? sizeof(double) * 2 * (size_t)d : 0, st, C, cnorm, sums, wsum,
                     k, d, eps2, converged);
  CYC_LAUNCH_CHECK("k_update_centers");
  return CYC_OK;
}

}  // namespace kmsums
}  // namespace cyc
