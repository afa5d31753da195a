// lda.hip -- LDA's online variational Bayes E step (mllib/clustering/
// LDAOptimizer.scala's OnlineLDAOptimizer, LDAModel.scala's LocalLDAModel) over
// CSR documents of term counts on gfx950 (MI355X).  The arithmetic is written
// out in include/cyclone.h (cyc_lda_*) and cycloneml_amd/lda.py.
//
// Why no matrix instructions: every document gathers its own rows of B =
// exp(E[log beta])^T (V x k), so the two products of a sweep, phi = B[ids] e
// and B[ids]^T (cts / phi), are gemvs over a slab no other document shares; an
// MFMA tile would need a second operand column that does not exist.  Per sweep
// of a document of nnz words and k topics: 4 nnz k flops (two multiply-adds an
// entry, not fused), nnz divisions, k + 1 digammas and k exps, and 16 nnz k
// bytes of slab read from LDS (tier 1) or from L2 (tier 2); HBM sees the slab
// once per document, 8 nnz k bytes.  The fp64 VALU does 128 flops a clock and
// CU and the LDS serves 128 bytes, so of the two floors the LDS reads are the
// tighter one in tier 1 (4 bytes a flop asked, 1 served); DESIGN.md 5o has
// what was measured.
//
// Layout.  KS = topic stride: the power of two >= k up to 64, then 64
// ceil(k / 64) up to kMaxTopics.  KP = min(KS, 64), T = KS / KP.  Lane =
// (slot, f) = (lane / KP, lane % KP) holds the topics f + KP j, j < T; the 64 /
// KP slots share a document's words.
//
// Prepared documents (cyc_lda_docs_create, once per shard): indices checked,
// counts checked (negative or NaN refused), the column copy of cyc::build_csc
// in one row block with the segment table of the words held by more than kSeg
// documents, and the documents ordered by stored length (ties by id), which
// depends on the data alone and chooses launches only, never a sum's order.
//
// Kernels
//   k_lda_rowsum, k_lda_topics
//                   per topic the sum of lambda's row (thread t's entries in
//                   order, then a fixed tree) and its digamma; then E(lambda)
//                   and B, both V x k with a word's k values contiguous.
//   k_lda_doc<KP, T, SLAB>
//                   one wave (one workgroup) per document.  SLAB (tier 1, a
//                   slab of at most kSlabBytes): B[ids] is gathered once into
//                   LDS (nnz x KS doubles, row w rotated by w columns within
//                   each 64-column block, so that the lane-per-word reads of
//                   phi spread over the banks) and every sweep reads it from
//                   there; the launches are by slab size (eight
//                   classes), each with the LDS its class needs.  !SLAB (tier
//                   2): the rows come from L2 every sweep.  A sweep walks the
//                   words in chunks of 64: lane w forms phi_w = sum_t B[w, t]
//                   e_t (t ascending) + 1e-100 and r_w = cts_w / phi_w, the
//                   chunk's r goes to LDS, then slot s adds B[w, t] r_w for
//                   the words w = s, s + 64 / KP, .. of the chunk, across all
//                   chunks in order.  The slots are added in slot order by
//                   cross-lane moves; sums over topics run j ascending in a
//                   lane, then a fixed xor tree over the KP lanes.
//   k_lda_stat<KP, T>, k_lda_stat_seg<KP, T>, k_lda_fold
//                   over the column copy: a group of KP lanes owns one word of
//                   at most one segment, holds B[v, :], walks the word's
//                   documents in ascending order, recomputes phi_dv from the
//                   final e_d and adds w_d cts_dv / phi_dv e_d; 16 (or 256 /
//                   KP) neighbouring words go through an LDS tile so that
//                   stat (k x V) is written in runs.  A longer word: one
//                   workgroup per segment (wave = quarter, groups added in
//                   group order, waves in wave order), folded in segment order.
//   k_lda_bound<KP, T>
//                   one wave per document: the bound's per-document term.
//   k_lda_runs, k_lda_tail
//                   column sums of a per-document matrix ([w E(gamma) | w] or
//                   the bound's terms): runs of kRunDocs documents in document
//                   order, the runs added in run order.
// The only atomic is the integer atomicMin of the counts' check.  No sum's
// order depends on the grid, the workspace or the call: the same bytes on
// every call.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <mutex>
#include <numeric>
#include <string>
#include <vector>

#include "common.hpp"

struct cyc_lda_docs_s {
  int64_t n = 0, nnz = 0, nseg = 0, nlong = 0;
  int V = 0;
  const int64_t* rowptr = nullptr;   // the caller's CSR, borrowed
  const int32_t* colidx = nullptr;
  const double* vals = nullptr;
  cyc::DeviceBuffer colptr, rowidx, cvals;   // the column copy
  cyc::DeviceBuffer segCol, segStart, longCol, longSeg;
  cyc::DeviceBuffer order;           // document ids by (stored length, id)
  std::vector<int64_t> sortedLen;    // their lengths, ascending
};

struct cyc_lda_plan_s {
  std::mutex mu;
  int k = 0, V = 0;
  bool topics = false;
  cyc::DeviceBuffer B, Elam, psum, part, ws;
};

namespace {

constexpr int kMaxTopics = 256;
constexpr int kSlabBytes = 61440;
constexpr int kClasses = 8;          // tier-1 launches: slabs up to c kSlabBytes / 8
constexpr int kSeg = 256;
constexpr int kRunDocs = 1024;
constexpr int64_t kOneRowBlock = (int64_t)1 << 31;
constexpr unsigned long long kNoBad = 0x7f7f7f7f7f7f7f7full;   // memset(0x7f)

int topic_stride(int k) {
  if (k > 64) return (k + 63) / 64 * 64;
  int p = 1;
  while (p < k) p <<= 1;
  return p;
}

__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
}

// digamma for x > 0 (NaN otherwise): psi(x) = psi(x + m) - sum 1 / (x + i) up
// to x + m >= 10, then ln x - 1 / (2 x) - sum B_2n / (2 n x^2n), n = 1 .. 7; the
// first term left out is below 5e-17 there.  At most ten trips.
__device__ __forceinline__ double lda_digamma(double x) {
  if (!(x > 0.0)) return __builtin_nan("");
  double s = 0.0;
  while (x < 10.0) {
    s += 1.0 / x;
    x += 1.0;
  }
  const double xi = 1.0 / x, x2 = xi * xi;
  const double p =
      x2 * (1.0 / 12 - x2 * (1.0 / 120 - x2 * (1.0 / 252 - x2 * (1.0 / 240 - x2 * (1.0 / 132 -
      x2 * (691.0 / 32760 - x2 * (1.0 / 12)))))));
  return ((log(x) - 0.5 * xi) - p) - s;
}

// the same total in every lane of a group of KP lanes: a fixed xor tree
template <int KP>
__device__ __forceinline__ double group_sum(double s) {
#pragma unroll
  for (int m = KP / 2; m > 0; m >>= 1) s += __shfl_xor(s, m);
  return s;
}

// the slab's element (word w, topic j KP + c)
template <int KP, int T>
__device__ __forceinline__ int slab_at(int w, int j, int c) {
  return w * (KP * T) + j * KP + ((c + w) & (KP - 1));
}

// -------------------------------------------------------------------- topics
__global__ __launch_bounds__(256) void k_lda_rowsum(const double* __restrict__ lam, int64_t V,
                                                    double* __restrict__ psum) {
  __shared__ double sh[256];
  const int tid = threadIdx.x;
  const double* row = lam + (int64_t)blockIdx.x * V;
  double s = 0.0;
  for (int64_t v = tid; v < V; v += 256) s += row[v];
  sh[tid] = s;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (tid < h) sh[tid] += sh[tid + h];
    __syncthreads();
  }
  if (tid == 0) psum[blockIdx.x] = lda_digamma(sh[0]);
}

__global__ __launch_bounds__(256) void k_lda_topics(const double* __restrict__ lam, int64_t V,
                                                    int k, const double* __restrict__ psum,
                                                    double* __restrict__ B,
                                                    double* __restrict__ Elam) {
  const int64_t total = V * k;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * 256) {
    const int64_t v = e / k;
    const int t = (int)(e % k);
    const double el = lda_digamma(lam[t * V + v]) - psum[t];
    Elam[e] = el;
    B[e] = exp(el);
  }
}

__global__ void k_lda_digamma(const double* __restrict__ x, int64_t n, double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = lda_digamma(x[i]);
}

// lowest stored position whose count is negative or NaN
__global__ void k_lda_check_counts(const double* __restrict__ vals, int64_t nnz,
                                   unsigned long long* __restrict__ bad) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nnz;
       i += (int64_t)gridDim.x * blockDim.x)
    if (!(vals[i] >= 0.0)) atomicMin(bad, (unsigned long long)i);
}

// ----------------------------------------------------------------- documents
// E(gamma) and exp(E(gamma)) of this lane's topics; exp(..) also to se[0 .. KS)
template <int KP, int T>
__device__ __forceinline__ void lda_expect(const double (&g)[T], int k, int f, int slot,
                                           double (&el)[T], double (&e)[T], double* se) {
  double s = 0.0;
#pragma unroll
  for (int j = 0; j < T; ++j) s += g[j];   // a lane past k holds zeros
  const double ps = lda_digamma(group_sum<KP>(s));
#pragma unroll
  for (int j = 0; j < T; ++j) {
    const bool on = f + KP * j < k;
    el[j] = on ? lda_digamma(g[j]) - ps : 0.0;
    e[j] = on ? exp(el[j]) : 0.0;
  }
  wave_sync();   // the previous sweep's reads of se
  if (slot == 0) {
#pragma unroll
    for (int j = 0; j < T; ++j) se[j * KP + f] = e[j];
  }
  wave_sync();
}

// LDS: se (KS doubles) | sr (64) | sid (64 ints) | slab (SLAB only)
template <int KP, int T, bool SLAB>
__global__ __launch_bounds__(64) void k_lda_doc(
    const int64_t* __restrict__ rowptr, const int32_t* __restrict__ colidx,
    const double* __restrict__ vals, const int32_t* __restrict__ order, int64_t lo, int64_t hi,
    int k, const double* __restrict__ B, const double* __restrict__ alpha,
    const double* __restrict__ gamma0, const double* __restrict__ weights, int maxInner,
    double* __restrict__ gamma, int32_t* __restrict__ iters, double* __restrict__ ex,
    double* __restrict__ wel) {
  constexpr int KS = KP * T, NS = 64 / KP;
  extern __shared__ double lds[];
  double* se = lds;
  double* sr = se + KS;
  int* sid = (int*)(sr + 64);
  double* slab = sr + 64 + 32;
  const int lane = threadIdx.x, slot = lane / KP, f = lane % KP;
  double al[T];
#pragma unroll
  for (int j = 0; j < T; ++j) al[j] = f + KP * j < k ? alpha[f + KP * j] : 0.0;

  for (int64_t i = lo + blockIdx.x; i < hi; i += gridDim.x) {
    const int64_t d = order[i];
    const int64_t p0 = rowptr[d];
    const int nnz = (int)(rowptr[d + 1] - p0);
    const double wd = weights ? weights[d] : 1.0;
    int some = 0;
    if (wd != 0.0)
      for (int w = lane; w < nnz; w += 64) some |= vals[p0 + w] != 0.0;
    const bool run = __any(some) != 0;

    double g[T], el[T], e[T];
    int it = 0;
#pragma unroll
    for (int j = 0; j < T; ++j) g[j] = el[j] = e[j] = 0.0;
    if (run) {
      if constexpr (SLAB) {
        wave_sync();   // the previous document's reads of the slab
        for (int w = slot; w < nnz; w += NS) {
          const double* b = B + (int64_t)colidx[p0 + w] * k;
#pragma unroll
          for (int j = 0; j < T; ++j)
            slab[slab_at<KP, T>(w, j, f)] = f + KP * j < k ? b[f + KP * j] : 0.0;
        }
      }
#pragma unroll
      for (int j = 0; j < T; ++j) g[j] = f + KP * j < k ? gamma0[d * k + f + KP * j] : 0.0;
      lda_expect<KP, T>(g, k, f, slot, el, e, se);   // its barrier publishes the slab too
      for (;;) {
        double acc[T];
#pragma unroll
        for (int j = 0; j < T; ++j) acc[j] = 0.0;
        for (int c0 = 0; c0 < nnz; c0 += 64) {
          const int cnt = min(64, nnz - c0);
          double r = 0.0;
          int id = 0;
          if (lane < cnt) {
            const int w = c0 + lane;
            double phi = 0.0;
            if constexpr (SLAB) {
              const double* row = slab + w * KS;
#pragma unroll 4
              for (int t = 0; t < k; ++t)
                phi += row[(t & ~(KP - 1)) + ((t + w) & (KP - 1))] * se[t];
            } else {
              id = colidx[p0 + w];
              const double* b = B + (int64_t)id * k;
#pragma unroll 4
              for (int t = 0; t < k; ++t) phi += b[t] * se[t];
            }
            phi += 1e-100;
            r = vals[p0 + w] / phi;
          }
          wave_sync();   // the previous chunk's reads of sr and sid
          sr[lane] = r;
          if constexpr (!SLAB) sid[lane] = id;
          wave_sync();
          for (int wi = slot; wi < cnt; wi += NS) {
            const double rr = sr[wi];
            if constexpr (SLAB) {
#pragma unroll
              for (int j = 0; j < T; ++j) acc[j] += slab[slab_at<KP, T>(c0 + wi, j, f)] * rr;
            } else {
              const double* b = B + (int64_t)sid[wi] * k;
#pragma unroll
              for (int j = 0; j < T; ++j)
                if (f + KP * j < k) acc[j] += b[f + KP * j] * rr;
            }
          }
        }
        double diff = 0.0;
#pragma unroll
        for (int j = 0; j < T; ++j) {
          // the slots in slot order; every slot ends with the same total
          double a = __shfl(acc[j], f);
#pragma nounroll
          for (int sl = 1; sl < NS; ++sl) a += __shfl(acc[j], sl * KP + f);
          const double last = g[j];
          g[j] = f + KP * j < k ? e[j] * a + al[j] : 0.0;
          diff += fabs(g[j] - last);
        }
        const double change = group_sum<KP>(diff) / (double)k;
        lda_expect<KP, T>(g, k, f, slot, el, e, se);
        ++it;
        if (!(change > 1e-3) || it >= maxInner) break;
      }
    }
    // an empty or weight-0 document: zeros and no sweep
    if (slot == 0) {
#pragma unroll
      for (int j = 0; j < T; ++j) {
        const int t = f + KP * j;
        if (t < k) {
          gamma[d * k + t] = g[j];
          if (ex) ex[d * k + t] = e[j];
          if (wel) wel[d * (k + 1) + t] = run ? wd * el[j] : 0.0;
        }
      }
    }
    if (lane == 0) {
      if (iters) iters[d] = it;
      if (wel) wel[d * (k + 1) + k] = run ? wd : 0.0;
    }
  }
}

// ---------------------------------------------------------------- statistics
// The entries q0, q0 + step, .. < q1 of the column copy in order: acc_t += w_d
// cts / phi e_dt with phi recomputed from the final e_d and this word's B row.
template <int KP, int T>
__device__ __forceinline__ void lda_walk(const int32_t* __restrict__ rowidx,
                                         const double* __restrict__ cvals, int64_t q0, int64_t q1,
                                         int step, int k, int f, const double* __restrict__ ex,
                                         const double* __restrict__ weights,
                                         const double (&bv)[T], double (&acc)[T]) {
  for (int64_t q = q0; q < q1; q += step) {
    const double c = cvals[q];
    const int64_t d = rowidx[q];
    const double wd = weights ? weights[d] : 1.0;
    if (c == 0.0 || wd == 0.0) continue;   // the same for the whole group
    double e[T], p = 0.0;
#pragma unroll
    for (int j = 0; j < T; ++j) {
      e[j] = f + KP * j < k ? ex[d * k + f + KP * j] : 0.0;
      p += bv[j] * e[j];
    }
    const double coef = wd * c / (group_sum<KP>(p) + 1e-100);
#pragma unroll
    for (int j = 0; j < T; ++j) acc[j] += coef * e[j];
  }
}

template <int KP, int T>
__global__ __launch_bounds__(256) void k_lda_stat(
    const int64_t* __restrict__ colptr, const int32_t* __restrict__ rowidx,
    const double* __restrict__ cvals, int64_t V, int k, const double* __restrict__ B,
    const double* __restrict__ ex, const double* __restrict__ weights, double* __restrict__ stat) {
  constexpr int KS = KP * T, NGB = 256 / KP, TW = NGB > 16 ? NGB : 16;
  __shared__ double tile[KS * TW];
  const int g = threadIdx.x / KP, f = threadIdx.x % KP;
  for (int64_t v0 = (int64_t)blockIdx.x * TW; v0 < V; v0 += (int64_t)gridDim.x * TW) {
    __syncthreads();   // the previous tile is written out
    for (int wi = g; wi < TW; wi += NGB) {
      const int64_t v = v0 + wi;
      if (v >= V) continue;
      const int64_t q0 = colptr[v], q1 = colptr[v + 1];
      if (q1 - q0 > kSeg) continue;   // k_lda_stat_seg and k_lda_fold own it
      double bv[T], acc[T];
#pragma unroll
      for (int j = 0; j < T; ++j) {
        bv[j] = f + KP * j < k ? B[v * k + f + KP * j] : 0.0;
        acc[j] = 0.0;
      }
      lda_walk<KP, T>(rowidx, cvals, q0, q1, 1, k, f, ex, weights, bv, acc);
#pragma unroll
      for (int j = 0; j < T; ++j)
        if (f + KP * j < k) tile[(f + KP * j) * TW + wi] = bv[j] * acc[j];
    }
    __syncthreads();
    for (int e = threadIdx.x; e < k * TW; e += 256) {
      const int64_t v = v0 + e % TW;
      if (v < V && colptr[v + 1] - colptr[v] <= kSeg) stat[(int64_t)(e / TW) * V + v] = tile[e];
    }
  }
}

template <int KP, int T>
__global__ __launch_bounds__(256) void k_lda_stat_seg(
    const int32_t* __restrict__ segCol, const int64_t* __restrict__ segStart,
    const int64_t* __restrict__ colptr, const int32_t* __restrict__ rowidx,
    const double* __restrict__ cvals, int k, const double* __restrict__ B,
    const double* __restrict__ ex, const double* __restrict__ weights,
    double* __restrict__ segPart) {
  constexpr int NG = 64 / KP, QUARTER = kSeg / 4;
  __shared__ double red[4][kMaxTopics];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane / KP, f = lane % KP;
  const int64_t seg = blockIdx.x, v = segCol[seg];
  const int64_t s0 = segStart[seg], s1 = min(s0 + kSeg, colptr[v + 1]);
  const int64_t q0 = min(s0 + wave * QUARTER, s1), q1 = min(q0 + QUARTER, s1);
  double bv[T], acc[T];
#pragma unroll
  for (int j = 0; j < T; ++j) {
    bv[j] = f + KP * j < k ? B[v * k + f + KP * j] : 0.0;
    acc[j] = 0.0;
  }
  lda_walk<KP, T>(rowidx, cvals, q0 + g, q1, NG, k, f, ex, weights, bv, acc);
#pragma unroll
  for (int j = 0; j < T; ++j) {
    double a = __shfl(acc[j], f);
#pragma nounroll
    for (int gg = 1; gg < NG; ++gg) a += __shfl(acc[j], gg * KP + f);
    if (g == 0 && f + KP * j < k) red[wave][f + KP * j] = a;
  }
  __syncthreads();
  for (int t = threadIdx.x; t < k; t += 256)
    segPart[seg * k + t] = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
}

// thread (long word c, topic t): its partials in segment order
__global__ __launch_bounds__(256) void k_lda_fold(
    const int32_t* __restrict__ longCol, const int64_t* __restrict__ longSeg, int64_t nlong,
    int64_t V, int k, const double* __restrict__ segPart, const double* __restrict__ B,
    double* __restrict__ stat) {
  const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t c = id / k;
  const int t = (int)(id % k);
  if (c >= nlong) return;
  const int64_t v = longCol[c];
  double a = 0.0;
  for (int64_t s = longSeg[c]; s < longSeg[c + 1]; ++s) a += segPart[s * k + t];
  stat[t * V + v] = B[v * k + t] * a;
}

// --------------------------------------------------------------------- bound
template <int KP, int T>
__global__ __launch_bounds__(64) void k_lda_bound(
    const int64_t* __restrict__ rowptr, const int32_t* __restrict__ colidx,
    const double* __restrict__ vals, int64_t n, int k, const double* __restrict__ Elam,
    const double* __restrict__ alpha, const double* __restrict__ gamma,
    const double* __restrict__ weights, double* __restrict__ docPart) {
  __shared__ double se[KP * T];
  const int lane = threadIdx.x, f = lane % KP;
  double al[T], sa = 0.0;
#pragma unroll
  for (int j = 0; j < T; ++j) {
    al[j] = f + KP * j < k ? alpha[f + KP * j] : 0.0;
    sa += al[j];
  }
  const double lgSumAlpha = lgamma(group_sum<KP>(sa));
  for (int64_t d = blockIdx.x; d < n; d += gridDim.x) {
    const int64_t p0 = rowptr[d];
    const int nnz = (int)(rowptr[d + 1] - p0);
    const double wd = weights ? weights[d] : 1.0;
    int some = 0;
    if (wd != 0.0)
      for (int w = lane; w < nnz; w += 64) some |= vals[p0 + w] != 0.0;
    if (!__any(some)) {   // an empty or weight-0 document
      if (lane == 0) docPart[d] = 0.0;
      continue;
    }
    double g[T], el[T], e[T], tt = 0.0, sg = 0.0;
#pragma unroll
    for (int j = 0; j < T; ++j) {
      g[j] = f + KP * j < k ? gamma[d * k + f + KP * j] : 0.0;
      sg += g[j];
    }
    lda_expect<KP, T>(g, k, f, lane / KP, el, e, se);
    wave_sync();   // every lane has left the last document's reads of se
    if (lane < KP) {
#pragma unroll
      for (int j = 0; j < T; ++j) se[j * KP + f] = el[j];
    }
    wave_sync();
#pragma unroll
    for (int j = 0; j < T; ++j)
      if (f + KP * j < k) tt += (al[j] - g[j]) * el[j] + (lgamma(g[j]) - lgamma(al[j]));
    tt = group_sum<KP>(tt);
    sg = group_sum<KP>(sg);
    double ws = 0.0;
    for (int w = lane; w < nnz; w += 64) {
      const double c = vals[p0 + w];
      if (c == 0.0) continue;
      const double* row = Elam + (int64_t)colidx[p0 + w] * k;
      double m = se[0] + row[0];
      for (int t = 1; t < k; ++t) m = fmax(m, se[t] + row[t]);
      double s = 0.0;
      for (int t = 0; t < k; ++t) s += exp((se[t] + row[t]) - m);
      ws += c * (m + log(s));
    }
    ws = group_sum<64>(ws);
    if (lane == 0) docPart[d] = wd * (((ws + tt) + lgSumAlpha) - lgamma(sg));
  }
}

// ---------------------------------------------------------------- reductions
// run blockIdx.x, thread q < m: column q of M (n x m) over the run's documents
__global__ __launch_bounds__(320) void k_lda_runs(const double* __restrict__ M, int64_t n, int m,
                                                  double* __restrict__ runPart) {
  const int q = threadIdx.x;
  if (q >= m) return;
  const int64_t R0 = (int64_t)blockIdx.x * kRunDocs, R1 = min(n, R0 + kRunDocs);
  double s = 0.0;
  for (int64_t d = R0; d < R1; ++d) s += M[d * m + q];
  runPart[(int64_t)blockIdx.x * m + q] = s;
}

// the runs in run order
__global__ __launch_bounds__(320) void k_lda_tail(const double* __restrict__ runPart,
                                                  int64_t runs, int m, double* __restrict__ out) {
  const int q = threadIdx.x;
  if (q >= m) return;
  double s = 0.0;
  for (int64_t r = 0; r < runs; ++r) s += runPart[r * m + q];
  out[q] = s;
}

#define CYC_LDA_KP(k_, CALL)                                          \
  if (k_ <= 1) { constexpr int KP = 1, T = 1; CALL; }                 \
  else if (k_ <= 2) { constexpr int KP = 2, T = 1; CALL; }            \
  else if (k_ <= 4) { constexpr int KP = 4, T = 1; CALL; }            \
  else if (k_ <= 8) { constexpr int KP = 8, T = 1; CALL; }            \
  else if (k_ <= 16) { constexpr int KP = 16, T = 1; CALL; }          \
  else if (k_ <= 32) { constexpr int KP = 32, T = 1; CALL; }          \
  else if (k_ <= 64) { constexpr int KP = 64, T = 1; CALL; }          \
  else if (k_ <= 128) { constexpr int KP = 64, T = 2; CALL; }         \
  else if (k_ <= 192) { constexpr int KP = 64, T = 3; CALL; }         \
  else { constexpr int KP = 64, T = 4; CALL; }

int upload(cyc::DeviceBuffer& buf, const void* src, size_t bytes) {
  if (int rc = buf.reserve(std::max<size_t>(bytes, 8))) return rc;
  if (bytes) CYC_HIP(hipMemcpy(buf.ptr, src, bytes, hipMemcpyHostToDevice));
  return CYC_OK;
}

// the counts' check, the length order and the segment table of the long words
int prepare_docs(cyc_lda_docs_s* r, hipStream_t st) {
  std::vector<int64_t> rowptr((size_t)r->n + 1, 0);
  CYC_HIP(hipStreamSynchronize(st));
  CYC_HIP(hipMemcpy(rowptr.data(), r->rowptr, sizeof(int64_t) * rowptr.size(),
                    hipMemcpyDeviceToHost));
  r->nnz = rowptr[(size_t)r->n];
  if (r->nnz > 0) {
    cyc::DeviceBuffer bad;
    if (int rc = bad.reserve(sizeof(unsigned long long))) return rc;
    CYC_HIP(hipMemsetAsync(bad.ptr, 0x7f, sizeof(unsigned long long), st));
    const int64_t grid = std::min<int64_t>((r->nnz + 255) / 256, 64 * (int64_t)cyc::device_cus());
    hipLaunchKernelGGL(k_lda_check_counts, dim3((unsigned)grid), dim3(256), 0, st, r->vals, r->nnz,
                       (unsigned long long*)bad.ptr);
    CYC_LAUNCH_CHECK("k_lda_check_counts");
    unsigned long long at = kNoBad;
    CYC_HIP(hipMemcpyAsync(&at, bad.ptr, sizeof(at), hipMemcpyDeviceToHost, st));
    CYC_HIP(hipStreamSynchronize(st));
    CYC_REQUIRE(at == kNoBad, "term counts must be non-negative numbers but stored entry " +
                                  std::to_string(at) + " is not");
  }
  std::vector<int32_t> order((size_t)r->n);
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) {
    return rowptr[a + 1] - rowptr[a] < rowptr[b + 1] - rowptr[b];
  });
  r->sortedLen.resize((size_t)r->n);
  for (int64_t i = 0; i < r->n; ++i)
    r->sortedLen[i] = rowptr[order[i] + 1] - rowptr[order[i]];
  if (int rc = upload(r->order, order.data(), sizeof(int32_t) * order.size())) return rc;

  std::vector<int64_t> colptr((size_t)r->V + 1);
  CYC_HIP(hipMemcpy(colptr.data(), r->colptr.ptr, sizeof(int64_t) * colptr.size(),
                    hipMemcpyDeviceToHost));
  std::vector<int32_t> segCol, longCol;
  std::vector<int64_t> segStart, longSeg;
  for (int v = 0; v < r->V; ++v) {
    if (colptr[v + 1] - colptr[v] <= kSeg) continue;
    longCol.push_back(v);
    longSeg.push_back((int64_t)segCol.size());
    for (int64_t q = colptr[v]; q < colptr[v + 1]; q += kSeg) {
      segCol.push_back(v);
      segStart.push_back(q);
    }
  }
  longSeg.push_back((int64_t)segCol.size());
  r->nseg = (int64_t)segCol.size();
  r->nlong = (int64_t)longCol.size();
  int rc;
  if ((rc = upload(r->segCol, segCol.data(), sizeof(int32_t) * segCol.size())) ||
      (rc = upload(r->segStart, segStart.data(), sizeof(int64_t) * segStart.size())) ||
      (rc = upload(r->longCol, longCol.data(), sizeof(int32_t) * longCol.size())) ||
      (rc = upload(r->longSeg, longSeg.data(), sizeof(int64_t) * longSeg.size())))
    return rc;
  return CYC_OK;
}

int check_call(const cyc_lda_plan_s* p, const cyc_lda_docs_s* r) {
  CYC_REQUIRE(p != nullptr && r != nullptr, "plan and docs must not be null");
  CYC_REQUIRE(p->topics, "cyc_lda_set_topics_dev must come first");
  CYC_REQUIRE(r->V == p->V, "the documents have a vocabulary of " + std::to_string(r->V) +
                                " but the plan has " + std::to_string(p->V));
  return CYC_OK;
}

// the document kernel over every length class, then tier 2
int launch_docs(const cyc_lda_plan_s* p, const cyc_lda_docs_s* r, const double* alpha,
                const double* gamma0, const double* weights, int maxInner, double* gamma,
                int32_t* iters, double* ex, double* wel, hipStream_t st) {
  const int k = p->k, KS = topic_stride(k);
  const size_t fixed = sizeof(double) * (size_t)(KS + 64 + 32);
  const int64_t maxGrid = 32 * (int64_t)cyc::device_cus();
  const auto* order = (const int32_t*)r->order.ptr;
  const auto* B = (const double*)p->B.ptr;
  cyc::KernelTimer timer("k_lda_doc", st);
  int64_t lo = 0;
  for (int c = 1; c <= kClasses + 1 && lo < r->n; ++c) {
    const bool slab = c <= kClasses;
    const int64_t bytes = (int64_t)kSlabBytes / kClasses * c;
    const int64_t hi = slab ? std::upper_bound(r->sortedLen.begin(), r->sortedLen.end(),
                                               bytes / (8 * KS)) - r->sortedLen.begin()
                            : r->n;
    if (hi == lo) continue;
    const dim3 grid((unsigned)std::min<int64_t>(hi - lo, maxGrid));
    if (slab) {
      CYC_LDA_KP(k, hipLaunchKernelGGL((k_lda_doc<KP, T, true>), grid, dim3(64),
                                       fixed + (size_t)bytes, st, r->rowptr, r->colidx, r->vals,
                                       order, lo, hi, k, B, alpha, gamma0, weights, maxInner,
                                       gamma, iters, ex, wel));
    } else {
      CYC_LDA_KP(k, hipLaunchKernelGGL((k_lda_doc<KP, T, false>), grid, dim3(64), fixed, st,
                                       r->rowptr, r->colidx, r->vals, order, lo, hi, k, B, alpha,
                                       gamma0, weights, maxInner, gamma, iters, ex, wel));
    }
    CYC_LAUNCH_CHECK("k_lda_doc");
    lo = hi;
  }
  return CYC_OK;
}

// out[0 .. m) = the column sums of M (n x m) by runs
int launch_runs(const double* M, int64_t n, int m, double* runPart, double* out, hipStream_t st) {
  const int64_t runs = (n + kRunDocs - 1) / kRunDocs;
  if (runs > 0) {
    hipLaunchKernelGGL(k_lda_runs, dim3((unsigned)runs), dim3(320), 0, st, M, n, m, runPart);
    CYC_LAUNCH_CHECK("k_lda_runs");
  }
  hipLaunchKernelGGL(k_lda_tail, dim3(1), dim3(320), 0, st, runPart, runs, m, out);
  CYC_LAUNCH_CHECK("k_lda_tail");
  return CYC_OK;
}

}  // namespace

extern "C" {

int cyc_lda_max_topics(void) { return kMaxTopics; }
int cyc_lda_slab_bytes(void) { return kSlabBytes; }
int cyc_lda_segment_entries(void) { return kSeg; }
int cyc_lda_run_docs(void) { return kRunDocs; }
int cyc_lda_topic_stride(int32_t k) { return k >= 1 && k <= kMaxTopics ? topic_stride(k) : 0; }

int cyc_lda_docs_create(const int64_t* rowptr, const int32_t* colidx, const double* counts,
                        int64_t ndocs, int32_t vocabSize, void* stream, cyc_lda_docs* docs) {
  CYC_REQUIRE(docs != nullptr && rowptr != nullptr, "output handle and rowptr must not be null");
  CYC_REQUIRE(ndocs >= 0 && ndocs < kOneRowBlock, "0 <= ndocs < 2^31");
  CYC_REQUIRE(vocabSize >= 1, "vocabSize >= 1");
  hipStream_t st = cyc::as_stream(stream);
  if (int rc = cyc::check_csr_indices(rowptr, colidx, ndocs, vocabSize, st)) return rc;
  auto* r = new cyc_lda_docs_s();
  r->n = ndocs;
  r->V = vocabSize;
  r->rowptr = rowptr;
  r->colidx = colidx;
  r->vals = counts;
  int rc = cyc::build_csc(rowptr, colidx, counts, ndocs, vocabSize, kOneRowBlock, r->colptr,
                          r->rowidx, r->cvals, st);
  if (!rc) rc = prepare_docs(r, st);
  if (rc) {
    delete r;
    return rc;
  }
  *docs = r;
  return CYC_OK;
}

int cyc_lda_docs_destroy(cyc_lda_docs docs) {
  delete docs;
  return CYC_OK;
}

int cyc_lda_plan_create(int32_t k, int32_t vocabSize, cyc_lda_plan* plan) {
  CYC_REQUIRE(plan != nullptr, "output handle must not be null");
  CYC_REQUIRE(k >= 1 && k <= kMaxTopics, "k must be in [1, " + std::to_string(kMaxTopics) +
                                             "] but got " + std::to_string(k));
  CYC_REQUIRE(vocabSize >= 1, "vocabSize >= 1");
  auto* p = new cyc_lda_plan_s();
  p->k = k;
  p->V = vocabSize;
  *plan = p;
  return CYC_OK;
}

int cyc_lda_plan_destroy(cyc_lda_plan plan) {
  delete plan;
  return CYC_OK;
}

int cyc_lda_set_topics_dev(cyc_lda_plan plan, const double* lambda, void* stream) {
  CYC_REQUIRE(plan != nullptr && lambda != nullptr, "plan and lambda must not be null");
  cyc_lda_plan_s* p = plan;
  hipStream_t st = cyc::as_stream(stream);
  std::lock_guard<std::mutex> guard(p->mu);
  const int64_t total = (int64_t)p->V * p->k;
  int rc;
  if ((rc = p->B.reserve(sizeof(double) * (size_t)total)) ||
      (rc = p->Elam.reserve(sizeof(double) * (size_t)total)) ||
      (rc = p->psum.reserve(sizeof(double) * (size_t)p->k)))
    return rc;
  cyc::KernelTimer timer("k_lda_topics", st);
  hipLaunchKernelGGL(k_lda_rowsum, dim3((unsigned)p->k), dim3(256), 0, st, lambda, (int64_t)p->V,
                     (double*)p->psum.ptr);
  CYC_LAUNCH_CHECK("k_lda_rowsum");
  const int64_t grid = std::min<int64_t>((total + 255) / 256, 64 * (int64_t)cyc::device_cus());
  hipLaunchKernelGGL(k_lda_topics, dim3((unsigned)grid), dim3(256), 0, st, lambda, (int64_t)p->V,
                     p->k, (const double*)p->psum.ptr, (double*)p->B.ptr, (double*)p->Elam.ptr);
  CYC_LAUNCH_CHECK("k_lda_topics");
  p->topics = true;
  return CYC_OK;
}

int cyc_lda_infer_dev(cyc_lda_plan plan, cyc_lda_docs docs, const double* alpha,
                      const double* gamma0, const double* weights, int32_t maxInner,
                      double* gamma, int32_t* iters, void* stream) {
  if (int rc = check_call(plan, docs)) return rc;
  CYC_REQUIRE(maxInner >= 1, "maxInner must be at least 1 but got " + std::to_string(maxInner));
  CYC_REQUIRE(alpha != nullptr, "alpha must not be null");
  if (docs->n == 0) return CYC_OK;
  CYC_REQUIRE(gamma0 != nullptr && gamma != nullptr, "gamma0 and gamma must not be null");
  std::lock_guard<std::mutex> guard(plan->mu);
  return launch_docs(plan, docs, alpha, gamma0, weights, maxInner, gamma, iters, nullptr, nullptr,
                     cyc::as_stream(stream));
}

int cyc_lda_estep_dev(cyc_lda_plan plan, cyc_lda_docs docs, const double* alpha,
                      const double* gamma0, const double* weights, int32_t maxInner,
                      double* gamma, int32_t* iters, double* out, void* stream) {
  if (int rc = check_call(plan, docs)) return rc;
  CYC_REQUIRE(maxInner >= 1, "maxInner must be at least 1 but got " + std::to_string(maxInner));
  CYC_REQUIRE(alpha != nullptr && out != nullptr, "alpha and out must not be null");
  cyc_lda_plan_s* p = plan;
  const cyc_lda_docs_s* r = docs;
  CYC_REQUIRE(r->n == 0 || gamma0 != nullptr, "gamma0 must not be null");
  hipStream_t st = cyc::as_stream(stream);
  std::lock_guard<std::mutex> guard(p->mu);
  const int k = p->k;
  const int64_t n = r->n, V = p->V, runs = (n + kRunDocs - 1) / kRunDocs;
  // gamma (n x k, when the caller wants none) | ex (n x k) | wel (n x (k + 1))
  // | runPart (runs x (k + 1)) | segPart (nseg x k)
  const int64_t words = n * (3 * (int64_t)k + 1) + runs * (k + 1) + r->nseg * k;
  if (int rc = p->ws.reserve(sizeof(double) * (size_t)std::max<int64_t>(words, 1))) return rc;
  double* gws = (double*)p->ws.ptr;
  double* ex = gws + n * k;
  double* wel = ex + n * k;
  double* runPart = wel + n * (k + 1);
  double* segPart = runPart + runs * (k + 1);
  if (n > 0)
    if (int rc = launch_docs(p, r, alpha, gamma0, weights, maxInner, gamma ? gamma : gws, iters,
                             ex, wel, st))
      return rc;
  const auto* B = (const double*)p->B.ptr;
  {
    cyc::KernelTimer timer("k_lda_stat", st);
    CYC_LDA_KP(k, {
      constexpr int TW = 256 / KP > 16 ? 256 / KP : 16;
      const int64_t grid = std::min<int64_t>((V + TW - 1) / TW, 64 * (int64_t)cyc::device_cus());
      hipLaunchKernelGGL((k_lda_stat<KP, T>), dim3((unsigned)grid), dim3(256), 0, st,
                         (const int64_t*)r->colptr.ptr, (const int32_t*)r->rowidx.ptr,
                         (const double*)r->cvals.ptr, V, k, B, ex, weights, out);
    });
    CYC_LAUNCH_CHECK("k_lda_stat");
  }
  if (r->nseg > 0) {
    cyc::KernelTimer timer("k_lda_stat_seg", st);
    CYC_LDA_KP(k, hipLaunchKernelGGL((k_lda_stat_seg<KP, T>), dim3((unsigned)r->nseg), dim3(256),
                                     0, st, (const int32_t*)r->segCol.ptr,
                                     (const int64_t*)r->segStart.ptr,
                                     (const int64_t*)r->colptr.ptr, (const int32_t*)r->rowidx.ptr,
                                     (const double*)r->cvals.ptr, k, B, ex, weights, segPart));
    CYC_LAUNCH_CHECK("k_lda_stat_seg");
    hipLaunchKernelGGL(k_lda_fold, dim3((unsigned)((r->nlong * k + 255) / 256)), dim3(256), 0, st,
                       (const int32_t*)r->longCol.ptr, (const int64_t*)r->longSeg.ptr, r->nlong,
                       V, k, segPart, B, out);
    CYC_LAUNCH_CHECK("k_lda_fold");
  }
  return launch_runs(wel, n, k + 1, runPart, out + V * k, st);
}

int cyc_lda_bound_dev(cyc_lda_plan plan, cyc_lda_docs docs, const double* alpha,
                      const double* gamma, const double* weights, double* out, void* stream) {
  if (int rc = check_call(plan, docs)) return rc;
  CYC_REQUIRE(alpha != nullptr && out != nullptr, "alpha and out must not be null");
  cyc_lda_plan_s* p = plan;
  const cyc_lda_docs_s* r = docs;
  CYC_REQUIRE(r->n == 0 || gamma != nullptr, "gamma must not be null");
  hipStream_t st = cyc::as_stream(stream);
  std::lock_guard<std::mutex> guard(p->mu);
  const int64_t n = r->n, runs = (n + kRunDocs - 1) / kRunDocs;
  if (int rc = p->part.reserve(sizeof(double) * (size_t)std::max<int64_t>(n + runs, 1))) return rc;
  double* docPart = (double*)p->part.ptr;
  if (n > 0) {
    cyc::KernelTimer timer("k_lda_bound", st);
    const dim3 grid((unsigned)std::min<int64_t>(n, 32 * (int64_t)cyc::device_cus()));
    CYC_LDA_KP(p->k, hipLaunchKernelGGL((k_lda_bound<KP, T>), grid, dim3(64), 0, st, r->rowptr,
                                        r->colidx, r->vals, n, p->k, (const double*)p->Elam.ptr,
                                        alpha, gamma, weights, docPart));
    CYC_LAUNCH_CHECK("k_lda_bound");
  }
  return launch_runs(docPart, n, 1, docPart + n, out, st);
}

int cyc_lda_digamma_dev(const double* x, int64_t n, double* out, void* stream) {
  CYC_REQUIRE(n >= 0 && (n == 0 || (x != nullptr && out != nullptr)), "n >= 0 and non-null arrays");
  if (n == 0) return CYC_OK;
  hipLaunchKernelGGL(k_lda_digamma, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                     cyc::as_stream(stream), x, n, out);
  CYC_LAUNCH_CHECK("k_lda_digamma");
  return CYC_OK;
}

}  // extern "C"
