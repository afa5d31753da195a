// kmeans_i8_lists.hip -- the row lists between the stages of the i8 screen:
// the compaction of the kernels' sharded appends (kmeans_i8.hpp AppendStage)
// and the carried-bounds filter that decides, before a screen, which rows
// keep their assignment, which are re-checked and which are screened
// (kmeans_i8.hpp Bounds; the bounds themselves: the head of kmeans_i8.hip).
#include "kmeans_i8_dev.hpp"

namespace cyc {
namespace km8 {
namespace {

// Sharded appends, compacted (kmeans_i8.hpp) in ONE launch: every block's
// first wave scans the kShards counters (64 values) for its shard's base
// behind *dstCount, the block copies that shard's entries there, and the last
// block to finish (a completion counter in shard 0's spare slot) clears the
// counters and advances *dstCount.  (A scan launch + a copy launch took ~5
// us each, nine pairs per screen call.)
struct CompactJobs {
  CompactJob j[kMaxCompactJobs];
};
__device__ __forceinline__ void shard_compact(const CompactJob& J, unsigned int cap) {
  __shared__ unsigned sb[2];
  const int j = blockIdx.y;
  unsigned int* counts = J.counts;
  if (threadIdx.x < 64) {
    const int l = threadIdx.x;
    const unsigned c = counts[l * kShardStride];
    unsigned incl = c;
#pragma unroll
    for (int m = 1; m < kShards; m <<= 1) {
      const unsigned o = __shfl_up(incl, m);
      if (l >= m) incl += o;
    }
    if (l == j) {
      sb[0] = incl - c;
      sb[1] = c;
    }
  }
  const unsigned old = *J.dstCount;   // advanced only by the last block
  __syncthreads();
  if (J.dst) {
    const size_t base = (size_t)old + sb[0], c = sb[1];
    const size_t t0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const int32_t* s1 = J.src + (size_t)j * cap * J.width;
    int32_t* d1 = J.dst + base * J.width;
    for (size_t i = t0; i < c * J.width; i += stride) d1[i] = s1[i];
    if (J.src2) {
      const int32_t* s2 = J.src2 + (size_t)j * cap * J.width2;
      int32_t* d2 = J.dst2 + base * J.width2;
      for (size_t i = t0; i < c * J.width2; i += stride) d2[i] = s2[i];
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    // no fence: this block's counter and count reads have returned (their
    // values were used above), and the copies reach the next launch at the
    // kernel boundary
    const unsigned blocks = gridDim.x * gridDim.y;
    if (atomicAdd(&counts[3], 1u) == blocks - 1) {
      // every block of this job has read the counters and *dstCount
      unsigned tot = 0;
      for (int l = 0; l < kShards; ++l) {
        tot += counts[l * kShardStride];
        counts[l * kShardStride] = 0u;
      }
      *J.dstCount = old + tot;
      counts[3] = 0u;
    }
  }
}
// Up to kMaxCompactJobs independent compactions (distinct count sets and
// destination counters) share one launch, one per blockIdx.z.
__global__ __launch_bounds__(256) void k_shard_compact(CompactJobs jobs, unsigned int cap) {
  shard_compact(jobs.j[blockIdx.z], cap);
}

}  // namespace

int compact_jobs(const CompactJob* jobs, int nj, unsigned int cap, hipStream_t st) {
  if (nj <= 0) return CYC_OK;
  KernelTimer timer("k_kmeans_compact", st);
  CompactJobs J{};
  bool anyDst = false;
  for (int i = 0; i < nj; ++i) {
    J.j[i] = jobs[i];
    anyDst = anyDst || jobs[i].dst;
  }
  // two blocks per shard: the completion counter's returning atomics
  // serialise (~11 ns each), 16 per shard measured 3x the two launches
  hipLaunchKernelGGL(k_shard_compact, anyDst ? dim3(2, kShards, nj) : dim3(1, 1, nj), dim3(256), 0,
                     st, J, cap);
  CYC_LAUNCH_CHECK("k_shard_compact");
  return CYC_OK;
}

int compact(unsigned int* counts, unsigned int cap, const int32_t* src, int32_t* dst, int width,
            const int32_t* src2, int32_t* dst2, int width2, unsigned int* dstCount,
            hipStream_t st) {
  const CompactJob j{counts, src, dst, width, src2, dst2, width2, dstCount};
  return compact_jobs(&j, 1, cap, st);
}

// ---------------------------------------------------------------------------
// Cross-iteration bounds (kmeans_i8.hpp Bounds).

namespace {

// The listed rows of a kBndRows-row block in row order: tmp[block *
// kBndRows ...], their count in bcount[block] (masks: the wave's ballot of
// `listed` per 256-row step it, wc: IT x 4 counts in LDS)
constexpr int kBndIT = kBndRows / 256;
__device__ __forceinline__ void bnd_block_list(const unsigned long long (&masks)[kBndIT],
                                               unsigned* wc, int64_t base, int32_t* tmp,
                                               unsigned int* bcount,
                                               const unsigned long long* flips = nullptr) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  __syncthreads();
  const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
  for (int it = 0; it < kBndIT; ++it) {
    unsigned before = 0;
    for (int j = 0; j < it * 4 + wave; ++j) before += wc[j];
    if ((masks[it] >> lane) & 1ull)
      tmp[base + before + (unsigned)__builtin_popcountll(masks[it] & below)] =
          (flips && ((flips[it] >> lane) & 1ull)) ? ~(int32_t)(base + it * 256 + tid)
                                                  : (int32_t)(base + it * 256 + tid);
  }
  if (tid == 0) {
    unsigned total = 0;
    for (int j = 0; j < kBndIT * 4; ++j) total += wc[j];
    bcount[blockIdx.x] = total;
  }
}

// kBndRows rows per workgroup (8 per thread, coalesced): a row keeps its
// assignment when its moved bounds still certify it (kmeans_i8.hpp Bounds,
// state 0); else it is re-checked against its carried set when the set's
// moved outside bound still stands (state 2, listed here), else screened
// (state 1).  Every carried bound is moved by the drift.  Round 6: a row
// left for the screen whose center a has a usable neighbourhood (nbrR[a],
// a lower bound of the distance from c_a to every center outside a and its
// kCandMax - 1 nearest, over twice the row's moved upper bound, or no
// bound at all) is re-checked against that neighbourhood instead (state 3,
// listed as ~row).
__global__ __launch_bounds__(256) void k_bounds_filter(const int32_t* __restrict__ assign,
                                                       float2* __restrict__ bnd,
                                                       float* __restrict__ lnc,
                                                       unsigned char* __restrict__ state,
                                                       const double* __restrict__ xnorm,
                                                       int64_t n, int k,
                                                       const double* __restrict__ delta,
                                                       const DriftParams* __restrict__ prm,
                                                       int32_t* __restrict__ tmp,
                                                       unsigned int* __restrict__ bcount,
                                                       const float* __restrict__ nbrR,
                                                       int32_t* __restrict__ tmp2,
                                                       unsigned int* __restrict__ bcount2) {
  __shared__ unsigned wc[kBndIT * 4], wc2[kBndIT * 4];
  unsigned long long masks2[kBndIT];
  const DriftParams P = *prm;
  unsigned long long flips[kBndIT];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t base = (int64_t)blockIdx.x * kBndRows;
  unsigned long long masks[kBndIT];
#pragma unroll
  for (int it = 0; it < kBndIT; ++it) {
    const int64_t r = base + it * 256 + tid;
    int st = 1;
    if (r < n) {
      const int a = assign[r];
      const float2 b = bnd[r];
      const float ln = lnc[r];
      const bool okA = !P.bad && a >= 0 && a < k;
      if (okA && b.x >= 0.0f && b.y > 0.0f) {
        const double U = (double)b.x + delta[a];
        const double L = (double)b.y - (a == P.i1 ? P.d2 : P.d1);
        // |x| <= |x - c_a| + |c_a| <= U + max |c| (no norm read: 80 MB a
        // call at 10M rows)
        const double xr = U + __builtin_sqrt(P.cmax2);
        const double xx = xr * xr * (1.0 + 0x1p-50);
        const double U2 = U * U, L2 = L * L;
        // the reference's rounding slack, plus this test's own rounding
        const double tau = 0x1p-29 * (xx + P.cmax2) + 0x1p-48 * (L2 + U2) + 0x1p-1000;
        if (L > 0.0 && (L2 - U2) > tau) {
          st = 0;
          bnd[r] = make_float2(fup(U * (1.0 + 0x1p-50)), fdown(L * (1.0 - 0x1p-50)));
        }
      }
      // which re-check: a carried set whose moved outside bound still
      // clears the row's moved upper bound (it will most likely certify);
      // else the neighbourhood when nbrR[a] exceeds twice that bound (or
      // the row has none); else a carried set with any margin left.  Both
      // tests only pick the work: the re-check itself decides.
      const double Ln = ln >= 0.0f && okA ? ((double)ln - P.d1) * (1.0 - 0x1p-50) : -1.0;
      const double Um = okA && b.x >= 0.0f ? (double)b.x + delta[a] : 0.0;
      if (st == 1 && Ln > 0.0 && Ln > Um) st = 2;
      if (st == 1 && nbrR && okA) {
        // (a row without a bound: only when its center moved little
        // against its neighbourhood -- early in a fit such rows mostly fail)
        const double R = (double)nbrR[a];
        if (R > 0.0 && R > 2.0 * Um && (b.x >= 0.0f || delta[a] < 0.125 * R)) st = 3;
      }
      if (st == 1 && Ln > 0.0) st = 2;
      if (ln >= 0.0f)   // a carried set (NaN / negative: none) kept while it has a margin
        lnc[r] = (st == 0 || st == 2) && Ln > 0.0 ? fdown(Ln) : -1.0f;
      state[r] = (unsigned char)st;
    }
    masks[it] = __builtin_amdgcn_ballot_w64(st >= 2);
    flips[it] = __builtin_amdgcn_ballot_w64(st == 3);
    masks2[it] = __builtin_amdgcn_ballot_w64(r < n && st == 1);
    if (lane == 0) {
      wc[it * 4 + wave] = (unsigned)__builtin_popcountll(masks[it]);
      wc2[it * 4 + wave] = (unsigned)__builtin_popcountll(masks2[it]);
    }
  }
  bnd_block_list(masks, wc, base, tmp, bcount, flips);
  if (tmp2) bnd_block_list(masks2, wc2, base, tmp2, bcount2);
}

// The rows a full screen takes (state 1), listed as the filter lists its
// re-checks.
__global__ __launch_bounds__(256) void k_bounds_collect(const unsigned char* __restrict__ state,
                                                        int64_t n, int32_t* __restrict__ tmp,
                                                        unsigned int* __restrict__ bcount) {
  __shared__ unsigned wc[kBndIT * 4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t base = (int64_t)blockIdx.x * kBndRows;
  unsigned long long masks[kBndIT];
#pragma unroll
  for (int it = 0; it < kBndIT; ++it) {
    const int64_t r = base + it * 256 + tid;
    masks[it] = __builtin_amdgcn_ballot_w64(r < n && state[r] == 1);
    if (lane == 0) wc[it * 4 + wave] = (unsigned)__builtin_popcountll(masks[it]);
  }
  bnd_block_list(masks, wc, base, tmp, bcount);
}

// Single block: bcount[0..nb) -> exclusive offsets, bcount[nb] = *listCount
// = the total, added to *cum.
__global__ __launch_bounds__(1024) void k_bounds_scan(unsigned int* __restrict__ bcount, int64_t nb,
                                                      unsigned int* __restrict__ listCount,
                                                      unsigned long long* __restrict__ cum,
                                                      unsigned int* __restrict__ bcount2 = nullptr,
                                                      unsigned int* __restrict__ listCount2 = nullptr,
                                                      unsigned long long* __restrict__ cum2 = nullptr) {
  __shared__ unsigned part[1024];
  if (blockIdx.x == 1) {   // the second list of the same blocks
    bcount = bcount2;
    listCount = listCount2;
    cum = cum2;
  }
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
    bcount[nb] = part[1023];
    *listCount = part[1023];
    if (cum) *cum += (unsigned long long)part[1023];
  }
}

__global__ __launch_bounds__(256) void k_bounds_scatter(const int32_t* __restrict__ tmp,
                                                        const unsigned int* __restrict__ off,
                                                        int32_t* __restrict__ list,
                                                        const int32_t* __restrict__ tmp2 = nullptr,
                                                        const unsigned int* __restrict__ off2 = nullptr,
                                                        int32_t* __restrict__ list2 = nullptr) {
  if (blockIdx.y == 1) {
    tmp = tmp2;
    off = off2;
    list = list2;
  }
  const int64_t b = blockIdx.x;
  const unsigned o = off[b], c = off[b + 1] - o;
  for (unsigned i = threadIdx.x; i < c; i += 256) list[o + i] = tmp[b * kBndRows + i];
}

}  // namespace

int bounds_filter(const Bounds& bd, const FilterArgs& fa, hipStream_t st) {
  const int64_t nb = bounds_blocks(bd.n);
  const bool two = fa.tmp2 && fa.bcount2 && bd.list && bd.listCount;
  if (nb <= 0) return CYC_OK;
  KernelTimer timer("k_kmeans_bounds", st);
  int rc;
  if (fa.stats && !fa.nbrsReady &&
      (rc = launch_center_nbrs(fa.stats, fa.k, fa.nbr, fa.nbrR, st)))
    return rc;
  hipLaunchKernelGGL(k_bounds_filter, dim3((unsigned)nb), dim3(256), 0, st, fa.assign, bd.ub_lb,
                     bd.lnc, bd.state, fa.xnorm, bd.n, fa.k, fa.delta, bd.dp, bd.tmp, bd.bcount,
                     fa.stats ? (const float*)fa.nbrR : nullptr, two ? fa.tmp2 : nullptr,
                     two ? fa.bcount2 : nullptr);
  CYC_LAUNCH_CHECK("k_bounds_filter");
  // both lists' scans and scatters as one launch each (block / y index 1:
  // the state-1 list)
  hipLaunchKernelGGL(k_bounds_scan, dim3(two ? 2 : 1), dim3(1024), 0, st, bd.bcount, nb,
                     fa.rcCount, fa.rcCum, two ? fa.bcount2 : nullptr,
                     two ? bd.listCount : nullptr, two ? bd.cum : nullptr);
  CYC_LAUNCH_CHECK("k_bounds_scan");
  hipLaunchKernelGGL(k_bounds_scatter, dim3((unsigned)nb, two ? 2 : 1), dim3(256), 0, st,
                     (const int32_t*)bd.tmp, (const unsigned int*)bd.bcount, fa.rcList,
                     two ? (const int32_t*)fa.tmp2 : nullptr,
                     two ? (const unsigned int*)fa.bcount2 : nullptr, two ? bd.list : nullptr);
  CYC_LAUNCH_CHECK("k_bounds_scatter");
  return CYC_OK;
}

bool recheck_two_phase() {
  static const bool two = [] {
    const char* e = std::getenv("CYC_KMEANS_RECHECK");
    return !(e && e[0] == '1');
  }();
  return two;
}

// After the re-check: the state-1 rows into the screen's list (bd.list).
int bounds_collect(const Bounds& bd, hipStream_t st) {
  const int64_t nb = bounds_blocks(bd.n);
  if (nb <= 0) return CYC_OK;
  hipLaunchKernelGGL(k_bounds_collect, dim3((unsigned)nb), dim3(256), 0, st,
                     (const unsigned char*)bd.state, bd.n, bd.tmp, bd.bcount);
  CYC_LAUNCH_CHECK("k_bounds_collect");
  hipLaunchKernelGGL(k_bounds_scan, dim3(1), dim3(1024), 0, st, bd.bcount, nb, bd.listCount,
                     bd.cum);
  CYC_LAUNCH_CHECK("k_bounds_scan");
  hipLaunchKernelGGL(k_bounds_scatter, dim3((unsigned)nb), dim3(256), 0, st,
                     (const int32_t*)bd.tmp, (const unsigned int*)bd.bcount, bd.list);
  CYC_LAUNCH_CHECK("k_bounds_scatter");
  return CYC_OK;
}

}  // namespace km8
}  // namespace cyc
