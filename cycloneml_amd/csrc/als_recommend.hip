// als_recommend.hip -- ALSModel.recommendForAll / recommendFor*Subset
// (ml/recommendation/ALS.scala, cited from memory) on gfx950 (MI355X): a fused
// score + top-num pass, and the merge of its partial lists.  No score reaches
// HBM; only the lists do.
//
// Contract.  S (rows x rank float32) are the source factors, D (ndst x rank
// float32) the destination factors, each with an optional presence mask.  For
// a requested source row u:
//   score(u, j) = ((0.0f + S[u,0] D[j,0]) + S[u,1] D[j,1]) + ...   fp32, unfused
// (the reference's sgemv("T") per source row through the Java BLAS, and the
// same bits as k_als_predict for the pair).  Absent destinations are never
// candidates.  Candidates are ordered by score descending under
// java.lang.Float.compare (NaN canonical and above everything, -0.0 below
// +0.0) and, where Spark leaves ties to its queue's internals, by the LOWER
// destination id.  That is a total order, written as ONE unsigned 64-bit key:
//   key = sortable(bits(score)) << 32 | ~id      sortable(b) = b ^ (b < 0 ? ~0 : 1 << 31)
// so the answer cannot depend on tiles, splits or merge order.  Key 0 is
// "no candidate" (a real key's high word is at least that of -inf, 0x007fffff).
// Row u of ids / scores holds the first num candidates, then -1 / NaN; a source
// id that is negative, at or past the row count, or absent gives a row of -1 /
// NaN and nothing is gathered through it.
//
// Kernels
//   k_als_score_topk  a workgroup (256 threads) owns kSrcTile = 512 requested
//                     source rows (thread t: rows t and t + 256 of the tile, kept
//                     in registers, rank padded with zeros to RP = the next
//                     multiple of 4: s + 0 * 0 leaves s unchanged, and a sum
//                     that starts from +0 never becomes -0) and one split of the
//                     destination range.  It walks the split in LDS-staged
//                     tiles of dst_tile(RP) = min(128, 2048 / RP) rows, a
//                     multiple of 4 (the next tile's loads are in
//                     flight while this one is scored) and scores 4
//                     destinations x 2 rows at a time: 8 independent chains, each
//                     D value one broadcast LDS read (ds_read_b128, every lane
//                     the same address) shared by both rows.  A float compare
//                     against the row's current num-th score screens the 8
//                     results; only a wave with a hit builds keys.  A row's list
//                     is UNSORTED with its least key and that key's slot kept in
//                     registers: a hit overwrites that slot and rescans the list
//                     for the new least key (independent reads, no shifting).
//                     Lists live in LDS (slot-major, a column per row: no bank
//                     conflict) when num <= kLdsNum and are copied to the
//                     workspace at the end; above that they live in the
//                     workspace itself, in the same layout.
//   k_als_topk_merge  a wave per requested row: over the row's splits x num
//                     keys, num rounds of "the greatest key below the previous
//                     one" (keys are distinct: the id is in them), then the
//                     key is taken apart into id and score.  Also the only
//                     writer of ids / scores, so it runs for one split too.
// The split count and span are fixed functions of (m, ndst) alone
// (rec_shape), never of the device.
//
// Every gather index is checked before use; a tile's rows at or past the
// split's end are staged as zeros with presence 0 and D is never read there.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "common.hpp"

namespace {

typedef unsigned long long u64;

constexpr int kThreads = 256;
constexpr int kSrcTile = 512;          // T: source rows per workgroup (2 per thread)
constexpr int kTileFloats = 2048;      // one staged destination tile (8 KB)
constexpr int kBlockJ = 4;             // destinations scored together
constexpr int kMaxRank = 64;
constexpr int kMaxNum = 128;
constexpr int kLdsNum = 16;            // lists in LDS up to this num (64 KB)
constexpr int64_t kTargetGroups = 1024;   // workgroups a launch aims for (4 per CU)
constexpr int64_t kMinSpan = 256;         // destinations per split, at least
constexpr int kMaxDstTile = 128;       // rows of a tile, at most (below kMinSpan)

inline int padded_rank(int rank) { return (rank + 3) & ~3; }
constexpr int dst_tile(int rp) {
  return std::min(kMaxDstTile, (kTileFloats / rp) & ~(kBlockJ - 1));
}

struct RecShape {
  int64_t tiles, splits, span;
};

// a function of (m, ndst) alone: the same lists, and so the same merge, on
// every device
inline RecShape rec_shape(int64_t m, int64_t ndst) {
  RecShape s;
  s.tiles = std::max<int64_t>(1, (m + kSrcTile - 1) / kSrcTile);
  const int64_t want = (kTargetGroups + s.tiles - 1) / s.tiles;
  const int64_t most = std::max<int64_t>(1, (ndst + kMinSpan - 1) / kMinSpan);
  const int64_t n = std::min(want, most);
  s.span = std::max<int64_t>(kBlockJ, cyc::round_up((ndst + n - 1) / n, kBlockJ));
  s.splits = std::max<int64_t>(1, (ndst + s.span - 1) / s.span);
  return s;
}

struct RecArgs {
  const float* S;
  const uint8_t* sp;
  const int32_t* srcIds;
  const float* D;
  const uint8_t* dp;
  u64* ws;
  int64_t nsrc, m, ndst, span;
  int rank, num, splits, ldsLists;
};

__device__ __forceinline__ float key_score(u64 key) {
  const uint32_t h = (uint32_t)(key >> 32);
  return __uint_as_float(h ^ ((h >> 31) ? 0x80000000u : 0xffffffffu));
}

template <int RP>
__global__ __launch_bounds__(kThreads, 2) void k_als_score_topk(RecArgs p) {
  constexpr int DT = dst_tile(RP);
  constexpr int PT = (DT * RP + kThreads - 1) / kThreads;   // staged values per thread
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* Ds = (float*)smem;
  uint8_t* pres = smem + sizeof(float) * kTileFloats;
  u64* llist = (u64*)(smem + sizeof(float) * kTileFloats + kMaxDstTile);

  const int tid = threadIdx.x, rank = p.rank, num = p.num;
  const int64_t tile = blockIdx.x / p.splits;
  const int split = (int)(blockIdx.x % p.splits);

  // the two source rows of this thread; nothing is gathered through a bad id
  float s[2][RP];
  bool valid[2];
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int64_t r = tile * kSrcTile + tid + q * kThreads;
    int64_t id = -1;
    if (r < p.m) id = p.srcIds ? (int64_t)p.srcIds[r] : r;
    valid[q] = id >= 0 && id < p.nsrc && (!p.sp || p.sp[id]);
#pragma unroll
    for (int f = 0; f < RP; ++f) s[q][f] = (valid[q] && f < rank) ? p.S[id * rank + f] : 0.0f;
  }

  // slot k of row (tid + 256 q) of the tile: list[k * kSrcTile + tid + 256 q]
  u64* wsl = p.ws + (size_t)blockIdx.x * num * kSrcTile;
  u64* list = p.ldsLists ? llist : wsl;
  for (int k = 0; k < num; ++k) {
    list[k * kSrcTile + tid] = 0;
    list[k * kSrcTile + tid + kThreads] = 0;
  }
  u64 least[2] = {0, 0};          // the row's least key (0 while a slot is empty)
  int slot[2] = {0, 0};           // and its slot
  // the screen: a score below this cannot enter.  An invalid row takes nothing.
  float bar[2];
#pragma unroll
  for (int q = 0; q < 2; ++q) bar[q] = valid[q] ? -__builtin_inff() : __builtin_inff();

  const int64_t jbeg = (int64_t)split * p.span;
  const int64_t jend = min(p.ndst, jbeg + p.span);

  float v[PT];
  uint8_t pv = 0;
  auto load = [&](int64_t j0) {
#pragma unroll
    for (int e = 0; e < PT; ++e) {
      const int x = tid + e * kThreads;
      const int64_t j = j0 + x / RP;
      const int col = x % RP;
      v[e] = (x < DT * RP && j < jend && col < rank) ? p.D[j * rank + col] : 0.0f;
    }
    pv = 0;
    if (tid < DT && j0 + tid < jend) pv = p.dp ? p.dp[j0 + tid] : 1;
  };
  if (jbeg < jend) load(jbeg);
  for (int64_t j0 = jbeg; j0 < jend; j0 += DT) {
    __syncthreads();   // the previous tile is read
#pragma unroll
    for (int e = 0; e < PT; ++e) {
      const int x = tid + e * kThreads;
      if (x < DT * RP) Ds[x] = v[e];
    }
    if (tid < DT) pres[tid] = pv;
    __syncthreads();
    if (j0 + DT < jend) load(j0 + DT);
    const int rows = (int)min<int64_t>(DT, jend - j0);
    for (int jl = 0; jl < rows; jl += kBlockJ) {   // rows past the end are zeros, absent
      float acc[2][kBlockJ];
#pragma unroll
      for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int jj = 0; jj < kBlockJ; ++jj) acc[q][jj] = 0.0f;
#pragma unroll
      for (int f = 0; f < RP; f += 4) {
        float4 d[kBlockJ];
#pragma unroll
        for (int jj = 0; jj < kBlockJ; ++jj) d[jj] = *(const float4*)(Ds + (jl + jj) * RP + f);
#pragma unroll
        for (int jj = 0; jj < kBlockJ; ++jj)
#pragma unroll
          for (int q = 0; q < 2; ++q) {
            acc[q][jj] = acc[q][jj] + s[q][f] * d[jj].x;
            acc[q][jj] = acc[q][jj] + s[q][f + 1] * d[jj].y;
            acc[q][jj] = acc[q][jj] + s[q][f + 2] * d[jj].z;
            acc[q][jj] = acc[q][jj] + s[q][f + 3] * d[jj].w;
          }
      }
      bool hit = false;
#pragma unroll
      for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int jj = 0; jj < kBlockJ; ++jj) hit |= !(acc[q][jj] < bar[q]);   // NaN passes
      if (hit) {
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
          for (int jj = 0; jj < kBlockJ; ++jj) {
            const float sc = acc[q][jj];
            uint32_t b = __float_as_uint(sc);
            if (sc != sc) b = 0x7fc00000u;
            const uint32_t h = b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
            const uint32_t j = (uint32_t)(j0 + jl + jj);
            u64 key = ((u64)h << 32) | (uint32_t)~j;
            if (!valid[q] || !pres[jl + jj]) key = 0;
            if (key > least[q]) {
              const int col = tid + q * kThreads;
              list[slot[q] * kSrcTile + col] = key;
              u64 mn = ~0ull;
              int mp = 0;
              for (int k = 0; k < num; ++k) {
                const u64 w = list[k * kSrcTile + col];
                if (w < mn) {
                  mn = w;
                  mp = k;
                }
              }
              least[q] = mn;
              slot[q] = mp;
              bar[q] = mn ? key_score(mn) : -__builtin_inff();
            }
          }
      }
    }
  }
  if (p.ldsLists)
    for (int k = 0; k < num; ++k) {
      wsl[k * kSrcTile + tid] = llist[k * kSrcTile + tid];
      wsl[k * kSrcTile + tid + kThreads] = llist[k * kSrcTile + tid + kThreads];
    }
}

__global__ __launch_bounds__(kThreads) void k_als_topk_merge(const u64* __restrict__ ws,
                                                             int64_t m, int splits, int num,
                                                             int32_t* __restrict__ ids,
                                                             float* __restrict__ scores) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  if (r >= m) return;
  const int64_t tile = r / kSrcTile;
  const int col = (int)(r % kSrcTile);
  const u64* base = ws + (size_t)tile * splits * num * kSrcTile + col;
  const int total = splits * num;   // entry e: split e / num, slot e % num
  u64 prev = ~0ull;
  for (int t = 0; t < num; ++t) {
    u64 best = 0;
    for (int e = lane; e < total; e += 64) {
      const u64 w = base[(size_t)e * kSrcTile];
      if (w < prev && w > best) best = w;
    }
#pragma unroll
    for (int sh = 1; sh < 64; sh <<= 1) {
      const u64 o = __shfl_xor(best, sh);
      best = o > best ? o : best;
    }
    prev = best;
    if (lane == 0) {
      ids[r * num + t] = best ? (int32_t)~(uint32_t)best : -1;
      scores[r * num + t] = best ? key_score(best) : __builtin_nanf("");
    }
  }
}

#define REC_DISPATCH(rp, CALL)                                                          \
  switch (rp) {                                                                         \
    case 4: CALL(4); break;   case 8: CALL(8); break;   case 12: CALL(12); break;       \
    case 16: CALL(16); break; case 20: CALL(20); break; case 24: CALL(24); break;       \
    case 28: CALL(28); break; case 32: CALL(32); break; case 36: CALL(36); break;       \
    case 40: CALL(40); break; case 44: CALL(44); break; case 48: CALL(48); break;       \
    case 52: CALL(52); break; case 56: CALL(56); break; case 60: CALL(60); break;       \
    default: CALL(64); break;                                                           \
  }

int check_shape(int64_t m, int64_t ndst, int32_t rank, int32_t num) {
  CYC_REQUIRE(rank >= 1 && rank <= kMaxRank,
              "ALS supports rank 1 to " + std::to_string(kMaxRank) + " but got " +
                  std::to_string(rank));
  CYC_REQUIRE(num >= 1 && num <= kMaxNum,
              "the number of recommendations must be in [1, " + std::to_string(kMaxNum) +
                  "] but got " + std::to_string(num));
  CYC_REQUIRE(m >= 0 && ndst >= 0, "counts must not be negative");
  CYC_REQUIRE(m <= 0x7fffffff && ndst <= 0x7fffffff, "ids are int32");
  return CYC_OK;
}

}  // namespace

extern "C" {

int cyc_als_recommend_src_tile(void) { return kSrcTile; }

int cyc_als_recommend_dst_tile(int32_t rank) {
  if (rank < 1 || rank > kMaxRank) return 0;
  return dst_tile(padded_rank(rank));
}

int cyc_als_recommend_max_num(void) { return kMaxNum; }

int cyc_als_recommend_lds_num(void) { return kLdsNum; }

int64_t cyc_als_recommend_splits(int64_t m, int64_t ndst) {
  if (m < 0 || ndst < 0) return 0;
  return rec_shape(m, ndst).splits;
}

int64_t cyc_als_recommend_span(int64_t m, int64_t ndst) {
  if (m < 0 || ndst < 0) return 0;
  return rec_shape(m, ndst).span;
}

int64_t cyc_als_recommend_workspace(int64_t m, int64_t ndst, int32_t rank, int32_t num) {
  if (m < 0 || ndst < 0 || rank < 1 || rank > kMaxRank || num < 1 || num > kMaxNum) return 0;
  const RecShape s = rec_shape(m, ndst);
  return (int64_t)sizeof(u64) * s.tiles * s.splits * num * kSrcTile;
}

int cyc_als_recommend_dev(const float* S, const uint8_t* srcPresent, int64_t nsrcRows,
                          const int32_t* srcIds, int64_t m, const float* D,
                          const uint8_t* dstPresent, int64_t ndst, int32_t rank, int32_t num,
                          int32_t* ids, float* scores, void* workspace, int64_t workspaceBytes,
                          void* stream) {
  if (int rc = check_shape(m, ndst, rank, num)) return rc;
  CYC_REQUIRE(nsrcRows >= 0, "counts must not be negative");
  CYC_REQUIRE(srcIds != nullptr || m <= nsrcRows,
              "without srcIds, m must not pass the " + std::to_string(nsrcRows) +
                  " source rows but got " + std::to_string(m));
  const int64_t need = cyc_als_recommend_workspace(m, ndst, rank, num);
  CYC_REQUIRE(workspaceBytes >= need,
              "the workspace must hold " + std::to_string(need) + " bytes but holds " +
                  std::to_string(workspaceBytes));
  if (m == 0) return CYC_OK;
  CYC_REQUIRE(ids != nullptr && scores != nullptr && workspace != nullptr,
              "ids, scores and workspace must not be null");
  CYC_REQUIRE((S != nullptr || nsrcRows == 0) && (D != nullptr || ndst == 0),
              "factors must not be null");
  const RecShape sh = rec_shape(m, ndst);
  CYC_REQUIRE(sh.tiles * sh.splits <= 0x7fffffff, "too many workgroups");
  hipStream_t st = cyc::as_stream(stream);
  RecArgs a{};
  a.S = S;
  a.sp = srcPresent;
  a.srcIds = srcIds;
  a.D = D;
  a.dp = dstPresent;
  a.ws = (u64*)workspace;
  a.nsrc = nsrcRows;
  a.m = m;
  a.ndst = ndst;
  a.span = sh.span;
  a.rank = rank;
  a.num = num;
  a.splits = (int)sh.splits;
  a.ldsLists = num <= kLdsNum ? 1 : 0;
  const size_t lds = sizeof(float) * kTileFloats + kMaxDstTile +
                     (a.ldsLists ? sizeof(u64) * (size_t)num * kSrcTile : 0);
  {
    cyc::KernelTimer timer("k_als_score_topk", st);
#define REC_SCORE(RP)                                                                         \
  do {                                                                                        \
    CYC_HIP(hipFuncSetAttribute((const void*)k_als_score_topk<RP>,                            \
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));       \
    hipLaunchKernelGGL((k_als_score_topk<RP>), dim3((unsigned)(sh.tiles * sh.splits)),        \
                       dim3(kThreads), lds, st, a);                                           \
  } while (0)
    REC_DISPATCH(padded_rank(rank), REC_SCORE);
#undef REC_SCORE
    CYC_LAUNCH_CHECK("k_als_score_topk");
  }
  {
    cyc::KernelTimer timer("k_als_topk_merge", st);
    hipLaunchKernelGGL(k_als_topk_merge, dim3((unsigned)((m + 3) / 4)), dim3(kThreads), 0, st,
                       (const u64*)workspace, m, (int)sh.splits, (int)num, ids, scores);
    CYC_LAUNCH_CHECK("k_als_topk_merge");
  }
  return CYC_OK;
}

}  // extern "C"
