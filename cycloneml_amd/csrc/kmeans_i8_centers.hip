// kmeans_i8_centers.hip -- everything the i8 screen derives from the k x d
// centers alone: the center image and its constants, the carried bounds'
// drift and neighbourhoods, the zeroed counters, and the fused three-level
// form of all of it (centers_prepare_all).  The bounds the constants carry
// are derived at the head of kmeans_i8.hip.
#include "kmeans_i8_dev.hpp"

#include "kmeans_centers.hpp"

namespace cyc {
namespace km8 {
namespace {

// One wave per center: max |c_j|, |c|_1, finiteness.
// (the d_* functions are the kernels' bodies, shared with the fused levels
// of centers_prepare_all; bid / tid: the stand-alone launch's block and
// thread index)
__device__ __forceinline__ void d_centers_scan(const double* __restrict__ C, int k, int d,
                                               double* __restrict__ cmax,
                                               double* __restrict__ cn1, unsigned bid,
                                               unsigned tid) {
  const int lane = tid & 63;
  const int c = (int)((bid * 256 + tid) >> 6);
  if (c >= k) return;
  double m = 0.0, s1 = 0.0;
  bool fin = true;
  for (int j = lane; j < d; j += 64) {
    const double t = C[(int64_t)c * d + j];
    fin = fin && __builtin_isfinite(t);
    m = __builtin_fmax(m, __builtin_fabs(t));
    s1 += __builtin_fabs(t);
  }
  m = wave_max(m);
  s1 = wave_sum(s1);
  const bool allFin = __all(fin);
  if (lane == 0) {
    cmax[c] = allFin ? m : __builtin_inf();
    cn1[c] = s1 * (1.0 + 0x1p-40);
  }
}
__global__ __launch_bounds__(256) void k_centers_scan(const double* __restrict__ C, int k, int d,
                                                      double* __restrict__ cmax,
                                                      double* __restrict__ cn1) {
  d_centers_scan(C, k, d, cmax, cn1, blockIdx.x, threadIdx.x);
}

// Single block: the launch's exponent, balance and on/off flag.
__device__ __forceinline__ void d_centers_params(int k, const double* __restrict__ cmax,
                                                 const double* __restrict__ cn1,
                                                 CenterParams* __restrict__ prm, unsigned tid) {
  __shared__ double sm[256], sn[256];
  double m = 0.0, nmax = 0.0;
  for (int c = tid; c < k; c += 256) {
    m = __builtin_fmax(m, cmax[c]);
    nmax = __builtin_fmax(nmax, cn1[c]);
    if (!(cmax[c] <= 0x1p60)) m = __builtin_inf();   // non-finite center
  }
  sm[tid] = m;
  sn[tid] = nmax;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (tid < (unsigned)off) {
      sm[tid] = __builtin_fmax(sm[tid], sm[tid + off]);
      sn[tid] = __builtin_fmax(sn[tid], sn[tid + off]);
    }
    __syncthreads();
  }
  if (tid == 0) {
    const double gm = sm[0];
    const int ec = choose_exp(__builtin_isfinite(gm) ? gm : 0.0);
    CenterParams p;
    p.ok = (__builtin_isfinite(gm) && ec <= kMaxExp) ? 1 : 0;
    p.ec = ec;
    const double Ac = __builtin_ldexp(1.0, ec - 22);
    const double mu = sn[0] / Ac;
    p.mu = (mu > 0.0 && __builtin_isfinite(mu)) ? mu : 1.0;
    p.k = k;
    *prm = p;
  }
}
__global__ __launch_bounds__(256) void k_centers_params(int k, const double* __restrict__ cmax,
                                                        const double* __restrict__ cn1,
                                                        CenterParams* __restrict__ prm) {
  d_centers_params(k, cmax, cn1, prm, threadIdx.x);
}

// Packed B fragments of v_mfma_i32_16x16x64_i8: lane l of 16-center tile ct,
// 64-dim step ks holds center ct*16 + (l & 15), dims ks*64 + 16 (l >> 4) + 0..15
// (the same element order as the rows' A fragments), limb planes a', b', c':
// Cb[((ct KS + ks) 3 + limb) 64 + l].  Plus cq (f32, rounded down) and g.
__global__ __launch_bounds__(256) void k_centers_pack(
    const double* __restrict__ C, const double* __restrict__ cnorm, int k, int d, int KS, int ktp,
    const double* __restrict__ cn1, const CenterParams* __restrict__ prm, uint4* __restrict__ Cb,
    float* __restrict__ cq, double* __restrict__ g) {
  const CenterParams p = *prm;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t total = (int64_t)ktp * KS * 64;
  if (idx < total) {
    const int lane = (int)(idx & 63);
    const int64_t t = idx >> 6;
    const int ks = (int)(t % KS), ct = (int)(t / KS);
    const int c = ct * 16 + (lane & 15), j0 = ks * 64 + 16 * (lane >> 4);
    int a[16], b[16], cc[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int j = j0 + e;
      const double v = (p.ok && c < k && j < d) ? C[(int64_t)c * d + j] : 0.0;
      quant3(v, p.ec, a[e], b[e], cc[e]);
    }
    uint4 pa, pb, pc;
    pa.x = pack4(a); pa.y = pack4(a + 4); pa.z = pack4(a + 8); pa.w = pack4(a + 12);
    pb.x = pack4(b); pb.y = pack4(b + 4); pb.z = pack4(b + 8); pb.w = pack4(b + 12);
    pc.x = pack4(cc); pc.y = pack4(cc + 4); pc.z = pack4(cc + 8); pc.w = pack4(cc + 12);
    uint4* dst = Cb + (t * 3) * 64 + lane;
    dst[0] = pa;
    dst[64] = pb;
    dst[128] = pc;
  }
  if (idx < (int64_t)ktp * 16) {
    const int c = (int)idx;
    if (c < k && p.ok) {
      const double gc = err_term(p.ec, cn1[c], p.mu, d);
      const double cn = cnorm[c];
      g[c] = gc;
      cq[c] = fdown((cn * cn) * (1.0 - kEpsF) - 2.0 * gc);
    } else {
      g[c] = 0.0;
      cq[c] = __builtin_inff();
    }
  }
}

// B fragments: lane l of 32-center tile ct, 32-dim substep s holds center
// 32 ct + (l & 31), dims 32 s + 16 (l >> 5) + 0..15, limb planes a', b', c':
// Cb[((ct S + s) 3 + limb) 64 + l]; the tile count is even (padding centers
// are zero with cq = +inf).
__device__ __forceinline__ void d_centers_pack32(
    const double* __restrict__ C, const double* __restrict__ cnorm, int k, int d, int S, int ktp,
    const double* __restrict__ cn1, const CenterParams* __restrict__ prm, uint4* __restrict__ Cb,
    float* __restrict__ cq, double* __restrict__ g, float* __restrict__ cq2,
    double* __restrict__ g2, float* __restrict__ cq1, double* __restrict__ g1, unsigned bid,
    unsigned tid) {
  const CenterParams p = *prm;
  const int64_t idx = (int64_t)bid * 256 + tid;
  const int64_t total = (int64_t)ktp * S * 64;
  if (idx < total) {
    const int lane = (int)(idx & 63);
    const int64_t t = idx >> 6;
    const int s = (int)(t % S), ct = (int)(t / S);
    const int c = ct * 32 + (lane & 31), j0 = s * 32 + 16 * (lane >> 5);
    int a[16], b[16], cc[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int j = j0 + e;
      const double v = (p.ok && c < k && j < d) ? C[(int64_t)c * d + j] : 0.0;
      quant3(v, p.ec, a[e], b[e], cc[e]);
    }
    uint4 pa, pb, pc;
    pa.x = pack4(a); pa.y = pack4(a + 4); pa.z = pack4(a + 8); pa.w = pack4(a + 12);
    pb.x = pack4(b); pb.y = pack4(b + 4); pb.z = pack4(b + 8); pb.w = pack4(b + 12);
    pc.x = pack4(cc); pc.y = pack4(cc + 4); pc.z = pack4(cc + 8); pc.w = pack4(cc + 12);
    uint4* dst = Cb + (t * 3) * 64 + lane;
    dst[0] = pa;
    dst[64] = pb;
    dst[128] = pc;
    // the center-major copy behind the fragments (k_screen32r's per-lane
    // gathers): center c's limb planes a', b', c' of D = 32 S bytes each,
    // dimensions in order, 6 S 16-byte pieces per center
    uint4* cr = Cb + (int64_t)ktp * S * 3 * 64 + (int64_t)c * (6 * S) + 2 * s + (lane >> 5);
    cr[0] = pa;
    cr[2 * S] = pb;
    cr[4 * S] = pc;
  }
  if (idx < (int64_t)ktp * 32) {
    const int c = (int)idx;
    if (c < k && p.ok) {
      const double gc = err_term(p.ec, cn1[c], p.mu, d);
      const double gc2 = err_term2(p.ec, cn1[c], p.mu * 0x1p-7, d);
      const double gc1 = err_term1(p.ec, cn1[c], p.mu * 0x1p-14);
      const double cn = cnorm[c];
      g[c] = gc;
      cq[c] = fdown((cn * cn) * (1.0 - kEpsF) - 2.0 * gc);
      g2[c] = gc2;
      cq2[c] = fdown((cn * cn) * (1.0 - kEpsF) - 2.0 * gc2);
      g1[c] = gc1;
      cq1[c] = fdown((cn * cn) * (1.0 - kEpsF) - 2.0 * gc1);
    } else {
      g[c] = g2[c] = g1[c] = 0.0;
      cq[c] = __builtin_inff();
      // finite: the integer passes keep index bits in L
      cq2[c] = cq1[c] = 0x1.fffffep127f;
    }
  }
}
__global__ __launch_bounds__(256) void k_centers_pack32(
    const double* __restrict__ C, const double* __restrict__ cnorm, int k, int d, int S, int ktp,
    const double* __restrict__ cn1, const CenterParams* __restrict__ prm, uint4* __restrict__ Cb,
    float* __restrict__ cq, double* __restrict__ g, float* __restrict__ cq2,
    double* __restrict__ g2, float* __restrict__ cq1, double* __restrict__ g1) {
  d_centers_pack32(C, cnorm, k, d, S, ktp, cn1, prm, Cb, cq, g, cq2, g2, cq1, g1, blockIdx.x,
                   threadIdx.x);
}

// Up to 8 counter ranges zeroed in one launch (a block per range; ZeroArgs).
__device__ __forceinline__ void d_zero_counters(const ZeroArgs& z, unsigned bid, unsigned tid) {
  unsigned int* q = z.p[bid];
  for (int i = (int)tid; i < z.w[bid]; i += 256) q[i] = 0u;
}
__global__ __launch_bounds__(256) void k_zero_counters(ZeroArgs z) {
  d_zero_counters(z, blockIdx.x, threadIdx.x);
}

// One wave per center: the drift |C_c - Cp_c| and |C_c|^2, both rounded up
// (fp64 sums of d <= 256 squares: relative error < (d + 2) 2^-53 < 2^-44),
// then Cp_c = C_c.
__device__ __forceinline__ void d_center_drift(const double* __restrict__ C,
                                               double* __restrict__ Cp, int k, int d,
                                               double* __restrict__ delta,
                                               double* __restrict__ ccs, unsigned bid,
                                               unsigned tid) {
  const int lane = tid & 63;
  const int c = (int)((bid * 256 + tid) >> 6);
  if (c >= k) return;
  double s = 0.0, q = 0.0;
  for (int j = lane; j < d; j += 64) {
    const double v = C[(int64_t)c * d + j], o = Cp[(int64_t)c * d + j];
    const double t = v - o;
    s += t * t;
    q += v * v;
    Cp[(int64_t)c * d + j] = v;
  }
  s = wave_sum(s);
  q = wave_sum(q);
  if (lane == 0) {
    delta[c] = __builtin_sqrt(s) * (1.0 + 0x1p-40) + 0x1p-500;
    ccs[c] = q * (1.0 + 0x1p-40);
  }
}
__global__ __launch_bounds__(256) void k_center_drift(const double* __restrict__ C,
                                                      double* __restrict__ Cp, int k, int d,
                                                      double* __restrict__ delta,
                                                      double* __restrict__ ccs) {
  d_center_drift(C, Cp, k, d, delta, ccs, blockIdx.x, threadIdx.x);
}

// Single block: the two largest drifts (and the largest one's center) and
// max |c|^2; any non-finite drift or norm sets `bad`.
__device__ __forceinline__ void d_drift_top(const double* __restrict__ delta,
                                            const double* __restrict__ ccs, int k,
                                            DriftParams* __restrict__ prm, unsigned tid) {
  __shared__ double s1[1024], s2[1024], sc[1024];
  __shared__ int si[1024];
  const int t = (int)tid;
  double d1 = 0.0, d2 = 0.0, cm = 0.0;
  int i1 = -1;
  bool bad = false;
  for (int c = t; c < k; c += 1024) {
    const double v = delta[c], q = ccs[c];
    bad = bad || !(v <= 0x1p1000) || !(q <= 0x1p1000);   // NaN, inf
    if (v > d1 || i1 < 0) {
      d2 = i1 < 0 ? 0.0 : d1;
      d1 = v;
      i1 = c;
    } else if (v > d2) {
      d2 = v;
    }
    cm = __builtin_fmax(cm, q);
  }
  s1[t] = d1;
  s2[t] = d2;
  si[t] = i1;
  sc[t] = cm;
  bad = __syncthreads_or(bad);
  for (int off = 512; off > 0; off >>= 1) {
    if (t < off && si[t + off] >= 0) {
      const double a1 = s1[t], a2 = s2[t], b1 = s1[t + off], b2 = s2[t + off];
      const bool aEmpty = si[t] < 0;
      if (aEmpty || b1 > a1) {
        s1[t] = b1;
        si[t] = si[t + off];
        s2[t] = aEmpty ? b2 : __builtin_fmax(a1, b2);
      } else {
        s2[t] = __builtin_fmax(a2, b1);
      }
      sc[t] = __builtin_fmax(sc[t], sc[t + off]);
    }
    __syncthreads();
  }
  if (t == 0) {
    DriftParams p;
    p.d1 = s1[0];
    p.d2 = s2[0];
    p.i1 = si[0];
    p.cmax2 = sc[0];
    p.bad = bad ? 1 : 0;
    *prm = p;
  }
}
__global__ __launch_bounds__(1024) void k_drift_top(const double* __restrict__ delta,
                                                    const double* __restrict__ ccs, int k,
                                                    DriftParams* __restrict__ prm) {
  d_drift_top(delta, ccs, k, prm, threadIdx.x);
}

// Each center's neighbourhood (one wave per center) from the packed
// statistics 0.25 dist^2 (computeStatistics, exact to ~2^-45): nbr[a] =
// a and its kCandMax - 1 nearest other centers (-1 padding when k is
// smaller), nbrR[a] = a lower bound of the distance from c_a to every
// other center (the next nearest; +inf when none is left).
// (a: the wave's center, lane: the thread's lane in it)
__device__ __forceinline__ void d_center_nbrs(const double* __restrict__ stats, int k,
                                              int32_t* __restrict__ nbr,
                                              float* __restrict__ nbrR, int a, int lane) {
  constexpr int T = kCandMax;   // kCandMax - 1 members + the next one
  double v[T];
  int ix[T];
#pragma unroll
  for (int i = 0; i < T; ++i) {
    v[i] = INFINITY;
    ix[i] = -1;
  }
  for (int j = lane; j < k; j += 64) {
    if (j == a) continue;
    const int64_t pi = a <= j ? (int64_t)j * (j + 1) / 2 + a : (int64_t)a * (a + 1) / 2 + j;
    double x = stats[pi];
    if (!(x >= 0.0)) x = INFINITY;   // NaN centers: the drift voids the bounds anyway
    // insert into the lane's sorted T smallest
    if (x < v[T - 1]) {
      double cv = x;
      int ci = j;
#pragma unroll
      for (int i = 0; i < T; ++i) {
        const bool sw = cv < v[i];
        const double tv = v[i];
        const int ti = ix[i];
        v[i] = sw ? cv : v[i];
        ix[i] = sw ? ci : ix[i];
        cv = sw ? tv : cv;
        ci = sw ? ti : ci;
      }
    }
  }
  // T rounds: the wave's smallest head, popped from its lane
  if (lane == 0) nbr[(int64_t)a * kCandMax] = a;
  for (int t = 0; t < T; ++t) {
    double bv = v[0];
    int bl = lane;
    for (int m = 32; m > 0; m >>= 1) {
      const double ov = __shfl_xor(bv, m);
      const int ol = __shfl_xor(bl, m);
      if (ov < bv || (ov == bv && ol < bl)) {
        bv = ov;
        bl = ol;
      }
    }
    const int bi = __shfl(ix[0], bl);
    if (lane == bl) {
#pragma unroll
      for (int i = 0; i < T - 1; ++i) {
        v[i] = v[i + 1];
        ix[i] = ix[i + 1];
      }
      v[T - 1] = INFINITY;
      ix[T - 1] = -1;
    }
    if (lane == 0) {
      if (t < T - 1) {
        nbr[(int64_t)a * kCandMax + 1 + t] = bv < INFINITY ? bi : -1;
      } else {
        // the next nearest: its distance, rounded down, bounds every center
        // outside the neighbourhood
        nbrR[a] = bv < INFINITY ? fdown(__builtin_sqrt(4.0 * bv) * (1.0 - 0x1p-40))
                                : __builtin_inff();
      }
    }
  }
}
__global__ __launch_bounds__(64) void k_center_nbrs(const double* __restrict__ stats, int k,
                                                    int32_t* __restrict__ nbr,
                                                    float* __restrict__ nbrR) {
  d_center_nbrs(stats, k, nbr, nbrR, blockIdx.x, threadIdx.x);
}

// ---------------------------------------------------------------------------
// centers_prepare_all (kmeans_i8.hpp PrepJobs): the center-only kernels of a
// Lloyd call as jobs of three launches, one per dependency level.
// blockIdx.y picks the job, blockIdx.x is the block index the job's
// stand-alone kernel has; a block at or past its job's extent (ext[job], 0
// for an absent job) exits.  Every job runs the stand-alone kernel's body
// with that kernel's block and thread indices, so each output is bitwise what
// the separate launches write.  No job uses dynamic LDS.
struct PrepLevel {
  unsigned ext[8];   // blocks per job
  int tps;           // statistics tiles per side
  int S, ktp32;      // center image: 32-dim substeps, 32-center tiles
};
enum { kP0Pairs, kP0Require, kP0Drift, kP0Scan, kP0Transpose, kP0Zero2, kP0Zero, kP0Jobs };
enum { kP1DriftTop, kP1Params, kP1Diag, kP1Jobs };
enum { kP2Pack, kP2Nbrs, kP2Jobs };

// Level 0: reads C, Cp (drift only, which also writes it: no other job may
// read Cp), xnorm.  Every job is a 256-thread kernel as launched alone,
// except the two-word zeroing (64 threads alone; only threads 0 and 1 act,
// so the surplus is idle).  The longest job (the pairs) is dispatched first.
__global__ __launch_bounds__(256) void k_prep_level0(PrepJobs J, PrepLevel L) {
  const unsigned job = blockIdx.y, bid = blockIdx.x, tid = threadIdx.x;
  if (bid >= L.ext[job]) return;
  switch (job) {
    case kP0Pairs:
      kmc::stats_pairs(J.C, J.k, J.d, L.tps, J.stats, J.dmin, bid, tid);
      break;
    case kP0Require:
      kmc::require_norms(J.C, J.k, J.d, J.xnorm, J.n, J.req, L.ext[kP0Require], bid, tid);
      break;
    case kP0Drift:
      d_center_drift(J.C, J.Cp, J.k, J.d, J.delta, J.ccs, bid, tid);
      break;
    case kP0Scan:
      d_centers_scan(J.C, J.k, J.d, J.scratch, J.scratch + J.k, bid, tid);
      break;
    case kP0Transpose:
      kmc::center_transpose_fill(J.C, J.k, J.d, J.d4, J.kpad, J.ct, nullptr, 0ull, bid, tid);
      break;
    case kP0Zero2:
      kmc::zero2(J.zeroA, J.zeroB, tid);
      break;
    default:
      d_zero_counters(J.zero, bid, tid);
      break;
  }
}

// Level 1: the single-block reductions of level 0's per-center scalars and
// the statistics' diagonal.  Launched at 1024 threads (k_drift_top's block);
// the 256-thread jobs are MASKED: waves 4..15 skip the body and end, so the
// body's barriers and its reduction tree see exactly the 256 threads of the
// stand-alone launch (a barrier waits only for the waves still alive).
__global__ __launch_bounds__(1024) void k_prep_level1(PrepJobs J, PrepLevel L) {
  const unsigned job = blockIdx.y, bid = blockIdx.x, tid = threadIdx.x;
  if (bid >= L.ext[job]) return;
  switch (job) {
    case kP1DriftTop:
      d_drift_top(J.delta, J.ccs, J.k, J.dprm, tid);
      break;
    case kP1Params:
      if (tid < 256) d_centers_params(J.k, J.scratch, J.scratch + J.k, J.cprm, tid);
      break;
    default:   // dmin was preset by a 0xff byte fill: ~0 marks an empty row
      if (tid < 256) kmc::stats_diag(J.k, J.stats, J.dmin, ~0ull, bid, tid);
      break;
  }
}

// Level 2: the center image (needs prm and cn1) at its own 256-thread
// tiling; the neighbourhoods (need the finished statistics) RE-TILED: one
// wave per center as alone, four centers per block instead of one (no
// barrier or LDS in the body: a wave's work and order are unchanged).
__global__ __launch_bounds__(256) void k_prep_level2(PrepJobs J, PrepLevel L) {
  const unsigned job = blockIdx.y, bid = blockIdx.x, tid = threadIdx.x;
  if (bid >= L.ext[job]) return;
  if (job == kP2Pack) {
    const size_t t16 = (size_t)J.ktp * 16;
    d_centers_pack32(J.C, J.cnorm, J.k, J.d, L.S, L.ktp32, J.scratch + J.k, J.cprm, (uint4*)J.Cb,
                     J.cq, J.g, J.cq + t16, J.g + t16, J.cq + 2 * t16, J.g + 2 * t16, bid, tid);
  } else {
    const int a = (int)(bid * 4 + (tid >> 6));
    if (a < J.k) d_center_nbrs(J.stats, J.k, J.nbr, J.nbrR, a, (int)(tid & 63));
  }
}

}  // namespace

// The center image as three dependent launches (scan, params, pack): the
// cosine plan, cyc_kmeans_assign_dev / point_cost_dev, d > 256 and
// CYC_KMEANS_PREP=0.  A Euclidean Lloyd call runs the same three bodies as
// jobs of centers_prepare_all's levels 0, 1 and 2.
int centers_prepare(const double* C, const double* cnorm, int k, int d, int ktp, void* Cb,
                    float* cq, double* g, CenterParams* prm, double* scratch, hipStream_t st) {
  const int KS = ksteps(d);
  double* cmax = scratch;
  double* cn1 = scratch + k;
  hipLaunchKernelGGL(k_centers_scan, dim3((unsigned)((k + 3) / 4)), dim3(256), 0, st, C, k, d,
                     cmax, cn1);
  CYC_LAUNCH_CHECK("k_centers_scan");
  hipLaunchKernelGGL(k_centers_params, dim3(1), dim3(256), 0, st, k, (const double*)cmax,
                     (const double*)cn1, prm);
  CYC_LAUNCH_CHECK("k_centers_params");
  if (uses32(d)) {
    // 32-center tiles, an even number of them (ktp 16-center tiles, a
    // multiple of kWaves = 4, cover them), 32-dim substeps
    const int ktp32 = tiles32(k), S = 2 * KS;
    const int64_t total = std::max<int64_t>((int64_t)ktp32 * S * 64, (int64_t)ktp32 * 32);
    hipLaunchKernelGGL(k_centers_pack32, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st,
                       C, cnorm, k, d, S, ktp32, (const double*)cn1, (const CenterParams*)prm,
                       (uint4*)Cb, cq, g, cq + pass_consts(ktp, 2), g + pass_consts(ktp, 2),
                       cq + pass_consts(ktp, 1), g + pass_consts(ktp, 1));
    CYC_LAUNCH_CHECK("k_centers_pack32");
    return CYC_OK;
  }
  const int64_t total = std::max<int64_t>((int64_t)ktp * KS * 64, (int64_t)ktp * 16);
  hipLaunchKernelGGL(k_centers_pack, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, C,
                     cnorm, k, d, KS, ktp, (const double*)cn1, (const CenterParams*)prm,
                     (uint4*)Cb, cq, g);
  CYC_LAUNCH_CHECK("k_centers_pack");
  return CYC_OK;
}

ZeroArgs screen_zero_args(unsigned int* list2Count, const CandArgs* ca, const RefineArgs* ra,
                          const AppendStage* stg) {
  const AppendStage* sg = ca ? stg : nullptr;
  ZeroArgs z{};
  auto add = [&](unsigned int* q, int words) {
    if (q) {
      z.p[z.n] = q;
      z.w[z.n++] = words;
    }
  };
  add(list2Count, 1);
  if (ca) {
    add(ca->candCount, 1);
    add(ca->candCount2, 1);
  }
  if (ra && ca) {
    add(ra->cand1Count, 1);
    add(ra->fullCount, 2);
  }
  add(sg ? sg->counts : nullptr, kSets * kShards * kShardStride);
  return z;
}

bool prep_fused() {
  static const bool on = [] {
    const char* e = std::getenv("CYC_KMEANS_PREP");
    return !(e && e[0] == '0');
  }();
  return on;
}

int launch_zero_counters(const ZeroArgs& z, hipStream_t st) {
  if (!z.n) return CYC_OK;
  hipLaunchKernelGGL(k_zero_counters, dim3(z.n), dim3(256), 0, st, z);
  CYC_LAUNCH_CHECK("k_zero_counters");
  return CYC_OK;
}

// The center-only work of a Lloyd call in three launches (kmeans_i8.hpp
// PrepJobs; the kernels above).  The require check's result is copied to the
// host right after level 0, so require_check's wait ends long before the
// row-side kernels do.
int centers_prepare_all(const PrepJobs& J, hipStream_t st, void* reqHost, hipEvent_t reqEv) {
  const int k = J.k, d = J.d;
  if (J.Cb && !uses32(d)) {
    set_error("centers_prepare_all packs the 32x32 screen's image only (d <= 256)");
    return CYC_ERR_INVALID_ARG;
  }
  if (J.nbr && !J.stats) {
    set_error("centers_prepare_all: neighbourhoods need the statistics");
    return CYC_ERR_INVALID_ARG;
  }
  auto launch = [&](auto kern, const PrepLevel& L, int jobs, unsigned threads) {
    unsigned gx = 0;
    for (int i = 0; i < jobs; ++i) gx = std::max(gx, L.ext[i]);
    if (gx) hipLaunchKernelGGL(kern, dim3(gx, (unsigned)jobs), dim3(threads), 0, st, J, L);
  };
  PrepLevel L0{};
  L0.tps = (k + kmc::kStT - 1) / kmc::kStT;
  L0.ext[kP0Pairs] = J.stats && k >= 2 ? (unsigned)(L0.tps * (L0.tps + 1) / 2) : 0u;
  L0.ext[kP0Require] = J.req ? J.reqBlocks : 0u;
  L0.ext[kP0Drift] = J.Cp ? (unsigned)((k + 3) / 4) : 0u;
  L0.ext[kP0Scan] = J.Cb ? (unsigned)((k + 3) / 4) : 0u;
  L0.ext[kP0Transpose] = J.ct ? (unsigned)(((int64_t)J.d4 * J.kpad + 255) / 256) : 0u;
  L0.ext[kP0Zero2] = J.zeroA ? 1u : 0u;
  L0.ext[kP0Zero] = (unsigned)J.zero.n;
  launch(k_prep_level0, L0, kP0Jobs, 256);
  CYC_LAUNCH_CHECK("k_prep_level0");
  if (J.req) {
    CYC_HIP(hipMemcpyAsync(reqHost, J.req, 5 * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                           st));
    CYC_HIP(hipEventRecord(reqEv, st));
  }
  PrepLevel L1{};
  L1.ext[kP1DriftTop] = J.Cp ? 1u : 0u;
  L1.ext[kP1Params] = J.Cb ? 1u : 0u;
  L1.ext[kP1Diag] = J.stats ? (unsigned)((k + 255) / 256) : 0u;
  launch(k_prep_level1, L1, kP1Jobs, 1024);
  CYC_LAUNCH_CHECK("k_prep_level1");
  PrepLevel L2{};
  if (J.Cb) {
    L2.S = 2 * ksteps(d);
    L2.ktp32 = tiles32(k);
    const int64_t total =
        std::max<int64_t>((int64_t)L2.ktp32 * L2.S * 64, (int64_t)L2.ktp32 * 32);
    L2.ext[kP2Pack] = (unsigned)((total + 255) / 256);
  }
  L2.ext[kP2Nbrs] = J.nbr ? (unsigned)((k + 3) / 4) : 0u;
  launch(k_prep_level2, L2, kP2Jobs, 256);
  CYC_LAUNCH_CHECK("k_prep_level2");
  return CYC_OK;
}

int centers_drift(const double* C, double* Cp, int k, int d, double* delta, double* ccs,
                  DriftParams* prm, hipStream_t st) {
  hipLaunchKernelGGL(k_center_drift, dim3((unsigned)((k + 3) / 4)), dim3(256), 0, st, C, Cp, k, d,
                     delta, ccs);
  CYC_LAUNCH_CHECK("k_center_drift");
  hipLaunchKernelGGL(k_drift_top, dim3(1), dim3(1024), 0, st, (const double*)delta,
                     (const double*)ccs, k, prm);
  CYC_LAUNCH_CHECK("k_drift_top");
  return CYC_OK;
}

// The neighbourhoods alone (bounds_filter, when centers_prepare_all has not
// built them).
int launch_center_nbrs(const double* stats, int k, int32_t* nbr, float* nbrR, hipStream_t st) {
  hipLaunchKernelGGL(k_center_nbrs, dim3((unsigned)k), dim3(64), 0, st, stats, k, nbr, nbrR);
  CYC_LAUNCH_CHECK("k_center_nbrs");
  return CYC_OK;
}

}  // namespace km8
}  // namespace cyc
