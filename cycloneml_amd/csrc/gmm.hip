// gmm.hip -- GaussianMixture on gfx950 (MI355X): the E step and the
// sufficient-statistics aggregate of ml/clustering/GaussianMixture.scala
// (ExpectationAggregator.add) over dense fp64 rows, and the model's
// predict / predictProbability / logpdf.
//
// Model (cyc_gmm_set_model_dev): k mixture weights w_j, means mu_j (k x d,
// row-major), rootSigmaInv A_j (k matrices d x d, row-major) and the constants
// u_j = -0.5 (d log 2 pi + logPseudoDet_j) of ml/stat/distribution/
// MultivariateGaussian.scala.  logpdf_j(x) = u_j - 0.5 |A_j (x - mu_j)|^2: the
// mean is subtracted BEFORE the product, as the reference does (A x - A mu
// cancels for a tight cluster far from the origin).
//
// Per row i of weight om_i: p_ij = EPSILON + w_j exp(logpdf_j(x_i)), s_i =
// sum_j p_ij, r_ij = om_i p_ij / s_i, ll += om_i log s_i.  sums is one fp64
// buffer [ll | W_j (k) | M_j (k x d) | S_j (k x d(d+1)/2, packed upper,
// column-major U[b(b+1)/2 + a], a <= b)]: W_j = sum_i r_ij, M_j = sum_i r_ij
// x_i, S_j = sum_i r_ij x_i x_i^T.  Calls ADD into it.
//
// Kernels
//   pack          row_gemm.hpp: every A_j^T into the image the E step stages
//                 as the MFMA B operand, one per component, explicit zeros
//                 past d.  Once per cyc_gmm_set_model_dev.
//   k_gmm_estep   a workgroup (8 waves x 32 rows) owns a 256-row tile and walks
//                 the components.  For component j the X values become the A
//                 operand of v_mfma_f64_16x16x4f64 as x - mu_j (one VALU
//                 subtract per element and component beside d^2 MACs), B is the
//                 staged A_j^T image (panels of <= 4 column tiles through two
//                 LDS buffers, the next chunk of X, mu and B one step ahead;
//                 the step stream runs across panels and components, so only
//                 the first step of a tile waits for its loads).  A panel's
//                 accumulators are squared and added per lane, and after the
//                 last panel the 16 lanes that hold one row are summed by a
//                 fixed xor tree: q_ij.  Lane (l & 15) keeps component jb +
//                 (l & 15) of each group of 16, so exp runs once per (row,
//                 component): p_ij goes to the N x k workspace, s_i is the
//                 groups' tree sums in order.  The last pass re-reads the
//                 lane's own p_ij and stores r_ij (TRAIN) or p_ij / s_i and
//                 the argmax (lowest index on ties); each wave adds its rows'
//                 om_i log s_i in a fixed order into one slab entry.
//   fold_add      row_gemm.hpp: sums[0] += the slab, in a fixed order.
//   k_gmm_mstep   sum_i r_ij z_i z_i^T over the augmented row z = [x, 1], so
//                 M_j is column d and W_j entry (d, d), as aSum and wSum ride
//                 k_wls_tiles.  A workgroup owns one pair of 32-column panels
//                 (upper block triangle only), one group of 16 components and
//                 one row split; 16-row chunks of the two panels and of the 16
//                 r columns are staged through LDS ONCE and serve all 16
//                 components: wave v multiplies the i-side operand by r of
//                 components 4v .. 4v + 3 as it leaves LDS.  Rows whose 16 r
//                 are all zero stage zeros (weight 0 rows never reach an
//                 accumulator, whatever their features hold).
//   k_gmm_fold    sums += the split-K slabs in split order.
// No atomics on doubles: every sum has one fixed order, so two calls on the
// same inputs give the same bits.  Padded rows and columns are explicit zeros
// and padded accumulators are never stored.
//
// Registers (gfx950: 512 unified VGPRs per SIMD lane).  k_gmm_mstep keeps,
// per wave, GC components x (2 x 2) tiles x 4 doubles of accumulators = 32 GC
// VGPRs; operands (2 + 2 + GC doubles and one product), the prefetched chunk
// (5 doubles) and addresses take about 50 more.  At two waves per SIMD (two
// workgroups per CU, so one can stage while the other multiplies) the budget
// is 256: GC = 4 (128 + ~50) fits, GC = 8 (256 for the accumulators alone)
// does not.  Four waves make the group of 16 components per staged chunk.
// k_gmm_estep: 2 x 4 tiles x 4 doubles = 64 VGPRs of accumulators, two X / mu
// chunks (2 x 12 doubles), q / qv / s (24 doubles): two waves per SIMD.
//
// Cost per row of one EM step: E 2 k d^2 flop, M k (d + 1)(d + 2) flop; X is
// read twice (once by each kernel's tile owner; the M step's panel pairs
// re-read it through L2) and r costs 16 k bytes (written once, read once).
// At d = 64, k = 16: 131,072 + 68,640 = 199,712 flop against 1,024 + 256 bytes
// = 156 flop / B, machine balance ~10 flop / B (78.6 TF fp64 MFMA, 8 TB/s):
// MFMA-bound, 2.5 ms per 1M rows at the roofline.  Calling the WLS plan k
// times would read X k times: 8 flop / B, HBM-bound.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <string>

#include "common.hpp"
#include "row_gemm.hpp"

struct cyc_gmm_plan_s {
  std::mutex mu;
  int k = 0, d = 0;
  int64_t chunkRows = 0;
  int64_t imgLen = 0;          // doubles of one component's packed A_j^T
  bool haveModel = false;
  cyc::DeviceBuffer model;     // w (k) | mu (k d) | u (k)
  cyc::DeviceBuffer pack, ws, slab, llSlab, flag;
};

namespace {

// the image's tiling (kChunk, kPanelTiles), the E step's workgroup (kWaves,
// kTileRows), pack and fold_add
using namespace cyc::rowgemm;

constexpr double kEps = 2.220446049250313e-16;   // ml.impl.Utils.EPSILON = 2^-52
constexpr int kEGrid = 4096;                // E step grid cap (ll slab: kEGrid x kWaves)
constexpr int kMaxFeatures = 1024;
constexpr int64_t kWorkspaceBytes = (int64_t)1 << 30;

constexpr int MKC = 16;                     // M step: rows per LDS chunk
constexpr int MP = 32;                      // columns per panel
constexpr int MLD = MP + 16;                // LDS row stride: rows kk, kk + 1 on disjoint banks
constexpr int MG = 16;                      // components per workgroup
constexpr int MGC = 4;                      // components per wave
constexpr int64_t kSlabBytes = (int64_t)256 << 20;

// TRAIN: P (nrows x k) = r_ij, llSlab[workgroup kWaves + wave] = the wave's
// sum of om_i log s_i, a negative or NaN row weight sets *flag (the row then
// counts as weight 0).  Otherwise P = p_ij / s_i (the caller's prob or a
// scratch), label = argmax.  logpdf (either mode) may be null.
template <bool TRAIN>
__global__ __launch_bounds__(64 * kWaves, 2) void k_gmm_estep(
    const double* __restrict__ X, int64_t nrows, int d, int k, const double* __restrict__ Bp,
    int64_t imgLen, int KT, const double* __restrict__ wt, const double* __restrict__ mu,
    const double* __restrict__ u, const double* __restrict__ rw, double* P,
    double* __restrict__ logpdf, int32_t* __restrict__ label, double* __restrict__ llSlab,
    int* __restrict__ flag) {
  constexpr int CHMAX = 256 * kPanelTiles;
  constexpr int PT = CHMAX / (64 * kWaves);
  __shared__ double Bs[2][CHMAX];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, c = lane & 15;
  const int nfull = d / kChunk, nch = nfull + (d % kChunk != 0);
  const int panels = (KT + kPanelTiles - 1) / kPanelTiles;
  const int64_t steps = (int64_t)k * panels * nch;
  const int64_t items = (nrows + kTileRows - 1) / kTileRows;
  double llAcc = 0.0;
  for (int64_t w = blockIdx.x; w < items; w += gridDim.x) {
    const int64_t r0 = w * kTileRows + wave * 32;
    // rows past nrows read the last row and indices past d the last index: a
    // valid address and no branch around a load; the multiply replaces both
    // by explicit zeros when it reads the registers
    const double* xp[2];
    bool ok[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int64_t row = r0 + t * 16 + c;
      ok[t] = row < nrows;
      xp[t] = X + (ok[t] ? row : nrows - 1) * d;
    }
    auto loadX = [&](int j, int ch, double (&x)[2][4], double (&m)[4]) {
      const int64_t f0 = (int64_t)ch * kChunk + 4 * g;
      const double* mp = mu + (int64_t)j * d;
      if (ch < nfull) {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          const double4_a8 v = *reinterpret_cast<const double4_a8*>(xp[t] + f0);
#pragma unroll
          for (int e = 0; e < 4; ++e) x[t][e] = v[e];
        }
        const double4_a8 v = *reinterpret_cast<const double4_a8*>(mp + f0);
#pragma unroll
        for (int e = 0; e < 4; ++e) m[e] = v[e];
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int64_t f = std::min<int64_t>(f0 + e, d - 1);
          x[0][e] = xp[0][f];
          x[1][e] = xp[1][f];
          m[e] = mp[f];
        }
      }
    };
    auto loadB = [&](int j, int pn, int ch, double (&b)[PT]) {
      const int ctn = min(kPanelTiles, KT - pn * kPanelTiles);
      const double* src = Bp + (int64_t)j * imgLen + ((int64_t)ch * KT + pn * kPanelTiles) * 256;
#pragma unroll
      for (int q = 0; q < PT; ++q) b[q] = src[min(tid + q * 64 * kWaves, 256 * ctn - 1)];
    };
    auto storeB = [&](int buf, const double (&b)[PT]) {
#pragma unroll
      for (int q = 0; q < PT; ++q) Bs[buf][tid + q * 64 * kWaves] = b[q];
    };
    cyc_double4 acc[2][kPanelTiles];
    double q[2][4], qv[2][4], s[2][4];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
#pragma unroll
      for (int ct = 0; ct < kPanelTiles; ++ct) acc[t][ct] = cyc_double4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int r = 0; r < 4; ++r) q[t][r] = qv[t][r] = s[t][r] = 0.0;
    }
    // components jb .. jb + 15 are done: lane c holds q of component jb + c
    auto group = [&](int jb) {
      const int jm = jb + c;
      const bool valid = jm < k;
      const double uj = valid ? u[jm] : 0.0, wj = valid ? wt[jm] : 0.0;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const double lp = uj - 0.5 * qv[t][r];
          const double p = valid ? kEps + wj * exp(lp) : 0.0;
          const int64_t row = r0 + t * 16 + g + 4 * r;
          if (valid && row < nrows) {
            if (logpdf) logpdf[row * k + jm] = lp;
            P[row * k + jm] = p;
          }
          double gs = p;
#pragma unroll
          for (int sh = 1; sh < 16; sh <<= 1) gs += __shfl_xor(gs, sh);
          s[t][r] += gs;
          qv[t][r] = 0.0;
        }
    };
    double xa[2][4], xb[2][4], ma[4], mb[4], bn[PT];
    int j = 0, pn = 0, ch = 0;
    int64_t st = 0;
    __syncthreads();   // the previous item's last chunk is read
    loadB(0, 0, 0, bn);
    loadX(0, 0, xa, ma);
    storeB(0, bn);
    __syncthreads();
    // step st = (j, pn, ch): issue the next step's loads, multiply, park the
    // next B chunk in the other buffer (free since the barrier that ended
    // step st - 1)
    auto step = [&](double (&xc)[2][4], double (&mc)[4], double (&xn)[2][4], double (&mn)[4]) {
      int jn = j, pnn = pn, chn = ch + 1;
      if (chn == nch) {
        chn = 0;
        if (++pnn == panels) {
          pnn = 0;
          ++jn;
        }
      }
      const bool more = st + 1 < steps;
      if (more) {
        loadB(jn, pnn, chn, bn);
        loadX(jn, chn, xn, mn);
      }
      const double* W = Bs[st & 1];
      const int ctn = min(kPanelTiles, KT - pn * kPanelTiles);
      const int64_t f0 = (int64_t)ch * kChunk + 4 * g;
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        const bool in = f0 + kk < d;
        const double a0 = (ok[0] && in) ? xc[0][kk] - mc[kk] : 0.0;
        const double a1 = (ok[1] && in) ? xc[1][kk] - mc[kk] : 0.0;
#pragma unroll
        for (int ct = 0; ct < kPanelTiles; ++ct) {
          if (ct < ctn) {
            const double b = W[(ct * 4 + kk) * 64 + lane];
            acc[0][ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b, acc[0][ct], 0, 0, 0);
            acc[1][ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b, acc[1][ct], 0, 0, 0);
          }
        }
      }
      if (ch == nch - 1) {
        // lane holds rows 16 t + g + 4 r, column c of each tile
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int ct = 0; ct < kPanelTiles; ++ct) {
            if (ct < ctn) {
#pragma unroll
              for (int r = 0; r < 4; ++r) q[t][r] += acc[t][ct][r] * acc[t][ct][r];
            }
            acc[t][ct] = cyc_double4{0.0, 0.0, 0.0, 0.0};
          }
        if (pn == panels - 1) {
#pragma unroll
          for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              double v = q[t][r];
#pragma unroll
              for (int sh = 1; sh < 16; sh <<= 1) v += __shfl_xor(v, sh);
              if (c == (j & 15)) qv[t][r] = v;
              q[t][r] = 0.0;
            }
          if ((j & 15) == 15 || j == k - 1) group(j & ~15);
        }
      }
      if (more) {
        storeB((int)((st + 1) & 1), bn);
        __syncthreads();
      }
      j = jn;
      pn = pnn;
      ch = chn;
      ++st;
    };
    while (st < steps) {
      step(xa, ma, xb, mb);
      if (st < steps) step(xb, mb, xa, ma);
    }
    // the lane's own p_ij again: r_ij or the probability, and the argmax
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t row = r0 + t * 16 + g + 4 * r;
        const bool rok = row < nrows;
        double om = 1.0;
        if constexpr (TRAIN) {
          om = (rok && rw) ? rw[row] : 1.0;
          if (!(om >= 0.0)) {
            if (c == 0) atomicOr(flag, 1);
            om = 0.0;
          }
        }
        const double si = s[t][r];
        double best = -__builtin_inf();
        int bi = 0x7fffffff;
        for (int jm = c; jm < k; jm += 16) {
          if (!rok) break;
          const double pr = P[row * k + jm] / si;
          if constexpr (TRAIN) {
            P[row * k + jm] = om > 0.0 ? om * pr : 0.0;
          } else {
            P[row * k + jm] = pr;
            if (pr > best) {
              best = pr;
              bi = jm;
            }
          }
        }
        if constexpr (TRAIN) {
          if (rok && om > 0.0) llAcc += om * log(si);
        } else {
#pragma unroll
          for (int sh = 1; sh < 16; sh <<= 1) {
            const double ob = __shfl_xor(best, sh);
            const int oi = __shfl_xor(bi, sh);
            if (ob > best || (ob == best && oi < bi)) {
              best = ob;
              bi = oi;
            }
          }
          if (rok && label && c == 0) label[row] = bi == 0x7fffffff ? 0 : bi;
        }
      }
  }
  if constexpr (TRAIN) {
    // every lane of a 16-group holds the same sum: add the four groups
    llAcc += __shfl_xor(llAcc, 16);
    llAcc += __shfl_xor(llAcc, 32);
    if (lane == 0) llSlab[(int64_t)blockIdx.x * kWaves + wave] = llAcc;
  }
}

// slab[((split k + j) pairs + pair) 1024 + a 32 + b] = sum over the split's
// rows of R[row][j] z[I0 + a] z[J0 + b], z = [x, 1] (zero past d).  blockIdx.x
// = pair of panels (upper block triangle), y = component group, z = split.
__global__ __launch_bounds__(256, 2) void k_gmm_mstep(
    const double* __restrict__ X, int64_t nrows, int d, int k, const double* __restrict__ R,
    int panelsPerSide, int64_t rowsPerSplit, double* __restrict__ slab) {
  __shared__ double Zi[MKC * MLD];
  __shared__ double Zj[MKC * MLD];
  __shared__ double Rc[MKC * MG];
  int t = blockIdx.x, pi = 0;
  while (t >= panelsPerSide - pi) {
    t -= panelsPerSide - pi;
    ++pi;
  }
  const int pj = pi + t;
  const bool diag = pi == pj;
  const int I0 = pi * MP, J0 = pj * MP;
  const int j0 = blockIdx.y * MG;
  const int64_t r0 = (int64_t)blockIdx.z * rowsPerSplit;
  const int64_t r1 = min<int64_t>(nrows, r0 + rowsPerSplit);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, c = lane & 15;
  const int ncomp = min(MGC, k - j0 - MGC * wave);   // this wave's components (<= 0: none)

  cyc_double4 acc[MGC][2][2];
#pragma unroll
  for (int cc = 0; cc < MGC; ++cc)
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b) acc[cc][a][b] = cyc_double4{0.0, 0.0, 0.0, 0.0};

  // staging map: thread -> row sr, component sc, columns sc and sc + 16 of
  // both panels; the 16 threads of a row are 16 consecutive lanes
  const int sr = tid >> 4, sc = tid & 15;
  double rr, zi[2], zj[2];
  auto load = [&](int64_t rb) {
    const int64_t row = rb + sr;
    const bool rok = row < r1;
    const int64_t rc = rok ? row : nrows - 1;   // a valid address either way
    const double rv = R[rc * k + min(j0 + sc, k - 1)];
    rr = (rok && j0 + sc < k) ? rv : 0.0;
    int alive = rr != 0.0;
#pragma unroll
    for (int sh = 1; sh < 16; sh <<= 1) alive |= __shfl_xor(alive, sh);
    const double* xr = X + rc * d;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int ci = I0 + sc + 16 * h, cj = J0 + sc + 16 * h;
      const double vi = xr[min(ci, d - 1)], vj = xr[min(cj, d - 1)];
      zi[h] = !alive ? 0.0 : (ci < d ? vi : (ci == d ? 1.0 : 0.0));
      zj[h] = !alive ? 0.0 : (cj < d ? vj : (cj == d ? 1.0 : 0.0));
    }
  };
  auto store = [&]() {
    Rc[sr * MG + sc] = rr;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      Zi[sr * MLD + sc + 16 * h] = zi[h];
      Zj[sr * MLD + sc + 16 * h] = zj[h];
    }
  };

  if (r0 < r1) load(r0);
  for (int64_t rb = r0; rb < r1; rb += MKC) {
    __syncthreads();
    store();
    __syncthreads();
    if (rb + MKC < r1) load(rb + MKC);
    if (ncomp <= 0) continue;
#pragma unroll
    for (int kk = 0; kk < MKC; kk += 4) {
      const int krow = kk + g;
      double a[2], b[2];
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        a[m] = Zi[krow * MLD + m * 16 + c];
        b[m] = Zj[krow * MLD + m * 16 + c];
      }
#pragma unroll
      for (int cc = 0; cc < MGC; ++cc) {
        if (cc < ncomp) {
          const double rv = Rc[krow * MG + MGC * wave + cc];
#pragma unroll
          for (int mi = 0; mi < 2; ++mi) {
            const double ra = rv * a[mi];
#pragma unroll
            for (int mj = 0; mj < 2; ++mj) {
              if (diag && mi > mj) continue;   // below the diagonal: never folded
              acc[cc][mi][mj] =
                  __builtin_amdgcn_mfma_f64_16x16x4f64(ra, b[mj], acc[cc][mi][mj], 0, 0, 0);
            }
          }
        }
      }
    }
  }

  const int64_t pairs = (int64_t)panelsPerSide * (panelsPerSide + 1) / 2;
#pragma unroll
  for (int cc = 0; cc < MGC; ++cc) {
    if (cc >= ncomp) continue;
    const int j = j0 + MGC * wave + cc;
    double* out = slab + (((int64_t)blockIdx.z * k + j) * pairs + blockIdx.x) * (MP * MP);
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int mj = 0; mj < 2; ++mj)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          out[(mi * 16 + g + 4 * r) * MP + mj * 16 + c] = acc[cc][mi][mj][r];
  }
}

// sums += the slabs in split order.  Entry (a, b), a <= b <= d, of component
// j: b < d -> S_j[b(b+1)/2 + a]; b == d, a < d -> M_j[a]; a == b == d -> W_j.
// blockIdx.x = quarter of a 32 x 32 tile, y = pair, z = component.
__global__ __launch_bounds__(256) void k_gmm_fold(const double* __restrict__ slab, int64_t splits,
                                                  int panelsPerSide, int d, int k,
                                                  double* __restrict__ sums) {
  int t = blockIdx.y, pi = 0;
  while (t >= panelsPerSide - pi) {
    t -= panelsPerSide - pi;
    ++pi;
  }
  const int pj = pi + t;
  const int e = blockIdx.x * 256 + threadIdx.x;
  const int a = pi * MP + (e >> 5), b = pj * MP + (e & 31);
  if (a > b || b > d) return;
  const int j = blockIdx.z;
  const int64_t pairs = (int64_t)panelsPerSide * (panelsPerSide + 1) / 2;
  const int64_t stride = (int64_t)k * pairs * (MP * MP);
  const double* src = slab + ((int64_t)j * pairs + blockIdx.y) * (MP * MP) + e;
  double s = 0.0;
  for (int64_t sp = 0; sp < splits; ++sp) s += src[sp * stride];
  const int64_t tri = (int64_t)d * (d + 1) / 2;
  double* dst;
  if (b < d) dst = sums + 1 + k + (int64_t)k * d + j * tri + (int64_t)b * (b + 1) / 2 + a;
  else if (a < d) dst = sums + 1 + k + (int64_t)j * d + a;
  else dst = sums + 1 + j;
  *dst += s;
}

const double* model_w(cyc_gmm_plan_s* p) { return (const double*)p->model.ptr; }
const double* model_mu(cyc_gmm_plan_s* p) { return model_w(p) + p->k; }
const double* model_u(cyc_gmm_plan_s* p) { return model_mu(p) + (int64_t)p->k * p->d; }

template <bool TRAIN>
int estep(cyc_gmm_plan_s* p, const double* X, int64_t rows, const double* rw, double* P,
          double* logpdf, int32_t* label, int64_t* waves, hipStream_t st) {
  const int64_t items = (rows + kTileRows - 1) / kTileRows;
  const int64_t grid = std::min<int64_t>(items, kEGrid);
  if (waves) *waves = grid * kWaves;
  cyc::KernelTimer timer("k_gmm_estep", st);
  hipLaunchKernelGGL((k_gmm_estep<TRAIN>), dim3((unsigned)grid), dim3(64 * kWaves), 0, st, X, rows,
                     p->d, p->k, (const double*)p->pack.ptr, p->imgLen, tiles16(p->d), model_w(p),
                     model_mu(p), model_u(p), rw, P, logpdf, label, (double*)p->llSlab.ptr,
                     (int*)p->flag.ptr);
  CYC_LAUNCH_CHECK("k_gmm_estep");
  return CYC_OK;
}

// sums += the aggregate of `rows` rows of X under the responsibilities R
int mstep(cyc_gmm_plan_s* p, const double* X, int64_t rows, const double* R, double* sums,
          hipStream_t st) {
  const int d = p->d, k = p->k;
  const int pps = (d + 1 + MP - 1) / MP;
  const int64_t pairs = (int64_t)pps * (pps + 1) / 2;
  const int groups = (k + MG - 1) / MG;
  const int64_t perSplit = (int64_t)k * pairs * (MP * MP);   // doubles
  // two workgroups per CU twice over, at least 64 rows per split, the slab
  // within its cap
  const int64_t want = 4 * (int64_t)cyc::device_cus();
  int64_t splits = std::max<int64_t>(1, (want + pairs * groups - 1) / (pairs * groups));
  splits = std::min<int64_t>(splits, std::max<int64_t>(1, rows / 64));
  splits = std::min<int64_t>(splits, std::max<int64_t>(1, kSlabBytes / (8 * perSplit)));
  splits = std::min<int64_t>(splits, 65535);
  const int64_t rps = cyc::round_up((rows + splits - 1) / splits, MKC);
  splits = (rows + rps - 1) / rps;
  if (int rc = p->slab.reserve(sizeof(double) * (size_t)splits * (size_t)perSplit)) return rc;
  {
    cyc::KernelTimer timer("k_gmm_mstep", st);
    hipLaunchKernelGGL(k_gmm_mstep, dim3((unsigned)pairs, (unsigned)groups, (unsigned)splits),
                       dim3(256), 0, st, X, rows, d, k, R, pps, rps, (double*)p->slab.ptr);
    CYC_LAUNCH_CHECK("k_gmm_mstep");
  }
  cyc::KernelTimer timer("k_gmm_fold", st);
  hipLaunchKernelGGL(k_gmm_fold, dim3(MP * MP / 256, (unsigned)pairs, (unsigned)k), dim3(256), 0,
                     st, (const double*)p->slab.ptr, splits, pps, d, k, sums);
  CYC_LAUNCH_CHECK("k_gmm_fold");
  return CYC_OK;
}

}  // namespace

extern "C" {

int cyc_gmm_plan_create(int32_t k, int32_t numFeatures, int64_t chunkRows, cyc_gmm_plan* plan) {
  CYC_REQUIRE(plan != nullptr, "plan must not be null");
  CYC_REQUIRE(k >= 1, "k must be positive but got " + std::to_string(k));
  CYC_REQUIRE(k <= 65535, "k up to 65535 is supported but got " + std::to_string(k));
  CYC_REQUIRE(numFeatures >= 1,
              "numFeatures must be positive but got " + std::to_string(numFeatures));
  CYC_REQUIRE(numFeatures <= kMaxFeatures,
              "GaussianMixture supports up to " + std::to_string(kMaxFeatures) +
                  " features but got " + std::to_string(numFeatures));
  CYC_REQUIRE(chunkRows >= 0, "chunkRows must not be negative");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    cyc::set_error("no HIP device visible");
    return CYC_ERR_NO_DEVICE;
  }
  auto* p = new cyc_gmm_plan_s();
  p->k = k;
  p->d = numFeatures;
  p->imgLen = packed_len(numFeatures, numFeatures);
  // chunkRows k doubles of r within the cap; whole row tiles when it allows
  if (chunkRows == 0) {
    chunkRows = std::max<int64_t>(1, kWorkspaceBytes / (8 * (int64_t)k));
    if (chunkRows > kTileRows) chunkRows -= chunkRows % kTileRows;
  }
  p->chunkRows = chunkRows;
  *plan = p;
  return CYC_OK;
}

int cyc_gmm_plan_destroy(cyc_gmm_plan plan) {
  delete plan;
  return CYC_OK;
}

int cyc_gmm_set_model_dev(cyc_gmm_plan plan, const double* weights, const double* means,
                          const double* rootSigmaInv, const double* u, void* stream) {
  CYC_REQUIRE(plan != nullptr, "plan must not be null");
  CYC_REQUIRE(weights != nullptr && means != nullptr && rootSigmaInv != nullptr && u != nullptr,
              "weights, means, rootSigmaInv and u must not be null");
  cyc_gmm_plan_s* p = plan;
  hipStream_t st = cyc::as_stream(stream);
  std::lock_guard<std::mutex> g(p->mu);
  const int64_t k = p->k, d = p->d;
  if (int rc = p->model.reserve(sizeof(double) * (size_t)(2 * k + k * d))) return rc;
  if (int rc = p->pack.reserve(sizeof(double) * (size_t)(k * p->imgLen))) return rc;
  double* m = (double*)p->model.ptr;
  CYC_HIP(hipMemcpyAsync(m, weights, sizeof(double) * k, hipMemcpyDeviceToDevice, st));
  CYC_HIP(hipMemcpyAsync(m + k, means, sizeof(double) * k * d, hipMemcpyDeviceToDevice, st));
  CYC_HIP(hipMemcpyAsync(m + k + k * d, u, sizeof(double) * k, hipMemcpyDeviceToDevice, st));
  // B_j(f, col) = A_j[col, f]: A_j^T
  if (int rc = pack(rootSigmaInv, (int)d, (int)d, 1, d, k, d * d, (double*)p->pack.ptr, st))
    return rc;
  p->haveModel = true;
  return CYC_OK;
}

int cyc_gmm_accumulate_dev(cyc_gmm_plan plan, const double* X, int64_t nrows, const double* w,
                           double* sums, void* stream) {
  CYC_REQUIRE(plan != nullptr, "plan must not be null");
  CYC_REQUIRE(nrows >= 0, "nrows >= 0");
  CYC_REQUIRE(sums != nullptr, "sums must not be null");
  cyc_gmm_plan_s* p = plan;
  hipStream_t st = cyc::as_stream(stream);
  std::lock_guard<std::mutex> g(p->mu);
  CYC_REQUIRE(p->haveModel, "cyc_gmm_set_model_dev must be called first");
  if (nrows == 0) return CYC_OK;
  CYC_REQUIRE(X != nullptr, "non-null rows");
  const int64_t chunk = std::min(p->chunkRows, nrows);
  if (int rc = p->ws.reserve(sizeof(double) * (size_t)chunk * (size_t)p->k)) return rc;
  if (int rc = p->llSlab.reserve(sizeof(double) * kEGrid * kWaves)) return rc;
  if (int rc = p->flag.reserve(sizeof(int))) return rc;
  CYC_HIP(hipMemsetAsync(p->flag.ptr, 0, sizeof(int), st));
  double* R = (double*)p->ws.ptr;
  for (int64_t r0 = 0; r0 < nrows; r0 += chunk) {
    const int64_t rows = std::min(chunk, nrows - r0);
    const double* Xc = X + r0 * p->d;
    int64_t waves = 0;
    if (int rc = estep<true>(p, Xc, rows, w ? w + r0 : nullptr, R, nullptr, nullptr, &waves, st))
      return rc;
    if (int rc = fold_add((const double*)p->llSlab.ptr, waves, sums, st)) return rc;
    if (int rc = mstep(p, Xc, rows, R, sums, st)) return rc;
  }
  int bad = 0;
  CYC_HIP(hipMemcpyAsync(&bad, p->flag.ptr, sizeof(int), hipMemcpyDeviceToHost, st));
  CYC_HIP(hipStreamSynchronize(st));
  CYC_REQUIRE(bad == 0, "illegal weight value: instance weights must be >= 0.0");
  return CYC_OK;
}

int cyc_gmm_mstep_dev(cyc_gmm_plan plan, const double* X, int64_t nrows, const double* R,
                      double* sums, void* stream) {
  CYC_REQUIRE(plan != nullptr, "plan must not be null");
  CYC_REQUIRE(nrows >= 0, "nrows >= 0");
  CYC_REQUIRE(sums != nullptr, "sums must not be null");
  if (nrows == 0) return CYC_OK;
  CYC_REQUIRE(X != nullptr && R != nullptr, "non-null rows and responsibilities");
  cyc_gmm_plan_s* p = plan;
  hipStream_t st = cyc::as_stream(stream);
  std::lock_guard<std::mutex> g(p->mu);
  const int64_t chunk = std::min(p->chunkRows, nrows);
  for (int64_t r0 = 0; r0 < nrows; r0 += chunk) {
    const int64_t rows = std::min(chunk, nrows - r0);
    if (int rc = mstep(p, X + r0 * p->d, rows, R + r0 * p->k, sums, st)) return rc;
  }
  return CYC_OK;
}

int cyc_gmm_predict_dev(cyc_gmm_plan plan, const double* X, int64_t nrows, double* prob,
                        int32_t* label, double* logpdf, void* stream) {
  CYC_REQUIRE(plan != nullptr, "plan must not be null");
  CYC_REQUIRE(nrows >= 0, "nrows >= 0");
  CYC_REQUIRE(prob != nullptr || label != nullptr || logpdf != nullptr,
              "at least one of prob, label and logpdf");
  cyc_gmm_plan_s* p = plan;
  hipStream_t st = cyc::as_stream(stream);
  std::lock_guard<std::mutex> g(p->mu);
  CYC_REQUIRE(p->haveModel, "cyc_gmm_set_model_dev must be called first");
  if (nrows == 0) return CYC_OK;
  CYC_REQUIRE(X != nullptr, "non-null rows");
  const int64_t chunk = std::min(p->chunkRows, nrows);
  if (!prob)
    if (int rc = p->ws.reserve(sizeof(double) * (size_t)chunk * (size_t)p->k)) return rc;
  if (int rc = p->llSlab.reserve(sizeof(double) * kEGrid * kWaves)) return rc;
  if (int rc = p->flag.reserve(sizeof(int))) return rc;
  for (int64_t r0 = 0; r0 < nrows; r0 += chunk) {
    const int64_t rows = std::min(chunk, nrows - r0);
    if (int rc = estep<false>(p, X + r0 * p->d, rows, nullptr,
                              prob ? prob + r0 * p->k : (double*)p->ws.ptr,
                              logpdf ? logpdf + r0 * p->k : nullptr,
                              label ? label + r0 : nullptr, nullptr, st))
      return rc;
  }
  return CYC_OK;
}

}  // extern "C"
