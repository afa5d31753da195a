// fm.hip -- FMRegressor / FMClassifier on gfx950 (MI355X): one evaluation of
// the factorization machine's loss and gradient over dense fp64 rows, and the
// models' forward (ml/regression/FMRegressor.scala's BaseFactorizationMachines
// Gradient, Spark 3.3).
//
// Layouts.  coef = [V (d x k row-major) | w (d, fitLinear) | b (1, fitIntercept)].
// Per row: raw = b + sum_i w_i x_i + sum_f 0.5 (s_f s_f - q_f), s_f = sum_i
// V[i,f] x_i, q_f = sum_i (V[i,f] x_i)^2; m = 2 (raw - y) (squared) or
// 1 / (1 + exp(-raw)) - y (logistic); the row's gradient is m (x_i s_f -
// V[i,f] x_i x_i | x_i | 1).  Summed over the rows of the batch:
//   gV = P - V o t,  P = X^T (m o S) (d x k),  t_i = sum_r m_r x_ri^2,
//   gw = X^T m,  gb = sum m,  L = sum loss,  cnt = rows taken.
// out = [gV | gw | gb | L | cnt] (the coefficients' layout, then two doubles).
//
// Operand images.  Once per call k_fm_operands writes [V | w] and [V o V | 0]
// (d x (k + 1) each) and row_gemm.hpp's k_row_pack turns both into the packed
// MFMA B layout: KT = tiles16(k + 1) column tiles, read from L2 by every wave
// as 64 consecutive doubles per MFMA.
//
// Rows are cut into runs of kRunRows (a constant: the sums' order never depends
// on the grid or the workspace).  A run's partial is len = d (k + 2) + 3
// doubles: [X^T [m o S | m] (d x (k + 1)) | t (d) | gb, L, cnt].  As many runs
// as the workspace holds are in flight; k_fm_fold adds their partials to the
// plan's accumulator in run order and k_fm_finish forms out.
//
// Kernels
//   k_fm_step<KT>   the fused form, d <= 64 (16 / KT): one workgroup (4 waves)
//                   per run.  A tile of 16 rows x d goes from HBM into LDS once
//                   (row stride S = 2 mod 32 doubles).  Forward: wave w takes
//                   the 16-feature chunks w, w + 4, ..; a lane reads the four
//                   doubles of its row as two 16-byte LDS reads (the 16 rows
//                   of a quarter wave fall on 16 distinct bank quads), squares
//                   them in registers and feeds v_mfma_f64_16x16x4f64 for both
//                   images; the four waves' partial products meet in LDS and
//                   are added in wave order.  Epilogue: one thread per row
//                   forms raw, the loss and m (batch selection and label check
//                   there); [m o S | m] is written to LDS (stride CW + 2).
//                   Gradient: wave w owns the feature tiles w, w + 4, .. and
//                   keeps their accumulators (16 x 4 doubles) in registers
//                   over the whole run; MFMA k-step kk of lane group g reads
//                   tile row 8 (g & 1) + 4 (g >> 1) + kk column-wise, so the 32
//                   lanes of a half wave read 32 consecutive-mod-32 doubles.
//                   t runs on the VALU, one thread per feature.
//   k_fm_forward<KT, TRAIN>
//                   the streaming forward: one wave per 16 rows, X from HBM
//                   straight into the MFMA A layout (k_row_gemm's), the same
//                   epilogue.  TRAIN: writes [m o S | m] (rows x (k + 1)) and
//                   (loss, taken) per row.  Otherwise: the models' margin, raw,
//                   probability and prediction.
//   k_fm_grad<KT>   the two-pass gradient: workgroup (run, panel of 64 (16 /
//                   KT) features), operands from HBM / L2 in the MFMA layout one
//                   k-step of 4 rows ahead, the same partial layout.
//   k_fm_fold, k_fm_finish
// No atomics on doubles, every sum has one fixed order: the same bytes on
// every call and for every workspace size.  The only atomic is the integer
// atomicMin of the lowest row whose label is not 0 / 1.  The plan, the batch
// rule and the row epilogue are fm_dev.hpp's, shared with fm_csr.hip (CSR rows).
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "fm_dev.hpp"
#include "row_gemm.hpp"

namespace {

using namespace cyc::rowgemm;
using namespace cyc::fmdev;

constexpr int kFmTileRows = 16;
constexpr int kMaxFmFeatures = 65535;
constexpr int64_t kDefaultWorkspace = (int64_t)256 << 20;
constexpr int64_t kMaxRunsPerRound = 1 << 20;

typedef double double2_a16 __attribute__((ext_vector_type(2), aligned(16)));

inline int fm_kt(int k) { return tiles16(k + 1); }
inline int fm_fused_features(int k) { return 64 * (16 / fm_kt(k)); }
// the tile's row stride in doubles: >= round_up(d, 16), = 2 mod 32
inline int fm_stride(int d) { return (int)cyc::round_up(d, 32) + 2; }

// W[0] = [V | w or 0], W[1] = [V o V | 0], each d x (k + 1)
__global__ __launch_bounds__(256) void k_fm_operands(const double* __restrict__ V,
                                                     const double* __restrict__ w, int d, int k,
                                                     double* __restrict__ W) {
  const int64_t total = (int64_t)d * (k + 1);
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * 256) {
    const int64_t i = e / (k + 1);
    const int c = (int)(e % (k + 1));
    const double v = c < k ? V[i * k + c] : 0.0;
    W[e] = c < k ? v : (w ? w[i] : 0.0);
    W[total + e] = v * v;
  }
}

// ------------------------------------------------------------- the fused form
// X, y: the round's first row; n: the round's rows; firstRow: that row's
// global index.  Workgroup blockIdx.x takes run blockIdx.x of the round.
// LDS (doubles): tile 16 S | red 4 x 2 x 16 x CW | sums 2 x 16 x CW |
// Mt 16 (CW + 2) | mrow 16 | scal 48 | sel 16 ints.
template <int KT>
__global__ __launch_bounds__(256) void k_fm_step(
    const double* __restrict__ X, const double* __restrict__ y, int64_t n, int d, int k,
    const double* __restrict__ Bp, int64_t imgLen, const double* __restrict__ bptr, int loss,
    uint64_t h1, uint64_t thr, int64_t firstRow, int S, double* __restrict__ part, int64_t len,
    unsigned long long* __restrict__ bad) {
  constexpr int CW = 16 * KT, FT = 16 / KT, MS = CW + 2;
  extern __shared__ __attribute__((aligned(16))) double lds[];
  double* tile = lds;
  double* red = tile + 16 * S;
  double* sums = red + 128 * CW;
  double* Mt = sums + 32 * CW;
  double* mrow = Mt + 16 * MS;
  double* scal = mrow + 16;
  int* sel = reinterpret_cast<int*>(scal + 48);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, c = lane & 15;
  const int64_t R0 = (int64_t)blockIdx.x * kFmRunRows, R1 = min(n, R0 + kFmRunRows);
  const int nch = (d + 15) / 16;
  // the columns d .. S of every row stay zero for the whole run
  const int pad = S - d;
  for (int e = tid; e < 16 * pad; e += 256) tile[(e / pad) * S + d + e % pad] = 0.0;
  const double b = bptr ? *bptr : 0.0;
  cyc_double4 acc[FT][KT];
#pragma unroll
  for (int j = 0; j < FT; ++j)
#pragma unroll
    for (int ct = 0; ct < KT; ++ct) acc[j][ct] = cyc_double4{0.0, 0.0, 0.0, 0.0};
  double tacc[4] = {0.0, 0.0, 0.0, 0.0};   // features tid + 256 j (d <= 1024)
  double lossAcc = 0.0, cntAcc = 0.0, gbAcc = 0.0;
  const int q256 = 256 / d, r256 = 256 % d;
  for (int64_t t0 = R0; t0 < R1; t0 += kFmTileRows) {
    __syncthreads();   // the previous tile is read
    if (tid < 16) sel[tid] = (t0 + tid < R1 && fm_take(h1, thr, firstRow + t0 + tid)) ? 1 : 0;
    __syncthreads();
    {
      // the tile's 16 d doubles are contiguous in X: thread e, e + 256, ..;
      // a row outside the batch (or past the run) is not loaded
      const double* src = X + t0 * d;
      int row = tid / d, col = tid % d;
#pragma unroll 8
      for (int e = tid; e < 16 * d; e += 256) {
        double v = 0.0;
        if (sel[row]) v = src[e];
        tile[row * S + col] = v;
        col += r256;
        row += q256;
        if (col >= d) {
          col -= d;
          ++row;
        }
      }
    }
    __syncthreads();
    // forward: this wave's chunks, rows read row-wise
    {
      cyc_double4 a1[KT], a2[KT];
#pragma unroll
      for (int ct = 0; ct < KT; ++ct) {
        a1[ct] = cyc_double4{0.0, 0.0, 0.0, 0.0};
        a2[ct] = cyc_double4{0.0, 0.0, 0.0, 0.0};
      }
      for (int ch = wave; ch < nch; ch += 4) {
        const double2_a16* xr = reinterpret_cast<const double2_a16*>(tile + c * S + ch * 16 + 4 * g);
        const double2_a16 lo = xr[0], hi = xr[1];
        const double x[4] = {lo[0], lo[1], hi[0], hi[1]};
        const double* B1 = Bp + (int64_t)ch * KT * 256 + lane;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
          const double x2 = x[kk] * x[kk];
#pragma unroll
          for (int ct = 0; ct < KT; ++ct) {
            const double b1 = B1[(ct * 4 + kk) * 64];
            const double b2 = B1[imgLen + (ct * 4 + kk) * 64];
            a1[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(x[kk], b1, a1[ct], 0, 0, 0);
            a2[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(x2, b2, a2[ct], 0, 0, 0);
          }
        }
      }
      // lane holds rows g + 4 r, column c of each tile
      double* rw = red + wave * 32 * CW;
#pragma unroll
      for (int ct = 0; ct < KT; ++ct)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          rw[(g + 4 * r) * CW + ct * 16 + c] = a1[ct][r];
          rw[(16 + g + 4 * r) * CW + ct * 16 + c] = a2[ct][r];
        }
    }
    __syncthreads();
    for (int e = tid; e < 32 * CW; e += 256)
      sums[e] = ((red[e] + red[32 * CW + e]) + red[64 * CW + e]) + red[96 * CW + e];
    __syncthreads();
    if (tid < 16) {
      double m = 0.0;
      if (sel[tid]) {
        const double raw = fm_raw(sums + tid * CW, sums + (16 + tid) * CW, k, b);
        double l = 0.0, mm = 0.0;
        if (fm_loss(loss, raw, y[t0 + tid], &l, &mm)) {
          m = mm;
          lossAcc += l;
          cntAcc += 1.0;
          gbAcc += mm;
        } else {
          fm_flag_bad(bad, firstRow + t0 + tid);
        }
      }
      mrow[tid] = m;
    }
    __syncthreads();
    for (int e = tid; e < 16 * CW; e += 256) {
      const int r = e / CW, cc = e % CW;
      Mt[r * MS + cc] = cc < k ? mrow[r] * sums[r * CW + cc] : (cc == k ? mrow[r] : 0.0);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int i = tid + 256 * j;
      if (i < d) {
        double t = tacc[j];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const double x = tile[r * S + i];
          t += mrow[r] * (x * x);
        }
        tacc[j] = t;
      }
    }
    __syncthreads();
    // gradient: this wave's feature tiles, the tile read column-wise
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const int rr = 8 * (g & 1) + 4 * (g >> 1) + kk;
      double bb[KT];
#pragma unroll
      for (int ct = 0; ct < KT; ++ct) bb[ct] = Mt[rr * MS + ct * 16 + c];
#pragma unroll
      for (int j = 0; j < FT; ++j) {
        const int ft = wave + 4 * j;
        if (ft < nch) {
          const double a = tile[rr * S + ft * 16 + c];
#pragma unroll
          for (int ct = 0; ct < KT; ++ct)
            acc[j][ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bb[ct], acc[j][ct], 0, 0, 0);
        }
      }
    }
  }
  // lane holds features 16 ft + g + 4 r, column 16 ct + c
  double* out = part + (int64_t)blockIdx.x * len;
#pragma unroll
  for (int j = 0; j < FT; ++j)
#pragma unroll
    for (int ct = 0; ct < KT; ++ct)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = (wave + 4 * j) * 16 + g + 4 * r, col = ct * 16 + c;
        if (i < d && col <= k) out[(int64_t)i * (k + 1) + col] = acc[j][ct][r];
      }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int i = tid + 256 * j;
    if (i < d) out[(int64_t)d * (k + 1) + i] = tacc[j];
  }
  if (tid < 16) {
    scal[tid] = gbAcc;
    scal[16 + tid] = lossAcc;
    scal[32 + tid] = cntAcc;
  }
  __syncthreads();
  if (tid < 3) {
    double s = 0.0;
    for (int r = 0; r < 16; ++r) s += scal[tid * 16 + r];
    out[(int64_t)d * (k + 2) + tid] = s;
  }
}

// --------------------------------------------------- the streaming forward
// One wave per 16 rows, 64 rows per workgroup pass.  LDS (doubles): per wave
// 2 x 16 x CW sums, then mrow 64.  TRAIN: M (n x (k + 1)) = [m o S | m] and
// aux (n x 2) = (loss, taken); otherwise the models' outputs (any may be null):
// margin (n), raw2 (n x 2) = (-raw, raw), prob2 = (1 - p, p), pred = raw
// (squared) or raw > 0 ? 1 : 0 (logistic).
template <int KT, bool TRAIN>
__global__ __launch_bounds__(256) void k_fm_forward(
    const double* __restrict__ X, const double* __restrict__ y, int64_t n, int d, int k,
    const double* __restrict__ Bp, int64_t imgLen, const double* __restrict__ bptr, int loss,
    uint64_t h1, uint64_t thr, int64_t firstRow, double* __restrict__ M, double* __restrict__ aux,
    unsigned long long* __restrict__ bad, double* __restrict__ margin, double* __restrict__ raw2,
    double* __restrict__ prob2, double* __restrict__ pred) {
  constexpr int CW = 16 * KT;
  extern __shared__ double lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, c = lane & 15;
  double* sw = lds + wave * 32 * CW;
  double* mrow = lds + 128 * CW + wave * 16;
  const int nfull = d / 16, nch = (d + 15) / 16;
  const double b = bptr ? *bptr : 0.0;
  const int64_t passes = (n + 63) / 64;
  for (int64_t w = blockIdx.x; w < passes; w += gridDim.x) {
    const int64_t r0 = w * 64 + wave * 16, row = r0 + c;
    const bool take = row < n && (!TRAIN || fm_take(h1, thr, firstRow + row));
    const double* xp = X + (take ? row : 0) * d;
    cyc_double4 a1[KT], a2[KT];
#pragma unroll
    for (int ct = 0; ct < KT; ++ct) {
      a1[ct] = cyc_double4{0.0, 0.0, 0.0, 0.0};
      a2[ct] = cyc_double4{0.0, 0.0, 0.0, 0.0};
    }
    for (int ch = 0; ch < nch; ++ch) {
      const int f0 = ch * 16 + 4 * g;
      double x[4] = {0.0, 0.0, 0.0, 0.0};
      if (take) {   // a row outside the batch is not loaded
        if (ch < nfull) {
          const double4_a8 v = *reinterpret_cast<const double4_a8*>(xp + f0);
#pragma unroll
          for (int j = 0; j < 4; ++j) x[j] = v[j];
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (f0 + j < d) x[j] = xp[f0 + j];
        }
      }
      const double* B1 = Bp + (int64_t)ch * KT * 256 + lane;
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        const double x2 = x[kk] * x[kk];
#pragma unroll
        for (int ct = 0; ct < KT; ++ct) {
          const double b1 = B1[(ct * 4 + kk) * 64];
          const double b2 = B1[imgLen + (ct * 4 + kk) * 64];
          a1[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(x[kk], b1, a1[ct], 0, 0, 0);
          a2[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(x2, b2, a2[ct], 0, 0, 0);
        }
      }
    }
    __syncthreads();   // the previous pass's sums are read
#pragma unroll
    for (int ct = 0; ct < KT; ++ct)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        sw[(g + 4 * r) * CW + ct * 16 + c] = a1[ct][r];
        sw[(16 + g + 4 * r) * CW + ct * 16 + c] = a2[ct][r];
      }
    __syncthreads();
    if (lane < 16) {
      double m = 0.0, l = 0.0, cnt = 0.0;
      const double raw = fm_raw(sw + lane * CW, sw + (16 + lane) * CW, k, b);
      if constexpr (TRAIN) {
        if (take) {
          double mm = 0.0;
          if (fm_loss(loss, raw, y[row], &l, &mm)) {
            m = mm;
            cnt = 1.0;
          } else {
            l = 0.0;
            fm_flag_bad(bad, firstRow + row);
          }
        }
        mrow[lane] = m;
        if (row < n) {
          aux[2 * row] = l;
          aux[2 * row + 1] = cnt;
        }
      } else if (row < n) {
        const double p = 1.0 / (1.0 + exp(-raw));
        if (margin) margin[row] = raw;
        if (raw2) {
          raw2[2 * row] = -raw;
          raw2[2 * row + 1] = raw;
        }
        if (prob2) {
          prob2[2 * row] = 1.0 - p;
          prob2[2 * row + 1] = p;
        }
        if (pred) pred[row] = loss == kLossLogistic ? (raw > 0.0 ? 1.0 : 0.0) : raw;
      }
    }
    if constexpr (TRAIN) {
      __syncthreads();
      for (int e = lane; e < 16 * (k + 1); e += 64) {
        const int r = e / (k + 1), cc = e % (k + 1);
        if (r0 + r < n)
          M[(r0 + r) * (k + 1) + cc] = cc < k ? mrow[r] * sw[r * CW + cc] : mrow[r];
      }
    }
  }
}

// ------------------------------------------------------ the two-pass gradient
// Workgroup blockIdx.x = run x panels + panel: wave w of panel p owns the
// feature tiles 4 FT p + w + 4 j, j < FT = 16 / KT.  Rows of the run in MFMA
// k-steps of 4 (lane group g takes row rb + g), one step ahead.
template <int KT>
__global__ __launch_bounds__(256) void k_fm_grad(const double* __restrict__ X, int64_t n, int d,
                                                 int k, const double* __restrict__ M,
                                                 const double* __restrict__ aux, int panels,
                                                 double* __restrict__ part, int64_t len) {
  constexpr int FT = 16 / KT;
  __shared__ double sh[3][256];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, c = lane & 15;
  const int64_t run = blockIdx.x / panels;
  const int panel = (int)(blockIdx.x % panels);
  const int64_t R0 = run * kFmRunRows, R1 = min(n, R0 + kFmRunRows);
  int feat[FT];
  bool fok[FT];
#pragma unroll
  for (int j = 0; j < FT; ++j) {
    feat[j] = (4 * FT * panel + wave + 4 * j) * 16 + c;
    fok[j] = feat[j] < d;
  }
  auto load = [&](int64_t rb, double (&a)[FT], double (&bb)[KT], double& mm) {
    const int64_t row = rb + g;
    const bool rok = row < R1 && aux[2 * row + 1] != 0.0;   // a row outside the batch is not loaded
    const double* mr = M + row * (k + 1);
    const double* xr = X + row * d;
#pragma unroll
    for (int ct = 0; ct < KT; ++ct) bb[ct] = (rok && ct * 16 + c <= k) ? mr[ct * 16 + c] : 0.0;
    mm = rok ? mr[k] : 0.0;
#pragma unroll
    for (int j = 0; j < FT; ++j) a[j] = (rok && fok[j]) ? xr[feat[j]] : 0.0;
  };
  cyc_double4 acc[FT][KT];
  double tl[FT];
#pragma unroll
  for (int j = 0; j < FT; ++j) {
    tl[j] = 0.0;
#pragma unroll
    for (int ct = 0; ct < KT; ++ct) acc[j][ct] = cyc_double4{0.0, 0.0, 0.0, 0.0};
  }
  double a[FT], an[FT], bb[KT], bn[KT], mm, mn;
  load(R0, a, bb, mm);
  for (int64_t rb = R0; rb < R1; rb += 4) {
    load(rb + 4, an, bn, mn);
#pragma unroll
    for (int j = 0; j < FT; ++j) {
#pragma unroll
      for (int ct = 0; ct < KT; ++ct)
        acc[j][ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[j], bb[ct], acc[j][ct], 0, 0, 0);
      tl[j] += mm * (a[j] * a[j]);
    }
#pragma unroll
    for (int j = 0; j < FT; ++j) a[j] = an[j];
#pragma unroll
    for (int ct = 0; ct < KT; ++ct) bb[ct] = bn[ct];
    mm = mn;
  }
  double* out = part + run * len;
#pragma unroll
  for (int j = 0; j < FT; ++j) {
#pragma unroll
    for (int ct = 0; ct < KT; ++ct)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = feat[j] - c + g + 4 * r, col = ct * 16 + c;
        if (i < d && col <= k) out[(int64_t)i * (k + 1) + col] = acc[j][ct][r];
      }
    // t: the four lane groups' rows, in group order
    const double v1 = __shfl(tl[j], c + 16), v2 = __shfl(tl[j], c + 32),
                 v3 = __shfl(tl[j], c + 48);
    if (g == 0 && fok[j]) out[(int64_t)d * (k + 1) + feat[j]] = ((tl[j] + v1) + v2) + v3;
  }
  if (panel == 0) {   // gb, L, cnt of the run: thread t's rows in order, then a fixed tree
    double s[3] = {0.0, 0.0, 0.0};
    for (int64_t row = R0 + tid; row < R1; row += 256) {
      s[0] += M[row * (k + 1) + k];
      s[1] += aux[2 * row];
      s[2] += aux[2 * row + 1];
    }
    for (int q = 0; q < 3; ++q) sh[q][tid] = s[q];
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
      if (tid < h)
        for (int q = 0; q < 3; ++q) sh[q][tid] += sh[q][tid + h];
      __syncthreads();
    }
    if (tid < 3) out[(int64_t)d * (k + 2) + tid] = sh[tid][0];
  }
}

// accum[e] += part[0][e] + part[1][e] + .. one add at a time, in run order
__global__ __launch_bounds__(256) void k_fm_fold(const double* __restrict__ part, int64_t runs,
                                                 int64_t len, double* __restrict__ accum) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= len) return;
  double s = accum[e];
  for (int64_t r = 0; r < runs; ++r) s += part[r * len + e];
  accum[e] = s;
}

// out = [P - V o t | gw | gb | L | cnt]
__global__ __launch_bounds__(256) void k_fm_finish(const double* __restrict__ accum,
                                                   const double* __restrict__ V, int d, int k,
                                                   int fitLinear, int fitIntercept,
                                                   double* __restrict__ out) {
  const int64_t dk = (int64_t)d * k, base = (int64_t)d * (k + 2);
  const int64_t total = dk + (fitLinear ? d : 0) + (fitIntercept ? 1 : 0) + 2;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * 256) {
    double v;
    if (e < dk) {
      const int64_t i = e / k;
      v = accum[i * (k + 1) + e % k] - V[e] * accum[(int64_t)d * (k + 1) + i];
    } else if (fitLinear && e < dk + d) {
      v = accum[(e - dk) * (k + 1) + k];
    } else if (fitIntercept && e == total - 3) {
      v = accum[base];
    } else {
      v = accum[base + 1 + (e - (total - 2))];
    }
    out[e] = v;
  }
}

size_t step_lds_bytes(int d, int KT) {
  return sizeof(double) * (size_t)(16 * fm_stride(d) + 176 * 16 * KT + 104);
}
size_t forward_lds_bytes(int KT) { return sizeof(double) * (size_t)(128 * 16 * KT + 64); }

template <class K>
int allow_lds(K kernel, size_t bytes) {
  CYC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  return CYC_OK;
}

#define CYC_FM_KT(KT_, CALL) \
  switch (KT_) {             \
    case 1: { constexpr int KT = 1; CALL; } break; \
    case 2: { constexpr int KT = 2; CALL; } break; \
    case 3: { constexpr int KT = 3; CALL; } break; \
    case 4: { constexpr int KT = 4; CALL; } break; \
    default: { constexpr int KT = 5; CALL; } break; \
  }

// the dense kernels' limit (a plan itself may hold any d, for CSR rows)
int check_dense_features(const cyc_fm_plan_s* p) {
  CYC_REQUIRE(p->d <= kMaxFmFeatures, "FM supports 1 to " + std::to_string(kMaxFmFeatures) +
                                          " features but got " + std::to_string(p->d));
  return CYC_OK;
}

// the two operand images of this call's coefficients
int pack_operands(cyc_fm_plan_s* p, const Coef& c, hipStream_t st) {
  const int d = p->d, k = p->k;
  const int64_t per = (int64_t)d * (k + 1), imgLen = packed_len(d, k + 1);
  if (int rc = p->dense.reserve(sizeof(double) * 2 * (size_t)per)) return rc;
  if (int rc = p->image.reserve(sizeof(double) * 2 * (size_t)imgLen)) return rc;
  hipLaunchKernelGGL(k_fm_operands, dim3((unsigned)std::min<int64_t>((per + 255) / 256, 4096)),
                     dim3(256), 0, st, c.V, c.w, d, k, (double*)p->dense.ptr);
  CYC_LAUNCH_CHECK("k_fm_operands");
  return pack((const double*)p->dense.ptr, d, k + 1, k + 1, 1, 2, per, (double*)p->image.ptr, st);
}

}  // namespace

extern "C" {

int cyc_fm_run_rows(void) { return kFmRunRows; }
int cyc_fm_tile_rows(void) { return kFmTileRows; }
int cyc_fm_max_factors(void) { return kMaxFactors; }
int cyc_fm_max_features(void) { return kMaxFmFeatures; }
int cyc_fm_fused_features(int32_t factorSize) {
  return (factorSize < 1 || factorSize > kMaxFactors) ? 0 : fm_fused_features(factorSize);
}

int cyc_fm_plan_create(int32_t numFeatures, int32_t factorSize, int32_t fitIntercept,
                       int32_t fitLinear, int32_t loss, int64_t workspaceBytes, cyc_fm_plan* plan) {
  CYC_REQUIRE(plan != nullptr, "plan must not be null");
  // the dense calls refuse d > cyc_fm_max_features themselves; CSR rows
  // (fm_csr.hip) take any d
  CYC_REQUIRE(numFeatures >= 1, "FM needs at least one feature but got " +
                                    std::to_string(numFeatures));
  CYC_REQUIRE(factorSize >= 1 && factorSize <= kMaxFactors,
              "factorSize must be in [1, " + std::to_string(kMaxFactors) + "] but got " +
                  std::to_string(factorSize));
  CYC_REQUIRE(loss == kLossSquared || loss == kLossLogistic,
              "loss must be 0 (squared) or 1 (logistic) but got " + std::to_string(loss));
  CYC_REQUIRE(workspaceBytes >= 0, "workspaceBytes must not be negative");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    cyc::set_error("no HIP device visible");
    return CYC_ERR_NO_DEVICE;
  }
  auto* p = new cyc_fm_plan_s();
  p->d = numFeatures;
  p->k = factorSize;
  p->fitIntercept = fitIntercept != 0;
  p->fitLinear = fitLinear != 0;
  p->loss = loss;
  p->wsBytes = workspaceBytes ? workspaceBytes : kDefaultWorkspace;
  *plan = p;
  return CYC_OK;
}

int cyc_fm_plan_destroy(cyc_fm_plan plan) {
  delete plan;
  return CYC_OK;
}

int cyc_fm_evaluate_dev(cyc_fm_plan plan, const double* X, const double* y, int64_t nrows,
                        const double* coef, int64_t iter, double fraction, int64_t rowOffset,
                        double* out, void* stream) {
  if (int rc = fm_check_evaluate(plan, nrows, rowOffset, coef, out, fraction)) return rc;
  CYC_REQUIRE(nrows == 0 || (X != nullptr && y != nullptr), "non-null rows and labels");
  cyc_fm_plan_s* p = plan;
  if (int rc = check_dense_features(p)) return rc;
  hipStream_t st = cyc::as_stream(stream);
  std::lock_guard<std::mutex> guard(p->mu);
  const int d = p->d, k = p->k, KTv = fm_kt(k);
  const int64_t len = (int64_t)d * (k + 2) + 3, imgLen = packed_len(d, k + 1);
  const Coef c = split_coef(p, coef);
  if (int rc = p->accum.reserve(sizeof(double) * (size_t)len)) return rc;
  CYC_HIP(hipMemsetAsync(p->accum.ptr, 0, sizeof(double) * (size_t)len, st));
  if (int rc = fm_clear_bad(p, st)) return rc;
  double* accum = (double*)p->accum.ptr;
  auto* bad = (unsigned long long*)p->bad.ptr;
  if (nrows > 0) {
    if (int rc = pack_operands(p, c, st)) return rc;
    const double* Bp = (const double*)p->image.ptr;
    const uint64_t thr = fm_threshold(fraction), h1 = fm_seed(iter);
    const bool fused = d <= fm_fused_features(k);
    // a run in flight: its partial, and in the two-pass form its rows of M and aux
    const int64_t perRun = sizeof(double) * (len + (fused ? 0 : (int64_t)kFmRunRows * (k + 3)));
    const int64_t runs = (nrows + kFmRunRows - 1) / kFmRunRows;
    const int64_t perRound =
        std::min(runs, std::min(kMaxRunsPerRound, std::max<int64_t>(1, p->wsBytes / perRun)));
    if (int rc = p->ws.reserve((size_t)(perRound * perRun))) return rc;
    double* part = (double*)p->ws.ptr;
    double* M = part + perRound * len;
    double* aux = M + perRound * kFmRunRows * (k + 1);
    const size_t stepLds = step_lds_bytes(d, KTv), fwdLds = forward_lds_bytes(KTv);
    if (fused) {
      CYC_FM_KT(KTv, if (int rc = allow_lds(k_fm_step<KT>, stepLds)) return rc);
    } else {
      CYC_FM_KT(KTv, if (int rc = allow_lds(k_fm_forward<KT, true>, fwdLds)) return rc);
    }
    const int S = fm_stride(d);
    const int panels = (d + 64 * (16 / KTv) - 1) / (64 * (16 / KTv));
    for (int64_t run0 = 0; run0 < runs; run0 += perRound) {
      const int64_t row0 = run0 * kFmRunRows;
      const int64_t rows = std::min(nrows - row0, perRound * kFmRunRows);
      const int64_t nr = (rows + kFmRunRows - 1) / kFmRunRows;
      const double* Xr = X + row0 * d;
      if (fused) {
        cyc::KernelTimer timer("k_fm_step", st);
        CYC_FM_KT(KTv, hipLaunchKernelGGL((k_fm_step<KT>), dim3((unsigned)nr), dim3(256), stepLds,
                                          st, Xr, y + row0, rows, d, k, Bp, imgLen, c.b, p->loss,
                                          h1, thr, rowOffset + row0, S, part, len, bad));
        CYC_LAUNCH_CHECK("k_fm_step");
      } else {
        {
          cyc::KernelTimer timer("k_fm_forward", st);
          const int64_t grid = std::min<int64_t>((rows + 63) / 64, 16 * (int64_t)cyc::device_cus());
          CYC_FM_KT(KTv, hipLaunchKernelGGL((k_fm_forward<KT, true>), dim3((unsigned)grid),
                                            dim3(256), fwdLds, st, Xr, y + row0, rows, d, k, Bp,
                                            imgLen, c.b, p->loss, h1, thr, rowOffset + row0, M,
                                            aux, bad, nullptr, nullptr, nullptr, nullptr));
          CYC_LAUNCH_CHECK("k_fm_forward");
        }
        cyc::KernelTimer timer("k_fm_grad", st);
        CYC_FM_KT(KTv, hipLaunchKernelGGL((k_fm_grad<KT>), dim3((unsigned)(nr * panels)),
                                          dim3(256), 0, st, Xr, rows, d, k, M, aux, panels, part,
                                          len));
        CYC_LAUNCH_CHECK("k_fm_grad");
      }
      hipLaunchKernelGGL(k_fm_fold, dim3((unsigned)((len + 255) / 256)), dim3(256), 0, st, part, nr,
                         len, accum);
      CYC_LAUNCH_CHECK("k_fm_fold");
    }
  }
  const int64_t total = (int64_t)d * k + (p->fitLinear ? d : 0) + (p->fitIntercept ? 1 : 0) + 2;
  hipLaunchKernelGGL(k_fm_finish, dim3((unsigned)std::min<int64_t>((total + 255) / 256, 4096)),
                     dim3(256), 0, st, accum, c.V, d, k, p->fitLinear, p->fitIntercept, out);
  CYC_LAUNCH_CHECK("k_fm_finish");
  return nrows > 0 ? fm_report_bad(p, st) : CYC_OK;
}

int cyc_fm_predict_dev(cyc_fm_plan plan, const double* X, int64_t nrows, const double* coef,
                       double* margin, double* raw, double* prob, double* pred, void* stream) {
  CYC_REQUIRE(plan != nullptr, "plan must not be null");
  CYC_REQUIRE(nrows >= 0, "nrows >= 0");
  CYC_REQUIRE(coef != nullptr, "coef must not be null");
  CYC_REQUIRE(margin != nullptr || raw != nullptr || prob != nullptr || pred != nullptr,
              "at least one of margin, raw, prob and pred");
  if (nrows == 0) return CYC_OK;
  CYC_REQUIRE(X != nullptr, "non-null rows");
  cyc_fm_plan_s* p = plan;
  if (int rc = check_dense_features(p)) return rc;
  CYC_REQUIRE(p->loss == kLossLogistic || (raw == nullptr && prob == nullptr),
              "raw and prob need a classifier");
  hipStream_t st = cyc::as_stream(stream);
  std::lock_guard<std::mutex> guard(p->mu);
  const int d = p->d, k = p->k, KTv = fm_kt(k);
  const Coef c = split_coef(p, coef);
  if (int rc = pack_operands(p, c, st)) return rc;
  const size_t fwdLds = forward_lds_bytes(KTv);
  CYC_FM_KT(KTv, if (int rc = allow_lds(k_fm_forward<KT, false>, fwdLds)) return rc);
  cyc::KernelTimer timer("k_fm_predict", st);
  const int64_t grid = std::min<int64_t>((nrows + 63) / 64, 16 * (int64_t)cyc::device_cus());
  CYC_FM_KT(KTv, hipLaunchKernelGGL((k_fm_forward<KT, false>), dim3((unsigned)grid), dim3(256),
                                    fwdLds, st, X, nullptr, nrows, d, k,
                                    (const double*)p->image.ptr, packed_len(d, k + 1), c.b, p->loss,
                                    0ull, 0ull, (int64_t)0, nullptr, nullptr, nullptr, margin, raw,
                                    prob, pred));
  CYC_LAUNCH_CHECK("k_fm_predict");
  return CYC_OK;
}

}  // extern "C"
