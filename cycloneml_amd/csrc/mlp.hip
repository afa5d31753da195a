// mlp.hip -- MultilayerPerceptronClassifier on gfx950 (MI355X): the forward
// chain, the softmax / cross-entropy top, delta back-propagation and the
// per-layer weight gradients of ml/ann/Layer.scala and ml/ann/LossFunction
// .scala, for the topology affine + sigmoid (hidden) / affine + softmax (top).
//
// Layouts.  layers = [n_0 .. n_L].  The weights are one flat fp64 array: for
// l = 1..L, W_l (column-major n_l x n_{l-1}: W_l[o, i] at i n_l + o) and then
// b_l (n_l).  Rows, activations and deltas are row-major.  The gradient has
// the weights' layout, so a layer's slice is the column-major n_l x
// (n_{l-1} + 1) matrix [gW_l | gb_l].
//
// Row i of a shard of nrows rows belongs to block b = i / blockSize of S_b =
// min(blockSize, nrows - b blockSize) rows and carries the scale s_i =
// 1 / (S_b B), B = totalBlocks over all ranks: loss += sum_i s_i l_i, grad +=
// sum_i s_i g_i.  Back-propagation is linear in delta_L, so delta_L is scaled
// by s_i once.
//
// Kernels
//   gemm           row_gemm.hpp: pack() writes W_l^T (forward pass) and
//                  W_{l+1} (delta pass) as images once per call, and
//                  k_row_gemm<CT, Epi> computes Y = epilogue(X B) (timer
//                  "k_mlp_gemm").  Sigmoid: 1 / (1 + exp(-(acc + b))), Bias:
//                  acc + b (z_L), Deriv: acc a (1 - a).
//   k_mlp_softmax<LPR, TRAIN>
//                  LPR = 4 / 16 / 64 lanes per row over z_L: max, exp, sum.
//                  TRAIN: -log p_y, delta_L = s_i (p - onehot(y)), the label
//                  check, one loss partial per wave (fold_add folds them in
//                  a fixed order).  Otherwise raw / probability / argmax
//                  (lowest index on ties).
//   k_mlp_grad<MT, NT>
//                  [gW_l | gb_l] = D_l^T [A_{l-1} | 1] on v_mfma_f64_16x16x4f64,
//                  split-K over rows: one wave per (16 MT x 16 NT tile, row
//                  split), operands straight from HBM / L2 one k-step ahead;
//                  the bias gradient is the column of ones.  k_mlp_fold_grad
//                  adds the slabs in split order.
// No atomics: every sum has one fixed order, so two calls on the same inputs
// give the same bits.  Padded operand elements are explicit zeros and padded
// accumulators are never stored.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <string>
#include <vector>

#include "common.hpp"
#include "row_gemm.hpp"

struct cyc_mlp_plan_s {
  std::mutex mu;
  std::vector<int> layers;      // n_0 .. n_L
  std::vector<int64_t> woff;    // woff[l]: layer l's slice of the flat weights, l = 1..L
  int L = 0;
  int blockSize = 0;
  int64_t chunkRows = 0;
  int64_t sumN = 0;             // n_1 + .. + n_L
  int64_t wlen = 0;
  std::vector<int64_t> pfOff, pbOff;   // packed W_l^T / W_l (doubles), l = 1..L
  int64_t pfLen = 0, pbLen = 0;
  cyc::DeviceBuffer ws, packF, packB, slab, lossSlab, flag;
};

namespace {

using namespace cyc::rowgemm;

constexpr int kMaxWidth = 4096;
constexpr int64_t kWorkspaceBytes = (int64_t)1 << 30;
constexpr int kLossBlocks = 1024;           // k_mlp_softmax grid cap (4 waves each)

// k_row_gemm's epilogues.  bias: the layer's k biases; act: the activations
// (nrows x k).  The sigmoid keeps 4 waves per SIMD at CT = 1 only (its exp
// spills at 128 registers beside two tiles' accumulators).
struct Sigmoid {
  static constexpr int kWideCT = 1;
  const double* bias;
  __device__ double operator()(double v, int64_t, int col, int) const {
    return 1.0 / (1.0 + exp(-(v + bias[col])));
  }
};
struct Bias {
  static constexpr int kWideCT = 2;
  const double* bias;
  __device__ double operator()(double v, int64_t, int col, int) const { return v + bias[col]; }
};
struct Deriv {
  static constexpr int kWideCT = 2;
  const double* act;
  __device__ double operator()(double v, int64_t row, int col, int k) const {
    const double a = act[row * k + col];
    return v * (a * (1.0 - a));
  }
};

// One row of z_L (C classes) per LPR lanes.  Rows [0, nrows) of a chunk that
// starts at row row0 of a shard of shardRows rows.
// TRAIN: D = s_i (p - onehot(y)), lossSlab[wave] = sum of the wave's s_i l_i
// (its rows in order, then a fixed shuffle tree); a label that is not an
// integer in [0, C) sets *flag and contributes nothing.
// Otherwise raw = z, prob = p, pred = argmax p (any of them may be null).
template <int LPR, bool TRAIN>
__global__ __launch_bounds__(256) void k_mlp_softmax(
    const double* __restrict__ Z, int64_t nrows, int C, const double* __restrict__ labels,
    int64_t row0, int64_t shardRows, int64_t blockSize, double totalBlocks,
    double* __restrict__ D, double* __restrict__ lossSlab, int* __restrict__ flag,
    double* __restrict__ raw, double* __restrict__ prob, double* __restrict__ pred) {
  constexpr int RPW = 64 / LPR;   // rows per wave
  const int lane = threadIdx.x & 63, sl = lane % LPR, sub = lane / LPR;
  const int64_t gw = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t stride = (int64_t)gridDim.x * 4 * RPW;
  double lossAcc = 0.0;
  for (int64_t rb = gw * RPW; rb < nrows; rb += stride) {
    const int64_t row = rb + sub;
    const bool ok = row < nrows;
    const double* z = Z + (ok ? row : nrows - 1) * C;
    double m = -__builtin_inf();
    for (int c = sl; c < C; c += LPR) m = fmax(m, z[c]);
#pragma unroll
    for (int s = 1; s < LPR; s <<= 1) m = fmax(m, __shfl_xor(m, s));
    double sum = 0.0;
    for (int c = sl; c < C; c += LPR) sum += exp(z[c] - m);
#pragma unroll
    for (int s = 1; s < LPR; s <<= 1) sum += __shfl_xor(sum, s);
    if constexpr (TRAIN) {
      const double y = ok ? labels[row] : 0.0;
      const bool yok = y >= 0.0 && y < (double)C && y == floor(y);
      const int yc = yok ? (int)y : -1;
      const int64_t gi = row0 + row;
      const int64_t b = gi / blockSize;
      const int64_t Sb = min<int64_t>(blockSize, shardRows - b * blockSize);
      const double s = 1.0 / ((double)Sb * totalBlocks);
      double py = 0.0;
      for (int c = sl; c < C; c += LPR) {
        const double p = exp(z[c] - m) / sum;
        if (c == yc) py = p;
        if (ok) D[row * C + c] = s * (c == yc ? p - 1.0 : p);
      }
#pragma unroll
      for (int t = 1; t < LPR; t <<= 1) py += __shfl_xor(py, t);   // one lane's p_y, else 0
      if (ok && sl == 0) {
        if (yok) lossAcc += s * -log(py);
        else *flag = 1;
      }
    } else {
      double best = -__builtin_inf();
      int bi = 0x7fffffff;
      for (int c = sl; c < C; c += LPR) {
        const double p = exp(z[c] - m) / sum;
        if (ok && raw) raw[row * C + c] = z[c];
        if (ok && prob) prob[row * C + c] = p;
        if (p > best) {
          best = p;
          bi = c;
        }
      }
#pragma unroll
      for (int t = 1; t < LPR; t <<= 1) {
        const double ob = __shfl_xor(best, t);
        const int oi = __shfl_xor(bi, t);
        if (ob > best || (ob == best && oi < bi)) {
          best = ob;
          bi = oi;
        }
      }
      if (ok && pred && sl == 0) pred[row] = bi == 0x7fffffff ? 0.0 : (double)bi;
    }
  }
  if constexpr (TRAIN) {
#pragma unroll
    for (int t = LPR; t < 64; t <<= 1) lossAcc += __shfl_xor(lossAcc, t);
    if (lane == 0) lossSlab[gw] = lossAcc;
  }
}

// slab[sp][o + j no] = sum over rows [sp rps, (sp + 1) rps) of D[r][o] Aj[r],
// Aj = A[r][j] for j < ni and 1 for j = ni: the column-major no x (ni + 1)
// slice [gW | gb] of one layer.  One wave per (tile, split): 16 MT outputs x
// 16 NT inputs, operands from memory in the MFMA layout (A operand: lane =
// output l & 15 of row 4 kk + (l >> 4); B operand: input l & 15 of that row),
// one k-step of 4 rows ahead.  Waves of a workgroup share the input tile and
// split; logical workgroups are dealt so that neighbours share an XCD's L2.
template <int MT, int NT>
__global__ __launch_bounds__(256) void k_mlp_grad(const double* __restrict__ D,
                                                  const double* __restrict__ A, int64_t rows,
                                                  int no, int ni, int64_t rps, int64_t splits,
                                                  int ot, int jt, int64_t nblocks,
                                                  double* __restrict__ slab) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, c = lane & 15;
  const int64_t nb8 = (nblocks + 7) / 8;
  const int64_t lb = (int64_t)(blockIdx.x & 7) * nb8 + (blockIdx.x >> 3);
  const int64_t tiles = (int64_t)ot * jt;
  const int64_t w = lb * 4 + wave;
  if (lb >= nblocks || w >= tiles * splits) return;
  const int tile = (int)(w % tiles);
  const int64_t sp = w / tiles;
  const int o0 = (tile % ot) * 16 * MT, j0 = (tile / ot) * 16 * NT;
  const int64_t r0 = sp * rps, r1 = min<int64_t>(rows, r0 + rps);
  bool aok[MT], bok[NT], one[NT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) aok[mt] = o0 + 16 * mt + c < no;
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    bok[nt] = j0 + 16 * nt + c < ni;
    one[nt] = j0 + 16 * nt + c == ni;
  }
  auto load = [&](int64_t rb, double (&a)[MT], double (&b)[NT]) {
    const int64_t row = rb + g;
    const bool rok = row < r1;
    const double* d = D + row * no + o0 + c;
    const double* x = A + row * ni + j0 + c;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) a[mt] = (rok && aok[mt]) ? d[16 * mt] : 0.0;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
      b[nt] = (rok && bok[nt]) ? x[16 * nt] : ((rok && one[nt]) ? 1.0 : 0.0);
  };
  cyc_double4 acc[MT][NT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = cyc_double4{0.0, 0.0, 0.0, 0.0};
  double a[MT], b[NT], an[MT], bn[NT];
  load(r0, a, b);
  for (int64_t rb = r0; rb < r1; rb += 4) {
    load(rb + 4, an, bn);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
        acc[mt][nt] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[mt], b[nt], acc[mt][nt], 0, 0, 0);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) a[mt] = an[mt];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) b[nt] = bn[nt];
  }
  // lane holds outputs o0 + 16 mt + g + 4 r, input j0 + 16 nt + c
  double* out = slab + sp * ((int64_t)no * (ni + 1));
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const int j = j0 + 16 * nt + c;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int o = o0 + 16 * mt + g + 4 * r;
        if (o < no && j <= ni) out[o + (int64_t)j * no] = acc[mt][nt][r];
      }
    }
}

// grad[e] += slab[0][e] + slab[1][e] + .. (split order)
__global__ __launch_bounds__(256) void k_mlp_fold_grad(const double* __restrict__ slab,
                                                       int64_t splits, int64_t len,
                                                       double* __restrict__ grad) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < len;
       e += (int64_t)gridDim.x * 256) {
    double s = 0.0;
    for (int64_t sp = 0; sp < splits; ++sp) s += slab[sp * len + e];
    grad[e] += s;
  }
}

template <bool TRAIN>
int softmax(const double* Z, int64_t nrows, int C, const double* labels, int64_t row0,
            int64_t shardRows, int64_t blockSize, double totalBlocks, double* D, double* lossSlab,
            int* flag, double* raw, double* prob, double* pred, int64_t* waves, hipStream_t st) {
  const int lpr = C <= 4 ? 4 : (C <= 16 ? 16 : 64);
  const int64_t need = (nrows + 64 / lpr - 1) / (64 / lpr);   // waves
  const int64_t grid = std::min<int64_t>((need + 3) / 4, kLossBlocks);
  if (waves) *waves = grid * 4;
#define CYC_MLP_SOFTMAX(LPR)                                                                   \
  hipLaunchKernelGGL((k_mlp_softmax<LPR, TRAIN>), dim3((unsigned)grid), dim3(256), 0, st, Z,   \
                     nrows, C, labels, row0, shardRows, blockSize, totalBlocks, D, lossSlab,   \
                     flag, raw, prob, pred)
  if (lpr == 4) CYC_MLP_SOFTMAX(4);
  else if (lpr == 16) CYC_MLP_SOFTMAX(16);
  else CYC_MLP_SOFTMAX(64);
#undef CYC_MLP_SOFTMAX
  CYC_LAUNCH_CHECK("k_mlp_softmax");
  return CYC_OK;
}

template <int MT, int NT>
void launch_grad(const double* D, const double* A, int64_t rows, int no, int ni, int64_t rps,
                 int64_t splits, double* slab, hipStream_t st) {
  const int ot = (no + 16 * MT - 1) / (16 * MT), jt = (ni + 1 + 16 * NT - 1) / (16 * NT);
  const int64_t nblocks = ((int64_t)ot * jt * splits + 3) / 4;
  hipLaunchKernelGGL((k_mlp_grad<MT, NT>), dim3((unsigned)((nblocks + 7) / 8 * 8)), dim3(256), 0,
                     st, D, A, rows, no, ni, rps, splits, ot, jt, nblocks, slab);
}

// grad (the layer's slice, no x (ni + 1) column-major) += D^T [A | 1] over
// `rows` rows
int layer_grad(cyc_mlp_plan_s* p, const double* D, const double* A, int64_t rows, int no, int ni,
               double* grad, hipStream_t st) {
  const int MT = no > 16 ? 2 : 1;
  const int NT = ni + 1 > 32 ? 4 : (ni + 1 > 16 ? 2 : 1);
  const int64_t tiles = (int64_t)((no + 16 * MT - 1) / (16 * MT)) *
                        ((ni + 1 + 16 * NT - 1) / (16 * NT));
  // four waves per SIMD over the device, at least 64 rows per split
  const int64_t want = 16 * (int64_t)cyc::device_cus();
  int64_t splits = std::max<int64_t>(1, (want + tiles - 1) / tiles);
  splits = std::min<int64_t>(splits, std::max<int64_t>(1, rows / 64));
  const int64_t rps = cyc::round_up((rows + splits - 1) / splits, 4);
  splits = (rows + rps - 1) / rps;
  const int64_t len = (int64_t)no * (ni + 1);
  if (int rc = p->slab.reserve(sizeof(double) * (size_t)splits * (size_t)len)) return rc;
  double* slab = (double*)p->slab.ptr;
  {
    cyc::KernelTimer timer("k_mlp_grad", st);
    if (MT == 1 && NT == 1) launch_grad<1, 1>(D, A, rows, no, ni, rps, splits, slab, st);
    else if (MT == 1 && NT == 2) launch_grad<1, 2>(D, A, rows, no, ni, rps, splits, slab, st);
    else if (MT == 1) launch_grad<1, 4>(D, A, rows, no, ni, rps, splits, slab, st);
    else if (NT == 1) launch_grad<2, 1>(D, A, rows, no, ni, rps, splits, slab, st);
    else if (NT == 2) launch_grad<2, 2>(D, A, rows, no, ni, rps, splits, slab, st);
    else launch_grad<2, 4>(D, A, rows, no, ni, rps, splits, slab, st);
    CYC_LAUNCH_CHECK("k_mlp_grad");
  }
  hipLaunchKernelGGL(k_mlp_fold_grad, dim3((unsigned)std::min<int64_t>((len + 255) / 256, 4096)),
                     dim3(256), 0, st, slab, splits, len, grad);
  CYC_LAUNCH_CHECK("k_mlp_fold_grad");
  return CYC_OK;
}

// the workspace of one chunk: act[l] and delta[l] (chunk x n_l), l = 1..L
struct Workspace {
  std::vector<double*> act, delta;
};

int reserve_workspace(cyc_mlp_plan_s* p, int64_t chunk, bool deltas, Workspace* w) {
  const size_t per = (size_t)chunk * (size_t)p->sumN;
  if (int rc = p->ws.reserve(sizeof(double) * per * (deltas ? 2 : 1))) return rc;
  double* base = (double*)p->ws.ptr;
  w->act.assign(p->L + 1, nullptr);
  w->delta.assign(p->L + 1, nullptr);
  size_t off = 0;
  for (int l = 1; l <= p->L; ++l) {
    w->act[l] = base + off;
    if (deltas) w->delta[l] = base + per + off;
    off += (size_t)chunk * (size_t)p->layers[l];
  }
  return CYC_OK;
}

// W_l^T of every layer (and W_l, l >= 2, for the delta pass) as k_row_gemm images
int pack_weights(cyc_mlp_plan_s* p, const double* weights, bool backward, hipStream_t st) {
  if (int rc = p->packF.reserve(sizeof(double) * (size_t)p->pfLen)) return rc;
  if (backward)
    if (int rc = p->packB.reserve(sizeof(double) * (size_t)p->pbLen)) return rc;
  for (int l = 1; l <= p->L; ++l) {
    const int ni = p->layers[l - 1], no = p->layers[l];
    const double* W = weights + p->woff[l];
    // forward: B(i, o) = W[i no + o]
    if (int rc = pack(W, ni, no, no, 1, 1, 0, (double*)p->packF.ptr + p->pfOff[l], st)) return rc;
    // delta: D_{l-1} = D_l W_l, B(o, i) = W[i no + o]
    if (backward && l >= 2)
      if (int rc = pack(W, no, ni, 1, no, 1, 0, (double*)p->packB.ptr + p->pbOff[l], st)) return rc;
  }
  return CYC_OK;
}

// act[1..L] of `rows` rows of X; act[L] = z_L
int forward_chunk(cyc_mlp_plan_s* p, const double* X, int64_t rows, const double* weights,
                  const Workspace& w, hipStream_t st) {
  const double* in = X;
  for (int l = 1; l <= p->L; ++l) {
    const int ni = p->layers[l - 1], no = p->layers[l];
    const double* Bp = (const double*)p->packF.ptr + p->pfOff[l];
    const double* bias = weights + p->woff[l] + (int64_t)no * ni;
    int rc = l < p->L ? gemm(in, rows, ni, no, Bp, Sigmoid{bias}, w.act[l], "k_mlp_gemm", st)
                      : gemm(in, rows, ni, no, Bp, Bias{bias}, w.act[l], "k_mlp_gemm", st);
    if (rc) return rc;
    in = w.act[l];
  }
  return CYC_OK;
}

}  // namespace

extern "C" {

int cyc_mlp_plan_create(const int32_t* layers, int nlayers, int blockSize, int64_t chunkRows,
                        cyc_mlp_plan* plan) {
  CYC_REQUIRE(plan != nullptr, "plan must not be null");
  CYC_REQUIRE(layers != nullptr && nlayers >= 2,
              "layers must hold at least the input and the output size");
  for (int l = 0; l < nlayers; ++l) {
    CYC_REQUIRE(layers[l] >= 1, "layer sizes must be positive but got " +
                                    std::to_string(layers[l]));
    CYC_REQUIRE(layers[l] <= kMaxWidth, "layer sizes up to " + std::to_string(kMaxWidth) +
                                            " are supported but got " +
                                            std::to_string(layers[l]));
  }
  CYC_REQUIRE(blockSize > 0, "blockSize must be positive but got " + std::to_string(blockSize));
  CYC_REQUIRE(chunkRows >= 0, "chunkRows must not be negative");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    cyc::set_error("no HIP device visible");
    return CYC_ERR_NO_DEVICE;
  }
  auto* p = new cyc_mlp_plan_s();
  p->layers.assign(layers, layers + nlayers);
  p->L = nlayers - 1;
  p->blockSize = blockSize;
  p->woff.assign(nlayers, 0);
  p->pfOff.assign(nlayers, 0);
  p->pbOff.assign(nlayers, 0);
  int64_t all = layers[0];
  for (int l = 1; l <= p->L; ++l) {
    p->woff[l] = p->wlen;
    p->wlen += (int64_t)layers[l] * (layers[l - 1] + 1);
    p->sumN += layers[l];
    all += layers[l];
    p->pfOff[l] = p->pfLen;
    p->pfLen += packed_len(layers[l - 1], layers[l]);
    if (l >= 2) {
      p->pbOff[l] = p->pbLen;
      p->pbLen += packed_len(layers[l], layers[l - 1]);
    }
  }
  // 2 chunkRows sum(n_l) doubles within the cap; whole row tiles when it allows
  if (chunkRows == 0) {
    chunkRows = std::max<int64_t>(1, kWorkspaceBytes / (16 * all));
    if (chunkRows > kTileRows) chunkRows -= chunkRows % kTileRows;
  }
  p->chunkRows = chunkRows;
  *plan = p;
  return CYC_OK;
}

int cyc_mlp_plan_destroy(cyc_mlp_plan plan) {
  delete plan;
  return CYC_OK;
}

int cyc_mlp_loss_grad_dev(cyc_mlp_plan plan, const double* X, const double* labels, int64_t nrows,
                          const double* weights, int64_t totalBlocks, double* grad, double* loss,
                          void* stream) {
  CYC_REQUIRE(plan != nullptr, "plan must not be null");
  CYC_REQUIRE(nrows >= 0, "nrows >= 0");
  CYC_REQUIRE(totalBlocks >= 1, "totalBlocks must be positive but got " +
                                    std::to_string(totalBlocks));
  CYC_REQUIRE(weights != nullptr && grad != nullptr && loss != nullptr,
              "weights, grad and loss must not be null");
  if (nrows == 0) return CYC_OK;
  CYC_REQUIRE(X != nullptr && labels != nullptr, "non-null rows and labels");
  cyc_mlp_plan_s* p = plan;
  hipStream_t st = cyc::as_stream(stream);
  std::lock_guard<std::mutex> g(p->mu);
  const int L = p->L, C = p->layers[L];
  const int64_t chunk = std::min(p->chunkRows, nrows);
  Workspace w;
  if (int rc = reserve_workspace(p, chunk, true, &w)) return rc;
  if (int rc = p->lossSlab.reserve(sizeof(double) * kLossBlocks * 4)) return rc;
  if (int rc = p->flag.reserve(sizeof(int))) return rc;
  CYC_HIP(hipMemsetAsync(p->flag.ptr, 0, sizeof(int), st));
  if (int rc = pack_weights(p, weights, true, st)) return rc;
  for (int64_t r0 = 0; r0 < nrows; r0 += chunk) {
    const int64_t rows = std::min(chunk, nrows - r0);
    const double* Xc = X + r0 * p->layers[0];
    if (int rc = forward_chunk(p, Xc, rows, weights, w, st)) return rc;
    int64_t waves = 0;
    if (int rc = softmax<true>(w.act[L], rows, C, labels + r0, r0, nrows, p->blockSize,
                               (double)totalBlocks, w.delta[L], (double*)p->lossSlab.ptr,
                               (int*)p->flag.ptr, nullptr, nullptr, nullptr, &waves, st))
      return rc;
    if (int rc = fold_add((const double*)p->lossSlab.ptr, waves, loss, st)) return rc;
    for (int l = L; l >= 1; --l) {
      const int ni = p->layers[l - 1], no = p->layers[l];
      if (l >= 2) {   // D_{l-1} = (D_l W_l) a_{l-1} (1 - a_{l-1})
        const double* Bp = (const double*)p->packB.ptr + p->pbOff[l];
        if (int rc = gemm(w.delta[l], rows, no, ni, Bp, Deriv{w.act[l - 1]}, w.delta[l - 1],
                          "k_mlp_gemm", st))
          return rc;
      }
      if (int rc = layer_grad(p, w.delta[l], l >= 2 ? w.act[l - 1] : Xc, rows, no, ni,
                              grad + p->woff[l], st))
        return rc;
    }
  }
  int bad = 0;
  CYC_HIP(hipMemcpyAsync(&bad, p->flag.ptr, sizeof(int), hipMemcpyDeviceToHost, st));
  CYC_HIP(hipStreamSynchronize(st));
  CYC_REQUIRE(bad == 0, "Classifier found a label that is not an integer in [0, " +
                            std::to_string(C) + ")");
  return CYC_OK;
}

int cyc_mlp_forward_dev(cyc_mlp_plan plan, const double* X, int64_t nrows, const double* weights,
                        double* raw, double* prob, double* pred, void* stream) {
  CYC_REQUIRE(plan != nullptr, "plan must not be null");
  CYC_REQUIRE(nrows >= 0, "nrows >= 0");
  CYC_REQUIRE(weights != nullptr, "weights must not be null");
  CYC_REQUIRE(raw != nullptr || prob != nullptr || pred != nullptr,
              "at least one of raw, prob and pred");
  if (nrows == 0) return CYC_OK;
  CYC_REQUIRE(X != nullptr, "non-null rows");
  cyc_mlp_plan_s* p = plan;
  hipStream_t st = cyc::as_stream(stream);
  std::lock_guard<std::mutex> g(p->mu);
  const int L = p->L, C = p->layers[L];
  const int64_t chunk = std::min(p->chunkRows, nrows);
  Workspace w;
  if (int rc = reserve_workspace(p, chunk, false, &w)) return rc;
  if (int rc = pack_weights(p, weights, false, st)) return rc;
  for (int64_t r0 = 0; r0 < nrows; r0 += chunk) {
    const int64_t rows = std::min(chunk, nrows - r0);
    if (int rc = forward_chunk(p, X + r0 * p->layers[0], rows, weights, w, st)) return rc;
    if (int rc = softmax<false>(w.act[L], rows, C, nullptr, 0, 0, 1, 1.0, nullptr, nullptr,
                                nullptr, raw ? raw + r0 * C : nullptr,
                                prob ? prob + r0 * C : nullptr, pred ? pred + r0 : nullptr,
                                nullptr, st))
      return rc;
  }
  return CYC_OK;
}

}  // extern "C"
