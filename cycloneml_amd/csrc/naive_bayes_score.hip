// naive_bayes_score.hip -- NaiveBayesModel's predictRaw / predictProbability /
// predict on gfx950 (MI355X) over dense fp64 rows (nrows x d, row-major) for
// the four model types of ml/classification/NaiveBayes.scala.
//
// Operands (device fp64, made on the host by naive_bayes.score_operands so
// that no log / log1p / exp of the model runs here): b (C), M (C x d,
// row-major) and, gaussian only, V (C x d, the variances) and ls (C, the sums
// of log variance).
//   linear forms  t_c = b_c + sum_j x_j M_cj, a term with x_j == 0 skipped
//                 (multinomial: b = pi, M = theta; complement: b = 0;
//                 bernoulli: b = pi + sum_j L_cj, M = theta - L)
//   gaussian      raw_c = b_c - (sum_j (x_j - M_cj)^2 / V_cj + ls_c) / 2
//
// Kernels
//   product path   row_gemm.hpp: pack() writes M^T's image once per model and
//                  k_row_gemm<CT, NbBias> computes b[col] + X M^T (timer
//                  "k_nbs_gemm").  Linear forms with a finite M only: a finite
//                  M_cj times an exact zero adds a signed zero, which is the
//                  skip; a -inf in M would turn it into NaN.
//   k_nbs_plain<GAUSS>
//                  one thread per class and 4 rows, j ascending: a workgroup
//                  owns 64 rows x 16 classes and stages 32 features of the rows
//                  and of the model in LDS at a time.  Gaussian always, written
//                  as (x - theta)^2 / sigma (the expanded form cancels), and
//                  the linear forms as x != 0 ? x M : skip when M has a
//                  non-finite entry (or on request).
//   k_nbs_finish<LPR, COMP>
//                  LPR = 4 / 16 / 64 lanes per row over the C raw values:
//                  complement's t - (max + log sum exp(t - max)) in place, the
//                  probabilities exp(raw - max) / sum, and the argmax (the
//                  first index of the largest value under >, from class 0: a
//                  NaN in class 0 stays the answer).  Each lane sums its
//                  classes c = lane, lane + LPR, .. in order, then a fixed
//                  shuffle tree.
//   k_nbs_check    a streamed pass over X: the lowest row with a value the
//                  model type refuses (atomicMin of row 8 + rule, as the
//                  aggregate of naive_bayes.hip records it).
//   k_nbs_finite   whether M is finite throughout (once per model).
// Rows go through in chunks of chunkRows, whose raw values (chunkRows C
// doubles) fit the workspace when the caller takes no raw.  Every output is
// summed by one thread or one wave in a fixed order: no atomics on doubles,
// the same bits on every call and for every workspace.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <string>
#include <vector>

#include "common.hpp"
#include "row_gemm.hpp"

enum { NBS_MULTINOMIAL = 0, NBS_COMPLEMENT = 1, NBS_BERNOULLI = 2, NBS_GAUSSIAN = 3 };
enum { NBS_AUTO = 0, NBS_PRODUCT = 1, NBS_PLAIN = 2 };

struct cyc_nbmodel_s {
  std::mutex mu;
  int C = 0, d = 0, type = 0, path = 0;
  int64_t chunkRows = 0;
  cyc::DeviceBuffer b, M, V, ls, image, ws, bad;
};

namespace {

using namespace cyc::rowgemm;

constexpr int kMaxClasses = 1024;
constexpr int64_t kDefaultWorkspace = (int64_t)256 << 20;
constexpr unsigned long long kNoBad = ~0ull;
constexpr int kRuleValue = 3;               // cyc_nb_aggregate_dev's rule of a refused value
constexpr int kPlainRows = 64, kPlainClasses = 16, kPlainFeat = 32;
constexpr int kPlainPad = kPlainFeat + 1;   // LDS row stride: lanes of a class group on distinct banks
constexpr int kFinishBlocks = 4096;         // k_nbs_finish grid cap (4 waves each)
constexpr int kCheckBlocks = 8192;
constexpr int kPlainBlocks = 1 << 16;

// k_row_gemm's epilogue: raw = b[col] + sum
struct NbBias {
  static constexpr int kWideCT = 2;
  const double* b;
  __device__ double operator()(double v, int64_t, int col, int) const { return b[col] + v; }
};

__global__ __launch_bounds__(256) void k_nbs_finite(const double* __restrict__ M, int64_t len,
                                                    int* __restrict__ flag) {
  bool bad = false;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < len;
       e += (int64_t)gridDim.x * 256) {
    const double v = M[e];
    bad |= !(v - v == 0.0);   // inf - inf and NaN - NaN are NaN
  }
  if (bad) atomicOr(flag, 1);
}

// values >= 0 (a NaN fails), or exactly 0 / 1 (bern)
__global__ __launch_bounds__(256) void k_nbs_check(const double* __restrict__ X, int64_t total,
                                                   int d, int bern,
                                                   unsigned long long* __restrict__ bad) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t e0 = (int64_t)blockIdx.x * 256 + threadIdx.x; e0 < total; e0 += 4 * stride) {
    double x[4];
    // the four loads before their tests; past the end: a value that passes
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t e = e0 + u * stride;
      x[u] = e < total ? X[e] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const bool ok = bern ? (x[u] == 0.0 || x[u] == 1.0) : (x[u] >= 0.0);
      if (!ok)
        atomicMin(bad, (unsigned long long)((e0 + u * stride) / d) * 8ull +
                           (unsigned long long)kRuleValue);
    }
  }
}

// Z[row C + c] for 64-row tiles (blockIdx.x, grid-stride) x 16 classes
// (blockIdx.y): thread (class tid & 15, rows 4 (tid >> 4) .. + 3)
template <bool GAUSS>
__global__ __launch_bounds__(256) void k_nbs_plain(
    const double* __restrict__ X, int64_t nrows, int d, int C, const double* __restrict__ b,
    const double* __restrict__ M, const double* __restrict__ V, const double* __restrict__ ls,
    double* __restrict__ Z) {
  __shared__ double Xs[kPlainRows][kPlainPad];
  __shared__ double Ms[kPlainClasses][kPlainPad];
  __shared__ double Vs[GAUSS ? kPlainClasses : 1][kPlainPad];
  const int tid = threadIdx.x, c = tid & 15, rg = tid >> 4;
  const int c0 = blockIdx.y * kPlainClasses;
  const int64_t tiles = (nrows + kPlainRows - 1) / kPlainRows;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t r0 = tile * kPlainRows;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t j0 = 0; j0 < d; j0 += kPlainFeat) {
      const int jn = (int)std::min<int64_t>(kPlainFeat, d - j0);
      __syncthreads();   // the previous chunk is read
      // rows past nrows, classes past C and features past d repeat the last
      // one: a valid address; they are never summed or stored
#pragma unroll
      for (int q = 0; q < kPlainRows * kPlainFeat / 256; ++q) {
        const int e = tid + q * 256, rr = e / kPlainFeat, jj = e % kPlainFeat;
        const int64_t row = std::min<int64_t>(r0 + rr, nrows - 1);
        Xs[rr][jj] = X[row * d + std::min<int64_t>(j0 + jj, d - 1)];
      }
#pragma unroll
      for (int q = 0; q < kPlainClasses * kPlainFeat / 256; ++q) {
        const int e = tid + q * 256, cc = e / kPlainFeat, jj = e % kPlainFeat;
        const int64_t at =
            (int64_t)std::min(c0 + cc, C - 1) * d + std::min<int64_t>(j0 + jj, d - 1);
        Ms[cc][jj] = M[at];
        if constexpr (GAUSS) Vs[cc][jj] = V[at];
      }
      __syncthreads();
      for (int jj = 0; jj < jn; ++jj) {
        const double m = Ms[c][jj];
        if constexpr (GAUSS) {
          const double v = Vs[c][jj];
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const double df = Xs[rg * 4 + i][jj] - m;
            acc[i] = acc[i] + df * df / v;
          }
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const double x = Xs[rg * 4 + i][jj];
            acc[i] = acc[i] + (x != 0.0 ? x * m : 0.0);
          }
        }
      }
    }
    if (c0 + c >= C) continue;
    const double bc = b[c0 + c];
    const double lc = GAUSS ? ls[c0 + c] : 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int64_t row = r0 + rg * 4 + i;
      if (row >= nrows) continue;
      Z[row * C + c0 + c] = GAUSS ? bc - (acc[i] + lc) / 2.0 : bc + acc[i];
    }
  }
}

// One row of Z (C values) per LPR lanes.  COMP: Z becomes t - (max + log sum
// exp(t - max)) in place.  prob and pred may be null.
template <int LPR, bool COMP>
__global__ __launch_bounds__(256) void k_nbs_finish(double* Z, int64_t nrows, int C,
                                                    double* __restrict__ prob,
                                                    double* __restrict__ pred) {
  constexpr int RPW = 64 / LPR;   // rows per wave
  constexpr int kNone = 0x7fffffff;
  const int lane = threadIdx.x & 63, sl = lane % LPR, sub = lane / LPR;
  const int64_t gw = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t stride = (int64_t)gridDim.x * 4 * RPW;
  for (int64_t rb = gw * RPW; rb < nrows; rb += stride) {
    const int64_t row = rb + sub;
    const bool ok = row < nrows;
    // a lane group past the end repeats its wave's first row (never another
    // wave's, which may be rewritten meanwhile) and stores nothing
    double* z = Z + (ok ? row : rb) * C;
    double lse = 0.0;
    if constexpr (COMP) {
      double m = -__builtin_inf();
      for (int c = sl; c < C; c += LPR) m = fmax(m, z[c]);
#pragma unroll
      for (int s = 1; s < LPR; s <<= 1) m = fmax(m, __shfl_xor(m, s));
      double sum = 0.0;
      for (int c = sl; c < C; c += LPR) sum += exp(z[c] - m);
#pragma unroll
      for (int s = 1; s < LPR; s <<= 1) sum += __shfl_xor(sum, s);
      lse = m + log(sum);
    }
    const bool nan0 = z[0] != z[0];
    double m2 = -__builtin_inf(), sum2 = 1.0;
    if (prob) {
      for (int c = sl; c < C; c += LPR) m2 = fmax(m2, COMP ? z[c] - lse : z[c]);
#pragma unroll
      for (int s = 1; s < LPR; s <<= 1) m2 = fmax(m2, __shfl_xor(m2, s));
      sum2 = 0.0;
      for (int c = sl; c < C; c += LPR) sum2 += exp((COMP ? z[c] - lse : z[c]) - m2);
#pragma unroll
      for (int s = 1; s < LPR; s <<= 1) sum2 += __shfl_xor(sum2, s);
    }
    // the largest value that is not a NaN and its lowest index
    double best = -__builtin_inf();
    int bi = kNone;
    for (int c = sl; c < C; c += LPR) {
      const double r = COMP ? z[c] - lse : z[c];
      if (ok && COMP) z[c] = r;
      if (ok && prob) prob[row * C + c] = exp(r - m2) / sum2;
      if (r == r && (r > best || bi == kNone)) {
        best = r;
        bi = c;
      }
    }
#pragma unroll
    for (int t = 1; t < LPR; t <<= 1) {
      const double ob = __shfl_xor(best, t);
      const int oi = __shfl_xor(bi, t);
      if (oi != kNone && (bi == kNone || ob > best || (ob == best && oi < bi))) {
        best = ob;
        bi = oi;
      }
    }
    if (ok && pred && sl == 0) pred[row] = (nan0 || bi == kNone) ? 0.0 : (double)bi;
  }
}

template <bool COMP>
int finish(double* Z, int64_t nrows, int C, double* prob, double* pred, hipStream_t st) {
  cyc::KernelTimer timer("k_nbs_finish", st);
  const int lpr = C <= 4 ? 4 : (C <= 16 ? 16 : 64);
  const int64_t need = (nrows + 64 / lpr - 1) / (64 / lpr);   // waves
  const unsigned grid = (unsigned)std::min<int64_t>((need + 3) / 4, kFinishBlocks);
  if (lpr == 4)
    hipLaunchKernelGGL((k_nbs_finish<4, COMP>), dim3(grid), dim3(256), 0, st, Z, nrows, C, prob,
                       pred);
  else if (lpr == 16)
    hipLaunchKernelGGL((k_nbs_finish<16, COMP>), dim3(grid), dim3(256), 0, st, Z, nrows, C, prob,
                       pred);
  else
    hipLaunchKernelGGL((k_nbs_finish<64, COMP>), dim3(grid), dim3(256), 0, st, Z, nrows, C, prob,
                       pred);
  CYC_LAUNCH_CHECK("k_nbs_finish");
  return CYC_OK;
}

int plain(cyc_nbmodel_s* p, const double* X, int64_t nrows, double* Z, hipStream_t st) {
  cyc::KernelTimer timer("k_nbs_plain", st);
  const int64_t tiles = (nrows + kPlainRows - 1) / kPlainRows;
  const dim3 grid((unsigned)std::min<int64_t>(tiles, kPlainBlocks),
                  (unsigned)((p->C + kPlainClasses - 1) / kPlainClasses));
  if (p->type == NBS_GAUSSIAN)
    hipLaunchKernelGGL(k_nbs_plain<true>, grid, dim3(256), 0, st, X, nrows, p->d, p->C,
                       (const double*)p->b.ptr, (const double*)p->M.ptr, (const double*)p->V.ptr,
                       (const double*)p->ls.ptr, Z);
  else
    hipLaunchKernelGGL(k_nbs_plain<false>, grid, dim3(256), 0, st, X, nrows, p->d, p->C,
                       (const double*)p->b.ptr, (const double*)p->M.ptr, (const double*)nullptr,
                       (const double*)nullptr, Z);
  CYC_LAUNCH_CHECK("k_nbs_plain");
  return CYC_OK;
}

int check_rows(cyc_nbmodel_s* p, const double* X, int64_t nrows, hipStream_t st) {
  if (int rc = p->bad.reserve(sizeof(unsigned long long))) return rc;
  CYC_HIP(hipMemsetAsync(p->bad.ptr, 0xff, sizeof(unsigned long long), st));
  cyc::KernelTimer timer("k_nbs_check", st);
  const int64_t total = nrows * p->d;
  hipLaunchKernelGGL(k_nbs_check,
                     dim3((unsigned)std::min<int64_t>((total + 1023) / 1024, kCheckBlocks)),
                     dim3(256), 0, st, X, total, p->d, p->type == NBS_BERNOULLI ? 1 : 0,
                     (unsigned long long*)p->bad.ptr);
  CYC_LAUNCH_CHECK("k_nbs_check");
  return CYC_OK;
}

bool value_ok(int type, double x) {
  return type == NBS_BERNOULLI ? (x == 0.0 || x == 1.0) : x >= 0.0;
}

// the message of the lowest offending row
int refuse(cyc_nbmodel_s* p, const double* X, int64_t row) {
  std::vector<double> h((size_t)p->d);
  CYC_HIP(hipMemcpy(h.data(), X + row * p->d, sizeof(double) * (size_t)p->d,
                    hipMemcpyDeviceToHost));
  double v = 0.0;
  for (double x : h)
    if (!value_ok(p->type, x)) {
      v = x;
      break;
    }
  cyc::set_error(std::string("requirement failed: ") +
                 (p->type == NBS_BERNOULLI
                      ? "Bernoulli naive Bayes requires 0 or 1 feature values but found "
                      : "Naive Bayes requires nonnegative feature values but found ") +
                 cyc::java_double(v) + ". (row " + std::to_string(row) + ")");
  return CYC_ERR_INVALID_ARG;
}

int copy_in(cyc::DeviceBuffer& dst, const double* src, int64_t len, hipStream_t st) {
  if (int rc = dst.reserve(sizeof(double) * (size_t)len)) return rc;
  CYC_HIP(hipMemcpyAsync(dst.ptr, src, sizeof(double) * (size_t)len, hipMemcpyDeviceToDevice, st));
  return CYC_OK;
}

// whether M (len doubles) holds an inf or a NaN
int non_finite(cyc_nbmodel_s* p, const double* M, int64_t len, bool* out, hipStream_t st) {
  if (int rc = p->bad.reserve(sizeof(unsigned long long))) return rc;
  CYC_HIP(hipMemsetAsync(p->bad.ptr, 0, sizeof(int), st));
  hipLaunchKernelGGL(k_nbs_finite, dim3((unsigned)std::min<int64_t>((len + 255) / 256, 1024)),
                     dim3(256), 0, st, M, len, (int*)p->bad.ptr);
  CYC_LAUNCH_CHECK("k_nbs_finite");
  int flag = 0;
  CYC_HIP(hipMemcpyAsync(&flag, p->bad.ptr, sizeof(flag), hipMemcpyDeviceToHost, st));
  CYC_HIP(hipStreamSynchronize(st));
  *out = flag != 0;
  return CYC_OK;
}

int fill(cyc_nbmodel_s* p, const double* b, const double* M, const double* V, const double* ls,
         int scorer, hipStream_t st) {
  const int64_t cd = (int64_t)p->C * p->d;
  const bool gauss = p->type == NBS_GAUSSIAN;
  p->path = NBS_PLAIN;
  if (!gauss && scorer != NBS_PLAIN) {
    bool nf = false;
    if (int rc = non_finite(p, M, cd, &nf, st)) return rc;
    CYC_REQUIRE(!(nf && scorer == NBS_PRODUCT),
                "the product scorer needs a finite model matrix (a -inf of smoothing = 0 "
                "takes the plain scorer)");
    if (!nf) p->path = NBS_PRODUCT;
  }
  if (int rc = copy_in(p->b, b, p->C, st)) return rc;
  if (p->path == NBS_PRODUCT) {
    if (int rc = p->image.reserve(sizeof(double) * (size_t)packed_len(p->d, p->C))) return rc;
    // B = M^T (d x C): B(f, col) = M[col d + f]
    if (int rc = pack(M, p->d, p->C, 1, p->d, 1, 0, (double*)p->image.ptr, st)) return rc;
  } else {
    if (int rc = copy_in(p->M, M, cd, st)) return rc;
    if (gauss) {
      if (int rc = copy_in(p->V, V, cd, st)) return rc;
      if (int rc = copy_in(p->ls, ls, p->C, st)) return rc;
    }
  }
  CYC_HIP(hipStreamSynchronize(st));   // the caller's operands are read
  return CYC_OK;
}

}  // namespace

extern "C" {

int cyc_nbmodel_create(int32_t numClasses, int32_t numFeatures, int32_t modelType,
                       int64_t workspaceBytes, const double* b, const double* M, const double* V,
                       const double* ls, int32_t scorer, void* stream, cyc_nbmodel* model) {
  CYC_REQUIRE(model != nullptr, "model must not be null");
  CYC_REQUIRE(numClasses >= 1 && numClasses <= kMaxClasses,
              "NaiveBayes supports 1 to " + std::to_string(kMaxClasses) + " classes but got " +
                  std::to_string(numClasses));
  CYC_REQUIRE(numFeatures >= 1,
              "numFeatures must be positive but got " + std::to_string(numFeatures));
  CYC_REQUIRE(modelType >= NBS_MULTINOMIAL && modelType <= NBS_GAUSSIAN,
              "modelType must be 0 (multinomial), 1 (complement), 2 (bernoulli) or 3 (gaussian) "
              "but got " + std::to_string(modelType));
  CYC_REQUIRE(scorer >= NBS_AUTO && scorer <= NBS_PLAIN,
              "scorer must be 0 (auto), 1 (product) or 2 (plain) but got " +
                  std::to_string(scorer));
  CYC_REQUIRE(!(scorer == NBS_PRODUCT && modelType == NBS_GAUSSIAN),
              "the product scorer serves the linear forms; a gaussian model takes the plain "
              "scorer");
  CYC_REQUIRE(workspaceBytes >= 0, "workspaceBytes must not be negative");
  CYC_REQUIRE((int64_t)numClasses * ((int64_t)numFeatures + 1) <= INT32_MAX / 2,
              std::to_string(numClasses) + " x " + std::to_string(numFeatures) +
                  " dense matrix is too large to allocate");
  CYC_REQUIRE(b != nullptr && M != nullptr, "non-null b and M");
  CYC_REQUIRE(modelType != NBS_GAUSSIAN || (V != nullptr && ls != nullptr),
              "a gaussian model needs V and ls");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    cyc::set_error("no HIP device visible");
    return CYC_ERR_NO_DEVICE;
  }
  auto* p = new cyc_nbmodel_s();
  p->C = numClasses;
  p->d = numFeatures;
  p->type = modelType;
  const int64_t wsb = workspaceBytes ? workspaceBytes : kDefaultWorkspace;
  p->chunkRows = std::max<int64_t>(1, wsb / (8 * (int64_t)numClasses));
  if (p->chunkRows > kTileRows) p->chunkRows -= p->chunkRows % kTileRows;   // whole row tiles
  if (int rc = fill(p, b, M, V, ls, scorer, cyc::as_stream(stream))) {
    delete p;
    return rc;
  }
  *model = p;
  return CYC_OK;
}

int cyc_nbmodel_destroy(cyc_nbmodel model) {
  delete model;
  return CYC_OK;
}

int32_t cyc_nbmodel_path(cyc_nbmodel model) { return model ? model->path : -1; }
int64_t cyc_nbmodel_chunk_rows(cyc_nbmodel model) { return model ? model->chunkRows : -1; }

int cyc_nbmodel_score_dev(cyc_nbmodel model, const double* X, int64_t nrows, double* raw,
                          double* prob, double* pred, int64_t* badRow, void* stream) {
  CYC_REQUIRE(model != nullptr, "model must not be null");
  CYC_REQUIRE(nrows >= 0, "nrows >= 0");
  CYC_REQUIRE(raw != nullptr || prob != nullptr || pred != nullptr,
              "one of raw, prob and pred must not be null");
  if (badRow) *badRow = -1;
  if (nrows == 0) return CYC_OK;
  CYC_REQUIRE(X != nullptr, "non-null rows");
  cyc_nbmodel_s* p = model;
  hipStream_t st = cyc::as_stream(stream);
  std::lock_guard<std::mutex> g(p->mu);
  const bool checked = p->type != NBS_GAUSSIAN, comp = p->type == NBS_COMPLEMENT;
  if (checked)
    if (int rc = check_rows(p, X, nrows, st)) return rc;
  const int64_t chunk = std::min(nrows, p->chunkRows);
  if (!raw)
    if (int rc = p->ws.reserve(sizeof(double) * (size_t)(chunk * p->C))) return rc;
  for (int64_t r0 = 0; r0 < nrows; r0 += chunk) {
    const int64_t nr = std::min(chunk, nrows - r0);
    const double* Xc = X + r0 * p->d;
    double* Z = raw ? raw + r0 * p->C : (double*)p->ws.ptr;
    if (p->path == NBS_PRODUCT) {
      if (int rc = gemm(Xc, nr, p->d, p->C, (const double*)p->image.ptr,
                        NbBias{(const double*)p->b.ptr}, Z, "k_nbs_gemm", st))
        return rc;
    } else if (int rc = plain(p, Xc, nr, Z, st)) {
      return rc;
    }
    if (!comp && !prob && !pred) continue;
    double* pc = prob ? prob + r0 * p->C : nullptr;
    double* yc = pred ? pred + r0 : nullptr;
    if (int rc = comp ? finish<true>(Z, nr, p->C, pc, yc, st)
                      : finish<false>(Z, nr, p->C, pc, yc, st))
      return rc;
  }
  if (!checked) return CYC_OK;
  unsigned long long v = 0;
  CYC_HIP(hipMemcpyAsync(&v, p->bad.ptr, sizeof(v), hipMemcpyDeviceToHost, st));
  CYC_HIP(hipStreamSynchronize(st));
  if (v == kNoBad) return CYC_OK;
  const int64_t row = (int64_t)(v >> 3);
  if (badRow) *badRow = row;
  return refuse(p, X, row);
}

}  // extern "C"
