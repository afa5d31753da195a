// fm_csr.hip -- FMRegressor / FMClassifier over CSR rows on gfx950 (MI355X):
// the evaluation and the models' forward of fm.hip (same semantics, same out =
// [gV | gw | gb | L | cnt]) as a gather, for shards of 10^5 .. 10^7 columns and
// a few dozen non-zeros a row.  A stored zero contributes nothing.
//
// Prepared rows (cyc_fmcsr_rows_create, once per shard).  The indices are
// checked (cyc::check_csr_indices); cyc::build_csc makes a column-major copy
// (row int32, value fp64, each column's entries in ascending row order) in ONE
// row block, so colptr has d + 1 entries; every column longer than kSeg
// entries is cut into segments of exactly kSeg entries (the last one shorter)
// and listed in a segment table.  The cut depends on the data alone.
//
// Kernels (KP = the power of two >= k)
//   k_fmcsr_forward<KP, TRAIN>
//                   one wave per row.  Lane = (slot, factor) = (lane / KP, lane
//                   % KP): 64 / KP non-zeros are in flight at once.  The wave
//                   stages the row's next 64 (column, value) pairs in LDS with
//                   one coalesced read; slot s takes the pairs s, s + 64 / KP,
//                   .. of the row in ascending order, gathers V[j, 0:k] (and
//                   w[j], in the slot's lane 0) straight from coef and
//                   accumulates s_f and q_f.  The slots' sums are added in slot
//                   order by cross-lane moves; fm_raw / fm_loss form the
//                   epilogue (batch selection and the label check there).
//                   TRAIN: M (n x (k + 1)) = [m o S | m] and aux (n x 2) =
//                   (loss, taken), zeros for a row outside the batch; otherwise
//                   the models' margin, raw, probability and prediction.
//   k_fmcsr_grad<KP>
//                   over the column copy: a group of KP lanes owns one column
//                   of at most one segment (64 / KP neighbouring columns share a
//                   wave) and walks it in row order, four entries in flight:
//                   P_f += x M[r, f], gw += x m_r, t += m_r x^2, then writes
//                   gV[j, f] = P_f - V[j, f] t and gw_j; an empty column
//                   writes zeros.
//   k_fmcsr_grad_seg<KP>
//                   one workgroup per segment of a long column: wave w takes
//                   the segment's quarter w, its groups the entries g, g + 64 /
//                   KP, .. of the quarter; the groups are added in group order
//                   by cross-lane moves, the four waves in wave order through
//                   LDS: one partial [P | gw | t] per segment.
//   k_fmcsr_fold    a long column's partials, added in segment order.
//   k_fmcsr_runs, k_fmcsr_tail
//                   gb, L and cnt from M and aux: runs of kFmRunRows rows
//                   (thread t's rows in order, then a fixed tree), the runs
//                   added in run order.
// No atomics on doubles and no sum whose order depends on the grid, the
// workspace or the call: the same bytes on every call.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "fm_dev.hpp"

struct cyc_fmcsr_rows_s {
  int64_t n = 0, nnz = 0, nseg = 0, nlong = 0;
  int d = 0;
  const int64_t* rowptr = nullptr;   // the caller's CSR, borrowed
  const int32_t* colidx = nullptr;
  const double* vals = nullptr;
  cyc::DeviceBuffer colptr, rowidx, cvals;   // the column copy
  // segment s: column segCol[s], entries from segStart[s]; long column c:
  // longCol[c], its segments longSeg[c] .. longSeg[c + 1]
  cyc::DeviceBuffer segCol, segStart, longCol, longSeg;
};

namespace {

using namespace cyc::fmdev;

constexpr int kSeg = 256;
constexpr int64_t kOneRowBlock = (int64_t)1 << 31;   // n < 2^31: one block

__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
}

// ------------------------------------------------------------------ forward
// LDS per wave: 64 columns, 64 values, then S1 (k + 1) and S2 (k) of fm_raw.
template <int KP, bool TRAIN>
__global__ __launch_bounds__(256) void k_fmcsr_forward(
    const int64_t* __restrict__ rowptr, const int32_t* __restrict__ colidx,
    const double* __restrict__ vals, const double* __restrict__ y, int64_t n, int k,
    const double* __restrict__ V, const double* __restrict__ w, const double* __restrict__ bptr,
    int loss, uint64_t h1, uint64_t thr, int64_t firstRow, double* __restrict__ M,
    double* __restrict__ aux, unsigned long long* __restrict__ bad, double* __restrict__ margin,
    double* __restrict__ raw2, double* __restrict__ prob2, double* __restrict__ pred) {
  constexpr int NS = 64 / KP;
  __shared__ int32_t scol[4][64];
  __shared__ double sval[4][64];
  __shared__ double ssum[4][2 * kMaxFactors + 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, slot = lane / KP, f = lane % KP;
  const bool fok = f < k;
  double* S1 = ssum[wave];
  double* S2 = S1 + kMaxFactors + 1;
  const double b = bptr ? *bptr : 0.0;
  for (int64_t r = (int64_t)blockIdx.x * 4 + wave; r < n; r += (int64_t)gridDim.x * 4) {
    const bool take = !TRAIN || fm_take(h1, thr, firstRow + r);
    double s = 0.0, q = 0.0, lin = 0.0;
    if (take) {   // a row outside the batch is not loaded
      const int64_t p1 = rowptr[r + 1];
      for (int64_t p0 = rowptr[r]; p0 < p1; p0 += 64) {
        const int cnt = (int)min((int64_t)64, p1 - p0);
        wave_sync();   // the previous chunk is read
        if (lane < cnt) {
          scol[wave][lane] = colidx[p0 + lane];
          sval[wave][lane] = vals[p0 + lane];
        }
        wave_sync();
        for (int e = slot; e < cnt; e += NS) {
          const int64_t j = scol[wave][e];
          const double x = sval[wave][e];
          if (x != 0.0) {
            if (fok) {
              const double t = V[j * k + f] * x;
              s += t;
              q += t * t;
            }
            if (f == 0 && w) lin += w[j] * x;
          }
        }
      }
    }
    // the slots in slot order; every lane ends with its factor's totals
    double S = __shfl(s, f), Q = __shfl(q, f), Lw = __shfl(lin, 0);
#pragma nounroll
    for (int sl = 1; sl < NS; ++sl) {
      S += __shfl(s, sl * KP + f);
      Q += __shfl(q, sl * KP + f);
      Lw += __shfl(lin, sl * KP);
    }
    wave_sync();   // the previous row's sums are read
    if (slot == 0 && fok) {
      S1[f] = S;
      S2[f] = Q;
    }
    if (lane == 0) S1[k] = Lw;
    wave_sync();
    const double raw = fm_raw(S1, S2, k, b);   // every lane, the same value
    if constexpr (TRAIN) {
      double l = 0.0, m = 0.0, cnt = 0.0;
      if (take) {
        if (fm_loss(loss, raw, y[r], &l, &m)) {
          cnt = 1.0;
        } else {
          l = m = 0.0;
          if (lane == 0) fm_flag_bad(bad, firstRow + r);
        }
      }
      double* mr = M + r * (k + 1);
      if (slot == 0 && fok) mr[f] = m * S;
      if (lane == 0) {
        mr[k] = m;
        aux[2 * r] = l;
        aux[2 * r + 1] = cnt;
      }
    } else if (lane == 0) {
      const double p = 1.0 / (1.0 + exp(-raw));
      if (margin) margin[r] = raw;
      if (raw2) {
        raw2[2 * r] = -raw;
        raw2[2 * r + 1] = raw;
      }
      if (prob2) {
        prob2[2 * r] = 1.0 - p;
        prob2[2 * r + 1] = p;
      }
      if (pred) pred[r] = loss == kLossLogistic ? (raw > 0.0 ? 1.0 : 0.0) : raw;
    }
  }
}

// ----------------------------------------------------------------- gradient
// The entries q0 + first, q0 + first + step, .. < q1 of the column copy in
// order, four gathers of M in flight: P (this lane's factor), gw and t.
template <int KP>
__device__ __forceinline__ void fmcsr_walk(const int32_t* __restrict__ rowidx,
                                           const double* __restrict__ cvals, int64_t q0,
                                           int64_t q1, int step, int k, int f,
                                           const double* __restrict__ M, double& P, double& gw,
                                           double& t) {
  const bool fok = f < k;
  for (int64_t q = q0; q < q1; q += 4 * (int64_t)step) {
    double x[4], mf[4], mm[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t e = q + (int64_t)u * step;
      x[u] = e < q1 ? cvals[e] : 0.0;
      const double* mr = M + (int64_t)(e < q1 ? rowidx[e] : 0) * (k + 1);
      const bool on = x[u] != 0.0;   // a stored zero gathers nothing
      mf[u] = (on && fok) ? mr[f] : 0.0;
      mm[u] = on ? mr[k] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (x[u] != 0.0) {
        P += x[u] * mf[u];
        gw += x[u] * mm[u];
        t += mm[u] * (x[u] * x[u]);
      }
  }
}

template <int KP>
__global__ __launch_bounds__(256) void k_fmcsr_grad(
    const int64_t* __restrict__ colptr, const int32_t* __restrict__ rowidx,
    const double* __restrict__ cvals, int d, int k, const double* __restrict__ M,
    const double* __restrict__ V, int fitLinear, double* __restrict__ out) {
  constexpr int GROUPS = 256 / KP;
  const int f = threadIdx.x % KP;
  const int64_t dk = (int64_t)d * k;
  for (int64_t j = (int64_t)blockIdx.x * GROUPS + threadIdx.x / KP; j < d;
       j += (int64_t)gridDim.x * GROUPS) {
    const int64_t q0 = colptr[j], q1 = colptr[j + 1];
    if (q1 - q0 > kSeg) continue;   // k_fmcsr_grad_seg and k_fmcsr_fold own it
    double P = 0.0, gw = 0.0, t = 0.0;
    fmcsr_walk<KP>(rowidx, cvals, q0, q1, 1, k, f, M, P, gw, t);
    if (f < k) out[j * k + f] = q0 == q1 ? 0.0 : P - V[j * k + f] * t;
    if (f == 0 && fitLinear) out[dk + j] = gw;
  }
}

template <int KP>
__global__ __launch_bounds__(256) void k_fmcsr_grad_seg(
    const int32_t* __restrict__ segCol, const int64_t* __restrict__ segStart,
    const int64_t* __restrict__ colptr, const int32_t* __restrict__ rowidx,
    const double* __restrict__ cvals, int k, const double* __restrict__ M,
    double* __restrict__ segPart) {
  constexpr int NG = 64 / KP, QUARTER = kSeg / 4;
  __shared__ double red[4][kMaxFactors + 2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane / KP, f = lane % KP;
  const int64_t seg = blockIdx.x;
  const int64_t s0 = segStart[seg], s1 = min(s0 + kSeg, colptr[segCol[seg] + 1]);
  const int64_t q0 = min(s0 + wave * QUARTER, s1), q1 = min(q0 + QUARTER, s1);
  double P = 0.0, gw = 0.0, t = 0.0;
  fmcsr_walk<KP>(rowidx, cvals, q0 + g, q1, NG, k, f, M, P, gw, t);
  double Pw = __shfl(P, f), gww = __shfl(gw, 0), tw = __shfl(t, 0);
#pragma nounroll
  for (int gg = 1; gg < NG; ++gg) {
    Pw += __shfl(P, gg * KP + f);
    gww += __shfl(gw, gg * KP);
    tw += __shfl(t, gg * KP);
  }
  if (g == 0 && f < k) red[wave][f] = Pw;
  if (lane == 0) {
    red[wave][k] = gww;
    red[wave][k + 1] = tw;
  }
  __syncthreads();
  if (threadIdx.x < k + 2) {
    const int e = threadIdx.x;
    segPart[seg * (k + 2) + e] = ((red[0][e] + red[1][e]) + red[2][e]) + red[3][e];
  }
}

// thread (long column c, e <= k): its partials in segment order
__global__ __launch_bounds__(256) void k_fmcsr_fold(
    const int32_t* __restrict__ longCol, const int64_t* __restrict__ longSeg, int64_t nlong, int d,
    int k, const double* __restrict__ segPart, const double* __restrict__ V, int fitLinear,
    double* __restrict__ out) {
  const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t c = id / (k + 1);
  const int e = (int)(id % (k + 1));
  if (c >= nlong) return;
  const int64_t j = longCol[c];
  double a = 0.0, t = 0.0;
  for (int64_t s = longSeg[c]; s < longSeg[c + 1]; ++s) {
    a += segPart[s * (k + 2) + e];
    t += segPart[s * (k + 2) + k + 1];
  }
  if (e < k) out[j * k + e] = a - V[j * k + e] * t;
  else if (fitLinear) out[(int64_t)d * k + j] = a;
}

// run blockIdx.x: (gb, L, cnt) of its rows
__global__ __launch_bounds__(256) void k_fmcsr_runs(const double* __restrict__ M,
                                                    const double* __restrict__ aux, int64_t n,
                                                    int k, double* __restrict__ runPart) {
  __shared__ double sh[3][256];
  const int tid = threadIdx.x;
  const int64_t R0 = (int64_t)blockIdx.x * kFmRunRows, R1 = min(n, R0 + kFmRunRows);
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
  if (tid < 3) runPart[3 * (int64_t)blockIdx.x + tid] = sh[tid][0];
}

// out's tail [gb (fitIntercept) | L | cnt]: the runs in run order
__global__ void k_fmcsr_tail(const double* __restrict__ runPart, int64_t runs, int fitIntercept,
                             double* __restrict__ tail) {
  const int q = threadIdx.x;
  if (q >= 3 || (q == 0 && !fitIntercept)) return;
  double s = 0.0;
  for (int64_t r = 0; r < runs; ++r) s += runPart[3 * r + q];
  tail[q - (fitIntercept ? 0 : 1)] = s;
}

#define CYC_FMCSR_KP(k_, CALL)                                        \
  if (k_ <= 1) { constexpr int KP = 1; CALL; }                        \
  else if (k_ <= 2) { constexpr int KP = 2; CALL; }                   \
  else if (k_ <= 4) { constexpr int KP = 4; CALL; }                   \
  else if (k_ <= 8) { constexpr int KP = 8; CALL; }                   \
  else if (k_ <= 16) { constexpr int KP = 16; CALL; }                 \
  else if (k_ <= 32) { constexpr int KP = 32; CALL; }                 \
  else { constexpr int KP = 64; CALL; }

int upload(cyc::DeviceBuffer& buf, const void* src, size_t bytes) {
  if (int rc = buf.reserve(std::max<size_t>(bytes, 8))) return rc;
  if (bytes) CYC_HIP(hipMemcpy(buf.ptr, src, bytes, hipMemcpyHostToDevice));
  return CYC_OK;
}

// the segment table of the columns longer than kSeg, from the copy's colptr
int build_segments(cyc_fmcsr_rows_s* r, hipStream_t st) {
  std::vector<int64_t> colptr((size_t)r->d + 1);
  CYC_HIP(hipStreamSynchronize(st));
  CYC_HIP(hipMemcpy(colptr.data(), r->colptr.ptr, sizeof(int64_t) * colptr.size(),
                    hipMemcpyDeviceToHost));
  std::vector<int32_t> segCol, longCol;
  std::vector<int64_t> segStart, longSeg;
  for (int j = 0; j < r->d; ++j) {
    if (colptr[j + 1] - colptr[j] <= kSeg) continue;
    longCol.push_back(j);
    longSeg.push_back((int64_t)segCol.size());
    for (int64_t q = colptr[j]; q < colptr[j + 1]; q += kSeg) {
      segCol.push_back(j);
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

int check_rows(const cyc_fm_plan_s* p, const cyc_fmcsr_rows_s* r) {
  CYC_REQUIRE(r != nullptr, "rows must not be null");
  CYC_REQUIRE(r->d == p->d, "the rows have " + std::to_string(r->d) +
                                " features but the plan has " + std::to_string(p->d));
  return CYC_OK;
}

int64_t forward_grid(int64_t n) {
  return std::min<int64_t>((n + 3) / 4, 32 * (int64_t)cyc::device_cus());
}

}  // namespace

extern "C" {

int cyc_fmcsr_segment_entries(void) { return kSeg; }

int cyc_fmcsr_rows_create(const int64_t* rowptr, const int32_t* colidx, const double* values,
                          int64_t nrows, int32_t numFeatures, void* stream,
                          cyc_fmcsr_rows* rows) {
  CYC_REQUIRE(rows != nullptr && rowptr != nullptr, "output handle and rowptr must not be null");
  CYC_REQUIRE(nrows >= 0 && nrows < kOneRowBlock, "0 <= nrows < 2^31");
  CYC_REQUIRE(numFeatures >= 1, "numFeatures >= 1");
  hipStream_t st = cyc::as_stream(stream);
  if (int rc = cyc::check_csr_indices(rowptr, colidx, nrows, numFeatures, st)) return rc;
  auto* r = new cyc_fmcsr_rows_s();
  r->n = nrows;
  r->d = numFeatures;
  r->rowptr = rowptr;
  r->colidx = colidx;
  r->vals = values;
  int rc = cyc::build_csc(rowptr, colidx, values, nrows, numFeatures, kOneRowBlock, r->colptr,
                          r->rowidx, r->cvals, st);
  if (!rc) rc = build_segments(r, st);
  if (rc) {
    delete r;
    return rc;
  }
  *rows = r;
  return CYC_OK;
}

int cyc_fmcsr_rows_destroy(cyc_fmcsr_rows rows) {
  delete rows;
  return CYC_OK;
}

int cyc_fmcsr_evaluate_dev(cyc_fm_plan plan, cyc_fmcsr_rows rows, const double* y,
                           const double* coef, int64_t iter, double fraction, int64_t rowOffset,
                           double* out, void* stream) {
  if (int rc = fm_check_evaluate(plan, 0, rowOffset, coef, out, fraction)) return rc;
  cyc_fm_plan_s* p = plan;
  if (int rc = check_rows(p, rows)) return rc;
  const cyc_fmcsr_rows_s* r = rows;
  CYC_REQUIRE(r->n == 0 || y != nullptr, "non-null labels");
  hipStream_t st = cyc::as_stream(stream);
  std::lock_guard<std::mutex> guard(p->mu);
  const int d = p->d, k = p->k;
  const int64_t n = r->n, runs = (n + kFmRunRows - 1) / kFmRunRows;
  const Coef c = split_coef(p, coef);
  if (int rc = fm_clear_bad(p, st)) return rc;
  // M (n x (k + 1)) | aux (n x 2) | runPart (runs x 3) | segPart (nseg x (k + 2))
  const int64_t words = n * (k + 3) + 3 * runs + r->nseg * (k + 2);
  if (int rc = p->ws.reserve(sizeof(double) * (size_t)std::max<int64_t>(words, 1))) return rc;
  double* M = (double*)p->ws.ptr;
  double* aux = M + n * (k + 1);
  double* runPart = aux + 2 * n;
  double* segPart = runPart + 3 * runs;
  auto* bad = (unsigned long long*)p->bad.ptr;
  const int64_t cus = cyc::device_cus();
  if (n > 0) {
    {
      cyc::KernelTimer timer("k_fmcsr_forward", st);
      CYC_FMCSR_KP(k, hipLaunchKernelGGL((k_fmcsr_forward<KP, true>),
                                         dim3((unsigned)forward_grid(n)), dim3(256), 0, st,
                                         r->rowptr, r->colidx, r->vals, y, n, k, c.V, c.w, c.b,
                                         p->loss, fm_seed(iter), fm_threshold(fraction), rowOffset,
                                         M, aux, bad, nullptr, nullptr, nullptr, nullptr));
      CYC_LAUNCH_CHECK("k_fmcsr_forward");
    }
    hipLaunchKernelGGL(k_fmcsr_runs, dim3((unsigned)runs), dim3(256), 0, st, M, aux, n, k, runPart);
    CYC_LAUNCH_CHECK("k_fmcsr_runs");
  }
  const int64_t dk = (int64_t)d * k;
  {
    cyc::KernelTimer timer("k_fmcsr_grad", st);
    CYC_FMCSR_KP(k, {
      const int64_t grid = std::min<int64_t>(((int64_t)d + 256 / KP - 1) / (256 / KP), 64 * cus);
      hipLaunchKernelGGL((k_fmcsr_grad<KP>), dim3((unsigned)grid), dim3(256), 0, st,
                         (const int64_t*)r->colptr.ptr, (const int32_t*)r->rowidx.ptr,
                         (const double*)r->cvals.ptr, d, k, M, c.V, p->fitLinear, out);
    });
    CYC_LAUNCH_CHECK("k_fmcsr_grad");
  }
  if (r->nseg > 0) {
    cyc::KernelTimer timer("k_fmcsr_grad_seg", st);
    CYC_FMCSR_KP(k, hipLaunchKernelGGL((k_fmcsr_grad_seg<KP>), dim3((unsigned)r->nseg), dim3(256),
                                       0, st, (const int32_t*)r->segCol.ptr,
                                       (const int64_t*)r->segStart.ptr,
                                       (const int64_t*)r->colptr.ptr,
                                       (const int32_t*)r->rowidx.ptr, (const double*)r->cvals.ptr,
                                       k, M, segPart));
    CYC_LAUNCH_CHECK("k_fmcsr_grad_seg");
    hipLaunchKernelGGL(k_fmcsr_fold, dim3((unsigned)((r->nlong * (k + 1) + 255) / 256)), dim3(256),
                       0, st, (const int32_t*)r->longCol.ptr, (const int64_t*)r->longSeg.ptr,
                       r->nlong, d, k, segPart, c.V, p->fitLinear, out);
    CYC_LAUNCH_CHECK("k_fmcsr_fold");
  }
  hipLaunchKernelGGL(k_fmcsr_tail, dim3(1), dim3(64), 0, st, runPart, runs, p->fitIntercept,
                     out + dk + (p->fitLinear ? d : 0));
  CYC_LAUNCH_CHECK("k_fmcsr_tail");
  return n > 0 ? fm_report_bad(p, st) : CYC_OK;
}

int cyc_fmcsr_predict_dev(cyc_fm_plan plan, cyc_fmcsr_rows rows, const double* coef,
                          double* margin, double* raw, double* prob, double* pred, void* stream) {
  CYC_REQUIRE(plan != nullptr, "plan must not be null");
  CYC_REQUIRE(coef != nullptr, "coef must not be null");
  CYC_REQUIRE(margin != nullptr || raw != nullptr || prob != nullptr || pred != nullptr,
              "at least one of margin, raw, prob and pred");
  cyc_fm_plan_s* p = plan;
  if (int rc = check_rows(p, rows)) return rc;
  const cyc_fmcsr_rows_s* r = rows;
  if (r->n == 0) return CYC_OK;
  CYC_REQUIRE(p->loss == kLossLogistic || (raw == nullptr && prob == nullptr),
              "raw and prob need a classifier");
  hipStream_t st = cyc::as_stream(stream);
  std::lock_guard<std::mutex> guard(p->mu);
  const Coef c = split_coef(p, coef);
  cyc::KernelTimer timer("k_fmcsr_predict", st);
  CYC_FMCSR_KP(p->k, hipLaunchKernelGGL((k_fmcsr_forward<KP, false>),
                                        dim3((unsigned)forward_grid(r->n)), dim3(256), 0, st,
                                        r->rowptr, r->colidx, r->vals, nullptr, r->n, p->k, c.V,
                                        c.w, c.b, p->loss, 0ull, 0ull, (int64_t)0, nullptr,
                                        nullptr, nullptr, margin, raw, prob, pred));
  CYC_LAUNCH_CHECK("k_fmcsr_predict");
  return CYC_OK;
}

}  // extern "C"
