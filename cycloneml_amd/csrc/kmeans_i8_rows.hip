// kmeans_i8_rows.hip -- the row image of the i8 screen: each row of X as
// three int8 limb planes with its exponent and 1-norm bound, built once per
// fit.  The fixed-point split is derived at the head of kmeans_i8.hip.
#include "kmeans_i8_dev.hpp"

namespace cyc {
namespace km8 {
namespace {

#ifndef CYC_QUANT_COAL
#define CYC_QUANT_COAL 1   // k_rows_quantize: 16 B coalesced row loads
#endif

// The same for 16-byte aligned rows of even d <= 128 H, the next row's loads
// issued before this row's reductions and stores (software-pipelined: two
// rows in flight per wave; the row-at-a-time loop left the stream latency
// bound at ~3.4 TB/s of reads + writes).  Same limbs, exponents and meta.
template <int H>
__global__ __launch_bounds__(256) void k_rows_quantize_pf(const double* __restrict__ X, int64_t n,
                                                          int d, int D, unsigned* __restrict__ img,
                                                          int2* __restrict__ meta,
                                                          const double* __restrict__ scale,
                                                          double* __restrict__ unorm) {
  const int lane = threadIdx.x & 63;
  const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
  int64_t row = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  v2d cur[H];
  auto load = [&](int64_t r, v2d (&w)[H]) {
    const double* x = X + (r < n ? r : 0) * d;
#pragma unroll
    for (int h = 0; h < H; ++h) {
      const int j = h * 128 + 2 * lane;
      w[h] = j < d ? __builtin_nontemporal_load(reinterpret_cast<const v2d*>(x + j)) : v2d{0.0, 0.0};
    }
  };
  if (row < n) load(row, cur);
  for (; row < n; row += nw) {
    v2d nxt[H];
    load(row + nw, nxt);   // in flight while this row is reduced and stored
    double v[2 * H];
    double m = 0.0, s1 = 0.0, s2 = 0.0;
    bool fin = true;
    const double sc = scale ? scale[row] : 1.0;
#pragma unroll
    for (int h = 0; h < H; ++h)
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        double t = q ? cur[h].y : cur[h].x;
        if (scale) t = t / sc;
        v[2 * h + q] = t;
        fin = fin && __builtin_isfinite(t);
        m = __builtin_fmax(m, __builtin_fabs(t));
        s1 += __builtin_fabs(t);
        s2 += t * t;
      }
    m = wave_max(m);
    s1 = wave_sum(s1);
    if (unorm) {
      s2 = wave_sum(s2);
      if (lane == 0) unorm[row] = __builtin_sqrt(s2);
    }
    const bool allFin = __all(fin);
    const int e = choose_exp(m);
    const bool bad = !allFin || e > kMaxExp;
    unsigned char* db = reinterpret_cast<unsigned char*>(img + row * (int64_t)(3 * D / 4));
#pragma unroll
    for (int h = 0; h < H; ++h) {
      const int j0 = h * 128 + 2 * lane;
      if (j0 < D) {
        int a[2], b[2], c[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          if (bad) a[q] = b[q] = c[q] = 0;
          else quant3(v[2 * h + q], e, a[q], b[q], c[q]);
        }
        *reinterpret_cast<unsigned short*>(db + j0) = (unsigned short)((a[0] & 0xff) | ((a[1] & 0xff) << 8));
        *reinterpret_cast<unsigned short*>(db + D + j0) = (unsigned short)((b[0] & 0xff) | ((b[1] & 0xff) << 8));
        *reinterpret_cast<unsigned short*>(db + 2 * D + j0) = (unsigned short)((c[0] & 0xff) | ((c[1] & 0xff) << 8));
      }
    }
    if (lane == 0) {
      const double n1 = bad ? 0.0 : s1 * (1.0 + 0x1p-40) + (double)d * __builtin_ldexp(1.0, e - 22);
      meta[row] = make_int2(bad ? INT_MIN : e, __float_as_int(fup(n1)));
    }
#pragma unroll
    for (int h = 0; h < H; ++h) cur[h] = nxt[h];
  }
}

// d % 4 == 0, d <= 256, rows 32-byte aligned: each lane quantises 4
// consecutive elements, so every limb plane leaves as one 4-byte store per
// lane (256 B per wave instruction; the 2-byte stores of k_rows_quantize_pf
// wrote half lines), the next row's loads in flight as there.
__global__ __launch_bounds__(256) void k_rows_quantize_q4(const double* __restrict__ X, int64_t n,
                                                          int d, int D, unsigned* __restrict__ img,
                                                          int2* __restrict__ meta,
                                                          const double* __restrict__ scale,
                                                          double* __restrict__ unorm) {
  const int lane = threadIdx.x & 63;
  const int j0 = 4 * lane;
  const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
  int64_t row = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  v2d cur[2];
  auto load = [&](int64_t r, v2d (&w)[2]) {
    const double* x = X + (r < n ? r : 0) * d + j0;
    w[0] = j0 < d ? __builtin_nontemporal_load(reinterpret_cast<const v2d*>(x)) : v2d{0.0, 0.0};
    w[1] = j0 < d ? __builtin_nontemporal_load(reinterpret_cast<const v2d*>(x + 2)) : v2d{0.0, 0.0};
  };
  if (row < n) load(row, cur);
  for (; row < n; row += nw) {
    v2d nxt[2];
    load(row + nw, nxt);   // in flight while this row is reduced and stored
    const double sc = scale ? scale[row] : 1.0;
    double v[4] = {cur[0].x, cur[0].y, cur[1].x, cur[1].y};
    double m = 0.0, s1 = 0.0, s2 = 0.0;
    bool fin = true;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (scale) v[q] = v[q] / sc;
      fin = fin && __builtin_isfinite(v[q]);
      m = __builtin_fmax(m, __builtin_fabs(v[q]));
      s1 += __builtin_fabs(v[q]);
      s2 += v[q] * v[q];
    }
    m = wave_max(m);
    s1 = wave_sum(s1);
    if (unorm) {
      s2 = wave_sum(s2);
      if (lane == 0) unorm[row] = __builtin_sqrt(s2);
    }
    const bool allFin = __all(fin);
    const int e = choose_exp(m);
    const bool bad = !allFin || e > kMaxExp;
    if (j0 < D) {
      int a[4], b[4], c[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (bad) a[q] = b[q] = c[q] = 0;
        else quant3(v[q], e, a[q], b[q], c[q]);
      }
      unsigned char* db = reinterpret_cast<unsigned char*>(img + row * (int64_t)(3 * D / 4));
      *reinterpret_cast<unsigned*>(db + j0) = pack4(a);
      *reinterpret_cast<unsigned*>(db + D + j0) = pack4(b);
      *reinterpret_cast<unsigned*>(db + 2 * D + j0) = pack4(c);
    }
    if (lane == 0) {
      const double n1 = bad ? 0.0 : s1 * (1.0 + 0x1p-40) + (double)d * __builtin_ldexp(1.0, e - 22);
      meta[row] = make_int2(bad ? INT_MIN : e, __float_as_int(fup(n1)));
    }
    cur[0] = nxt[0];
    cur[1] = nxt[1];
  }
}

// One wave per row: limbs into the image, exponent and |xh|_1 bound into meta.
// scale (optional): the row is x / scale[row] (the cosine plan's unit
// directions), whose norm goes to unorm[row] (any summation order: it only
// enters the certification margins, like the fp64 norms do).
__global__ __launch_bounds__(256) void k_rows_quantize(const double* __restrict__ X, int64_t n,
                                                       int d, int D, unsigned* __restrict__ img,
                                                       int2* __restrict__ meta,
                                                       const double* __restrict__ scale,
                                                       double* __restrict__ unorm, int vec) {
  const int lane = threadIdx.x & 63;
  const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t row = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; row < n; row += nw) {
    const double* x = X + row * d;
    double v[8];
    double m = 0.0, s1 = 0.0, s2 = 0.0;
    bool fin = true;
    const double sc = scale ? scale[row] : 1.0;
#if CYC_QUANT_COAL
    // lane holds elements 128 h + 2 lane + {0, 1}: one 16 B load per lane and
    // 1 KiB contiguous per wave instruction (vec: d even, X 16 B aligned)
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      const int j = h * 128 + 2 * lane;
      v2d w = {0.0, 0.0};
      if (vec) {
        if (j < d) w = __builtin_nontemporal_load(reinterpret_cast<const v2d*>(x + j));
      } else {
        if (j < d) w.x = x[j];
        if (j + 1 < d) w.y = x[j + 1];
      }
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        double t = q ? w.y : w.x;
        if (scale) t = t / sc;
        v[2 * h + q] = t;
        fin = fin && __builtin_isfinite(t);
        m = __builtin_fmax(m, __builtin_fabs(t));
        s1 += __builtin_fabs(t);
        s2 += t * t;
      }
    }
#else
#pragma unroll
    for (int p = 0; p < 2; ++p) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int j = p * 256 + 4 * lane + q;
        double t = j < d ? x[j] : 0.0;
        if (scale) t = t / sc;
        v[4 * p + q] = t;
        fin = fin && __builtin_isfinite(t);
        m = __builtin_fmax(m, __builtin_fabs(t));
        s1 += __builtin_fabs(t);
        s2 += t * t;
      }
    }
#endif
    m = wave_max(m);
    s1 = wave_sum(s1);
    if (unorm) {
      s2 = wave_sum(s2);
      if (lane == 0) unorm[row] = __builtin_sqrt(s2);
    }
    const bool allFin = __all(fin);
    const int e = choose_exp(m);
    const bool bad = !allFin || e > kMaxExp;
#if CYC_QUANT_COAL
    unsigned char* db = reinterpret_cast<unsigned char*>(img + row * (int64_t)(3 * D / 4));
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      const int j0 = h * 128 + 2 * lane;
      if (j0 < D) {
        int a[2], b[2], c[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          if (bad) {
            a[q] = b[q] = c[q] = 0;
          } else {
            quant3(v[2 * h + q], e, a[q], b[q], c[q]);
          }
        }
        *reinterpret_cast<unsigned short*>(db + j0) = (unsigned short)((a[0] & 0xff) | ((a[1] & 0xff) << 8));
        *reinterpret_cast<unsigned short*>(db + D + j0) = (unsigned short)((b[0] & 0xff) | ((b[1] & 0xff) << 8));
        *reinterpret_cast<unsigned short*>(db + 2 * D + j0) = (unsigned short)((c[0] & 0xff) | ((c[1] & 0xff) << 8));
      }
    }
#else
    unsigned* dst = img + row * (int64_t)(3 * D / 4);
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const int j0 = p * 256 + 4 * lane;
      if (j0 < D) {
        int a[4], b[4], c[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          if (bad) {
            a[q] = b[q] = c[q] = 0;
          } else {
            quant3(v[4 * p + q], e, a[q], b[q], c[q]);
          }
        }
        dst[j0 / 4] = pack4(a);
        dst[(D + j0) / 4] = pack4(b);
        dst[(2 * D + j0) / 4] = pack4(c);
      }
    }
#endif
    if (lane == 0) {
      // |xh|_1 <= |x|_1 + d 2^(e-22); the fp64 sum is rounded up generously
      const double n1 = bad ? 0.0 : s1 * (1.0 + 0x1p-40) + (double)d * __builtin_ldexp(1.0, e - 22);
      meta[row] = make_int2(bad ? INT_MIN : e, __float_as_int(fup(n1)));
    }
  }
}

}  // namespace

int rows_quantize(const double* X, int64_t n, int d, void* img, int2* meta, hipStream_t st,
                  const double* scale, double* unorm) {
  if (n <= 0) return CYC_OK;
  const int D = 64 * ksteps(d);
  const int64_t blocks = std::min<int64_t>((n + 3) / 4, 65536);
  const int vec = (d % 2 == 0) && (reinterpret_cast<uintptr_t>(X) % 16 == 0);
  static const bool pf = [] {   // CYC_QUANT_PF=0: the row-at-a-time kernel
    const char* e = std::getenv("CYC_QUANT_PF");
    return !(e && e[0] == '0');
  }();
  const bool q4 = d % 4 == 0 && reinterpret_cast<uintptr_t>(X) % 32 == 0;
  if (q4 && pf && d <= 256)
    hipLaunchKernelGGL(k_rows_quantize_q4, dim3((unsigned)blocks), dim3(256), 0, st, X, n, d, D,
                       (unsigned*)img, meta, scale, unorm);
  else if (vec && pf && d <= 256)
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_rows_quantize_pf<2>), dim3((unsigned)blocks), dim3(256), 0,
                       st, X, n, d, D, (unsigned*)img, meta, scale, unorm);
  else if (vec && pf)
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_rows_quantize_pf<4>), dim3((unsigned)blocks), dim3(256), 0,
                       st, X, n, d, D, (unsigned*)img, meta, scale, unorm);
  else
    hipLaunchKernelGGL(k_rows_quantize, dim3((unsigned)blocks), dim3(256), 0, st, X, n, d, D,
                       (unsigned*)img, meta, scale, unorm, vec);
  CYC_LAUNCH_CHECK("k_rows_quantize");
  return CYC_OK;
}

}  // namespace km8
}  // namespace cyc
