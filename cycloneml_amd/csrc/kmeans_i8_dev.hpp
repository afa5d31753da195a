// kmeans_i8_dev.hpp -- what the units of the i8 screen (kmeans_i8*.hip) share
// and nobody else sees: the device helpers of the fixed-point split and its
// error bounds (derivation: the head of kmeans_i8.hip), and the launchers one
// stage calls in another.  kmeans_i8.hpp is the interface of the whole.
#pragma once

#include "kmeans_i8.hpp"

#include <climits>
#include <cstdlib>
#include <type_traits>

#include "common.hpp"

namespace cyc {
namespace km8 {
namespace {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef unsigned v4u __attribute__((ext_vector_type(4)));
typedef double v2d __attribute__((ext_vector_type(2)));

// one f32 ulp toward -inf; f32 rounded down / up from fp64
__device__ __forceinline__ float ulp_dn(float f) {
  const int b = __float_as_int(f);
  if (f == 0.0f) return -__int_as_float(1);
  return __int_as_float(f > 0.0f ? b - 1 : b + 1);
}
__device__ __forceinline__ float fdown(double x) {
  const float f = (float)x;
  return ((double)f > x) ? ulp_dn(f) : f;
}
__device__ __forceinline__ float fup(double x) {
  const float f = (float)x;
  return ((double)f < x) ? -ulp_dn(-f) : f;
}

constexpr int kMinExp = -50, kMaxExp = 50;
constexpr double kEpsF = 0x1p-20;

__device__ __forceinline__ int choose_exp(double m) {
  if (!(m > 0.0)) return kMinExp;
  int E;
  const double f = __builtin_frexp(m, &E);   // m = f 2^E, f in [0.5, 1)
  const int e = (f * 128.0 >= 127.5) ? E + 1 : E;
  return e < kMinExp ? kMinExp : e;          // a coarser grid is always valid
}

// three limbs of v on the 2^(e-7) grid (exact fp64 steps)
__device__ __forceinline__ void quant3(double v, int e, int& a, int& b, int& c) {
  const double u = __builtin_ldexp(v, 7 - e);
  const double ar = __builtin_rint(u);
  const double t = (u - ar) * 128.0;
  const double br = __builtin_rint(t);
  const double cr = __builtin_rint((t - br) * 128.0);
  a = (int)ar;
  b = (int)br;
  c = (int)cr;
}

__device__ __forceinline__ unsigned pack4(const int* v) {
  return (unsigned)(v[0] & 0xff) | ((unsigned)(v[1] & 0xff) << 8) |
         ((unsigned)(v[2] & 0xff) << 16) | ((unsigned)(v[3] & 0xff) << 24);
}

__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = __builtin_fmax(v, __shfl_xor(v, m));
  return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}

// fx (or gc): separable half of the error bound (see the header comment)
__device__ __forceinline__ double err_term(int e, double n1, double mu, int d) {
  const double A = __builtin_ldexp(1.0, e - 22);
  const double kd = 0.502 * (double)d * 0x1p22;
  return (0.5 * mu * A * A + 0.5 * n1 * n1 / mu + kd * A * A) * (1.0 + 0x1p-40);
}

// fx / gc of the TWO-limb screen: |x_j - xh2_j| <= 2^(e-15) (u - a - b/128
// = (t - b)/128 with |t - b| <= 1/2), the dropped b.b' / 2^14 term <=
// d 2^(ex+ec-16) = d 2^14 A2x A2c <= 0.5 d 2^14 (A2x^2 + A2c^2) (AM-GM);
// A2 carries a 2^-7 slack.  n1 must bound |xh2|_1 (rows) or |c|_1 (centers).
// fx / gc of the ONE-limb screen: |x_j - xh1_j| <= 2^(e-8) (a = rint(u)),
// no dropped products (S1 = a.a' exactly): |x.c - xh1.ch1| <= A1x |c|_1 +
// A1c |xh1|_1, split by AM-GM as for the other limb counts; A1 carries a
// 2^-7 slack.  n1 must bound |xh1|_1 (rows) or |c|_1 (centers).
__device__ __forceinline__ double err_term1(int e, double n1, double mu) {
  const double A = __builtin_ldexp(1.0078125, e - 8);
  return (0.5 * mu * A * A + 0.5 * n1 * n1 / mu) * (1.0 + 0x1p-40);
}

__device__ __forceinline__ double err_term2(int e, double n1, double mu, int d) {
  const double A = __builtin_ldexp(1.0078125, e - 15);
  const double kd = 0.502 * (double)d * 0x1p14;
  return (0.5 * mu * A * A + 0.5 * n1 * n1 / mu + kd * A * A) * (1.0 + 0x1p-40);
}

// Carried bounds (kmeans_i8.hpp Bounds) from a screen's computed bounds.
// With Lt_c = |c|^2 - 2 x.c and L'_c = cq_c - 2 s_c its exact integer form
// (cq_c <= |c|^2 - 2 g_c, |x.c - s_c| <= fx + g_c): Lt_c >= L'_c - 2 fx, and
// a computed bound l is within enc of L' (the integer passes' index bits and
// floors; 0 for the three-limb f32 bounds, whose rounding the 2^-20 slack
// covers together with xx = xnorm^2, within 2^-44 xx of the true |x|^2).
// Every center whose computed bound is >= l therefore has
//   |x - c|^2 >= xx + l - enc - 2 fx                       (bnd_lb_sq)
// and the winner, bound l1, |x - c_w|^2 <= xx + l1 + enc + 2 fx + 4 g_w
// + eps |c_w|^2 (cq rounded down; the 2^-20 terms as in the margins M).
// `extra`: a further slack (the f32 three-limb bounds: 2^-20 max cq).
__device__ __forceinline__ double bnd_ub_sq(double xx, double cc, double l1, double fx, double gw,
                                            double enc) {
  return (xx + l1 + enc + 2.0 * fx + 4.0 * gw + 2.0 * kEpsF * (xx + cc) +
          0x1p-20 * (xx + __builtin_fabs(l1) + cc + 2.0 * gw) + 0x1p-90) *
         (1.0 + 0x1p-30);
}
__device__ __forceinline__ double bnd_lb_sq(double xx, double l, double fx, double enc,
                                            double extra) {
  return xx + l - enc - 2.0 * fx - 2.0 * kEpsF * xx -
         0x1p-20 * (xx + __builtin_fabs(l) + 2.0 * fx + enc) - extra;
}
// as f32 distances: up rounded up; a lower bound <= 0 (or NaN) is "none" (-1)
__device__ __forceinline__ float bnd_dist_up(double s2) {
  return fup(__builtin_sqrt(s2) * (1.0 + 0x1p-50));
}
__device__ __forceinline__ float bnd_dist_dn(double s2) {
  return s2 > 0.0 ? fdown(__builtin_sqrt(s2) * (1.0 - 0x1p-50)) : -1.0f;
}

}  // namespace

// Where a kernel appends rows (and, with cands, their candidate sets): a list
// with its counter, or a shard set of the AppendStage with its counters.
struct AppendTarget {
  int32_t* rows = nullptr;
  unsigned int* count = nullptr;
  int32_t* cands = nullptr;
};

// kmeans_i8_centers.hip
int launch_zero_counters(const ZeroArgs& z, hipStream_t st);
int launch_center_nbrs(const double* stats, int k, int32_t* nbr, float* nbrR, hipStream_t st);

// kmeans_i8_cands.hip (d <= 256).  launch_cands: the fp64 candidate pass over
// ca's candidate rows, undecided rows to `out`.  launch_cands3: the
// three-limb tier ahead of it, undecided rows and their sets to `out`; bd
// (optional): it writes the rows' bounds and carried sets.  launch_recheck:
// the rows of bd.rcRows against their carried sets, in the form
// recheck_two_phase() picks.  scap: `out` is a shard set of that capacity.
int launch_cands(const CandArgs& ca, int64_t n, int d, int32_t* assign, const AppendTarget& out,
                 hipStream_t st, unsigned int scap = 0);
int launch_cands3(const ScreenCall& sc, const CandArgs& ca, const AppendTarget& out,
                  unsigned int scap, const Bounds* bd = nullptr);
int launch_recheck(const ScreenCall& sc, const Bounds& bd);

// kmeans_i8_lists.hip: up to kMaxCompactJobs compactions (compact() each) of
// distinct count sets and destination counters in one launch.
struct CompactJob {
  unsigned int* counts;
  const int32_t* src;
  int32_t* dst;
  int width;
  const int32_t* src2;
  int32_t* dst2;
  int width2;
  unsigned int* dstCount;
};
constexpr int kMaxCompactJobs = 4;
int compact_jobs(const CompactJob* jobs, int nj, unsigned int cap, hipStream_t st);

}  // namespace km8
}  // namespace cyc
