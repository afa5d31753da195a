// kmeans_fp64.hpp -- the dense KMeans screens that decide in fp64 and the
// exact tier behind them (kmeans_fp64.hip), for the Euclidean plan of
// kmeans.hip.  Plain pointers and the plan's Sizing; no plan type here.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "common.hpp"

namespace cyc {
namespace kmfp64 {

// Everything the screens derive from (d, k) alone, filled by sizing().
struct Sizing {
  int d = 0, k = 0, d4 = 0, kpad = 0;   // d4: d rounded up to 4, kpad: k to 16
  // k_kmeans_assign: rows per workgroup (0: d > 1216, no LDS-resident dense
  // assign), LDS row stride (== 2 mod 32 doubles) and bytes
  int bm = 0, ldsStride = 0;
  size_t assignLds = 0;
  int variant = 1;          // 2: k_kmeans_assign2 (fp64 screen), 3: bf16x3 screen
  // variant 2: row stride d4 + 1 (== 1 mod 16 doubles: the two 16-lane
  // halves of a ds_read2_b64 fragment read hit distinct banks)
  int ldsStride2 = 0;
  size_t assignLds2 = 0;
  // bf16x3 screen (variant 3): k-steps of 32 dims, padded 16-center tiles,
  // LDS bytes, error-bound constants
  int ks3 = 0, ktp3 = 0;
  size_t lds3 = 0;
  double omE3 = 1.0, tauL3 = 0.0, facU3 = 0.0, tauU3 = 0.0;
};

// want (the CYC_KMEANS_ASSIGN test hook, 0: none): the screen tier a plan
// uses without a row image -- 1 fp64 screen, 2 fp64 screen with the
// conflict-free stride, 3 bf16x3 screen in front of it; taken where it fits.
Sizing sizing(int d, int k, int want);

// The fp64 MFMA screen (k_kmeans_assign, or k_kmeans_assign2 for variants 2
// and 3) with bm rows per workgroup over every row, or over the rowCount[0]
// rows of rowList; undecided rows are appended to slowList / slowCount.
int launch_assign(const Sizing& s, int bm, const double* X, const double* xnorm, int64_t n,
                  const double* C, const double* cnorm, const double* ct, int32_t* assign,
                  double* cost, int32_t* slowList, unsigned int* slowCount, hipStream_t st,
                  const int32_t* rowList = nullptr, const unsigned int* rowCount = nullptr);

// The bf16x3 screen over every row (variant 3): the centers' split image
// into cb3 / cq3 (k_center_split; ok3 cleared by a center beyond the cap),
// then k_kmeans_assign3; undecided rows go to list3 / list3Count.
int launch_assign3(const Sizing& s, const double* X, const double* xnorm, int64_t n,
                   const double* C, const double* cnorm, void* cb3, float* cq3, int* ok3,
                   int32_t* assign, double* cost, int32_t* list3, unsigned int* list3Count,
                   hipStream_t st);

// The exact tier over the slow queue: the split kernels for a queue of
// <= 512 rows (allowSplit), k_assign_exact for a longer one; known = the
// queue's length when the host has it (-1: decided on the device, both
// enqueued).  exactDist: the split kernels' distances, grown here.
int launch_exact(const Sizing& s, const double* X, const double* xnorm, int64_t n,
                 const double* C, const double* cnorm, const double* ct, const double* statsArg,
                 const int32_t* slowList, const unsigned int* slowCount, DeviceBuffer& exactDist,
                 int32_t* assign, double* cost, bool approxNorm, int64_t known, bool allowSplit,
                 hipStream_t st);

}  // namespace kmfp64
}  // namespace cyc
