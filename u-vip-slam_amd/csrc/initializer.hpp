// Two-view initialisation (initializer.hip; arithmetic in initializer_core.hpp): what the kernels and the host side share.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "initializer_core.hpp"

namespace uvo {

constexpr int kInitMaxIterations = 1024;  // hypothesis slots of an object = the largest `iterations`
constexpr int kInitMaxKeys = 16384;
constexpr int kInitHypLanes = 64;         // lanes of a workgroup that runs a Jacobi per lane
constexpr int kInitChunk = 2048;          // matches whose score terms one workgroup holds in LDS at a time

// one initialize call, written by the host; keys2 [n2][2], matches12 [n2] and the sets [T][8] follow it in the same upload
struct InitCall {
  int32_t n1, n2, T, words;  // words = ceil(n2 / 64)
  twoview::Norm N1, N2;
  twoview::Cam K;
  float inv_sigma2, th2;
  int32_t pad_[14];
};
static_assert(sizeof(InitCall) == 128, "InitCall is 128 bytes");

// what k_init_select leaves for the two kernels behind it
struct InitSel {
  int32_t best, n_inliers;
  float score, F[9];
  twoview::Motion M;
  int32_t pad_[31];
};
static_assert(sizeof(InitSel) == 256, "InitSel is 256 bytes");

// what k_init_finish writes; the mask words [words], vP3D [n2][3] and vbTriangulated [n2] follow it in the same download
struct InitOut {
  int32_t ok, best, n_inliers, deciding, n_good[4];
  float parallax[4], score, R[9], t[3], F[9];
  int32_t pad_[30];
};
static_assert(sizeof(InitOut) == 256, "InitOut is 256 bytes");

}  // namespace uvo
