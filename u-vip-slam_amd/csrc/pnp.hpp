// cv::solvePnPRansac(..., SOLVEPNP_EPNP) on the device (pnp.hip; arithmetic in epnp_core.hpp): scratch owned by the uvo_klt handle,
// launches in its stream.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "epnp_core.hpp"
#include "fundamental.hpp"

namespace uvo {

// what k_pnp_finish writes; the inlier index list (n int32 slots, `inliers` of them used) follows it
struct PnpOut {
  int32_t ok, iterations, inliers;
  uint32_t rng_draws;
  int32_t winner, pad_[3];
  double R[9], t[3];
};
static_assert(sizeof(PnpOut) == 128, "PnpOut is 128 bytes");

struct PnpScratch {  // one device block and its page-locked mirror of the call's input / output, sized at uvo_klt_create
  uint8_t* h_io = nullptr;
  float* io = nullptr;         // obj [n][3] | img [n][2] of the call
  float* und_f = nullptr;      // [max_points][2] normalised image points as cv::undistortPoints stores them for float input
  double* und_d = nullptr;     // [max_points][2] the same in double (the refit's input is converted to double first)
  int32_t* subsets = nullptr;  // [kFmCap][5]
  uint32_t* hyp_end = nullptr; // [kFmCap] RNG draws consumed once hypothesis h is drawn
  double* poses = nullptr;     // [kFmCap][12] R (row-major), t; zeros where EPnP gave no finite pose
  int32_t* counts = nullptr;   // [kFmCap] inliers of the pose; -1 where there is none
  PnpOut* out = nullptr;
  int32_t* inliers = nullptr;  // [max_points] directly behind *out: one download
};

int pnp_alloc(DevMem& m, PnpScratch& p, int max_points);  // from the handle's memory
// n >= 5 points already in p.io; hypotheses = min(iterations, kFmCap) are all evaluated, the replay decides how many count
int pnp_enqueue(hipStream_t s, const PnpScratch& p, int n, const pnp::Cam& cam, int iterations, double thr, double conf);

}  // namespace uvo
