// cv::findFundamentalMat on the device (fundamental.hip): scratch owned by the uvo_klt handle, launches in its stream.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace uvo {

constexpr int kFmCap = 1000;  // hypotheses: maxIters of both estimators

struct DevMem;
struct FmState;
struct FmScratch {              // one device block, sized at uvo_klt_create
  FmState* state = nullptr;
  int32_t* subsets = nullptr;   // [kFmCap][7]
  uint32_t* hyp_end = nullptr;  // [kFmCap] RNG draws consumed once hypothesis h is drawn
  int32_t* nmodels = nullptr;   // [kFmCap] run7Point's count (<= 0: no model)
  double* models = nullptr;     // [kFmCap][3][9]
  double* scores = nullptr;     // [kFmCap][3] inlier count (RANSAC) or median (LMedS); -1 where no model
  uint64_t* jump = nullptr;     // [k_fm_subsets lanes] A^(draws per lane * lane) mod M
};

// what k_fm_replay writes; the n mask bytes follow it (its first 16 bytes are a uvo_fm_info)
struct FmOut {
  int32_t method, iterations, inliers;
  uint32_t rng_draws;
  int32_t overflow, pad_[3];
  double F[9];
  double pad2_[3];
};
static_assert(sizeof(FmOut) == 128, "FmOut is 128 bytes");

int fm_alloc(DevMem& m, FmScratch& f);  // from the handle's memory
// OpenCV's parameter fix-ups (thr <= 0 -> 3, conf outside (DBL_EPSILON, 1 - DBL_EPSILON) -> 0.99); NaN is an argument error
int fm_fixup(double& thr, double& conf);
// n >= 7 point pairs d_p0 / d_p1 ([n][2] float); mask = inlier && d_status[i] (d_status NULL: inlier)
int fm_enqueue(hipStream_t s, const FmScratch& f, const float* d_p0, const float* d_p1, int n, double thr, double conf, const uint8_t* d_status,
               FmOut* d_out, uint8_t* d_mask);

}  // namespace uvo
