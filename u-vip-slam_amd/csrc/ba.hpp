// Bundle adjuster (ba.hip; arithmetic and the launch sequence in ba_core.hpp): what the kernels and the host side share.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ba_core.hpp"

namespace uvo {

// the arrays the host writes per call; the same description places them on the device and in the page-locked mirror
struct BaUpload {
  float* kf_T;
  int32_t *kf_free, *free_kf;
  float* pts;
  uint8_t* pt_bad;
  int32_t *pt_begin, *e_kf, *e_pt, *e_cam;
  float *e_obs, *cams;
  int32_t *kl_begin, *kl_edge, *fp_edge;
};

// the arrays the host reads per call
struct BaDownload {
  double* kf_est;
  float* kf_T_out;
  double* pt_est;
  float* pt_out;
  uint8_t *removed1, *removed2;
  ba::Ctl* ctl;
};

static_assert(sizeof(ba::TraceLin) == 40 && sizeof(ba::Ctl) == 80, "ba::TraceLin is 40 bytes, ba::Ctl 80");

}  // namespace uvo
