// Visual-inertial bundle adjuster (navba.hip; arithmetic and the launch sequence in navba_core.hpp): what the kernels and the host
// side share.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "navba_core.hpp"

namespace uvo {

// the arrays the host writes per call; the same description places them on the device and in the page-locked mirror
struct NavBaUpload {
  navopt::State* kf_in;
  int32_t *kf_free, *free_kf;
  uint8_t* kf_bias;
  float* pts;
  uint8_t* pt_bad;
  int32_t *pt_begin, *e_kf, *e_pt, *e_cam;
  float *e_obs, *cams;
  int32_t *kl_begin, *kl_edge, *fp_edge;
  navba::Link* links;
  navba::Depth* depths;
  navba::Params* prm;
};

// the arrays the host reads per call
struct NavBaDownload {
  navopt::State* kf_out;
  float* kf_T_out;
  double* pt_est;
  float* pt_out;
  uint8_t *excluded, *erased;
  navba::Ctl* ctl;
};

static_assert(sizeof(navopt::State) == 22 * 8 && sizeof(navba::Link) == 8 + 8 * 142 && sizeof(navba::Depth) == 40 && sizeof(navba::Params) == 17 * 8,
              "the C ABI's records are the core's");

}  // namespace uvo
