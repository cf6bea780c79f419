// Pose optimizer sets (poseopt.hip; arithmetic in poseopt_core.hpp): what the kernel and the host side share.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pnpsolver.hpp"  // klt_stream, klt_device
#include "poseopt_core.hpp"

namespace uvo {

constexpr int kPoseMaxProblems = 64;
constexpr int kPoseMaxPoints = 16384;
constexpr int kPoseLdsEdges = 2048;    // up to here a problem's chi2 and state bytes live in LDS (18 KiB), beyond in the set's block
constexpr int kPoseEdgeFloats = 6;     // an uploaded edge: the point, the observation, invSigma2

// one problem of one call, written by the host; the edges of all problems follow the records, packed in problem order
struct PoseProblemDev {
  int32_t n, off;  // off: index of its first edge among the call's
  float fx, fy, cx, cy;
  float Tcw[16];
  int32_t pad_[2];
};
static_assert(sizeof(PoseProblemDev) == 96, "PoseProblemDev is 96 bytes");
static_assert(sizeof(poseopt::Out) == 72, "poseopt::Out is 72 bytes");

}  // namespace uvo
