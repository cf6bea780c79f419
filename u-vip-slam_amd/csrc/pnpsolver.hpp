// PnPsolver sets (pnpsolver.hip; arithmetic in pnpsolver_core.hpp and epnp_core.hpp): what the kernels and the host side share, and
// the two things a set borrows from the uvo_klt handle it is created on.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pnpsolver_core.hpp"

struct uvo_klt;

namespace uvo {

hipStream_t klt_stream(const uvo_klt* k);  // klt.hip
int klt_device(const uvo_klt* k);

constexpr int kPnpsHypPerSolver = 320;   // hypothesis slots per solver of the set; one call may spend them unevenly
constexpr int kPnpsMaxSolvers = 64;
constexpr int kPnpsMaxPoints = 16384;    // 256 mask words: one per lane of the finishing workgroup
constexpr int kPnpsSubsetStride = 9;     // int32 per hypothesis record: position in the call's list, then up to 8 point indices

// one listed solver of one iterate call, written by the host
struct PnpsCall {
  int32_t id, n, min_set, min_inliers, max_its, iterations, best_count, parity;
  int32_t hyp_off, hyp_n, n_iterations, pad_;
  double fu, fv, uc, vc;
};
static_assert(sizeof(PnpsCall) == 80, "PnpsCall is 80 bytes");

// what k_pnps_finish writes per listed solver; the mask words of the returned set follow all records
struct PnpsResult {
  int32_t performed, returned, no_more, inliers, best_count, pad_[3];
  double pose[12];  // R row-major, t: the refined pose, or the best one at exhaustion
};
static_assert(sizeof(PnpsResult) == 128, "PnpsResult is 128 bytes");

}  // namespace uvo
