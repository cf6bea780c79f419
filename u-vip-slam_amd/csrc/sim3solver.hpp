// Sim3Solver sets (sim3solver.hip; arithmetic in sim3_core.hpp): what the kernels and the host side share.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sim3_core.hpp"

namespace uvo {

constexpr int kSim3HypPerSolver = 320;  // hypothesis slots per solver of the set = the largest max_iterations: no call can plan more
constexpr int kSim3MaxSolvers = 64;
constexpr int kSim3MaxPoints = 16384;
constexpr int kSim3SubsetStride = 4;    // int32 per hypothesis record: position in the call's list, then the three point indices
constexpr int kSim3HypFloats = 48;      // floats per evaluated hypothesis: T12[16], T21[16], R[9], t[3], s, finite (as 0 / 1), 2 unused

// one listed solver of one iterate call, written by the host
struct Sim3Call {
  int32_t id, n, min_inliers, max_its, iterations, best_count, hyp_off, hyp_n;
  sim3::Cam K1, K2;
};
static_assert(sizeof(Sim3Call) == 64, "Sim3Call is 64 bytes");

// what k_sim3_finish writes per listed solver; the mask words of the returned set follow all records
struct Sim3Result {
  int32_t performed, returned, no_more, inliers, best_count, pad_[3];
  float hyp[32];  // of the returned hypothesis: T12[16], R[9], t[3], s, 3 unused
};
static_assert(sizeof(Sim3Result) == 160, "Sim3Result is 160 bytes");

}  // namespace uvo
