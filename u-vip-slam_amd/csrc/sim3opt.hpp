// Sim3 optimizer sets (sim3opt.hip; arithmetic in sim3opt_core.hpp): what the kernel and the host side share.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sim3opt_core.hpp"

namespace uvo {

constexpr int kSim3OptMaxProblems = 64;
constexpr int kSim3OptMaxPairs = 16384;
constexpr int kSim3OptLdsPairs = 1024;  // up to here a problem's two chi2 and its state byte per pair live in LDS (17 KiB), beyond in the set's block

// one problem of one call, written by the host; the pairs of all problems follow the records, packed in problem order
struct Sim3OptProblemDev {
  int32_t n, off;  // off: index of its first pair among the call's
  float K1[4], K2[4];  // fx fy cx cy
  float R12[9], t12[3], s12, th2;
};
static_assert(sizeof(Sim3OptProblemDev) == 96, "Sim3OptProblemDev is 96 bytes");
static_assert(sizeof(sim3opt::Out) == 136, "sim3opt::Out is 136 bytes");

}  // namespace uvo
