// Visual-inertial pose optimizer sets (navopt.hip; arithmetic in navopt_core.hpp): what the kernel and the host side share.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "navopt_core.hpp"
#include "pnpsolver.hpp"  // klt_stream, klt_device

namespace uvo {

constexpr int kNavMaxProblems = 64;
constexpr int kNavMaxPoints = 16384;   // per frame; a problem of the frame form carries up to twice as many edges
constexpr int kNavLdsEdges = 2048;     // up to here a problem's chi2 and state bytes (both frames') live in LDS, beyond in the set's block
constexpr int kNavEdgeFloats = 6;      // an uploaded edge: the point, the observation, invSigma2

static_assert(sizeof(navopt::Problem) % 8 == 0 && sizeof(navopt::Out) % 8 == 0, "records are whole doubles");

}  // namespace uvo
