// Visual-inertial bundle adjuster (navba.hip; arithmetic and the launch sequence in navba_core.hpp): what the kernels and the host
// side share beyond ba.hpp, whose team, kernel macro, executor and graph exchange it uses.
#pragma once
#include "ba.hpp"
#include "navba_core.hpp"

namespace uvo {

using NavBaTeam = BaTeam;

// the inertial arrays the host writes per call, in front of ba.hpp's graph on the device and in the page-locked mirror
struct NavBaInertial {
  navopt::State* kf_in;
  navba::Link* links;
  navba::Depth* depths;
  navba::Params* prm;
  uint8_t* kf_bias;
  void layout(Carve& c, size_t K, size_t D) { c.take(kf_in, K).take(links, (size_t)navba::kMaxLinks).take(depths, D + 1).take(prm, 1).take(kf_bias, K); }
};

static_assert(sizeof(navopt::State) == 22 * 8 && sizeof(navba::Link) == 8 + 8 * 142 && sizeof(navba::Depth) == 40 && sizeof(navba::Params) == 17 * 8,
              "the C ABI's records are the core's");
static_assert(navba::kMaxCams == ba::kMaxCams, "BaGraph's cameras");

}  // namespace uvo
