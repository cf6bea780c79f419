// The strip plan (u-vip-slam_amd/csrc/strip_plan.hpp) of a window, for tests that choose image sizes by the plan they produce:
// out = {nfull, nseg, items, sub[0], sub[1], x0[0], x0[1]}.
#include "../../u-vip-slam_amd/csrc/strip_plan.hpp"

extern "C" void emu_strip_plan(int w, int h, int rows_per_seg, int* out) {
  uvo::StripPlan P;
  uvo::fast_strip_plan(w, h, rows_per_seg, P);
  out[0] = P.nfull, out[1] = P.nseg, out[2] = P.items, out[3] = P.sub[0], out[4] = P.sub[1], out[5] = P.x0[0], out[6] = P.x0[1];
}
