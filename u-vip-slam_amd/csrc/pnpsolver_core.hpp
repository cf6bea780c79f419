// PnPsolver (src/PnPsolver.cc of the reference, the RANSAC around EPnP that Tracking::Relocalisation runs per candidate key frame) as
// plain C++: everything of it that is not the EPnP itself, which is pnp::solve of epnp_core.hpp on pixel coordinates.  pnpsolver.hip
// runs this on the device, tests/emu/pnpsolver_emu.cpp on the host; the two are held to each other bit for bit under the rules of
// epnp_core.hpp's header (sqrt and fabs only on the shared path, no contraction, every lane owns whole scalars).
//
// The source is followed line by line where it does what one would not write today:
//   * the random stream is libc's rand() and the subset draw can repeat a point: both are glibc_rand.hpp, which Sim3Solver shares;
//   * SetRansacParameters' exponent is a literal 3; iterate's loop condition is an OR; Refine runs on the best set whether or not the
//     hypothesis was a new best and succeeds only with strictly more than nMinInliers;
//   * CheckInliers mixes float and double, and every rounding of it is kept.
// derive_params uses pow / log / ceil and is HOST ONLY: the library computes it when a solver is added, the device never does.
#pragma once
#include "epnp_core.hpp"
#include "glibc_rand.hpp"

namespace uvo {
namespace pnps {

constexpr int kMinSetLo = 4, kMinSetHi = 8;

// ---- SetRansacParameters :122-158 (host only) --------------------------------------------------------------------------------------
struct Params {
  double probability;
  int min_inliers, max_iterations, min_set;
  float epsilon, th2;
};
struct Derived {
  int n, min_inliers, max_its;
};
inline Derived derive_params(int n, const Params& p) {
  float eps = p.epsilon;
  int m = (int)((float)n * eps);
  if (m < p.min_inliers) m = p.min_inliers;
  if (m < p.min_set) m = p.min_set;
  if (eps < (float)m / (float)n) eps = (float)m / (float)n;
  double its = 1.;
  if (m != n) its = ceil(log(1. - p.probability) / log(1. - pow((double)eps, 3.)));
  // min(nIterations, maxIterations) where the ratio is an int.  Where it is not, the reference's conversion is undefined: a ratio too
  // large for an int means maxIterations; NaN (epsilon raised past 1: fewer points than nMinInliers, a solver that never iterates)
  // gives 1, which is also what the reference's x86 build makes of it
  int it = its < (double)p.max_iterations ? (int)its : p.max_iterations;
  if (it < 1 || its != its) it = 1;
  return Derived{n, m, it};
}

// ---- CheckInliers :309-340 for one point ------------------------------------------------------------------------------------------
PNP_HD bool check_inlier(const double* R, const double* t, const float* P, const float* m, double fu, double fv, double uc, double vc, float max_error) {
  const float Xc = (float)(R[0] * P[0] + R[1] * P[1] + R[2] * P[2] + t[0]);
  const float Yc = (float)(R[3] * P[0] + R[4] * P[1] + R[5] * P[2] + t[1]);
  const float invZc = (float)(1 / (R[6] * P[0] + R[7] * P[1] + R[8] * P[2] + t[2]));
  const double ue = uc + fu * Xc * invZc;
  const double ve = vc + fv * Yc * invZc;
  const float distX = (float)(m[0] - ue);
  const float distY = (float)(m[1] - ve);
  const float error2 = distX * distX + distY * distY;
  return error2 < max_error;
}

// ---- iterate :166-259 over hypotheses that were all evaluated beforehand -----------------------------------------------------------
// what persists in a solver between calls (with the best set and the best pose, which the caller's Ops keep)
struct State {
  int32_t iterations;  // mnIterations
  int32_t best_count;  // mnBestInliers
};
enum : int32_t { kNone = 0, kRefined = 1, kBestAtExhaustion = 2 };
struct Outcome {
  int32_t performed;  // iterations of this call = hypotheses consumed
  int32_t returned;   // kNone / kRefined / kBestAtExhaustion
  int32_t no_more;    // bNoMore
  int32_t inliers;    // nInliers
};

// the iterations one call runs unless it returns early: the loop condition is an OR
PNP_HD int iterations_ahead(int iterations_so_far, int max_its, int n_iterations) {
  const int a = max_its - iterations_so_far;
  const int k = a > n_iterations ? a : n_iterations;
  return k > 0 ? k : 0;
}

// Ops: take_best(h) makes hypothesis h's pose and inlier set the best; refine() is Refine() on the current best set and returns its
// count (0 where EPnP gave no finite pose).  Refine's outcome depends on the best set only, so Ops may keep it until take_best.
template <class Ops>
PNP_HD Outcome replay(State& st, const int32_t* counts, int n_iterations, int max_its, int min_inliers, Ops& ops) {
  Outcome o = {0, kNone, 0, 0};
  int cur = 0;
  while (st.iterations < max_its || cur < n_iterations) {
    const int c = counts[cur];
    ++cur, ++st.iterations;
    if (c >= min_inliers) {
      if (c > st.best_count) {
        st.best_count = c;
        ops.take_best(cur - 1);
      }
      const int r = ops.refine();
      if (r > min_inliers) {
        o.performed = cur, o.returned = kRefined, o.inliers = r;
        return o;
      }
    }
  }
  o.performed = cur, o.no_more = 1;
  if (st.best_count >= min_inliers) o.returned = kBestAtExhaustion, o.inliers = st.best_count;
  return o;
}

}  // namespace pnps
}  // namespace uvo
