// PnPsolver (src/PnPsolver.cc of the reference, the RANSAC around EPnP that Tracking::Relocalisation runs per candidate key frame) as
// plain C++: everything of it that is not the EPnP itself, which is pnp::solve of epnp_core.hpp on pixel coordinates.  pnpsolver.hip
// runs this on the device, tests/emu/pnpsolver_emu.cpp on the host; the two are held to each other bit for bit under the rules of
// epnp_core.hpp's header (sqrt and fabs only on the shared path, no contraction, every lane owns whole scalars).
//
// The source is followed line by line where it does what one would not write today:
//   * the random stream is libc's rand() (DUtils::Random::RandomInt, never seeded: srand(1)), restated as a value type so that the
//     library can draw ahead without touching the process's generator;
//   * the subset draw removes the slot named by the drawn VALUE, not the drawn position, so a minimal set can repeat a point;
//   * SetRansacParameters' exponent is a literal 3; iterate's loop condition is an OR; Refine runs on the best set whether or not the
//     hypothesis was a new best and succeeds only with strictly more than nMinInliers;
//   * CheckInliers mixes float and double, and every rounding of it is kept.
// derive_params uses pow / log / ceil and is HOST ONLY: the library computes it when a solver is added, the device never does.
#pragma once
#include "epnp_core.hpp"

namespace uvo {
namespace pnps {

constexpr int kMinSetLo = 4, kMinSetHi = 8;

// ---- glibc's default generator (TYPE_3: x^31 + x^3 + 1) ---------------------------------------------------------------------------
// 34 words of history in a ring and the position of the next output.  Equal to srand / rand for seeds in [0, 2^31); seed 0 is seed 1.
struct GlibcRand {
  int32_t r[34];
  int32_t k;
  PNP_HD void srand(uint32_t seed) {
    int32_t w = seed == 0 ? 1 : (int32_t)seed;
    r[0] = w;
    for (int i = 1; i < 31; ++i) {  // the 16807 Lehmer step in Schrage's form
      const int32_t hi = w / 127773, lo = w % 127773;
      w = 16807 * lo - 2836 * hi;
      if (w < 0) w += 2147483647;
      r[i] = w;
    }
    for (int i = 31; i < 34; ++i) r[i] = r[i - 31];
    k = 0;  // ring position of element 34
    for (int i = 0; i < 310; ++i) (void)next();
  }
  PNP_HD int32_t next() {
    const int a = k + 3 >= 34 ? k + 3 - 34 : k + 3, b = k + 31 >= 34 ? k + 31 - 34 : k + 31;  // elements i - 31 and i - 3
    const uint32_t o = (uint32_t)r[a] + (uint32_t)r[b];
    r[k] = (int32_t)o;
    k = k + 1 == 34 ? 0 : k + 1;
    return (int32_t)(o >> 1);
  }
};

// DUtils::Random::RandomInt (Thirdparty/DBoW2/DUtils/Random.cpp:47-50) with RAND_MAX = 2^31 - 1
PNP_HD int random_int(GlibcRand& g, int lo, int hi) {
  const double d = (double)g.next() / 2147483648.0;
  return (int)(d * (double)(hi - lo + 1)) + lo;
}

// PnPsolver::iterate :189-202 (Sim3Solver.cc:163-177 is the same): `avail` is the caller's n slots; the write lands in slot idx, which
// lies inside them and sometimes past the live length, where nothing reads it again
PNP_HD void draw_subset(GlibcRand& g, int n, int min_set, int32_t* avail, int32_t* out) {
  for (int i = 0; i < n; ++i) avail[i] = i;
  int live = n;
  for (int i = 0; i < min_set; ++i) {
    const int randi = random_int(g, 0, live - 1);
    const int idx = avail[randi];
    out[i] = idx;
    avail[idx] = avail[live - 1];
    --live;
  }
}

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
