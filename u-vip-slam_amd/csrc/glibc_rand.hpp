// The random stream of the reference's RANSACs (PnPsolver, Sim3Solver, Initializer) as plain C++: libc's rand() as DUtils::Random::RandomInt
// calls it (never seeded: srand(1)), restated as a value type so that the library can draw ahead without touching the process's
// generator, and the subset draw both solvers make from it, which removes the slot named by the drawn VALUE, not the drawn position, so
// a minimal set can repeat a point.  The names stay in namespace pnps, where every caller and the host builds of tests/emu look for them.
#pragma once
#include <stdint.h>

#ifndef PNP_HD  // epnp_core.hpp's
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PNP_HD __host__ __device__ inline
#else
#define PNP_HD inline
#endif
#endif

namespace uvo {
namespace pnps {

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

}  // namespace pnps
}  // namespace uvo
