// Host build of the Sim3 optimisation: csrc/sim3opt_core.hpp compiled by the host compiler with -ffp-contract=off, the same source
// k_sim3_optimize runs, with sim3opt::HostTeam walking the reduction shape of 256 lanes.  tests/sim3opt_checks.py holds it to the numpy
// model (tests/sim3opt_model.py) layer by layer; tests/test_gpu_sim3opt.py holds the device to it bit for bit.
//
// Seven seeded mutations exist behind -DSIM3OPT_MUT=k of THIS file only (the library has none), to show that the checks can fail:
// 1 e21 through the forward map, 2 a one-sided difference (e(+) - e in place of e(+) - e(-), the scalar kept: half the column),
// 3 round 2 always 10 iterations, 4 removed pairs re-admitted in round 2, 5 info2 inverted, 6 exp(x) as 1 + x, 7 S12 written on the
// early return; and two in the Levenberg driver: 8 the 1e-3 left off scale, 9 ni not doubled after a rejected trial.
//
// With -DSIM3OPT_EMU_MAIN the file is a stand-alone program that runs the committed scene list (the file named by its argument:
// tests/golden/sim3opt_scenes.bin) and a list of seeded scenes of its own (the sizes of the GPU tests) once: the form in which it is
// run under -fsanitize=address,undefined.
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/uvo/uvo.h"
#include "../../u-vip-slam_amd/csrc/sim3opt_core.hpp"

#ifndef SIM3OPT_MUT
#define SIM3OPT_MUT 0
#endif

using namespace uvo;

static_assert(sizeof(uvo_sim3_opt_trace) == sizeof(sim3opt::Trace), "uvo_sim3_opt_trace is sim3opt::Trace");

namespace {
void unpack(const double v[8], sim3opt::Sim& S) {
  for (int e = 0; e < 4; ++e) S.q[e] = v[e];
  for (int e = 0; e < 3; ++e) S.t[e] = v[4 + e];
  S.s = v[7];
}
void pack(const sim3opt::Sim& S, double v[8]) {
  for (int e = 0; e < 4; ++e) v[e] = S.q[e];
  for (int e = 0; e < 3; ++e) v[4 + e] = S.t[e];
  v[7] = S.s;
}
}  // namespace

extern "C" {

int emu_sim3opt_mutation() { return SIM3OPT_MUT; }

double emu_sim3opt_exp(double x) { return sim3opt::exp_<SIM3OPT_MUT>(x); }

// Sim3(R, t, s) from floats: q (x y z w), t, s
void emu_sim3opt_from_floats(const float* R12, const float* t12, float s12, double* sim) {
  sim3opt::Sim S;
  sim3opt::sim_of(R12, t12, s12, S);
  pack(S, sim);
}

// Sim3(dx) * sim
void emu_sim3opt_oplus(const double* dx, const double* sim, double* out) {
  sim3opt::Sim S, Q;
  unpack(sim, S);
  sim3opt::oplus<SIM3OPT_MUT>(dx, S, Q);
  pack(Q, out);
}

// the 24 words of a similarity: s R | t of map() and of inverse()
void emu_sim3opt_mats(const double* sim, double* M) {
  sim3opt::Sim S;
  unpack(sim, S);
  sim3opt::mats_of(S, M);
}

// the library's host-side gather of one pair: 12 floats
void emu_sim3opt_pack_pair(const float* R1w, const float* t1w, const float* R2w, const float* t2w, const float* x1w, const float* x2w, const float* obs1,
                           const float* obs2, float info1, float info2, float* e) {
  sim3opt::pack_pair(R1w, t1w, R2w, t2w, x1w, x2w, obs1, obs2, info1, info2, e);
}

// one linearisation over the pairs whose state byte is 0: sums = H[28] b[7] chi2 through the team's shape, chi2 [n][2] the edges' own
void emu_sim3opt_linearise(const double* sim, const float* K1, const float* K2, const float* pairs, const uint8_t* state, int n, float th2, double* sums,
                           double* chi2) {
  sim3opt::Sim S;
  unpack(sim, S);
  static sim3opt::HostTeam T;
  for (int k = 0; k < sim3opt::kSims; ++k) sim3opt::build_sim<SIM3OPT_MUT>(S, k, T.sims() + k * sim3opt::kSimWords);
  std::vector<double> c2(2 * (size_t)n + 2);
  std::vector<uint8_t> st(state, state + n), m((size_t)n + 1);
  st.push_back(0);
  const sim3opt::Pairs E = {pairs, c2.data(), st.data(), m.data(), n};
  const sim3opt::Cams C = {K1, K2};
  const double delta = sim3opt::delta_of(th2);
  T.sum<sim3opt::kHalf>([&](int lane, double* acc) { sim3opt::lane_linearise<SIM3OPT_MUT, 0>(T.sims(), C, E, delta, lane, acc); }, sums);
  T.sum<sim3opt::kHalf>([&](int lane, double* acc) { sim3opt::lane_linearise<SIM3OPT_MUT, 1>(T.sims(), C, E, delta, lane, acc); }, sums + sim3opt::kHalf);
  if (chi2 && n > 0) std::memcpy(chi2, c2.data(), sizeof(double) * 2 * (size_t)n);
}

// (H + lambda I) x = b; returns ok
int emu_sim3opt_solve(const double* H, double lambda, const double* b, double* x) { return sim3opt::solve7(H, lambda, b, x) ? 1 : 0; }

// one trial from given H, b, lambda, estimate and currentChi: solve, oplus, the robust chi2 at the tried estimate over the pairs whose
// state byte is 0 (through the team's shape), scale and rho.  Returns ok; dx is written only then (it comes in as the previous step);
// tmp is DBL_MAX after a failed solve.  out = tmp, scale, rho.
int emu_sim3opt_trial(const double* H, double lambda, const double* b, const double* sim, double cur, const float* K1, const float* K2, const float* pairs,
                      const uint8_t* state, int n, float th2, double* dx, double* sim_out, double* out) {
  sim3opt::Sim S, Q;
  unpack(sim, S);
  const bool ok = sim3opt::solve7(H, lambda, b, dx);
  sim3opt::oplus<SIM3OPT_MUT>(dx, S, Q);
  pack(Q, sim_out);
  double M[sim3opt::kSimWords], tmp;
  sim3opt::mats_of(Q, M);
  std::vector<double> c2(2 * (size_t)n + 2);
  std::vector<uint8_t> st(state, state + n), m((size_t)n + 1);
  st.push_back(0);
  const sim3opt::Pairs E = {pairs, c2.data(), st.data(), m.data(), n};
  const sim3opt::Cams C = {K1, K2};
  const double delta = sim3opt::delta_of(th2);
  static sim3opt::HostTeam T;
  T.sum<1>([&](int lane, double* acc) { sim3opt::lane_robust_chi2<SIM3OPT_MUT>(M, C, E, delta, lane, acc); }, &tmp);
  if (!ok) tmp = DBL_MAX;
  const double scale = sim3opt::trial_scale<SIM3OPT_MUT>(dx, lambda, b);
  out[0] = tmp, out[1] = scale, out[2] = (cur - tmp) / scale;
  return ok ? 1 : 0;
}

// the call.  pairs [n][12]; out: uvo-independent record q[4] t[3] s | R12[9] t12[3] scale | n_inliers n_corr n_bad more; mask [n]
void emu_sim3opt_optimize(const float* pairs, int n, const float* K1, const float* K2, const float* R12, const float* t12, float s12, float th2, double* est,
                          float* estf, int32_t* counts, uint8_t* mask, uvo_sim3_opt_trace* trace) {
  std::vector<double> chi2(2 * (size_t)n + 2);
  std::vector<uint8_t> state((size_t)n + 1), m((size_t)n + 1);
  const sim3opt::Pairs E = {pairs, chi2.data(), state.data(), m.data(), n};
  const sim3opt::Cams C = {K1, K2};
  static sim3opt::HostTeam T;
  sim3opt::Out out;
  if (trace) std::memset(trace, 0, sizeof *trace);
  sim3opt::run<SIM3OPT_MUT>(T, E, C, R12, t12, s12, th2, &out, reinterpret_cast<sim3opt::Trace*>(trace));
  std::memcpy(est, out.q, sizeof(double) * 8);   // q, t, s are adjacent
  std::memcpy(estf, out.R12, sizeof(float) * 13);  // R12, t12, scale are adjacent
  counts[0] = out.n_inliers, counts[1] = out.n_correspondences, counts[2] = out.n_bad, counts[3] = out.more_iterations;
  if (mask && n > 0) std::memcpy(mask, m.data(), (size_t)n);
}

}  // extern "C"

static_assert(offsetof(sim3opt::Out, s) == 56 && offsetof(sim3opt::Out, scale) == 64 + 48, "q t s and R12 t12 scale are adjacent");

#ifdef SIM3OPT_EMU_MAIN
#include <cstdio>

namespace {
struct Lcg {
  uint64_t s;
  double next() {  // in [0, 1)
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(s >> 11) * (1. / 9007199254740992.);
  }
};

int run_one(const char* what, const std::vector<float>& pairs, int n, const float* K1, const float* K2, const float* R12, const float* t12, float s12, float th2) {
  double est[8];
  float estf[13];
  int32_t c[4] = {-1, -1, -1, -1};
  std::vector<uint8_t> mask((size_t)n + 1);
  static uvo_sim3_opt_trace tr;
  emu_sim3opt_optimize(pairs.data(), n, K1, K2, R12, t12, s12, th2, est, estf, c, mask.data(), &tr);
  std::printf("%s n %d: inliers %d bad %d more %d lin %d trials %d s = %.9g t = %g %g %g\n", what, n, c[0], c[2], c[3], tr.n_lin, tr.n_trials, est[7], est[4], est[5],
              est[6]);
  return c[0] < 0 || c[0] > n || c[1] != n || c[2] < 0 || c[2] > n || (c[3] != 0 && c[3] != 5 && c[3] != 10) || tr.n_lin > 15 || tr.n_trials > 150;
}

// n points seen by two cameras related by a similarity a little off the start; `shifted` of them moved by 8 px in image 2
int scene(uint64_t seed, int n, int shifted) {
  Lcg g{seed * 2654435761ull + 12345};
  const float K1[4] = {458.f, 457.f, 367.f, 248.f}, K2[4] = {460.f, 459.f, 365.f, 250.f};
  const float R12[9] = {1.f, 0.f, 0.f, 0.f, 0.9998f, -0.02f, 0.f, 0.02f, 0.9998f}, t12[3] = {0.33f, -0.18f, 0.08f};
  const float s12 = 1.03f;
  std::vector<float> p((size_t)n * 12 + 12);
  for (int i = 0; i < n; ++i) {
    const double x = (g.next() - 0.5) * 6., y = (g.next() - 0.5) * 4., z = 3. + g.next() * 6.;  // in camera 2
    const double X1[3] = {1.05 * x + 0.3, 1.05 * (y - 0.01 * z) - 0.2, 1.05 * (0.01 * y + z) + 0.1};  // in camera 1: scale 1.05, a small rotation, a baseline
    float* r = &p[(size_t)i * 12];
    r[0] = (float)X1[0], r[1] = (float)X1[1], r[2] = (float)X1[2], r[3] = (float)x, r[4] = (float)y, r[5] = (float)z;
    r[6] = (float)(K1[0] * X1[0] / X1[2] + K1[2] + (g.next() - 0.5)), r[7] = (float)(K1[1] * X1[1] / X1[2] + K1[3] + (g.next() - 0.5));
    r[8] = (float)(K2[0] * x / z + K2[2] + (g.next() - 0.5)) + (i < shifted ? 8.f : 0.f), r[9] = (float)(K2[1] * y / z + K2[3] + (g.next() - 0.5));
    r[10] = i % 3 == 0 ? 1.f : 0.694444f, r[11] = i % 3 == 0 ? 1.f : 1.44f;
  }
  char what[64];
  std::snprintf(what, sizeof what, "seed %llu shifted %d", (unsigned long long)seed, shifted);
  return run_one(what, p, n, K1, K2, R12, t12, s12, 10.f);
}

// the committed scene list (tests/golden/sim3opt_scenes.bin, written by tests/sim3opt_model.py's dump): int32 count; per scene int32 n,
// float th2, K1[4], K2[4], R12[9], t12[3], s12, then n x 12 floats
int scene_file(const char* path) {
  FILE* f = std::fopen(path, "rb");
  if (!f) return 1;
  int32_t count = 0;
  int bad = std::fread(&count, 4, 1, f) != 1 || count < 0 || count > 1000;
  for (int s = 0; s < count && !bad; ++s) {
    int32_t n = 0;
    float h[22];
    if (std::fread(&n, 4, 1, f) != 1 || n < 0 || n > 16384 || std::fread(h, 4, 22, f) != 22) {
      bad = 1;
      break;
    }
    std::vector<float> p((size_t)n * 12 + 12);
    if (n && std::fread(p.data(), 48, (size_t)n, f) != (size_t)n) {
      bad = 1;
      break;
    }
    char what[32];
    std::snprintf(what, sizeof what, "scene %d", s);
    bad = run_one(what, p, n, h + 1, h + 5, h + 9, h + 18, h[21], h[0]);
  }
  std::fclose(f);
  return bad;
}
}  // namespace

int main(int argc, char** argv) {
  int bad = 0;
  if (argc > 1) bad += scene_file(argv[1]);
  const int sizes[] = {0, 1, 9, 10, 11, 63, 64, 65, 255, 256, 257, 513, 1024, 1025, 3000};
  uint64_t seed = 1;
  for (int n : sizes) bad += scene(seed++, n, 0);
  for (int n : {30, 100, 300}) bad += scene(seed++, n, n / 5);
  bad += scene(seed++, 12, 12);
  bad += scene(seed++, 15, 6);
  std::printf("%s\n", bad ? "FAILED" : "ok");
  return bad ? 1 : 0;
}
#endif
