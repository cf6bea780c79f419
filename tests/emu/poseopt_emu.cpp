// Host build of the pose-only optimisation: csrc/poseopt_core.hpp compiled by the host compiler with -ffp-contract=off, the same
// source k_pose_optimize runs, with poseopt::HostTeam walking the reduction shape of 256 lanes.  tests/poseopt_checks.py holds it to
// the numpy model (tests/poseopt_model.py) layer by layer; tests/test_gpu_poseopt.py holds the device to it bit for bit.
//
// Six seeded mutations exist behind -DPOSEOPT_MUT=k of THIS file only (the library has none), to show that the checks can fail:
// 1 the Huber weight left off b, 2 flagged edges not re-evaluated before classification, 3 the break test counting active edges,
// 4 lambda initialised once per call, 5 `else if (chi2 <= th)` not restoring the level, 6 the 1e-3 left off scale.
//
// With -DPOSEOPT_EMU_MAIN the file is a stand-alone program that runs the committed scene list (the file named by its argument:
// tests/golden/poseopt_scenes.bin) and a list of seeded scenes of its own (the sizes of the GPU tests, up to 5000 edges) once: the
// form in which it is run under -fsanitize=address,undefined.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/uvo/uvo.h"
#include "../../u-vip-slam_amd/csrc/poseopt_core.hpp"

#ifndef POSEOPT_MUT
#define POSEOPT_MUT 0
#endif

using namespace uvo;

static_assert(sizeof(uvo_pose_trace) == sizeof(poseopt::Trace), "uvo_pose_trace is poseopt::Trace");

namespace {
void unpack(const double qt[7], poseopt::Pose& P) {
  for (int e = 0; e < 4; ++e) P.q[e] = qt[e];
  for (int e = 0; e < 3; ++e) P.t[e] = qt[4 + e];
}
void pack(const poseopt::Pose& P, double qt[7]) {
  for (int e = 0; e < 4; ++e) qt[e] = P.q[e];
  for (int e = 0; e < 3; ++e) qt[4 + e] = P.t[e];
}
}  // namespace

extern "C" {

int emu_pose_mutation() { return POSEOPT_MUT; }

// toSE3Quat: q (x y z w), t
void emu_pose_from_T(const float* Tcw, double* qt) {
  poseopt::Pose P;
  poseopt::pose_of(Tcw, P);
  pack(P, qt);
}

// to_homogeneous_matrix rounded to float, and R in double
void emu_pose_to_T(const double* qt, float* Tcw, double* R) {
  poseopt::Pose P;
  unpack(qt, P);
  poseopt::matrix_of(P, Tcw, R);
}

// layer 1: one edge (6 floats) at a pose: out = e0 e1 chi2 rho0 rho1 J[2][6]
void emu_pose_edge(const double* qt, const float* K, const float* edge, double* out) {
  poseopt::Pose P;
  unpack(qt, P);
  const poseopt::Cam C = {(double)K[0], (double)K[1], (double)K[2], (double)K[3]};
  poseopt::EdgeEval ev;
  poseopt::edge_error(P, C, edge, ev);
  out[0] = ev.e0, out[1] = ev.e1, out[2] = ev.chi2;
  poseopt::huber(ev.chi2, out + 3, out + 4);
  poseopt::jacobian(ev, C, out + 5, out + 11);
}

// layer 2: one linearisation over the edges whose state byte has no level bit: sums = H[21] b[6] chi2, through the team's shape
void emu_pose_linearise(const double* qt, const float* K, const float* edges, const uint8_t* state, int n, double* sums) {
  poseopt::Pose P;
  unpack(qt, P);
  const poseopt::Cam C = {(double)K[0], (double)K[1], (double)K[2], (double)K[3]};
  poseopt::HostTeam T;
  T.sum<poseopt::kSums>(
      [&](int lane, double* acc) {
        for (int i = lane; i < n; i += poseopt::kLanes) {
          if (state[i] & poseopt::kLevel) continue;
          poseopt::EdgeEval ev;
          poseopt::edge_error(P, C, edges + 6 * i, ev);
          double term[poseopt::kSums];
          poseopt::edge_terms<POSEOPT_MUT>(ev, C, term);
          for (int k = 0; k < poseopt::kSums; ++k) acc[k] = acc[k] + term[k];
        }
      },
      sums);
}

// layer 3: one trial from given H, b, lambda, pose and currentChi: solve, oplus, the robust chi2 at the tried pose over the edges whose
// state byte has no level bit (through the team's shape), scale and rho.  Returns ok; dx is written only then (it comes in as the
// previous step); tmp is DBL_MAX after a failed solve.  out = tmp, scale, rho.
int emu_pose_trial(const double* H, double lambda, const double* b, const double* qt, double cur, const float* K, const float* edges,
                   const uint8_t* state, int n, double* dx, double* qt_out, double* out) {
  poseopt::Pose P, Q;
  unpack(qt, P);
  const bool ok = poseopt::solve6(H, lambda, b, dx);
  poseopt::oplus(dx, P, Q);
  pack(Q, qt_out);
  const poseopt::Cam C = {(double)K[0], (double)K[1], (double)K[2], (double)K[3]};
  std::vector<double> chi2((size_t)n + 1);
  std::vector<uint8_t> st(state, state + n), m((size_t)n + 1);
  st.push_back(0);
  const poseopt::Edges E = {edges, chi2.data(), st.data(), m.data(), n};
  poseopt::HostTeam T;
  double tmp;
  T.sum<1>([&](int lane, double* acc) { poseopt::lane_robust_chi2(Q, C, E, lane, acc); }, &tmp);
  if (!ok) tmp = DBL_MAX;
  const double scale = poseopt::trial_scale<POSEOPT_MUT>(dx, lambda, b);
  out[0] = tmp, out[1] = scale, out[2] = (cur - tmp) / scale;
  return ok ? 1 : 0;
}

// layers 4 and 5: the call.  edges [n][6]; mask [n]; trace may be null.
void emu_pose_optimize(const float* edges, int n, const float* K, const float* Tcw, float* Tcw_out, int32_t* n_inliers, int32_t* rounds, uint8_t* mask,
                       uvo_pose_trace* trace) {
  std::vector<double> chi2((size_t)n + 1);
  std::vector<uint8_t> state((size_t)n + 1), m((size_t)n + 1);
  poseopt::Edges E = {edges, chi2.data(), state.data(), m.data(), n};
  const poseopt::Cam C = {(double)K[0], (double)K[1], (double)K[2], (double)K[3]};
  poseopt::HostTeam T;
  poseopt::Out out;
  if (trace) std::memset(trace, 0, sizeof *trace);
  poseopt::run<POSEOPT_MUT>(T, E, C, Tcw, &out, reinterpret_cast<poseopt::Trace*>(trace));
  std::memcpy(Tcw_out, out.Tcw, sizeof out.Tcw);
  *n_inliers = out.n_inliers, *rounds = out.rounds;
  if (mask && n > 0) std::memcpy(mask, m.data(), (size_t)n);
}

}  // extern "C"

#ifdef POSEOPT_EMU_MAIN
#include <cstdio>

namespace {
struct Lcg {
  uint64_t s;
  double next() {  // in [0, 1)
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(s >> 11) * (1. / 9007199254740992.);
  }
};

// n points in front of a camera near the origin, observed with a little noise; `shifted` of them moved by 6 px; the start pose a few
// centimetres and degrees off.  plane: the first point is put on the camera plane of the start pose.
int scene(uint64_t seed, int n, int shifted, bool plane) {
  Lcg g{seed * 2654435761ull + 12345};
  const float K[4] = {458.f, 457.f, 367.f, 248.f};
  std::vector<float> e((size_t)n * 6 + 6);
  for (int i = 0; i < n; ++i) {
    const double x = (g.next() - 0.5) * 6., y = (g.next() - 0.5) * 4., z = 2. + g.next() * 8.;
    float* r = &e[(size_t)i * 6];
    r[0] = (float)x, r[1] = (float)y, r[2] = (float)z;
    r[3] = (float)(K[0] * x / z + K[2] + (g.next() - 0.5)) + (i < shifted ? 6.f : 0.f);
    r[4] = (float)(K[1] * y / z + K[3] + (g.next() - 0.5)) + (i < shifted ? 6.f : 0.f);
    r[5] = i % 3 == 0 ? 1.f : i % 3 == 1 ? 0.694444f : 0.482253f;
  }
  float T[16] = {1.f, 0.f, 0.f, 0.03f, 0.f, 0.9998f, -0.02f, -0.02f, 0.f, 0.02f, 0.9998f, 0.05f, 0.f, 0.f, 0.f, 1.f};
  if (plane && n > 0) e[2] = (-T[11] - T[9] * e[1]) / T[10];
  float To[16];
  int32_t inl = -1, rounds = -1;
  std::vector<uint8_t> mask((size_t)n + 1);
  static uvo_pose_trace tr;
  emu_pose_optimize(e.data(), n, K, T, To, &inl, &rounds, mask.data(), &tr);
  std::printf("seed %llu n %d shifted %d plane %d: inliers %d rounds %d lin %d trials %d t = %g %g %g\n", (unsigned long long)seed, n, shifted, (int)plane,
              inl, rounds, tr.n_lin, tr.n_trials, To[3], To[7], To[11]);
  return inl < 0 || inl > n || rounds < 1 || rounds > 4 || tr.n_lin > 32 || tr.n_trials > 320;
}
// the committed scene list (tests/golden/poseopt_scenes.bin, written by tests/poseopt_model.py's dump): one line per scene
int scene_file(const char* path) {
  FILE* f = std::fopen(path, "rb");
  if (!f) return 1;
  int32_t count = 0;
  int bad = std::fread(&count, 4, 1, f) != 1 || count < 0 || count > 1000;
  for (int s = 0; s < count && !bad; ++s) {
    int32_t n = 0;
    float K[4], T[16], To[16];
    if (std::fread(&n, 4, 1, f) != 1 || n < 0 || n > 16384 || std::fread(K, 4, 4, f) != 4 || std::fread(T, 4, 16, f) != 16) {
      bad = 1;
      break;
    }
    std::vector<float> e((size_t)n * 6 + 6);
    if (n && std::fread(e.data(), 24, (size_t)n, f) != (size_t)n) {
      bad = 1;
      break;
    }
    int32_t inl = -1, rounds = -1;
    std::vector<uint8_t> mask((size_t)n + 1);
    static uvo_pose_trace tr;
    emu_pose_optimize(e.data(), n, K, T, To, &inl, &rounds, mask.data(), &tr);
    std::printf("scene %d n %d inliers %d rounds %d lin %d trials %d\n", s, n, inl, rounds, tr.n_lin, tr.n_trials);
    bad = inl < 0 || inl > n || rounds < 1 || rounds > 4 || tr.n_lin > 32 || tr.n_trials > 320;
  }
  std::fclose(f);
  return bad;
}
}  // namespace

int main(int argc, char** argv) {
  int bad = 0;
  if (argc > 1) bad += scene_file(argv[1]);
  const int sizes[] = {0, 1, 2, 3, 5, 9, 10, 11, 63, 64, 65, 255, 256, 257, 513, 2048, 2049, 5000};
  uint64_t seed = 1;
  for (int n : sizes) bad += scene(seed++, n, 0, false);
  for (int n : {30, 100, 300}) bad += scene(seed++, n, n / 3, false);
  bad += scene(seed++, 12, 12, false);
  bad += scene(seed++, 12, 5, false);
  bad += scene(seed++, 50, 0, true);
  std::printf("%s\n", bad ? "FAILED" : "ok");
  return bad ? 1 : 0;
}
#endif
