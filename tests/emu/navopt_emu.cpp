// Host build of the visual-inertial pose optimisation: csrc/navopt_core.hpp compiled by the host compiler with -ffp-contract=off, the
// same source k_nav_optimize runs, with navopt::HostTeam walking the reduction shape of 256 lanes and running each() in index order.
// tests/navopt_checks.py holds it to the numpy model (tests/navopt_model.py) layer by layer; tests/test_gpu_navopt.py holds the device
// to it bit for bit.
//
// Seeded mutations exist behind -DNAVOPT_MUT=k of THIS file only (the library has none), to show that the checks can fail:
// 1 the estimates not reset between rounds, 2 the break test counting active edges, 3 the kernel taken off the IMU edge too, 4 the depth
// edge's vertices swapped in the frame form, 5 the 1/2 added to the depth edge's gravity term, 6 the marginals taken from a fresh
// linearisation at the final estimate, 7 the block-diagonal and the joint marg_cov_inv exchanged, 8 the Hessian ordered bias first,
// 9 the Huber weight left off the reprojection edges' b, 10 the sign of JacobianRInv's hat term.
//
// With -DNAVOPT_EMU_MAIN the file is a stand-alone program that runs the committed scene list (the file named by its argument:
// tests/golden/navopt_scenes.bin) once: the form in which it is run under -fsanitize=address,undefined.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/uvo/uvo.h"
#include "../../u-vip-slam_amd/csrc/navopt_core.hpp"

#ifndef NAVOPT_MUT
#define NAVOPT_MUT 0
#endif

using namespace uvo;

static_assert(sizeof(uvo_nav_trace) == sizeof(navopt::Trace), "uvo_nav_trace is navopt::Trace");
static_assert(sizeof(uvo_nav_state) == sizeof(navopt::State), "uvo_nav_state is navopt::State");

namespace {
struct Scratch {
  std::vector<double> chi2;
  std::vector<uint8_t> state, mask;
  navopt::Edges E;
  Scratch(const navopt::Problem& p, const float* edges, const uint8_t* st) {
    const size_t n = (size_t)p.n + (size_t)(p.form == navopt::kFrame ? p.n_last : 0);
    chi2.assign(n + 1, 0.), state.assign(n + 1, 0), mask.assign(n + 1, 0);
    if (st) std::memcpy(state.data(), st, n);
    E = {edges, chi2.data(), state.data(), mask.data()};
  }
};
void prepare(const navopt::Problem& p, const navopt::State* est, navopt::Work& W) {
  navopt::HostTeam T;
  std::memset(&W, 0, sizeof W);
  W.est[0] = est[0], W.est[1] = est[1];
  double Rcb[9];
  navopt::mat3_t(p.Rbc, Rcb);
  navopt::mat3_vec(Rcb, p.Pbc, W.camc);
  navopt::ldl_inverse(T, [&](int i, int k) { return p.cov[i * 9 + k]; }, W.A, 9, navopt::kND, W.X, 9, 15);
  for (int t = 0; t < 81; ++t) W.oimu[t] = W.X[(t / 9) * 15 + t % 9];
}
}  // namespace

extern "C" {

int emu_nav_mutation() { return NAVOPT_MUT; }
int emu_nav_sizes(int what) { return what == 0 ? (int)sizeof(navopt::Problem) : what == 1 ? (int)sizeof(navopt::Out) : (int)sizeof(navopt::Trace); }

// so3.cpp: 0 exp (3 -> q), 1 log (q -> 3), 2 JacobianR (3 -> 9), 3 JacobianRInv (3 -> 9), 4 product (q, q -> q), 5 matrix (q -> 9)
void emu_nav_so3(int what, const double* in, double* out) {
  if (what == 0) navopt::so3_exp(in, out);
  else if (what == 1) navopt::so3_log(in, out);
  else if (what == 2) navopt::so3_jr(in, out);
  else if (what == 3) navopt::so3_jrinv<NAVOPT_MUT>(in, out);
  else if (what == 4) navopt::q_mul(in, in + 4, out);
  else poseopt::rotation_of(in, out);
}

// layer 1a: one reprojection edge (6 floats) at a state: out = e0 e1 chi2 rho0 rho1 J[2][6] over (dP, dPhi)
void emu_nav_reproj(const navopt::Problem* p, const navopt::State* s, const float* edge, int robust, double* out) {
  double cam[12], camc[3], Rcb[9];
  navopt::frame_camera(*s, p->Rbc, cam);
  navopt::mat3_t(p->Rbc, Rcb);
  navopt::mat3_vec(Rcb, p->Pbc, camc);
  navopt::ReprojEval ev;
  navopt::reproj_error(cam, camc, *p, edge, ev);
  out[0] = ev.e0, out[1] = ev.e1, out[2] = ev.chi2;
  navopt::robustify(ev.chi2, navopt::kDeltaMono, robust != 0, out + 3, out + 4);
  navopt::reproj_jacobian(ev, *p, out + 5, out + 11);
}

// layer 1b: the single edges at est[2]: e[31], J[31][30], sing[3][4] (chi2, rho0, rho1 of prior, IMU, bias, depth), oimu[81]
void emu_nav_single(const navopt::Problem* p, const navopt::State* est, double* e, double* J, double* sing, double* oimu) {
  static navopt::Work W;
  prepare(*p, est, W);
  for (int k = 0; k < 4; ++k) navopt::single_edge<NAVOPT_MUT>(*p, W, k, true);
  std::memcpy(e, W.e, sizeof W.e), std::memcpy(J, W.J, sizeof W.J), std::memcpy(sing, W.sing, sizeof W.sing), std::memcpy(oimu, W.oimu, sizeof W.oimu);
}

// layer 2: one linearisation at est[2] over the edges whose state byte has no level bit: H [30][30] (upper triangle), b[30]; returns chi2
double emu_nav_linearise(const navopt::Problem* p, const navopt::State* est, const float* edges, const uint8_t* state, int robust, double* H, double* b) {
  static navopt::Work W;
  prepare(*p, est, W);
  Scratch S(*p, edges, state);
  navopt::HostTeam T;
  const double chi = navopt::linearise<NAVOPT_MUT>(T, *p, S.E, W, robust != 0, p->form == navopt::kFrame ? 30 : 15);
  std::memcpy(H, W.H, sizeof W.H), std::memcpy(b, W.b, sizeof W.b);
  return chi;
}

// layer 3: one trial from given H (upper triangle, [30][30]), b, lambda, est[2]: dx comes in as the previous step and goes out as the
// step taken; est_out the tried estimates; out = tmp, scale.  Returns ok.
int emu_nav_trial(const navopt::Problem* p, const navopt::State* est, const float* edges, const uint8_t* state, int robust, const double* H, const double* b,
                  double lambda, double* dx, navopt::State* est_out, double* out) {
  static navopt::Work W;
  prepare(*p, est, W);
  std::memcpy(W.H, H, sizeof W.H), std::memcpy(W.b, b, sizeof W.b), std::memcpy(W.dx, dx, sizeof W.dx);
  Scratch S(*p, edges, state);
  navopt::HostTeam T;
  const bool ok = navopt::try_step<NAVOPT_MUT>(T, *p, S.E, W, robust != 0, p->form == navopt::kFrame ? 30 : 15, lambda, out, out + 1);
  std::memcpy(dx, W.dx, sizeof W.dx);
  est_out[0] = W.est[0], est_out[1] = W.est[1];
  return ok ? 1 : 0;
}

// layer 6: the marginals of a given H (upper triangle, [30][30]): marg_cov, marg_cov_inv of out.  Returns ok.
int emu_nav_marginals(const navopt::Problem* p, const double* H, navopt::Out* out) {
  static navopt::Work W;
  std::memset(&W, 0, sizeof W);
  std::memcpy(W.H, H, sizeof W.H);
  navopt::HostTeam T;
  return navopt::marginals<NAVOPT_MUT>(T, *p, W, p->form == navopt::kFrame ? 30 : 15, out) ? 1 : 0;
}

// layers 4 and 5: the call.  edges [n + n_last][6]; mask [n + n_last]; trace may be null.
void emu_nav_optimize(const navopt::Problem* p, const float* edges, navopt::Out* out, uint8_t* mask, uvo_nav_trace* trace) {
  static navopt::Work W;
  std::memset(&W, 0, sizeof W);
  Scratch S(*p, edges, nullptr);
  navopt::HostTeam T;
  if (trace) std::memset(trace, 0, sizeof *trace);
  std::memset(out, 0, sizeof *out);
  navopt::run<NAVOPT_MUT>(T, *p, S.E, W, out, reinterpret_cast<navopt::Trace*>(trace));
  const size_t n = (size_t)p->n + (size_t)(p->form == navopt::kFrame ? p->n_last : 0);
  if (mask && n > 0) std::memcpy(mask, S.mask.data(), n);
}

}  // extern "C"

#ifdef NAVOPT_EMU_MAIN
#include <cstdio>

// the committed scene list (tests/golden/navopt_scenes.bin, written by tests/navopt_model.py's dump): int32 count, int32 record size; per
// scene the problem record, then its edges
int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t head[2] = {0, 0};
  int bad = std::fread(head, 4, 2, f) != 2 || head[0] < 0 || head[0] > 1000 || head[1] != (int32_t)sizeof(navopt::Problem);
  for (int s = 0; s < head[0] && !bad; ++s) {
    static navopt::Problem p;
    if (std::fread(&p, sizeof p, 1, f) != 1 || p.n < 0 || p.n > 16384 || p.n_last < 0 || p.n_last > 16384 || (p.form != 0 && p.form != 1)) {
      bad = 1;
      break;
    }
    const size_t n = (size_t)p.n + (size_t)(p.form == navopt::kFrame ? p.n_last : 0);
    std::vector<float> e(n * 6 + 6);
    if (n && std::fread(e.data(), 24, n, f) != n) {
      bad = 1;
      break;
    }
    static navopt::Out out;
    static uvo_nav_trace tr;
    std::vector<uint8_t> mask(n + 1);
    emu_nav_optimize(&p, e.data(), &out, mask.data(), &tr);
    std::printf("scene %d form %d n %d + %d inliers %d rounds %d lin %d trials %d marg_ok %d P = %g %g %g\n", s, p.form, p.n, p.n_last, out.n_inliers, out.rounds,
                tr.n_lin, tr.n_trials, out.marg_ok, out.ns.P[0], out.ns.P[1], out.ns.P[2]);
    bad = out.n_inliers < 0 || out.n_inliers > p.n || out.rounds < 0 || out.rounds > 4 || tr.n_lin > 40 || tr.n_trials > 400;
  }
  std::fclose(f);
  std::printf("%s\n", bad ? "FAILED" : "ok");
  return bad ? 1 : 0;
}
#endif
