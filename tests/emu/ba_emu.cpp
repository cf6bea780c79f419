// Host build of the bundle adjustment: csrc/ba_core.hpp compiled by the host compiler with -ffp-contract=off, the same source the
// k_ba_* kernels run, with ba::HostTeam walking the reduction shape of 256 lanes and ba::drive choosing the phases as it does on the
// device.  tests/ba_checks.py holds it to the numpy model (tests/ba_model.py) layer by layer; tests/test_gpu_ba.py holds the device to
// it bit for bit.
//
// Nine seeded mutations exist behind -DBA_MUT=k of THIS file only (the library has none), to show that the checks can fail:
// 1 lambda added to Hpp but not Hll (the points see no lambda, neither in Dinv nor in their share of the scale), 2 Dinv from the
// unaugmented block (the scale keeps lambda), 3 a fixed key frame's W kept (it lands in a free key frame's rows of x_l), 4 the Schur term added
// instead of subtracted, 5 x_l without the W^T x_p term, 6 the stored error re-evaluated after a rejected trial, 7 removed edges
// returning in round 2, 8 a vertex without edges still stepped (by the step the last optimize() left), 9 tau taken over poses only.
//
// With -DBA_EMU_MAIN the file is a stand-alone program that runs the committed scene list (the file named by its argument:
// tests/golden/ba_scenes.bin) once: the form in which it is run under -fsanitize=address,undefined.
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/uvo/uvo.h"
#include "../../u-vip-slam_amd/csrc/ba_core.hpp"

#ifndef BA_MUT
#define BA_MUT 0
#endif

using namespace uvo;

static_assert(sizeof(uvo_ba_trace) == sizeof(ba::Trace), "uvo_ba_trace is ba::Trace");

namespace {

// the arrays of a call, owned
struct HostWs {
  ba::Ws W;
  ba::Ctl ctl;
  ba::Trace trace;
  std::vector<float> kf_T, pts, e_obs, cams, kf_T_out, pt_out;
  std::vector<int32_t> kf_free, free_kf, pt_begin, e_kf, e_pt, e_cam, kl_begin, kl_edge, fp_edge, chunk_n;
  std::vector<uint8_t> pt_bad, e_off, p_on, f_on, removed1, removed2;
  std::vector<ba::Pose> pose, pose_try;
  std::vector<double> X, X_try, e_chi2, e_lin, Hll, Dinv, Hpp, Hs, bs, xp, xl, chunk_chi2, chunk_scale, chunk_max, kf_est, pt_est;
  int F = 0;

  // 0, or 1: not well formed
  int load(const uvo_ba_problem& q) {
    const size_t K = (size_t)q.n_keyframes, P = (size_t)q.n_points, E = (size_t)q.n_edges;
    size_t nf = 0;
    for (size_t k = 0; k < K; ++k) nf += q.kf_fixed[k] ? 0 : 1;
    kf_free.assign(K + 1, 0), free_kf.assign(nf + 1, 0), e_pt.assign(E + 1, 0), kl_begin.assign(nf + 2, 0), kl_edge.assign(E + 1, 0), fp_edge.assign(nf * P + 1, -1);
    if (ba::derive((int)K, q.kf_fixed, (int)P, q.point_edge_begin, (int)E, q.edge_kf, q.edge_camera, q.n_cameras, kf_free.data(), free_kf.data(), &F, e_pt.data(),
                   kl_begin.data(), kl_edge.data(), fp_edge.data()))
      return 1;
    const size_t N = 6 * (size_t)F, ce = (size_t)ba::chunks((int)E), cp = (size_t)ba::chunks((int)P);
    kf_T.assign(q.kf_Tcw, q.kf_Tcw + 12 * K), pts.assign(q.points, q.points + 3 * P);
    pt_bad.assign(P + 1, 0);
    if (q.point_bad) std::memcpy(pt_bad.data(), q.point_bad, P);
    pt_begin.assign(q.point_edge_begin, q.point_edge_begin + P + 1);
    e_kf.assign(q.edge_kf, q.edge_kf + E), e_cam.assign(q.edge_camera, q.edge_camera + E), e_kf.push_back(0), e_cam.push_back(0);
    e_obs.assign(3 * E + 3, 0.f);
    for (size_t e = 0; e < E; ++e) e_obs[3 * e] = q.edge_obs[2 * e], e_obs[3 * e + 1] = q.edge_obs[2 * e + 1], e_obs[3 * e + 2] = q.edge_inv_sigma2[e];
    cams.assign(q.cameras, q.cameras + 4 * (size_t)q.n_cameras);
    pose.assign(K + 1, ba::Pose()), pose_try = pose;
    X.assign(3 * P + 3, 0.), X_try = X, xl = X, pt_est = X, pt_out.assign(3 * P + 3, 0.f);
    e_off.assign(E + 1, 0), removed1 = e_off, removed2 = e_off, e_chi2.assign(E + 1, 0.), e_lin.assign((E + 1) * ba::kEdgeWords, 0.);
    Hll.assign(9 * P + 9, 0.), Dinv = Hll, p_on.assign(P + 1, 0), Hpp.assign(27 * (size_t)F + 27, 0.), f_on.assign((size_t)F + 1, 0);
    Hs.assign(N * N + 1, 0.), bs.assign(N + 1, 0.), xp = bs;
    chunk_chi2.assign(ce + 1, 0.), chunk_scale.assign(cp + 1, 0.), chunk_max.assign(cp + (size_t)F + 1, 0.), chunk_n.assign(ce + 1, 0);
    kf_est.assign(7 * K + 7, 0.), kf_T_out.assign(16 * K + 16, 0.f);
    std::memset(&ctl, 0, sizeof ctl), std::memset(&trace, 0, sizeof trace);
    W.K = (int)K, W.F = F, W.P = (int)P, W.E = (int)E, W.C = q.n_cameras, W.pad_ = 0;
    W.kf_T = kf_T.data(), W.kf_free = kf_free.data(), W.free_kf = free_kf.data(), W.pts = pts.data(), W.pt_bad = pt_bad.data(), W.pt_begin = pt_begin.data();
    W.e_kf = e_kf.data(), W.e_pt = e_pt.data(), W.e_cam = e_cam.data(), W.e_obs = e_obs.data(), W.cams = cams.data();
    W.kl_begin = kl_begin.data(), W.kl_edge = kl_edge.data(), W.fp_edge = fp_edge.data();
    W.pose = pose.data(), W.pose_try = pose_try.data(), W.X = X.data(), W.X_try = X_try.data(), W.e_off = e_off.data(), W.e_chi2 = e_chi2.data(), W.e_lin = e_lin.data();
    W.Hll = Hll.data(), W.Dinv = Dinv.data(), W.p_on = p_on.data(), W.Hpp = Hpp.data(), W.f_on = f_on.data(), W.Hs = Hs.data(), W.bs = bs.data(), W.xp = xp.data();
    W.xl = xl.data(), W.chunk_chi2 = chunk_chi2.data(), W.chunk_scale = chunk_scale.data(), W.chunk_max = chunk_max.data(), W.chunk_n = chunk_n.data();
    W.ctl = &ctl, W.trace = &trace, W.removed1 = removed1.data(), W.removed2 = removed2.data();
    W.kf_est = kf_est.data(), W.kf_T_out = kf_T_out.data(), W.pt_est = pt_est.data(), W.pt_out = pt_out.data();
    return 0;
  }
};

struct HostExec {
  HostWs* h;
  ba::HostTeam T;
  int launch(int ph, int blocks) {
    for (int b = 0; b < blocks; ++b) ba::run_phase<BA_MUT>(ph, h->W, T, b);
    return 0;
  }
  int status(int* out) {
    *out = h->ctl.status;
    return 0;
  }
};

void store(const HostWs& h, const uvo_ba_problem& q, uvo_ba_result& r, int syncs) {
  const size_t K = (size_t)q.n_keyframes, P = (size_t)q.n_points, E = (size_t)q.n_edges;
  if (r.kf_estimate) std::memcpy(r.kf_estimate, h.kf_est.data(), sizeof(double) * 7 * K);
  if (r.kf_Tcw) std::memcpy(r.kf_Tcw, h.kf_T_out.data(), sizeof(float) * 16 * K);
  if (r.point_estimate) std::memcpy(r.point_estimate, h.pt_est.data(), sizeof(double) * 3 * P);
  if (r.points) std::memcpy(r.points, h.pt_out.data(), sizeof(float) * 3 * P);
  if (r.removed1) std::memcpy(r.removed1, h.removed1.data(), E);
  if (r.removed2) std::memcpy(r.removed2, h.removed2.data(), E);
  int n1 = 0, n2 = 0;
  for (size_t e = 0; e < E; ++e) n1 += h.removed1[e], n2 += h.removed2[e];
  r.n_removed1 = n1, r.n_removed2 = n2, r.iterations[0] = h.ctl.its[0], r.iterations[1] = h.ctl.its[1], r.n_trials = h.ctl.n_trials, r.n_syncs = syncs + 1;
}

}  // namespace

extern "C" {

int emu_ba_mutation() { return BA_MUT; }

// the call, as uvo_bundle_adjust answers it (a problem without a free key frame or an edge is the library's host side, not here).
// Returns 0, or 1 when the lists are not well formed.
int emu_ba_adjust(const uvo_ba_problem* q, uvo_ba_result* r, uvo_ba_trace* trace) {
  static HostWs h;
  if (h.load(*q) || h.F == 0 || q->n_edges == 0) return 1;
  HostExec x = {&h, {}};
  int syncs = 0;
  const ba::Dims d = {q->n_keyframes, h.F, q->n_points, q->n_edges};
  ba::drive(x, d, q->mode == UVO_BA_LOCAL ? ba::kModeLocal : ba::kModeFull, q->n_iterations, &syncs);
  store(h, *q, *r, syncs);
  if (trace) std::memcpy(trace, &h.trace, sizeof h.trace);
  return 0;
}

// One linearisation and one trial at GIVEN estimates: est [K][7] (q x y z w, t), X [P][3], off [E] (1: the edge is removed), lambda.
// Out: chi2 [E], lin [E][22] (Jp 2 x 6, Jl 2 x 3, rho1 w, the two weighted residuals, rho0), Hll [P][9], Hpp [F][27], Dinv [P][9],
// Hs [6F][6F] (lower triangle as assembled, before the factorisation), bs [6F], xp [6F], xl [P][3], est_try [K][7], X_try [P][3],
// chi2_try [E], scal = chi2 at the linearisation, the largest diagonal entry, ok, tmp, scale.  Returns 0, or 1: not well formed.
int emu_ba_one_trial(const uvo_ba_problem* q, const double* est, const double* X, const uint8_t* off, double lambda, double* chi2, double* lin, double* Hll,
                     double* Hpp, double* Dinv, double* Hs, double* bs, double* xp, double* xl, double* est_try, double* X_try, double* chi2_try, double* scal) {
  static HostWs h;
  if (h.load(*q) || h.F == 0) return 1;
  const size_t K = (size_t)q->n_keyframes, P = (size_t)q->n_points, E = (size_t)q->n_edges, N = 6 * (size_t)h.F;
  HostExec x = {&h, {}};
  x.launch(ba::kInit, ba::chunks((int)(K > P ? (K > E ? K : E) : (P > E ? P : E))));
  x.launch(ba::kBegin, 1);
  for (size_t k = 0; k < K; ++k) {
    std::memcpy(h.pose[k].q, est + 7 * k, sizeof(double) * 4), std::memcpy(h.pose[k].t, est + 7 * k + 4, sizeof(double) * 3);
  }
  std::memcpy(h.X.data(), X, sizeof(double) * 3 * P);
  if (off) std::memcpy(h.e_off.data(), off, E);
  x.launch(ba::kEdgeLin, ba::chunks((int)E)), x.launch(ba::kPointSum, ba::chunks((int)P)), x.launch(ba::kKfSum, h.F), x.launch(ba::kLinCtl, 1);
  std::memcpy(chi2, h.e_chi2.data(), sizeof(double) * E), std::memcpy(lin, h.e_lin.data(), sizeof(double) * E * ba::kEdgeWords);
  std::memcpy(Hll, h.Hll.data(), sizeof(double) * 9 * P), std::memcpy(Hpp, h.Hpp.data(), sizeof(double) * 27 * (size_t)h.F);
  scal[0] = h.ctl.cur, scal[1] = h.ctl.lambda / 1e-5;
  scal[1] = h.trace.lin[0].maxdiag;
  h.ctl.lambda = lambda;
  x.launch(ba::kDinv, ba::chunks((int)P)), x.launch(ba::kSchur, ba::schur_blocks(h.F));
  std::memcpy(Dinv, h.Dinv.data(), sizeof(double) * 9 * P), std::memcpy(Hs, h.Hs.data(), sizeof(double) * N * N), std::memcpy(bs, h.bs.data(), sizeof(double) * N);
  x.launch(ba::kSolve, 1), x.launch(ba::kStep, ba::chunks((int)P)), x.launch(ba::kEdgeErr, ba::chunks((int)E));
  const int ok = h.ctl.solve_ok;
  x.launch(ba::kTrialCtl, 1);
  std::memcpy(xp, h.xp.data(), sizeof(double) * N), std::memcpy(xl, h.xl.data(), sizeof(double) * 3 * P);
  for (size_t k = 0; k < K; ++k) {
    std::memcpy(est_try + 7 * k, h.pose_try[k].q, sizeof(double) * 4), std::memcpy(est_try + 7 * k + 4, h.pose_try[k].t, sizeof(double) * 3);
  }
  std::memcpy(X_try, h.X_try.data(), sizeof(double) * 3 * P), std::memcpy(chi2_try, h.e_chi2.data(), sizeof(double) * E);
  scal[2] = (double)ok, scal[3] = h.trace.trial[0].tmp, scal[4] = h.trace.trial[0].scale;
  return 0;
}

}  // extern "C"

#ifdef BA_EMU_MAIN
#include <cstdio>

// the committed scene list (tests/golden/ba_scenes.bin, written by tests/ba_model.py's dump): int32 count; per scene int32 mode,
// n_iterations, K, P, E, C; float Tcw [K][12]; uint8 fixed [K]; float points [P][3]; uint8 bad [P]; int32 begin [P + 1]; int32 kf [E];
// float obs [E][2]; float inv_sigma2 [E]; int32 camera [E]; float cameras [C][4]
int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t count = 0;
  int bad = std::fread(&count, 4, 1, f) != 1 || count < 0 || count > 1000;
  for (int s = 0; s < count && !bad; ++s) {
    int32_t h[6];
    if (std::fread(h, 4, 6, f) != 6 || h[2] < 0 || h[2] > 320 || h[3] < 0 || h[3] > ba::kMaxPoints || h[4] < 0 || h[4] > ba::kMaxEdges || h[5] < 1 || h[5] > ba::kMaxCams) {
      bad = 1;
      break;
    }
    const size_t K = (size_t)h[2], P = (size_t)h[3], E = (size_t)h[4], C = (size_t)h[5];
    std::vector<float> T(12 * K + 1), pts(3 * P + 1), obs(2 * E + 1), w(E + 1), cams(4 * C);
    std::vector<uint8_t> fixed(K + 1), pbad(P + 1);
    std::vector<int32_t> begin(P + 1), kf(E + 1), cam(E + 1);
    bad = std::fread(T.data(), 48, K, f) != K || std::fread(fixed.data(), 1, K, f) != K || std::fread(pts.data(), 12, P, f) != P || std::fread(pbad.data(), 1, P, f) != P ||
          std::fread(begin.data(), 4, P + 1, f) != P + 1 || std::fread(kf.data(), 4, E, f) != E || std::fread(obs.data(), 8, E, f) != E ||
          std::fread(w.data(), 4, E, f) != E || std::fread(cam.data(), 4, E, f) != E || std::fread(cams.data(), 16, C, f) != C;
    if (bad) break;
    const uvo_ba_problem q = {h[0], h[1], h[2], h[3], h[4], h[5], T.data(), fixed.data(), pts.data(), pbad.data(), begin.data(), kf.data(), obs.data(), w.data(), cam.data(), cams.data()};
    std::vector<double> est(7 * K + 1), pe(3 * P + 1);
    std::vector<float> To(16 * K + 1), po(3 * P + 1);
    std::vector<uint8_t> r1(E + 1), r2(E + 1);
    uvo_ba_result r = {est.data(), To.data(), pe.data(), po.data(), r1.data(), r2.data(), -1, -1, {-1, -1}, -1, -1};
    static uvo_ba_trace tr;
    const int rc = emu_ba_adjust(&q, &r, &tr);
    std::printf("scene %d: K %d P %d E %d rc %d removed %d %d iterations %d %d trials %d\n", s, h[2], h[3], h[4], rc, r.n_removed1, r.n_removed2, r.iterations[0], r.iterations[1], r.n_trials);
    bad = rc != 0 || r.n_removed1 < 0 || r.n_removed1 + r.n_removed2 > h[4] || r.iterations[0] < 0 || r.iterations[0] > 32 || r.iterations[1] > 10 || r.n_trials > 320 ||
          tr.n_trials != r.n_trials;
  }
  std::fclose(f);
  std::printf("%s\n", bad ? "FAILED" : "ok");
  return bad ? 1 : 0;
}
#endif
