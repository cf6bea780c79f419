// Host build of the visual-inertial bundle adjustment: csrc/navba_core.hpp compiled by the host compiler with -ffp-contract=off, the
// same source the k_navba_* kernels run, with navba::HostTeam walking the reduction shape of 256 lanes and navba::drive choosing the
// phases as it does on the device.  tests/navba_checks.py holds it to the numpy model (tests/navba_model.py) layer by layer;
// tests/test_gpu_navba.py holds the device to it bit for bit.
//
// Ten seeded mutations exist behind -DNAVBA_MUT=k of THIS file only (the library has none), to show that the checks can fail:
// 1 the V columns of the mono Jacobian not zero (a copy of the P columns, in the diagonal blocks), 2 the Schur block scattered to
// columns 0..5 instead of {0,1,2,6,7,8}, 3 the backward depth edge reading pKF0's preintegration (every depth entry reads the link that
// ends in its first vertex), 4 the first check's comparison in float, 5 the kernel kept on checked edges in round two, 6 the kernel
// taken off flagged points, 7 the final check skipping excluded edges, 8 PVR and bias columns swapped, 9 the bias edge's information
// not divided by dT, 10 tau over the poses only.
//
// With -DNAVBA_EMU_MAIN the file is a stand-alone program that runs the committed scene list (the file named by its argument:
// tests/golden/navba_scenes.bin) once: the form in which it is run under -fsanitize=address,undefined.
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/uvo/uvo.h"
#include "../../u-vip-slam_amd/csrc/navba_core.hpp"

#ifndef NAVBA_MUT
#define NAVBA_MUT 0
#endif

using namespace uvo;

static_assert(sizeof(uvo_nav_ba_trace) == sizeof(navba::Trace), "uvo_nav_ba_trace is navba::Trace");
static_assert(sizeof(uvo_nav_state) == sizeof(navopt::State) && sizeof(uvo_nav_ba_link) == sizeof(navba::Link) && sizeof(uvo_nav_ba_depth) == sizeof(navba::Depth),
              "the C ABI's records are the core's");

namespace {

struct HostWs {
  navba::Ws W;
  navba::Ctl ctl;
  navba::Trace trace;
  navba::Params prm;
  std::vector<navopt::State> kf_in, ns, ns_try, kf_out;
  std::vector<navba::Link> links;
  std::vector<navba::Depth> depths;
  std::vector<float> pts, e_obs, cams, kf_T_out, pt_out;
  std::vector<int32_t> kf_free, free_kf, pt_begin, e_kf, e_pt, e_cam, kl_begin, kl_edge, fp_edge, chunk_n, ie_col;
  std::vector<uint8_t> kf_bias, pt_bad, e_off, e_rob, p_on, excluded, erased;
  std::vector<double> cam, cam_try, camc, X, X_try, e_chi2, e_lin, Hll, Dinv, Hpp, hdiag, link_info, ie_lin, ie_try, ie_etry, Hs, bs, bfull, xp, xl, chunk_chi2,
      chunk_scale, chunk_max, pt_est;
  int F = 0;

  // 0, or 1: not well formed, or beyond the library's limits
  int load(const uvo_nav_ba_problem& q) {
    const size_t K = (size_t)q.n_keyframes, P = (size_t)q.n_points, E = (size_t)q.n_edges, L = (size_t)q.n_links, D = (size_t)q.n_depth;
    if (q.n_keyframes < 0 || q.n_keyframes > navba::kMaxFree + navba::kMaxFixed || q.n_links < 0 || q.n_links > navba::kMaxLinks || q.n_depth < 0 ||
        q.n_depth > navba::kMaxDepth)
      return 1;
    size_t nf = 0;
    for (size_t k = 0; k < K; ++k) nf += q.kf_fixed[k] ? 0 : 1;
    if (nf > (size_t)navba::kMaxFree) return 1;
    kf_free.assign(K + 1, 0), free_kf.assign(nf + 1, 0), e_pt.assign(E + 1, 0), kl_begin.assign(nf + 2, 0), kl_edge.assign(E + 1, 0), fp_edge.assign(nf * P + 1, -1);
    if (ba::derive((int)K, q.kf_fixed, (int)P, q.point_edge_begin, (int)E, q.edge_kf, q.edge_camera, q.n_cameras, kf_free.data(), free_kf.data(), &F, e_pt.data(),
                   kl_begin.data(), kl_edge.data(), fp_edge.data()))
      return 1;
    links.assign(L + 1, navba::Link()), depths.assign(D + 1, navba::Depth());
    if (L) std::memcpy(links.data(), q.links, sizeof(navba::Link) * L);
    if (D) std::memcpy(depths.data(), q.depth, sizeof(navba::Depth) * D);
    if (navba::check_inertial((int)K, q.kf_fixed, q.kf_has_bias, (int)L, links.data(), (int)D, depths.data())) return 1;
    if (NAVBA_MUT == navba::kMutBackPre)
      for (size_t d = 0; d < D; ++d)
        for (size_t l = 0; l < L; ++l)
          if (links[l].kf1 == depths[d].ka) depths[d].link = (int32_t)l;
    const size_t N = 15 * (size_t)F, G = 2 * L + D, ce = (size_t)navba::chunks((int)E), cp = (size_t)navba::chunks((int)P);
    kf_in.assign(K + 1, navopt::State());
    if (K) std::memcpy(kf_in.data(), q.kf_state, sizeof(navopt::State) * K);
    ns = kf_in, ns_try = kf_in, kf_out = kf_in;
    kf_bias.assign(q.kf_has_bias, q.kf_has_bias + K), kf_bias.push_back(0);
    std::memcpy(prm.Rbc, q.Rbc, sizeof prm.Rbc), std::memcpy(prm.Pbc, q.Pbc, sizeof prm.Pbc), std::memcpy(prm.gw, q.gw, sizeof prm.gw);
    prm.gyr_rw2 = q.gyr_bias_rw2, prm.acc_rw2 = q.acc_bias_rw2;
    pts.assign(q.points, q.points + 3 * P), pts.push_back(0.f);
    pt_bad.assign(P + 1, 0);
    if (q.point_bad) std::memcpy(pt_bad.data(), q.point_bad, P);
    pt_begin.assign(q.point_edge_begin, q.point_edge_begin + P + 1);
    e_kf.assign(q.edge_kf, q.edge_kf + E), e_cam.assign(q.edge_camera, q.edge_camera + E), e_kf.push_back(0), e_cam.push_back(0);
    e_obs.assign(3 * E + 3, 0.f);
    for (size_t e = 0; e < E; ++e) e_obs[3 * e] = q.edge_obs[2 * e], e_obs[3 * e + 1] = q.edge_obs[2 * e + 1], e_obs[3 * e + 2] = q.edge_inv_sigma2[e];
    cams.assign(q.cameras, q.cameras + 4 * (size_t)q.n_cameras), cams.push_back(0.f);
    cam.assign(12 * K + 12, 0.), cam_try = cam, camc.assign(3, 0.);
    X.assign(3 * P + 3, 0.), X_try = X, xl = X, pt_est = X, pt_out.assign(3 * P + 3, 0.f);
    e_off.assign(E + 1, 0), e_rob = e_off, excluded = e_off, erased = e_off, e_chi2.assign(E + 1, 0.), e_lin.assign((E + 1) * navba::kEdgeWords, 0.);
    Hll.assign(9 * P + 9, 0.), Dinv = Hll, p_on.assign(P + 1, 0), Hpp.assign(27 * (size_t)F + 27, 0.), hdiag.assign(N + 1, 0.);
    link_info.assign(81 * L + 81, 0.), ie_lin.assign((G + 1) * navba::kIeWords, 0.), ie_col.assign(4 * G + 4, -1), ie_try.assign(G + 1, 0.), ie_etry.assign(9 * G + 9, 0.);
    Hs.assign(N * N + 1, 0.), bs.assign(N + 1, 0.), bfull = bs, xp = bs;
    chunk_chi2.assign(ce + 1, 0.), chunk_scale.assign(cp + 1, 0.), chunk_max.assign(cp + (size_t)F + 1, 0.), chunk_n.assign(ce + 1, 0);
    kf_T_out.assign(16 * K + 16, 0.f);
    std::memset(&ctl, 0, sizeof ctl), std::memset(&trace, 0, sizeof trace);
    W.K = (int)K, W.F = F, W.P = (int)P, W.E = (int)E, W.C = q.n_cameras, W.L = (int)L, W.D = (int)D, W.pad_ = 0;
    W.kf_in = kf_in.data(), W.kf_free = kf_free.data(), W.kf_bias = kf_bias.data(), W.free_kf = free_kf.data(), W.pts = pts.data(), W.pt_bad = pt_bad.data();
    W.pt_begin = pt_begin.data(), W.e_kf = e_kf.data(), W.e_pt = e_pt.data(), W.e_cam = e_cam.data(), W.e_obs = e_obs.data(), W.cams = cams.data();
    W.kl_begin = kl_begin.data(), W.kl_edge = kl_edge.data(), W.fp_edge = fp_edge.data(), W.links = links.data(), W.depths = depths.data(), W.prm = &prm;
    W.ns = ns.data(), W.ns_try = ns_try.data(), W.cam = cam.data(), W.cam_try = cam_try.data(), W.camc = camc.data(), W.X = X.data(), W.X_try = X_try.data();
    W.e_off = e_off.data(), W.e_rob = e_rob.data(), W.e_chi2 = e_chi2.data(), W.e_lin = e_lin.data(), W.Hll = Hll.data(), W.Dinv = Dinv.data(), W.p_on = p_on.data();
    W.Hpp = Hpp.data(), W.hdiag = hdiag.data(), W.link_info = link_info.data(), W.ie_lin = ie_lin.data(), W.ie_col = ie_col.data(), W.ie_try = ie_try.data();
    W.ie_etry = ie_etry.data(), W.Hs = Hs.data(), W.bs = bs.data(), W.bfull = bfull.data(), W.xp = xp.data(), W.xl = xl.data();
    W.chunk_chi2 = chunk_chi2.data(), W.chunk_scale = chunk_scale.data(), W.chunk_max = chunk_max.data(), W.chunk_n = chunk_n.data();
    W.ctl = &ctl, W.trace = &trace, W.excluded = excluded.data(), W.erased = erased.data();
    W.kf_out = kf_out.data(), W.kf_T_out = kf_T_out.data(), W.pt_est = pt_est.data(), W.pt_out = pt_out.data();
    return 0;
  }
  navba::Dims dims() const { return {W.K, W.F, W.P, W.E, W.L, W.D}; }
};

struct HostExec {
  HostWs* h;
  navba::HostTeam T;
  int launch(int ph, int blocks) {
    for (int b = 0; b < blocks; ++b) navba::run_phase<NAVBA_MUT>(ph, h->W, T, b);
    return 0;
  }
  int status(int* out) {
    *out = h->ctl.status;
    return 0;
  }
};

void store(const HostWs& h, const uvo_nav_ba_problem& q, uvo_nav_ba_result& r, int syncs) {
  const size_t K = (size_t)q.n_keyframes, P = (size_t)q.n_points, E = (size_t)q.n_edges;
  if (r.kf_state) std::memcpy(r.kf_state, h.kf_out.data(), sizeof(navopt::State) * K);
  if (r.kf_Tcw) std::memcpy(r.kf_Tcw, h.kf_T_out.data(), sizeof(float) * 16 * K);
  if (r.point_estimate) std::memcpy(r.point_estimate, h.pt_est.data(), sizeof(double) * 3 * P);
  if (r.points) std::memcpy(r.points, h.pt_out.data(), sizeof(float) * 3 * P);
  if (r.excluded) std::memcpy(r.excluded, h.excluded.data(), E);
  if (r.erased) std::memcpy(r.erased, h.erased.data(), E);
  int n1 = 0, n2 = 0;
  for (size_t e = 0; e < E; ++e) n1 += h.excluded[e], n2 += h.erased[e];
  r.n_excluded = n1, r.n_erased = n2, r.iterations[0] = h.ctl.its[0], r.iterations[1] = h.ctl.its[1], r.n_trials = h.ctl.n_trials, r.n_syncs = syncs + 1;
}

}  // namespace

extern "C" {

int emu_navba_mutation() { return NAVBA_MUT; }

// the call, as uvo_nav_bundle_adjust answers it (a problem without a free key frame is the library's host side, not here).
// Returns 0, or 1 when the lists are not well formed.
int emu_navba_adjust(const uvo_nav_ba_problem* q, uvo_nav_ba_result* r, uvo_nav_ba_trace* trace) {
  static HostWs h;
  if (h.load(*q) || h.F == 0) return 1;
  HostExec x = {&h, {}};
  int syncs = 0;
  const navba::Dims d = h.dims();
  navba::drive(x, d, &syncs);
  store(h, *q, *r, syncs);
  if (trace) std::memcpy(trace, &h.trace, sizeof h.trace);
  return 0;
}

// One linearisation and one trial at GIVEN estimates: est [K] states, X [P][3], off [E] (1: at level 1), rob [E] (1: kernel on), lambda.
// Out: chi2 [E], lin [E][22] (Jp 2 x 6 over dP dPhi, Jl 2 x 3, rho1 w, the two weighted residuals, rho0), ie [2L + D][kIeWords] (J 9 x 30,
// WJ, e, We, chi2 rho0 rho1), Hll [P][9], Hpp [F][27], Hs [15F][15F] (lower triangle as assembled, before the factorisation), bs, bfull,
// xp [15F], xl [P][3], est_try [K], X_try [P][3], chi2_try [E], scal = chi2 at the linearisation, the largest diagonal entry, ok, tmp,
// scale.  Returns 0, or 1: not well formed.
int emu_navba_one_trial(const uvo_nav_ba_problem* q, const uvo_nav_state* est, const double* X, const uint8_t* off, const uint8_t* rob, double lambda, double* chi2,
                        double* lin, double* ie, double* Hll, double* Hpp, double* Hs, double* bs, double* bfull, double* xp, double* xl, uvo_nav_state* est_try,
                        double* X_try, double* chi2_try, double* scal) {
  static HostWs h;
  if (h.load(*q) || h.F == 0) return 1;
  const size_t K = (size_t)q->n_keyframes, P = (size_t)q->n_points, E = (size_t)q->n_edges, N = 15 * (size_t)h.F, G = 2 * (size_t)q->n_links + (size_t)q->n_depth;
  HostExec x = {&h, {}};
  const navba::Dims d = h.dims();
  const int ce = navba::chunks(d.E), cp = navba::chunks(d.P), cg = navba::chunks((int)G), sb = navba::schur_blocks(d.F);
  x.launch(navba::kInit, navba::imax(navba::chunks(navba::imax(navba::imax(d.K, d.P), navba::imax(d.E, (int)G))), d.L));
  x.launch(navba::kBegin, 1);
  for (size_t k = 0; k < K; ++k) {
    std::memcpy(&h.ns[k], est + k, sizeof(navopt::State));
    navopt::frame_camera(h.ns[k], h.prm.Rbc, h.cam.data() + 12 * k);
  }
  std::memcpy(h.X.data(), X, sizeof(double) * 3 * P);
  if (off) std::memcpy(h.e_off.data(), off, E);
  if (rob) std::memcpy(h.e_rob.data(), rob, E);
  x.launch(navba::kEdgeLin, ce), x.launch(navba::kInertLin, cg), x.launch(navba::kPointSum, cp), x.launch(navba::kKfSum, d.F), x.launch(navba::kLinCtl, 1);
  std::memcpy(chi2, h.e_chi2.data(), sizeof(double) * E), std::memcpy(lin, h.e_lin.data(), sizeof(double) * E * navba::kEdgeWords);
  std::memcpy(ie, h.ie_lin.data(), sizeof(double) * G * navba::kIeWords);
  std::memcpy(Hll, h.Hll.data(), sizeof(double) * 9 * P), std::memcpy(Hpp, h.Hpp.data(), sizeof(double) * 27 * (size_t)h.F);
  scal[0] = h.ctl.cur, scal[1] = h.trace.lin[0].maxdiag;
  h.ctl.lambda = lambda;
  x.launch(navba::kDinv, cp), x.launch(navba::kSchur, sb), x.launch(navba::kInertAdd, sb);
  std::memcpy(Hs, h.Hs.data(), sizeof(double) * N * N), std::memcpy(bs, h.bs.data(), sizeof(double) * N), std::memcpy(bfull, h.bfull.data(), sizeof(double) * N);
  x.launch(navba::kSolve, 1), x.launch(navba::kStep, cp), x.launch(navba::kEdgeErr, ce), x.launch(navba::kInertErr, cg);
  const int ok = h.ctl.solve_ok;
  x.launch(navba::kTrialCtl, 1);
  std::memcpy(xp, h.xp.data(), sizeof(double) * N), std::memcpy(xl, h.xl.data(), sizeof(double) * 3 * P);
  std::memcpy(est_try, h.ns_try.data(), sizeof(navopt::State) * K);
  std::memcpy(X_try, h.X_try.data(), sizeof(double) * 3 * P), std::memcpy(chi2_try, h.e_chi2.data(), sizeof(double) * E);
  scal[2] = (double)ok, scal[3] = h.trace.trial[0].tmp, scal[4] = h.trace.trial[0].scale;
  return 0;
}

}  // extern "C"

#ifdef NAVBA_EMU_MAIN
#include <cstdio>

// the committed scene list (tests/golden/navba_scenes.bin, written by tests/navba_model.py's dump): int32 count; per scene int32 K, P, E,
// C, L, D; double states [K][22]; uint8 fixed [K]; uint8 has_bias [K]; float points [P][3]; uint8 bad [P]; int32 begin [P + 1]; int32 kf
// [E]; float obs [E][2]; float inv_sigma2 [E]; int32 camera [E]; float cameras [C][4]; double Rbc [9], Pbc [3], gw [3], gyr_rw2, acc_rw2;
// per link int32 kf0, kf1 and 142 doubles; per depth entry int32 ka, kb, kc, link and 3 doubles; int32 expected n_excluded, n_erased,
// iterations [2] of the model
int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t count = 0;
  int bad = std::fread(&count, 4, 1, f) != 1 || count < 0 || count > 1000;
  for (int s = 0; s < count && !bad; ++s) {
    int32_t h[6];
    if (std::fread(h, 4, 6, f) != 6 || h[0] < 0 || h[0] > navba::kMaxFree + navba::kMaxFixed || h[1] < 0 || h[1] > navba::kMaxPoints || h[2] < 0 || h[2] > navba::kMaxEdges ||
        h[3] < 1 || h[3] > navba::kMaxCams || h[4] < 0 || h[4] > navba::kMaxLinks || h[5] < 0 || h[5] > navba::kMaxDepth) {
      bad = 1;
      break;
    }
    const size_t K = (size_t)h[0], P = (size_t)h[1], E = (size_t)h[2], C = (size_t)h[3], L = (size_t)h[4], D = (size_t)h[5];
    std::vector<uvo_nav_state> st(K + 1), so(K + 1);
    std::vector<float> pts(3 * P + 1), obs(2 * E + 1), w(E + 1), cams(4 * C);
    std::vector<uint8_t> fixed(K + 1), hb(K + 1), pbad(P + 1);
    std::vector<int32_t> begin(P + 1), kf(E + 1), cam(E + 1);
    std::vector<uvo_nav_ba_link> links(L + 1);
    std::vector<uvo_nav_ba_depth> depth(D + 1);
    double prm[17];
    int32_t expect[4];
    bad = std::fread(st.data(), sizeof(uvo_nav_state), K, f) != K || std::fread(fixed.data(), 1, K, f) != K || std::fread(hb.data(), 1, K, f) != K ||
          std::fread(pts.data(), 12, P, f) != P || std::fread(pbad.data(), 1, P, f) != P || std::fread(begin.data(), 4, P + 1, f) != P + 1 ||
          std::fread(kf.data(), 4, E, f) != E || std::fread(obs.data(), 8, E, f) != E || std::fread(w.data(), 4, E, f) != E || std::fread(cam.data(), 4, E, f) != E ||
          std::fread(cams.data(), 16, C, f) != C || std::fread(prm, 8, 17, f) != 17 || std::fread(links.data(), sizeof(uvo_nav_ba_link), L, f) != L ||
          std::fread(depth.data(), sizeof(uvo_nav_ba_depth), D, f) != D || std::fread(expect, 4, 4, f) != 4;
    if (bad) break;
    uvo_nav_ba_problem q;
    std::memset(&q, 0, sizeof q);
    q.n_keyframes = h[0], q.n_points = h[1], q.n_edges = h[2], q.n_cameras = h[3], q.n_links = h[4], q.n_depth = h[5];
    q.kf_state = st.data(), q.kf_fixed = fixed.data(), q.kf_has_bias = hb.data(), q.points = pts.data(), q.point_bad = pbad.data(), q.point_edge_begin = begin.data();
    q.edge_kf = kf.data(), q.edge_obs = obs.data(), q.edge_inv_sigma2 = w.data(), q.edge_camera = cam.data(), q.cameras = cams.data();
    std::memcpy(q.Rbc, prm, 72), std::memcpy(q.Pbc, prm + 9, 24), std::memcpy(q.gw, prm + 12, 24), q.gyr_bias_rw2 = prm[15], q.acc_bias_rw2 = prm[16];
    q.links = links.data(), q.depth = depth.data();
    std::vector<double> pe(3 * P + 1);
    std::vector<float> To(16 * K + 1), po(3 * P + 1);
    std::vector<uint8_t> r1(E + 1), r2(E + 1);
    uvo_nav_ba_result r = {so.data(), To.data(), pe.data(), po.data(), r1.data(), r2.data(), -1, -1, {-1, -1}, -1, -1};
    static uvo_nav_ba_trace tr;
    const int rc = emu_navba_adjust(&q, &r, &tr);
    std::printf("scene %d: K %d P %d E %d L %d D %d rc %d excluded %d (%d) erased %d (%d) iterations %d %d (%d %d) trials %d\n", s, h[0], h[1], h[2], h[4], h[5], rc,
                r.n_excluded, expect[0], r.n_erased, expect[1], r.iterations[0], r.iterations[1], expect[2], expect[3], r.n_trials);
    bad = rc != 0 || r.n_excluded != expect[0] || r.n_erased != expect[1] || r.iterations[0] != expect[2] || r.iterations[1] != expect[3] || r.n_trials > 320 ||
          tr.n_trials != r.n_trials;
  }
  std::fclose(f);
  std::printf("%s\n", bad ? "FAILED" : "ok");
  return bad ? 1 : 0;
}
#endif
