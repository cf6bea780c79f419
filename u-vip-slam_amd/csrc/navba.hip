// Optimizer::LocalBundleAdjustmentNavState (src/Optimizer.cc:1105-1732) as one call.  All arithmetic, the phases and their launch
// sequence are navba_core.hpp, shared with the host build tests/emu/navba_emu.cpp; this file is one kernel per phase and the host side
// of the C ABI: the inertial arrays here, the device's Team, the executor and the exchange of the observation graph in ba.hpp.
//
// As ba.hip: a phase is one launch with one workgroup of 256 lanes per block, the launches of a call follow each other in the
// matcher's stream, no kernel waits for another workgroup.  k_navba_lin_ctl and k_navba_trial_ctl leave the Levenberg decision as a
// status word, which the host reads through page-locked memory once per trial: at most 15 x 10 reads a call.
#include "navba.hpp"

namespace uvo {

#define UVO_K(name, ph) UVO_BA_KERNEL(navba, 2 * 15 * navba::kMaxFree, name, navba::ph)
UVO_K(k_navba_init, kInit)
UVO_K(k_navba_begin, kBegin)
UVO_K(k_navba_edge_lin, kEdgeLin)
UVO_K(k_navba_inert_lin, kInertLin)
UVO_K(k_navba_point_sum, kPointSum)
UVO_K(k_navba_kf_sum, kKfSum)
UVO_K(k_navba_lin_ctl, kLinCtl)
UVO_K(k_navba_dinv, kDinv)
UVO_K(k_navba_schur, kSchur)
UVO_K(k_navba_inert_add, kInertAdd)
UVO_K(k_navba_solve, kSolve)
UVO_K(k_navba_step, kStep)
UVO_K(k_navba_edge_err, kEdgeErr)
UVO_K(k_navba_inert_err, kInertErr)
UVO_K(k_navba_trial_ctl, kTrialCtl)
UVO_K(k_navba_check, kCheck)
UVO_K(k_navba_finish, kFinish)
#undef UVO_K

}  // namespace uvo

// ---------------------------------------------------------------------------------------------------------------------------
using namespace uvo;

static_assert(sizeof(uvo_nav_ba_trace) == sizeof(navba::Trace) && sizeof(uvo_nav_ba_trace_lin) == sizeof(navba::TraceLin), "uvo_nav_ba_trace is navba::Trace");
static_assert(sizeof(uvo_nav_state) == sizeof(navopt::State) && sizeof(uvo_nav_ba_link) == sizeof(navba::Link) && sizeof(uvo_nav_ba_depth) == sizeof(navba::Depth),
              "the C ABI's records are the core's");

struct uvo_nav_bundle_adjuster : BaHandle {
  int max_free = 0, max_fixed = 0, max_points = 0, max_edges = 0, max_depth = 0;
  navba::Ws W;
  NavBaInertial d_in, h_in;                                // the upload's own arrays, in front of the graph's
  navopt::State *d_kf_out = nullptr, *h_kf_out = nullptr;  // the download's, in front of the shared answer
};

namespace {

#define UVO_K(name) {name, #name}
const BaPhaseKernel<navba::Ws> kKernels[navba::kPhases] = {
    UVO_K(k_navba_init),      UVO_K(k_navba_begin), UVO_K(k_navba_edge_lin), UVO_K(k_navba_inert_lin), UVO_K(k_navba_point_sum), UVO_K(k_navba_kf_sum),
    UVO_K(k_navba_lin_ctl),   UVO_K(k_navba_dinv),  UVO_K(k_navba_schur),    UVO_K(k_navba_inert_add), UVO_K(k_navba_solve),     UVO_K(k_navba_step),
    UVO_K(k_navba_edge_err),  UVO_K(k_navba_inert_err), UVO_K(k_navba_trial_ctl), UVO_K(k_navba_check), UVO_K(k_navba_finish)};
#undef UVO_K

BaResultFields fields_of(uvo_nav_ba_result& r) {
  return {r.kf_Tcw, r.point_estimate, r.points, r.excluded, r.erased, &r.n_excluded, &r.n_erased, r.iterations, &r.n_trials, &r.n_syncs};
}

// the answer when nothing is optimised: the inputs' conversions
void answer_unchanged(const uvo_nav_ba_problem& q, uvo_nav_ba_result& r) {
  navba::Params prm;
  std::memcpy(prm.Rbc, q.Rbc, sizeof prm.Rbc), std::memcpy(prm.Pbc, q.Pbc, sizeof prm.Pbc);
  for (int k = 0; k < q.n_keyframes; ++k) {
    navopt::State s;
    std::memcpy(&s, q.kf_state + k, sizeof s);
    navopt::q_normalize(s.q);
    if (r.kf_state) std::memcpy(r.kf_state + k, &s, sizeof s);
    if (r.kf_Tcw) navba::pose_from_ns(s, prm, r.kf_Tcw + 16 * k);
  }
  ba_answer_unchanged(q, fields_of(r));
}

}  // namespace

extern "C" {

void uvo_nav_bundle_adjuster_destroy(uvo_nav_bundle_adjuster* a) { ba_destroy(a); }

int uvo_nav_bundle_adjuster_create(uvo_matcher* m, int max_free, int max_fixed, int max_points, int max_edges, int max_depth, uvo_nav_bundle_adjuster** out) {
  if (!m || !out) return fail(UVO_E_BADARG, "null pointer");
  *out = nullptr;
  if (max_free < 1 || max_free > navba::kMaxFree || max_fixed < 0 || max_fixed > navba::kMaxFixed || max_points < 1 || max_points > navba::kMaxPoints ||
      max_edges < 1 || max_edges > navba::kMaxEdges || max_depth < 0 || max_depth > navba::kMaxDepth)
    return fail(UVO_E_BADARG, "nav bundle adjuster: 1..24 free and 0..256 fixed key frames, 1..32768 points, 1..262144 edges, 0..256 depth entries");
  uvo_nav_bundle_adjuster* a = new uvo_nav_bundle_adjuster();
  a->m = m, a->max_free = max_free, a->max_fixed = max_fixed, a->max_points = max_points, a->max_edges = max_edges, a->max_depth = max_depth;
  const size_t F = (size_t)max_free, K = F + (size_t)max_fixed, P = (size_t)max_points, E = (size_t)max_edges, D = (size_t)max_depth, N = 15 * F;
  const size_t G = 2 * (size_t)navba::kMaxLinks + D;
  const size_t ce = (size_t)navba::chunks(max_edges), cp = (size_t)navba::chunks(max_points);
  navba::Ws& W = a->W;
  std::memset(&W, 0, sizeof W);
  int rc = hipSetDevice(m->device) == hipSuccess ? UVO_OK : fail(UVO_E_NOMEM, "nav bundle adjuster allocation failed");
  if (!rc) rc = alloc_carved(a->mem, [&](Carve& c) {
    a->d_in.layout(c, K, D), a->d_graph.layout(c, K, F, P, E);
    c.take(W.ns, K).take(W.ns_try, K).take(W.cam, 12 * K).take(W.cam_try, 12 * K).take(W.camc, 3).take(W.X, 3 * P).take(W.X_try, 3 * P);
    c.take(W.e_off, E).take(W.e_rob, E).take(W.e_chi2, E).take(W.e_lin, E * navba::kEdgeWords);
    c.take(W.Hll, 9 * P).take(W.Dinv, 9 * P).take(W.p_on, P).take(W.Hpp, 27 * F).take(W.hdiag, N).take(W.link_info, 81 * (size_t)navba::kMaxLinks);
    c.take(W.ie_lin, G * navba::kIeWords).take(W.ie_col, 4 * G).take(W.ie_try, G).take(W.ie_etry, 9 * G);
    c.take(W.Hs, N * N).take(W.bs, N).take(W.bfull, N).take(W.xp, N).take(W.xl, 3 * P);
    c.take(W.chunk_chi2, ce).take(W.chunk_scale, cp).take(W.chunk_max, cp + F).take(W.chunk_n, ce).take(W.trace, 1);
    c.take(a->d_kf_out, K), a->d_ans.layout(c, K, P, E);
  });
  if (!rc) rc = alloc_carved(a->mem, [&](Carve& c) { a->h_in.layout(c, K, D), a->h_graph.layout(c, K, F, P, E); }, true);
  if (!rc) rc = alloc_carved(a->mem, [&](Carve& c) { c.take(a->h_kf_out, K), a->h_ans.layout(c, K, P, E), c.take(a->h_status, 1); }, true);
  if (rc) return uvo_nav_bundle_adjuster_destroy(a), rc;
  a->d_graph.bind(W);
  const NavBaInertial& u = a->d_in;
  W.kf_in = u.kf_in, W.kf_bias = u.kf_bias, W.links = u.links, W.depths = u.depths, W.prm = u.prm;
  const BaAnswer& d = a->d_ans;
  W.kf_out = a->d_kf_out, W.kf_T_out = d.kf_T_out, W.pt_est = d.pt_est, W.pt_out = d.pt_out, W.excluded = d.mask1, W.erased = d.mask2, W.ctl = d.ctl;
  *out = a;
  return UVO_OK;
}

int uvo_nav_bundle_adjust(uvo_nav_bundle_adjuster* a, const uvo_nav_ba_problem* problem, uvo_nav_ba_result* result) {
  if (!a) return fail(UVO_E_BADARG, "null handle");
  if (!problem || !result) return fail(UVO_E_BADARG, "null pointer");
  const uvo_nav_ba_problem& q = *problem;
  if (q.n_keyframes < 0 || q.n_points < 0 || q.n_edges < 0 || q.n_cameras < 0 || q.n_cameras > navba::kMaxCams || q.n_links < 0 || q.n_depth < 0)
    return fail(UVO_E_BADARG, "nav bundle adjustment: count out of range");
  if ((q.n_keyframes > 0 && (!q.kf_state || !q.kf_fixed || !q.kf_has_bias)) || (q.n_points > 0 && !q.points) || !q.point_edge_begin ||
      (q.n_edges > 0 && (!q.edge_kf || !q.edge_obs || !q.edge_inv_sigma2 || !q.edge_camera || !q.cameras)) || (q.n_links > 0 && !q.links) ||
      (q.n_depth > 0 && !q.depth))
    return fail(UVO_E_BADARG, "null pointer");
  const int K = q.n_keyframes, P = q.n_points, E = q.n_edges, L = q.n_links, D = q.n_depth;
  int n_free = 0;
  for (int k = 0; k < K; ++k) n_free += q.kf_fixed[k] ? 0 : 1;
  if (n_free > a->max_free || K - n_free > a->max_fixed || P > a->max_points || E > a->max_edges || L > navba::kMaxLinks || D > a->max_depth)
    return fail(UVO_E_CAPACITY, "more key frames, points, edges, links or depth entries than the nav bundle adjuster was sized for");
  const NavBaInertial& h = a->h_in;
  int F = 0;
  if (a->h_graph.derive(q, &F))
    return fail(UVO_E_BADARG, "nav bundle adjustment: an edge names a key frame or camera out of range, or the edge lists are not well formed");
  if (L > 0) std::memcpy(h.links, q.links, sizeof(navba::Link) * (size_t)L);
  if (D > 0) std::memcpy(h.depths, q.depth, sizeof(navba::Depth) * (size_t)D);
  if (navba::check_inertial(K, q.kf_fixed, q.kf_has_bias, L, h.links, D, h.depths))
    return fail(UVO_E_BADARG, "nav bundle adjustment: a link or depth entry names a key frame out of range or a bias vertex that is not there, or a free key frame has no link");
  if (F == 0) return a->ran = a->last_empty = true, answer_unchanged(q, *result), UVO_OK;
  std::memcpy(h.kf_in, q.kf_state, sizeof(navopt::State) * (size_t)K);
  std::memcpy(h.kf_bias, q.kf_has_bias, (size_t)K);
  a->h_graph.pack(q);
  navba::Params& prm = *h.prm;
  std::memcpy(prm.Rbc, q.Rbc, sizeof prm.Rbc), std::memcpy(prm.Pbc, q.Pbc, sizeof prm.Pbc), std::memcpy(prm.gw, q.gw, sizeof prm.gw);
  prm.gyr_rw2 = q.gyr_bias_rw2, prm.acc_rw2 = q.acc_bias_rw2;

  uvo_matcher* m = a->m;
  UVO_HIP_CHECK(hipSetDevice(m->device));
  hipStream_t st = m->stream;
  const NavBaInertial& d = a->d_in;
#define UVO_NAVBA_UP(field, count) \
  if ((size_t)(count) > 0) UVO_HIP_CHECK(hipMemcpyAsync(d.field, h.field, sizeof(*h.field) * (size_t)(count), hipMemcpyHostToDevice, st))
  UVO_NAVBA_UP(kf_in, K);
  UVO_NAVBA_UP(links, L);
  UVO_NAVBA_UP(depths, D);
  UVO_NAVBA_UP(prm, 1);
  UVO_NAVBA_UP(kf_bias, K);
#undef UVO_NAVBA_UP
  RC(a->h_graph.send(a->d_graph, K, F, P, E, q.n_cameras, st));
  navba::Ws& W = a->W;
  W.K = K, W.F = F, W.P = P, W.E = E, W.C = q.n_cameras, W.L = L, W.D = D;
  BaExec<navba::Ws> x = {st, &m->prof, &W, a->h_status, kKernels};
  int syncs = 0;
  const navba::Dims dims = {K, F, P, E, L, D};
  RC(navba::drive(x, dims, &syncs));
  UVO_HIP_CHECK(hipMemcpyAsync(a->h_kf_out, a->d_kf_out, sizeof(navopt::State) * (size_t)K, hipMemcpyDeviceToHost, st));
  RC(a->h_ans.receive(a->d_ans, K, P, E, st));
  UVO_HIP_CHECK(hipStreamSynchronize(st));
  a->ran = true, a->last_empty = false;
  if (result->kf_state) std::memcpy(result->kf_state, a->h_kf_out, sizeof(navopt::State) * (size_t)K);
  a->h_ans.store(fields_of(*result), K, P, E, syncs);
  return UVO_OK;
}

int uvo_nav_bundle_adjuster_trace(uvo_nav_bundle_adjuster* a, uvo_nav_ba_trace* out) { return ba_read_trace(a, out); }

}  // extern "C"
