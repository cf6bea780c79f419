// Optimizer::LocalBundleAdjustment (src/Optimizer.cc:2147-2405) and Optimizer::BundleAdjustment (:1896-2010) as one call.  All arithmetic,
// the phases and their launch sequence are ba_core.hpp, shared with the host build tests/emu/ba_emu.cpp; this file is one kernel per
// phase and the host side of the C ABI.  The device's Team, the executor and the exchange of the observation graph are ba.hpp's, shared
// with navba.hip.
//
// A phase is one launch with one workgroup of 256 lanes per block; the launches of a call follow each other in the matcher's stream.
// No kernel waits for another workgroup: what a phase needs of an earlier one is in global memory when it starts.  The Levenberg
// decision is taken by k_ba_lin_ctl and k_ba_trial_ctl (one workgroup) and left as a status word, which the host reads through
// page-locked memory after a stream synchronise to choose the next launches: one read per trial and one per optimize(), at most
// 2 + 15 x 10 a call in local mode.  A HIP error ends the call at once.  The reduction is lane_team.hpp's.
#include "ba.hpp"

namespace uvo {

#define UVO_K(name, ph) UVO_BA_KERNEL(ba, 2 * 6 * ba::kMaxFree, name, ba::ph)
UVO_K(k_ba_init, kInit)
UVO_K(k_ba_begin, kBegin)
UVO_K(k_ba_edge_lin, kEdgeLin)
UVO_K(k_ba_point_sum, kPointSum)
UVO_K(k_ba_kf_sum, kKfSum)
UVO_K(k_ba_lin_ctl, kLinCtl)
UVO_K(k_ba_dinv, kDinv)
UVO_K(k_ba_schur, kSchur)
UVO_K(k_ba_solve, kSolve)
UVO_K(k_ba_step, kStep)
UVO_K(k_ba_edge_err, kEdgeErr)
UVO_K(k_ba_trial_ctl, kTrialCtl)
UVO_K(k_ba_check, kCheck)
UVO_K(k_ba_finish, kFinish)
#undef UVO_K

}  // namespace uvo

// ---------------------------------------------------------------------------------------------------------------------------
using namespace uvo;

static_assert(sizeof(uvo_ba_trace) == sizeof(ba::Trace) && sizeof(uvo_ba_trace_lin) == sizeof(ba::TraceLin), "uvo_ba_trace is ba::Trace");

struct uvo_bundle_adjuster : BaHandle {
  int max_free = 0, max_fixed = 0, max_points = 0, max_edges = 0;
  ba::Ws W;       // the device's arrays
  float *d_kf_T = nullptr, *h_kf_T = nullptr;      // the upload's own array, in front of the graph's
  double *d_kf_est = nullptr, *h_kf_est = nullptr; // the download's, in front of the shared answer
};

namespace {

#define UVO_K(name) {name, #name}
const BaPhaseKernel<ba::Ws> kKernels[ba::kPhases] = {UVO_K(k_ba_init),   UVO_K(k_ba_begin), UVO_K(k_ba_edge_lin), UVO_K(k_ba_point_sum), UVO_K(k_ba_kf_sum),
                                                     UVO_K(k_ba_lin_ctl), UVO_K(k_ba_dinv),  UVO_K(k_ba_schur),    UVO_K(k_ba_solve),     UVO_K(k_ba_step),
                                                     UVO_K(k_ba_edge_err), UVO_K(k_ba_trial_ctl), UVO_K(k_ba_check), UVO_K(k_ba_finish)};
#undef UVO_K

BaResultFields fields_of(uvo_ba_result& r) {
  return {r.kf_Tcw, r.point_estimate, r.points, r.removed1, r.removed2, &r.n_removed1, &r.n_removed2, r.iterations, &r.n_trials, &r.n_syncs};
}

// the answer when nothing is optimised: the inputs' conversions
void answer_unchanged(const uvo_ba_problem& q, uvo_ba_result& r) {
  for (int k = 0; k < q.n_keyframes; ++k) {
    float M[16];
    std::memcpy(M, q.kf_Tcw + 12 * k, sizeof(float) * 12);
    M[12] = M[13] = M[14] = 0.f, M[15] = 1.f;
    poseopt::Pose P;
    poseopt::pose_of(M, P);
    if (r.kf_estimate) std::memcpy(r.kf_estimate + 7 * k, P.q, sizeof(double) * 4), std::memcpy(r.kf_estimate + 7 * k + 4, P.t, sizeof(double) * 3);
    if (r.kf_Tcw) std::memcpy(r.kf_Tcw + 16 * k, M, sizeof M);
  }
  ba_answer_unchanged(q, fields_of(r));
}

}  // namespace

extern "C" {

void uvo_bundle_adjuster_destroy(uvo_bundle_adjuster* a) { ba_destroy(a); }

int uvo_bundle_adjuster_create(uvo_matcher* m, int max_free, int max_fixed, int max_points, int max_edges, uvo_bundle_adjuster** out) {
  if (!m || !out) return fail(UVO_E_BADARG, "null pointer");
  *out = nullptr;
  if (max_free < 1 || max_free > ba::kMaxFree || max_fixed < 0 || max_fixed > ba::kMaxFixed || max_points < 1 || max_points > ba::kMaxPoints ||
      max_edges < 1 || max_edges > ba::kMaxEdges)
    return fail(UVO_E_BADARG, "bundle adjuster: 1..64 free and 0..256 fixed key frames, 1..32768 points, 1..262144 edges");
  uvo_bundle_adjuster* a = new uvo_bundle_adjuster();
  a->m = m, a->max_free = max_free, a->max_fixed = max_fixed, a->max_points = max_points, a->max_edges = max_edges;
  const size_t F = (size_t)max_free, K = F + (size_t)max_fixed, P = (size_t)max_points, E = (size_t)max_edges, N = 6 * F;
  const size_t ce = (size_t)ba::chunks(max_edges), cp = (size_t)ba::chunks(max_points);
  ba::Ws& W = a->W;
  std::memset(&W, 0, sizeof W);
  int rc = hipSetDevice(m->device) == hipSuccess ? UVO_OK : fail(UVO_E_NOMEM, "bundle adjuster allocation failed");
  if (!rc) rc = alloc_carved(a->mem, [&](Carve& c) {
    c.take(a->d_kf_T, 12 * K), a->d_graph.layout(c, K, F, P, E);
    c.take(W.pose, K).take(W.pose_try, K).take(W.X, 3 * P).take(W.X_try, 3 * P).take(W.e_off, E).take(W.e_chi2, E).take(W.e_lin, E * ba::kEdgeWords);
    c.take(W.Hll, 9 * P).take(W.Dinv, 9 * P).take(W.p_on, P).take(W.Hpp, 27 * F).take(W.f_on, F).take(W.Hs, N * N).take(W.bs, N).take(W.xp, N).take(W.xl, 3 * P);
    c.take(W.chunk_chi2, ce).take(W.chunk_scale, cp).take(W.chunk_max, cp + F).take(W.chunk_n, ce).take(W.trace, 1);
    c.take(a->d_kf_est, 7 * K), a->d_ans.layout(c, K, P, E);
  });
  if (!rc) rc = alloc_carved(a->mem, [&](Carve& c) { c.take(a->h_kf_T, 12 * K), a->h_graph.layout(c, K, F, P, E); }, true);
  if (!rc) rc = alloc_carved(a->mem, [&](Carve& c) { c.take(a->h_kf_est, 7 * K), a->h_ans.layout(c, K, P, E), c.take(a->h_status, 1); }, true);
  if (rc) return uvo_bundle_adjuster_destroy(a), rc;
  a->d_graph.bind(W);
  const BaAnswer& d = a->d_ans;
  W.kf_T = a->d_kf_T, W.kf_est = a->d_kf_est, W.kf_T_out = d.kf_T_out, W.pt_est = d.pt_est, W.pt_out = d.pt_out, W.removed1 = d.mask1, W.removed2 = d.mask2, W.ctl = d.ctl;
  *out = a;
  return UVO_OK;
}

int uvo_bundle_adjust(uvo_bundle_adjuster* a, const uvo_ba_problem* problem, uvo_ba_result* result) {
  if (!a) return fail(UVO_E_BADARG, "null handle");
  if (!problem || !result) return fail(UVO_E_BADARG, "null pointer");
  const uvo_ba_problem& q = *problem;
  if (q.mode != UVO_BA_LOCAL && q.mode != UVO_BA_FULL) return fail(UVO_E_BADARG, "bundle adjustment: unknown mode");
  if (q.mode == UVO_BA_FULL && (q.n_iterations < 1 || q.n_iterations > ba::kMaxIterations)) return fail(UVO_E_BADARG, "bundle adjustment: 1..32 iterations");
  if (q.n_keyframes < 0 || q.n_points < 0 || q.n_edges < 0 || q.n_cameras < 0 || q.n_cameras > ba::kMaxCams) return fail(UVO_E_BADARG, "bundle adjustment: count out of range");
  if ((q.n_keyframes > 0 && (!q.kf_Tcw || !q.kf_fixed)) || (q.n_points > 0 && !q.points) || !q.point_edge_begin ||
      (q.n_edges > 0 && (!q.edge_kf || !q.edge_obs || !q.edge_inv_sigma2 || !q.edge_camera || !q.cameras)))
    return fail(UVO_E_BADARG, "null pointer");
  const int K = q.n_keyframes, P = q.n_points, E = q.n_edges;
  int n_free = 0;
  for (int k = 0; k < K; ++k) n_free += q.kf_fixed[k] ? 0 : 1;
  if (n_free > a->max_free || K - n_free > a->max_fixed || P > a->max_points || E > a->max_edges)
    return fail(UVO_E_CAPACITY, "more key frames, points or edges than the bundle adjuster was sized for");
  int F = 0;
  if (a->h_graph.derive(q, &F))
    return fail(UVO_E_BADARG, "bundle adjustment: an edge names a key frame or camera out of range, or the edge lists are not well formed");
  if (F == 0 || E == 0) return a->ran = a->last_empty = true, answer_unchanged(q, *result), UVO_OK;
  std::memcpy(a->h_kf_T, q.kf_Tcw, sizeof(float) * 12 * (size_t)K);
  a->h_graph.pack(q);

  uvo_matcher* m = a->m;
  UVO_HIP_CHECK(hipSetDevice(m->device));
  hipStream_t st = m->stream;
  UVO_HIP_CHECK(hipMemcpyAsync(a->d_kf_T, a->h_kf_T, sizeof(float) * 12 * (size_t)K, hipMemcpyHostToDevice, st));
  RC(a->h_graph.send(a->d_graph, K, F, P, E, q.n_cameras, st));
  ba::Ws& W = a->W;
  W.K = K, W.F = F, W.P = P, W.E = E, W.C = q.n_cameras;
  BaExec<ba::Ws> x = {st, &m->prof, &W, a->h_status, kKernels};
  int syncs = 0;
  const ba::Dims dims = {K, F, P, E};
  RC(ba::drive(x, dims, q.mode == UVO_BA_LOCAL ? ba::kModeLocal : ba::kModeFull, q.n_iterations, &syncs));
  UVO_HIP_CHECK(hipMemcpyAsync(a->h_kf_est, a->d_kf_est, sizeof(double) * 7 * (size_t)K, hipMemcpyDeviceToHost, st));
  RC(a->h_ans.receive(a->d_ans, K, P, E, st));
  UVO_HIP_CHECK(hipStreamSynchronize(st));
  a->ran = true, a->last_empty = false;
  if (result->kf_estimate) std::memcpy(result->kf_estimate, a->h_kf_est, sizeof(double) * 7 * (size_t)K);
  a->h_ans.store(fields_of(*result), K, P, E, syncs);
  return UVO_OK;
}

int uvo_bundle_adjuster_trace(uvo_bundle_adjuster* a, uvo_ba_trace* out) { return ba_read_trace(a, out); }

}  // extern "C"
