// Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:2409-2658) as one call.  All arithmetic, the phases and their launch sequence
// are essential_core.hpp, shared with the host build tests/emu/essential_emu.cpp; this file is one kernel per phase and the host side
// of the C ABI.  The device's team, the kernel of a phase and the executor are ba.hpp's, the exchange essential.hpp's.
//
// A phase is one launch with one workgroup of 256 lanes per block; the launches of a call follow each other in the matcher's stream.
// No kernel waits for another workgroup.  k_essential_solve, the block-envelope LDL^T, is one workgroup: the seven pivots and the
// diagonal block's factor of the column in hand stand in LDS, the envelope in global memory.  The Levenberg decision is taken by
// k_essential_trial_ctl and left as a status word, which the host reads through page-locked memory after a stream synchronise: one
// read per trial, at most 200 a call of 20 iterations.  A HIP error ends the call at once.
#include "essential.hpp"

#include <cstdio>
#include <vector>

namespace uvo {

#define UVO_K(name, ph) UVO_BA_KERNEL(essential, essential::kTeamWords, name, essential::ph)
UVO_K(k_essential_init, kInit)
UVO_K(k_essential_measure, kMeasure)
UVO_K(k_essential_edge_lin, kEdgeLin)
UVO_K(k_essential_kf_sum, kKfSum)
UVO_K(k_essential_pair_sum, kPairSum)
UVO_K(k_essential_lin_ctl, kLinCtl)
UVO_K(k_essential_copy, kCopy)
UVO_K(k_essential_solve, kSolve)
UVO_K(k_essential_step, kStepPh)
UVO_K(k_essential_edge_err, kEdgeErr)
UVO_K(k_essential_trial_ctl, kTrialCtl)
UVO_K(k_essential_finish_kf, kFinishKf)
UVO_K(k_essential_finish_pts, kFinishPts)
#undef UVO_K

}  // namespace uvo

// ---------------------------------------------------------------------------------------------------------------------------
using namespace uvo;

static_assert(sizeof(uvo_sim3d) == sizeof(essential::Sim) && sizeof(uvo_sim3d) == 64, "uvo_sim3d is sim3opt::Sim");
static_assert(sizeof(uvo_essential_trace) == sizeof(ba::Trace), "uvo_essential_trace is ba::Trace");

struct uvo_essential_graph {
  uvo_matcher* m = nullptr;
  bool ran = false, last_empty = false;
  int max_keyframes = 0, max_edges = 0, max_blocks = 0, max_points = 0;
  DevMem mem;
  essential::Ws W;  // the device's arrays
  EssGraph d_graph, h_graph;
  EssAnswer d_ans, h_ans;
  int32_t* h_status = nullptr;
  std::vector<int64_t> scratch;
};

namespace {

#define UVO_K(name) {name, #name}
const BaPhaseKernel<essential::Ws> kKernels[essential::kPhases] = {
    UVO_K(k_essential_init),  UVO_K(k_essential_measure), UVO_K(k_essential_edge_lin), UVO_K(k_essential_kf_sum),    UVO_K(k_essential_pair_sum),
    UVO_K(k_essential_lin_ctl), UVO_K(k_essential_copy),  UVO_K(k_essential_solve),    UVO_K(k_essential_step),      UVO_K(k_essential_edge_err),
    UVO_K(k_essential_trial_ctl), UVO_K(k_essential_finish_kf), UVO_K(k_essential_finish_pts)};
#undef UVO_K

}  // namespace

extern "C" {

void uvo_essential_graph_destroy(uvo_essential_graph* g) {
  if (!g) return;
  hipSetDevice(g->m->device);
  if (g->m->stream) hipStreamSynchronize(g->m->stream);
  g->mem.release_all();
  delete g;
}

int uvo_essential_graph_create(uvo_matcher* m, int max_keyframes, int max_edges, int max_envelope_blocks, int max_points, uvo_essential_graph** out) {
  if (!m || !out) return fail(UVO_E_BADARG, "null pointer");
  *out = nullptr;
  if (max_keyframes < 1 || max_keyframes > essential::kMaxKeyframes || max_edges < 1 || max_edges > essential::kMaxEdges || max_envelope_blocks < 1 ||
      max_envelope_blocks > essential::kMaxBlocks || max_points < 0 || max_points > essential::kMaxPoints)
    return fail(UVO_E_BADARG, "essential graph: 1..8192 key frames, 1..262144 edges, 1..4194304 envelope blocks, 0..1048576 points");
  uvo_essential_graph* g = new uvo_essential_graph();
  g->m = m, g->max_keyframes = max_keyframes, g->max_edges = max_edges, g->max_blocks = max_envelope_blocks, g->max_points = max_points;
  const size_t K = (size_t)max_keyframes, E = (size_t)max_edges, NB = (size_t)max_envelope_blocks, P = (size_t)max_points, N = 7 * K;
  g->scratch.resize(std::max(E, K) + 1);
  essential::Ws& W = g->W;
  std::memset(&W, 0, sizeof W);
  int rc = hipSetDevice(m->device) == hipSuccess ? UVO_OK : fail(UVO_E_NOMEM, "essential graph allocation failed");
  if (!rc) rc = alloc_carved(g->mem, [&](Carve& c) {
    g->d_graph.layout(c, K, E, P, NB);
    c.take(W.est, K).take(W.est_try, K).take(W.meas, E).take(W.e_lin, E * essential::kEdgeWords).take(W.H, 49 * NB).take(W.L, 49 * NB);
    c.take(W.b, N).take(W.x, N).take(W.y, N).take(W.chunk_chi2, (size_t)essential::chunks(max_edges));
    c.take(W.chunk_scale, (size_t)essential::chunks((int)N)).take(W.chunk_max, (size_t)essential::kf_blocks(max_keyframes)).take(W.trace, 1);
    g->d_ans.layout(c, K, P);
  });
  if (!rc) rc = alloc_carved(g->mem, [&](Carve& c) { g->h_graph.layout(c, K, E, P, NB); }, true);
  if (!rc) rc = alloc_carved(g->mem, [&](Carve& c) { g->h_ans.layout(c, K, P), c.take(g->h_status, 1); }, true);
  if (rc) return uvo_essential_graph_destroy(g), rc;
  g->d_graph.bind(W);
  W.Scw_out = g->d_ans.Scw_out, W.kf_T_out = g->d_ans.kf_T_out, W.pt_out = g->d_ans.pt_out, W.ctl = g->d_ans.ctl;
  *out = g;
  return UVO_OK;
}

int uvo_essential_graph_optimize(uvo_essential_graph* g, const uvo_essential_problem* problem, uvo_essential_result* result) {
  if (!g) return fail(UVO_E_BADARG, "null handle");
  if (!problem || !result) return fail(UVO_E_BADARG, "null pointer");
  const uvo_essential_problem& q = *problem;
  const int K = q.n_keyframes, E = q.n_edges, P = q.n_points;
  if (K < 1 || E < 0 || P < 0) return fail(UVO_E_BADARG, "essential graph: count out of range");
  if (q.n_iterations < 1 || q.n_iterations > essential::kMaxIterations) return fail(UVO_E_BADARG, "essential graph: 1..32 iterations");
  if (!q.Scw || !q.Scw_normal || (E > 0 && (!q.edge_i || !q.edge_j || !q.edge_connection)) || (P > 0 && (!q.points || !q.point_ref)))
    return fail(UVO_E_BADARG, "null pointer");
  if (K > g->max_keyframes || E > g->max_edges || P > g->max_points) return fail(UVO_E_CAPACITY, "more key frames, edges or points than the essential graph was sized for");
  for (int j = 0; j < P; ++j)
    if (q.point_ref[j] < 0 || q.point_ref[j] >= K) return fail(UVO_E_BADARG, "essential graph: a point's reference key frame is out of range");
  EssGraph& h = g->h_graph;
  essential::Dims d = {K, K - 1, P, E, 0, 0};
  const int bad = essential::derive<essential::kMutNone>(K, q.fixed, E, q.edge_i, q.edge_j, g->max_blocks, h.kf_free, h.inc_begin, h.inc_edge, h.pair_begin, h.pair_rc,
                                                         h.pair_edge, h.first, h.env_off, h.col_begin, h.col_rows, h.blk_row, g->scratch.data(), &d);
  if (bad == essential::kDeriveRange) return fail(UVO_E_BADARG, "essential graph: the fixed key frame or an edge's key frame is out of range");
  if (bad == essential::kDeriveSelf) return fail(UVO_E_BADARG, "essential graph: an edge joins a key frame to itself");
  if (bad == essential::kDeriveCapacity) {
    char msg[160];
    std::snprintf(msg, sizeof msg, "essential graph: the envelope needs %d blocks, the handle was sized for %d", d.NB, g->max_blocks);
    return fail(UVO_E_CAPACITY, msg);
  }
  d.P = P;
  std::memcpy(h.Scw, q.Scw, sizeof(uvo_sim3d) * (size_t)K), std::memcpy(h.Scwn, q.Scw_normal, sizeof(uvo_sim3d) * (size_t)K);
  if (E > 0) std::memcpy(h.e_i, q.edge_i, 4 * (size_t)E), std::memcpy(h.e_j, q.edge_j, 4 * (size_t)E), std::memcpy(h.e_conn, q.edge_connection, (size_t)E);
  if (P > 0) std::memcpy(h.pts, q.points, 12 * (size_t)P), std::memcpy(h.pt_ref, q.point_ref, 4 * (size_t)P);

  uvo_matcher* m = g->m;
  UVO_HIP_CHECK(hipSetDevice(m->device));
  hipStream_t st = m->stream;
  RC(h.send(g->d_graph, d, st));
  essential::Ws& W = g->W;
  W.K = K, W.F = d.F, W.P = P, W.E = E, W.NP = d.NP, W.NB = d.NB, W.fixed = q.fixed, W.pad_ = 0;
  BaExec<essential::Ws> x = {st, &m->prof, &W, g->h_status, kKernels};
  int syncs = 0;
  RC(essential::drive(x, d, q.n_iterations, &syncs));
  RC(g->h_ans.receive(g->d_ans, K, P, st));
  UVO_HIP_CHECK(hipStreamSynchronize(st));
  g->ran = true, g->last_empty = false;
  const EssAnswer& a = g->h_ans;
  if (result->Scw) std::memcpy(result->Scw, a.Scw_out, sizeof(uvo_sim3d) * (size_t)K);
  if (result->kf_Tcw) std::memcpy(result->kf_Tcw, a.kf_T_out, sizeof(float) * 16 * (size_t)K);
  if (result->points && P > 0) std::memcpy(result->points, a.pt_out, sizeof(float) * 3 * (size_t)P);
  result->iterations = a.ctl->its[0], result->n_trials = a.ctl->n_trials, result->n_syncs = syncs + 1, result->envelope_blocks = d.NB;
  return UVO_OK;
}

int uvo_essential_graph_trace(uvo_essential_graph* g, uvo_essential_trace* out) { return ba_read_trace(g, out); }

}  // extern "C"
