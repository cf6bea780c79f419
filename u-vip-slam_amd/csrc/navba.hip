// Optimizer::LocalBundleAdjustmentNavState (src/Optimizer.cc:1105-1732) as one call.  All arithmetic, the phases and their launch
// sequence are navba_core.hpp, shared with the host build tests/emu/navba_emu.cpp; this file is the device's Team -- which lane takes
// which entry; how the 256 lane sums meet is lane_team.hpp's LaneTeam -- one kernel per phase, and the host side of the C ABI.
//
// As ba.hip: a phase is one launch with one workgroup of 256 lanes per block, the launches of a call follow each other in the
// matcher's stream, no kernel waits for another workgroup.  k_navba_lin_ctl and k_navba_trial_ctl leave the Levenberg decision as a
// status word, which the host reads through page-locked memory once per trial: at most 15 x 10 reads a call.
#include <cstring>

#include "devmem.hpp"
#include "matcher_priv.hpp"
#include "navba.hpp"

namespace uvo {
namespace {

struct NavBaTeam : LaneTeam<navba::kSchurSums> {
  double* v;  // LDS [2][15 * kMaxFree]
  __device__ __forceinline__ double* vec() const { return v; }
  template <class F>
  __device__ __forceinline__ double maxr(F f) {
    double m = f((int)threadIdx.x);
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) m = navba::max_nan(m, __shfl_xor(m, k));
    double* buf = red + phase * 4 * navba::kSchurSums;
    phase ^= 1;
    if ((threadIdx.x & 63) == 0) buf[wave_in_block()] = m;
    __syncthreads();
    return navba::max_nan(navba::max_nan(buf[0], buf[1]), navba::max_nan(buf[2], buf[3]));
  }
  // items 0..n-1 over the lanes, then a barrier: what the lanes wrote, to LDS or to global memory, is there for the whole workgroup
  template <class F>
  __device__ __forceinline__ void par(int n, F f) {
    for (int i = (int)threadIdx.x; i < n; i += navba::kLanes) f(i);
    __syncthreads();
  }
  template <class F>
  __device__ __forceinline__ void each(int n, F f) {
    par(n, f);
  }
  // rows over the wavefronts, columns over a wavefront's lanes
  template <class F>
  __device__ __forceinline__ void par2(int rows, int cols, F f) {
    const int lane = (int)threadIdx.x & 63;
    for (int r = wave_in_block(); r < rows; r += 4)
      for (int c = lane; c < cols; c += 64) f(r, c);
    __syncthreads();
  }
};

}  // namespace

#define UVO_NAVBA_KERNEL(name, ph)                                            \
  __global__ __launch_bounds__(256) void name(navba::Ws W) {                  \
    __shared__ double s_red[2 * 4 * navba::kSchurSums];                       \
    __shared__ double s_store[navba::kSchurSums];                             \
    __shared__ double s_vec[2 * 15 * navba::kMaxFree];                        \
    __shared__ int32_t s_redi[2 * 4];                                         \
    NavBaTeam T = {{s_red, s_redi, s_store, 0}, s_vec};                       \
    navba::run_phase<navba::kMutNone>(ph, W, T, (int)blockIdx.x);             \
  }

UVO_NAVBA_KERNEL(k_navba_init, navba::kInit)
UVO_NAVBA_KERNEL(k_navba_begin, navba::kBegin)
UVO_NAVBA_KERNEL(k_navba_edge_lin, navba::kEdgeLin)
UVO_NAVBA_KERNEL(k_navba_inert_lin, navba::kInertLin)
UVO_NAVBA_KERNEL(k_navba_point_sum, navba::kPointSum)
UVO_NAVBA_KERNEL(k_navba_kf_sum, navba::kKfSum)
UVO_NAVBA_KERNEL(k_navba_lin_ctl, navba::kLinCtl)
UVO_NAVBA_KERNEL(k_navba_dinv, navba::kDinv)
UVO_NAVBA_KERNEL(k_navba_schur, navba::kSchur)
UVO_NAVBA_KERNEL(k_navba_inert_add, navba::kInertAdd)
UVO_NAVBA_KERNEL(k_navba_solve, navba::kSolve)
UVO_NAVBA_KERNEL(k_navba_step, navba::kStep)
UVO_NAVBA_KERNEL(k_navba_edge_err, navba::kEdgeErr)
UVO_NAVBA_KERNEL(k_navba_inert_err, navba::kInertErr)
UVO_NAVBA_KERNEL(k_navba_trial_ctl, navba::kTrialCtl)
UVO_NAVBA_KERNEL(k_navba_check, navba::kCheck)
UVO_NAVBA_KERNEL(k_navba_finish, navba::kFinish)

}  // namespace uvo

// ---------------------------------------------------------------------------------------------------------------------------
using namespace uvo;

static_assert(sizeof(uvo_nav_ba_trace) == sizeof(navba::Trace) && sizeof(uvo_nav_ba_trace_lin) == sizeof(navba::TraceLin), "uvo_nav_ba_trace is navba::Trace");
static_assert(sizeof(uvo_nav_state) == sizeof(navopt::State) && sizeof(uvo_nav_ba_link) == sizeof(navba::Link) && sizeof(uvo_nav_ba_depth) == sizeof(navba::Depth),
              "the C ABI's records are the core's");

struct uvo_nav_bundle_adjuster {
  uvo_matcher* m = nullptr;
  int max_free = 0, max_fixed = 0, max_points = 0, max_edges = 0, max_depth = 0;
  bool ran = false, last_empty = false;
  DevMem mem;
  navba::Ws W;
  NavBaUpload d_up, h_up;
  NavBaDownload d_down, h_down;
  int32_t* h_status = nullptr;
};

namespace {

struct DevExec {
  uvo_nav_bundle_adjuster* a;
  int launch(int ph, int blocks) {
    if (blocks <= 0) return UVO_OK;
    static const struct {
      void (*fn)(navba::Ws);
      const char* name;
    } k[navba::kPhases] = {{k_navba_init, "k_navba_init"},           {k_navba_begin, "k_navba_begin"},         {k_navba_edge_lin, "k_navba_edge_lin"},
                           {k_navba_inert_lin, "k_navba_inert_lin"}, {k_navba_point_sum, "k_navba_point_sum"}, {k_navba_kf_sum, "k_navba_kf_sum"},
                           {k_navba_lin_ctl, "k_navba_lin_ctl"},     {k_navba_dinv, "k_navba_dinv"},           {k_navba_schur, "k_navba_schur"},
                           {k_navba_inert_add, "k_navba_inert_add"}, {k_navba_solve, "k_navba_solve"},         {k_navba_step, "k_navba_step"},
                           {k_navba_edge_err, "k_navba_edge_err"},   {k_navba_inert_err, "k_navba_inert_err"}, {k_navba_trial_ctl, "k_navba_trial_ctl"},
                           {k_navba_check, "k_navba_check"},         {k_navba_finish, "k_navba_finish"}};
    hipStream_t st = a->m->stream;
    {
      Profiler::Scope ps(&a->m->prof, k[ph].name, st);
      hipLaunchKernelGGL(k[ph].fn, dim3(blocks), dim3(256), 0, st, a->W);
    }
    UVO_HIP_CHECK(hipGetLastError());
    return UVO_OK;
  }
  int status(int* out) {
    hipStream_t st = a->m->stream;
    UVO_HIP_CHECK(hipMemcpyAsync(a->h_status, &a->W.ctl->status, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    UVO_HIP_CHECK(hipStreamSynchronize(st));
    *out = *a->h_status;
    return UVO_OK;
  }
};

void layout_upload(Carve& c, NavBaUpload& u, size_t K, size_t F, size_t P, size_t E, size_t D) {
  c.take(u.kf_in, K).take(u.links, (size_t)navba::kMaxLinks).take(u.depths, D + 1).take(u.prm, 1);
  c.take(u.kf_free, K).take(u.free_kf, F).take(u.kf_bias, K).take(u.pts, 3 * P).take(u.pt_bad, P).take(u.pt_begin, P + 1);
  c.take(u.e_kf, E).take(u.e_pt, E).take(u.e_cam, E).take(u.e_obs, 3 * E).take(u.cams, 4 * (size_t)navba::kMaxCams);
  c.take(u.kl_begin, F + 1).take(u.kl_edge, E).take(u.fp_edge, F * P);
}

void layout_download(Carve& c, NavBaDownload& d, size_t K, size_t P, size_t E) {
  c.take(d.kf_out, K).take(d.kf_T_out, 16 * K).take(d.pt_est, 3 * P).take(d.pt_out, 3 * P).take(d.excluded, E).take(d.erased, E).take(d.ctl, 1);
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
  for (int i = 0; i < 3 * q.n_points; ++i) {
    if (r.point_estimate) r.point_estimate[i] = (double)q.points[i];
    if (r.points) r.points[i] = q.points[i];
  }
  if (r.excluded && q.n_edges > 0) std::memset(r.excluded, 0, (size_t)q.n_edges);
  if (r.erased && q.n_edges > 0) std::memset(r.erased, 0, (size_t)q.n_edges);
  r.n_excluded = r.n_erased = 0, r.iterations[0] = r.iterations[1] = 0, r.n_trials = 0, r.n_syncs = 0;
}

}  // namespace

extern "C" {

void uvo_nav_bundle_adjuster_destroy(uvo_nav_bundle_adjuster* a) {
  if (!a) return;
  hipSetDevice(a->m->device);
  if (a->m->stream) hipStreamSynchronize(a->m->stream);
  a->mem.release_all();
  delete a;
}

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
    layout_upload(c, a->d_up, K, F, P, E, D);
    c.take(W.ns, K).take(W.ns_try, K).take(W.cam, 12 * K).take(W.cam_try, 12 * K).take(W.camc, 3).take(W.X, 3 * P).take(W.X_try, 3 * P);
    c.take(W.e_off, E).take(W.e_rob, E).take(W.e_chi2, E).take(W.e_lin, E * navba::kEdgeWords);
    c.take(W.Hll, 9 * P).take(W.Dinv, 9 * P).take(W.p_on, P).take(W.Hpp, 27 * F).take(W.hdiag, N).take(W.link_info, 81 * (size_t)navba::kMaxLinks);
    c.take(W.ie_lin, G * navba::kIeWords).take(W.ie_col, 4 * G).take(W.ie_try, G).take(W.ie_etry, 9 * G);
    c.take(W.Hs, N * N).take(W.bs, N).take(W.bfull, N).take(W.xp, N).take(W.xl, 3 * P);
    c.take(W.chunk_chi2, ce).take(W.chunk_scale, cp).take(W.chunk_max, cp + F).take(W.chunk_n, ce).take(W.trace, 1);
    layout_download(c, a->d_down, K, P, E);
  });
  if (!rc) rc = alloc_carved(a->mem, [&](Carve& c) { layout_upload(c, a->h_up, K, F, P, E, D); }, true);
  if (!rc) rc = alloc_carved(a->mem, [&](Carve& c) { layout_download(c, a->h_down, K, P, E), c.take(a->h_status, 1); }, true);
  if (rc) return uvo_nav_bundle_adjuster_destroy(a), rc;
  const NavBaUpload& u = a->d_up;
  W.kf_in = u.kf_in, W.kf_free = u.kf_free, W.kf_bias = u.kf_bias, W.free_kf = u.free_kf, W.pts = u.pts, W.pt_bad = u.pt_bad, W.pt_begin = u.pt_begin;
  W.e_kf = u.e_kf, W.e_pt = u.e_pt, W.e_cam = u.e_cam, W.e_obs = u.e_obs, W.cams = u.cams, W.kl_begin = u.kl_begin, W.kl_edge = u.kl_edge, W.fp_edge = u.fp_edge;
  W.links = u.links, W.depths = u.depths, W.prm = u.prm;
  const NavBaDownload& d = a->d_down;
  W.kf_out = d.kf_out, W.kf_T_out = d.kf_T_out, W.pt_est = d.pt_est, W.pt_out = d.pt_out, W.excluded = d.excluded, W.erased = d.erased, W.ctl = d.ctl;
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
  NavBaUpload& h = a->h_up;
  int F = 0;
  if (ba::derive(K, q.kf_fixed, P, q.point_edge_begin, E, q.edge_kf, q.edge_camera, q.n_cameras, h.kf_free, h.free_kf, &F, h.e_pt, h.kl_begin, h.kl_edge, h.fp_edge))
    return fail(UVO_E_BADARG, "nav bundle adjustment: an edge names a key frame or camera out of range, or the edge lists are not well formed");
  static_assert(sizeof(uvo_nav_ba_link) == sizeof(navba::Link) && sizeof(uvo_nav_ba_depth) == sizeof(navba::Depth), "records copied as they are");
  if (L > 0) std::memcpy(h.links, q.links, sizeof(navba::Link) * (size_t)L);
  if (D > 0) std::memcpy(h.depths, q.depth, sizeof(navba::Depth) * (size_t)D);
  if (navba::check_inertial(K, q.kf_fixed, q.kf_has_bias, L, h.links, D, h.depths))
    return fail(UVO_E_BADARG, "nav bundle adjustment: a link or depth entry names a key frame out of range or a bias vertex that is not there, or a free key frame has no link");
  if (F == 0) return a->ran = a->last_empty = true, answer_unchanged(q, *result), UVO_OK;
  std::memcpy(h.kf_in, q.kf_state, sizeof(navopt::State) * (size_t)K);
  std::memcpy(h.kf_bias, q.kf_has_bias, (size_t)K);
  if (P > 0) std::memcpy(h.pts, q.points, sizeof(float) * 3 * (size_t)P);
  if (q.point_bad && P > 0) std::memcpy(h.pt_bad, q.point_bad, (size_t)P);
  else if (P > 0) std::memset(h.pt_bad, 0, (size_t)P);
  std::memcpy(h.pt_begin, q.point_edge_begin, sizeof(int32_t) * ((size_t)P + 1));
  if (E > 0) {
    std::memcpy(h.e_kf, q.edge_kf, sizeof(int32_t) * (size_t)E);
    std::memcpy(h.e_cam, q.edge_camera, sizeof(int32_t) * (size_t)E);
    for (int e = 0; e < E; ++e) h.e_obs[3 * e] = q.edge_obs[2 * e], h.e_obs[3 * e + 1] = q.edge_obs[2 * e + 1], h.e_obs[3 * e + 2] = q.edge_inv_sigma2[e];
    std::memcpy(h.cams, q.cameras, sizeof(float) * 4 * (size_t)q.n_cameras);
  }
  navba::Params& prm = *h.prm;
  std::memcpy(prm.Rbc, q.Rbc, sizeof prm.Rbc), std::memcpy(prm.Pbc, q.Pbc, sizeof prm.Pbc), std::memcpy(prm.gw, q.gw, sizeof prm.gw);
  prm.gyr_rw2 = q.gyr_bias_rw2, prm.acc_rw2 = q.acc_bias_rw2;

  uvo_matcher* m = a->m;
  UVO_HIP_CHECK(hipSetDevice(m->device));
  hipStream_t st = m->stream;
  const NavBaUpload& d = a->d_up;
#define UVO_NAVBA_UP(field, count) \
  if ((size_t)(count) > 0) UVO_HIP_CHECK(hipMemcpyAsync(d.field, h.field, sizeof(*h.field) * (size_t)(count), hipMemcpyHostToDevice, st))
  UVO_NAVBA_UP(kf_in, K);
  UVO_NAVBA_UP(links, L);
  UVO_NAVBA_UP(depths, D);
  UVO_NAVBA_UP(prm, 1);
  UVO_NAVBA_UP(kf_free, K);
  UVO_NAVBA_UP(free_kf, F);
  UVO_NAVBA_UP(kf_bias, K);
  UVO_NAVBA_UP(pts, 3 * P);
  UVO_NAVBA_UP(pt_bad, P);
  UVO_NAVBA_UP(pt_begin, P + 1);
  UVO_NAVBA_UP(e_kf, E);
  UVO_NAVBA_UP(e_pt, E);
  UVO_NAVBA_UP(e_cam, E);
  UVO_NAVBA_UP(e_obs, 3 * (size_t)E);
  UVO_NAVBA_UP(cams, 4 * q.n_cameras);
  UVO_NAVBA_UP(kl_begin, F + 1);
  UVO_NAVBA_UP(kl_edge, E);
  UVO_NAVBA_UP(fp_edge, (size_t)F * (size_t)P);
#undef UVO_NAVBA_UP
  navba::Ws& W = a->W;
  W.K = K, W.F = F, W.P = P, W.E = E, W.C = q.n_cameras, W.L = L, W.D = D;
  DevExec x = {a};
  int syncs = 0;
  const navba::Dims dims = {K, F, P, E, L, D};
  RC(navba::drive(x, dims, &syncs));
  const NavBaDownload &dd = a->d_down, &hd = a->h_down;
#define UVO_NAVBA_DOWN(field, count) \
  if ((size_t)(count) > 0) UVO_HIP_CHECK(hipMemcpyAsync(hd.field, dd.field, sizeof(*hd.field) * (size_t)(count), hipMemcpyDeviceToHost, st))
  UVO_NAVBA_DOWN(kf_out, K);
  UVO_NAVBA_DOWN(kf_T_out, 16 * K);
  UVO_NAVBA_DOWN(pt_est, 3 * (size_t)P);
  UVO_NAVBA_DOWN(pt_out, 3 * (size_t)P);
  UVO_NAVBA_DOWN(excluded, E);
  UVO_NAVBA_DOWN(erased, E);
  UVO_NAVBA_DOWN(ctl, 1);
#undef UVO_NAVBA_DOWN
  UVO_HIP_CHECK(hipStreamSynchronize(st));
  a->ran = true, a->last_empty = false;
  uvo_nav_ba_result& r = *result;
  if (r.kf_state) std::memcpy(r.kf_state, hd.kf_out, sizeof(navopt::State) * (size_t)K);
  if (r.kf_Tcw) std::memcpy(r.kf_Tcw, hd.kf_T_out, sizeof(float) * 16 * (size_t)K);
  if (r.point_estimate && P > 0) std::memcpy(r.point_estimate, hd.pt_est, sizeof(double) * 3 * (size_t)P);
  if (r.points && P > 0) std::memcpy(r.points, hd.pt_out, sizeof(float) * 3 * (size_t)P);
  if (r.excluded && E > 0) std::memcpy(r.excluded, hd.excluded, (size_t)E);
  if (r.erased && E > 0) std::memcpy(r.erased, hd.erased, (size_t)E);
  int n1 = 0, n2 = 0;
  for (int e = 0; e < E; ++e) n1 += hd.excluded[e], n2 += hd.erased[e];
  r.n_excluded = n1, r.n_erased = n2;
  r.iterations[0] = hd.ctl->its[0], r.iterations[1] = hd.ctl->its[1], r.n_trials = hd.ctl->n_trials, r.n_syncs = syncs + 1;
  return UVO_OK;
}

int uvo_nav_bundle_adjuster_trace(uvo_nav_bundle_adjuster* a, uvo_nav_ba_trace* out) {
  if (!a || !out) return fail(UVO_E_BADARG, "null pointer");
  if (!a->ran) return fail(UVO_E_BADARG, "the adjuster has not optimised anything yet");
  if (a->last_empty) return std::memset(out, 0, sizeof *out), UVO_OK;
  UVO_HIP_CHECK(hipSetDevice(a->m->device));
  UVO_HIP_CHECK(hipMemcpy(out, a->W.trace, sizeof(navba::Trace), hipMemcpyDeviceToHost));
  const int nl = out->n_lin < navba::kMaxLin ? out->n_lin : navba::kMaxLin, nt = out->n_trials < navba::kMaxTrialRecs ? out->n_trials : navba::kMaxTrialRecs;
  std::memset(out->lin + nl, 0, sizeof(uvo_nav_ba_trace_lin) * (size_t)(navba::kMaxLin - nl));
  std::memset(out->trial + nt, 0, sizeof(uvo_pose_trace_trial) * (size_t)(navba::kMaxTrialRecs - nt));
  return UVO_OK;
}

}  // extern "C"
