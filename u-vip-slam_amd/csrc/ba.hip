// Optimizer::LocalBundleAdjustment (src/Optimizer.cc:2147-2405) and Optimizer::BundleAdjustment (:1896-2010) as one call.  All arithmetic,
// the phases and their launch sequence are ba_core.hpp, shared with the host build tests/emu/ba_emu.cpp; this file is the device's Team
// -- which lane takes which entry; how the 256 lane sums meet is lane_team.hpp's LaneTeam -- one kernel per phase, and the host side of
// the C ABI.
//
// A phase is one launch with one workgroup of 256 lanes per block; the launches of a call follow each other in the matcher's stream.
// No kernel waits for another workgroup: what a phase needs of an earlier one is in global memory when it starts.  The Levenberg
// decision is taken by k_ba_lin_ctl and k_ba_trial_ctl (one workgroup) and left as a status word, which the host reads through
// page-locked memory after a stream synchronise to choose the next launches: one read per trial and one per optimize(), at most
// 2 + 15 x 10 a call in local mode.  A HIP error ends the call at once.  The reduction is lane_team.hpp's.
#include <cstring>
#include <vector>

#include "ba.hpp"
#include "devmem.hpp"
#include "matcher_priv.hpp"

namespace uvo {
namespace {

struct BaTeam : LaneTeam<ba::kSchurSums> {
  double* v;  // LDS [2][6 * kMaxFree]
  __device__ __forceinline__ double* vec() const { return v; }
  // the maximum over the lanes, through the reduction's words and its barrier
  template <class F>
  __device__ __forceinline__ double maxr(F f) {
    double m = f((int)threadIdx.x);
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) m = ba::max_nan(m, __shfl_xor(m, k));
    double* buf = red + phase * 4 * ba::kSchurSums;
    phase ^= 1;
    if ((threadIdx.x & 63) == 0) buf[wave_in_block()] = m;
    __syncthreads();
    return ba::max_nan(ba::max_nan(buf[0], buf[1]), ba::max_nan(buf[2], buf[3]));
  }
  // items 0..n-1 over the lanes, then a barrier: what the lanes wrote, to LDS or to global memory, is there for the whole workgroup
  template <class F>
  __device__ __forceinline__ void par(int n, F f) {
    for (int i = (int)threadIdx.x; i < n; i += ba::kLanes) f(i);
    __syncthreads();
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

#define UVO_BA_KERNEL(name, ph)                                              \
  __global__ __launch_bounds__(256) void name(ba::Ws W) {                    \
    __shared__ double s_red[2 * 4 * ba::kSchurSums];                         \
    __shared__ double s_store[ba::kSchurSums];                               \
    __shared__ double s_vec[2 * 6 * ba::kMaxFree];                           \
    __shared__ int32_t s_redi[2 * 4];                                        \
    BaTeam T = {{s_red, s_redi, s_store, 0}, s_vec};                         \
    ba::run_phase<ba::kMutNone>(ph, W, T, (int)blockIdx.x);                  \
  }

UVO_BA_KERNEL(k_ba_init, ba::kInit)
UVO_BA_KERNEL(k_ba_begin, ba::kBegin)
UVO_BA_KERNEL(k_ba_edge_lin, ba::kEdgeLin)
UVO_BA_KERNEL(k_ba_point_sum, ba::kPointSum)
UVO_BA_KERNEL(k_ba_kf_sum, ba::kKfSum)
UVO_BA_KERNEL(k_ba_lin_ctl, ba::kLinCtl)
UVO_BA_KERNEL(k_ba_dinv, ba::kDinv)
UVO_BA_KERNEL(k_ba_schur, ba::kSchur)
UVO_BA_KERNEL(k_ba_solve, ba::kSolve)
UVO_BA_KERNEL(k_ba_step, ba::kStep)
UVO_BA_KERNEL(k_ba_edge_err, ba::kEdgeErr)
UVO_BA_KERNEL(k_ba_trial_ctl, ba::kTrialCtl)
UVO_BA_KERNEL(k_ba_check, ba::kCheck)
UVO_BA_KERNEL(k_ba_finish, ba::kFinish)

}  // namespace uvo

// ---------------------------------------------------------------------------------------------------------------------------
using namespace uvo;

static_assert(sizeof(uvo_ba_trace) == sizeof(ba::Trace) && sizeof(uvo_ba_trace_lin) == sizeof(ba::TraceLin), "uvo_ba_trace is ba::Trace");

struct uvo_bundle_adjuster {
  uvo_matcher* m = nullptr;
  int max_free = 0, max_fixed = 0, max_points = 0, max_edges = 0;
  bool ran = false, last_empty = false;  // last_empty: the last call optimised nothing, its trace has no record
  DevMem mem;     // owns the device block and the page-locked mirrors of its two exchanges
  ba::Ws W;       // the device's arrays
  BaUpload d_up, h_up;
  BaDownload d_down, h_down;
  int32_t* h_status = nullptr;
};

namespace {

struct DevExec {
  uvo_bundle_adjuster* a;
  int launch(int ph, int blocks) {
    if (blocks <= 0) return UVO_OK;
    static const struct {
      void (*fn)(ba::Ws);
      const char* name;
    } k[ba::kPhases] = {{k_ba_init, "k_ba_init"},       {k_ba_begin, "k_ba_begin"},       {k_ba_edge_lin, "k_ba_edge_lin"}, {k_ba_point_sum, "k_ba_point_sum"},
                        {k_ba_kf_sum, "k_ba_kf_sum"},   {k_ba_lin_ctl, "k_ba_lin_ctl"},   {k_ba_dinv, "k_ba_dinv"},         {k_ba_schur, "k_ba_schur"},
                        {k_ba_solve, "k_ba_solve"},     {k_ba_step, "k_ba_step"},         {k_ba_edge_err, "k_ba_edge_err"}, {k_ba_trial_ctl, "k_ba_trial_ctl"},
                        {k_ba_check, "k_ba_check"},     {k_ba_finish, "k_ba_finish"}};
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

void layout_upload(Carve& c, BaUpload& u, size_t K, size_t F, size_t P, size_t E) {
  c.take(u.kf_T, 12 * K).take(u.kf_free, K).take(u.free_kf, F).take(u.pts, 3 * P).take(u.pt_bad, P).take(u.pt_begin, P + 1);
  c.take(u.e_kf, E).take(u.e_pt, E).take(u.e_cam, E).take(u.e_obs, 3 * E).take(u.cams, 4 * (size_t)ba::kMaxCams);
  c.take(u.kl_begin, F + 1).take(u.kl_edge, E).take(u.fp_edge, F * P);
}

void layout_download(Carve& c, BaDownload& d, size_t K, size_t P, size_t E) {
  c.take(d.kf_est, 7 * K).take(d.kf_T_out, 16 * K).take(d.pt_est, 3 * P).take(d.pt_out, 3 * P).take(d.removed1, E).take(d.removed2, E).take(d.ctl, 1);
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
  for (int i = 0; i < 3 * q.n_points; ++i) {
    if (r.point_estimate) r.point_estimate[i] = (double)q.points[i];
    if (r.points) r.points[i] = q.points[i];
  }
  if (r.removed1 && q.n_edges > 0) std::memset(r.removed1, 0, (size_t)q.n_edges);
  if (r.removed2 && q.n_edges > 0) std::memset(r.removed2, 0, (size_t)q.n_edges);
  r.n_removed1 = r.n_removed2 = 0, r.iterations[0] = r.iterations[1] = 0, r.n_trials = 0, r.n_syncs = 0;
}

}  // namespace

extern "C" {

void uvo_bundle_adjuster_destroy(uvo_bundle_adjuster* a) {
  if (!a) return;
  hipSetDevice(a->m->device);
  if (a->m->stream) hipStreamSynchronize(a->m->stream);
  a->mem.release_all();
  delete a;
}

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
    layout_upload(c, a->d_up, K, F, P, E);
    c.take(W.pose, K).take(W.pose_try, K).take(W.X, 3 * P).take(W.X_try, 3 * P).take(W.e_off, E).take(W.e_chi2, E).take(W.e_lin, E * ba::kEdgeWords);
    c.take(W.Hll, 9 * P).take(W.Dinv, 9 * P).take(W.p_on, P).take(W.Hpp, 27 * F).take(W.f_on, F).take(W.Hs, N * N).take(W.bs, N).take(W.xp, N).take(W.xl, 3 * P);
    c.take(W.chunk_chi2, ce).take(W.chunk_scale, cp).take(W.chunk_max, cp + F).take(W.chunk_n, ce).take(W.trace, 1);
    layout_download(c, a->d_down, K, P, E);
  });
  if (!rc) rc = alloc_carved(a->mem, [&](Carve& c) { layout_upload(c, a->h_up, K, F, P, E); }, true);
  if (!rc) rc = alloc_carved(a->mem, [&](Carve& c) { layout_download(c, a->h_down, K, P, E), c.take(a->h_status, 1); }, true);
  if (rc) return uvo_bundle_adjuster_destroy(a), rc;
  const BaUpload& u = a->d_up;
  W.kf_T = u.kf_T, W.kf_free = u.kf_free, W.free_kf = u.free_kf, W.pts = u.pts, W.pt_bad = u.pt_bad, W.pt_begin = u.pt_begin, W.e_kf = u.e_kf, W.e_pt = u.e_pt;
  W.e_cam = u.e_cam, W.e_obs = u.e_obs, W.cams = u.cams, W.kl_begin = u.kl_begin, W.kl_edge = u.kl_edge, W.fp_edge = u.fp_edge;
  const BaDownload& d = a->d_down;
  W.kf_est = d.kf_est, W.kf_T_out = d.kf_T_out, W.pt_est = d.pt_est, W.pt_out = d.pt_out, W.removed1 = d.removed1, W.removed2 = d.removed2, W.ctl = d.ctl;
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
  BaUpload& h = a->h_up;
  int F = 0;
  if (ba::derive(K, q.kf_fixed, P, q.point_edge_begin, E, q.edge_kf, q.edge_camera, q.n_cameras, h.kf_free, h.free_kf, &F, h.e_pt, h.kl_begin, h.kl_edge, h.fp_edge))
    return fail(UVO_E_BADARG, "bundle adjustment: an edge names a key frame or camera out of range, or the edge lists are not well formed");
  if (F == 0 || E == 0) return a->ran = a->last_empty = true, answer_unchanged(q, *result), UVO_OK;
  std::memcpy(h.kf_T, q.kf_Tcw, sizeof(float) * 12 * (size_t)K);
  std::memcpy(h.pts, q.points, sizeof(float) * 3 * (size_t)P);
  if (q.point_bad) std::memcpy(h.pt_bad, q.point_bad, (size_t)P);
  else std::memset(h.pt_bad, 0, (size_t)P);
  std::memcpy(h.pt_begin, q.point_edge_begin, sizeof(int32_t) * ((size_t)P + 1));
  std::memcpy(h.e_kf, q.edge_kf, sizeof(int32_t) * (size_t)E);
  std::memcpy(h.e_cam, q.edge_camera, sizeof(int32_t) * (size_t)E);
  for (int e = 0; e < E; ++e) h.e_obs[3 * e] = q.edge_obs[2 * e], h.e_obs[3 * e + 1] = q.edge_obs[2 * e + 1], h.e_obs[3 * e + 2] = q.edge_inv_sigma2[e];
  std::memcpy(h.cams, q.cameras, sizeof(float) * 4 * (size_t)q.n_cameras);

  uvo_matcher* m = a->m;
  UVO_HIP_CHECK(hipSetDevice(m->device));
  hipStream_t st = m->stream;
  const BaUpload& d = a->d_up;
#define UVO_BA_UP(field, count) UVO_HIP_CHECK(hipMemcpyAsync(d.field, h.field, sizeof(*h.field) * (size_t)(count), hipMemcpyHostToDevice, st))
  UVO_BA_UP(kf_T, 12 * K);
  UVO_BA_UP(kf_free, K);
  UVO_BA_UP(free_kf, F);
  UVO_BA_UP(pts, 3 * P);
  UVO_BA_UP(pt_bad, P);
  UVO_BA_UP(pt_begin, P + 1);
  UVO_BA_UP(e_kf, E);
  UVO_BA_UP(e_pt, E);
  UVO_BA_UP(e_cam, E);
  UVO_BA_UP(e_obs, 3 * (size_t)E);
  UVO_BA_UP(cams, 4 * q.n_cameras);
  UVO_BA_UP(kl_begin, F + 1);
  UVO_BA_UP(kl_edge, E);
  UVO_BA_UP(fp_edge, (size_t)F * (size_t)P);
#undef UVO_BA_UP
  ba::Ws& W = a->W;
  W.K = K, W.F = F, W.P = P, W.E = E, W.C = q.n_cameras;
  DevExec x = {a};
  int syncs = 0;
  const ba::Dims dims = {K, F, P, E};
  RC(ba::drive(x, dims, q.mode == UVO_BA_LOCAL ? ba::kModeLocal : ba::kModeFull, q.n_iterations, &syncs));
  const BaDownload &dd = a->d_down, &hd = a->h_down;
#define UVO_BA_DOWN(field, count) UVO_HIP_CHECK(hipMemcpyAsync(hd.field, dd.field, sizeof(*hd.field) * (size_t)(count), hipMemcpyDeviceToHost, st))
  UVO_BA_DOWN(kf_est, 7 * K);
  UVO_BA_DOWN(kf_T_out, 16 * K);
  UVO_BA_DOWN(pt_est, 3 * (size_t)P);
  UVO_BA_DOWN(pt_out, 3 * (size_t)P);
  UVO_BA_DOWN(removed1, E);
  UVO_BA_DOWN(removed2, E);
  UVO_BA_DOWN(ctl, 1);
#undef UVO_BA_DOWN
  UVO_HIP_CHECK(hipStreamSynchronize(st));
  a->ran = true, a->last_empty = false;
  uvo_ba_result& r = *result;
  if (r.kf_estimate) std::memcpy(r.kf_estimate, hd.kf_est, sizeof(double) * 7 * (size_t)K);
  if (r.kf_Tcw) std::memcpy(r.kf_Tcw, hd.kf_T_out, sizeof(float) * 16 * (size_t)K);
  if (r.point_estimate) std::memcpy(r.point_estimate, hd.pt_est, sizeof(double) * 3 * (size_t)P);
  if (r.points) std::memcpy(r.points, hd.pt_out, sizeof(float) * 3 * (size_t)P);
  if (r.removed1) std::memcpy(r.removed1, hd.removed1, (size_t)E);
  if (r.removed2) std::memcpy(r.removed2, hd.removed2, (size_t)E);
  int n1 = 0, n2 = 0;
  for (int e = 0; e < E; ++e) n1 += hd.removed1[e], n2 += hd.removed2[e];
  r.n_removed1 = n1, r.n_removed2 = n2;
  r.iterations[0] = hd.ctl->its[0], r.iterations[1] = hd.ctl->its[1], r.n_trials = hd.ctl->n_trials, r.n_syncs = syncs + 1;
  return UVO_OK;
}

int uvo_bundle_adjuster_trace(uvo_bundle_adjuster* a, uvo_ba_trace* out) {
  if (!a || !out) return fail(UVO_E_BADARG, "null pointer");
  if (!a->ran) return fail(UVO_E_BADARG, "the adjuster has not optimised anything yet");
  if (a->last_empty) return std::memset(out, 0, sizeof *out), UVO_OK;
  UVO_HIP_CHECK(hipSetDevice(a->m->device));
  UVO_HIP_CHECK(hipMemcpy(out, a->W.trace, sizeof(ba::Trace), hipMemcpyDeviceToHost));
  // records beyond the counts are whatever an earlier call left: not part of the answer
  const int nl = out->n_lin < ba::kMaxLin ? out->n_lin : ba::kMaxLin, nt = out->n_trials < ba::kMaxTrialRecs ? out->n_trials : ba::kMaxTrialRecs;
  std::memset(out->lin + nl, 0, sizeof(uvo_ba_trace_lin) * (size_t)(ba::kMaxLin - nl));
  std::memset(out->trial + nt, 0, sizeof(uvo_pose_trace_trial) * (size_t)(ba::kMaxTrialRecs - nt));
  return UVO_OK;
}

}  // extern "C"
