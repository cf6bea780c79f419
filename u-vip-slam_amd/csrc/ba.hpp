// The bundle adjusters (ba.hip, navba.hip; arithmetic and launch sequences in ba_core.hpp and navba_core.hpp): what their kernels and
// host sides share, stated once.  The device's team, the kernel of a phase, the executor drive() launches through, and the host
// exchange of the observation graph -- the thirteen arrays that both problems carry -- with the shared part of the answer.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>

#include "ba_core.hpp"
#include "devmem.hpp"
#include "matcher_priv.hpp"

namespace uvo {

static_assert(sizeof(ba::TraceLin) == 40 && sizeof(ba::Ctl) == 80, "ba::TraceLin is 40 bytes, ba::Ctl 80");

// ---- the device's team: which lane takes which entry; how the 256 lane sums meet is lane_team.hpp's LaneTeam ---------------------------
struct BaTeam : LaneTeam<ba::kSchurSums> {
  double* v;  // LDS, the solve's two vectors: [2][6 * ba::kMaxFree] or [2][15 * navba::kMaxFree]
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
  template <class F>
  __device__ __forceinline__ void each(int n, F f) {  // navopt_core.hpp's name for par
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

// one phase of core `ns` as a kernel: one workgroup of 256 lanes per block; vec_words: the LDS words of the solve's two vectors
#define UVO_BA_KERNEL(ns, vec_words, name, ph)                               \
  __global__ __launch_bounds__(256) void name(ns::Ws W) {                    \
    __shared__ double s_red[2 * 4 * ba::kSchurSums];                         \
    __shared__ double s_store[ba::kSchurSums];                               \
    __shared__ double s_vec[vec_words];                                      \
    __shared__ int32_t s_redi[2 * 4];                                        \
    BaTeam T = {{s_red, s_redi, s_store, 0}, s_vec};                         \
    ns::run_phase<ns::kMutNone>(ph, W, T, (int)blockIdx.x);                  \
  }

// ---- drive()'s executor on the device ---------------------------------------------------------------------------------------------------
template <class WS>
struct BaPhaseKernel {
  void (*fn)(WS);
  const char* name;  // under which the matcher's profiler lists it
};

// launch queues a phase in the stream; status waits for what is queued and reads the status word through page-locked memory
template <class WS>
struct BaExec {
  hipStream_t st;
  Profiler* prof;
  const WS* W;
  int32_t* h_status;
  const BaPhaseKernel<WS>* k;  // [the core's kPhases]
  int launch(int ph, int blocks) {
    if (blocks <= 0) return UVO_OK;
    {
      Profiler::Scope ps(prof, k[ph].name, st);
      hipLaunchKernelGGL(k[ph].fn, dim3(blocks), dim3(256), 0, st, *W);
    }
    UVO_HIP_CHECK(hipGetLastError());
    return UVO_OK;
  }
  int status(int* out) {
    UVO_HIP_CHECK(hipMemcpyAsync(h_status, &W->ctl->status, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    UVO_HIP_CHECK(hipStreamSynchronize(st));
    *out = *h_status;
    return UVO_OK;
  }
};

// ---- the host exchange ------------------------------------------------------------------------------------------------------------------
#define UVO_BA_COPY(dst, src, field, count, kind) \
  if ((size_t)(count) > 0) UVO_HIP_CHECK(hipMemcpyAsync((dst).field, (src).field, sizeof(*(src).field) * (size_t)(count), kind, st))

// The observation graph as the host writes it per call: ba::Ws's and navba::Ws's fields of these names.  One description places the
// arrays on the device and in the page-locked mirror, fills the mirror from a problem (Q: uvo_ba_problem or uvo_nav_ba_problem, which
// name these lists alike) and copies it up.
struct BaGraph {
  int32_t *kf_free, *free_kf;
  float* pts;
  uint8_t* pt_bad;
  int32_t *pt_begin, *e_kf, *e_pt, *e_cam;
  float *e_obs, *cams;
  int32_t *kl_begin, *kl_edge, *fp_edge;

  void layout(Carve& c, size_t K, size_t F, size_t P, size_t E) {
    c.take(kf_free, K).take(free_kf, F).take(pts, 3 * P).take(pt_bad, P).take(pt_begin, P + 1);
    c.take(e_kf, E).take(e_pt, E).take(e_cam, E).take(e_obs, 3 * E).take(cams, 4 * (size_t)ba::kMaxCams);
    c.take(kl_begin, F + 1).take(kl_edge, E).take(fp_edge, F * P);
  }
  template <class WS>
  void bind(WS& W) const {
    W.kf_free = kf_free, W.free_kf = free_kf, W.pts = pts, W.pt_bad = pt_bad, W.pt_begin = pt_begin, W.e_kf = e_kf, W.e_pt = e_pt, W.e_cam = e_cam;
    W.e_obs = e_obs, W.cams = cams, W.kl_begin = kl_begin, W.kl_edge = kl_edge, W.fp_edge = fp_edge;
  }
  // what ba::derive works out of the problem's lists: kf_free, free_kf and their count, e_pt, kl_begin, kl_edge, fp_edge.  0, or 1: see there
  template <class Q>
  int derive(const Q& q, int* F) {
    return ba::derive(q.n_keyframes, q.kf_fixed, q.n_points, q.point_edge_begin, q.n_edges, q.edge_kf, q.edge_camera, q.n_cameras, kf_free, free_kf, F, e_pt, kl_begin,
                      kl_edge, fp_edge);
  }
  // the arrays that are the caller's own: copied, the observation and its inverse variance put side by side
  template <class Q>
  void pack(const Q& q) {
    const size_t P = (size_t)q.n_points, E = (size_t)q.n_edges;
    if (P > 0) std::memcpy(pts, q.points, sizeof(float) * 3 * P);
    if (q.point_bad && P > 0) std::memcpy(pt_bad, q.point_bad, P);
    else if (P > 0) std::memset(pt_bad, 0, P);
    std::memcpy(pt_begin, q.point_edge_begin, sizeof(int32_t) * (P + 1));
    if (E == 0) return;
    std::memcpy(e_kf, q.edge_kf, sizeof(int32_t) * E);
    std::memcpy(e_cam, q.edge_camera, sizeof(int32_t) * E);
    for (size_t e = 0; e < E; ++e) e_obs[3 * e] = q.edge_obs[2 * e], e_obs[3 * e + 1] = q.edge_obs[2 * e + 1], e_obs[3 * e + 2] = q.edge_inv_sigma2[e];
    std::memcpy(cams, q.cameras, sizeof(float) * 4 * (size_t)q.n_cameras);
  }
  // the mirror (this) to the device: one copy per array that is not empty
  int send(const BaGraph& dev, int K, int F, int P, int E, int C, hipStream_t st) const {
    UVO_BA_COPY(dev, *this, kf_free, K, hipMemcpyHostToDevice);
    UVO_BA_COPY(dev, *this, free_kf, F, hipMemcpyHostToDevice);
    UVO_BA_COPY(dev, *this, pts, 3 * P, hipMemcpyHostToDevice);
    UVO_BA_COPY(dev, *this, pt_bad, P, hipMemcpyHostToDevice);
    UVO_BA_COPY(dev, *this, pt_begin, P + 1, hipMemcpyHostToDevice);
    UVO_BA_COPY(dev, *this, e_kf, E, hipMemcpyHostToDevice);
    UVO_BA_COPY(dev, *this, e_pt, E, hipMemcpyHostToDevice);
    UVO_BA_COPY(dev, *this, e_cam, E, hipMemcpyHostToDevice);
    UVO_BA_COPY(dev, *this, e_obs, 3 * (size_t)E, hipMemcpyHostToDevice);
    UVO_BA_COPY(dev, *this, cams, 4 * C, hipMemcpyHostToDevice);
    UVO_BA_COPY(dev, *this, kl_begin, F + 1, hipMemcpyHostToDevice);
    UVO_BA_COPY(dev, *this, kl_edge, E, hipMemcpyHostToDevice);
    UVO_BA_COPY(dev, *this, fp_edge, (size_t)F * (size_t)P, hipMemcpyHostToDevice);
    return UVO_OK;
  }
};

// Where a result's shared fields are: the C ABI's two result structs name their masks and counts differently
struct BaResultFields {
  float* kf_Tcw;
  double* point_estimate;
  float* points;
  uint8_t *mask1, *mask2;
  int32_t *n_mask1, *n_mask2, *iterations, *n_trials, *n_syncs;
};

// What both calls bring down besides the key frames' estimates (which stand in front of it, device and mirror): the float poses, the
// points in double and in float, the masks of the two checks, the control block
struct BaAnswer {
  float* kf_T_out;
  double* pt_est;
  float* pt_out;
  uint8_t *mask1, *mask2;
  ba::Ctl* ctl;

  void layout(Carve& c, size_t K, size_t P, size_t E) { c.take(kf_T_out, 16 * K).take(pt_est, 3 * P).take(pt_out, 3 * P).take(mask1, E).take(mask2, E).take(ctl, 1); }
  // the device's (dev) to the mirror (this); the caller synchronises
  int receive(const BaAnswer& dev, int K, int P, int E, hipStream_t st) const {
    UVO_BA_COPY(*this, dev, kf_T_out, 16 * K, hipMemcpyDeviceToHost);
    UVO_BA_COPY(*this, dev, pt_est, 3 * (size_t)P, hipMemcpyDeviceToHost);
    UVO_BA_COPY(*this, dev, pt_out, 3 * (size_t)P, hipMemcpyDeviceToHost);
    UVO_BA_COPY(*this, dev, mask1, E, hipMemcpyDeviceToHost);
    UVO_BA_COPY(*this, dev, mask2, E, hipMemcpyDeviceToHost);
    UVO_BA_COPY(*this, dev, ctl, 1, hipMemcpyDeviceToHost);
    return UVO_OK;
  }
  // the mirror into the caller's result, after the synchronise; syncs: drive()'s status reads
  void store(const BaResultFields& r, int K, int P, int E, int syncs) const {
    if (r.kf_Tcw) std::memcpy(r.kf_Tcw, kf_T_out, sizeof(float) * 16 * (size_t)K);
    if (r.point_estimate && P > 0) std::memcpy(r.point_estimate, pt_est, sizeof(double) * 3 * (size_t)P);
    if (r.points && P > 0) std::memcpy(r.points, pt_out, sizeof(float) * 3 * (size_t)P);
    if (r.mask1 && E > 0) std::memcpy(r.mask1, mask1, (size_t)E);
    if (r.mask2 && E > 0) std::memcpy(r.mask2, mask2, (size_t)E);
    int n1 = 0, n2 = 0;
    for (int e = 0; e < E; ++e) n1 += mask1[e], n2 += mask2[e];
    *r.n_mask1 = n1, *r.n_mask2 = n2;
    r.iterations[0] = ctl->its[0], r.iterations[1] = ctl->its[1], *r.n_trials = ctl->n_trials, *r.n_syncs = syncs + 1;
  }
};

// the shared part of the answer when nothing is optimised: the points' conversions, empty masks, no iteration
template <class Q>
void ba_answer_unchanged(const Q& q, const BaResultFields& r) {
  for (int i = 0; i < 3 * q.n_points; ++i) {
    if (r.point_estimate) r.point_estimate[i] = (double)q.points[i];
    if (r.points) r.points[i] = q.points[i];
  }
  if (r.mask1 && q.n_edges > 0) std::memset(r.mask1, 0, (size_t)q.n_edges);
  if (r.mask2 && q.n_edges > 0) std::memset(r.mask2, 0, (size_t)q.n_edges);
  *r.n_mask1 = *r.n_mask2 = 0, r.iterations[0] = r.iterations[1] = 0, *r.n_trials = 0, *r.n_syncs = 0;
}

// ---- a handle's life: A is uvo_bundle_adjuster or uvo_nav_bundle_adjuster --------------------------------------------------------------
// what both handles hold besides their capacities and their workspace
struct BaHandle {
  uvo_matcher* m = nullptr;
  bool ran = false, last_empty = false;  // last_empty: the last call optimised nothing, its trace has no record
  DevMem mem;  // owns the device block and the page-locked mirrors of its two exchanges
  BaGraph d_graph, h_graph;
  BaAnswer d_ans, h_ans;
  int32_t* h_status = nullptr;
};

template <class A>
void ba_destroy(A* a) {
  if (!a) return;
  hipSetDevice(a->m->device);
  if (a->m->stream) hipStreamSynchronize(a->m->stream);
  a->mem.release_all();
  delete a;
}

// CTrace: the C ABI's struct of ba::Trace's layout (the caller asserts the sizes)
template <class A, class CTrace>
int ba_read_trace(A* a, CTrace* out) {
  if (!a || !out) return fail(UVO_E_BADARG, "null pointer");
  if (!a->ran) return fail(UVO_E_BADARG, "the adjuster has not optimised anything yet");
  if (a->last_empty) return std::memset(out, 0, sizeof *out), UVO_OK;
  UVO_HIP_CHECK(hipSetDevice(a->m->device));
  UVO_HIP_CHECK(hipMemcpy(out, a->W.trace, sizeof(ba::Trace), hipMemcpyDeviceToHost));
  // records beyond the counts are whatever an earlier call left: not part of the answer
  const int nl = out->n_lin < ba::kMaxLin ? out->n_lin : ba::kMaxLin, nt = out->n_trials < ba::kMaxTrialRecs ? out->n_trials : ba::kMaxTrialRecs;
  std::memset(out->lin + nl, 0, sizeof out->lin[0] * (size_t)(ba::kMaxLin - nl));
  std::memset(out->trial + nt, 0, sizeof out->trial[0] * (size_t)(ba::kMaxTrialRecs - nt));
  return UVO_OK;
}

#undef UVO_BA_COPY

}  // namespace uvo
