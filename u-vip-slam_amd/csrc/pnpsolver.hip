// USLAM::PnPsolver for Tracking::Relocalisation (src/Tracking.cc:2415-2517, src/PnPsolver.cc): iterate(n) over a LIST of solvers as one
// call.  All arithmetic is pnpsolver_core.hpp / epnp_core.hpp, shared with the host build tests/emu/pnpsolver_emu.cpp; this file
// decides which lane computes which scalar.  What makes it one call: the iterations a solver runs unless it returns are known before
// anything is evaluated (max(max_its - mnIterations, n_iterations), the loop condition being an OR), so the host draws every subset of
// the call from the caller's generator state up front, and the stream position of each solver is a prefix sum.  That host side -- the
// set, the exchange, iterate's walk -- is solver_set.hpp, shared with sim3solver.hip; below the kernels stands what is the PnPsolver's.
//
// Three launches in the uvo_klt handle's stream, all scratch sized at uvo_pnpsolver_set_create:
//   k_pnps_hypotheses : EPnP on min_set points, one lane per (solver, hypothesis), eight lanes per workgroup with their 589-double
//                       workspaces interleaved in LDS -- the lane shape of k_pnp_hypotheses (pnp.hip), but the grid now holds every
//                       listed solver's hypotheses: 8 candidates x 35 fill 35 workgroups instead of 5 per call.
//   k_pnps_score      : one workgroup per (solver, hypothesis): CheckInliers over the solver's points, the inlier set as 64-bit
//                       ballot words (one ordinary store per wavefront and word), the count.
//   k_pnps_finish     : one workgroup per listed solver replays iterate() over the counts (pnps::replay; every lane runs the same
//                       scalar control flow).  Where the best set changes and Refine() is consulted, the 256 lanes compact the set,
//                       share pnp::solve's phases scalar by scalar, and score the refined pose.  It writes the result record and
//                       the refined or best set.  The best set and pose are double-buffered per solver: the kernel reads one copy
//                       and writes the other, and the host adopts the new copy only for solvers the replay actually reached --
//                       a solver behind the returning one stays untouched although its hypotheses were evaluated.
#include <cmath>
#include <cstring>
#include <vector>

#include "pnpsolver.hpp"
#include "solver_set.hpp"

namespace uvo {

constexpr int kPnpsHypLanes = 8;

struct PnpsSync {
  __device__ void operator()() const { __syncthreads(); }
};

// the device block of a set, by value to every kernel
struct PnpsDev {
  int32_t max_points, words;  // per solver; words = ceil(max_points / 64)
  const float* p3d;           // [S][max_points][3]
  const float* p2d;           // [S][max_points][2]
  const float* max_err;       // [S][max_points]  sigma2 * th2 in float
  uint64_t* best_mask;        // [S][2][words]
  double* best_pose;          // [S][2][12]
  const PnpsCall* call;       // [S]
  const int32_t* hyp;         // [T][kPnpsSubsetStride]
  double* poses;              // [T][12]
  int32_t* counts;            // [T]
  uint64_t* masks;            // [T][words]
  int32_t* list;              // [S][max_points]  Refine()'s indices
  PnpsResult* result;         // [S]
  uint64_t* out_mask;         // [S][words], indexed by the position in the call's list
};

__global__ __launch_bounds__(kPnpsHypLanes) void k_pnps_hypotheses(PnpsDev D, int total) {
  __shared__ double s_ws[pnp::W_SIZE * kPnpsHypLanes];
  const int g = blockIdx.x * kPnpsHypLanes + threadIdx.x;
  if (g >= total) return;
  const int32_t* rec = D.hyp + (size_t)g * kPnpsSubsetStride;
  const PnpsCall& c = D.call[rec[0]];
  const pnp::Ws<kPnpsHypLanes> W{s_ws + threadIdx.x};
  const pnp::PixelPoints P{D.p3d + (size_t)c.id * D.max_points * 3, D.p2d + (size_t)c.id * D.max_points * 2, rec + 1, c.min_set, c.fu, c.fv, c.uc, c.vc};
  double* out = D.poses + (size_t)g * 12;
  for (int e = 0; e < 12; ++e) out[e] = 0.;
  const bool ok = pnp::solve(W, P, 0, 1, pnp::NoSync(), out);
  D.counts[g] = ok ? 0 : -1;
}

// CheckInliers of `pose` over the solver's n points by the 256 lanes: mask words to `words_out`, returns the count on every lane
__device__ int pnps_check_inliers(const PnpsDev& D, const PnpsCall& c, const double* pose, uint64_t* words_out, int32_t* s_wcnt) {
  const int lane = threadIdx.x & 63, wave = wave_in_block();
  const float* p3d = D.p3d + (size_t)c.id * D.max_points * 3;
  const float* p2d = D.p2d + (size_t)c.id * D.max_points * 2;
  const float* me = D.max_err + (size_t)c.id * D.max_points;
  int cnt = 0;
  for (int w = wave; w * 64 < c.n; w += 4) {
    const int i = w * 64 + lane;
    const bool inl = i < c.n && pnps::check_inlier(pose, pose + 9, p3d + 3 * i, p2d + 2 * i, c.fu, c.fv, c.uc, c.vc, me[i]);
    const uint64_t m = __ballot(inl);
    if (lane == 0) words_out[w] = m;
    cnt += __builtin_popcountll(m);
  }
  __syncthreads();  // s_wcnt may still be read from an earlier call
  if (lane == 0) s_wcnt[wave] = cnt;
  __syncthreads();
  return s_wcnt[0] + s_wcnt[1] + s_wcnt[2] + s_wcnt[3];
}

__global__ __launch_bounds__(256) void k_pnps_score(PnpsDev D) {
  __shared__ int32_t s_wcnt[4];
  const int g = blockIdx.x;
  const PnpsCall& c = D.call[D.hyp[(size_t)g * kPnpsSubsetStride]];
  uint64_t* words = D.masks + (size_t)g * D.words;
  if (D.counts[g] < 0) {  // no finite pose (uniform over the workgroup): zero inliers
    for (int w = threadIdx.x; w * 64 < c.n; w += 256) words[w] = 0;
    if (threadIdx.x == 0) D.counts[g] = 0;
    return;
  }
  const int cnt = pnps_check_inliers(D, c, D.poses + (size_t)g * 12, words, s_wcnt);
  if (threadIdx.x == 0) D.counts[g] = cnt;
}

// pnps::replay's operations with 256 cooperating lanes; every member is uniform over the workgroup
struct PnpsFinishOps {
  const PnpsDev& D;
  const PnpsCall& c;
  uint64_t* bm;   // the solver's new best set
  double* bp;     // and pose
  uint64_t* out;  // the refined set
  double* s_ws;
  double* s_pose;
  int32_t* s_pref;  // [257]
  int32_t* s_wcnt;  // [4]
  bool valid;
  int refined;

  __device__ void take_best(int h) {
    const size_t g = (size_t)(c.hyp_off + h);
    for (int w = threadIdx.x; w * 64 < c.n; w += 256) bm[w] = D.masks[g * D.words + w];
    if (threadIdx.x < 12) bp[threadIdx.x] = D.poses[g * 12 + threadIdx.x];
    valid = false;
    __syncthreads();
  }

  __device__ int refine() {
    if (valid) return refined;
    const int tid = threadIdx.x, nw = (c.n + 63) >> 6;
    __syncthreads();
    if (tid < nw) s_pref[tid + 1] = __builtin_popcountll(bm[tid]);
    __syncthreads();
    if (tid == 0) {
      s_pref[0] = 0;
      for (int w = 0; w < nw; ++w) s_pref[w + 1] += s_pref[w];
    }
    __syncthreads();
    int32_t* list = D.list + (size_t)c.id * D.max_points;
    for (int i = tid; i < c.n; i += 256) {  // Refine's vIndices: the best set in ascending order
      const uint64_t word = bm[i >> 6];
      if (word >> (i & 63) & 1) list[s_pref[i >> 6] + __builtin_popcountll(word & ((1ull << (i & 63)) - 1))] = i;
    }
    const int total = s_pref[nw];
    __syncthreads();
    const pnp::PixelPoints P{D.p3d + (size_t)c.id * D.max_points * 3, D.p2d + (size_t)c.id * D.max_points * 2, list, total, c.fu, c.fv, c.uc, c.vc};
    const bool ok = pnp::solve(pnp::Ws<1>{s_ws}, P, tid, 256, PnpsSync(), s_pose);
    __syncthreads();
    refined = ok ? pnps_check_inliers(D, c, s_pose, out, s_wcnt) : 0;
    valid = true;
    return refined;
  }
};

__global__ __launch_bounds__(256) void k_pnps_finish(PnpsDev D) {
  __shared__ double s_ws[pnp::W_SIZE];
  __shared__ double s_pose[12];
  __shared__ int32_t s_pref[257];
  __shared__ int32_t s_wcnt[4];
  const int slot = blockIdx.x, tid = threadIdx.x;
  const PnpsCall& c = D.call[slot];
  if (c.hyp_n == 0) return;  // fewer points than nMinInliers: the host answers bNoMore by itself
  const int nw = (c.n + 63) >> 6;
  uint64_t* bm_old = D.best_mask + ((size_t)c.id * 2 + c.parity) * D.words;
  uint64_t* bm = D.best_mask + ((size_t)c.id * 2 + (c.parity ^ 1)) * D.words;
  double* bp_old = D.best_pose + ((size_t)c.id * 2 + c.parity) * 12;
  double* bp = D.best_pose + ((size_t)c.id * 2 + (c.parity ^ 1)) * 12;
  uint64_t* out = D.out_mask + (size_t)slot * D.words;
  for (int w = tid; w < nw; w += 256) bm[w] = bm_old[w];
  if (tid < 12) bp[tid] = bp_old[tid], s_pose[tid] = 0.;
  __syncthreads();
  PnpsFinishOps ops{D, c, bm, bp, out, s_ws, s_pose, s_pref, s_wcnt, false, 0};
  pnps::State st = {c.iterations, c.best_count};
  const pnps::Outcome o = pnps::replay(st, D.counts + c.hyp_off, c.n_iterations, c.max_its, c.min_inliers, ops);
  __syncthreads();
  if (o.returned == pnps::kBestAtExhaustion)
    for (int w = tid; w < nw; w += 256) out[w] = bm[w];
  PnpsResult* r = D.result + slot;
  if (tid < 12) r->pose[tid] = o.returned == pnps::kRefined ? s_pose[tid] : o.returned == pnps::kBestAtExhaustion ? bp[tid] : 0.;
  if (tid == 0) r->performed = o.performed, r->returned = o.returned, r->no_more = o.no_more, r->inliers = o.inliers, r->best_count = st.best_count;
}

}  // namespace uvo

// ---------------------------------------------------------------------------------------------------------------------------
using namespace uvo;

namespace {
struct Solver : SetSolver {
  pnps::Params params;
  pnps::Derived d;
  double fu = 0, fv = 0, uc = 0, vc = 0;
  int parity = 0;
};
}  // namespace

struct uvo_pnpsolver_set : SolverSet<PnpsCall, PnpsResult> {
  uvo_klt* klt = nullptr;
  PnpsDev D;
  float *p3d = nullptr, *p2d = nullptr, *max_err = nullptr;  // writable views of D's
  std::vector<Solver> solvers;

  // what solver_set.hpp asks of a family
  static constexpr int kMaxSolvers = kPnpsMaxSolvers, kMinPoints = pnps::kMinSetLo, kMaxPoints = kPnpsMaxPoints, kHypPerSolver = kPnpsHypPerSolver;
  static constexpr int kSubsetStride = kPnpsSubsetStride;
  static constexpr const char* kRangeText = "PnPsolver set: 1..64 solvers of 4..16384 points";
  static constexpr const char* kNoMemText = "PnPsolver set allocation failed";
  static constexpr const char* kFullText = "the PnPsolver set is full";
  void arrays(Carve& c, bool scratch) {
    const size_t S = (size_t)max_solvers, N = (size_t)max_points, W = (size_t)words, T = (size_t)total;
    if (!scratch) c.take(p3d, S * N * 3).take(p2d, S * N * 2).take(max_err, S * N).take(D.best_mask, S * 2 * W).take(D.best_pose, S * 2 * 12);
    else c.take(D.poses, T * 12).take(D.counts, T).take(D.masks, T * W).take(D.list, S * N);
  }
  static int min_set(const Solver& v) { return v.params.min_set; }
  // the loop condition is an OR; with fewer points than nMinInliers: bNoMore at once, nothing drawn
  static int plan(const Solver& v, int n_iterations) { return v.n < v.d.min_inliers ? 0 : pnps::iterations_ahead(v.iterations, v.d.max_its, n_iterations); }
  static PnpsCall call(int id, const Solver& v, int off, int K, int n_iterations) {
    return PnpsCall{id, v.n, v.params.min_set, v.d.min_inliers, v.d.max_its, v.iterations, v.best_count, v.parity, off, K, n_iterations, 0, v.fu, v.fv, v.uc, v.vc};
  }
  void launch(int n_ids, int total) const {  // no profiler scope: a uvo_klt handle has no profiler
    hipLaunchKernelGGL(k_pnps_hypotheses, dim3((total + kPnpsHypLanes - 1) / kPnpsHypLanes), dim3(kPnpsHypLanes), 0, stream, D, total);
    hipLaunchKernelGGL(k_pnps_score, dim3(total), dim3(256), 0, stream, D);
    hipLaunchKernelGGL(k_pnps_finish, dim3(n_ids), dim3(256), 0, stream, D);
  }
  static int idle_no_more(const Solver&) { return 1; }
  static bool adopt(Solver& v, const PnpsResult& r, uvo_pnpsolver_result* result) {
    v.parity ^= 1;  // k_pnps_finish wrote the other copy of the best set and pose
    if (r.returned == pnps::kNone) return false;
    result->refined = r.returned == pnps::kRefined ? 1 : 0;
    float* T = result->Tcw;
    for (int a = 0; a < 3; ++a) {
      for (int b = 0; b < 3; ++b) T[4 * a + b] = (float)r.pose[3 * a + b];
      T[4 * a + 3] = (float)r.pose[9 + a];
    }
    T[15] = 1.f;
    return true;
  }
};

extern "C" {

void uvo_glibc_srand(uvo_glibc_rand* g, uint32_t seed) {
  static_assert(sizeof(uvo_glibc_rand) == sizeof(pnps::GlibcRand), "uvo_glibc_rand is pnps::GlibcRand");
  if (g) reinterpret_cast<pnps::GlibcRand*>(g)->srand(seed);
}

int32_t uvo_glibc_rand_next(uvo_glibc_rand* g) { return g ? reinterpret_cast<pnps::GlibcRand*>(g)->next() : 0; }

void uvo_pnpsolver_set_destroy(uvo_pnpsolver_set* s) { set_destroy(s); }

int uvo_pnpsolver_set_create(uvo_klt* k, int max_solvers, int max_points, uvo_pnpsolver_set** out) {
  if (!k || !out) return fail(UVO_E_BADARG, "null pointer");
  *out = nullptr;
  uvo_pnpsolver_set* s = nullptr;
  RC(set_create(klt_device(k), klt_stream(k), max_solvers, max_points, &s));
  s->klt = k;
  PnpsDev& D = s->D;
  D.max_points = max_points, D.words = s->words;
  D.p3d = s->p3d, D.p2d = s->p2d, D.max_err = s->max_err;
  D.call = s->d_call, D.hyp = s->d_sub, D.result = s->d_res, D.out_mask = s->d_om;
  *out = s;
  return UVO_OK;
}

int uvo_pnpsolver_set_clear(uvo_pnpsolver_set* s) { return set_clear(s); }

int uvo_pnpsolver_add(uvo_pnpsolver_set* s, const float* p3d, const float* p2d, const float* sigma2, const int32_t* kp_index, int n, int n_matches,
                      float fx, float fy, float cx, float cy, const uvo_pnpsolver_params* params, int* id) {
  RC(add_check(s, params && id, n, n_matches, p3d && p2d && sigma2 && kp_index));
  const uvo_pnpsolver_params& q = *params;
  if (!(q.probability > 0. && q.probability < 1.) || !(q.epsilon >= 0.f && q.epsilon <= 1.f) || !(q.th2 >= 0.f) || !(fx == fx) || !(fy == fy) ||
      !(cx == cx) || !(cy == cy))
    return fail(UVO_E_BADARG, "PnPsolver parameters: probability in (0,1), epsilon in [0,1], th2 >= 0, no NaN");
  if (q.min_set < pnps::kMinSetLo || q.min_set > pnps::kMinSetHi || q.max_iterations < 1 || q.min_inliers < 0)
    return fail(UVO_E_BADARG, "PnPsolver parameters: min_set 4..8, max_iterations >= 1, min_inliers >= 0");
  for (int i = 0; i < n; ++i)
    if (kp_index[i] < 0 || kp_index[i] >= n_matches) return fail(UVO_E_BADARG, "kp_index outside 0..n_matches-1");
  Solver v;
  v.n = n, v.n_matches = n_matches;
  v.params = pnps::Params{q.probability, q.min_inliers, q.max_iterations, q.min_set, q.epsilon, q.th2};
  v.d = n > 0 ? pnps::derive_params(n, v.params) : pnps::Derived{0, q.min_inliers > q.min_set ? q.min_inliers : q.min_set, 1};
  v.fu = fx, v.fv = fy, v.uc = cx, v.vc = cy;
  v.index.assign(kp_index, kp_index + n);
  if (n > 0) {
    UVO_HIP_CHECK(hipSetDevice(s->device));
    const size_t N = (size_t)s->max_points, sid = s->solvers.size();
    std::vector<float> me(n);
    for (int i = 0; i < n; ++i) me[i] = sigma2[i] * q.th2;  // mvMaxError, in float
    UVO_HIP_CHECK(hipMemcpyAsync(s->p3d + sid * N * 3, p3d, (size_t)n * 12, hipMemcpyHostToDevice, s->stream));
    UVO_HIP_CHECK(hipMemcpyAsync(s->p2d + sid * N * 2, p2d, (size_t)n * 8, hipMemcpyHostToDevice, s->stream));
    UVO_HIP_CHECK(hipMemcpyAsync(s->max_err + sid * N, me.data(), (size_t)n * 4, hipMemcpyHostToDevice, s->stream));
    UVO_HIP_CHECK(hipStreamSynchronize(s->stream));  // the sources are the caller's pageable memory and a local
  }
  return add_finish(s, v, id);
}

int uvo_pnpsolver_query(uvo_pnpsolver_set* s, int id, uvo_pnpsolver_info* info) {
  RC(solver_check(s, info != nullptr, id));
  const Solver& v = s->solvers[id];
  *info = uvo_pnpsolver_info{v.n, v.d.min_inliers, v.d.max_its, v.iterations, v.best_count};
  return UVO_OK;
}

int uvo_pnpsolver_iterate(uvo_pnpsolver_set* s, const int32_t* ids, int n_ids, int n_iterations, uvo_glibc_rand* rng, uvo_pnpsolver_result* result) {
  return set_iterate(s, ids, n_ids, n_iterations, rng, result);
}

int uvo_pnpsolver_hypotheses(uvo_pnpsolver_set* s, int id, int32_t* subsets, double* poses, int32_t* counts, int cap, int* n) {
  RC(tap_subsets(s, id, subsets, poses && counts, cap, n));
  if (*n == 0) return UVO_OK;
  const int off = s->solvers[id].tap_off;
  UVO_HIP_CHECK(hipSetDevice(s->device));
  UVO_HIP_CHECK(hipMemcpy(poses, s->D.poses + (size_t)off * 12, (size_t)*n * 96, hipMemcpyDeviceToHost));
  UVO_HIP_CHECK(hipMemcpy(counts, s->D.counts + off, (size_t)*n * 4, hipMemcpyDeviceToHost));
  return UVO_OK;
}

}  // extern "C"
