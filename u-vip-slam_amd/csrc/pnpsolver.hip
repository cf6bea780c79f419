// USLAM::PnPsolver for Tracking::Relocalisation (src/Tracking.cc:2415-2517, src/PnPsolver.cc): iterate(n) over a LIST of solvers as one
// call.  All arithmetic is pnpsolver_core.hpp / epnp_core.hpp, shared with the host build tests/emu/pnpsolver_emu.cpp; this file
// decides which lane computes which scalar.  What makes it one call: the iterations a solver runs unless it returns are known before
// anything is evaluated (max(max_its - mnIterations, n_iterations), the loop condition being an OR), so the host draws every subset of
// the call from the caller's generator state up front, and the stream position of each solver is a prefix sum.
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

#include "devmem.hpp"
#include "pnpsolver.hpp"

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
struct Solver {
  int n = 0, n_matches = 0;
  pnps::Params params;
  pnps::Derived d;
  double fu = 0, fv = 0, uc = 0, vc = 0;
  pnps::State st = {0, 0};
  int parity = 0;
  std::vector<int32_t> kp_index;
  int tap_off = 0, tap_n = 0;  // the hypotheses it consumed in the last iterate call
};
}  // namespace

struct uvo_pnpsolver_set {
  uvo_klt* klt = nullptr;
  hipStream_t stream = nullptr;
  int device = 0, max_solvers = 0, max_points = 0, words = 0, total = 0;
  DevMem mem;  // owns D's block and the page-locked mirrors of its two exchanges
  PnpsDev D;
  float *p3d = nullptr, *p2d = nullptr, *max_err = nullptr;  // writable views of D's
  PnpsCall* h_call = nullptr;  // the upload: call records, then hypothesis records
  int32_t* h_hyp = nullptr;
  PnpsResult* h_res = nullptr;  // the download: result records, then the returned sets
  uint64_t* h_om = nullptr;
  std::vector<Solver> solvers;
  std::vector<int32_t> avail;  // draw_subset's slots
  std::vector<char> seen;      // per solver: listed in the current call
};

extern "C" {

void uvo_glibc_srand(uvo_glibc_rand* g, uint32_t seed) {
  static_assert(sizeof(uvo_glibc_rand) == sizeof(pnps::GlibcRand), "uvo_glibc_rand is pnps::GlibcRand");
  if (g) reinterpret_cast<pnps::GlibcRand*>(g)->srand(seed);
}

int32_t uvo_glibc_rand_next(uvo_glibc_rand* g) { return g ? reinterpret_cast<pnps::GlibcRand*>(g)->next() : 0; }

void uvo_pnpsolver_set_destroy(uvo_pnpsolver_set* s) {
  if (!s) return;
  hipSetDevice(s->device);
  if (s->stream) hipStreamSynchronize(s->stream);
  s->mem.release_all();
  delete s;
}

int uvo_pnpsolver_set_create(uvo_klt* k, int max_solvers, int max_points, uvo_pnpsolver_set** out) {
  if (!k || !out) return fail(UVO_E_BADARG, "null pointer");
  *out = nullptr;
  if (max_solvers < 1 || max_solvers > kPnpsMaxSolvers || max_points < pnps::kMinSetLo || max_points > kPnpsMaxPoints)
    return fail(UVO_E_BADARG, "PnPsolver set: 1..64 solvers of 4..16384 points");
  uvo_pnpsolver_set* s = new uvo_pnpsolver_set();
  s->klt = k, s->stream = klt_stream(k), s->device = klt_device(k);
  s->max_solvers = max_solvers, s->max_points = max_points, s->words = (max_points + 63) / 64, s->total = max_solvers * kPnpsHypPerSolver;
  const size_t S = (size_t)max_solvers, N = (size_t)max_points, W = (size_t)s->words, T = (size_t)s->total;
  PnpsDev& D = s->D;
  D.max_points = max_points, D.words = s->words;
  // each exchange is one copy: its two arrays are adjacent, on the device and in the mirror
  auto upload = [&](Carve& c, auto*& call, auto*& hyp) { c.take(call, S).take(hyp, T * kPnpsSubsetStride, alignof(int32_t)); };
  auto download = [&](Carve& c, auto*& res, auto*& om) { c.take(res, S).take(om, S * W, alignof(uint64_t)); };
  int rc = hipSetDevice(s->device) == hipSuccess ? UVO_OK : fail(UVO_E_NOMEM, "PnPsolver set allocation failed");
  if (!rc) rc = alloc_carved(s->mem, [&](Carve& c) {
    c.take(s->p3d, S * N * 3).take(s->p2d, S * N * 2).take(s->max_err, S * N).take(D.best_mask, S * 2 * W).take(D.best_pose, S * 2 * 12);
    upload(c, D.call, D.hyp);
    c.take(D.poses, T * 12).take(D.counts, T).take(D.masks, T * W).take(D.list, S * N);
    download(c, D.result, D.out_mask);
  });
  if (!rc) rc = alloc_carved(s->mem, [&](Carve& c) { upload(c, s->h_call, s->h_hyp); }, true);
  if (!rc) rc = alloc_carved(s->mem, [&](Carve& c) { download(c, s->h_res, s->h_om); }, true);
  if (rc) return uvo_pnpsolver_set_destroy(s), rc;
  D.p3d = s->p3d, D.p2d = s->p2d, D.max_err = s->max_err;
  s->avail.resize(N);
  s->seen.resize(S);
  s->solvers.reserve(S);
  *out = s;
  return UVO_OK;
}

int uvo_pnpsolver_set_clear(uvo_pnpsolver_set* s) {
  if (!s) return fail(UVO_E_BADARG, "null handle");
  s->solvers.clear();
  return UVO_OK;
}

int uvo_pnpsolver_add(uvo_pnpsolver_set* s, const float* p3d, const float* p2d, const float* sigma2, const int32_t* kp_index, int n, int n_matches,
                      float fx, float fy, float cx, float cy, const uvo_pnpsolver_params* params, int* id) {
  if (!s || !params || !id) return fail(UVO_E_BADARG, "null pointer");
  if (n < 0 || n > s->max_points || n_matches < n) return fail(UVO_E_BADARG, "point count outside 0..max_points, or more points than matches");
  if (n > 0 && (!p3d || !p2d || !sigma2 || !kp_index)) return fail(UVO_E_BADARG, "null pointer");
  if ((int)s->solvers.size() >= s->max_solvers) return fail(UVO_E_BADARG, "the PnPsolver set is full");
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
  v.kp_index.assign(kp_index, kp_index + n);
  const int sid = (int)s->solvers.size();
  if (n > 0) {
    UVO_HIP_CHECK(hipSetDevice(s->device));
    const size_t N = (size_t)s->max_points;
    std::vector<float> me(n);
    for (int i = 0; i < n; ++i) me[i] = sigma2[i] * q.th2;  // mvMaxError, in float
    UVO_HIP_CHECK(hipMemcpyAsync(s->p3d + sid * N * 3, p3d, (size_t)n * 12, hipMemcpyHostToDevice, s->stream));
    UVO_HIP_CHECK(hipMemcpyAsync(s->p2d + sid * N * 2, p2d, (size_t)n * 8, hipMemcpyHostToDevice, s->stream));
    UVO_HIP_CHECK(hipMemcpyAsync(s->max_err + sid * N, me.data(), (size_t)n * 4, hipMemcpyHostToDevice, s->stream));
    UVO_HIP_CHECK(hipStreamSynchronize(s->stream));  // the sources are the caller's pageable memory and a local
  }
  s->solvers.push_back(std::move(v));
  *id = sid;
  return UVO_OK;
}

int uvo_pnpsolver_query(uvo_pnpsolver_set* s, int id, uvo_pnpsolver_info* info) {
  if (!s || !info) return fail(UVO_E_BADARG, "null pointer");
  if (id < 0 || id >= (int)s->solvers.size()) return fail(UVO_E_BADARG, "no such solver");
  const Solver& v = s->solvers[id];
  *info = uvo_pnpsolver_info{v.n, v.d.min_inliers, v.d.max_its, v.st.iterations, v.st.best_count};
  return UVO_OK;
}

int uvo_pnpsolver_iterate(uvo_pnpsolver_set* s, const int32_t* ids, int n_ids, int n_iterations, uvo_glibc_rand* rng, uvo_pnpsolver_result* result) {
  if (!s || !rng || !result || (n_ids > 0 && !ids)) return fail(UVO_E_BADARG, "null pointer");
  if (n_ids < 0 || n_ids > s->max_solvers) return fail(UVO_E_BADARG, "more ids than the set has solvers");
  if (n_iterations < 1) return fail(UVO_E_BADARG, "n_iterations must be at least 1");
  uvo_pnpsolver_status* status = result->status;
  uint8_t* mask_out = result->inliers;
  result->returned = -1, result->solver = -1, result->n_inliers = 0, result->refined = 0, result->draws = 0;
  std::fill(result->Tcw, result->Tcw + 16, 0.f);
  std::vector<char>& seen = s->seen;
  std::fill(seen.begin(), seen.end(), 0);
  for (int j = 0; j < n_ids; ++j) {
    if (ids[j] < 0 || ids[j] >= (int)s->solvers.size()) return fail(UVO_E_BADARG, "no such solver");
    if (seen[ids[j]]) return fail(UVO_E_BADARG, "a solver is listed twice in one iterate call");
    seen[ids[j]] = 1;
    if (mask_out && result->inliers_cap < s->solvers[ids[j]].n_matches)
      return fail(UVO_E_CAPACITY, "inliers_cap is smaller than a listed solver's n_matches");
  }
  for (Solver& v : s->solvers) v.tap_off = v.tap_n = 0;
  if (status)
    for (int j = 0; j < n_ids; ++j) status[j] = uvo_pnpsolver_status{0, 0, s->solvers[ids[j]].st.iterations};
  // every subset of the call, from a copy of the caller's state: the stream position of a solver is the prefix sum of what the
  // solvers in front of it run
  pnps::GlibcRand g;
  std::memcpy(&g, rng, sizeof g);
  PnpsCall* call = s->h_call;
  int32_t* hyp = s->h_hyp;
  int total = 0;
  for (int j = 0; j < n_ids; ++j) {
    const Solver& v = s->solvers[ids[j]];
    const int K = v.n < v.d.min_inliers ? 0 : pnps::iterations_ahead(v.st.iterations, v.d.max_its, n_iterations);
    if (total + K > s->total) return fail(UVO_E_BADARG, "the call needs more hypothesis slots than the set has (320 per solver)");
    call[j] = PnpsCall{ids[j], v.n, v.params.min_set, v.d.min_inliers, v.d.max_its, v.st.iterations, v.st.best_count, v.parity, total, K, n_iterations, 0,
                       v.fu, v.fv, v.uc, v.vc};
    for (int h = 0; h < K; ++h) {
      int32_t* rec = hyp + (size_t)(total + h) * kPnpsSubsetStride;
      rec[0] = j;
      for (int e = 1; e < kPnpsSubsetStride; ++e) rec[e] = 0;
      pnps::draw_subset(g, v.n, v.params.min_set, s->avail.data(), rec + 1);
    }
    total += K;
  }
  const PnpsResult* res = s->h_res;
  const size_t W = (size_t)s->words;
  if (total > 0) {
    UVO_HIP_CHECK(hipSetDevice(s->device));
    hipStream_t st = s->stream;
    UVO_HIP_CHECK(hipMemcpyAsync(const_cast<PnpsCall*>(s->D.call), call, (size_t)s->max_solvers * sizeof(PnpsCall) + (size_t)total * kPnpsSubsetStride * 4,
                                 hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_pnps_hypotheses, dim3((total + kPnpsHypLanes - 1) / kPnpsHypLanes), dim3(kPnpsHypLanes), 0, st, s->D, total);
    hipLaunchKernelGGL(k_pnps_score, dim3(total), dim3(256), 0, st, s->D);
    hipLaunchKernelGGL(k_pnps_finish, dim3(n_ids), dim3(256), 0, st, s->D);
    UVO_HIP_CHECK(hipGetLastError());
    // result records of all solver slots, then the sets of the listed ones: adjacent on the device
    UVO_HIP_CHECK(hipMemcpyAsync(s->h_res, s->D.result, (size_t)s->max_solvers * sizeof(PnpsResult) + (size_t)n_ids * W * 8, hipMemcpyDeviceToHost, st));
    UVO_HIP_CHECK(hipStreamSynchronize(st));
  }
  int draws = 0;
  for (int j = 0; j < n_ids; ++j) {
    Solver& v = s->solvers[ids[j]];
    if (call[j].hyp_n == 0) {  // fewer points than nMinInliers: bNoMore at once, nothing drawn (n_iterations >= 1: every other solver has iterations to run)
      if (status) status[j] = uvo_pnpsolver_status{1, 1, v.st.iterations};
      continue;
    }
    const PnpsResult& r = res[j];
    v.st.iterations += r.performed, v.st.best_count = r.best_count, v.parity ^= 1;
    v.tap_off = call[j].hyp_off, v.tap_n = r.performed;
    draws += r.performed * v.params.min_set;
    if (status) status[j] = uvo_pnpsolver_status{1, r.no_more, v.st.iterations};
    if (r.returned == pnps::kNone) continue;
    result->returned = j, result->solver = ids[j], result->n_inliers = r.inliers, result->refined = r.returned == pnps::kRefined ? 1 : 0;
    float* T = result->Tcw;
    for (int a = 0; a < 3; ++a) {
      for (int b = 0; b < 3; ++b) T[4 * a + b] = (float)r.pose[3 * a + b];
      T[4 * a + 3] = (float)r.pose[9 + a];
    }
    T[15] = 1.f;
    if (mask_out) {
      std::fill(mask_out, mask_out + v.n_matches, (uint8_t)0);
      const uint64_t* words = s->h_om + (size_t)j * W;
      for (int i = 0; i < v.n; ++i)
        if (words[i >> 6] >> (i & 63) & 1) mask_out[v.kp_index[i]] = 1;
    }
    break;
  }
  result->draws = (uint32_t)draws;  // the caller's state moves to where rand() would stand after the iterations actually performed
  pnps::GlibcRand* gr = reinterpret_cast<pnps::GlibcRand*>(rng);
  for (int d = 0; d < draws; ++d) (void)gr->next();
  return UVO_OK;
}

int uvo_pnpsolver_hypotheses(uvo_pnpsolver_set* s, int id, int32_t* subsets, double* poses, int32_t* counts, int cap, int* n) {
  if (!s || !n) return fail(UVO_E_BADARG, "null pointer");
  if (id < 0 || id >= (int)s->solvers.size()) return fail(UVO_E_BADARG, "no such solver");
  if (cap < 0) return fail(UVO_E_BADARG, "negative capacity");
  const Solver& v = s->solvers[id];
  const int m = cap < v.tap_n ? cap : v.tap_n;
  if (m > 0 && (!subsets || !poses || !counts)) return fail(UVO_E_BADARG, "null pointer");
  *n = m;
  if (m == 0) return UVO_OK;
  const int32_t* hyp = s->h_hyp;  // the subsets were drawn on the host
  for (int h = 0; h < m; ++h)
    for (int e = 0; e < v.params.min_set; ++e) subsets[h * v.params.min_set + e] = hyp[(size_t)(v.tap_off + h) * kPnpsSubsetStride + 1 + e];
  UVO_HIP_CHECK(hipSetDevice(s->device));
  UVO_HIP_CHECK(hipMemcpy(poses, s->D.poses + (size_t)v.tap_off * 12, (size_t)m * 96, hipMemcpyDeviceToHost));
  UVO_HIP_CHECK(hipMemcpy(counts, s->D.counts + v.tap_off, (size_t)m * 4, hipMemcpyDeviceToHost));
  return UVO_OK;
}

}  // extern "C"
