// USLAM::Sim3Solver for LoopClosing::ComputeSim3 (src/LoopClosing.cc:373-479, src/Sim3Solver.cc): iterate(n) over a LIST of solvers as
// one call.  All arithmetic is sim3_core.hpp, shared with the host build tests/emu/sim3solver_emu.cpp; this file decides which lane
// computes which scalar.  What makes it one call: iterate's loop condition is an AND, so a solver runs min(n_iterations, max_its -
// mnIterations) iterations unless it returns; the host draws every subset of the call from the caller's generator state up front, and
// the stream position of each solver is a prefix sum.  That host side -- the set, the exchange, iterate's walk -- is solver_set.hpp,
// shared with pnpsolver.hip; below the kernels stands what is the Sim3Solver's.
//
// Three launches in the uvo_matcher handle's stream, all scratch sized at uvo_sim3solver_set_create:
//   k_sim3_hypotheses : computeT on three points, one lane per (solver, hypothesis).  The 4 x 4 Jacobi indexes its matrices by a
//                       run-time pivot: A, V, W, indR and indC of the 64 lanes of a workgroup lie interleaved in LDS (176 bytes a lane).
//   k_sim3_score      : one workgroup per (solver, hypothesis): CheckInliers over the solver's points, the inlier set as 64-bit
//                       ballot words (one ordinary store per wavefront and word), the count (integers, reduced through LDS).
//   k_sim3_finish     : one workgroup per listed solver replays iterate() over the counts (sim3::replay; every lane runs the same
//                       scalar control flow) and copies the returned hypothesis and its set into the result.
// Nothing of a solver lives on the device between calls but its points: mnIterations and mnBestInliers are the host's, and the best
// transform of a call that does not return is not observable through the interface.
#include <cmath>
#include <cstring>
#include <vector>

#include "matcher_priv.hpp"
#include "sim3solver.hpp"
#include "solver_set.hpp"

namespace uvo {

constexpr int kSim3HypLanes = 64;

// the device block of a set, by value to every kernel
struct Sim3Dev {
  int32_t max_points, words;  // per solver; words = ceil(max_points / 64)
  const float* x1c;           // [S][max_points][3]  mvX3Dc1
  const float* x2c;           // [S][max_points][3]  mvX3Dc2
  const float* p1;            // [S][max_points][2]  mvP1im1
  const float* p2;            // [S][max_points][2]  mvP2im2
  const float* e1;            // [S][max_points]     mvnMaxError1 as float
  const float* e2;            // [S][max_points]
  const Sim3Call* call;       // [S]
  const int32_t* sub;         // [T][kSim3SubsetStride]
  float* hyp;                 // [T][kSim3HypFloats]
  int32_t* counts;            // [T]
  uint64_t* masks;            // [T][words]
  Sim3Result* result;         // [S]
  uint64_t* out_mask;         // [S][words], indexed by the position in the call's list
};

__global__ __launch_bounds__(kSim3HypLanes) void k_sim3_hypotheses(Sim3Dev D, int total) {
  __shared__ float s_f[sim3::kWsFloats * kSim3HypLanes];
  __shared__ int32_t s_i[sim3::kWsInts * kSim3HypLanes];
  const int g = blockIdx.x * kSim3HypLanes + threadIdx.x;
  if (g >= total) return;
  const int32_t* rec = D.sub + (size_t)g * kSim3SubsetStride;
  const Sim3Call& c = D.call[rec[0]];
  const float* x1 = D.x1c + (size_t)c.id * D.max_points * 3;
  const float* x2 = D.x2c + (size_t)c.id * D.max_points * 3;
  float P1[3][3], P2[3][3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int idx = rec[1 + k];
#pragma unroll
    for (int r = 0; r < 3; ++r) P1[r][k] = x1[3 * idx + r], P2[r][k] = x2[3 * idx + r];
  }
  const sim3::Ws<kSim3HypLanes> W{s_f + threadIdx.x, s_i + threadIdx.x};
  sim3::Hyp H;
  sim3::compute_t(W, P1, P2, H);
  float* out = D.hyp + (size_t)g * kSim3HypFloats;
#pragma unroll
  for (int e = 0; e < 16; ++e) out[e] = H.finite ? H.T12[e] : 0.f, out[16 + e] = H.finite ? H.T21[e] : 0.f;
#pragma unroll
  for (int e = 0; e < 9; ++e) out[32 + e] = H.finite ? H.R[e] : 0.f;
#pragma unroll
  for (int e = 0; e < 3; ++e) out[41 + e] = H.finite ? H.t[e] : 0.f;
  out[44] = H.finite ? H.s : 0.f;
  out[45] = H.finite ? 1.f : 0.f;
  out[46] = out[47] = 0.f;
}

__global__ __launch_bounds__(256) void k_sim3_score(Sim3Dev D) {
  __shared__ int32_t s_wcnt[4];
  __shared__ float s_T[32];
  const int g = blockIdx.x, lane = threadIdx.x & 63, wave = wave_in_block();
  const Sim3Call& c = D.call[D.sub[(size_t)g * kSim3SubsetStride]];
  const float* hyp = D.hyp + (size_t)g * kSim3HypFloats;
  uint64_t* words = D.masks + (size_t)g * D.words;
  if (hyp[45] == 0.f) {  // no finite transform (uniform over the workgroup): zero inliers
    for (int w = threadIdx.x; w * 64 < c.n; w += 256) words[w] = 0;
    if (threadIdx.x == 0) D.counts[g] = 0;
    return;
  }
  if (threadIdx.x < 32) s_T[threadIdx.x] = hyp[threadIdx.x];
  __syncthreads();
  const size_t base = (size_t)c.id * D.max_points;
  const float *x1 = D.x1c + base * 3, *x2 = D.x2c + base * 3, *p1 = D.p1 + base * 2, *p2 = D.p2 + base * 2, *e1 = D.e1 + base, *e2 = D.e2 + base;
  int cnt = 0;
  for (int w = wave; w * 64 < c.n; w += 4) {
    const int i = w * 64 + lane;
    const bool inl = i < c.n && sim3::check_inlier(s_T, s_T + 16, x1 + 3 * i, x2 + 3 * i, p1 + 2 * i, p2 + 2 * i, c.K1, c.K2, e1[i], e2[i]);
    const uint64_t m = __ballot(inl);
    if (lane == 0) words[w] = m;
    cnt += __builtin_popcountll(m);
  }
  if (lane == 0) s_wcnt[wave] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) D.counts[g] = s_wcnt[0] + s_wcnt[1] + s_wcnt[2] + s_wcnt[3];
}

__global__ __launch_bounds__(256) void k_sim3_finish(Sim3Dev D) {
  const int slot = blockIdx.x, tid = threadIdx.x;
  const Sim3Call& c = D.call[slot];
  if (c.hyp_n == 0) return;  // nothing to run: the host answers by itself
  sim3::State st = {c.iterations, c.best_count};
  const sim3::Outcome o = sim3::replay(st, D.counts + c.hyp_off, c.hyp_n, c.max_its, c.min_inliers);
  Sim3Result* r = D.result + slot;
  if (o.returned >= 0) {
    const size_t g = (size_t)(c.hyp_off + o.returned);
    const float* hyp = D.hyp + g * kSim3HypFloats;
    if (tid < 16) r->hyp[tid] = hyp[tid];
    if (tid >= 16 && tid < 32) r->hyp[tid] = tid < 29 ? hyp[16 + tid] : 0.f;  // R, t, s lie behind T21
    uint64_t* out = D.out_mask + (size_t)slot * D.words;
    for (int w = tid; w * 64 < c.n; w += 256) out[w] = D.masks[g * D.words + w];
  } else if (tid < 32) {
    r->hyp[tid] = 0.f;
  }
  if (tid == 0) r->performed = o.performed, r->returned = o.returned, r->no_more = o.no_more, r->inliers = o.inliers, r->best_count = st.best_count;
}

}  // namespace uvo

// ---------------------------------------------------------------------------------------------------------------------------
using namespace uvo;

namespace {
struct Solver : SetSolver {
  int max_its = 1;
  sim3::Params params;
  sim3::Cam K1, K2;
  bool never() const { return n < sim3::kMinSet || n < params.min_inliers; }  // bNoMore at once, nothing drawn
};

bool params_ok(const uvo_sim3solver_params& q) {
  // max_iterations bounds mRansacMaxIts and with it the hypotheses one call plans for a solver: its share of the set's slots
  return q.probability > 0. && q.probability < 1. && q.min_inliers >= 0 && q.max_iterations >= 1 && q.max_iterations <= kSim3HypPerSolver;
}
int max_its_of(int n, const sim3::Params& p) { return n >= sim3::kMinSet ? sim3::derive_max_its(n, p) : 1; }
}  // namespace

struct uvo_sim3solver_set : SolverSet<Sim3Call, Sim3Result> {
  uvo_matcher* m = nullptr;
  Sim3Dev D;
  float *x1c = nullptr, *x2c = nullptr, *p1 = nullptr, *p2 = nullptr, *e1 = nullptr, *e2 = nullptr;  // writable views of D's
  std::vector<Solver> solvers;
  // the matcher's stream moves when the handle is attached to an extractor: every entry that enqueues reads it again
  uvo_sim3solver_set* follow() { return device = m->device, stream = m->stream, this; }

  // what solver_set.hpp asks of a family
  static constexpr int kMaxSolvers = kSim3MaxSolvers, kMinPoints = sim3::kMinSet, kMaxPoints = kSim3MaxPoints, kHypPerSolver = kSim3HypPerSolver;
  static constexpr int kSubsetStride = kSim3SubsetStride;
  static constexpr const char* kRangeText = "Sim3Solver set: 1..64 solvers of 3..16384 points";
  static constexpr const char* kNoMemText = "Sim3Solver set allocation failed";
  static constexpr const char* kFullText = "the Sim3Solver set is full";
  void arrays(Carve& c, bool scratch) {
    const size_t S = (size_t)max_solvers, N = (size_t)max_points, W = (size_t)words, T = (size_t)total;
    if (!scratch) c.take(x1c, S * N * 3).take(x2c, S * N * 3).take(p1, S * N * 2).take(p2, S * N * 2).take(e1, S * N).take(e2, S * N);
    else c.take(D.hyp, T * kSim3HypFloats).take(D.counts, T).take(D.masks, T * W);
  }
  static int min_set(const Solver&) { return sim3::kMinSet; }
  // the loop condition is an AND: never more than max_its <= 320 hypotheses, a solver's share of the set's slots
  static int plan(const Solver& v, int n_iterations) { return v.never() ? 0 : sim3::iterations_ahead(v.iterations, v.max_its, n_iterations); }
  static Sim3Call call(int id, const Solver& v, int off, int K, int) {
    return Sim3Call{id, v.n, v.params.min_inliers, v.max_its, v.iterations, v.best_count, off, K, v.K1, v.K2};
  }
  void launch(int n_ids, int total) const {
    {
      Profiler::Scope ps(&m->prof, "k_sim3_hypotheses", stream);
      hipLaunchKernelGGL(k_sim3_hypotheses, dim3((total + kSim3HypLanes - 1) / kSim3HypLanes), dim3(kSim3HypLanes), 0, stream, D, total);
    }
    {
      Profiler::Scope ps(&m->prof, "k_sim3_score", stream);
      hipLaunchKernelGGL(k_sim3_score, dim3(total), dim3(256), 0, stream, D);
    }
    {
      Profiler::Scope ps(&m->prof, "k_sim3_finish", stream);
      hipLaunchKernelGGL(k_sim3_finish, dim3(n_ids), dim3(256), 0, stream, D);
    }
  }
  // too few points, or mnIterations has reached mRansacMaxIts
  static int idle_no_more(const Solver& v) { return v.never() || v.iterations >= v.max_its ? 1 : 0; }
  static bool adopt(Solver&, const Sim3Result& r, uvo_sim3solver_result* result) {
    if (r.returned < 0) return false;
    std::memcpy(result->T12, r.hyp, 64);
    std::memcpy(result->R12, r.hyp + 16, 36);
    std::memcpy(result->t12, r.hyp + 25, 12);
    result->scale = r.hyp[28];
    return true;
  }
};

extern "C" {

void uvo_sim3solver_set_destroy(uvo_sim3solver_set* s) { set_destroy(s ? s->follow() : s); }

int uvo_sim3solver_set_create(uvo_matcher* m, int max_solvers, int max_points, uvo_sim3solver_set** out) {
  if (!m || !out) return fail(UVO_E_BADARG, "null pointer");
  *out = nullptr;
  uvo_sim3solver_set* s = nullptr;
  RC(set_create(m->device, m->stream, max_solvers, max_points, &s));
  s->m = m;
  Sim3Dev& D = s->D;
  D.max_points = max_points, D.words = s->words;
  D.x1c = s->x1c, D.x2c = s->x2c, D.p1 = s->p1, D.p2 = s->p2, D.e1 = s->e1, D.e2 = s->e2;
  D.call = s->d_call, D.sub = s->d_sub, D.result = s->d_res, D.out_mask = s->d_om;
  *out = s;
  return UVO_OK;
}

int uvo_sim3solver_set_clear(uvo_sim3solver_set* s) { return set_clear(s); }

int uvo_sim3solver_add(uvo_sim3solver_set* s, const float* x1w, const float* x2w, const float* sigma2_1, const float* sigma2_2, const int32_t* index1,
                       int n, int n_matches, const uvo_sim3_keyframe* kf1, const uvo_sim3_keyframe* kf2, const uvo_sim3solver_params* params, int* id) {
  RC(add_check(s, kf1 && kf2 && params && id, n, n_matches, x1w && x2w && sigma2_1 && sigma2_2 && index1));
  if (!params_ok(*params)) return fail(UVO_E_BADARG, "Sim3Solver parameters: probability in (0,1), min_inliers >= 0, max_iterations 1..320");
  for (const uvo_sim3_keyframe* kf : {kf1, kf2}) {
    bool ok = kf->fx == kf->fx && kf->fy == kf->fy && kf->cx == kf->cx && kf->cy == kf->cy;
    for (int e = 0; e < 9; ++e) ok = ok && kf->Rcw[e] == kf->Rcw[e];
    for (int e = 0; e < 3; ++e) ok = ok && kf->tcw[e] == kf->tcw[e];
    if (!ok) return fail(UVO_E_BADARG, "NaN in a key frame's pose or intrinsics");
  }
  for (int i = 0; i < n; ++i) {
    if (index1[i] < 0 || index1[i] >= n_matches) return fail(UVO_E_BADARG, "index1 outside 0..n_matches-1");
    if (!(sigma2_1[i] >= 0.f && sigma2_1[i] <= 1e12f) || !(sigma2_2[i] >= 0.f && sigma2_2[i] <= 1e12f))
      return fail(UVO_E_BADARG, "sigma2 outside 0..1e12");
  }
  Solver v;
  v.n = n, v.n_matches = n_matches;
  v.params = sim3::Params{params->probability, params->min_inliers, params->max_iterations};
  v.max_its = max_its_of(n, v.params);
  v.K1 = sim3::Cam{kf1->fx, kf1->fy, kf1->cx, kf1->cy}, v.K2 = sim3::Cam{kf2->fx, kf2->fy, kf2->cx, kf2->cy};
  v.index.assign(index1, index1 + n);
  if (n > 0) {
    // the constructor's per-point work, once, on the host: mvX3Dc1/2, FromCameraToImage, the thresholds
    std::vector<float> buf((size_t)n * 12);
    float *x1 = buf.data(), *x2 = x1 + 3 * (size_t)n, *p1 = x2 + 3 * (size_t)n, *p2 = p1 + 2 * (size_t)n, *e1 = p2 + 2 * (size_t)n, *e2 = e1 + n;
    for (int i = 0; i < n; ++i) {
      sim3::transform(kf1->Rcw, 3, kf1->tcw[0], kf1->tcw[1], kf1->tcw[2], x1w + 3 * i, x1 + 3 * i);
      sim3::transform(kf2->Rcw, 3, kf2->tcw[0], kf2->tcw[1], kf2->tcw[2], x2w + 3 * i, x2 + 3 * i);
      sim3::to_image(x1 + 3 * i, v.K1, p1 + 2 * i);
      sim3::to_image(x2 + 3 * i, v.K2, p2 + 2 * i);
      e1[i] = sim3::max_error(sigma2_1[i]), e2[i] = sim3::max_error(sigma2_2[i]);
    }
    UVO_HIP_CHECK(hipSetDevice(s->follow()->device));
    hipStream_t st = s->stream;
    const size_t N = (size_t)s->max_points, sid = s->solvers.size();
    UVO_HIP_CHECK(hipMemcpyAsync(s->x1c + sid * N * 3, x1, (size_t)n * 12, hipMemcpyHostToDevice, st));
    UVO_HIP_CHECK(hipMemcpyAsync(s->x2c + sid * N * 3, x2, (size_t)n * 12, hipMemcpyHostToDevice, st));
    UVO_HIP_CHECK(hipMemcpyAsync(s->p1 + sid * N * 2, p1, (size_t)n * 8, hipMemcpyHostToDevice, st));
    UVO_HIP_CHECK(hipMemcpyAsync(s->p2 + sid * N * 2, p2, (size_t)n * 8, hipMemcpyHostToDevice, st));
    UVO_HIP_CHECK(hipMemcpyAsync(s->e1 + sid * N, e1, (size_t)n * 4, hipMemcpyHostToDevice, st));
    UVO_HIP_CHECK(hipMemcpyAsync(s->e2 + sid * N, e2, (size_t)n * 4, hipMemcpyHostToDevice, st));
    UVO_HIP_CHECK(hipStreamSynchronize(st));  // the source is a local
  }
  return add_finish(s, v, id);
}

int uvo_sim3solver_set_ransac_parameters(uvo_sim3solver_set* s, int id, const uvo_sim3solver_params* params) {
  RC(solver_check(s, params != nullptr, id));
  if (!params_ok(*params)) return fail(UVO_E_BADARG, "Sim3Solver parameters: probability in (0,1), min_inliers >= 0, max_iterations 1..320");
  Solver& v = s->solvers[id];
  v.params = sim3::Params{params->probability, params->min_inliers, params->max_iterations};
  v.max_its = max_its_of(v.n, v.params);
  v.iterations = 0;  // mnBestInliers and the best stay, as in the reference
  return UVO_OK;
}

int uvo_sim3solver_query(uvo_sim3solver_set* s, int id, uvo_sim3solver_info* info) {
  RC(solver_check(s, info != nullptr, id));
  const Solver& v = s->solvers[id];
  *info = uvo_sim3solver_info{v.n, v.max_its, v.iterations, v.best_count};
  return UVO_OK;
}

int uvo_sim3solver_iterate(uvo_sim3solver_set* s, const int32_t* ids, int n_ids, int n_iterations, uvo_glibc_rand* rng, uvo_sim3solver_result* result) {
  return set_iterate(s ? s->follow() : s, ids, n_ids, n_iterations, rng, result);
}

int uvo_sim3solver_find(uvo_sim3solver_set* s, int id, uvo_glibc_rand* rng, uvo_sim3solver_result* result) {
  RC(solver_check(s, true, id));
  const int32_t ids[1] = {id};
  return uvo_sim3solver_iterate(s, ids, 1, s->solvers[id].max_its, rng, result);
}

int uvo_sim3solver_hypotheses(uvo_sim3solver_set* s, int id, int32_t* subsets, float* T12, float* T21, int32_t* counts, int cap, int* n) {
  RC(tap_subsets(s, id, subsets, T12 && T21 && counts, cap, n));
  if (*n == 0) return UVO_OK;
  const size_t m = (size_t)*n, off = (size_t)s->solvers[id].tap_off;
  std::vector<float> hyp(m * kSim3HypFloats);
  UVO_HIP_CHECK(hipSetDevice(s->m->device));
  UVO_HIP_CHECK(hipMemcpy(hyp.data(), s->D.hyp + off * kSim3HypFloats, hyp.size() * 4, hipMemcpyDeviceToHost));
  UVO_HIP_CHECK(hipMemcpy(counts, s->D.counts + off, m * 4, hipMemcpyDeviceToHost));
  for (size_t h = 0; h < m; ++h) {
    std::memcpy(T12 + h * 16, &hyp[h * kSim3HypFloats], 64);
    std::memcpy(T21 + h * 16, &hyp[h * kSim3HypFloats + 16], 64);
  }
  return UVO_OK;
}

}  // extern "C"
