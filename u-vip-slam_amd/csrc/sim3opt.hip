// Optimizer::OptimizeSim3 (src/Optimizer.cc:2660-2856) over a LIST of independent loop candidates as one call.  All arithmetic and the
// whole control flow is sim3opt_core.hpp (sim3opt::run), shared with the host build tests/emu/sim3opt_emu.cpp; this file is the device's
// Team -- which lane adds which pairs, how the 256 lane sums meet, who computes the perturbed similarities -- and the host side of
// the C ABI.
//
// One launch: k_sim3_optimize, one workgroup of 256 lanes per problem, both rounds.  A lane owns the pairs l, l + 256, ... for the whole
// call: it alone reads and writes their two chi2 and their state byte (LDS up to kSim3OptLdsPairs pairs, the set's block beyond).  Lanes
// exchange two things.  The reduction is poseopt.hip's: a butterfly of __shfl_xor inside each wavefront, one LDS word per wavefront and
// sum, one barrier, alternating between two buffers; a linearisation's 36 sums stay in LDS for the trials to come.  And before each
// linearisation lanes 0..14 write the 15 x 24 words of the perturbed similarities and their inverses into LDS (2880 bytes), one
// barrier; the words are read until the reduction's barrier and written next after it.  A linearisation is TWO passes of 18 sums over
// the lane's pairs (rows 0..2 of H; rows 3..6, b and the robust chi2): 36 sums, an edge's 2 x 7 Jacobian and the call's state do not
// fit 256 registers together, 18 do.  Values all lanes hold alike (the estimate, the step, lambda, a trial's matrices) are moved to
// scalar registers (Team::uni).  The kernel has no scratch (tests/test_kernel_resources_sim3opt.py).  All branches of sim3opt::run are uniform, every loop has a compile-time bound
// (2 x 10 x 10), and there is no return before the last barrier.
#include <cstring>
#include <vector>

#include "devmem.hpp"
#include "matcher_priv.hpp"
#include "sim3opt.hpp"

namespace uvo {

struct Sim3OptDev {
  const Sim3OptProblemDev* prob;  // [P]
  const float* pairs;             // [sum n][12]
  double* chi2;                   // [P * N][2], used by problems above kSim3OptLdsPairs
  uint8_t* state;                 // [P * N]
  sim3opt::Trace* trace;          // [P]
  sim3opt::Out* result;           // [P]
  uint8_t* mask;                  // [sum n]
};

namespace {

struct Sim3OptTeam {
  double* red;    // LDS [2][4][kSums]
  int32_t* redi;  // LDS [2][4]
  double* store;  // LDS [kSums]
  double* simw;   // LDS [kSims][kSimWords]
  int phase;
  __device__ __forceinline__ bool lead() const { return threadIdx.x == 0; }
  // a value all lanes hold alike, moved to scalar registers
  __device__ __forceinline__ double uni(double v) const {
    return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)), __builtin_amdgcn_readfirstlane(__double2loint(v)));
  }
  template <int K, class F>
  __device__ __forceinline__ const double* gather(F f) {
    double acc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = 0.;
    f((int)threadIdx.x, acc);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1)
#pragma unroll
      for (int k = 0; k < K; ++k) acc[k] = acc[k] + __shfl_xor(acc[k], m);
    double* buf = red + phase * 4 * sim3opt::kSums;
    phase ^= 1;
    const int wave = wave_in_block();
    if ((threadIdx.x & 63) == 0)
#pragma unroll
      for (int k = 0; k < K; ++k) buf[wave * sim3opt::kSums + k] = acc[k];
    __syncthreads();
    return buf;
  }
  static __device__ __forceinline__ double combine(const double* buf, int k) {
    return (buf[k] + buf[sim3opt::kSums + k]) + (buf[2 * sim3opt::kSums + k] + buf[3 * sim3opt::kSums + k]);
  }
  template <int K, class F>
  __device__ __forceinline__ void sum(F f, double* out) {
    const double* buf = gather<K>(f);
#pragma unroll
    for (int k = 0; k < K; ++k) out[k] = combine(buf, k);
  }
  __device__ __forceinline__ double* shared() const { return store; }
  __device__ __forceinline__ double* sims() const { return simw; }
  template <int K, class F>
  __device__ __forceinline__ void sum_shared(F f, double* out) {
    const double* buf = gather<K>(f);
    const int k = (int)threadIdx.x;
    if (k < K) out[k] = combine(buf, k);
    __syncthreads();
  }
  template <class F>
  __device__ __forceinline__ int count(F f) {
    int c = f((int)threadIdx.x);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) c += __shfl_xor(c, m);
    int32_t* buf = redi + phase * 4;
    phase ^= 1;
    if ((threadIdx.x & 63) == 0) buf[wave_in_block()] = c;
    __syncthreads();
    return buf[0] + buf[1] + buf[2] + buf[3];
  }
  // every lane once, then a barrier: what the lanes wrote is there for all
  template <class F>
  __device__ __forceinline__ void each(F f) {
    f((int)threadIdx.x);
    __syncthreads();
  }
};

}  // namespace

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void k_sim3_optimize(Sim3OptDev D) {
  __shared__ double s_chi2[2 * kSim3OptLdsPairs];
  __shared__ double s_red[2 * 4 * sim3opt::kSums];
  __shared__ double s_store[sim3opt::kSums];
  __shared__ double s_sims[sim3opt::kSims * sim3opt::kSimWords];
  __shared__ int32_t s_redi[2 * 4];
  __shared__ uint8_t s_state[kSim3OptLdsPairs];
  const Sim3OptProblemDev& p = D.prob[blockIdx.x];
  const int n = p.n;
  const bool in_lds = n <= kSim3OptLdsPairs;  // uniform
  sim3opt::Pairs E;
  E.in = D.pairs + (size_t)p.off * sim3opt::kPairFloats;
  E.chi2 = in_lds ? s_chi2 : D.chi2 + 2 * (size_t)p.off;
  E.state = in_lds ? s_state : D.state + p.off;
  E.mask = D.mask + p.off;
  E.n = n;
  const sim3opt::Cams C = {p.K1, p.K2};
  Sim3OptTeam T = {s_red, s_redi, s_store, s_sims, 0};
  sim3opt::run<sim3opt::kMutNone>(T, E, C, p.R12, p.t12, p.s12, p.th2, D.result + blockIdx.x, D.trace + blockIdx.x);
}

}  // namespace uvo

// ---------------------------------------------------------------------------------------------------------------------------
using namespace uvo;

static_assert(sizeof(uvo_sim3_opt_trace) == sizeof(sim3opt::Trace) && sizeof(uvo_sim3_opt_trace_lin) == sizeof(sim3opt::TraceLin) &&
                  sizeof(uvo_pose_trace_trial) == sizeof(poseopt::TraceTrial),
              "uvo_sim3_opt_trace is sim3opt::Trace");

struct uvo_sim3_optimizer {
  uvo_matcher* m = nullptr;
  int max_problems = 0, max_pairs = 0, last_n = 0;
  DevMem mem;  // owns D's block and the page-locked mirrors of its two exchanges
  Sim3OptDev D;
  Sim3OptProblemDev* h_prob = nullptr;  // the upload: problem records, then the pairs
  float* h_pairs = nullptr;
  sim3opt::Out* h_res = nullptr;  // the download: result records, then the masks
  uint8_t* h_mask = nullptr;
};

extern "C" {

void uvo_sim3_optimizer_destroy(uvo_sim3_optimizer* o) {
  if (!o) return;
  hipSetDevice(o->m->device);
  if (o->m->stream) hipStreamSynchronize(o->m->stream);
  o->mem.release_all();
  delete o;
}

int uvo_sim3_optimizer_create(uvo_matcher* m, int max_problems, int max_pairs, uvo_sim3_optimizer** out) {
  if (!m || !out) return fail(UVO_E_BADARG, "null pointer");
  *out = nullptr;
  if (max_problems < 1 || max_problems > kSim3OptMaxProblems || max_pairs < 1 || max_pairs > kSim3OptMaxPairs)
    return fail(UVO_E_BADARG, "Sim3 optimizer: 1..64 problems of 1..16384 pairs");
  uvo_sim3_optimizer* o = new uvo_sim3_optimizer();
  o->m = m, o->max_problems = max_problems, o->max_pairs = max_pairs;
  const size_t P = (size_t)max_problems, N = (size_t)max_pairs;
  Sim3OptDev& D = o->D;
  float* pairs = nullptr;
  Sim3OptProblemDev* prob = nullptr;
  // each exchange is one copy: its two arrays are adjacent, on the device and in the mirror
  auto upload = [&](Carve& c, auto*& pr, auto*& pa) { c.take(pr, P).take(pa, P * N * sim3opt::kPairFloats, alignof(float)); };
  auto download = [&](Carve& c, auto*& res, auto*& mk) { c.take(res, P).take(mk, P * N, alignof(uint8_t)); };
  int rc = hipSetDevice(m->device) == hipSuccess ? UVO_OK : fail(UVO_E_NOMEM, "Sim3 optimizer allocation failed");
  if (!rc) rc = alloc_carved(o->mem, [&](Carve& c) {
    upload(c, prob, pairs);
    c.take(D.chi2, 2 * P * N).take(D.state, P * N).take(D.trace, P);
    download(c, D.result, D.mask);
  });
  if (!rc) rc = alloc_carved(o->mem, [&](Carve& c) { upload(c, o->h_prob, o->h_pairs); }, true);
  if (!rc) rc = alloc_carved(o->mem, [&](Carve& c) { download(c, o->h_res, o->h_mask); }, true);
  if (rc) return uvo_sim3_optimizer_destroy(o), rc;
  D.prob = prob, D.pairs = pairs;
  *out = o;
  return UVO_OK;
}

int uvo_sim3_optimize(uvo_sim3_optimizer* o, const uvo_sim3_opt_problem* problems, int n_problems, uvo_sim3_opt_result* results) {
  if (!o) return fail(UVO_E_BADARG, "null handle");
  if (n_problems < 0) return fail(UVO_E_BADARG, "negative problem count");
  if (n_problems > o->max_problems) return fail(UVO_E_CAPACITY, "more problems than the Sim3 optimizer was sized for");
  if (n_problems > 0 && (!problems || !results)) return fail(UVO_E_BADARG, "null pointer");
  size_t total = 0;
  for (int j = 0; j < n_problems; ++j) {
    const uvo_sim3_opt_problem& q = problems[j];
    if (q.n < 0) return fail(UVO_E_BADARG, "negative pair count");
    if (q.n > o->max_pairs) return fail(UVO_E_CAPACITY, "more pairs than the Sim3 optimizer was sized for");
    if (q.n > 0 && (!q.x1w || !q.x2w || !q.obs1 || !q.obs2 || !q.info1 || !q.info2)) return fail(UVO_E_BADARG, "null pointer");
    if (results[j].removed && results[j].removed_cap < q.n) return fail(UVO_E_CAPACITY, "removed_cap is smaller than the problem's n");
    total += (size_t)q.n;
  }
  if (n_problems == 0) return UVO_OK;
  int off = 0;
  for (int j = 0; j < n_problems; ++j) {
    const uvo_sim3_opt_problem& q = problems[j];
    Sim3OptProblemDev& r = o->h_prob[j];
    r.n = q.n, r.off = off;
    r.K1[0] = q.kf1.fx, r.K1[1] = q.kf1.fy, r.K1[2] = q.kf1.cx, r.K1[3] = q.kf1.cy;
    r.K2[0] = q.kf2.fx, r.K2[1] = q.kf2.fy, r.K2[2] = q.kf2.cx, r.K2[3] = q.kf2.cy;
    std::memcpy(r.R12, q.R12, sizeof r.R12);
    std::memcpy(r.t12, q.t12, sizeof r.t12);
    r.s12 = q.s12, r.th2 = q.th2;
    float* e = o->h_pairs + (size_t)off * sim3opt::kPairFloats;
    for (int i = 0; i < q.n; ++i, e += sim3opt::kPairFloats) {
      sim3opt::pack_pair(q.kf1.Rcw, q.kf1.tcw, q.kf2.Rcw, q.kf2.tcw, q.x1w + 3 * i, q.x2w + 3 * i, q.obs1 + 2 * i, q.obs2 + 2 * i, q.info1[i], q.info2[i], e);
    }
    off += q.n;
  }
  const size_t P = (size_t)o->max_problems;
  uvo_matcher* m = o->m;
  UVO_HIP_CHECK(hipSetDevice(m->device));
  hipStream_t st = m->stream;
  UVO_HIP_CHECK(hipMemcpyAsync(const_cast<Sim3OptProblemDev*>(o->D.prob), o->h_prob,
                               P * sizeof(Sim3OptProblemDev) + total * sim3opt::kPairFloats * sizeof(float), hipMemcpyHostToDevice, st));
  {
    Profiler::Scope ps(&m->prof, "k_sim3_optimize", st);
    hipLaunchKernelGGL(k_sim3_optimize, dim3(n_problems), dim3(256), 0, st, o->D);
  }
  UVO_HIP_CHECK(hipGetLastError());
  UVO_HIP_CHECK(hipMemcpyAsync(o->h_res, o->D.result, P * sizeof(sim3opt::Out) + total, hipMemcpyDeviceToHost, st));
  UVO_HIP_CHECK(hipStreamSynchronize(st));
  o->last_n = n_problems;
  for (int j = 0; j < n_problems; ++j) {
    const sim3opt::Out& r = o->h_res[j];
    uvo_sim3_opt_result& w = results[j];
    std::memcpy(w.q, r.q, sizeof r.q), std::memcpy(w.t, r.t, sizeof r.t), w.s = r.s;
    std::memcpy(w.R12, r.R12, sizeof r.R12), std::memcpy(w.t12, r.t12, sizeof r.t12), w.scale = r.scale;
    w.n_inliers = r.n_inliers, w.n_correspondences = r.n_correspondences, w.n_bad = r.n_bad, w.more_iterations = r.more_iterations;
    if (w.removed && problems[j].n > 0) std::memcpy(w.removed, o->h_mask + o->h_prob[j].off, (size_t)problems[j].n);
  }
  return UVO_OK;
}

int uvo_sim3_optimizer_trace(uvo_sim3_optimizer* o, int problem, uvo_sim3_opt_trace* out) {
  if (!o || !out) return fail(UVO_E_BADARG, "null pointer");
  if (problem < 0 || problem >= o->last_n) return fail(UVO_E_BADARG, "the last call had no such problem");
  UVO_HIP_CHECK(hipSetDevice(o->m->device));
  UVO_HIP_CHECK(hipMemcpy(out, o->D.trace + problem, sizeof(sim3opt::Trace), hipMemcpyDeviceToHost));
  // records beyond the counts are whatever an earlier call left: not part of the answer
  std::memset(out->lin + out->n_lin, 0, sizeof(uvo_sim3_opt_trace_lin) * (size_t)(sim3opt::kMaxLin - out->n_lin));
  std::memset(out->trial + out->n_trials, 0, sizeof(uvo_pose_trace_trial) * (size_t)(sim3opt::kMaxTrialRecs - out->n_trials));
  return UVO_OK;
}

}  // extern "C"
