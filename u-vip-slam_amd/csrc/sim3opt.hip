// Optimizer::OptimizeSim3 (src/Optimizer.cc:2660-2856) over a LIST of independent loop candidates as one call.  All arithmetic and the
// whole control flow is sim3opt_core.hpp (sim3opt::run), shared with the host build tests/emu/sim3opt_emu.cpp; this file is the device's
// Team -- lane_team.hpp's LaneTeam (which lane adds which pairs, how the 256 lane sums meet) and who computes the perturbed
// similarities -- and the host side of the C ABI, whose memory and copies are opt_exchange.hpp's.
//
// One launch: k_sim3_optimize, one workgroup of 256 lanes per problem, both rounds.  A lane owns the pairs l, l + 256, ... for the whole
// call: it alone reads and writes their two chi2 and their state byte (LDS up to kSim3OptLdsPairs pairs, the set's block beyond).  Lanes
// exchange two things.  The reduction is lane_team.hpp's; a linearisation's 36 sums stay in LDS for the trials to come.  And before each
// linearisation lanes 0..14 write the 15 x 24 words of the perturbed similarities and their inverses into LDS (2880 bytes), one
// barrier; the words are read until the reduction's barrier and written next after it.  A linearisation is TWO passes of 18 sums over
// the lane's pairs (rows 0..2 of H; rows 3..6, b and the robust chi2): 36 sums, an edge's 2 x 7 Jacobian and the call's state do not
// fit 256 registers together, 18 do.  Values all lanes hold alike (the estimate, the step, lambda, a trial's matrices) are moved to
// scalar registers (Team::uni).  The kernel has no scratch (tests/test_kernel_resources_sim3opt.py).  All branches of sim3opt::run are uniform, every loop has a compile-time bound
// (2 x 10 x 10), and there is no return before the last barrier.
#include <cstring>

#include "matcher_priv.hpp"
#include "opt_exchange.hpp"
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

struct Sim3OptTeam : LaneTeam<sim3opt::kSums> {
  double* simw;  // LDS [kSims][kSimWords]
  // a value all lanes hold alike, moved to scalar registers
  __device__ __forceinline__ double uni(double v) const {
    return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)), __builtin_amdgcn_readfirstlane(__double2loint(v)));
  }
  __device__ __forceinline__ double* sims() const { return simw; }
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
  Sim3OptTeam T = {{s_red, s_redi, s_store, 0}, s_sims};
  sim3opt::run<sim3opt::kMutNone>(T, E, C, p.R12, p.t12, p.s12, p.th2, D.result + blockIdx.x, D.trace + blockIdx.x);
}

}  // namespace uvo

// ---------------------------------------------------------------------------------------------------------------------------
using namespace uvo;

static_assert(sizeof(uvo_sim3_opt_trace) == sizeof(sim3opt::Trace) && sizeof(uvo_sim3_opt_trace_lin) == sizeof(sim3opt::TraceLin) &&
                  sizeof(uvo_pose_trace_trial) == sizeof(poseopt::TraceTrial),
              "uvo_sim3_opt_trace is sim3opt::Trace");

struct uvo_sim3_optimizer : OptExchange<Sim3OptProblemDev, sim3opt::Out, sim3opt::Trace> {  // items: pairs
  uvo_matcher* m = nullptr;
};

extern "C" {

void uvo_sim3_optimizer_destroy(uvo_sim3_optimizer* o) {
  if (!o) return;
  o->stream = o->m->stream;
  o->destroy();
  delete o;
}

int uvo_sim3_optimizer_create(uvo_matcher* m, int max_problems, int max_pairs, uvo_sim3_optimizer** out) {
  if (!m || !out) return fail(UVO_E_BADARG, "null pointer");
  *out = nullptr;
  if (max_problems < 1 || max_problems > kSim3OptMaxProblems || max_pairs < 1 || max_pairs > kSim3OptMaxPairs)
    return fail(UVO_E_BADARG, "Sim3 optimizer: 1..64 problems of 1..16384 pairs");
  uvo_sim3_optimizer* o = new uvo_sim3_optimizer();
  o->m = m;
  const int rc = o->create(m->device, m->stream, max_problems, max_pairs, sim3opt::kPairFloats, 2, "Sim3 optimizer allocation failed");
  if (rc) return uvo_sim3_optimizer_destroy(o), rc;
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
    if (q.n > o->max_items) return fail(UVO_E_CAPACITY, "more pairs than the Sim3 optimizer was sized for");
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
    float* e = o->h_items + (size_t)off * sim3opt::kPairFloats;
    for (int i = 0; i < q.n; ++i, e += sim3opt::kPairFloats) {
      sim3opt::pack_pair(q.kf1.Rcw, q.kf1.tcw, q.kf2.Rcw, q.kf2.tcw, q.x1w + 3 * i, q.x2w + 3 * i, q.obs1 + 2 * i, q.obs2 + 2 * i, q.info1[i], q.info2[i], e);
    }
    off += q.n;
  }
  o->stream = o->m->stream;  // the matcher's of now: attaching an extractor changes it
  RC(o->send(total));
  const Sim3OptDev D = {o->prob, o->items, o->chi2, o->state, o->trace, o->result, o->mask};
  {
    Profiler::Scope ps(&o->m->prof, "k_sim3_optimize", o->stream);
    hipLaunchKernelGGL(k_sim3_optimize, dim3(n_problems), dim3(256), 0, o->stream, D);
  }
  UVO_HIP_CHECK(hipGetLastError());
  RC(o->receive(total));
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
  return !o || !out ? fail(UVO_E_BADARG, "null pointer") : o->read_trace(problem, out);
}

}  // extern "C"
