// Optimizer::PoseOptimization(Frame*) (src/Optimizer.cc:2012-2145) over a LIST of independent problems as one call.  All arithmetic and
// the whole control flow is poseopt_core.hpp (poseopt::run), shared with the host build tests/emu/poseopt_emu.cpp; this file is the
// kernel around it and the host side of the C ABI.  The device's Team -- which lane adds which edges and how the 256 lane sums meet --
// is lane_team.hpp's LaneTeam; the handle's memory and the two copies of a call are opt_exchange.hpp's.
//
// One launch: k_pose_optimize, one workgroup of 256 lanes per problem, all four rounds.  A lane owns the edges l, l + 256, ... for the
// whole call: it alone reads and writes their chi2 and state bytes (LDS up to kPoseLdsEdges edges, the set's block beyond), so the only
// exchange between lanes is the reduction (lane_team.hpp: one barrier for a trial's sum; a linearisation's 28 sums stay in LDS for the
// ten trials to come).  Every lane then computes the 6 x 6 solve and the Levenberg decision from the same words: all branches of
// poseopt::run are uniform, every loop has a compile-time bound (4 x 10 x 10), and there is no return before the last barrier.
#include <cstring>

#include "opt_exchange.hpp"
#include "poseopt.hpp"

namespace uvo {

struct PoseDev {
  const PoseProblemDev* prob;  // [P]
  const float* edges;          // [sum n][6]
  double* chi2;                // [P * N], used by problems above kPoseLdsEdges
  uint8_t* state;              // [P * N]
  poseopt::Trace* trace;       // [P]
  poseopt::Out* result;        // [P]
  uint8_t* mask;               // [sum n]
};

using DevTeam = LaneTeam<poseopt::kSums>;

// Two wavefronts per SIMD asked for: one workgroup would be allowed 512 registers a lane and the scheduler spends what it is allowed;
// at 256 (arch and accumulation registers together) it still needs no scratch (tests/test_kernel_resources_poseopt.py).
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void k_pose_optimize(PoseDev D) {
  __shared__ double s_chi2[kPoseLdsEdges];
  __shared__ double s_red[2 * 4 * poseopt::kSums];
  __shared__ double s_store[poseopt::kSums];
  __shared__ int32_t s_redi[2 * 4];
  __shared__ uint8_t s_state[kPoseLdsEdges];
  const PoseProblemDev& p = D.prob[blockIdx.x];
  const int n = p.n;
  const bool in_lds = n <= kPoseLdsEdges;  // uniform
  poseopt::Edges E;
  E.in = D.edges + (size_t)p.off * kPoseEdgeFloats;
  E.chi2 = in_lds ? s_chi2 : D.chi2 + p.off;
  E.state = in_lds ? s_state : D.state + p.off;
  E.mask = D.mask + p.off;
  E.n = n;
  const poseopt::Cam C = {(double)p.fx, (double)p.fy, (double)p.cx, (double)p.cy};
  DevTeam T = {s_red, s_redi, s_store, 0};
  poseopt::run<poseopt::kMutNone>(T, E, C, p.Tcw, D.result + blockIdx.x, D.trace + blockIdx.x);
}

}  // namespace uvo

// ---------------------------------------------------------------------------------------------------------------------------
using namespace uvo;

static_assert(sizeof(uvo_pose_trace) == sizeof(poseopt::Trace) && sizeof(uvo_pose_trace_lin) == sizeof(poseopt::TraceLin) &&
                  sizeof(uvo_pose_trace_trial) == sizeof(poseopt::TraceTrial),
              "uvo_pose_trace is poseopt::Trace");

struct uvo_pose_optimizer : OptExchange<PoseProblemDev, poseopt::Out, poseopt::Trace> {};  // items: edges, on the KLT handle's stream

extern "C" {

void uvo_pose_optimizer_destroy(uvo_pose_optimizer* o) {
  if (!o) return;
  o->destroy();
  delete o;
}

int uvo_pose_optimizer_create(uvo_klt* k, int max_problems, int max_points, uvo_pose_optimizer** out) {
  if (!k || !out) return fail(UVO_E_BADARG, "null pointer");
  *out = nullptr;
  if (max_problems < 1 || max_problems > kPoseMaxProblems || max_points < 1 || max_points > kPoseMaxPoints)
    return fail(UVO_E_BADARG, "pose optimizer: 1..64 problems of 1..16384 points");
  uvo_pose_optimizer* o = new uvo_pose_optimizer();
  const int rc = o->create(klt_device(k), klt_stream(k), max_problems, max_points, kPoseEdgeFloats, 1, "pose optimizer allocation failed");
  if (rc) return uvo_pose_optimizer_destroy(o), rc;
  *out = o;
  return UVO_OK;
}

int uvo_pose_optimize(uvo_pose_optimizer* o, const uvo_pose_problem* problems, int n_problems, uvo_pose_result* results) {
  if (!o) return fail(UVO_E_BADARG, "null handle");
  if (n_problems < 0) return fail(UVO_E_BADARG, "negative problem count");
  if (n_problems > o->max_problems) return fail(UVO_E_CAPACITY, "more problems than the pose optimizer was sized for");
  if (n_problems > 0 && (!problems || !results)) return fail(UVO_E_BADARG, "null pointer");
  size_t total = 0;
  for (int j = 0; j < n_problems; ++j) {
    const uvo_pose_problem& q = problems[j];
    if (q.n < 0) return fail(UVO_E_BADARG, "negative point count");
    if (q.n > o->max_items) return fail(UVO_E_CAPACITY, "more points than the pose optimizer was sized for");
    if (q.n > 0 && (!q.p3d || !q.p2d || !q.inv_sigma2)) return fail(UVO_E_BADARG, "null pointer");
    if (results[j].outlier && results[j].outlier_cap < q.n) return fail(UVO_E_CAPACITY, "outlier_cap is smaller than the problem's n");
    total += (size_t)q.n;
  }
  if (n_problems == 0) return UVO_OK;
  int off = 0;
  for (int j = 0; j < n_problems; ++j) {
    const uvo_pose_problem& q = problems[j];
    PoseProblemDev& r = o->h_prob[j];
    r.n = q.n, r.off = off, r.fx = q.fx, r.fy = q.fy, r.cx = q.cx, r.cy = q.cy, r.pad_[0] = r.pad_[1] = 0;
    std::memcpy(r.Tcw, q.Tcw, sizeof r.Tcw);
    float* e = o->h_items + (size_t)off * kPoseEdgeFloats;
    for (int i = 0; i < q.n; ++i, e += kPoseEdgeFloats) {
      e[0] = q.p3d[3 * i], e[1] = q.p3d[3 * i + 1], e[2] = q.p3d[3 * i + 2];
      e[3] = q.p2d[2 * i], e[4] = q.p2d[2 * i + 1], e[5] = q.inv_sigma2[i];
    }
    off += q.n;
  }
  RC(o->send(total));
  const PoseDev D = {o->prob, o->items, o->chi2, o->state, o->trace, o->result, o->mask};
  hipLaunchKernelGGL(k_pose_optimize, dim3(n_problems), dim3(256), 0, o->stream, D);
  UVO_HIP_CHECK(hipGetLastError());
  RC(o->receive(total));
  o->last_n = n_problems;
  for (int j = 0; j < n_problems; ++j) {
    const poseopt::Out& r = o->h_res[j];
    std::memcpy(results[j].Tcw, r.Tcw, sizeof r.Tcw);
    results[j].n_inliers = r.n_inliers, results[j].rounds = r.rounds;
    if (results[j].outlier && problems[j].n > 0) std::memcpy(results[j].outlier, o->h_mask + o->h_prob[j].off, (size_t)problems[j].n);
  }
  return UVO_OK;
}

int uvo_pose_optimizer_trace(uvo_pose_optimizer* o, int problem, uvo_pose_trace* out) {
  return !o || !out ? fail(UVO_E_BADARG, "null pointer") : o->read_trace(problem, out);
}

}  // extern "C"
