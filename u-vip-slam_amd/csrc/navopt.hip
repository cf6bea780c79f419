// The two IMU overloads of Optimizer::PoseOptimization (src/Optimizer.cc:319-777, :779-1103) over a LIST of independent problems as one
// call.  All arithmetic and the whole control flow is navopt_core.hpp (navopt::run), shared with the host build tests/emu/navopt_emu.cpp;
// this file is the kernel around it and the host side of the C ABI.  The reduction over the reprojection edges is lane_team.hpp's
// LaneTeam; the handle's memory and the two copies of a call are opt_exchange.hpp's.
//
// One launch: k_nav_optimize, one workgroup of 256 lanes per problem, all four rounds.  A lane owns the edges l, l + 256, ... of the
// current frame and l, l + 256, ... of the last for the whole call: it alone reads and writes their chi2 and state bytes (LDS up to
// kNavLdsEdges edges, the set's block beyond).  Everything else -- the two NavStates, H, the factor, the right-hand sides, the stacked
// Jacobian of the single edges -- is navopt::Work in LDS, written through DevTeam::each: lane l runs the indices l, l + 256, ..., then
// one barrier.  All branches of navopt::run are uniform and there is no return before the last barrier.
#include <cstring>

#include "navopt.hpp"
#include "opt_exchange.hpp"

namespace uvo {

struct NavDev {
  const navopt::Problem* prob;  // [P]
  const float* edges;           // [sum (n + n_last)][6]
  double* chi2;                 // [P * 2N], used by problems above kNavLdsEdges
  uint8_t* state;               // [P * 2N]
  navopt::Trace* trace;         // [P]
  navopt::Out* result;          // [P]
  uint8_t* mask;                // [sum (n + n_last)]
};

struct DevTeam : LaneTeam<navopt::kSums> {
  template <class F>
  __device__ __forceinline__ void each(int count, F f) {
    for (int i = (int)threadIdx.x; i < count; i += navopt::kLanes) f(i);
    __syncthreads();
  }
};

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void k_nav_optimize(NavDev D) {
  __shared__ navopt::Work s_work;
  __shared__ double s_chi2[kNavLdsEdges];
  __shared__ double s_red[2 * 4 * navopt::kSums];
  __shared__ double s_store[navopt::kSums];
  __shared__ int32_t s_redi[2 * 4];
  __shared__ uint8_t s_state[kNavLdsEdges];
  const navopt::Problem& p = D.prob[blockIdx.x];
  const int nall = p.n + (p.form == navopt::kFrame ? p.n_last : 0);
  const bool in_lds = nall <= kNavLdsEdges;  // uniform
  navopt::Edges E;
  E.in = D.edges + (size_t)p.off * kNavEdgeFloats;
  E.chi2 = in_lds ? s_chi2 : D.chi2 + p.off;
  E.state = in_lds ? s_state : D.state + p.off;
  E.mask = D.mask + p.off;
  DevTeam T;
  T.red = s_red, T.redi = s_redi, T.store = s_store, T.phase = 0;
  navopt::run<navopt::kMutNone>(T, p, E, s_work, D.result + blockIdx.x, D.trace + blockIdx.x);
}

}  // namespace uvo

// ---------------------------------------------------------------------------------------------------------------------------
using namespace uvo;

static_assert(sizeof(uvo_nav_trace) == sizeof(navopt::Trace) && sizeof(uvo_nav_trace_lin) == sizeof(navopt::TraceLin), "uvo_nav_trace is navopt::Trace");
static_assert(sizeof(uvo_nav_state) == sizeof(navopt::State), "uvo_nav_state is navopt::State");

struct uvo_nav_optimizer : OptExchange<navopt::Problem, navopt::Out, navopt::Trace> {};  // items: edges, on the KLT handle's stream

namespace {
void pack_edges(float* e, const float* p3d, const float* p2d, const float* w, int n) {
  for (int i = 0; i < n; ++i, e += kNavEdgeFloats) {
    e[0] = p3d[3 * i], e[1] = p3d[3 * i + 1], e[2] = p3d[3 * i + 2];
    e[3] = p2d[2 * i], e[4] = p2d[2 * i + 1], e[5] = w[i];
  }
}
}  // namespace

extern "C" {

void uvo_nav_optimizer_destroy(uvo_nav_optimizer* o) {
  if (!o) return;
  o->destroy();
  delete o;
}

int uvo_nav_optimizer_create(uvo_klt* k, int max_problems, int max_points, uvo_nav_optimizer** out) {
  if (!k || !out) return fail(UVO_E_BADARG, "null pointer");
  *out = nullptr;
  if (max_problems < 1 || max_problems > kNavMaxProblems || max_points < 1 || max_points > kNavMaxPoints)
    return fail(UVO_E_BADARG, "nav optimizer: 1..64 problems of 1..16384 points a frame");
  uvo_nav_optimizer* o = new uvo_nav_optimizer();
  const int rc = o->create(klt_device(k), klt_stream(k), max_problems, 2 * max_points, kNavEdgeFloats, 1, "nav optimizer allocation failed");
  if (rc) return uvo_nav_optimizer_destroy(o), rc;
  *out = o;
  return UVO_OK;
}

int uvo_nav_optimize(uvo_nav_optimizer* o, const uvo_nav_problem* problems, int n_problems, uvo_nav_result* results) {
  if (!o) return fail(UVO_E_BADARG, "null handle");
  if (n_problems < 0) return fail(UVO_E_BADARG, "negative problem count");
  if (n_problems > o->max_problems) return fail(UVO_E_CAPACITY, "more problems than the nav optimizer was sized for");
  if (n_problems > 0 && (!problems || !results)) return fail(UVO_E_BADARG, "null pointer");
  const int max_points = o->max_items / 2;
  size_t total = 0;
  for (int j = 0; j < n_problems; ++j) {
    const uvo_nav_problem& q = problems[j];
    if (q.form != UVO_NAV_KEYFRAME && q.form != UVO_NAV_FRAME) return fail(UVO_E_BADARG, "form is neither UVO_NAV_KEYFRAME nor UVO_NAV_FRAME");
    const int nl = q.form == UVO_NAV_FRAME ? q.n_last : 0;
    if (q.n < 0 || nl < 0) return fail(UVO_E_BADARG, "negative point count");
    if (q.n > max_points || nl > max_points) return fail(UVO_E_CAPACITY, "more points than the nav optimizer was sized for");
    if (q.n > 0 && (!q.p3d || !q.p2d || !q.inv_sigma2)) return fail(UVO_E_BADARG, "null pointer");
    if (nl > 0 && (!q.p3d_last || !q.p2d_last || !q.inv_sigma2_last)) return fail(UVO_E_BADARG, "null pointer");
    if (results[j].outlier && results[j].outlier_cap < q.n) return fail(UVO_E_CAPACITY, "outlier_cap is smaller than the problem's n");
    if (results[j].outlier_last && results[j].outlier_last_cap < nl) return fail(UVO_E_CAPACITY, "outlier_last_cap is smaller than the problem's n_last");
    total += (size_t)q.n + (size_t)nl;
  }
  if (n_problems == 0) return UVO_OK;
  int off = 0;
  for (int j = 0; j < n_problems; ++j) {
    const uvo_nav_problem& q = problems[j];
    navopt::Problem& r = o->h_prob[j];
    const int nl = q.form == UVO_NAV_FRAME ? q.n_last : 0;
    r.form = q.form, r.has_depth = q.has_depth ? 1 : 0, r.compute_marg = q.compute_marg ? 1 : 0, r.n = q.n, r.n_last = nl, r.off = off;
    r.pad_[0] = r.pad_[1] = 0;
    std::memcpy(&r.cur, &q.cur, sizeof r.cur), std::memcpy(&r.last, &q.last, sizeof r.last), std::memcpy(&r.prior, &q.prior, sizeof r.prior);
    r.dT = q.dT;
    std::memcpy(r.dP, q.dP, sizeof r.dP), std::memcpy(r.dV, q.dV, sizeof r.dV), std::memcpy(r.dR, q.dR, sizeof r.dR);
    std::memcpy(r.JPg, q.JPg, sizeof r.JPg), std::memcpy(r.JPa, q.JPa, sizeof r.JPa), std::memcpy(r.JVg, q.JVg, sizeof r.JVg);
    std::memcpy(r.JVa, q.JVa, sizeof r.JVa), std::memcpy(r.JRg, q.JRg, sizeof r.JRg), std::memcpy(r.cov, q.cov_pvphi, sizeof r.cov);
    std::memcpy(r.gw, q.gw, sizeof r.gw), std::memcpy(r.Rbc, q.Rbc, sizeof r.Rbc), std::memcpy(r.Pbc, q.Pbc, sizeof r.Pbc);
    r.fx = q.fx, r.fy = q.fy, r.cx = q.cx, r.cy = q.cy, r.gyr_rw2 = q.gyr_bias_rw2, r.acc_rw2 = q.acc_bias_rw2;
    std::memcpy(r.prior_info, q.prior_info, sizeof r.prior_info);
    r.depth_meas = q.depth_meas, r.shi = q.shi, r.depth_info = q.depth_info;
    float* e = o->h_items + (size_t)off * kNavEdgeFloats;
    pack_edges(e, q.p3d, q.p2d, q.inv_sigma2, q.n);
    pack_edges(e + (size_t)q.n * kNavEdgeFloats, q.p3d_last, q.p2d_last, q.inv_sigma2_last, nl);
    off += q.n + nl;
  }
  RC(o->send(total));
  const NavDev D = {o->prob, o->items, o->chi2, o->state, o->trace, o->result, o->mask};
  hipLaunchKernelGGL(k_nav_optimize, dim3(n_problems), dim3(256), 0, o->stream, D);
  UVO_HIP_CHECK(hipGetLastError());
  RC(o->receive(total));
  o->last_n = n_problems;
  for (int j = 0; j < n_problems; ++j) {
    const navopt::Out& r = o->h_res[j];
    const navopt::Problem& q = o->h_prob[j];
    uvo_nav_result& w = results[j];
    std::memcpy(&w.ns, &r.ns, sizeof w.ns);
    std::memcpy(w.Tcw, r.Tcw, sizeof r.Tcw);
    w.n_inliers = r.n_inliers, w.rounds = r.rounds, w.marg_ok = r.marg_ok;
    std::memcpy(w.marg_cov, r.marg_cov, sizeof r.marg_cov), std::memcpy(w.marg_cov_inv, r.marg_cov_inv, sizeof r.marg_cov_inv);
    if (w.outlier && q.n > 0) std::memcpy(w.outlier, o->h_mask + q.off, (size_t)q.n);
    if (w.outlier_last && q.n_last > 0) std::memcpy(w.outlier_last, o->h_mask + q.off + q.n, (size_t)q.n_last);
  }
  return UVO_OK;
}

int uvo_nav_optimizer_trace(uvo_nav_optimizer* o, int problem, uvo_nav_trace* out) {
  return !o || !out ? fail(UVO_E_BADARG, "null pointer") : o->read_trace(problem, out);
}

}  // extern "C"
