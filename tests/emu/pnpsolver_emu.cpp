// Host build of the PnPsolver arithmetic (u-vip-slam_amd/csrc/pnpsolver_core.hpp over epnp_core.hpp): the same source the HIP kernels
// of pnpsolver.hip run, driven by one "lane", behind entry points of the C ABI's own shape (include/uvo/uvo.h, emu_ for uvo_) so that
// one test driver serves both.  Where the library draws every subset of a call up front, evaluates all hypotheses in one grid and
// replays the loop over the counts, this file walks src/PnPsolver.cc's iterate() as it is written: solver by solver, one hypothesis
// at a time, drawing as it goes and stopping where it returns.  The two have to agree bit for bit -- on the poses because the
// arithmetic is shared, on everything else because the library's reordering must not be observable.  Test scaffolding only.
// Build with -ffp-contract=off, as the library is.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/uvo/uvo.h"
#include "../../u-vip-slam_amd/csrc/pnpsolver_core.hpp"

using namespace uvo;

namespace {

struct Solver {
  int n = 0, n_matches = 0;
  pnps::Params prm;
  pnps::Derived d;
  double fu, fv, uc, vc;
  std::vector<float> p3d, p2d, max_err;
  std::vector<int32_t> kp;
  int iterations = 0, best_count = 0;  // mnIterations, mnBestInliers
  std::vector<uint8_t> best;           // mvbBestInliers
  double best_pose[12];
  std::vector<int32_t> tap_sub, tap_cnt;
  std::vector<double> tap_pose;
};

struct Set {
  int max_solvers, max_points;
  std::vector<Solver> v;
};

// compute_pose on the listed points + CheckInliers; false (and zero inliers) where EPnP gives no finite pose
int pose_and_inliers(const Solver& s, const int32_t* idx, int m, double* pose, std::vector<uint8_t>& inl) {
  double ws[pnp::W_SIZE];
  const pnp::PixelPoints P{s.p3d.data(), s.p2d.data(), idx, m, s.fu, s.fv, s.uc, s.vc};
  for (int e = 0; e < 12; ++e) pose[e] = 0.;
  inl.assign(s.n, 0);
  if (!pnp::solve(pnp::Ws<1>{ws}, P, 0, 1, pnp::NoSync(), pose)) return 0;
  int c = 0;
  for (int i = 0; i < s.n; ++i) {
    inl[i] = pnps::check_inlier(pose, pose + 9, &s.p3d[3 * i], &s.p2d[2 * i], s.fu, s.fv, s.uc, s.vc, s.max_err[i]) ? 1 : 0;
    c += inl[i];
  }
  return c;
}

void to_tcw(const double* pose, float* T) {
  for (int a = 0; a < 3; ++a) {
    for (int b = 0; b < 3; ++b) T[4 * a + b] = (float)pose[3 * a + b];
    T[4 * a + 3] = (float)pose[9 + a];
  }
  T[12] = T[13] = T[14] = 0.f, T[15] = 1.f;
}

// what pnps::replay asks of its caller, scripted: the refined count of the best set taken at hypothesis h is script[h], that of the
// set carried over from earlier calls is `carried`
struct ScriptOps {
  const int32_t* script;
  int carried, current, takes = 0, refines = 0;
  void take_best(int h) { current = script[h], ++takes; }
  int refine() { return ++refines, current; }
};

}  // namespace

extern "C" {

void emu_glibc_rand(uint32_t seed, int count, int32_t* out) {
  pnps::GlibcRand g;
  g.srand(seed);
  for (int i = 0; i < count; ++i) out[i] = g.next();
}

// `count` subsets over n points from the generator seeded with `seed`: out [count][min_set]
void emu_pnps_subsets(uint32_t seed, int n, int min_set, int count, int32_t* out) {
  pnps::GlibcRand g;
  g.srand(seed);
  std::vector<int32_t> avail(n);
  for (int h = 0; h < count; ++h) pnps::draw_subset(g, n, min_set, avail.data(), out + (size_t)h * min_set);
}

void emu_pnps_derive(int n, const uvo_pnpsolver_params* q, int32_t* out) {
  const pnps::Derived d = pnps::derive_params(n, pnps::Params{q->probability, q->min_inliers, q->max_iterations, q->min_set, q->epsilon, q->th2});
  out[0] = d.n, out[1] = d.min_inliers, out[2] = d.max_its;
}

void emu_pnps_check_inliers(const double* pose, const float* p3d, const float* p2d, const float* max_err, int n, double fu, double fv, double uc,
                            double vc, uint8_t* inl) {
  for (int i = 0; i < n; ++i) inl[i] = pnps::check_inlier(pose, pose + 9, p3d + 3 * i, p2d + 2 * i, fu, fv, uc, vc, max_err[i]) ? 1 : 0;
}

int emu_pnps_iterations_ahead(int iterations, int max_its, int n_iterations) { return pnps::iterations_ahead(iterations, max_its, n_iterations); }

// pnps::replay over given counts with scripted Refine outcomes.  state: {mnIterations, mnBestInliers} in and out;
// out: performed, returned, no_more, inliers, take_best calls, refine calls
void emu_pnps_replay(int32_t* state, const int32_t* counts, const int32_t* script, int carried, int n_iterations, int max_its, int min_inliers,
                     int32_t* out) {
  pnps::State st = {state[0], state[1]};
  ScriptOps ops{script, carried, carried};
  const pnps::Outcome o = pnps::replay(st, counts, n_iterations, max_its, min_inliers, ops);
  state[0] = st.iterations, state[1] = st.best_count;
  out[0] = o.performed, out[1] = o.returned, out[2] = o.no_more, out[3] = o.inliers, out[4] = ops.takes, out[5] = ops.refines;
}

// EPnP on the listed points as PnPsolver hands them over (pixel coordinates as they are)
int emu_pnps_epnp(const float* p3d, const float* p2d, const int32_t* idx, int m, double fu, double fv, double uc, double vc, double* pose) {
  double ws[pnp::W_SIZE];
  const pnp::PixelPoints P{p3d, p2d, idx, m, fu, fv, uc, vc};
  for (int e = 0; e < 12; ++e) pose[e] = 0.;
  return pnp::solve(pnp::Ws<1>{ws}, P, 0, 1, pnp::NoSync(), pose) ? 1 : 0;
}

// ---- the C ABI's entry points, on the host ---------------------------------------------------------------------------------------
int emu_pnpsolver_set_create(void*, int max_solvers, int max_points, void** out) {
  Set* s = new Set();
  s->max_solvers = max_solvers, s->max_points = max_points;
  *out = s;
  return 0;
}

void emu_pnpsolver_set_destroy(void* p) { delete static_cast<Set*>(p); }

int emu_pnpsolver_set_clear(void* p) {
  static_cast<Set*>(p)->v.clear();
  return 0;
}

int emu_pnpsolver_add(void* p, const float* p3d, const float* p2d, const float* sigma2, const int32_t* kp_index, int n, int n_matches, float fx,
                      float fy, float cx, float cy, const uvo_pnpsolver_params* q, int* id) {
  Set* S = static_cast<Set*>(p);
  if (n < 0 || n > S->max_points || (int)S->v.size() >= S->max_solvers || q->min_set < 4 || q->min_set > 8) return UVO_E_BADARG;
  Solver s;
  s.n = n, s.n_matches = n_matches;
  s.prm = pnps::Params{q->probability, q->min_inliers, q->max_iterations, q->min_set, q->epsilon, q->th2};
  s.d = n > 0 ? pnps::derive_params(n, s.prm) : pnps::Derived{0, q->min_inliers > q->min_set ? q->min_inliers : q->min_set, 1};
  s.fu = fx, s.fv = fy, s.uc = cx, s.vc = cy;
  s.p3d.assign(p3d, p3d + 3 * (size_t)n), s.p2d.assign(p2d, p2d + 2 * (size_t)n), s.kp.assign(kp_index, kp_index + n);
  s.max_err.resize(n);
  for (int i = 0; i < n; ++i) s.max_err[i] = sigma2[i] * q->th2;
  s.best.assign(n, 0);
  for (int e = 0; e < 12; ++e) s.best_pose[e] = 0.;
  *id = (int)S->v.size();
  S->v.push_back(s);
  return 0;
}

int emu_pnpsolver_query(void* p, int id, uvo_pnpsolver_info* info) {
  const Solver& s = static_cast<Set*>(p)->v[id];
  *info = uvo_pnpsolver_info{s.n, s.d.min_inliers, s.d.max_its, s.iterations, s.best_count};
  return 0;
}

int emu_pnpsolver_iterate(void* p, const int32_t* ids, int n_ids, int n_iterations, uvo_glibc_rand* rng, uvo_pnpsolver_result* res) {
  Set* S = static_cast<Set*>(p);
  pnps::GlibcRand& g = *reinterpret_cast<pnps::GlibcRand*>(rng);
  res->returned = -1, res->solver = -1, res->n_inliers = 0, res->refined = 0, res->draws = 0;
  for (int i = 0; i < 16; ++i) res->Tcw[i] = 0.f;
  for (Solver& s : S->v) s.tap_sub.clear(), s.tap_cnt.clear(), s.tap_pose.clear();
  for (int j = 0; j < n_ids; ++j)
    if (res->status) res->status[j] = uvo_pnpsolver_status{0, 0, S->v[ids[j]].iterations};
  std::vector<int32_t> avail(S->max_points);
  std::vector<uint8_t> inl, refined_inl;
  for (int j = 0; j < n_ids; ++j) {
    Solver& s = S->v[ids[j]];
    const int min_set = s.prm.min_set, min_inl = s.d.min_inliers;
    bool no_more = false;
    const uint8_t* ret_set = nullptr;
    double ret_pose[12];
    int ret_inliers = 0, refined = 0;
    // ---- PnPsolver::iterate, :166-259
    if (s.n < min_inl) {
      no_more = true;
    } else {
      int cur = 0;
      while (s.iterations < s.d.max_its || cur < n_iterations) {
        ++cur, ++s.iterations;
        int32_t sub[8];
        pnps::draw_subset(g, s.n, min_set, avail.data(), sub);
        res->draws += (uint32_t)min_set;
        double pose[12];
        const int c = pose_and_inliers(s, sub, min_set, pose, inl);
        s.tap_sub.insert(s.tap_sub.end(), sub, sub + min_set), s.tap_cnt.push_back(c), s.tap_pose.insert(s.tap_pose.end(), pose, pose + 12);
        if (c >= min_inl) {
          if (c > s.best_count) {
            s.best = inl, s.best_count = c;
            std::memcpy(s.best_pose, pose, sizeof pose);
          }
          // Refine(), :261-306
          std::vector<int32_t> list;
          for (int i = 0; i < s.n; ++i)
            if (s.best[i]) list.push_back(i);
          const int r = pose_and_inliers(s, list.data(), (int)list.size(), ret_pose, refined_inl);
          if (r > min_inl) {
            ret_set = refined_inl.data(), ret_inliers = r, refined = 1;
            break;
          }
        }
      }
      if (!ret_set && s.iterations >= s.d.max_its) {
        no_more = true;
        if (s.best_count >= min_inl) ret_set = s.best.data(), ret_inliers = s.best_count, std::memcpy(ret_pose, s.best_pose, sizeof ret_pose);
      }
    }
    if (res->status) res->status[j] = uvo_pnpsolver_status{1, no_more ? 1 : 0, s.iterations};
    if (!ret_set) continue;
    res->returned = j, res->solver = ids[j], res->n_inliers = ret_inliers, res->refined = refined;
    to_tcw(ret_pose, res->Tcw);
    if (res->inliers) {
      if (res->inliers_cap < s.n_matches) return UVO_E_CAPACITY;
      std::memset(res->inliers, 0, s.n_matches);
      for (int i = 0; i < s.n; ++i)
        if (ret_set[i]) res->inliers[s.kp[i]] = 1;
    }
    break;
  }
  return 0;
}

int emu_pnpsolver_hypotheses(void* p, int id, int32_t* subsets, double* poses, int32_t* counts, int cap, int* n) {
  const Solver& s = static_cast<Set*>(p)->v[id];
  const int m = (int)s.tap_cnt.size() < cap ? (int)s.tap_cnt.size() : cap;
  *n = m;
  if (m == 0) return 0;
  std::memcpy(subsets, s.tap_sub.data(), (size_t)m * s.prm.min_set * 4);
  std::memcpy(poses, s.tap_pose.data(), (size_t)m * 96);
  std::memcpy(counts, s.tap_cnt.data(), (size_t)m * 4);
  return 0;
}

}  // extern "C"
