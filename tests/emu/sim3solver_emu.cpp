// Host build of the Sim3Solver arithmetic (u-vip-slam_amd/csrc/sim3_core.hpp): the same source the HIP kernels of sim3solver.hip run,
// driven by one "lane", behind entry points of the C ABI's own shape (include/uvo/uvo.h, emu_ for uvo_) so that one test driver serves
// both.  Where the library draws every subset of a call up front, evaluates all hypotheses in one grid and replays the loop over the
// counts, this file walks src/Sim3Solver.cc's iterate() as it is written: solver by solver, one hypothesis at a time, drawing as it
// goes and stopping where it returns.  The two have to agree bit for bit -- on the transforms because the arithmetic is shared, on
// everything else because the library's reordering must not be observable.  Test scaffolding only.
// Build with -ffp-contract=off, as the library is.
//
// Four seeded mutations exist behind -D switches of THIS file only (the library has none), to show that the checks of
// tests/sim3_checks.py can fail: SIM3_MUT_OR (the loop's AND as an OR), SIM3_MUT_GT (> for >= at the best update),
// SIM3_MUT_THRESHOLD (the threshold not truncated), SIM3_MUT_DRAW (the draw removing the slot by position).
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/uvo/uvo.h"
#include "../../u-vip-slam_amd/csrc/sim3_core.hpp"

using namespace uvo;

namespace {

struct Solver {
  int n = 0, n_matches = 0, max_its = 1;
  sim3::Params prm;
  sim3::Cam K1, K2;
  std::vector<float> x1c, x2c, p1, p2, e1, e2;
  std::vector<int32_t> index1;
  int iterations = 0, best_count = 0;  // mnIterations, mnBestInliers
  std::vector<uint8_t> best;           // mvbBestInliers
  sim3::Hyp best_hyp;                  // mBestT12, mBestRotation, mBestTranslation, mBestScale
  std::vector<int32_t> tap_sub, tap_cnt;
  std::vector<float> tap_t12, tap_t21;
};

struct Set {
  int max_solvers, max_points;
  std::vector<Solver> v;
};

float threshold(float sigma2) {
#ifdef SIM3_MUT_THRESHOLD
  return (float)(9.210 * (double)sigma2);
#else
  return sim3::max_error(sigma2);
#endif
}

void draw(pnps::GlibcRand& g, int n, int32_t* avail, int32_t* out) {
#ifdef SIM3_MUT_DRAW
  for (int i = 0; i < n; ++i) avail[i] = i;
  int live = n;
  for (int i = 0; i < 3; ++i) {
    const int randi = pnps::random_int(g, 0, live - 1);
    out[i] = avail[randi];
    avail[randi] = avail[live - 1];
    --live;
  }
#else
  pnps::draw_subset(g, n, sim3::kMinSet, avail, out);
#endif
}

void hypothesis(const float* x1c, const float* x2c, const int32_t* idx, sim3::Hyp& H) {
  float f[sim3::kWsFloats];
  int32_t i[sim3::kWsInts];
  float P1[3][3], P2[3][3];
  for (int k = 0; k < 3; ++k)
    for (int r = 0; r < 3; ++r) P1[r][k] = x1c[3 * idx[k] + r], P2[r][k] = x2c[3 * idx[k] + r];
  sim3::compute_t(sim3::Ws<1>{f, i}, P1, P2, H);
  if (!H.finite) {
    std::memset(&H, 0, sizeof H);
  }
}

// computeT + CheckInliers on the drawn triple; zero inliers where the transform is not finite
int hypothesis_and_inliers(const Solver& s, const int32_t* idx, sim3::Hyp& H, std::vector<uint8_t>& inl) {
  hypothesis(s.x1c.data(), s.x2c.data(), idx, H);
  inl.assign(s.n, 0);
  if (!H.finite) return 0;
  int c = 0;
  for (int i = 0; i < s.n; ++i) {
    inl[i] = sim3::check_inlier(H.T12, H.T21, &s.x1c[3 * i], &s.x2c[3 * i], &s.p1[2 * i], &s.p2[2 * i], s.K1, s.K2, s.e1[i], s.e2[i]) ? 1 : 0;
    c += inl[i];
  }
  return c;
}

int max_its_of(int n, const sim3::Params& p) { return n >= sim3::kMinSet ? sim3::derive_max_its(n, p) : 1; }

}  // namespace

extern "C" {

int emu_sim3_derive(int n, const uvo_sim3solver_params* q) { return sim3::derive_max_its(n, sim3::Params{q->probability, q->min_inliers, q->max_iterations}); }

float emu_sim3_max_error(float sigma2) { return threshold(sigma2); }

// `count` triples over n points from the generator seeded with `seed`: out [count][3]
void emu_sim3_subsets(uint32_t seed, int n, int count, int32_t* out) {
  pnps::GlibcRand g;
  g.srand(seed);
  std::vector<int32_t> avail(n);
  for (int h = 0; h < count; ++h) draw(g, n, avail.data(), out + (size_t)h * 3);
}

// the constructor's per-point work: xc [n][3] = Rcw xw + tcw, uv [n][2] = FromCameraToImage
void emu_sim3_prepare(const uvo_sim3_keyframe* kf, const float* xw, int n, float* xc, float* uv) {
  const sim3::Cam K{kf->fx, kf->fy, kf->cx, kf->cy};
  for (int i = 0; i < n; ++i) {
    sim3::transform(kf->Rcw, 3, kf->tcw[0], kf->tcw[1], kf->tcw[2], xw + 3 * i, xc + 3 * i);
    sim3::to_image(xc + 3 * i, K, uv + 2 * i);
  }
}

// computeT on the three listed points: out T12[16], T21[16], R[9], t[3], s; returns 1 where every element is finite (zeros otherwise)
int emu_sim3_compute_t(const float* x1c, const float* x2c, const int32_t* idx, float* out) {
  sim3::Hyp H;
  hypothesis(x1c, x2c, idx, H);
  std::memcpy(out, H.T12, 64), std::memcpy(out + 16, H.T21, 64), std::memcpy(out + 32, H.R, 36), std::memcpy(out + 41, H.t, 12);
  out[44] = H.s;
  return H.finite;
}

void emu_sim3_check_inliers(const float* T12, const float* T21, const float* x1c, const float* x2c, const float* p1, const float* p2, const float* e1,
                            const float* e2, int n, const float* K1, const float* K2, uint8_t* inl) {
  const sim3::Cam A{K1[0], K1[1], K1[2], K1[3]}, B{K2[0], K2[1], K2[2], K2[3]};
  for (int i = 0; i < n; ++i) inl[i] = sim3::check_inlier(T12, T21, x1c + 3 * i, x2c + 3 * i, p1 + 2 * i, p2 + 2 * i, A, B, e1[i], e2[i]) ? 1 : 0;
}

int emu_sim3_iterations_ahead(int iterations, int max_its, int n_iterations) { return sim3::iterations_ahead(iterations, max_its, n_iterations); }

// sim3::replay over given counts.  state: {mnIterations, mnBestInliers} in and out; out: performed, returned, no_more, inliers, best_from
void emu_sim3_replay(int32_t* state, const int32_t* counts, int n_iterations, int max_its, int min_inliers, int32_t* out) {
  sim3::State st = {state[0], state[1]};
  const sim3::Outcome o = sim3::replay(st, counts, n_iterations, max_its, min_inliers);
  state[0] = st.iterations, state[1] = st.best_count;
  out[0] = o.performed, out[1] = o.returned, out[2] = o.no_more, out[3] = o.inliers, out[4] = o.best_from;
}

void emu_sim3_sincos(int n, const double* th, double* s, double* c) {
  for (int i = 0; i < n; ++i) sim3::sincos(th[i], s + i, c + i);
}
void emu_sim3_atan2_pos(int n, const double* y, const double* x, double* out) {
  for (int i = 0; i < n; ++i) out[i] = sim3::atan2_pos(y[i], x[i]);
}
// the rotation of n float quaternions (w, x, y, z) as computeT builds it: R [n][9]
void emu_sim3_rotation(int n, const float* q, float* R) {
  for (int i = 0; i < n; ++i) sim3::quaternion_to_rotation(q[4 * i], q[4 * i + 1], q[4 * i + 2], q[4 * i + 3], R + 9 * (size_t)i);
}

// ---- the C ABI's entry points, on the host ---------------------------------------------------------------------------------------
int emu_sim3solver_set_create(void*, int max_solvers, int max_points, void** out) {
  if (max_solvers < 1 || max_solvers > 64 || max_points < 3 || max_points > 16384) return UVO_E_BADARG;
  Set* s = new Set();
  s->max_solvers = max_solvers, s->max_points = max_points;
  *out = s;
  return 0;
}

void emu_sim3solver_set_destroy(void* p) { delete static_cast<Set*>(p); }

int emu_sim3solver_set_clear(void* p) {
  static_cast<Set*>(p)->v.clear();
  return 0;
}

int emu_sim3solver_add(void* p, const float* x1w, const float* x2w, const float* sigma2_1, const float* sigma2_2, const int32_t* index1, int n,
                       int n_matches, const uvo_sim3_keyframe* kf1, const uvo_sim3_keyframe* kf2, const uvo_sim3solver_params* q, int* id) {
  Set* S = static_cast<Set*>(p);
  if (n < 0 || n > S->max_points || n_matches < n || (int)S->v.size() >= S->max_solvers) return UVO_E_BADARG;
  if (!(q->probability > 0. && q->probability < 1.) || q->min_inliers < 0 || q->max_iterations < 1 || q->max_iterations > 320) return UVO_E_BADARG;
  Solver s;
  s.n = n, s.n_matches = n_matches;
  s.prm = sim3::Params{q->probability, q->min_inliers, q->max_iterations};
  s.max_its = max_its_of(n, s.prm);
  s.K1 = sim3::Cam{kf1->fx, kf1->fy, kf1->cx, kf1->cy}, s.K2 = sim3::Cam{kf2->fx, kf2->fy, kf2->cx, kf2->cy};
  s.x1c.resize(3 * (size_t)n), s.x2c.resize(3 * (size_t)n), s.p1.resize(2 * (size_t)n), s.p2.resize(2 * (size_t)n), s.e1.resize(n), s.e2.resize(n);
  emu_sim3_prepare(kf1, x1w, n, s.x1c.data(), s.p1.data());
  emu_sim3_prepare(kf2, x2w, n, s.x2c.data(), s.p2.data());
  for (int i = 0; i < n; ++i) s.e1[i] = threshold(sigma2_1[i]), s.e2[i] = threshold(sigma2_2[i]);
  s.index1.assign(index1, index1 + n);
  s.best.assign(n, 0);
  std::memset(&s.best_hyp, 0, sizeof s.best_hyp);
  *id = (int)S->v.size();
  S->v.push_back(s);
  return 0;
}

int emu_sim3solver_set_ransac_parameters(void* p, int id, const uvo_sim3solver_params* q) {
  Set* S = static_cast<Set*>(p);
  if (id < 0 || id >= (int)S->v.size()) return UVO_E_BADARG;
  if (!(q->probability > 0. && q->probability < 1.) || q->min_inliers < 0 || q->max_iterations < 1 || q->max_iterations > 320) return UVO_E_BADARG;
  Solver& s = S->v[id];
  s.prm = sim3::Params{q->probability, q->min_inliers, q->max_iterations};
  s.max_its = max_its_of(s.n, s.prm);
  s.iterations = 0;
  return 0;
}

int emu_sim3solver_query(void* p, int id, uvo_sim3solver_info* info) {
  const Solver& s = static_cast<Set*>(p)->v[id];
  *info = uvo_sim3solver_info{s.n, s.max_its, s.iterations, s.best_count};
  return 0;
}

int emu_sim3solver_iterate(void* p, const int32_t* ids, int n_ids, int n_iterations, uvo_glibc_rand* rng, uvo_sim3solver_result* res) {
  Set* S = static_cast<Set*>(p);
  if (n_iterations < 1 || n_ids < 0 || n_ids > S->max_solvers) return UVO_E_BADARG;
  pnps::GlibcRand& g = *reinterpret_cast<pnps::GlibcRand*>(rng);
  res->returned = -1, res->solver = -1, res->n_inliers = 0, res->draws = 0, res->scale = 0.f;
  std::memset(res->T12, 0, sizeof res->T12), std::memset(res->R12, 0, sizeof res->R12), std::memset(res->t12, 0, sizeof res->t12);
  for (int j = 0; j < n_ids; ++j) {
    if (ids[j] < 0 || ids[j] >= (int)S->v.size()) return UVO_E_BADARG;
    for (int k = 0; k < j; ++k)
      if (ids[k] == ids[j]) return UVO_E_BADARG;
    if (res->inliers && res->inliers_cap < S->v[ids[j]].n_matches) return UVO_E_CAPACITY;
  }
  for (Solver& s : S->v) s.tap_sub.clear(), s.tap_cnt.clear(), s.tap_t12.clear(), s.tap_t21.clear();
  for (int j = 0; j < n_ids; ++j)
    if (res->status) res->status[j] = uvo_sim3solver_status{0, 0, S->v[ids[j]].iterations};
  std::vector<int32_t> avail(S->max_points);
  std::vector<uint8_t> inl;
  for (int j = 0; j < n_ids; ++j) {
    Solver& s = S->v[ids[j]];
    bool no_more = false, returned = false;
    // ---- Sim3Solver::iterate, :140-207
    if (s.n < s.prm.min_inliers || s.n < sim3::kMinSet) {
      no_more = true;
    } else {
      int cur = 0;
#ifdef SIM3_MUT_OR
      while (s.iterations < s.max_its || cur < n_iterations) {
#else
      while (s.iterations < s.max_its && cur < n_iterations) {
#endif
        ++cur, ++s.iterations;
        int32_t sub[3];
        draw(g, s.n, avail.data(), sub);
        res->draws += 3u;
        sim3::Hyp H;
        const int c = hypothesis_and_inliers(s, sub, H, inl);
        s.tap_sub.insert(s.tap_sub.end(), sub, sub + 3), s.tap_cnt.push_back(c);
        s.tap_t12.insert(s.tap_t12.end(), H.T12, H.T12 + 16), s.tap_t21.insert(s.tap_t21.end(), H.T21, H.T21 + 16);
#ifdef SIM3_MUT_GT
        if (c > s.best_count) {
#else
        if (c >= s.best_count) {
#endif
          s.best = inl, s.best_count = c, s.best_hyp = H;
          if (c > s.prm.min_inliers) {
            returned = true;
            break;
          }
        }
      }
      if (!returned && s.iterations >= s.max_its) no_more = true;
    }
    if (res->status) res->status[j] = uvo_sim3solver_status{1, no_more ? 1 : 0, s.iterations};
    if (!returned) continue;
    res->returned = j, res->solver = ids[j], res->n_inliers = s.best_count;
    std::memcpy(res->T12, s.best_hyp.T12, 64), std::memcpy(res->R12, s.best_hyp.R, 36), std::memcpy(res->t12, s.best_hyp.t, 12);
    res->scale = s.best_hyp.s;
    if (res->inliers) {
      std::memset(res->inliers, 0, s.n_matches);
      for (int i = 0; i < s.n; ++i)
        if (s.best[i]) res->inliers[s.index1[i]] = 1;
    }
    break;
  }
  return 0;
}

int emu_sim3solver_find(void* p, int id, uvo_glibc_rand* rng, uvo_sim3solver_result* res) {
  Set* S = static_cast<Set*>(p);
  if (id < 0 || id >= (int)S->v.size()) return UVO_E_BADARG;
  const int32_t ids[1] = {id};
  return emu_sim3solver_iterate(p, ids, 1, S->v[id].max_its, rng, res);
}

int emu_sim3solver_hypotheses(void* p, int id, int32_t* subsets, float* T12, float* T21, int32_t* counts, int cap, int* n) {
  const Solver& s = static_cast<Set*>(p)->v[id];
  const int m = (int)s.tap_cnt.size() < cap ? (int)s.tap_cnt.size() : cap;
  *n = m;
  if (m == 0) return 0;
  std::memcpy(subsets, s.tap_sub.data(), (size_t)m * 12);
  std::memcpy(T12, s.tap_t12.data(), (size_t)m * 64);
  std::memcpy(T21, s.tap_t21.data(), (size_t)m * 64);
  std::memcpy(counts, s.tap_cnt.data(), (size_t)m * 4);
  return 0;
}

}  // extern "C"
