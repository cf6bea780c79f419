// Host build of the two-view initialisation arithmetic (u-vip-slam_amd/csrc/initializer_core.hpp): the same source the HIP kernels of
// initializer.hip run, driven by one "lane", behind entry points of the C ABI's own shape (include/uvo/uvo.h, emu_ for uvo_) so that
// one test driver serves both.  Where the library evaluates every hypothesis in one grid, sums the score terms from LDS, picks the
// maximum in a tree and selects the parallax order statistic bit by bit, this file walks src/Initializer.cc's Initialize() as it is
// written: FindFundamental's loop with its running best, CheckRT four times with std::sort.  The two have to agree bit for bit -- on
// the matrices because the arithmetic is shared, on everything else because the library's reordering must not be observable.  Test
// scaffolding only.  Build with -ffp-contract=off, as the library is.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/uvo/uvo.h"
#include "../../u-vip-slam_amd/csrc/initializer_core.hpp"

using namespace uvo;

namespace {

struct Init {
  int max_keys = 0, n1 = 0, iterations = 0;
  bool ready = false;
  float sigma = 1.f;
  twoview::Cam K;
  twoview::Norm N1;
  std::vector<float> keys1;
  std::vector<int32_t> tap_sets;
  std::vector<float> tap_F, tap_score;
};

struct Lane {
  float f[twoview::kWsFloats];
  double d[twoview::kWsDoubles];
  twoview::Ws<1> ws() { return twoview::Ws<1>{f, d}; }
};

}  // namespace

extern "C" {

int emu_initializer_create(void*, int max_keys, void** out) {
  if (!out || max_keys < twoview::kSet || max_keys > 16384) return UVO_E_BADARG;
  Init* s = new Init();
  s->max_keys = max_keys;
  *out = s;
  return UVO_OK;
}

void emu_initializer_destroy(void* h) { delete static_cast<Init*>(h); }

int emu_initializer_set_reference(void* h, const float* keys1_xy, int n1, const uvo_camera_model* cam, float sigma, int iterations) {
  Init* s = static_cast<Init*>(h);
  if (!s || !keys1_xy || !cam) return UVO_E_BADARG;
  if (n1 < 1 || n1 > s->max_keys || iterations < 1 || iterations > 1024 || !(sigma > 0.f) || !(sigma <= 1e6f)) return UVO_E_BADARG;
  s->keys1.assign(keys1_xy, keys1_xy + 2 * (size_t)n1);
  s->N1 = twoview::normalize(keys1_xy, n1);
  s->K = twoview::Cam{cam->fx, cam->fy, cam->cx, cam->cy};
  s->n1 = n1, s->sigma = sigma, s->iterations = iterations, s->ready = true;
  s->tap_sets.clear(), s->tap_F.clear(), s->tap_score.clear();
  return UVO_OK;
}

int emu_initializer_initialize(void* h, const float* keys2, int n2, const int32_t* matches12, uvo_glibc_rand* rng, uvo_initializer_result* result) {
  Init* s = static_cast<Init*>(h);
  if (!s || !rng || !result || !s->ready || n2 < 0 || n2 > s->max_keys || (n2 > 0 && (!keys2 || !matches12))) return UVO_E_BADARG;
  for (int i = 0; i < n2; ++i)
    if (matches12[i] < 0 || matches12[i] >= s->n1) return UVO_E_BADARG;
  uint8_t *inl = result->inliers, *tri = result->triangulated;
  float* p3d = result->p3d;
  std::memset(result, 0, sizeof *result);
  result->inliers = inl, result->p3d = p3d, result->triangulated = tri;
  result->best = -1, result->deciding = -1;
  s->tap_sets.clear(), s->tap_F.clear(), s->tap_score.clear();
  if (inl) std::memset(inl, 0, (size_t)n2);
  if (tri) std::memset(tri, 0, (size_t)n2);
  if (p3d) std::memset(p3d, 0, (size_t)n2 * 12);
  if (n2 < twoview::kSet) return UVO_OK;
  const int N = n2, T = s->iterations;
  const float* keys1 = s->keys1.data();
  pnps::GlibcRand* g = reinterpret_cast<pnps::GlibcRand*>(rng);
  // :63-90 every set, drawing as it goes
  std::vector<int32_t> avail((size_t)N), sets((size_t)T * 8);
  for (int it = 0; it < T; ++it) twoview::draw_set(*g, N, avail.data(), &sets[(size_t)it * 8]);
  result->draws = (uint32_t)(T * 8);
  // FindFundamental :167-215
  const twoview::Norm N1 = s->N1, N2 = twoview::normalize(keys2, n2);
  const float invSigmaSquare = twoview::inv_sigma_square(s->sigma);
  float score = 0.f, F21[9] = {0};
  std::vector<uint8_t> best_in, cur((size_t)N);
  Lane lane;
  s->tap_sets = sets;
  s->tap_F.resize((size_t)T * 9), s->tap_score.resize((size_t)T);
  for (int it = 0; it < T; ++it) {
    for (int j = 0; j < 8; ++j) {
      const int idx = sets[(size_t)it * 8 + j], i1 = matches12[idx];
      float u1, v1, u2, v2;
      twoview::normalized(N1, keys1[2 * i1], keys1[2 * i1 + 1], &u1, &v1);
      twoview::normalized(N2, keys2[2 * idx], keys2[2 * idx + 1], &u2, &v2);
      twoview::set_row(lane.ws(), j, u1, v1, u2, v2);
    }
    float F[9];
    twoview::f21_from_rows(lane.ws(), N1, N2, F);
    float currentScore = 0.f;  // CheckFundamental :381-460
    for (int i = 0; i < N; ++i) {
      const int i1 = matches12[i];
      float t1, t2;
      const bool bIn = twoview::score_terms(F, keys1[2 * i1], keys1[2 * i1 + 1], keys2[2 * i], keys2[2 * i + 1], invSigmaSquare, &t1, &t2);
      currentScore += t1;  // + 0.f where the reference adds nothing: the same bits (the score is never -0)
      currentScore += t2;
      cur[i] = bIn ? 1 : 0;
    }
    std::memcpy(&s->tap_F[(size_t)it * 9], F, 36);
    s->tap_score[it] = currentScore;
    if (currentScore > score) {
      std::memcpy(F21, F, 36);
      best_in = cur;
      score = currentScore;
      result->best = it;
    }
  }
  if (result->best < 0) return UVO_OK;  // departure (2): the reference would index an empty vector
  result->score = score;
  std::memcpy(result->F21, F21, 36);
  // ReconstructF :462-562
  int Nin = 0;
  for (int i = 0; i < N; ++i) Nin += best_in[i];
  result->n_inliers = Nin;
  if (inl) std::memcpy(inl, best_in.data(), (size_t)N);
  twoview::Motion M;
  twoview::decompose_e(lane.ws(), F21, s->K, M);
  const float th2 = twoview::th2_of(s->sigma);
  std::vector<float> P[4];
  std::vector<uint8_t> G[4];
  for (int k = 0; k < 4; ++k) {  // CheckRT :790-904
    float R[9], t[3];
    twoview::motion_of(M, k, R, t);
    P[k].assign((size_t)N * 3, 0.f), G[k].assign((size_t)N, 0);
    std::vector<float> vCosParallax;
    int nGood = 0;
    for (int i = 0; i < N; ++i) {
      if (!best_in[i]) continue;
      const int i1 = matches12[i];
      float X[3], c;
      const int f = twoview::check_rt_one(lane.ws(), R, t, s->K, keys1[2 * i1], keys1[2 * i1 + 1], keys2[2 * i], keys2[2 * i + 1], th2, X, &c);
      if (!(f & twoview::kCounted)) continue;
      vCosParallax.push_back(c);
      std::memcpy(&P[k][(size_t)i * 3], X, 12);
      ++nGood;
      if (f & twoview::kGood) G[k][i] = 1;
    }
    float parallax = 0.f;
    if (nGood > 0) {
      std::sort(vCosParallax.begin(), vCosParallax.end());
      const size_t idx = (size_t)std::min(50, (int)vCosParallax.size() - 1);
      parallax = twoview::parallax_deg(vCosParallax[idx]);
    }
    result->n_good[k] = nGood, result->parallax[k] = parallax;
  }
  const twoview::Verdict v = twoview::verdict_of(Nin, result->n_good, result->parallax);
  result->deciding = v.deciding, result->initialized = v.ok;
  if (v.ok) {
    float R[9], t[3];
    twoview::motion_of(M, v.deciding, R, t);
    std::memcpy(result->R21, R, 36);
    std::memcpy(result->t21, t, 12);
    if (p3d) std::memcpy(p3d, P[v.deciding].data(), (size_t)N * 12);
    if (tri) std::memcpy(tri, G[v.deciding].data(), (size_t)N);
  }
  return UVO_OK;
}

int emu_initializer_hypotheses(void* h, int32_t* subsets, float* F, float* scores, int cap, int* n) {
  Init* s = static_cast<Init*>(h);
  if (!s || !n || cap < 0) return UVO_E_BADARG;
  const int have = (int)s->tap_score.size(), m = cap < have ? cap : have;
  *n = m;
  if (m == 0) return UVO_OK;
  if (!subsets || !F || !scores) return UVO_E_BADARG;
  std::memcpy(subsets, s->tap_sets.data(), (size_t)m * 32);
  std::memcpy(F, s->tap_F.data(), (size_t)m * 36);
  std::memcpy(scores, s->tap_score.data(), (size_t)m * 4);
  return UVO_OK;
}

// pieces for the layer tests: one ComputeF21 + denormalisation on already normalised points, the completion row, acos, the draw
void emu_init_compute_f21(const float* pn1, const float* pn2, const float* norm1, const float* norm2, float* F, float* fpre) {
  Lane lane;
  for (int j = 0; j < 8; ++j) twoview::set_row(lane.ws(), j, pn1[2 * j], pn1[2 * j + 1], pn2[2 * j], pn2[2 * j + 1]);
  twoview::Norm A{norm1[0], norm1[1], norm1[2], norm1[3]}, B{norm2[0], norm2[1], norm2[2], norm2[3]};
  Lane l2 = lane;
  twoview::jacobi_svd(l2.ws(), 9, 8, 9, false);
  for (int e = 0; e < 9; ++e) fpre[e] = l2.ws().A(8, e);
  twoview::f21_from_rows(lane.ws(), A, B, F);
}
void emu_init_normalize(const float* xy, int n, float* out) {
  const twoview::Norm T = twoview::normalize(xy, n);
  out[0] = T.meanX, out[1] = T.meanY, out[2] = T.sX, out[3] = T.sY;
}
void emu_init_acos(int n, const double* x, double* out) {
  for (int i = 0; i < n; ++i) out[i] = twoview::acos_ieee(x[i]);
}
void emu_init_decompose(const float* F, const float* k4, float* R1, float* R2, float* t) {
  Lane lane;
  twoview::Motion M;
  twoview::decompose_e(lane.ws(), F, twoview::Cam{k4[0], k4[1], k4[2], k4[3]}, M);
  std::memcpy(R1, M.R1, 36), std::memcpy(R2, M.R2, 36), std::memcpy(t, M.t, 12);
}
// the device's selection of the order statistic of :895-897, bit by bit over twoview::ordered_key, one value at a time
float emu_init_kth(const float* v, int n, int idx) {
  uint32_t key = 0;
  for (int bit = 31; bit >= 0; --bit) {
    const uint32_t cand = key | (1u << bit);
    int below = 0;
    for (int i = 0; i < n; ++i) below += twoview::ordered_key(v[i]) < cand;
    if (below <= idx) key = cand;
  }
  return twoview::from_ordered_key(key);
}
int emu_init_check_rt(const float* R, const float* t, const float* k4, const float* k1, const float* k2, float th2, float* X, float* cosp) {
  Lane lane;
  return twoview::check_rt_one(lane.ws(), R, t, twoview::Cam{k4[0], k4[1], k4[2], k4[3]}, k1[0], k1[1], k2[0], k2[1], th2, X, cosp);
}

}  // extern "C"
