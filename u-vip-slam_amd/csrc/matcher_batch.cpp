// Batched forms of the two matcher loops of the LocalMapping thread.
//
//   CreateNewMapPoints (src/LocalMapping.cc:1058-1180) calls SearchForTriangulation(current KF, neighbour k) for up to 20 neighbours;
//   between two calls it triangulates pair k's matches and gives the accepted ones map points, which makes those features of the
//   current key frame ineligible for pair k + 1 (`if(pMP1) continue;`, src/ORBmatcher.cc:885-889).  The descriptor distances and the
//   epipolar test do not depend on that: uvo_search_for_triangulation_batch computes them for every pair in ONE launch and one host
//   wait; uvo_search_for_triangulation_next(k, has_mp1 now) then replays the reference's acceptance loop (:886-960) for pair k on the
//   host, in the reference's order -- the same result as 20 single calls, with one device round trip instead of 20.
//
//   SearchInNeighbors (src/LocalMapping.cc:1228-1236) calls Fuse(target k, the current key frame's map points) per target.  Fuse has no
//   exclusivity among the map points, so uvo_fuse_batch computes the projection tests and the best key point of every (target, map
//   point) in one pass (one upload of the map points, per target: grid + projection + walk, all stream-ordered, one download, one
//   wait); the map mutation between targets stays with the caller (include/uvo/compat/ORBmatcher.h: FuseTargets).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <utility>
#include <vector>

#include "matcher_priv.hpp"
#include "triangulate.hpp"

namespace uvo {
// what uvo_search_for_triangulation_batch leaves in the handle for the _next calls
struct TriBatch {
  int n1 = 0, n_pairs = 0;
  std::vector<uint8_t> has_mp1;   // as given to _batch: a feature that had a map point then is never a query
  std::vector<float> angle1;
  struct Pair {
    int n2 = 0, q_begin = 0, q_end = 0;  // this pair's queries [q_begin, q_end) in the reference's visiting order
    std::vector<float> angle2;
  };
  std::vector<Pair> pairs;
  std::vector<int32_t> q_idx1, start;  // query -> feature of key frame 1; CSR offsets into cand
  std::vector<uint32_t> cand;          // packed: idx2 | distance << 16 | octave << 25 | epipolar ok << 31
};
void tri_batch_free(void* p) { delete static_cast<TriBatch*>(p); }
}  // namespace uvo

using namespace uvo;

namespace {
// ORBmatcher::ComputeThreeMaxima (src/ORBmatcher.cc:1748-1789) on bin populations
void three_maxima(const int* hist, int L, int& ind1, int& ind2, int& ind3) {
  int max1 = 0, max2 = 0, max3 = 0;
  ind1 = ind2 = ind3 = -1;
  for (int i = 0; i < L; i++) {
    const int s = hist[i];
    if (s > max1) {
      max3 = max2, max2 = max1, max1 = s;
      ind3 = ind2, ind2 = ind1, ind1 = i;
    } else if (s > max2) {
      max3 = max2, max2 = s;
      ind3 = ind2, ind2 = i;
    } else if (s > max3) {
      max3 = s, ind3 = i;
    }
  }
  if (max2 < 0.1f * (float)max1) {
    ind2 = -1, ind3 = -1;
  } else if (max3 < 0.1f * (float)max1) {
    ind3 = -1;
  }
}

struct Drain {  // waits for the stream on every way out of a block whose host vectors an enqueued copy still reads
  hipStream_t s;
  bool armed;
  ~Drain() {
    if (armed) (void)hipStreamSynchronize(s);
  }
};

// Host staging of the candidate lists of every pair of a CreateNewMapPoints loop and, after tri_stage_launch, their device copies.
struct TriStage {
  std::vector<int32_t> cidx, q_pair, pair_base, tlevel, il;
  std::vector<float> tx, ty, tangle, f12, sigma, fl;
  std::vector<uint8_t> qdesc, tdesc;
  int sig_stride = 1, nq = 0, total = 0;
  size_t nt = 0;
  bool with_angles = false;  // also stage key frame 2's key point angles (the device-side rotation filter reads them)
  uint8_t *d_qdesc = nullptr, *d_tdesc = nullptr;
  int32_t *d_tlevel = nullptr, *d_start = nullptr, *d_cidx = nullptr, *d_il = nullptr;
  float* d_fl = nullptr;
  uint32_t* d_cand = nullptr;
  const float *d_tx = nullptr, *d_ty = nullptr, *d_tangle = nullptr;
};

// argument checks + the query / candidate lists of all pairs in the reference's visiting order (host work only)
int tri_stage_build(const uvo_feature_vector* fv1, const uvo_keypoint* kp1, int n1, const uint8_t* desc1, const uint8_t* has_mp1, int n_pairs,
                    const uvo_triangulation_pair* pairs, bool with_angles, TriBatch* tb, TriStage& S) {
  if (n1 < 0 || n_pairs < 0 || n_pairs > 4096) return fail(UVO_E_BADARG, "bad sizes");
  if (n_pairs > 0 && !pairs) return fail(UVO_E_BADARG, "null pointer");
  if (n1 > 0 && (!kp1 || !desc1 || !has_mp1)) return fail(UVO_E_BADARG, "null pointer");
  RC(check_fv(fv1, n1));
  S.with_angles = with_angles;
  tb->n1 = n1, tb->n_pairs = n_pairs;
  tb->has_mp1.assign(has_mp1, has_mp1 + n1);
  tb->angle1.resize(n1);
  for (int i = 0; i < n1; ++i) tb->angle1[i] = kp1[i].angle;
  tb->pairs.resize(n_pairs);
  tb->start.assign(1, 0);
  S.pair_base.assign(std::max(n_pairs, 1), 0);
  S.f12.assign((size_t)std::max(n_pairs, 1) * 9, 0.f);
  for (int p = 0; p < n_pairs; ++p) S.sig_stride = std::max(S.sig_stride, pairs[p].nlevels);
  S.sigma.assign((size_t)std::max(n_pairs, 1) * S.sig_stride, 0.f);
  size_t nt = 0;
  for (int p = 0; p < n_pairs; ++p) {
    const uvo_triangulation_pair& P = pairs[p];
    if (P.n2 < 0 || P.n2 > 65535 || P.nlevels < 1 || P.nlevels > 64) return fail(UVO_E_BADARG, "bad pair (at most 65535 keypoints, 1 <= nlevels <= 64)");
    if (P.n2 > 0 && (!P.kp2 || !P.desc2 || !P.has_mp2 || !P.sigma2)) return fail(UVO_E_BADARG, "null pointer in a pair");
    RC(check_fv(P.fv2, P.n2));
    for (int k = 0; k < P.n2; ++k)
      if (P.kp2[k].octave < 0 || P.kp2[k].octave >= P.nlevels) return fail(UVO_E_BADARG, "keypoint level outside the pair's sigma table");
    TriBatch::Pair& Q = tb->pairs[p];
    Q.n2 = P.n2, Q.q_begin = (int)tb->q_idx1.size();
    Q.angle2.resize(P.n2);
    S.pair_base[p] = (int32_t)nt;
    for (int k = 0; k < P.n2; ++k) {
      Q.angle2[k] = P.kp2[k].angle;
      S.tx.push_back(P.kp2[k].x), S.ty.push_back(P.kp2[k].y), S.tlevel.push_back(P.kp2[k].octave);
      if (with_angles) S.tangle.push_back(P.kp2[k].angle);
    }
    memcpy(&S.f12[(size_t)p * 9], P.f12, 9 * sizeof(float));
    memcpy(&S.sigma[(size_t)p * S.sig_stride], P.sigma2, (size_t)P.nlevels * sizeof(float));
    // queries in the reference's visiting order: shared nodes ascending, features of key frame 1 in node order (:886-892); candidates =
    // the node's features of key frame 2 without a map point (`|| pMP2`, :903-905), in node order
    int a = 0, b = 0;
    while (n1 > 0 && P.n2 > 0 && a < fv1->n_nodes && b < P.fv2->n_nodes) {
      if (fv1->node[a] == P.fv2->node[b]) {
        for (int e = fv1->start[a]; e < fv1->start[a + 1]; ++e) {
          const int idx1 = fv1->feat[e];
          if (has_mp1[idx1]) continue;
          tb->q_idx1.push_back(idx1);
          S.q_pair.push_back(p);
          for (int e2 = P.fv2->start[b]; e2 < P.fv2->start[b + 1]; ++e2) {
            const int idx2 = P.fv2->feat[e2];
            if (!P.has_mp2[idx2]) S.cidx.push_back((int32_t)nt + idx2);
          }
          tb->start.push_back((int32_t)S.cidx.size());
        }
        ++a, ++b;
      } else if (fv1->node[a] < P.fv2->node[b]) {
        ++a;
      } else {
        ++b;
      }
    }
    Q.q_end = (int)tb->q_idx1.size();
    nt += (size_t)P.n2;
  }
  S.nt = nt;
  S.nq = (int)tb->q_idx1.size(), S.total = (int)S.cidx.size();
  tb->cand.assign((size_t)S.total, 0u);
  return UVO_OK;
}

// uploads + the distances and epipolar tests of every pair in one launch; the packed candidates stay in S.d_cand.  S.total > 0.
int tri_stage_launch(uvo_matcher* m, const uvo_keypoint* kp1, const uint8_t* desc1, int n_pairs, const uvo_triangulation_pair* pairs,
                     const TriBatch* tb, TriStage& S) {
  const int nq = S.nq;
  const size_t nt = S.nt;
  S.qdesc.resize((size_t)nq * 32), S.tdesc.resize(nt * 32);
  std::vector<float> qx(nq), qy(nq);
  for (int i = 0; i < nq; ++i) {
    memcpy(&S.qdesc[(size_t)i * 32], desc1 + (size_t)tb->q_idx1[i] * 32, 32);
    qx[i] = kp1[tb->q_idx1[i]].x, qy[i] = kp1[tb->q_idx1[i]].y;
  }
  for (int p = 0; p < n_pairs; ++p)
    if (pairs[p].n2 > 0) memcpy(&S.tdesc[(size_t)S.pair_base[p] * 32], pairs[p].desc2, (size_t)pairs[p].n2 * 32);
  // one float block: qx | qy | tx | ty | f12 | sigma [| tangle]
  std::vector<float>& fl = S.fl;
  fl.insert(fl.end(), qx.begin(), qx.end());
  fl.insert(fl.end(), qy.begin(), qy.end());
  fl.insert(fl.end(), S.tx.begin(), S.tx.end());
  fl.insert(fl.end(), S.ty.begin(), S.ty.end());
  fl.insert(fl.end(), S.f12.begin(), S.f12.end());
  fl.insert(fl.end(), S.sigma.begin(), S.sigma.end());
  if (S.with_angles) fl.insert(fl.end(), S.tangle.begin(), S.tangle.end());
  S.il = S.q_pair;
  S.il.insert(S.il.end(), S.pair_base.begin(), S.pair_base.end());
  RC(upload(m, S_QDESC, S.qdesc.data(), S.qdesc.size(), &S.d_qdesc));
  RC(upload(m, S_TDESC, S.tdesc.data(), S.tdesc.size(), &S.d_tdesc));
  RC(upload(m, S_TLEVEL, S.tlevel.data(), S.tlevel.size(), &S.d_tlevel));
  RC(upload(m, S_START, tb->start.data(), tb->start.size(), &S.d_start));
  RC(upload(m, S_CIDX, S.cidx.data(), S.cidx.size(), &S.d_cidx));
  RC(upload(m, S_QPAIR, S.il.data(), S.il.size(), &S.d_il));
  RC(upload(m, S_MISC, fl.data(), fl.size(), &S.d_fl));
  RC(reserve(m, S_CAND, (size_t)S.total, &S.d_cand));
  const float *d_qx = S.d_fl, *d_qy = d_qx + nq, *d_f12, *d_sigma;
  S.d_tx = d_qy + nq, S.d_ty = S.d_tx + nt, d_f12 = S.d_ty + nt, d_sigma = d_f12 + S.f12.size(), S.d_tangle = d_sigma + S.sigma.size();
  {
    Profiler::Scope ps(&m->prof, "k_group_dist_pairs", m->stream);
    launch_group_dist_pairs(m->stream, nq, S.total, S.d_start, S.d_cidx, S.d_qdesc, S.d_tdesc, S.d_tlevel, S.d_il, S.d_il + nq, d_f12, d_qx, d_qy, S.d_tx, S.d_ty,
                            d_sigma, S.sig_stride, S.d_cand);
  }
  UVO_HIP_CHECK(hipGetLastError());
  return UVO_OK;
}

// a caller's camera -> the device record; the level tables are copied in
int tri_cam_pack(const uvo_triangulation_camera* c, TriCam* out) {
  if (!c || !c->scale_factors || !c->sigma2) return fail(UVO_E_BADARG, "null camera");
  if (c->nlevels < 1 || c->nlevels > kTriMaxLevels) return fail(UVO_E_BADARG, "camera: 1 <= nlevels <= 64");
  memset(out, 0, sizeof(*out));
  memcpy(out->r, c->rcw, sizeof(out->r));
  memcpy(out->t, c->tcw, sizeof(out->t));
  memcpy(out->ow, c->ow, sizeof(out->ow));
  out->fx = c->fx, out->fy = c->fy, out->cx = c->cx, out->cy = c->cy;
  memcpy(out->sf, c->scale_factors, (size_t)c->nlevels * sizeof(float));
  memcpy(out->sigma2, c->sigma2, (size_t)c->nlevels * sizeof(float));
  return UVO_OK;
}
int tri_check_octaves(const uvo_keypoint* kp, int n, int nlevels) {
  for (int i = 0; i < n; ++i)
    if (kp[i].octave < 0 || kp[i].octave >= nlevels) return fail(UVO_E_BADARG, "keypoint level outside the camera's level tables");
  return UVO_OK;
}
}  // namespace

extern "C" {

int uvo_search_for_triangulation_batch(uvo_matcher* m, const uvo_feature_vector* fv1, const uvo_keypoint* kp1, int n1, const uint8_t* desc1,
                                       const uint8_t* has_mp1, int n_pairs, const uvo_triangulation_pair* pairs) {
  if (!m) return fail(UVO_E_BADARG, "null handle");
  tri_batch_free(m->tri_batch);
  m->tri_batch = nullptr;
  TriBatch* tb = new TriBatch();
  struct Guard {
    TriBatch* t;
    ~Guard() { delete t; }
  } guard{tb};
  TriStage S;
  RC(tri_stage_build(fv1, kp1, n1, desc1, has_mp1, n_pairs, pairs, false, tb, S));
  if (S.total > 0) {
    UVO_HIP_CHECK(hipSetDevice(m->device));
    // the uploads below read the staging vectors asynchronously: whatever way this block is left, the stream is drained first
    Drain drain{m->stream, true};
    RC(tri_stage_launch(m, kp1, desc1, n_pairs, pairs, tb, S));
    UVO_HIP_CHECK(hipMemcpyAsync(tb->cand.data(), S.d_cand, (size_t)S.total * 4, hipMemcpyDeviceToHost, m->stream));
    UVO_HIP_CHECK(hipStreamSynchronize(m->stream));  // the only host wait of the batch
    drain.armed = false;
  }
  guard.t = nullptr;
  m->tri_batch = tb;
  return UVO_OK;
}

int uvo_search_for_triangulation_next(uvo_matcher* m, int pair, const uint8_t* has_mp1_now, int check_orientation, int32_t* match12, int* n_matches) {
  if (!m || !n_matches) return fail(UVO_E_BADARG, "null pointer");
  *n_matches = 0;
  const TriBatch* tb = static_cast<const TriBatch*>(m->tri_batch);
  if (!tb) return fail(UVO_E_BADARG, "no batch: call uvo_search_for_triangulation_batch first");
  if (pair < 0 || pair >= tb->n_pairs) return fail(UVO_E_BADARG, "pair outside the batch");
  if (tb->n1 == 0) return UVO_OK;
  if (!match12 || !has_mp1_now) return fail(UVO_E_BADARG, "null pointer");
  for (int i = 0; i < tb->n1; ++i) {
    match12[i] = -1;
    // the batch only prepared the features that had no map point when it began; one that LOST its point since would be a query now
    if (tb->has_mp1[i] && !has_mp1_now[i]) return fail(UVO_E_BADARG, "a feature lost its map point since the batch began: start a new batch");
  }
  const TriBatch::Pair& P = tb->pairs[pair];
  std::vector<uint8_t> vbMatched2(P.n2, 0);
  std::vector<std::pair<int, uint32_t> > vDistIndex;  // (distance, idx2 | ok << 31): sorts like the reference's pair<int, size_t>
  int nmatches = 0;
  constexpr int HISTO_LENGTH = 30, TH_LOW = 50;
  std::vector<int> rotHist[HISTO_LENGTH];
  const float factor = 1.0f / HISTO_LENGTH;
  for (int q = P.q_begin; q < P.q_end; ++q) {
    const int idx1 = tb->q_idx1[q];
    if (has_mp1_now[idx1]) continue;  // :885-889
    vDistIndex.clear();
    for (int e = tb->start[q]; e < tb->start[q + 1]; ++e) {
      const uint32_t w = tb->cand[e];
      const uint32_t idx2 = w & 0xffffu;
      const int dist = (int)((w >> 16) & 0x1ffu);
      if (vbMatched2[idx2]) continue;  // :903-905 (the map-point half of the test was applied when the lists were built)
      if (dist > TH_LOW) continue;     // :911-912
      vDistIndex.push_back(std::make_pair(dist, idx2 | (w & 0x80000000u)));
    }
    if (vDistIndex.empty()) continue;
    // sort(vDistIndex): by distance, then by idx2 -- the flag in bit 31 must not take part
    std::sort(vDistIndex.begin(), vDistIndex.end(), [](const std::pair<int, uint32_t>& a, const std::pair<int, uint32_t>& b) {
      return a.first != b.first ? a.first < b.first : (a.second & 0x7fffffffu) < (b.second & 0x7fffffffu);
    });
    const int BestDist = vDistIndex.front().first;
    const int DistTh = (int)std::round((double)(2 * BestDist));  // :921
    for (size_t id = 0; id < vDistIndex.size(); id++) {
      if (vDistIndex[id].first > DistTh) break;
      if (!(vDistIndex[id].second >> 31)) continue;  // CheckDistEpipolarLine, :928
      const int currentIdx2 = (int)(vDistIndex[id].second & 0x7fffffffu);
      vbMatched2[currentIdx2] = 1;
      match12[idx1] = currentIdx2;
      nmatches++;
      if (check_orientation) {  // :934-944
        float rot = tb->angle1[idx1] - P.angle2[currentIdx2];
        if (rot < 0.0) rot += 360.0f;
        int bin = (int)std::round(rot * factor);
        if (bin == HISTO_LENGTH) bin = 0;
        if (bin >= 0 && bin < HISTO_LENGTH) rotHist[bin].push_back(idx1);
        else match12[idx1] = -1, nmatches--;  // the reference asserts the range (angles are in [0, 360)); such a match lands in no bin
      }
      break;
    }
  }
  if (check_orientation) {  // :966-984
    int hist[HISTO_LENGTH], ind1, ind2, ind3;
    for (int i = 0; i < HISTO_LENGTH; ++i) hist[i] = (int)rotHist[i].size();
    three_maxima(hist, HISTO_LENGTH, ind1, ind2, ind3);
    for (int i = 0; i < HISTO_LENGTH; i++) {
      if (i == ind1 || i == ind2 || i == ind3) continue;
      for (size_t j = 0; j < rotHist[i].size(); j++) {
        match12[rotHist[i][j]] = -1;
        nmatches--;
      }
    }
  }
  *n_matches = nmatches;
  return UVO_OK;
}

int uvo_fuse_batch(uvo_matcher* m, int n_targets, const uvo_fuse_target* targets, int nmp, const float* xyz, const float* normal,
                   const float* min_distance_inv, const float* max_distance_inv, const uint8_t* usable, const uint8_t* mp_desc, float th,
                   int32_t* best_idx, int32_t* best_dist) {
  if (!m) return fail(UVO_E_BADARG, "null handle");
  if (n_targets < 0 || nmp < 0) return fail(UVO_E_BADARG, "bad sizes");
  if (n_targets == 0 || nmp == 0) return UVO_OK;
  if (!targets || !xyz || !normal || !min_distance_inv || !max_distance_inv || !mp_desc || !best_idx || !best_dist) return fail(UVO_E_BADARG, "null pointer");
  for (int t = 0; t < n_targets; ++t) {
    const uvo_fuse_target& T = targets[t];
    if (T.n < 0 || T.n > 65535 || T.nlevels < 1 || T.nlevels > 64 || T.max_x <= T.min_x || T.max_y <= T.min_y) return fail(UVO_E_BADARG, "bad target");
    if (!T.scale_factors || (T.n > 0 && (!T.kp || !T.desc))) return fail(UVO_E_BADARG, "null pointer in a target");
  }
  UVO_HIP_CHECK(hipSetDevice(m->device));
  hipStream_t s = m->stream;
  // the map points once: xyz | normal | min | max as one float block, usable, descriptors
  std::vector<float> fl((size_t)nmp * 8);
  struct Drain {  // declared after the staging block: runs before it is freed, on every way out
    hipStream_t s;
    bool armed;
    ~Drain() {
      if (armed) (void)hipStreamSynchronize(s);
    }
  } drain{s, true};
  memcpy(&fl[0], xyz, (size_t)nmp * 3 * sizeof(float));
  memcpy(&fl[(size_t)nmp * 3], normal, (size_t)nmp * 3 * sizeof(float));
  memcpy(&fl[(size_t)nmp * 6], min_distance_inv, (size_t)nmp * sizeof(float));
  memcpy(&fl[(size_t)nmp * 7], max_distance_inv, (size_t)nmp * sizeof(float));
  float* d_fl;
  uint8_t *d_usable = nullptr, *d_mpdesc;
  RC(upload(m, S_MISC, fl.data(), fl.size(), &d_fl));
  if (usable) RC(upload(m, S_QVALID, usable, (size_t)nmp, &d_usable));
  RC(upload(m, S_MPDESC, mp_desc, (size_t)nmp * 32, &d_mpdesc));
  // per-point projection outputs (reused by every target) and the results of all targets
  float *d_u, *d_v;
  int32_t *d_level, *d_best;
  uint8_t* d_valid;
  RC(reserve(m, S_PX, (size_t)nmp, &d_u));
  RC(reserve(m, S_PY, (size_t)nmp, &d_v));
  RC(reserve(m, S_LEVEL, (size_t)nmp, &d_level));
  RC(reserve(m, S_INVIEW, (size_t)nmp, &d_valid));
  RC(reserve(m, S_MATCH, (size_t)2 * n_targets * nmp, &d_best));
  int max_n = 1, max_lev = 1;
  for (int t = 0; t < n_targets; ++t) max_n = std::max(max_n, targets[t].n), max_lev = std::max(max_lev, targets[t].nlevels);
  // every buffer a target needs is sized for the largest one up front: nothing grows (and synchronises) inside the loop
  uvo_keypoint* d_kp;
  uint8_t* d_desc;
  float* d_sf;
  int32_t *d_cell_start, *d_cell_items, *d_cell_of;
  RC(reserve(m, S_KP, (size_t)max_n, &d_kp));
  RC(reserve(m, S_TDESC, (size_t)max_n * 32, &d_desc));
  RC(reserve(m, S_SCALE, (size_t)max_lev, &d_sf));
  RC(reserve(m, S_CELL_START, (size_t)kGridCells + 1, &d_cell_start));
  RC(reserve(m, S_CELL_ITEMS, (size_t)max_n, &d_cell_items));
  RC(reserve(m, S_CELL_OF, (size_t)max_n, &d_cell_of));
  for (int t = 0; t < n_targets; ++t) {
    const uvo_fuse_target& T = targets[t];
    int32_t* bi = d_best + (size_t)t * nmp;
    int32_t* bd = d_best + (size_t)(n_targets + t) * nmp;
    if (T.n == 0) {
      UVO_HIP_CHECK(hipMemsetAsync(bi, 0xff, (size_t)nmp * 4, s));
      UVO_HIP_CHECK(hipMemsetAsync(bd, 0xff, (size_t)nmp * 4, s));
      continue;
    }
    UVO_HIP_CHECK(hipMemcpyAsync(d_kp, T.kp, (size_t)T.n * sizeof(uvo_keypoint), hipMemcpyHostToDevice, s));
    UVO_HIP_CHECK(hipMemcpyAsync(d_desc, T.desc, (size_t)T.n * 32, hipMemcpyHostToDevice, s));
    UVO_HIP_CHECK(hipMemcpyAsync(d_sf, T.scale_factors, (size_t)T.nlevels * sizeof(float), hipMemcpyHostToDevice, s));
    // projection tests of Fuse (:1037-1075) with this target's pose, then the window walk on its grid
    launch_project(s, UVO_PROJECT_FUSE, T.cam, nmp, d_fl, d_fl + (size_t)nmp * 3, d_fl + (size_t)nmp * 6, d_fl + (size_t)nmp * 7, nullptr, d_usable, d_sf,
                   T.nlevels, 0.f, 0.f, d_valid, d_u, d_v, d_level, nullptr);
    launch_fuse_walk(s, d_kp, d_desc, T.n, T.min_x, T.min_y, T.max_x, T.max_y, nmp, d_valid, d_u, d_v, d_level, d_mpdesc, d_sf, th, d_cell_start,
                     d_cell_items, d_cell_of, bi, bd);
  }
  UVO_HIP_CHECK(hipGetLastError());
  UVO_HIP_CHECK(hipMemcpyAsync(best_idx, d_best, (size_t)n_targets * nmp * 4, hipMemcpyDeviceToHost, s));
  UVO_HIP_CHECK(hipMemcpyAsync(best_dist, d_best + (size_t)n_targets * nmp, (size_t)n_targets * nmp * 4, hipMemcpyDeviceToHost, s));
  UVO_HIP_CHECK(hipStreamSynchronize(s));  // the only host wait of the batch
  drain.armed = false;
  return UVO_OK;
}

int uvo_triangulate_matches(uvo_matcher* m, const uvo_triangulation_camera* cam1, const uvo_triangulation_camera* cam2, float ratio_factor,
                            const uvo_keypoint* kp1, const uvo_keypoint* kp2, int n, int32_t* verdict, float* x3d) {
  if (!m) return fail(UVO_E_BADARG, "null handle");
  if (n < 0) return fail(UVO_E_BADARG, "bad sizes");
  TriCam cams[2];
  RC(tri_cam_pack(cam1, &cams[0]));
  RC(tri_cam_pack(cam2, &cams[1]));
  if (n == 0) return UVO_OK;
  if (!kp1 || !kp2 || !verdict || !x3d) return fail(UVO_E_BADARG, "null pointer");
  RC(tri_check_octaves(kp1, n, cam1->nlevels));
  RC(tri_check_octaves(kp2, n, cam2->nlevels));
  UVO_HIP_CHECK(hipSetDevice(m->device));
  hipStream_t s = m->stream;
  Drain drain{s, true};
  TriCam* d_cams;
  uvo_keypoint *d_kp1, *d_kp2;
  int32_t* d_verdict;
  float* d_x3d;
  RC(upload(m, S_QR, cams, 2, &d_cams));
  RC(upload(m, S_KP, kp1, (size_t)n, &d_kp1));
  RC(upload(m, S_QDESC, kp2, (size_t)n, &d_kp2));
  RC(reserve(m, S_MATCH, (size_t)n, &d_verdict));
  RC(reserve(m, S_PX, (size_t)n * 3, &d_x3d));
  {
    Profiler::Scope ps(&m->prof, "k_triangulate", s);
    launch_triangulate(s, n, d_cams, ratio_factor, d_kp1, d_kp2, d_verdict, d_x3d);
  }
  UVO_HIP_CHECK(hipGetLastError());
  UVO_HIP_CHECK(hipMemcpyAsync(verdict, d_verdict, (size_t)n * 4, hipMemcpyDeviceToHost, s));
  UVO_HIP_CHECK(hipMemcpyAsync(x3d, d_x3d, (size_t)n * 12, hipMemcpyDeviceToHost, s));
  UVO_HIP_CHECK(hipStreamSynchronize(s));
  drain.armed = false;
  return UVO_OK;
}

int uvo_create_new_map_points(uvo_matcher* m, const uvo_feature_vector* fv1, const uvo_keypoint* kp1, int n1, const uint8_t* desc1,
                              const uint8_t* has_mp1, int n_pairs, const uvo_triangulation_pair* pairs, const uvo_triangulation_camera* cam1,
                              const uvo_triangulation_camera* cams2, float ratio_factor, int check_orientation, const uvo_new_map_points* out) {
  if (!m) return fail(UVO_E_BADARG, "null handle");
  if (!out || !out->n_matches || !out->n_accepted) return fail(UVO_E_BADARG, "null output");
  if (n_pairs > 0 && n1 > 0 && (!out->idx1 || !out->idx2 || !out->verdict || !out->x3d)) return fail(UVO_E_BADARG, "null output");
  TriBatch tb;  // the lists live for this call only: nothing is kept in the handle
  TriStage S;
  RC(tri_stage_build(fv1, kp1, n1, desc1, has_mp1, n_pairs, pairs, true, &tb, S));
  std::vector<TriCam> cams((size_t)n_pairs + 1);
  RC(tri_cam_pack(cam1, &cams[0]));
  if (n_pairs > 0 && !cams2) return fail(UVO_E_BADARG, "null camera");
  RC(tri_check_octaves(kp1, n1, cam1->nlevels));
  for (int p = 0; p < n_pairs; ++p) {
    RC(tri_cam_pack(&cams2[p], &cams[1 + p]));
    RC(tri_check_octaves(pairs[p].kp2, pairs[p].n2, cams2[p].nlevels));
  }
  for (int p = 0; p < n_pairs; ++p) out->n_matches[p] = 0, out->n_accepted[p] = 0;
  if (out->has_mp1_out && n1 > 0) memcpy(out->has_mp1_out, has_mp1, (size_t)n1);
  if (S.total == 0) return UVO_OK;  // no query has a candidate: no pair can match
  const int nq = S.nq;
  int max_n2 = 1, max_q = 1;
  std::vector<int32_t> pair_tab((size_t)n_pairs * 4);
  for (int p = 0; p < n_pairs; ++p) {
    const TriBatch::Pair& Q = tb.pairs[p];
    pair_tab[4 * p] = Q.q_begin, pair_tab[4 * p + 1] = Q.q_end, pair_tab[4 * p + 2] = Q.n2, pair_tab[4 * p + 3] = S.pair_base[p];
    max_n2 = std::max(max_n2, Q.n2), max_q = std::max(max_q, Q.q_end - Q.q_begin);
  }
  UVO_HIP_CHECK(hipSetDevice(m->device));
  hipStream_t s = m->stream;
  std::vector<int32_t> h_outi((size_t)3 * nq + 2 * n_pairs);
  std::vector<float> h_x3d((size_t)3 * nq);
  Drain drain{s, true};
  RC(tri_stage_launch(m, kp1, desc1, n_pairs, pairs, &tb, S));
  TriChain A;
  TriCam* d_cams;
  uvo_keypoint* d_kp1;
  int32_t *d_pair, *d_qidx, *d_outi;
  RC(upload(m, S_QR, cams.data(), cams.size(), &d_cams));
  RC(upload(m, S_KP, kp1, (size_t)n1, &d_kp1));
  RC(upload(m, S_BLOCKED, has_mp1, (size_t)n1, &A.has_mp1));
  RC(upload(m, S_QMIN, tb.q_idx1.data(), tb.q_idx1.size(), &d_qidx));
  RC(upload(m, S_QMAX, pair_tab.data(), pair_tab.size(), &d_pair));
  RC(reserve(m, S_OWNER, (size_t)max_n2, &A.owner));
  RC(reserve(m, S_OWNER2, (size_t)max_n2, &A.owner_next));
  RC(reserve(m, S_CHOICE, (size_t)max_q, &A.choice));
  RC(reserve(m, S_MATCH, (size_t)n1, &A.match12));
  RC(reserve(m, S_IDX0, (size_t)3 * nq + 2 * n_pairs, &d_outi));  // idx1 | idx2 | verdict | n_matches | n_accepted
  RC(reserve(m, S_PX, (size_t)3 * nq, &A.x3d));
  A.n_pairs = n_pairs, A.n1 = n1, A.check_orientation = check_orientation ? 1 : 0, A.ratio_factor = ratio_factor;
  A.cams = d_cams, A.pair = d_pair, A.q_idx1 = d_qidx, A.cand_start = S.d_start, A.cand = S.d_cand, A.kp1 = d_kp1;
  A.tx = S.d_tx, A.ty = S.d_ty, A.tangle = S.d_tangle, A.tlevel = S.d_tlevel;
  A.out_idx1 = d_outi, A.out_idx2 = d_outi + nq, A.verdict = d_outi + 2 * (size_t)nq;
  A.n_matches = d_outi + 3 * (size_t)nq, A.n_accepted = A.n_matches + n_pairs;
  {
    Profiler::Scope ps(&m->prof, "k_create_new_map_points", s);
    launch_create_new_map_points(s, A);
  }
  UVO_HIP_CHECK(hipGetLastError());
  UVO_HIP_CHECK(hipMemcpyAsync(h_outi.data(), d_outi, h_outi.size() * 4, hipMemcpyDeviceToHost, s));
  UVO_HIP_CHECK(hipMemcpyAsync(h_x3d.data(), A.x3d, h_x3d.size() * 4, hipMemcpyDeviceToHost, s));
  if (out->has_mp1_out) UVO_HIP_CHECK(hipMemcpyAsync(out->has_mp1_out, A.has_mp1, (size_t)n1, hipMemcpyDeviceToHost, s));
  UVO_HIP_CHECK(hipStreamSynchronize(s));  // the only host wait of the loop
  drain.armed = false;
  for (int p = 0; p < n_pairs; ++p) {
    const int nm = h_outi[(size_t)3 * nq + p], qb = tb.pairs[p].q_begin;
    if (nm < 0 || nm > tb.pairs[p].q_end - qb || nm > n1) return fail(UVO_E_HIP, "device returned an impossible match count");
    out->n_matches[p] = nm, out->n_accepted[p] = h_outi[(size_t)3 * nq + n_pairs + p];
    const size_t o = (size_t)p * n1;
    memcpy(out->idx1 + o, &h_outi[qb], (size_t)nm * 4);
    memcpy(out->idx2 + o, &h_outi[(size_t)nq + qb], (size_t)nm * 4);
    memcpy(out->verdict + o, &h_outi[(size_t)2 * nq + qb], (size_t)nm * 4);
    memcpy(out->x3d + o * 3, &h_x3d[(size_t)3 * qb], (size_t)nm * 12);
  }
  return UVO_OK;
}

}  // extern "C"
