// Host side of the matcher entry points of include/uvo/uvo.h (replacing the arithmetic and search cores of
// USLAM::ORBmatcher, src/ORBmatcher.cc, and Utils::ratioMatching, include/utils.h:81-111).
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "extractor_priv.hpp"
#include "matcher_priv.hpp"
#include "uvo_math.hpp"

using namespace uvo;

namespace {
// the device side of SearchByProjection after its inputs are in place (uvo_search_by_projection, uvo_search_points_in_frustum)
struct SbpWork {
  int32_t *cell_start, *cell_items, *cell_of, *cnt, *start, *owner, *owner_next, *choice, *nm;
};
int sbp_work(uvo_matcher* m, int n, int nmp, SbpWork* w) {
  RC(reserve(m, S_CELL_START, (size_t)kGridCells + 1, &w->cell_start));
  RC(reserve(m, S_CELL_ITEMS, (size_t)n, &w->cell_items));
  RC(reserve(m, S_CELL_OF, (size_t)n, &w->cell_of));
  RC(reserve(m, S_CNT, (size_t)nmp + 1, &w->cnt));
  RC(reserve(m, S_START, (size_t)nmp + 1, &w->start));
  RC(reserve(m, S_OWNER, (size_t)n, &w->owner));
  RC(reserve(m, S_OWNER2, (size_t)n, &w->owner_next));
  RC(reserve(m, S_CHOICE, (size_t)nmp, &w->choice));
  return reserve(m, S_NM, 1, &w->nm);
}
// entries the candidate-list slot holds (the kernels never write or read past the capacity they are given)
int64_t cand_cap(uvo_matcher* m) { return (int64_t)(m->buf[S_CAND].cap / sizeof(uint32_t)); }
}  // namespace

extern "C" {

int uvo_matcher_create(const uvo_matcher_cfg* cfg, uvo_matcher** out) {
  if (!cfg || !out) return fail(UVO_E_BADARG, "null pointer");
  *out = nullptr;
  if (cfg->max_query < 1 || cfg->max_train < 1 || cfg->max_batch < 1 || cfg->max_map_points < 0 || cfg->max_query > 65535 ||
      cfg->max_train > 65535)
    return fail(UVO_E_BADARG, "bad matcher configuration");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(UVO_E_NODEVICE, "no HIP device available (no CPU fallback exists)");
  if (cfg->device < 0 || cfg->device >= ndev) return fail(UVO_E_BADARG, "device ordinal out of range");
  uvo_matcher* m = new uvo_matcher();
  m->cfg = *cfg;
  m->device = cfg->device;
  if (hipSetDevice(m->device) != hipSuccess || hipStreamCreateWithFlags(&m->own_stream, hipStreamNonBlocking) != hipSuccess) {
    delete m;
    return fail(UVO_E_HIP, "stream creation failed");
  }
  m->stream = m->own_stream;
  // the slots the configuration bounds, at their full size: an oversized configuration fails here, and no call within it grows them
  const size_t B = cfg->max_batch, Q = cfg->max_query, T = cfg->max_train, MP = std::max(cfg->max_map_points, 1);
  const struct {
    Slot slot;
    size_t bytes;
  } fixed[] = {{S_Q, Q * 32},
               {S_T, T * 32},
               {S_IDX0, B * Q * 4},
               {S_IDX1, B * Q * 4},
               {S_D0, B * Q * 2},
               {S_D1, B * Q * 2},
               {S_KP, Q * sizeof(uvo_keypoint)},
               {S_ASSIGNED, Q * 4},
               {S_CELL_START, (kGridCells + 1) * 4},
               {S_CELL_ITEMS, Q * 4},
               {S_CELL_OF, Q * 4},
               {S_OWNER, Q * 4},
               {S_OWNER2, Q * 4},
               {S_PX, MP * 4},
               {S_PY, MP * 4},
               {S_VC, MP * 4},
               {S_LEVEL, MP * 4},
               {S_INVIEW, MP},
               {S_MPDESC, MP * 32},
               {S_CNT, (MP + 1) * 4},
               {S_START, (MP + 1) * 4},
               {S_CHOICE, MP * 4},
               {S_SCALE, kMaxLevels * 4 * 4},
               {S_NM, 4}};
  for (const auto& f : fixed) {
    void* p;
    const int rc = ensure(m, f.slot, f.bytes, &p);
    if (rc) {
      uvo_matcher_destroy(m);
      return rc;
    }
  }
  if (hipEventCreateWithFlags(&m->ev, hipEventDisableTiming) != hipSuccess) {
    uvo_matcher_destroy(m);
    return fail(UVO_E_HIP, "event creation failed");
  }
  *out = m;
  return UVO_OK;
}

void uvo_matcher_destroy(uvo_matcher* m) {
  if (!m) return;
  hipSetDevice(m->device);
  if (m->attached_to) uvo_extractor_drop_follower_internal(m->attached_to, m);
  if (m->stream) hipStreamSynchronize(m->stream);
  if (m->own_stream && m->own_stream != m->stream) hipStreamSynchronize(m->own_stream);
  for (Buf& b : m->buf)
    if (b.p) hipFree(b.p);
  if (m->h_arena.p) (void)hipHostFree(m->h_arena.p);
  uvo::tri_batch_free(m->tri_batch);
  m->prof.clear();
  if (m->ev) (void)hipEventDestroy(m->ev);
  if (m->own_stream) hipStreamDestroy(m->own_stream);
  delete m;
}

int uvo_matcher_synchronize(uvo_matcher* m) {
  if (!m) return fail(UVO_E_BADARG, "null handle");
  UVO_HIP_CHECK(hipSetDevice(m->device));
  UVO_HIP_CHECK(hipStreamSynchronize(m->stream));
  return UVO_OK;
}

int uvo_hamming_knn2(uvo_matcher* m, const uint8_t* q, int nq, const uint8_t* t, int nt, const uint8_t* mask, int32_t* idx0, uint16_t* d0,
                     int32_t* idx1, uint16_t* d1) {
  if (!m || !idx0 || !d0 || !idx1 || !d1) return fail(UVO_E_BADARG, "null pointer");
  if (nq < 0 || nt < 0 || nq > m->cfg.max_query || nt > m->cfg.max_train) return fail(UVO_E_BADARG, "descriptor count outside handle capacity");
  if (nq == 0) return UVO_OK;  // ratioMatching returns early on empty inputs (include/utils.h:85-86)
  if (!q || (nt > 0 && !t)) return fail(UVO_E_BADARG, "null descriptor pointer");
  UVO_HIP_CHECK(hipSetDevice(m->device));
  hipStream_t s = m->stream;
  uint8_t *d_q, *d_t, *d_mask = nullptr;
  int32_t *d_idx0, *d_idx1;
  uint16_t *d_d0, *d_d1;
  RC(upload(m, S_Q, q, (size_t)nq * 32, &d_q));
  RC(upload(m, S_T, t, (size_t)nt * 32, &d_t));
  if (mask && nt > 0) RC(upload(m, S_MASK, mask, (size_t)nq * nt, &d_mask));
  RC(reserve(m, S_IDX0, (size_t)nq, &d_idx0));
  RC(reserve(m, S_IDX1, (size_t)nq, &d_idx1));
  RC(reserve(m, S_D0, (size_t)nq, &d_d0));
  RC(reserve(m, S_D1, (size_t)nq, &d_d1));
  launch_knn2(s, 1, nq, d_q, nullptr, nq, 0, d_t, nullptr, nt, 0, d_mask, m->cfg.max_query, d_idx0, d_d0, d_idx1, d_d1);
  UVO_HIP_CHECK(hipGetLastError());
  UVO_HIP_CHECK(hipMemcpyAsync(idx0, d_idx0, (size_t)nq * 4, hipMemcpyDeviceToHost, s));
  UVO_HIP_CHECK(hipMemcpyAsync(idx1, d_idx1, (size_t)nq * 4, hipMemcpyDeviceToHost, s));
  UVO_HIP_CHECK(hipMemcpyAsync(d0, d_d0, (size_t)nq * 2, hipMemcpyDeviceToHost, s));
  UVO_HIP_CHECK(hipMemcpyAsync(d1, d_d1, (size_t)nq * 2, hipMemcpyDeviceToHost, s));
  UVO_HIP_CHECK(hipStreamSynchronize(s));
  return UVO_OK;
}

int uvo_hamming_knn2_batch_device(uvo_matcher* m, int pairs, const uint8_t* d_q, const int32_t* d_nq, int q_stride, const uint8_t* d_t,
                                  const int32_t* d_nt, int t_stride, int32_t* d_idx0, uint16_t* d_d0, int32_t* d_idx1, uint16_t* d_d1) {
  if (!m || !d_q || !d_t || !d_nq || !d_nt || !d_idx0 || !d_d0 || !d_idx1 || !d_d1) return fail(UVO_E_BADARG, "null pointer");
  if (pairs < 1 || pairs > m->cfg.max_batch || q_stride < 1 || t_stride < 1) return fail(UVO_E_BADARG, "bad batch / stride");
  // the launch covers max_query rows per pair and the outputs are [pairs][max_query]: a wider query slice would lose rows silently
  if (q_stride > m->cfg.max_query) return fail(UVO_E_BADARG, "q_stride above the handle's max_query");
  if (t_stride > 65535) return fail(UVO_E_BADARG, "t_stride above 65535 (train indices are packed in 16 bits)");
  UVO_HIP_CHECK(hipSetDevice(m->device));
  {
    Profiler::Scope ps(&m->prof, "k_knn2", m->stream);
    launch_knn2(m->stream, pairs, m->cfg.max_query, d_q, d_nq, 0, q_stride, d_t, d_nt, 0, t_stride, nullptr, m->cfg.max_query, d_idx0, d_d0,
                d_idx1, d_d1);
  }
  UVO_HIP_CHECK(hipGetLastError());
  return UVO_OK;
}

int uvo_hamming_matrix(uvo_matcher* m, const uint8_t* q, int nq, const uint8_t* t, int nt, uint16_t* dist) {
  if (!m || !dist) return fail(UVO_E_BADARG, "null pointer");
  if (nq < 0 || nt < 0 || nq > m->cfg.max_query || nt > m->cfg.max_train) return fail(UVO_E_BADARG, "descriptor count outside handle capacity");
  if (nq == 0 || nt == 0) return UVO_OK;
  if (!q || !t) return fail(UVO_E_BADARG, "null descriptor pointer");
  UVO_HIP_CHECK(hipSetDevice(m->device));
  hipStream_t s = m->stream;
  const size_t need = (size_t)nq * nt;
  uint8_t *d_q, *d_t;
  uint16_t* d_dist;
  RC(upload(m, S_Q, q, (size_t)nq * 32, &d_q));
  RC(upload(m, S_T, t, (size_t)nt * 32, &d_t));
  RC(reserve(m, S_DIST, need, &d_dist));
  launch_matrix(s, d_q, nq, d_t, nt, d_dist);
  UVO_HIP_CHECK(hipGetLastError());
  UVO_HIP_CHECK(hipMemcpyAsync(dist, d_dist, need * 2, hipMemcpyDeviceToHost, s));
  UVO_HIP_CHECK(hipStreamSynchronize(s));
  return UVO_OK;
}

int uvo_distinctive_descriptors(uvo_matcher* m, const uint8_t* desc, const int32_t* offsets, int npoints, int32_t* best_idx,
                                int32_t* best_median) {
  if (!m || !offsets || !best_idx || !best_median) return fail(UVO_E_BADARG, "null pointer");
  if (npoints < 0) return fail(UVO_E_BADARG, "negative point count");
  if (npoints == 0) return UVO_OK;
  if (offsets[0] != 0) return fail(UVO_E_BADARG, "offsets[0] must be 0");
  for (int p = 0; p < npoints; ++p)
    if (offsets[p + 1] < offsets[p] || offsets[p + 1] - offsets[p] > 65535) return fail(UVO_E_BADARG, "offsets must be non-decreasing, <= 65535 rows per point");
  const size_t rows = (size_t)offsets[npoints];
  if (rows > 0 && !desc) return fail(UVO_E_BADARG, "null descriptor pointer");
  UVO_HIP_CHECK(hipSetDevice(m->device));
  hipStream_t s = m->stream;
  uint8_t* d_md;
  int32_t *d_off, *d_res;
  RC(upload(m, S_MD_DESC, desc, rows * 32, &d_md));
  RC(upload(m, S_MD_OFF, offsets, (size_t)npoints + 1, &d_off));
  RC(reserve(m, S_MD_RES, (size_t)2 * npoints, &d_res));
  launch_medoid(s, d_md, d_off, npoints, d_res, d_res + npoints);
  UVO_HIP_CHECK(hipGetLastError());
  UVO_HIP_CHECK(hipMemcpyAsync(best_idx, d_res, (size_t)npoints * 4, hipMemcpyDeviceToHost, s));
  UVO_HIP_CHECK(hipMemcpyAsync(best_median, d_res + npoints, (size_t)npoints * 4, hipMemcpyDeviceToHost, s));
  UVO_HIP_CHECK(hipStreamSynchronize(s));
  return UVO_OK;
}

int uvo_search_by_projection(uvo_matcher* m, const uvo_keypoint* kp, int n, const uint8_t* desc, int min_x, int min_y, int max_x, int max_y,
                             int32_t* assigned, int nmp, const float* proj_x, const float* proj_y, const int32_t* level,
                             const float* view_cos, const uint8_t* in_view, const uint8_t* mp_desc, const float* scale_factors,
                             int nlevels, float th, float nnratio, int* n_matches) {
  if (!m || !n_matches) return fail(UVO_E_BADARG, "null pointer");
  *n_matches = 0;
  if (n < 0 || nmp < 0 || n > m->cfg.max_query || nmp > m->cfg.max_map_points || nlevels < 1 || nlevels > kMaxLevels * 4 || max_x <= min_x ||
      max_y <= min_y)
    return fail(UVO_E_BADARG, "sizes outside handle capacity");
  if (n == 0 || nmp == 0) return UVO_OK;
  if (!kp || !desc || !assigned || !proj_x || !proj_y || !level || !view_cos || !in_view || !mp_desc || !scale_factors)
    return fail(UVO_E_BADARG, "null pointer");
  for (int i = 0; i < nmp; ++i)
    if (in_view[i] && (level[i] < 0 || level[i] >= nlevels)) return fail(UVO_E_BADARG, "map point level outside 0..nlevels-1");
  UVO_HIP_CHECK(hipSetDevice(m->device));
  hipStream_t s = m->stream;
  uvo_keypoint* d_kp;
  uint8_t *d_desc, *d_inview, *d_mpdesc;
  float *d_px, *d_py, *d_vc, *d_scale;
  int32_t *d_assigned, *d_level;
  RC(upload(m, S_KP, kp, (size_t)n, &d_kp));
  RC(upload(m, S_Q, desc, (size_t)n * 32, &d_desc));
  RC(upload(m, S_ASSIGNED, assigned, (size_t)n, &d_assigned));
  RC(upload(m, S_PX, proj_x, (size_t)nmp, &d_px));
  RC(upload(m, S_PY, proj_y, (size_t)nmp, &d_py));
  RC(upload(m, S_VC, view_cos, (size_t)nmp, &d_vc));
  RC(upload(m, S_LEVEL, level, (size_t)nmp, &d_level));
  RC(upload(m, S_INVIEW, in_view, (size_t)nmp, &d_inview));
  RC(upload(m, S_MPDESC, mp_desc, (size_t)nmp * 32, &d_mpdesc));
  RC(upload(m, S_SCALE, scale_factors, (size_t)nlevels, &d_scale));
  SbpWork w;
  RC(sbp_work(m, n, nmp, &w));
  uint32_t* d_cand = nullptr;  // sized from the count stage's total
  auto go = [&](int stage) {
    launch_sbp(s, d_kp, n, d_desc, min_x, min_y, max_x, max_y, d_assigned, nmp, d_px, d_py, d_level, d_vc, d_inview, d_mpdesc, d_scale, th, nnratio,
               w.cell_start, w.cell_items, w.cell_of, w.cnt, w.start, d_cand, w.owner, w.owner_next, w.choice, w.nm, stage, cand_cap(m));
  };
  go(0);
  UVO_HIP_CHECK(hipGetLastError());
  int32_t total = 0;
  UVO_HIP_CHECK(hipMemcpyAsync(&total, w.start + nmp, 4, hipMemcpyDeviceToHost, s));
  UVO_HIP_CHECK(hipStreamSynchronize(s));
  RC(reserve(m, S_CAND, (size_t)total, &d_cand));
  go(1);
  UVO_HIP_CHECK(hipGetLastError());
  int32_t nm = 0;
  UVO_HIP_CHECK(hipMemcpyAsync(assigned, d_assigned, (size_t)n * 4, hipMemcpyDeviceToHost, s));
  UVO_HIP_CHECK(hipMemcpyAsync(&nm, w.nm, 4, hipMemcpyDeviceToHost, s));
  UVO_HIP_CHECK(hipStreamSynchronize(s));
  *n_matches = nm;
  return UVO_OK;
}

// Tracking::SearchReferencePointsInFrustum (src/Tracking.cc:2176-2230) as one call: FrameKTL::isInFrustum on every local map
// point, then SearchByProjection(mCurrentFrame, mvpLocalMapPoints, th) on the ones in view.  All inputs travel as one packed block
// through a pinned mirror, the projection results never leave the device, and the host waits once.
int uvo_search_points_in_frustum(uvo_matcher* m, const uvo_keypoint* kp, int n, const uint8_t* desc, int32_t* assigned, const uvo_camera_pose* cam,
                                 int npts, const float* xyz, const float* normal, const float* min_distance_inv, const float* max_distance_inv,
                                 const float* max_distance, const uint8_t* usable, const uint8_t* mp_desc, const float* scale_factors, int nlevels,
                                 float scale_factor, float viewing_cos_limit, float th, float nnratio, uint8_t* in_view, float* proj_x,
                                 float* proj_y, int32_t* level, float* view_cos, int* n_to_match, int* n_matches) {
  if (!m || !n_matches || !cam) return fail(UVO_E_BADARG, "null pointer");
  *n_matches = 0;
  if (n_to_match) *n_to_match = 0;
  const int min_x = (int)cam->min_x, min_y = (int)cam->min_y, max_x = (int)cam->max_x, max_y = (int)cam->max_y;
  if (n < 0 || npts < 0 || n > m->cfg.max_query || npts > m->cfg.max_map_points || nlevels < 1 || nlevels > kMaxLevels * 4 || max_x <= min_x ||
      max_y <= min_y)
    return fail(UVO_E_BADARG, "sizes outside handle capacity");
  if (npts == 0) return UVO_OK;
  if (!xyz || !normal || !min_distance_inv || !max_distance_inv || !max_distance || !mp_desc || !scale_factors)
    return fail(UVO_E_BADARG, "null pointer");
  if (n > 0 && (!kp || !desc || !assigned)) return fail(UVO_E_BADARG, "null pointer");
  if (!(scale_factor > 1.0f)) return fail(UVO_E_BADARG, "scale_factor must be > 1");
  UVO_HIP_CHECK(hipSetDevice(m->device));
  hipStream_t s = m->stream;
  // ---- packed layout (offsets in bytes, every array 16-byte aligned) ----
  size_t off = 0;
  auto take = [&](size_t bytes) {
    const size_t o = off;
    off = (off + bytes + 15) & ~(size_t)15;
    return o;
  };
  const size_t N = (size_t)n, P = (size_t)npts;
  const size_t o_kp = take(N * sizeof(uvo_keypoint)), o_desc = take(N * 32), o_asg = take(N * 4), o_xyz = take(P * 12), o_nrm = take(P * 12);
  const size_t o_min = take(P * 4), o_max = take(P * 4), o_raw = take(P * 4), o_use = take(P), o_mpd = take(P * 32), o_sf = take((size_t)nlevels * 4);
  const size_t in_bytes = off;
  const size_t o_valid = take(P), o_u = take(P * 4), o_v = take(P * 4), o_lvl = take(P * 4), o_vc = take(P * 4), o_tail = take(16);
  const size_t total_bytes = off;
  uint8_t* D;
  RC(reserve(m, S_ARENA, total_bytes, &D));
  Buf& h = m->h_arena;
  if (h.cap < m->buf[S_ARENA].cap) {  // the slot grew (after draining the stream): the mirror follows
    if (h.p) (void)hipHostFree(h.p);
    h = Buf();
    if (hipHostMalloc(&h.p, m->buf[S_ARENA].cap, hipHostMallocDefault) != hipSuccess) {
      h.p = nullptr;
      return fail(UVO_E_NOMEM, "pinned staging allocation failed");
    }
    h.cap = m->buf[S_ARENA].cap;
  }
  uint8_t* H = static_cast<uint8_t*>(h.p);
  if (n > 0) {
    std::memcpy(H + o_kp, kp, N * sizeof(uvo_keypoint));
    std::memcpy(H + o_desc, desc, N * 32);
    std::memcpy(H + o_asg, assigned, N * 4);
  }
  std::memcpy(H + o_xyz, xyz, P * 12);
  std::memcpy(H + o_nrm, normal, P * 12);
  std::memcpy(H + o_min, min_distance_inv, P * 4);
  std::memcpy(H + o_max, max_distance_inv, P * 4);
  std::memcpy(H + o_raw, max_distance, P * 4);
  if (usable)
    std::memcpy(H + o_use, usable, P);
  else
    std::memset(H + o_use, 1, P);
  std::memcpy(H + o_mpd, mp_desc, P * 32);
  std::memcpy(H + o_sf, scale_factors, (size_t)nlevels * 4);
  UVO_HIP_CHECK(hipMemcpyAsync(D, H, in_bytes, hipMemcpyHostToDevice, s));
  uint8_t* d_valid = D + o_valid;
  float *d_u = (float*)(D + o_u), *d_v = (float*)(D + o_v), *d_vc = (float*)(D + o_vc);
  int32_t *d_lvl = (int32_t*)(D + o_lvl), *d_asg = (int32_t*)(D + o_asg);
  const float* d_sf = (const float*)(D + o_sf);
  {
    Profiler::Scope ps(&m->prof, "k_project", s);
    launch_project(s, UVO_PROJECT_FRUSTUM, *cam, npts, (const float*)(D + o_xyz), (const float*)(D + o_nrm), (const float*)(D + o_min),
                   (const float*)(D + o_max), (const float*)(D + o_raw), D + o_use, d_sf, nlevels, uvo_logf(scale_factor), viewing_cos_limit, d_valid,
                   d_u, d_v, d_lvl, d_vc);
  }
  int32_t total = 0, nm = 0;
  UVO_HIP_CHECK(hipGetLastError());
  if (n > 0) {
    // candidate lists: sized for 8 per map point up front; a denser frame is detected from the returned total and the match
    // stage is repeated once with a larger buffer (the kernels never write or read past the capacity they are given)
    SbpWork w;
    uint32_t* d_cand;
    RC(sbp_work(m, n, npts, &w));
    RC(reserve(m, S_CAND, P * 8, &d_cand));
    auto go = [&](int stage) {
      Profiler::Scope ps(&m->prof, stage ? "k_sbp_match" : "k_sbp_count", s);
      launch_sbp(s, (const uvo_keypoint*)(D + o_kp), n, D + o_desc, min_x, min_y, max_x, max_y, d_asg, npts, d_u, d_v, d_lvl, d_vc, d_valid, D + o_mpd,
                 d_sf, th, nnratio, w.cell_start, w.cell_items, w.cell_of, w.cnt, w.start, d_cand, w.owner, w.owner_next, w.choice, w.nm, stage,
                 cand_cap(m));
    };
    auto fetch = [&]() -> int {
      UVO_HIP_CHECK(hipGetLastError());
      UVO_HIP_CHECK(hipMemcpyAsync(H + o_asg, d_asg, N * 4, hipMemcpyDeviceToHost, s));
      UVO_HIP_CHECK(hipMemcpyAsync(H + o_tail, w.start + npts, 4, hipMemcpyDeviceToHost, s));
      UVO_HIP_CHECK(hipMemcpyAsync(H + o_tail + 4, w.nm, 4, hipMemcpyDeviceToHost, s));
      UVO_HIP_CHECK(hipMemcpyAsync(H + o_valid, d_valid, o_tail - o_valid, hipMemcpyDeviceToHost, s));
      UVO_HIP_CHECK(hipStreamSynchronize(s));
      return UVO_OK;
    };
    go(0);
    go(1);
    int rc = fetch();
    if (rc) return rc;
    std::memcpy(&total, H + o_tail, 4);
    if (total > cand_cap(m)) {
      RC(reserve(m, S_CAND, (size_t)total, &d_cand));
      UVO_HIP_CHECK(hipMemcpyAsync(d_asg, assigned, N * 4, hipMemcpyHostToDevice, s));  // undo the truncated run's assignments
      go(1);
      rc = fetch();
      if (rc) return rc;
    }
    std::memcpy(&nm, H + o_tail + 4, 4);
    std::memcpy(assigned, H + o_asg, N * 4);
  } else {
    UVO_HIP_CHECK(hipMemcpyAsync(H + o_valid, d_valid, o_tail - o_valid, hipMemcpyDeviceToHost, s));
    UVO_HIP_CHECK(hipStreamSynchronize(s));
  }
  int to_match = 0;
  for (size_t i = 0; i < P; ++i) to_match += H[o_valid + i] != 0;
  if (n_to_match) *n_to_match = to_match;
  if (in_view) std::memcpy(in_view, H + o_valid, P);
  if (proj_x) std::memcpy(proj_x, H + o_u, P * 4);
  if (proj_y) std::memcpy(proj_y, H + o_v, P * 4);
  if (level) std::memcpy(level, H + o_lvl, P * 4);
  if (view_cos) std::memcpy(view_cos, H + o_vc, P * 4);
  *n_matches = nm;
  return UVO_OK;
}

hipStream_t uvo_matcher_stream_internal(uvo_matcher* m) { return m->stream; }
// Called by the extractor a matcher is attached to: whenever a batch moves to another pipeline lane the followers move with it (a
// matcher that kept the previous lane's stream would read the new batch's descriptors with no ordering at all), and when the
// extractor is destroyed they go back to their own streams instead of keeping a dead one.
void uvo_matcher_follow_internal(uvo_matcher* m, hipStream_t s) {
  if (m->stream == s) return;
  if (m->prof.on) (void)hipStreamSynchronize(m->stream);  // the profiler's open events belong to the stream they were recorded on
  m->stream = s;
}
void uvo_matcher_orphaned_internal(uvo_matcher* m) {
  m->attached_to = nullptr;
  m->stream = m->own_stream;
}

int uvo_matcher_wait_extractor(uvo_matcher* m, uvo_extractor* h) {
  if (!m || !h) return fail(UVO_E_BADARG, "null handle");
  if (uvo_extractor_device_internal(h) != m->device) return fail(UVO_E_BADARG, "handles live on different devices");
  UVO_HIP_CHECK(hipSetDevice(m->device));
  UVO_HIP_CHECK(hipEventRecord(m->ev, uvo_extractor_stream_internal(h)));
  UVO_HIP_CHECK(hipStreamWaitEvent(m->stream, m->ev, 0));
  return UVO_OK;
}

int uvo_extractor_wait_matcher(uvo_extractor* h, uvo_matcher* m) {
  if (!m || !h) return fail(UVO_E_BADARG, "null handle");
  if (uvo_extractor_device_internal(h) != m->device) return fail(UVO_E_BADARG, "handles live on different devices");
  UVO_HIP_CHECK(hipSetDevice(m->device));
  UVO_HIP_CHECK(hipEventRecord(m->ev, m->stream));
  UVO_HIP_CHECK(hipStreamWaitEvent(uvo_extractor_stream_internal(h), m->ev, 0));
  return UVO_OK;
}

// Event hand-offs between two queues cost tens of microseconds each on this runtime (tools/step_trace_summary.py: 0.32 ms between a
// lane's k_describe and its next k_pad_level0 with the matcher on its own stream -- two hand-offs around a 0.13 ms kernel); in the
// extractor lane's own stream the matcher's kernels simply queue up behind the batch that feeds them.
int uvo_matcher_attach_extractor(uvo_matcher* m, uvo_extractor* h) {
  if (!m) return fail(UVO_E_BADARG, "null handle");
  UVO_HIP_CHECK(hipSetDevice(m->device));
  if (h && uvo_extractor_device_internal(h) != m->device) return fail(UVO_E_BADARG, "handles live on different devices");
  if (m->prof.on) UVO_HIP_CHECK(hipStreamSynchronize(m->stream));  // the profiler's open events belong to the stream they were recorded on
  if (m->attached_to && m->attached_to != h) uvo_extractor_drop_follower_internal(m->attached_to, m);
  m->attached_to = h;
  if (!h) {
    m->stream = m->own_stream;
    return UVO_OK;
  }
  uvo_extractor_add_follower_internal(h, m);  // from now on the extractor moves this handle's stream with its batches
  m->stream = uvo_extractor_stream_internal(h);
  return UVO_OK;
}

int uvo_matcher_profile(uvo_matcher* m, int enable) {
  if (!m) return fail(UVO_E_BADARG, "null handle");
  UVO_HIP_CHECK(hipSetDevice(m->device));
  UVO_HIP_CHECK(hipStreamSynchronize(m->stream));
  m->prof.on = enable != 0;
  m->prof.clear();
  return UVO_OK;
}

int uvo_matcher_kernel_times(uvo_matcher* m, char* names, int names_cap, float* ms, int32_t* launches, int cap, int* n) {
  if (!m || !names || !ms || !launches || !n) return fail(UVO_E_BADARG, "null pointer");
  UVO_HIP_CHECK(hipSetDevice(m->device));
  UVO_HIP_CHECK(hipStreamSynchronize(m->stream));
  *n = m->prof.report(names, names_cap, ms, launches, cap);
  return UVO_OK;
}

}  // extern "C"
