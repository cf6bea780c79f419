// Private to the matcher translation units (matcher.cpp, matcher_search.cpp, matcher_batch.cpp): the handle behind uvo_matcher* and
// the one way its device buffers are obtained.
#pragma once
#include <algorithm>

#include "common.hpp"
#include "profiler.hpp"

namespace uvo {

// Every device buffer of the handle is a slot.  Within one entry point, every array that is live at the same time has its own slot:
// a slot requested twice in one call hands back the same memory (and a growth frees what the first request returned).  Entry points
// share slots with each other -- nothing a slot holds outlives the call that wrote it.
enum Slot {
  // reserved by uvo_matcher_create for max_query (Q), max_train (T), max_batch (B) and max_map_points (MP)
  S_Q,            // knn2 / matrix queries, SearchByProjection key point descriptors [Q][32]
  S_T,            // knn2 / matrix train rows [T][32]
  S_IDX0, S_IDX1, S_D0, S_D1,  // knn2 results [B][Q]
  S_KP,           // the searched frame's key points [Q]
  S_ASSIGNED,     // SearchByProjection: key point -> map point [Q]
  S_CELL_START, S_CELL_ITEMS, S_CELL_OF,  // the 64x48 key point grid: cell offsets [64 * 48 + 1], items and cell of each key point [Q]
  S_OWNER, S_OWNER2,                      // ownership of the key points [Q]
  S_PX, S_PY, S_VC, S_LEVEL, S_INVIEW, S_MPDESC,  // projected map points: u, v, viewing cosine, level, in view [MP], descriptors [MP][32]
  S_CNT, S_START,  // candidates per query and their offsets [MP + 1]
  S_CHOICE,        // SearchByProjection: map point -> key point [MP]
  S_SCALE,         // scale factors [4 * kMaxLevels]
  S_NM,            // match count
  // grown on demand
  S_CAND,          // packed candidate lists
  S_MASK, S_DIST,  // knn2 mask, distance matrix
  S_MD_DESC, S_MD_OFF, S_MD_RES,  // distinctive descriptors: rows, offsets, results
  S_ARENA,         // uvo_search_points_in_frustum's packed block (pinned host mirror: uvo_matcher::h_arena)
  S_TDESC, S_TLEVEL, S_TANGLE, S_BLOCKED,  // targets of the generic engine
  S_QX, S_QY, S_QR, S_QMIN, S_QMAX, S_QVALID, S_QDESC, S_QANGLE, S_QPAIR,  // queries of the generic engine
  S_CIDX, S_MATCH, S_STEAL, S_MISC,  // caller-given candidates, per-query results, the steal rule's scratch, packed extras
  S_COUNT
};
constexpr int kGridCells = 64 * 48;

struct Buf {
  void* p = nullptr;
  size_t cap = 0;  // bytes
};

}  // namespace uvo

struct uvo_matcher {
  uvo_matcher_cfg cfg;
  int device = 0;
  hipStream_t stream = nullptr;      // where the handle's work is enqueued: its own stream, or an extractor lane's (uvo_matcher_attach_extractor)
  hipStream_t own_stream = nullptr;
  uvo_extractor* attached_to = nullptr;  // the extractor whose current lane `stream` follows (it keeps a list of its followers and lets go of them when it dies)
  hipEvent_t ev = nullptr;
  uvo::Buf buf[uvo::S_COUNT];  // device slots (uvo::ensure)
  uvo::Buf h_arena;            // pinned host mirror of slot S_ARENA, grown with it
  void* tri_batch = nullptr;   // candidate lists of uvo_search_for_triangulation_batch (uvo::TriBatch, matcher_batch.cpp)
  uvo::Profiler prof;
};

namespace uvo {
void tri_batch_free(void* p);

// device buffer of at least `bytes` in `slot` (contents undefined after growth).  Growth: bytes + bytes/2 + 256, after the handle's
// stream has drained (the old buffer may still be read by enqueued work).
inline int ensure(uvo_matcher* m, Slot slot, size_t bytes, void** out) {
  Buf& b = m->buf[slot];
  if (bytes > b.cap) {
    if (b.p) {
      UVO_HIP_CHECK(hipStreamSynchronize(m->stream));
      (void)hipFree(b.p);
      b = Buf();
    }
    const size_t want = bytes + bytes / 2 + 256;
    RC(dev_malloc(&b.p, want));
    b.cap = want;
  }
  *out = b.p;
  return UVO_OK;
}

// `count` elements in `slot`, the first `count` of them copied from src (when given) on the handle's stream
template <class T>
int upload(uvo_matcher* m, Slot slot, const T* src, size_t count, T** dev) {
  void* p = nullptr;
  RC(ensure(m, slot, std::max<size_t>(count, 1) * sizeof(T), &p));
  *dev = static_cast<T*>(p);
  if (count && src) UVO_HIP_CHECK(hipMemcpyAsync(p, src, count * sizeof(T), hipMemcpyHostToDevice, m->stream));
  return UVO_OK;
}
template <class T>
int reserve(uvo_matcher* m, Slot slot, size_t count, T** dev) {
  return upload<T>(m, slot, nullptr, count, dev);
}

// a feature vector (uvo_feature_vector) of strictly ascending nodes whose features index [0, n)
inline int check_fv(const uvo_feature_vector* fv, int n) {
  if (!fv || fv->n_nodes < 0) return fail(UVO_E_BADARG, "null feature vector");
  if (fv->n_nodes == 0) return UVO_OK;
  if (!fv->node || !fv->start || !fv->feat) return fail(UVO_E_BADARG, "null feature vector arrays");
  for (int k = 0; k < fv->n_nodes; ++k) {
    if (k && fv->node[k] <= fv->node[k - 1]) return fail(UVO_E_BADARG, "feature vector node ids must be strictly ascending");
    if (fv->start[k + 1] < fv->start[k]) return fail(UVO_E_BADARG, "feature vector offsets must be non-decreasing");
  }
  for (int e = fv->start[0]; e < fv->start[fv->n_nodes]; ++e)
    if (fv->feat[e] < 0 || fv->feat[e] >= n) return fail(UVO_E_BADARG, "feature index outside the keypoint range");
  return UVO_OK;
}

}  // namespace uvo
