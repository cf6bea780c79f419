// Host side of uvo_kfdb_* (include/uvo/uvo.h): the slots' device arrays, one row upload per add, one staging copy up and one result
// copy down per query.  The small per-slot arrays (add sequence, flags, BoW length) and the covisible rows are mirrored in pinned host
// memory and flushed in front of the next query; the mnIds stay on the host, where the haloc query's exclusions are decided; the kernels are in kfdb.hip, the rules in kfdb_core.hpp.
// Not thread-safe: the reference guards its database with one mutex, the adaptor (include/uvo/compat/KeyFrameDatabase.h) does the same.
#include <string.h>

#include <algorithm>
#include <unordered_set>
#include <vector>

#include "devmem.hpp"
#include "kfdb.hpp"
#include "kfdb_core.hpp"

using namespace uvo;

struct uvo_kfdb {
  int device = 0, max_kf = 0, max_words = 0, hash_len = 0, npad = 0;
  int n_slots = 0;
  hipStream_t stream = nullptr;
  DevMem mem;  // owns every d_* and the pinned block of the h_*
  // device, per slot
  uint32_t* d_seq = nullptr;
  int32_t *d_slot_of_seq = nullptr, *d_kf_n = nullptr, *d_cov = nullptr;
  uint8_t *d_in_file = nullptr, *d_has_hash = nullptr;
  uint32_t* d_bow_id = nullptr;
  double* d_bow_val = nullptr;
  float* d_hash_t = nullptr;
  uvo_kfdb_fields* d_state = nullptr;
  // device, per query
  uint8_t* d_stage = nullptr;
  int32_t *d_cnt = nullptr, *d_first = nullptr, *d_first_r = nullptr, *d_out = nullptr;
  float *d_score = nullptr, *d_hm = nullptr;
  uint64_t* d_keys = nullptr;
  uvo_kfdb_query_row* d_rows = nullptr;
  // pinned host: mirrors, staging, results
  int64_t* h_id = nullptr;
  uint32_t* h_seq = nullptr;
  int32_t *h_slot_of_seq = nullptr, *h_kf_n = nullptr, *h_cov = nullptr, *h_out = nullptr;
  uint8_t *h_in_file = nullptr, *h_has_hash = nullptr, *h_stage = nullptr;
  size_t stage_bytes = 0;
  int meta_dirty_from = 0;  // slots from here on differ between mirror and device (n_slots: none)
  bool cov_dirty = false;
  int last_kind = 0;        // 0 nothing yet, 1 a BoW query, 2 a haloc query
  int last_listed = 0, last_maxc = 0, last_minc = 0, last_haloc_n = 0;
};

static size_t up16(size_t x) { return (x + 15) & ~(size_t)15; }

static int pad_pow2(int n) {
  int p = 2;
  while (p < n) p <<= 1;
  return p;
}

static KfdbView view_of(const uvo_kfdb* db) {
  KfdbView v{};
  v.n_slots = db->n_slots, v.max_kf = db->max_kf, v.max_words = db->max_words, v.hash_len = db->hash_len;
  v.seq = db->d_seq, v.slot_of_seq = db->d_slot_of_seq, v.in_file = db->d_in_file, v.has_hash = db->d_has_hash, v.kf_n = db->d_kf_n;
  v.bow_id = db->d_bow_id, v.bow_val = db->d_bow_val, v.hash_t = db->d_hash_t, v.cov = db->d_cov, v.state = db->d_state;
  v.cnt = db->d_cnt, v.first = db->d_first, v.score = db->d_score, v.keys = db->d_keys, v.first_r = db->d_first_r, v.rows = db->d_rows, v.hm = db->d_hm;
  v.out = db->d_out;
  return v;
}

// mirror -> device for everything a query reads that add / erase / set_covisibles changed since the last one
static int flush(uvo_kfdb* db) {
  hipStream_t s = db->stream;
  const int a = db->meta_dirty_from, n = db->n_slots - a;
  if (n > 0) {
    UVO_HIP_CHECK(hipMemcpyAsync(db->d_seq + a, db->h_seq + a, (size_t)n * 4, hipMemcpyHostToDevice, s));
    UVO_HIP_CHECK(hipMemcpyAsync(db->d_slot_of_seq + a, db->h_slot_of_seq + a, (size_t)n * 4, hipMemcpyHostToDevice, s));
    UVO_HIP_CHECK(hipMemcpyAsync(db->d_kf_n + a, db->h_kf_n + a, (size_t)n * 4, hipMemcpyHostToDevice, s));
    UVO_HIP_CHECK(hipMemcpyAsync(db->d_in_file + a, db->h_in_file + a, (size_t)n, hipMemcpyHostToDevice, s));
    UVO_HIP_CHECK(hipMemcpyAsync(db->d_has_hash + a, db->h_has_hash + a, (size_t)n, hipMemcpyHostToDevice, s));
  }
  db->meta_dirty_from = db->n_slots;
  if (db->cov_dirty && db->n_slots > 0)
    UVO_HIP_CHECK(hipMemcpyAsync(db->d_cov, db->h_cov, (size_t)db->n_slots * kfdb::kCovisibles * 4, hipMemcpyHostToDevice, s));
  db->cov_dirty = false;
  return UVO_OK;
}

static int check_bow(const uvo_kfdb* db, const uint32_t* bow_id, const double* bow_value, int n_bow) {
  if (n_bow < 0) return fail(UVO_E_BADARG, "negative BoW length");
  if (n_bow > db->max_words) return fail(UVO_E_CAPACITY, "BoW vector longer than max_words");
  if (n_bow > 0 && (!bow_id || !bow_value)) return fail(UVO_E_BADARG, "null BoW vector");
  for (int i = 1; i < n_bow; ++i)
    if (bow_id[i] <= bow_id[i - 1]) return fail(UVO_E_BADARG, "BoW ids must ascend strictly (unsorted or duplicate id)");
  return UVO_OK;
}

static int bow_query(uvo_kfdb* db, int mode, int64_t id, const uint32_t* bow_id, const double* bow_value, int n_bow, const int32_t* connected, int n_connected,
                     float min_score, int32_t* cand_slot, int cap, int* n_cand) {
  if (!db || !n_cand) return fail(UVO_E_BADARG, "null pointer");
  *n_cand = 0;
  if (cap < 0 || (cap > 0 && !cand_slot)) return fail(UVO_E_BADARG, "bad candidate buffer");
  RC(check_bow(db, bow_id, bow_value, n_bow));
  if (n_connected < 0 || (n_connected > 0 && !connected)) return fail(UVO_E_BADARG, "bad connected list");
  for (int i = 0; i < n_connected; ++i)
    if (connected[i] < 0 || connected[i] >= db->n_slots) return fail(UVO_E_BADARG, "connected slot holds no keyframe");
  if (min_score != min_score) return fail(UVO_E_BADARG, "minScore is NaN");
  db->last_kind = 1, db->last_listed = 0, db->last_maxc = 0, db->last_minc = 0;
  if (db->n_slots == 0 || n_bow == 0) return UVO_OK;  // no word, no inverted list: nothing is touched
  UVO_HIP_CHECK(hipSetDevice(db->device));
  hipStream_t s = db->stream;
  RC(flush(db));
  const size_t off_id = (size_t)n_bow * 8, off_conn = up16((size_t)n_bow * 12), total = off_conn + (mode == kfdb::kLoop ? (size_t)db->n_slots : 0);
  memcpy(db->h_stage, bow_value, (size_t)n_bow * 8);
  memcpy(db->h_stage + off_id, bow_id, (size_t)n_bow * 4);
  if (mode == kfdb::kLoop) {
    memset(db->h_stage + off_conn, 0, (size_t)db->n_slots);
    for (int i = 0; i < n_connected; ++i) db->h_stage[off_conn + (size_t)connected[i]] = 1;
  }
  UVO_HIP_CHECK(hipMemcpyAsync(db->d_stage, db->h_stage, total, hipMemcpyHostToDevice, s));
  KfdbView v = view_of(db);
  v.q_val = reinterpret_cast<const double*>(db->d_stage);
  v.q_id = reinterpret_cast<const uint32_t*>(db->d_stage + off_id);
  v.connected = db->d_stage + off_conn;
  (void)hipGetLastError();  // an error an earlier, unrelated call left behind is not this launch's
  launch_kfdb_bow(s, v, mode, id, n_bow, min_score);
  UVO_HIP_CHECK(hipGetLastError());
  const int want = std::min(cap, db->n_slots);
  UVO_HIP_CHECK(hipMemcpyAsync(db->h_out, db->d_out, (size_t)(kKfdbMeta + want) * 4, hipMemcpyDeviceToHost, s));
  UVO_HIP_CHECK(hipStreamSynchronize(s));
  db->last_listed = db->h_out[0], db->last_maxc = db->h_out[2], db->last_minc = db->h_out[3];
  *n_cand = db->h_out[1];
  if (*n_cand > cap) return fail(UVO_E_CAPACITY, "more candidates than the output capacity");
  for (int i = 0; i < *n_cand; ++i) cand_slot[i] = db->h_out[kKfdbMeta + i];
  return UVO_OK;
}

extern "C" {

void uvo_kfdb_destroy(uvo_kfdb* db) {
  if (!db) return;
  hipSetDevice(db->device);
  if (db->stream) hipStreamSynchronize(db->stream);
  db->mem.release_all();
  if (db->stream) hipStreamDestroy(db->stream);
  delete db;
}

int uvo_kfdb_create(int max_keyframes, int max_words, int hash_len, int device, uvo_kfdb** out) {
  if (!out) return fail(UVO_E_BADARG, "null pointer");
  *out = nullptr;
  if (max_keyframes < 1 || max_keyframes > kKfdbMaxKeyframes || max_words < 1 || max_words > kKfdbMaxWords || hash_len < 1 || hash_len > kKfdbMaxHash)
    return fail(UVO_E_BADARG, "max_keyframes 1..65536, max_words 1..4096, hash_len 1..4096");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(UVO_E_NODEVICE, "no HIP device available (no CPU fallback exists)");
  if (device < 0 || device >= ndev) return fail(UVO_E_BADARG, "device ordinal out of range");
  uvo_kfdb* db = new uvo_kfdb();
  db->device = device, db->max_kf = max_keyframes, db->max_words = max_words, db->hash_len = hash_len, db->npad = pad_pow2(max_keyframes);
  if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&db->stream, hipStreamNonBlocking) != hipSuccess) {
    delete db;
    return fail(UVO_E_HIP, "stream creation failed");
  }
  const size_t K = (size_t)max_keyframes, W = (size_t)max_words, H = (size_t)hash_len, C = kfdb::kCovisibles;
  // staging: a BoW query (values, ids, connected flags) or a haloc query (hash, skip flags)
  db->stage_bytes = std::max(up16(W * 12) + K, up16(H * 4) + K) + 16;
  const size_t n_out = kKfdbMeta + std::max(K, (size_t)3);
  auto alloc_all = [&, &m = db->mem]() {
    RC(m.alloc(&db->d_seq, K));
    RC(m.alloc(&db->d_slot_of_seq, K));
    RC(m.alloc(&db->d_kf_n, K));
    RC(m.alloc(&db->d_cov, K * C));
    RC(m.alloc(&db->d_in_file, K));
    RC(m.alloc(&db->d_has_hash, K));
    RC(m.alloc(&db->d_bow_id, K * W));
    RC(m.alloc(&db->d_bow_val, K * W));
    RC(m.alloc(&db->d_hash_t, K * H));
    RC(m.alloc(&db->d_state, K));
    RC(m.alloc(&db->d_stage, db->stage_bytes));
    RC(m.alloc(&db->d_cnt, K));
    RC(m.alloc(&db->d_first, K));
    RC(m.alloc(&db->d_first_r, K));
    RC(m.alloc(&db->d_out, n_out));
    RC(m.alloc(&db->d_score, K));
    RC(m.alloc(&db->d_hm, K));
    RC(m.alloc(&db->d_keys, (size_t)db->npad));
    RC(m.alloc(&db->d_rows, K));
    // one pinned block: mirrors, results, staging
    return alloc_carved(m, [&](Carve& c) {
      c.take(db->h_id, K, 16).take(db->h_seq, K, 16).take(db->h_slot_of_seq, K, 16).take(db->h_kf_n, K, 16).take(db->h_cov, K * C, 16);
      c.take(db->h_out, n_out, 16).take(db->h_in_file, K, 16).take(db->h_has_hash, K, 16).take(db->h_stage, db->stage_bytes, 16);
    }, true);
  };
  if (const int rc = alloc_all()) return uvo_kfdb_destroy(db), rc;
  *out = db;
  return UVO_OK;
}

int uvo_kfdb_size(uvo_kfdb* db) { return db ? db->n_slots : fail(UVO_E_BADARG, "null pointer"); }

int uvo_kfdb_add(uvo_kfdb* db, int64_t id, const uint32_t* bow_id, const double* bow_value, int n_bow, const float* hash, int* slot) {
  if (!db || !slot) return fail(UVO_E_BADARG, "null pointer");
  *slot = -1;
  RC(check_bow(db, bow_id, bow_value, n_bow));
  if (db->n_slots >= db->max_kf) return fail(UVO_E_CAPACITY, "every slot is taken");
  UVO_HIP_CHECK(hipSetDevice(db->device));
  hipStream_t s = db->stream;
  const int k = db->n_slots;
  // the row: BoW ids, BoW values, the hash as one column of the transposed table, the six fields at their constructor values
  if (n_bow) {
    UVO_HIP_CHECK(hipMemcpyAsync(db->d_bow_id + (size_t)k * db->max_words, bow_id, (size_t)n_bow * 4, hipMemcpyHostToDevice, s));
    UVO_HIP_CHECK(hipMemcpyAsync(db->d_bow_val + (size_t)k * db->max_words, bow_value, (size_t)n_bow * 8, hipMemcpyHostToDevice, s));
  }
  if (hash) UVO_HIP_CHECK(hipMemcpy2DAsync(db->d_hash_t + k, (size_t)db->max_kf * 4, hash, 4, 4, (size_t)db->hash_len, hipMemcpyHostToDevice, s));
  UVO_HIP_CHECK(hipMemsetAsync(db->d_state + k, 0, sizeof(uvo_kfdb_fields), s));
  UVO_HIP_CHECK(hipStreamSynchronize(s));  // the caller's buffers are free again
  db->h_id[k] = id, db->h_seq[k] = (uint32_t)k, db->h_slot_of_seq[k] = k;  // slots are handed out in add order and freed only by clear
  db->h_kf_n[k] = n_bow, db->h_in_file[k] = 1, db->h_has_hash[k] = hash ? 1 : 0;
  for (int c = 0; c < kfdb::kCovisibles; ++c) db->h_cov[(size_t)k * kfdb::kCovisibles + c] = -1;
  db->cov_dirty = true;
  db->meta_dirty_from = std::min(db->meta_dirty_from, k);
  db->n_slots = k + 1;
  *slot = k;
  return UVO_OK;
}

int uvo_kfdb_erase(uvo_kfdb* db, int slot) {
  if (!db) return fail(UVO_E_BADARG, "null pointer");
  if (slot < 0 || slot >= db->n_slots) return fail(UVO_E_BADARG, "slot holds no keyframe");
  if (db->h_in_file[slot]) {
    db->h_in_file[slot] = 0;
    db->meta_dirty_from = std::min(db->meta_dirty_from, slot);
  }
  return UVO_OK;
}

int uvo_kfdb_clear(uvo_kfdb* db) {
  if (!db) return fail(UVO_E_BADARG, "null pointer");
  db->n_slots = 0, db->meta_dirty_from = 0, db->cov_dirty = false, db->last_kind = 0, db->last_listed = 0, db->last_haloc_n = 0;
  return UVO_OK;
}

int uvo_kfdb_set_covisibles(uvo_kfdb* db, int slot, const int32_t* neigh_slots, int n) {
  if (!db) return fail(UVO_E_BADARG, "null pointer");
  if (slot < 0 || slot >= db->n_slots) return fail(UVO_E_BADARG, "slot holds no keyframe");
  if (n < 0 || n > kfdb::kCovisibles || (n > 0 && !neigh_slots)) return fail(UVO_E_BADARG, "0..10 covisibles");
  for (int c = 0; c < n; ++c)
    if (neigh_slots[c] < -1 || neigh_slots[c] >= db->n_slots) return fail(UVO_E_BADARG, "covisible slot holds no keyframe");
  int32_t* row = db->h_cov + (size_t)slot * kfdb::kCovisibles;
  bool same = true;
  for (int c = 0; c < kfdb::kCovisibles; ++c) {
    const int32_t x = c < n ? neigh_slots[c] : -1;
    same = same && row[c] == x;
    row[c] = x;
  }
  if (!same) db->cov_dirty = true;
  return UVO_OK;
}

int uvo_kfdb_detect_reloc(uvo_kfdb* db, int64_t query_id, const uint32_t* bow_id, const double* bow_value, int n_bow, int32_t* cand_slot, int cap, int* n_cand) {
  return bow_query(db, kfdb::kReloc, query_id, bow_id, bow_value, n_bow, nullptr, 0, 0.0f, cand_slot, cap, n_cand);
}

int uvo_kfdb_detect_loop(uvo_kfdb* db, int64_t query_id, const uint32_t* bow_id, const double* bow_value, int n_bow, const int32_t* connected_slots, int n_connected,
                         float min_score, int32_t* cand_slot, int cap, int* n_cand) {
  return bow_query(db, kfdb::kLoop, query_id, bow_id, bow_value, n_bow, connected_slots, n_connected, min_score, cand_slot, cap, n_cand);
}

int uvo_kfdb_detect_loop_haloc(uvo_kfdb* db, int64_t query_id, const float* hash, const int64_t* exclude_ids, int n_exclude, float max_score, int32_t cand_slot[3],
                               int* n_cand) {
  if (!db || !n_cand || !cand_slot) return fail(UVO_E_BADARG, "null pointer");
  *n_cand = 0;
  if (n_exclude < 0 || (n_exclude > 0 && !exclude_ids)) return fail(UVO_E_BADARG, "bad exclude list");
  if (max_score != max_score) return fail(UVO_E_BADARG, "maxScore is NaN");
  db->last_kind = 2, db->last_haloc_n = db->n_slots;
  if (db->n_slots == 0) return UVO_OK;
  UVO_HIP_CHECK(hipSetDevice(db->device));
  hipStream_t s = db->stream;
  RC(flush(db));
  // who is not compared (:106-110), decided here: the ids are mirrored on the host, and the list may name keyframes the database never saw
  const size_t off_skip = up16((size_t)db->hash_len * 4), total = off_skip + (size_t)db->n_slots;
  if (hash) memcpy(db->h_stage, hash, (size_t)db->hash_len * 4);
  std::unordered_set<int64_t> no_candidates(exclude_ids, exclude_ids + n_exclude);
  no_candidates.insert(query_id);
  for (int k = 0; k < db->n_slots; ++k) db->h_stage[off_skip + (size_t)k] = no_candidates.count(db->h_id[k]) ? 1 : 0;
  UVO_HIP_CHECK(hipMemcpyAsync(db->d_stage, db->h_stage, total, hipMemcpyHostToDevice, s));
  KfdbView v = view_of(db);
  v.q_hash = reinterpret_cast<const float*>(db->d_stage);
  v.skip = db->d_stage + off_skip;
  (void)hipGetLastError();
  launch_kfdb_haloc(s, v, hash ? 1 : 0, max_score);
  UVO_HIP_CHECK(hipGetLastError());
  UVO_HIP_CHECK(hipMemcpyAsync(db->h_out, db->d_out, (size_t)(kKfdbMeta + 3) * 4, hipMemcpyDeviceToHost, s));
  UVO_HIP_CHECK(hipStreamSynchronize(s));
  *n_cand = db->h_out[1];
  for (int i = 0; i < *n_cand; ++i) cand_slot[i] = db->h_out[kKfdbMeta + i];
  return UVO_OK;
}

int uvo_kfdb_last_query(uvo_kfdb* db, uvo_kfdb_query_row* rows, int cap, int* n, int* max_common, int* min_common) {
  if (!db || !n) return fail(UVO_E_BADARG, "null pointer");
  *n = 0;
  if (db->last_kind != 1) return fail(UVO_E_BADARG, "no BoW query since create / clear");
  if (max_common) *max_common = db->last_maxc;
  if (min_common) *min_common = db->last_minc;
  *n = db->last_listed;
  if (db->last_listed > cap) return fail(UVO_E_CAPACITY, "more listed keyframes than the output capacity");
  if (db->last_listed == 0) return UVO_OK;
  if (!rows) return fail(UVO_E_BADARG, "null rows");
  UVO_HIP_CHECK(hipSetDevice(db->device));
  UVO_HIP_CHECK(hipMemcpyAsync(rows, db->d_rows, (size_t)db->last_listed * sizeof(uvo_kfdb_query_row), hipMemcpyDeviceToHost, db->stream));
  UVO_HIP_CHECK(hipStreamSynchronize(db->stream));
  return UVO_OK;
}

int uvo_kfdb_last_haloc(uvo_kfdb* db, float* m, uint8_t* kept, int cap, int* n) {
  if (!db || !n) return fail(UVO_E_BADARG, "null pointer");
  *n = 0;
  if (db->last_kind != 2) return fail(UVO_E_BADARG, "no haloc query since create / clear");
  const int k = db->last_haloc_n;
  *n = k;
  if (k > cap) return fail(UVO_E_CAPACITY, "more slots than the output capacity");
  if (k == 0) return UVO_OK;
  if (!m || !kept) return fail(UVO_E_BADARG, "null outputs");
  UVO_HIP_CHECK(hipSetDevice(db->device));
  std::vector<uint64_t> keys((size_t)k);
  UVO_HIP_CHECK(hipMemcpyAsync(m, db->d_hm, (size_t)k * 4, hipMemcpyDeviceToHost, db->stream));
  UVO_HIP_CHECK(hipMemcpyAsync(keys.data(), db->d_keys, (size_t)k * 8, hipMemcpyDeviceToHost, db->stream));
  UVO_HIP_CHECK(hipStreamSynchronize(db->stream));
  for (int i = 0; i < k; ++i) kept[i] = keys[(size_t)i] != kfdb::kNoKey;
  return UVO_OK;
}

int uvo_kfdb_state(uvo_kfdb* db, int first_slot, int n, uvo_kfdb_fields* out) {
  if (!db || !out) return fail(UVO_E_BADARG, "null pointer");
  if (first_slot < 0 || n < 0 || first_slot + n > db->n_slots) return fail(UVO_E_BADARG, "slot holds no keyframe");
  if (n == 0) return UVO_OK;
  UVO_HIP_CHECK(hipSetDevice(db->device));
  UVO_HIP_CHECK(hipMemcpyAsync(out, db->d_state + first_slot, (size_t)n * sizeof(uvo_kfdb_fields), hipMemcpyDeviceToHost, db->stream));
  UVO_HIP_CHECK(hipStreamSynchronize(db->stream));
  return UVO_OK;
}

}  // extern "C"
