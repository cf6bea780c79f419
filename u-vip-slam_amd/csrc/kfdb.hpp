// Device view of the keyframe database and the launchers of its two queries (kfdb.hip), shared with the host side (kfdb.cpp).
#pragma once
#include "common.hpp"

namespace uvo {

constexpr int kKfdbMaxKeyframes = 65536;
constexpr int kKfdbMaxWords = 4096;    // the query vector is staged in LDS: 12 bytes a word
constexpr int kKfdbMaxHash = 4096;
constexpr int kKfdbLdsSort = 4096;     // up to this many (padded) slots the list is ordered in LDS, beyond in global memory
constexpr int kKfdbMeta = 8;           // ints in front of the candidate list: n_listed, n_cand, maxCommonWords, minCommonWords, n_kept

struct KfdbView {
  int n_slots, max_kf, max_words, hash_len;
  // per slot
  const uint32_t* seq;         // add sequence number
  const int32_t* slot_of_seq;  // its inverse
  const uint8_t* in_file;      // in the inverted file (added, not erased)
  const uint8_t* has_hash;
  const int32_t* kf_n;         // BoW length
  const uint32_t* bow_id;      // [max_kf][max_words]
  const double* bow_val;       // [max_kf][max_words]
  const float* hash_t;         // [hash_len][max_kf]: lane = slot reads coalesce
  const int32_t* cov;          // [max_kf][10]
  uvo_kfdb_fields* state;
  // the query
  const double* q_val;
  const uint32_t* q_id;
  const uint8_t* connected;    // [n_slots], loop query only
  const float* q_hash;
  const uint8_t* skip;         // [n_slots], haloc query only: the query's own mnId or one of no_candidates
  // per-query scratch and results
  int32_t *cnt, *first;        // common words, index of the first common query word
  float* score;                // L1 score of every slot against the query
  uint64_t* keys;              // ordering keys, padded to a power of two
  int32_t* first_r;            // per slot: first retained list entry that elects it
  uvo_kfdb_query_row* rows;
  float* hm;                   // haloc distances
  int32_t* out;                // kKfdbMeta ints, then the candidate slots (room for three even in a smaller database)
};

void launch_kfdb_bow(hipStream_t s, const KfdbView& v, int mode, int64_t id, int nq, float min_score);
void launch_kfdb_haloc(hipStream_t s, const KfdbView& v, int q_has, float max_score);

}  // namespace uvo
