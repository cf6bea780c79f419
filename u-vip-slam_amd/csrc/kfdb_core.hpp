// Arithmetic and per-keyframe rules of the keyframe database (uvo_kfdb_*, include/uvo/uvo.h), shared by the device kernels (kfdb.hip) and
// the host build the CPU suite runs (tests/emu/kfdb_emu.cpp).  Everything here is one keyframe's (or one list entry's) share of
//   KeyFrameDatabase::DetectRelocalisationCandidates  src/KeyFrameDatabase.cc:267-377
//   KeyFrameDatabase::DetectLoopCandidates            src/KeyFrameDatabase.cc:144-265
//   KeyFrameDatabase::DetectLoopCandidatesHaloc       src/KeyFrameDatabase.cc:74-136, haloc::Hash::match src/hash.cpp:189-205
//   DBoW2::L1Scoring::score                           Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68
// written so that the caller only decides who runs it: one wavefront or lane per slot on the device, a serial loop on the host.
// Built with -ffp-contract=off on both sides: every operation below rounds once, in the order written.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/uvo/uvo.h"

#if defined(__HIPCC__)
#define KFDB_HD __host__ __device__ __forceinline__
#else
#define KFDB_HD inline
#endif

namespace uvo {
namespace kfdb {

constexpr int kReloc = 0, kLoop = 1;
constexpr int kCovisibles = UVO_KFDB_COVISIBLES;  // GetBestCovisibilityKeyFrames(10)
constexpr uint64_t kNoKey = ~0ull;                // sorts behind every real key

// index of word w in the ascending ids[0..n), -1 when absent
KFDB_HD int find_word(const uint32_t* ids, int n, uint32_t w) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (ids[mid] < w) lo = mid + 1; else hi = mid;
  }
  return (lo < n && ids[lo] == w) ? lo : -1;
}

// one common word's term of the L1 score (ScoringObject.cpp:41); vi: the query's value, wi: the keyframe's
KFDB_HD double l1_term(double vi, double wi) { return fabs(vi - wi) - fabs(vi) - fabs(wi); }
// :65 and the float the callers keep it in (KeyFrameDatabase.cc:201, :317)
KFDB_HD float l1_finish(double sum) { return (float)(-sum / 2.0); }

// int minCommonWords = maxCommonWords*0.8f  (:188, :303): a float product, truncated
KFDB_HD int min_common_words(int max_common) { return (int)((float)max_common * 0.8f); }

// The inverted-file walk (:154-172, :275-290) as seen by ONE keyframe that shares c > 0 words with the query: query / words are its stored
// mn{Loop,Reloc}Query / mn{Loop,Reloc}Words, updated in place.  Returns whether the walk lists it.
KFDB_HD bool touch(int mode, int64_t id, int c, bool connected, int64_t& query, int32_t& words) {
  if (c <= 0) return false;
  if (query == id) {  // the != test never fires: the count goes on from the stored value and the keyframe is not listed
    words = (int32_t)((uint32_t)words + (uint32_t)c);
    return false;
  }
  if (mode == kLoop && connected) {  // reset at every word, never marked: ends at 1
    words = 1;
    return false;
  }
  query = id;
  words = c;
  return true;
}

// list order = first touch: (index of the first common query word, add sequence), unique per keyframe
KFDB_HD uint64_t list_key(int first, uint32_t seq) { return ((uint64_t)(uint32_t)first << 32) | seq; }

// accumulation over the covisibles of one scored entry (:216-241, :330-355); st = the slots' state AFTER the scoring loop
KFDB_HD void accumulate(int mode, int64_t id, int min_common, float si, int slot, const int32_t* cov, const uvo_kfdb_fields* st, float& acc, int& best) {
  float best_score = si;
  acc = si;
  best = slot;
  for (int k = 0; k < kCovisibles; ++k) {
    const int nb = cov[k];
    if (nb < 0) continue;
    float s2;
    if (mode == kLoop) {
      if (!(st[nb].loop_query == id && st[nb].loop_words > min_common)) continue;
      s2 = st[nb].loop_score;
    } else {
      if (st[nb].reloc_query != id) continue;
      s2 = st[nb].reloc_score;
    }
    acc += s2;
    if (s2 > best_score) {
      best = nb;
      best_score = s2;
    }
  }
}

// haloc::Hash::match: 1.0f is EXIT_FAILURE as a float.  t is read with a stride (the database keeps the hashes transposed).
KFDB_HD float hash_match(const float* q, bool q_has, const float* t, int64_t t_stride, bool t_has, int len) {
  if (!q_has || !t_has) return 1.0f;
  float sum = 0.0f;
  for (int i = 0; i < len; ++i) sum += fabsf(q[i] - t[(int64_t)i * t_stride]);
  if (sum != sum) return 1.0f;
  return sum;
}
// if (m < maxScore*0.8): the literal 0.8 is a double, so both sides are
KFDB_HD bool haloc_keep(float m, float max_score) { return (double)m < (double)max_score * 0.8; }
// order of the kept matches: m ascending (m is never negative nor NaN, so its bits order as it does), ties by add sequence
KFDB_HD uint64_t haloc_key(float m, uint32_t seq) {
  uint32_t b;
  memcpy(&b, &m, 4);
  return ((uint64_t)b << 32) | seq;
}

}  // namespace kfdb
}  // namespace uvo
