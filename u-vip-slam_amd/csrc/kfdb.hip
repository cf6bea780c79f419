// Keyframe database queries on the device (uvo_kfdb_detect_*, include/uvo/uvo.h; rules and arithmetic: kfdb_core.hpp).
//
// A BoW query is two launches in one stream, nothing read back between them:
//   k_kfdb_words        one wavefront per slot, the query vector staged in LDS.  Lanes stride over the keyframe's words and binary-search
//                       the query's ids; a ballot gives the common count and, from its first set bit, the first common query word (both
//                       id lists ascend, so the keyframe's first common word is the query's too).  The L1 terms are added by walking the
//                       ballot's set bits in order, every lane performing the same chain of double additions: the order is
//                       L1Scoring::score's, no tree, no reordering.
//   k_kfdb_bow_epilogue one workgroup: the inverted-file walk's effect on every slot's stored fields (kfdb::touch), maxCommonWords, the
//                       threshold, the score write-back, the list ordered by the unique key (first common word, add sequence) -- a
//                       bitonic sort, any correct sort gives the same list --, the covisibility accumulation per list entry, the best
//                       accumulated score, retention, first-occurrence dedup of the elected keyframes and the ordered candidate list.
// The haloc query likewise: k_kfdb_haloc_dist, one lane per slot over the transposed hashes (a chain of hash_len fp32 additions), then
// k_kfdb_haloc_top3, one workgroup that counts the kept matches and takes the three smallest (distance, add sequence) keys.
#include "kfdb.hpp"
#include "kfdb_core.hpp"

namespace uvo {

using namespace kfdb;

constexpr int kWordsThreads = 512;  // 8 slots per workgroup
constexpr int kEpiThreads = 1024;
constexpr int kEpiHdr = 64;         // bytes in front of the reduction array

__global__ __launch_bounds__(kWordsThreads) void k_kfdb_words(KfdbView v, int nq) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* s_val = reinterpret_cast<double*>(smem);
  uint32_t* s_id = reinterpret_cast<uint32_t*>(smem + (size_t)nq * 8);
  for (int i = threadIdx.x; i < nq; i += kWordsThreads) s_val[i] = v.q_val[i], s_id[i] = v.q_id[i];
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int slot = blockIdx.x * (kWordsThreads / 64) + wave_in_block();
  if (slot >= v.n_slots) return;  // whole wavefronts, after the only barrier
  int cnt = 0, first = -1;
  double sum = 0.0;
  if (v.in_file[slot]) {
    const int n = v.kf_n[slot];
    const uint32_t* ids = v.bow_id + (size_t)slot * v.max_words;
    const double* vals = v.bow_val + (size_t)slot * v.max_words;
    for (int base = 0; base < n; base += 64) {
      const int j = base + lane;
      int qi = -1;
      double term = 0.0;
      if (j < n) {
        qi = find_word(s_id, nq, ids[j]);
        if (qi >= 0) term = l1_term(s_val[qi], vals[j]);
      }
      unsigned long long m = __ballot(qi >= 0);
      if (m) {
        if (first < 0) first = __shfl(qi, __ffsll((long long)m) - 1, 64);
        cnt += __popcll(m);
        while (m) {  // wave-uniform: the same chain in every lane, in ascending word order
          sum += __shfl(term, __ffsll((long long)m) - 1, 64);
          m &= m - 1;
        }
      }
    }
  }
  if (lane == 0) v.cnt[slot] = cnt, v.first[slot] = first, v.score[slot] = l1_finish(sum);
}

struct EpiHdr {
  int maxc, nlisted;
};

__global__ __launch_bounds__(kEpiThreads) void k_kfdb_bow_epilogue(KfdbView v, int mode, int64_t id, float min_score, int npad, int lds_sort) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  EpiHdr* hdr = reinterpret_cast<EpiHdr*>(smem);
  float* red = reinterpret_cast<float*>(smem + kEpiHdr);
  int* scan = reinterpret_cast<int*>(smem + kEpiHdr);
  uint64_t* keys = lds_sort ? reinterpret_cast<uint64_t*>(smem + kEpiHdr + kEpiThreads * 4) : v.keys;
  const int tid = threadIdx.x, n = v.n_slots;
  if (tid == 0) hdr->maxc = 0, hdr->nlisted = 0;
  __syncthreads();
  // the walk over the inverted file, per slot
  {
    int lmax = 0, lcount = 0;
    for (int s = tid; s < npad; s += kEpiThreads) {
      uint64_t key = kNoKey;
      if (s < n) {
        const int c = v.cnt[s];
        if (c > 0) {
          const bool loop = mode == kLoop;
          int64_t q = loop ? v.state[s].loop_query : v.state[s].reloc_query;
          int32_t w = loop ? v.state[s].loop_words : v.state[s].reloc_words;
          const bool listed = touch(mode, id, c, loop && v.connected[s], q, w);
          if (loop) v.state[s].loop_query = q, v.state[s].loop_words = w;
          else v.state[s].reloc_query = q, v.state[s].reloc_words = w;
          if (listed) {
            key = list_key(v.first[s], v.seq[s]);
            lmax = w > lmax ? w : lmax;
            ++lcount;
          }
        }
        __hip_atomic_store(&v.first_r[s], 0x7fffffff, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      keys[s] = key;
    }
    if (lcount) atomicMax(&hdr->maxc, lmax), atomicAdd(&hdr->nlisted, lcount);
  }
  __syncthreads();
  const int nlisted = hdr->nlisted, maxc = hdr->maxc;
  const int minc = min_common_words(maxc);
  if (tid == 0) v.out[0] = nlisted, v.out[1] = 0, v.out[2] = maxc, v.out[3] = minc;
  if (nlisted == 0) return;  // uniform
  // the scoring loop: a listed slot with enough words keeps its score (each thread revisits the slots it walked)
  for (int s = tid; s < n; s += kEpiThreads) {
    if (keys[s] == kNoKey) continue;
    if (mode == kLoop) {
      if (v.state[s].loop_words > minc) v.state[s].loop_score = v.score[s];
    } else {
      if (v.state[s].reloc_words > minc) v.state[s].reloc_score = v.score[s];
    }
  }
  __syncthreads();
  // list order
  for (int k = 2; k <= npad; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < npad; i += kEpiThreads) {
        const int x = i ^ j;
        if (x > i) {
          const uint64_t a = keys[i], b = keys[x];
          if ((a > b) == ((i & k) == 0)) keys[i] = b, keys[x] = a;
        }
      }
      __syncthreads();
    }
  // accumulation per list entry, the best accumulated score
  const float init = mode == kLoop ? min_score : 0.0f;
  float lbest = init;
  for (int r = tid; r < nlisted; r += kEpiThreads) {
    const int s = v.slot_of_seq[(uint32_t)keys[r]];
    const int32_t w = mode == kLoop ? v.state[s].loop_words : v.state[s].reloc_words;
    const float si = mode == kLoop ? v.state[s].loop_score : v.state[s].reloc_score;
    int flags = UVO_KFDB_LISTED;
    float acc = 0.0f;
    int best = -1;
    if (w > minc) {
      flags |= UVO_KFDB_SCORED;
      if (mode != kLoop || si >= min_score) {
        flags |= UVO_KFDB_ENTERED;
        accumulate(mode, id, minc, si, s, v.cov + (size_t)s * kCovisibles, v.state, acc, best);
        if (acc > lbest) lbest = acc;
      }
    }
    uvo_kfdb_query_row row;
    row.slot = s, row.words = w, row.flags = flags, row.best = best, row.score = si, row.acc = acc;
    v.rows[r] = row;
  }
  red[tid] = lbest;
  __syncthreads();
  for (int off = kEpiThreads / 2; off > 0; off >>= 1) {
    if (tid < off) {
      const float a = red[tid], b = red[tid + off];
      red[tid] = b > a ? b : a;
    }
    __syncthreads();
  }
  const float min_retain = 0.75f * red[0];
  __syncthreads();  // red becomes scan below
  // retention; the first retained entry that elects a keyframe owns it
  for (int r = tid; r < nlisted; r += kEpiThreads) {
    const int flags = v.rows[r].flags;
    if ((flags & UVO_KFDB_ENTERED) && v.rows[r].acc > min_retain) {
      v.rows[r].flags = flags | UVO_KFDB_RETAINED;
      atomicMin(&v.first_r[v.rows[r].best], r);
    }
  }
  __syncthreads();
  // the candidates in list order: each thread a contiguous run of entries, an exclusive scan of the runs' counts
  const int chunk = (nlisted + kEpiThreads - 1) / kEpiThreads;
  const int r0 = tid * chunk < nlisted ? tid * chunk : nlisted, r1 = r0 + chunk < nlisted ? r0 + chunk : nlisted;
  int mine = 0;
  for (int r = r0; r < r1; ++r)
    if ((v.rows[r].flags & UVO_KFDB_RETAINED) && __hip_atomic_load(&v.first_r[v.rows[r].best], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == r) ++mine;
  scan[tid] = mine;
  __syncthreads();
  for (int off = 1; off < kEpiThreads; off <<= 1) {
    const int add = tid >= off ? scan[tid - off] : 0;
    __syncthreads();
    scan[tid] += add;
    __syncthreads();
  }
  int at = scan[tid] - mine;
  for (int r = r0; r < r1; ++r)
    if ((v.rows[r].flags & UVO_KFDB_RETAINED) && __hip_atomic_load(&v.first_r[v.rows[r].best], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == r)
      v.out[kKfdbMeta + at++] = v.rows[r].best;
  if (tid == kEpiThreads - 1) v.out[1] = scan[tid];
}

__global__ __launch_bounds__(256) void k_kfdb_haloc_dist(KfdbView v, int q_has, float max_score, int npad) {
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s >= npad) return;
  uint64_t key = kNoKey;
  if (s < v.n_slots) {
    float m = 0.0f;
    if (!v.skip[s]) {
      m = hash_match(v.q_hash, q_has != 0, v.hash_t + s, v.max_kf, v.has_hash[s] != 0, v.hash_len);
      if (haloc_keep(m, max_score)) key = haloc_key(m, v.seq[s]);
    }
    v.hm[s] = m;
  }
  v.keys[s] = key;
}

__global__ __launch_bounds__(kEpiThreads) void k_kfdb_haloc_top3(KfdbView v, int npad) {
  __shared__ unsigned long long s_min[3];
  __shared__ int s_kept;
  const int tid = threadIdx.x;
  if (tid == 0) s_min[0] = s_min[1] = s_min[2] = kNoKey, s_kept = 0;
  __syncthreads();
  int kept = 0;
  for (int s = tid; s < npad; s += kEpiThreads) kept += v.keys[s] != kNoKey;
  if (kept) atomicAdd(&s_kept, kept);
  unsigned long long floor_key = 0;  // round r takes the smallest key above round r-1's (keys are unique)
  for (int r = 0; r < 3; ++r) {
    unsigned long long lmin = kNoKey;
    for (int s = tid; s < npad; s += kEpiThreads) {
      const unsigned long long k = v.keys[s];
      if ((r == 0 || k > floor_key) && k < lmin) lmin = k;
    }
    if (lmin != kNoKey) atomicMin(&s_min[r], lmin);
    __syncthreads();
    floor_key = s_min[r];
  }
  if (tid == 0) {
    const int nk = s_kept;
    v.out[4] = nk;
    v.out[1] = nk >= 3 ? 3 : 0;  // :125-132: the best three only when at least three were kept
    for (int r = 0; r < 3; ++r) v.out[kKfdbMeta + r] = (nk >= 3) ? v.slot_of_seq[(uint32_t)s_min[r]] : -1;
  }
}

static int pad_pow2(int n) {
  int p = 2;
  while (p < n) p <<= 1;
  return p;
}

void launch_kfdb_bow(hipStream_t s, const KfdbView& v, int mode, int64_t id, int nq, float min_score) {
  const int per = kWordsThreads / 64;
  hipLaunchKernelGGL(k_kfdb_words, dim3((v.n_slots + per - 1) / per), dim3(kWordsThreads), (size_t)nq * 12 + 16, s, v, nq);
  const int npad = pad_pow2(v.n_slots);
  const int lds_sort = npad <= kKfdbLdsSort;
  hipLaunchKernelGGL(k_kfdb_bow_epilogue, dim3(1), dim3(kEpiThreads), (size_t)kEpiHdr + kEpiThreads * 4 + (lds_sort ? (size_t)npad * 8 : 0), s, v, mode, id,
                     min_score, npad, lds_sort);
}

void launch_kfdb_haloc(hipStream_t s, const KfdbView& v, int q_has, float max_score) {
  const int npad = pad_pow2(v.n_slots);
  hipLaunchKernelGGL(k_kfdb_haloc_dist, dim3((npad + 255) / 256), dim3(256), 0, s, v, q_has, max_score, npad);
  hipLaunchKernelGGL(k_kfdb_haloc_top3, dim3(1), dim3(kEpiThreads), 0, s, v, npad);
}

}  // namespace uvo
