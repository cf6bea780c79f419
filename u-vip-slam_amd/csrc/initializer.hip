// USLAM::Initializer for Tracking::Initialize (src/Tracking.cc:1340, :1582; src/Initializer.cc): Initialize as one call -- the F path,
// which is all the reference executes (initializer_core.hpp's header).  All arithmetic is initializer_core.hpp, shared with the host
// build tests/emu/initializer_emu.cpp; this file decides which lane computes which scalar.  What makes it one call: every set is drawn
// before any is evaluated (:73-90) and no hypothesis ends the loop early, so the host draws the 8 x iterations indices from a copy of
// the caller's generator and uploads them with the current frame's keys and matches.  Normalize's serial float sums run on the host
// (four numbers per frame); the device normalises the points it reads.
//
// Five launches in the uvo_klt handle's stream between one upload and one download, all memory sized at uvo_initializer_create:
//   k_init_hypotheses : ComputeF21 and T2^T Fn T1, one lane per hypothesis.  The one-sided Jacobi picks its rows by pair and by sort
//                       position: the nine rows of nine floats and W of the 64 lanes of a workgroup lie interleaved in LDS (388 bytes
//                       a lane).  The u of the 8 x 9 decomposition is never read and not carried.
//   k_init_score      : CheckFundamental, one workgroup per hypothesis.  Lanes compute the two score terms of a match (+0 where the
//                       reference adds nothing, which leaves every partial sum's bits alone) into LDS, 2048 matches at a time; one
//                       lane adds them to the float score in match order; the inlier set leaves as 64-bit ballot words.
//   k_init_select     : the first hypothesis of the largest score (> 0), its inlier count and mask, DecomposeE.
//   k_init_check_rt   : one lane per (motion, match): Triangulate and the gates of CheckRT for the inliers of the best hypothesis.
//   k_init_finish     : wavefront k counts nGood_k and selects the parallax order statistic of motion k bit by bit (exact: a value,
//                       not a sum); then the verdict of ReconstructF and the result record, vP3D and vbTriangulated.
#include <cmath>
#include <cstring>
#include <utility>
#include <vector>

#include "devmem.hpp"
#include "initializer.hpp"
#include "pnpsolver.hpp"

namespace uvo {

// the device block of an object, by value to every kernel
struct InitDev {
  int32_t max_keys, max_words;
  const float* keys1;     // [max_keys][2]
  const uint8_t* up;      // InitCall, keys2, matches12, sets
  float* F;               // [T][9]
  float* scores;          // [T]
  uint64_t* masks;        // [T][max_words]
  InitSel* sel;
  uint8_t* flags;         // [4][max_keys]  twoview::kCounted | kGood
  float* cosp;            // [4][max_keys]
  float* p3d;             // [4][max_keys][3]
  uint8_t* down;          // InitOut, mask words, vP3D, vbTriangulated
};

__device__ __forceinline__ const InitCall& call_of(const InitDev& D) { return *reinterpret_cast<const InitCall*>(D.up); }
__device__ __forceinline__ const float* keys2_of(const InitDev& D) { return reinterpret_cast<const float*>(D.up + sizeof(InitCall)); }
__device__ __forceinline__ const int32_t* matches_of(const InitDev& D, int n2) { return reinterpret_cast<const int32_t*>(keys2_of(D) + 2 * (size_t)n2); }
__device__ __forceinline__ const int32_t* sets_of(const InitDev& D, int n2) { return matches_of(D, n2) + n2; }

__global__ __launch_bounds__(kInitHypLanes) void k_init_hypotheses(InitDev D) {
  __shared__ float s_f[twoview::kWsFloats * kInitHypLanes];
  __shared__ double s_d[twoview::kWsDoubles * kInitHypLanes];
  const InitCall& c = call_of(D);
  const int g = blockIdx.x * kInitHypLanes + threadIdx.x;
  if (g >= c.T) return;
  const float* keys2 = keys2_of(D);
  const int32_t* m12 = matches_of(D, c.n2);
  const int32_t* set = sets_of(D, c.n2) + (size_t)g * twoview::kSet;
  const twoview::Ws<kInitHypLanes> W{s_f + threadIdx.x, s_d + threadIdx.x};
  for (int j = 0; j < twoview::kSet; ++j) {
    const int idx = set[j], i1 = m12[idx];
    float u1, v1, u2, v2;
    twoview::normalized(c.N1, D.keys1[2 * i1], D.keys1[2 * i1 + 1], &u1, &v1);
    twoview::normalized(c.N2, keys2[2 * idx], keys2[2 * idx + 1], &u2, &v2);
    twoview::set_row(W, j, u1, v1, u2, v2);
  }
  float F[9];
  twoview::f21_from_rows(W, c.N1, c.N2, F);
#pragma unroll
  for (int e = 0; e < 9; ++e) D.F[(size_t)g * 9 + e] = F[e];
}

__global__ __launch_bounds__(256) void k_init_score(InitDev D) {
  __shared__ float s_t[2 * kInitChunk];
  __shared__ float s_F[9];
  const InitCall& c = call_of(D);
  const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  if (tid < 9) s_F[tid] = D.F[(size_t)g * 9 + tid];
  __syncthreads();
  float F[9];
#pragma unroll
  for (int e = 0; e < 9; ++e) F[e] = s_F[e];
  const float* keys2 = keys2_of(D);
  const int32_t* m12 = matches_of(D, c.n2);
  uint64_t* words = D.masks + (size_t)g * D.max_words;
  float score = 0.f;
  for (int base = 0; base < c.n2; base += kInitChunk) {
    for (int r = 0; r < kInitChunk / 256; ++r) {
      const int i = base + r * 256 + tid;  // the 64 lanes of a wavefront hold one mask word
      bool inl = false;
      if (i < c.n2) {
        const int i1 = m12[i];
        float t1, t2;
        inl = twoview::score_terms(F, D.keys1[2 * i1], D.keys1[2 * i1 + 1], keys2[2 * i], keys2[2 * i + 1], c.inv_sigma2, &t1, &t2);
        s_t[2 * (i - base)] = t1, s_t[2 * (i - base) + 1] = t2;
      }
      const uint64_t m = __ballot(inl);
      if (lane == 0 && i < c.n2) words[i >> 6] = m;
    }
    __syncthreads();
    if (tid == 0) {  // one float accumulator, added to in match order, as :433 and :451 do
      const int cnt = 2 * (c.n2 - base < kInitChunk ? c.n2 - base : kInitChunk);
      for (int e = 0; e < cnt; e += 2) {
        const float a = s_t[e], b = s_t[e + 1];
        score += a;
        score += b;
      }
    }
    __syncthreads();
  }
  if (tid == 0) D.scores[g] = score;
}

__global__ __launch_bounds__(256) void k_init_select(InitDev D) {
  __shared__ float s_s[256];
  __shared__ int32_t s_i[256];
  __shared__ int32_t s_cnt;
  __shared__ float s_f[twoview::kWsFloats];
  __shared__ double s_d[twoview::kWsDoubles];
  const InitCall& c = call_of(D);
  const int tid = threadIdx.x;
  float bs = 0.f;  // score = 0.0 at :180; a new best needs currentScore > score
  int bi = -1;
  for (int g = tid; g < c.T; g += 256) {
    const float s = D.scores[g];
    if (s > bs) bs = s, bi = g;
  }
  s_s[tid] = bs, s_i[tid] = bi;
  if (tid == 0) s_cnt = 0;
  __syncthreads();
  for (int step = 128; step > 0; step >>= 1) {  // a maximum, not a sum: exact in any order; equal scores keep the lower index
    if (tid < step) {
      const float os = s_s[tid + step];
      const int oi = s_i[tid + step];
      if (oi >= 0 && (os > s_s[tid] || (os == s_s[tid] && oi < s_i[tid]) || s_i[tid] < 0)) s_s[tid] = os, s_i[tid] = oi;
    }
    __syncthreads();
  }
  const int best = s_i[0];
  uint64_t* out_words = reinterpret_cast<uint64_t*>(D.down + sizeof(InitOut));
  int cnt = 0;
  for (int w = tid; w < c.words; w += 256) {
    const uint64_t m = best >= 0 ? D.masks[(size_t)best * D.max_words + w] : 0;
    out_words[w] = m;
    cnt += __builtin_popcountll(m);
  }
  if (cnt) atomicAdd(&s_cnt, cnt);
  __syncthreads();
  if (tid == 0) {
    InitSel* S = D.sel;
    S->best = best, S->n_inliers = s_cnt, S->score = best >= 0 ? s_s[0] : 0.f;
    float F[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) F[e] = best >= 0 ? D.F[(size_t)best * 9 + e] : 0.f, S->F[e] = F[e];
    if (best >= 0) {
      const twoview::Ws<1> W{s_f, s_d};
      twoview::Motion M;
      twoview::decompose_e(W, F, c.K, M);
      S->M = M;
    }
  }
}

__global__ __launch_bounds__(kInitHypLanes) void k_init_check_rt(InitDev D) {
  __shared__ float s_f[twoview::kWsFloats * kInitHypLanes];
  __shared__ double s_d[twoview::kWsDoubles * kInitHypLanes];
  const InitCall& c = call_of(D);
  const InitSel& S = *D.sel;
  if (S.best < 0) return;
  const int i = blockIdx.x * kInitHypLanes + threadIdx.x, k = blockIdx.y;
  if (i >= c.n2) return;
  const size_t o = (size_t)k * D.max_keys + i;
  float X[3] = {0.f, 0.f, 0.f}, cosp = 0.f;
  int flags = 0;
  if (D.masks[(size_t)S.best * D.max_words + (i >> 6)] >> (i & 63) & 1) {
    const float* keys2 = keys2_of(D);
    const int i1 = matches_of(D, c.n2)[i];
    float R[9], t[3];
    twoview::motion_of(S.M, k, R, t);
    const twoview::Ws<kInitHypLanes> W{s_f + threadIdx.x, s_d + threadIdx.x};
    flags = twoview::check_rt_one(W, R, t, c.K, D.keys1[2 * i1], D.keys1[2 * i1 + 1], keys2[2 * i], keys2[2 * i + 1], c.th2, X, &cosp);
  }
  D.flags[o] = (uint8_t)flags, D.cosp[o] = cosp;
  D.p3d[3 * o] = X[0], D.p3d[3 * o + 1] = X[1], D.p3d[3 * o + 2] = X[2];
}

__global__ __launch_bounds__(256) void k_init_finish(InitDev D) {
  __shared__ int32_t s_good[4];
  __shared__ float s_par[4];
  const InitCall& c = call_of(D);
  const InitSel& S = *D.sel;
  const int tid = threadIdx.x, lane = tid & 63, k = wave_in_block();
  InitOut* out = reinterpret_cast<InitOut*>(D.down);
  float* out_p3d = reinterpret_cast<float*>(D.down + sizeof(InitOut) + (size_t)c.words * 8);
  uint8_t* out_tri = reinterpret_cast<uint8_t*>(out_p3d + 3 * (size_t)c.n2);
  twoview::Verdict v = {0, -1};
  if (S.best >= 0) {  // uniform over the workgroup
    const uint8_t* fl = D.flags + (size_t)k * D.max_keys;
    const float* cs = D.cosp + (size_t)k * D.max_keys;
    int cnt = 0;
    for (int base = 0; base < c.n2; base += 64) {
      const int i = base + lane;
      cnt += __builtin_popcountll(__ballot(i < c.n2 && (fl[i] & twoview::kCounted)));
    }
    float par = 0.f;
    if (cnt > 0) {
      const int idx = 50 < cnt - 1 ? 50 : cnt - 1;  // :897
      uint32_t key = 0;                             // the largest key with at most idx counted values below it
      for (int bit = 31; bit >= 0; --bit) {
        const uint32_t cand = key | (1u << bit);
        int below = 0;
        for (int base = 0; base < c.n2; base += 64) {
          const int i = base + lane;
          below += __builtin_popcountll(__ballot(i < c.n2 && (fl[i] & twoview::kCounted) && twoview::ordered_key(cs[i]) < cand));
        }
        if (below <= idx) key = cand;
      }
      par = twoview::parallax_deg(twoview::from_ordered_key(key));
    }
    if (lane == 0) s_good[k] = cnt, s_par[k] = par;
    __syncthreads();
    v = twoview::verdict_of(S.n_inliers, s_good, s_par);
  }
  const int d = v.deciding < 0 ? 0 : v.deciding;
  for (int i = tid; i < c.n2; i += 256) {
    const size_t o = (size_t)d * D.max_keys + i;
    const int f = v.ok ? D.flags[o] : 0;
    out_tri[i] = (f & twoview::kGood) ? 1 : 0;
    out_p3d[3 * i] = (f & twoview::kCounted) ? D.p3d[3 * o] : 0.f;
    out_p3d[3 * i + 1] = (f & twoview::kCounted) ? D.p3d[3 * o + 1] : 0.f;
    out_p3d[3 * i + 2] = (f & twoview::kCounted) ? D.p3d[3 * o + 2] : 0.f;
  }
  if (tid == 0) {
    out->ok = v.ok, out->best = S.best, out->n_inliers = S.n_inliers, out->deciding = v.deciding, out->score = S.score;
    float R[9], t[3];
    twoview::motion_of(S.M, d, R, t);
    for (int e = 0; e < 4; ++e) out->n_good[e] = S.best >= 0 ? s_good[e] : 0, out->parallax[e] = S.best >= 0 ? s_par[e] : 0.f;
    for (int e = 0; e < 9; ++e) out->R[e] = v.ok ? R[e] : 0.f, out->F[e] = S.F[e];
    for (int e = 0; e < 3; ++e) out->t[e] = v.ok ? t[e] : 0.f;
  }
}

}  // namespace uvo

// ---------------------------------------------------------------------------------------------------------------------------
using namespace uvo;

struct uvo_initializer {
  uvo_klt* klt = nullptr;
  hipStream_t stream = nullptr;
  int device = 0, max_keys = 0, max_words = 0;
  DevMem mem;  // owns D's block and the two mirrors
  InitDev D;
  float* keys1 = nullptr;  // writable view of D's
  // page-locked mirrors of the two exchanges, and the arrays of the last initialize call in them (exchanges)
  uint8_t *h_up = nullptr, *h_down = nullptr, *tri = nullptr;
  InitCall* call = nullptr;
  float *keys2 = nullptr, *p3d = nullptr;
  int32_t *m12 = nullptr, *sets = nullptr;
  InitOut* out = nullptr;
  uint64_t* mask = nullptr;
  bool ready = false;      // set_reference has run
  int n1 = 0, iterations = 0, tap_n = 0;
  float sigma = 1.f;
  twoview::Norm N1;
  twoview::Cam K;
  std::vector<int32_t> avail;  // draw_set's slots
};

// The two exchanges of an initialize call of n2 keys and T sets, each one copy (the kernels find their side with call_of .. sets_of, and in
// k_init_finish): places the call's arrays in the mirrors -- before there are any, at create, it only measures; -> bytes up, bytes down
static std::pair<size_t, size_t> exchanges(uvo_initializer* s, size_t n2, size_t T) {
  Carve u{s->h_up}, d{s->h_down};
  u.take(s->call, 1).take(s->keys2, n2 * 2, alignof(float)).take(s->m12, n2, alignof(int32_t)).take(s->sets, T * twoview::kSet, alignof(int32_t));
  d.take(s->out, 1).take(s->mask, (n2 + 63) / 64, alignof(uint64_t)).take(s->p3d, n2 * 3, alignof(float)).take(s->tri, n2, 1);
  return {u.off, d.off};
}

extern "C" {

void uvo_initializer_destroy(uvo_initializer* s) {
  if (!s) return;
  hipSetDevice(s->device);
  if (s->stream) hipStreamSynchronize(s->stream);
  s->mem.release_all();
  delete s;
}

int uvo_initializer_create(uvo_klt* k, int max_keys, uvo_initializer** out) {
  if (!k || !out) return fail(UVO_E_BADARG, "null pointer");
  *out = nullptr;
  if (max_keys < twoview::kSet || max_keys > kInitMaxKeys) return fail(UVO_E_BADARG, "Initializer: 8..16384 keys per frame");
  uvo_initializer* s = new uvo_initializer();
  s->klt = k, s->stream = klt_stream(k), s->device = klt_device(k);
  s->max_keys = max_keys, s->max_words = (max_keys + 63) / 64;
  const size_t N = (size_t)max_keys, W = (size_t)s->max_words, T = (size_t)kInitMaxIterations;
  const auto [up_bytes, down_bytes] = exchanges(s, N, T);
  InitDev& D = s->D;
  D.max_keys = max_keys, D.max_words = s->max_words;
  int rc = hipSetDevice(s->device) == hipSuccess ? UVO_OK : fail(UVO_E_NOMEM, "Initializer allocation failed");
  if (!rc) rc = alloc_carved(s->mem, [&, up = up_bytes, down = down_bytes](Carve& c) {
    c.take(s->keys1, N * 2).take(D.up, up).take(D.F, T * 9).take(D.scores, T).take(D.masks, T * W).take(D.sel, 1);
    c.take(D.flags, 4 * N).take(D.cosp, 4 * N).take(D.p3d, 4 * N * 3).take(D.down, down);
  });
  if (!rc) rc = s->mem.alloc(&s->h_up, up_bytes, true);
  if (!rc) rc = s->mem.alloc(&s->h_down, down_bytes, true);
  if (rc) return uvo_initializer_destroy(s), rc;
  D.keys1 = s->keys1;
  s->avail.resize(N);
  *out = s;
  return UVO_OK;
}

int uvo_initializer_set_reference(uvo_initializer* s, const float* keys1_xy, int n1, const uvo_camera_model* cam, float sigma, int iterations) {
  if (!s || !keys1_xy || !cam) return fail(UVO_E_BADARG, "null pointer");
  if (n1 < 1 || n1 > s->max_keys) return fail(UVO_E_BADARG, "Initializer: reference key count outside 1..max_keys");
  if (iterations < 1 || iterations > kInitMaxIterations) return fail(UVO_E_BADARG, "Initializer: iterations outside 1..1024");
  if (!(sigma > 0.f) || !(sigma <= 1e6f)) return fail(UVO_E_BADARG, "Initializer: sigma outside (0, 1e6]");
  if (!(cam->fx == cam->fx && cam->fy == cam->fy && cam->cx == cam->cx && cam->cy == cam->cy)) return fail(UVO_E_BADARG, "NaN in the camera matrix");
  s->ready = false, s->tap_n = 0;
  UVO_HIP_CHECK(hipSetDevice(s->device));
  UVO_HIP_CHECK(hipMemcpyAsync(s->keys1, keys1_xy, (size_t)n1 * 8, hipMemcpyHostToDevice, s->stream));
  UVO_HIP_CHECK(hipStreamSynchronize(s->stream));  // the source is the caller's pageable memory
  s->N1 = twoview::normalize(keys1_xy, n1);
  s->K = twoview::Cam{cam->fx, cam->fy, cam->cx, cam->cy};
  s->n1 = n1, s->sigma = sigma, s->iterations = iterations, s->ready = true;
  return UVO_OK;
}

int uvo_initializer_initialize(uvo_initializer* s, const float* keys2_xy, int n2, const int32_t* matches12, uvo_glibc_rand* rng, uvo_initializer_result* result) {
  if (!s || !rng || !result || (n2 > 0 && (!keys2_xy || !matches12))) return fail(UVO_E_BADARG, "null pointer");
  if (!s->ready) return fail(UVO_E_BADARG, "Initializer: set_reference has not been called");
  if (n2 < 0 || n2 > s->max_keys) return fail(UVO_E_BADARG, "Initializer: current key count outside 0..max_keys");
  for (int i = 0; i < n2; ++i)
    if (matches12[i] < 0 || matches12[i] >= s->n1) return fail(UVO_E_BADARG, "Initializer: matches12 outside 0..n1-1");
  uint8_t *inl = result->inliers, *tri = result->triangulated;
  float* p3d = result->p3d;
  std::memset(result, 0, sizeof *result);
  result->inliers = inl, result->p3d = p3d, result->triangulated = tri;
  result->best = -1, result->deciding = -1;
  s->tap_n = 0;
  if (n2 < twoview::kSet) {  // departure (1): nothing drawn
    if (inl) std::memset(inl, 0, (size_t)n2);
    if (tri) std::memset(tri, 0, (size_t)n2);
    if (p3d) std::memset(p3d, 0, (size_t)n2 * 12);
    return UVO_OK;
  }
  const int T = s->iterations, words = (n2 + 63) / 64;
  const auto [up_bytes, down_bytes] = exchanges(s, (size_t)n2, (size_t)T);
  InitCall* call = s->call;
  std::memset(call, 0, sizeof *call);
  call->n1 = s->n1, call->n2 = n2, call->T = T, call->words = words;
  call->N1 = s->N1, call->N2 = twoview::normalize(keys2_xy, n2), call->K = s->K;
  call->inv_sigma2 = twoview::inv_sigma_square(s->sigma), call->th2 = twoview::th2_of(s->sigma);
  std::memcpy(s->keys2, keys2_xy, (size_t)n2 * 8);
  std::memcpy(s->m12, matches12, (size_t)n2 * 4);
  pnps::GlibcRand g;
  std::memcpy(&g, rng, sizeof g);
  for (int it = 0; it < T; ++it) twoview::draw_set(g, n2, s->avail.data(), s->sets + (size_t)it * twoview::kSet);
  UVO_HIP_CHECK(hipSetDevice(s->device));
  hipStream_t st = s->stream;
  UVO_HIP_CHECK(hipMemcpyAsync(const_cast<uint8_t*>(s->D.up), s->h_up, up_bytes, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_init_hypotheses, dim3((T + kInitHypLanes - 1) / kInitHypLanes), dim3(kInitHypLanes), 0, st, s->D);
  hipLaunchKernelGGL(k_init_score, dim3(T), dim3(256), 0, st, s->D);
  hipLaunchKernelGGL(k_init_select, dim3(1), dim3(256), 0, st, s->D);
  hipLaunchKernelGGL(k_init_check_rt, dim3((n2 + kInitHypLanes - 1) / kInitHypLanes, 4), dim3(kInitHypLanes), 0, st, s->D);
  hipLaunchKernelGGL(k_init_finish, dim3(1), dim3(256), 0, st, s->D);
  UVO_HIP_CHECK(hipGetLastError());
  UVO_HIP_CHECK(hipMemcpyAsync(s->h_down, s->D.down, down_bytes, hipMemcpyDeviceToHost, st));
  UVO_HIP_CHECK(hipStreamSynchronize(st));
  s->tap_n = T;
  const InitOut& o = *s->out;
  result->initialized = o.ok, result->best = o.best, result->n_inliers = o.n_inliers, result->deciding = o.deciding, result->score = o.score;
  std::memcpy(result->n_good, o.n_good, 16);
  std::memcpy(result->parallax, o.parallax, 16);
  std::memcpy(result->R21, o.R, 36);
  std::memcpy(result->t21, o.t, 12);
  std::memcpy(result->F21, o.F, 36);
  if (inl)
    for (int i = 0; i < n2; ++i) inl[i] = (uint8_t)(s->mask[i >> 6] >> (i & 63) & 1);
  if (p3d) std::memcpy(p3d, s->p3d, (size_t)n2 * 12);
  if (tri) std::memcpy(tri, s->tri, (size_t)n2);
  result->draws = (uint32_t)(T * twoview::kSet);
  std::memcpy(rng, &g, sizeof g);  // the caller's state stands where rand() would after the 8 * iterations draws
  return UVO_OK;
}

int uvo_initializer_hypotheses(uvo_initializer* s, int32_t* subsets, float* F, float* scores, int cap, int* n) {
  if (!s || !n) return fail(UVO_E_BADARG, "null pointer");
  if (cap < 0) return fail(UVO_E_BADARG, "negative capacity");
  const int m = cap < s->tap_n ? cap : s->tap_n;
  if (m > 0 && (!subsets || !F || !scores)) return fail(UVO_E_BADARG, "null pointer");
  *n = m;
  if (m == 0) return UVO_OK;
  std::memcpy(subsets, s->sets, (size_t)m * twoview::kSet * 4);  // drawn on the host in the last call
  UVO_HIP_CHECK(hipSetDevice(s->device));
  UVO_HIP_CHECK(hipMemcpy(F, s->D.F, (size_t)m * 36, hipMemcpyDeviceToHost));
  UVO_HIP_CHECK(hipMemcpy(scores, s->D.scores, (size_t)m * 4, hipMemcpyDeviceToHost));
  return UVO_OK;
}

}  // extern "C"
