// The RANSAC solver sets (pnpsolver.hip, sim3solver.hip): the one host side behind both C ABIs.  A set holds a list of solvers and runs
// iterate(n) over some of them as one call: every subset is drawn on the host from a copy of the caller's generator, one upload, the
// family's three launches, one download, and the caller's generator moves by the draws of the iterations actually performed.  Host only.
//
// A family is its handle: a struct Set derived from SolverSet<Call, Result> with `solvers`, a vector of structs derived from SetSolver,
// its limits and texts, arrays(carve, scratch) for what it keeps on the device, and what differs between the two iterate calls:
//   plan(v, n_iterations)              the iterations the call runs on solver v unless it returns; 0: v never iterates
//   call(id, v, off, K, n_iterations)  the call record; min_set(v) is the length of the subsets drawn for it
//   launch(n_ids, total)               the three launches in `stream`
//   idle_no_more(v)                    bNoMore of a solver the call planned nothing for
//   adopt(v, r, result)                result record r into the family's own state and the family's fields of the C result; false: v did not return
#pragma once
#include <algorithm>
#include <cstring>
#include <type_traits>
#include <vector>

#include "devmem.hpp"
#include "glibc_rand.hpp"

namespace uvo {

struct SetSolver {
  int n = 0, n_matches = 0;
  int32_t iterations = 0, best_count = 0;  // mnIterations, mnBestInliers
  std::vector<int32_t> index;              // mvKeyPointIndices / mvnIndices1: where point i stands in the caller's mask
  int tap_off = 0, tap_n = 0;              // the hypotheses it consumed in the last iterate call
};

template <class Call, class Result>
struct SolverSet {
  int device = 0;
  hipStream_t stream = nullptr;
  int max_solvers = 0, max_points = 0, words = 0, total = 0;  // words: of a mask; total: hypothesis slots
  DevMem mem;  // owns the device block and the page-locked mirrors of its two exchanges
  // each exchange is one copy: its two arrays are adjacent, on the device (d_) and in the mirror (h_)
  Call *d_call = nullptr, *h_call = nullptr;  // the upload: call records, then subset records
  int32_t *d_sub = nullptr, *h_sub = nullptr;
  Result *d_res = nullptr, *h_res = nullptr;  // the download: result records, then the returned sets
  uint64_t *d_om = nullptr, *h_om = nullptr;
  std::vector<int32_t> avail;  // draw_subset's slots
  std::vector<char> seen;      // per solver: listed in the current call
};

template <class Set>
void set_destroy(Set* s) {
  if (!s) return;
  hipSetDevice(s->device);
  if (s->stream) hipStreamSynchronize(s->stream);
  s->mem.release_all();
  delete s;
}

// the device block: the family's point arrays (arrays(c, false)), the upload, its scratch (arrays(c, true)), the download
template <class Set>
int set_create(int device, hipStream_t stream, int max_solvers, int max_points, Set** out) {
  if (max_solvers < 1 || max_solvers > Set::kMaxSolvers || max_points < Set::kMinPoints || max_points > Set::kMaxPoints) return fail(UVO_E_BADARG, Set::kRangeText);
  Set* s = new Set();
  s->device = device, s->stream = stream;
  s->max_solvers = max_solvers, s->max_points = max_points, s->words = (max_points + 63) / 64, s->total = max_solvers * Set::kHypPerSolver;
  const size_t S = (size_t)max_solvers, T = (size_t)s->total;
  auto upload = [&](Carve& c, auto*& call, int32_t*& sub) { c.take(call, S).take(sub, T * Set::kSubsetStride, alignof(int32_t)); };
  auto download = [&](Carve& c, auto*& res, uint64_t*& om) { c.take(res, S).take(om, S * (size_t)s->words, alignof(uint64_t)); };
  int rc = hipSetDevice(device) == hipSuccess ? UVO_OK : fail(UVO_E_NOMEM, Set::kNoMemText);
  if (!rc) rc = alloc_carved(s->mem, [&](Carve& c) {
    s->arrays(c, false);
    upload(c, s->d_call, s->d_sub);
    s->arrays(c, true);
    download(c, s->d_res, s->d_om);
  });
  if (!rc) rc = alloc_carved(s->mem, [&](Carve& c) { upload(c, s->h_call, s->h_sub); }, true);
  if (!rc) rc = alloc_carved(s->mem, [&](Carve& c) { download(c, s->h_res, s->h_om); }, true);
  if (rc) return set_destroy(s), rc;
  s->avail.resize((size_t)max_points);
  s->seen.resize(S);
  s->solvers.reserve(S);
  *out = s;
  return UVO_OK;
}

template <class Set>
int set_clear(Set* s) {
  if (!s) return fail(UVO_E_BADARG, "null handle");
  s->solvers.clear();
  return UVO_OK;
}

// add's checks in front of the family's own.  `handles`, `arrays`: the family's pointers are all there; the arrays may be NULL at n = 0
template <class Set>
int add_check(const Set* s, bool handles, int n, int n_matches, bool arrays) {
  if (!s || !handles) return fail(UVO_E_BADARG, "null pointer");
  if (n < 0 || n > s->max_points || n_matches < n) return fail(UVO_E_BADARG, "point count outside 0..max_points, or more points than matches");
  if (n > 0 && !arrays) return fail(UVO_E_BADARG, "null pointer");
  if ((int)s->solvers.size() >= s->max_solvers) return fail(UVO_E_BADARG, Set::kFullText);
  return UVO_OK;
}

// and its end: the solver's points are on the device, its id is its place in the list
template <class Set, class Solver>
int add_finish(Set* s, Solver& v, int* id) {
  *id = (int)s->solvers.size();
  s->solvers.push_back(std::move(v));
  return UVO_OK;
}

// the front of query and of whatever else addresses one solver
template <class Set>
int solver_check(const Set* s, bool pointers, int id) {
  if (!s || !pointers) return fail(UVO_E_BADARG, "null pointer");
  if (id < 0 || id >= (int)s->solvers.size()) return fail(UVO_E_BADARG, "no such solver");
  return UVO_OK;
}

template <class Set, class CResult>
int set_iterate(Set* s, const int32_t* ids, int n_ids, int n_iterations, uvo_glibc_rand* rng, CResult* result) {
  using Status = typename std::remove_pointer<decltype(result->status)>::type;
  if (!s || !rng || !result || (n_ids > 0 && !ids)) return fail(UVO_E_BADARG, "null pointer");
  if (n_ids < 0 || n_ids > s->max_solvers) return fail(UVO_E_BADARG, "more ids than the set has solvers");
  if (n_iterations < 1) return fail(UVO_E_BADARG, "n_iterations must be at least 1");
  Status* status = result->status;
  uint8_t* mask_out = result->inliers;
  const int mask_cap = result->inliers_cap;
  *result = CResult{};  // nothing returned: zeros in every field of either family but these
  result->returned = -1, result->solver = -1, result->status = status, result->inliers = mask_out, result->inliers_cap = mask_cap;
  std::vector<char>& seen = s->seen;
  std::fill(seen.begin(), seen.end(), 0);
  for (int j = 0; j < n_ids; ++j) {
    if (ids[j] < 0 || ids[j] >= (int)s->solvers.size()) return fail(UVO_E_BADARG, "no such solver");
    if (seen[ids[j]]) return fail(UVO_E_BADARG, "a solver is listed twice in one iterate call");
    seen[ids[j]] = 1;
    if (mask_out && mask_cap < s->solvers[ids[j]].n_matches) return fail(UVO_E_CAPACITY, "inliers_cap is smaller than a listed solver's n_matches");
  }
  for (auto& v : s->solvers) v.tap_off = v.tap_n = 0;
  if (status)
    for (int j = 0; j < n_ids; ++j) status[j] = Status{0, 0, s->solvers[ids[j]].iterations};
  // every subset of the call, from a copy of the caller's state: the stream position of a solver is the prefix sum of what the solvers
  // in front of it run, which is where the stream stands in the only case in which the solver is reached
  pnps::GlibcRand g;
  std::memcpy(&g, rng, sizeof g);
  auto* call = s->h_call;
  int total = 0;
  for (int j = 0; j < n_ids; ++j) {
    const auto& v = s->solvers[ids[j]];
    const int K = Set::plan(v, n_iterations);
    // the PnPsolver's OR rule can ask for this; the Sim3Solver's max_iterations is capped at its share of the slots when it is added
    if (total + K > s->total) return fail(UVO_E_BADARG, "the call needs more hypothesis slots than the set has (320 per solver)");
    call[j] = Set::call(ids[j], v, total, K, n_iterations);
    for (int h = 0; h < K; ++h) {
      int32_t* rec = s->h_sub + (size_t)(total + h) * Set::kSubsetStride;
      rec[0] = j;
      for (int e = 1; e < Set::kSubsetStride; ++e) rec[e] = 0;
      pnps::draw_subset(g, v.n, Set::min_set(v), s->avail.data(), rec + 1);
    }
    total += K;
  }
  const size_t W = (size_t)s->words;
  if (total > 0) {
    UVO_HIP_CHECK(hipSetDevice(s->device));
    UVO_HIP_CHECK(hipMemcpyAsync(s->d_call, call, (size_t)s->max_solvers * sizeof *call + (size_t)total * Set::kSubsetStride * 4, hipMemcpyHostToDevice, s->stream));
    s->launch(n_ids, total);
    UVO_HIP_CHECK(hipGetLastError());
    // result records of all solver slots, then the sets of the listed ones: adjacent on the device
    UVO_HIP_CHECK(hipMemcpyAsync(s->h_res, s->d_res, (size_t)s->max_solvers * sizeof *s->h_res + (size_t)n_ids * W * 8, hipMemcpyDeviceToHost, s->stream));
    UVO_HIP_CHECK(hipStreamSynchronize(s->stream));
  }
  int draws = 0;
  for (int j = 0; j < n_ids; ++j) {
    auto& v = s->solvers[ids[j]];
    if (call[j].hyp_n == 0) {  // no iteration, nothing drawn (n_iterations >= 1: every solver that can iterate has iterations to run)
      if (status) status[j] = Status{1, Set::idle_no_more(v), v.iterations};
      continue;
    }
    const auto& r = s->h_res[j];
    v.iterations += r.performed, v.best_count = r.best_count;
    v.tap_off = call[j].hyp_off, v.tap_n = r.performed;
    draws += r.performed * Set::min_set(v);
    if (status) status[j] = Status{1, r.no_more, v.iterations};
    if (!Set::adopt(v, r, result)) continue;
    result->returned = j, result->solver = ids[j], result->n_inliers = r.inliers;
    if (mask_out) {
      std::fill(mask_out, mask_out + v.n_matches, (uint8_t)0);
      const uint64_t* words = s->h_om + (size_t)j * W;
      for (int i = 0; i < v.n; ++i)
        if (words[i >> 6] >> (i & 63) & 1) mask_out[v.index[i]] = 1;
    }
    break;
  }
  result->draws = (uint32_t)draws;  // the caller's state moves to where rand() would stand after the iterations actually performed
  pnps::GlibcRand* gr = reinterpret_cast<pnps::GlibcRand*>(rng);
  for (int d = 0; d < draws; ++d) (void)gr->next();
  return UVO_OK;
}

// The test tap's front: m = min(cap, the hypotheses solver id consumed in the last iterate call) to *n, and their subsets out of the
// host mirror, where they were drawn.  `others`: the family's own output arrays are all there.  The caller copies the rest if *n > 0.
template <class Set>
int tap_subsets(const Set* s, int id, int32_t* subsets, bool others, int cap, int* n) {
  RC(solver_check(s, n != nullptr, id));
  if (cap < 0) return fail(UVO_E_BADARG, "negative capacity");
  const auto& v = s->solvers[id];
  const int m = cap < v.tap_n ? cap : v.tap_n, k = Set::min_set(v);
  if (m > 0 && (!subsets || !others)) return fail(UVO_E_BADARG, "null pointer");
  *n = m;
  for (int h = 0; h < m; ++h)
    for (int e = 0; e < k; ++e) subsets[h * k + e] = s->h_sub[(size_t)(v.tap_off + h) * Set::kSubsetStride + 1 + e];
  return UVO_OK;
}

}  // namespace uvo
