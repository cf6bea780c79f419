// csrc/carve.hpp walked on the host: a program of its own, built plain and under -fsanitize=address,undefined by tests/test_carve_emu.py.
// A description is a list of arrays (element size, count, alignment).  For a few hundred random ones and for the library's own blocks
// at their smallest, an odd and their largest shapes it checks that
//   1. the measuring walk and the placing walk end at the same offset
//   2. every placed pointer is aligned as asked
//   3. the arrays lie in description order inside [base, base + total) and do not overlap: each is filled with its index, and the whole
//      block is read back byte by byte (the bytes between arrays still hold the block's initial zero)
//   4. an array of no elements takes no bytes and still gets a pointer inside the block or at its end
//   5. take(.., alignof(T)) behind an array whose byte size is a multiple of alignof(T) leaves no gap (what a single copy of both needs)
//   6. with 256-byte alignment throughout, the offsets are (previous end + 255) & ~255, computed here
// and that the library's blocks have the offsets of the hand-written chains they replace (written out below as they stood).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../u-vip-slam_amd/csrc/carve.hpp"

using uvo::Carve;

namespace {

int g_fail = 0;
#define CHECK(cond, ...)                        \
  do {                                          \
    if (!(cond)) {                              \
      if (++g_fail <= 20) {                     \
        printf("FAIL %s:%d  ", __FILE__, __LINE__); \
        printf(__VA_ARGS__);                    \
        printf("\n");                           \
      }                                         \
    }                                           \
  } while (0)

template <size_t N>
struct Elem {
  uint8_t b[N];
};

struct Array {
  size_t esize, count, align;
};

// one take of the description's element size; the pointer comes back as bytes
void take(Carve& c, const Array& a, uint8_t*& p) {
#define CASE(N)                                   \
  case N: {                                       \
    Elem<N>* q = reinterpret_cast<Elem<N>*>(p);   \
    c.take(q, a.count, a.align);                  \
    p = reinterpret_cast<uint8_t*>(q);            \
    return;                                       \
  }
  switch (a.esize) {
    CASE(1) CASE(2) CASE(4) CASE(8) CASE(12) CASE(16) CASE(64) CASE(80) CASE(96) CASE(128) CASE(160) CASE(256)
    default:
      printf("FAIL no element of %zu bytes\n", a.esize);
      exit(2);
  }
#undef CASE
}

// checks 1 - 4 (and 6 where every alignment is 256); returns the offsets, the total last
std::vector<size_t> walk(const char* what, const std::vector<Array>& d) {
  Carve m{nullptr};
  uint8_t* const untouched = reinterpret_cast<uint8_t*>(uintptr_t(0x55));
  for (const Array& a : d) {
    uint8_t* p = untouched;
    take(m, a, p);
    CHECK(p == untouched, "%s: the measuring walk wrote a pointer", what);
  }
  const size_t total = m.off;
  void* mem = nullptr;
  if (posix_memalign(&mem, 256, std::max<size_t>(total, 1)) != 0) exit(2);  // a device block is aligned at least as well
  uint8_t* base = static_cast<uint8_t*>(mem);
  memset(base, 0, total);
  Carve c{base};
  std::vector<uint8_t*> ptr(d.size());
  std::vector<size_t> off;
  size_t prev_end = 0;
  bool all256 = true;
  for (size_t i = 0; i < d.size(); ++i) {
    ptr[i] = nullptr;
    take(c, d[i], ptr[i]);
    const size_t o = (size_t)(ptr[i] - base), bytes = d[i].count * d[i].esize;
    off.push_back(o);
    CHECK(reinterpret_cast<uintptr_t>(ptr[i]) % d[i].align == 0, "%s: array %zu at %p is not aligned to %zu", what, i, (void*)ptr[i], d[i].align);
    CHECK(o >= prev_end && o - prev_end < d[i].align && o + bytes <= total, "%s: array %zu at %zu (+%zu) after %zu in %zu", what, i, o, bytes, prev_end, total);
    CHECK(c.off == o + bytes, "%s: array %zu moved the offset to %zu, not %zu", what, i, c.off, o + bytes);
    all256 = all256 && d[i].align == 256;
    if (all256) CHECK(o == ((prev_end + 255) & ~(size_t)255), "%s: array %zu at %zu, not at the next multiple of 256 behind %zu", what, i, o, prev_end);
    prev_end = o + bytes;
  }
  CHECK(c.off == total, "%s: placing ends at %zu, measuring at %zu", what, c.off, total);
  for (size_t i = 0; i < d.size(); ++i) memset(ptr[i], (int)(i + 1), d[i].count * d[i].esize);
  size_t at = 0;
  for (size_t i = 0; i <= d.size(); ++i) {  // gap (zeros), array i (i + 1), ..., the tail gap is empty
    const size_t gap_end = i < d.size() ? off[i] : total;
    for (; at < gap_end; ++at) CHECK(base[at] == 0, "%s: byte %zu in front of array %zu holds %d", what, at, i, base[at]);
    if (i == d.size()) break;
    for (const size_t end = at + d[i].count * d[i].esize; at < end; ++at)
      CHECK(base[at] == (uint8_t)(i + 1), "%s: byte %zu of array %zu holds %d", what, at, i, base[at]);
  }
  free(mem);
  off.push_back(total);
  return off;
}

void expect(const char* what, const std::vector<Array>& d, const std::vector<size_t>& want) {
  const std::vector<size_t> got = walk(what, d);
  CHECK(got == want, "%s: the offsets differ from the chain's", what);
  if (got != want)
    for (size_t i = 0; i < got.size() && i < want.size(); ++i) printf("  %zu: %zu, chain %zu\n", i, got[i], want[i]);
  printf("%-40s %2zu arrays, %zu bytes\n", what, d.size(), got.back());
}

size_t up(size_t v) { return (v + 255) & ~(size_t)255; }
size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }

// ---- the library's blocks: the description as the create function gives it, and the offset chain it replaced ----
void pnpsolver_set(size_t S, size_t N) {
  const size_t W = (N + 63) / 64, T = S * 320, call = 80, result = 128, stride = 9;
  const size_t o_p3d = 0, o_p2d = up(o_p3d + S * N * 12), o_me = up(o_p2d + S * N * 8), o_bm = up(o_me + S * N * 4), o_bp = up(o_bm + S * 2 * W * 8),
               o_call = up(o_bp + S * 2 * 96), o_hyp = o_call + S * call, o_pose = up(o_hyp + T * stride * 4), o_cnt = up(o_pose + T * 96),
               o_mask = up(o_cnt + T * 4), o_list = up(o_mask + T * W * 8), o_res = up(o_list + S * N * 4), o_om = o_res + S * result, bytes = o_om + S * W * 8;
  char what[64];
  snprintf(what, sizeof what, "PnPsolver set (%zu, %zu)", S, N);
  expect(what, {{4, S * N * 3, 256}, {4, S * N * 2, 256}, {4, S * N, 256}, {8, S * 2 * W, 256}, {8, S * 2 * 12, 256}, {call, S, 256}, {4, T * stride, 4},
                {8, T * 12, 256}, {4, T, 256}, {8, T * W, 256}, {4, S * N, 256}, {result, S, 256}, {8, S * W, 8}},
         {o_p3d, o_p2d, o_me, o_bm, o_bp, o_call, o_hyp, o_pose, o_cnt, o_mask, o_list, o_res, o_om, bytes});
  expect("  its upload mirror", {{call, S, 256}, {4, T * stride, 4}}, {0, S * call, S * call + T * stride * 4});
  expect("  its download mirror", {{result, S, 256}, {8, S * W, 8}}, {0, S * result, S * result + S * W * 8});
}

void sim3solver_set(size_t S, size_t N) {
  const size_t W = (N + 63) / 64, T = S * 320, call = 64, result = 160, stride = 4, hyp = 48;
  const size_t o_x1 = 0, o_x2 = up(o_x1 + S * N * 12), o_p1 = up(o_x2 + S * N * 12), o_p2 = up(o_p1 + S * N * 8), o_e1 = up(o_p2 + S * N * 8),
               o_e2 = up(o_e1 + S * N * 4), o_call = up(o_e2 + S * N * 4), o_sub = o_call + S * call, o_hyp = up(o_sub + T * stride * 4),
               o_cnt = up(o_hyp + T * hyp * 4), o_mask = up(o_cnt + T * 4), o_res = up(o_mask + T * W * 8), o_om = o_res + S * result, bytes = o_om + S * W * 8;
  char what[64];
  snprintf(what, sizeof what, "Sim3Solver set (%zu, %zu)", S, N);
  expect(what, {{4, S * N * 3, 256}, {4, S * N * 3, 256}, {4, S * N * 2, 256}, {4, S * N * 2, 256}, {4, S * N, 256}, {4, S * N, 256}, {call, S, 256},
                {4, T * stride, 4}, {4, T * hyp, 256}, {4, T, 256}, {8, T * W, 256}, {result, S, 256}, {8, S * W, 8}},
         {o_x1, o_x2, o_p1, o_p2, o_e1, o_e2, o_call, o_sub, o_hyp, o_cnt, o_mask, o_res, o_om, bytes});
  expect("  its upload mirror", {{call, S, 256}, {4, T * stride, 4}}, {0, S * call, S * call + T * stride * 4});
  expect("  its download mirror", {{result, S, 256}, {8, S * W, 8}}, {0, S * result, S * result + S * W * 8});
}

void initializer(size_t N) {
  const size_t W = (N + 63) / 64, T = 1024, call = 128, sel = 256, out = 256;
  const size_t up_bytes = call + N * 8 + N * 4 + T * 8 * 4, down_bytes = out + W * 8 + N * 12 + N;
  const size_t o_k1 = 0, o_up = up(o_k1 + N * 8), o_F = up(o_up + up_bytes), o_sc = up(o_F + T * 36), o_mask = up(o_sc + T * 4), o_sel = up(o_mask + T * W * 8),
               o_fl = up(o_sel + sel), o_cos = up(o_fl + 4 * N), o_p3d = up(o_cos + 16 * N), o_down = up(o_p3d + 48 * N), bytes = o_down + down_bytes;
  char what[64];
  snprintf(what, sizeof what, "Initializer (%zu)", N);
  // the exchanges, as the host wrote and read them with pointer arithmetic: InitCall | keys2 | matches12 | sets, InitOut | mask words | p3d | triangulated
  expect("  its upload", {{call, 1, 256}, {4, N * 2, 4}, {4, N, 4}, {4, T * 8, 4}}, {0, call, call + N * 8, call + N * 12, up_bytes});
  expect("  its download", {{out, 1, 256}, {8, W, 8}, {4, N * 3, 4}, {1, N, 1}}, {0, out, out + W * 8, out + W * 8 + N * 12, down_bytes});
  expect(what, {{4, N * 2, 256}, {1, up_bytes, 256}, {4, T * 9, 256}, {4, T, 256}, {8, T * W, 256}, {sel, 1, 256}, {1, 4 * N, 256}, {4, 4 * N, 256},
                {4, 4 * N * 3, 256}, {1, down_bytes, 256}},
         {o_k1, o_up, o_F, o_sc, o_mask, o_sel, o_fl, o_cos, o_p3d, o_down, bytes});
}

void pnp_scratch(size_t N) {
  const size_t cap = 1000, out = 128;
  const size_t o_io = 0, o_uf = up(o_io + N * 20), o_ud = up(o_uf + N * 8), o_sub = up(o_ud + N * 16), o_end = up(o_sub + cap * 5 * 4), o_pose = up(o_end + cap * 4),
               o_cnt = up(o_pose + cap * 12 * 8), o_out = up(o_cnt + cap * 4), bytes = o_out + out + N * 4;
  char what[64];
  snprintf(what, sizeof what, "PnP scratch (%zu)", N);
  expect(what, {{4, N * 5, 256}, {4, N * 2, 256}, {8, N * 2, 256}, {4, cap * 5, 256}, {4, cap, 256}, {8, cap * 12, 256}, {4, cap, 256}, {out, 1, 256}, {4, N, 4}},
         {o_io, o_uf, o_ud, o_sub, o_end, o_pose, o_cnt, o_out, o_out + out, bytes});
}

void fm_scratch() {
  const size_t cap = 1000, lanes = 1024;
  const size_t o_sub = 64, o_end = o_sub + cap * 7 * 4, o_nm = o_end + cap * 4, o_mod = (o_nm + cap * 4 + 63) & ~(size_t)63, o_sc = o_mod + cap * 27 * 8,
               o_jump = o_sc + cap * 3 * 8, bytes = o_jump + lanes * 8;
  expect("findFundamentalMat scratch", {{16, 1, 64}, {4, cap * 7, 64}, {4, cap, 4}, {4, cap, 4}, {8, cap * 27, 64}, {8, cap * 3, 8}, {8, lanes, 8}},
         {0, o_sub, o_end, o_nm, o_mod, o_sc, o_jump, bytes});
}

void kfdb_pinned(size_t K, size_t W, size_t H) {
  const size_t C = 10, meta = 8, stage = std::max(up16(W * 12) + K, up16(H * 4) + K) + 16, n_out = meta + std::max(K, (size_t)3);
  const size_t o_id = 0, o_seq = o_id + up16(K * 8), o_sos = o_seq + up16(K * 4), o_n = o_sos + up16(K * 4), o_cov = o_n + up16(K * 4), o_out = o_cov + up16(K * C * 4),
               o_in = o_out + up16(n_out * 4), o_hh = o_in + up16(K), o_st = o_hh + up16(K), total = o_st + stage;
  char what[64];
  snprintf(what, sizeof what, "keyframe database, pinned (%zu, %zu, %zu)", K, W, H);
  expect(what, {{8, K, 16}, {4, K, 16}, {4, K, 16}, {4, K, 16}, {4, K * C, 16}, {4, n_out, 16}, {1, K, 16}, {1, K, 16}, {1, stage, 16}},
         {o_id, o_seq, o_sos, o_n, o_cov, o_out, o_in, o_hh, o_st, total});
}

// check 5 with real types: T directly behind an array whose size is a multiple of alignof(T)
template <class A, class T>
void adjacent(size_t na, size_t nt, size_t first_align) {
  A* a = nullptr;
  T* t = nullptr;
  Carve m{nullptr};
  m.take(a, na, first_align).take(t, nt, alignof(T));
  CHECK((na * sizeof(A)) % alignof(T) == 0, "adjacent: a case for the other branch");
  CHECK(m.off == na * sizeof(A) + nt * sizeof(T), "adjacent: %zu bytes for %zu + %zu", m.off, na * sizeof(A), nt * sizeof(T));
  void* mem = nullptr;
  if (posix_memalign(&mem, 256, std::max<size_t>(m.off, 1)) != 0) exit(2);
  Carve c{static_cast<uint8_t*>(mem)};
  c.take(a, na, first_align).take(t, nt, alignof(T));
  CHECK(reinterpret_cast<uint8_t*>(t) == reinterpret_cast<uint8_t*>(a + na), "adjacent: a gap of %td bytes", reinterpret_cast<uint8_t*>(t) - reinterpret_cast<uint8_t*>(a + na));
  const T* ct = nullptr;  // the form the kernels' read-only views take
  Carve c2{static_cast<uint8_t*>(mem)};
  c2.take(a, na, first_align).take(ct, nt, alignof(T));
  CHECK(ct == t, "adjacent: const T*& placed elsewhere");
  free(mem);
}

}  // namespace

int main() {
  std::mt19937 rng(20240607);
  const size_t esizes[] = {1, 2, 4, 8, 12, 96}, aligns[] = {1, 4, 8, 16, 64, 256};
  int zero_counts = 0, n256 = 0;
  for (int it = 0; it < 400; ++it) {
    std::vector<Array> d(1 + rng() % 12);
    const bool all256 = it % 4 == 0;  // a quarter of them the shape of the device blocks
    for (Array& a : d) {
      a.esize = esizes[rng() % 6];
      a.count = rng() % 8 == 0 ? 0 : rng() % 5001;
      a.align = all256 ? 256 : aligns[rng() % 6];
      zero_counts += a.count == 0;
    }
    n256 += all256;
    char what[32];
    snprintf(what, sizeof what, "random %d", it);
    walk(what, d);
  }
  printf("400 random descriptions, %d of them 256-aligned throughout, %d empty arrays\n", n256, zero_counts);
  walk("empty description", {});
  walk("one empty array", {{4, 0, 256}});
  walk("empty arrays only", {{4, 0, 256}, {8, 0, 8}, {1, 0, 1}});

  for (size_t na : {1, 2, 3, 64}) {
    adjacent<Elem<80>, int32_t>(na, 2880, 256);       // call records, then subset records
    adjacent<Elem<128>, uint64_t>(na, 2 * na, 256);   // result records, then the returned sets
    adjacent<Elem<64>, int32_t>(na, 1280, 256);
    adjacent<Elem<160>, uint64_t>(na, na, 256);
    adjacent<double, uint64_t>(na * 3, 1024, 64);
    adjacent<Elem<12>, float>(na, 7, 4);
    adjacent<uint64_t, uint8_t>(na, 5, 8);
  }

  const size_t sets[][2] = {{1, 4}, {2, 65}, {64, 16384}};
  for (const auto& s : sets) pnpsolver_set(s[0], s[1]);
  for (const auto& s : sets) sim3solver_set(s[0], s[1] == 4 ? 3 : s[1]), sim3solver_set(s[0], s[1]);
  for (size_t n : {8, 65, 16384}) initializer(n);
  for (size_t n : {1, 5, 4096}) pnp_scratch(n);
  fm_scratch();
  kfdb_pinned(1, 1, 1);
  kfdb_pinned(3, 4, 2);
  kfdb_pinned(65536, 4096, 4096);

  if (g_fail) {
    printf("%d checks FAILed\n", g_fail);
    return 1;
  }
  printf("all checks passed\n");
  return 0;
}
