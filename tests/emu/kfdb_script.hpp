// The text form of a keyframe-database case (tests/kfdb_cases.py: to_script / parse_output), read and answered by the stand-alone
// programs that run a case outside Python: the host build of kfdb_core.hpp (kfdb_emu.cpp) and the C++ adaptor's driver
// (tests/cpp/compat_kfdb.cpp).  Floats and doubles travel as the decimal of their bits.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <istream>
#include <string>
#include <vector>

#include "../../include/uvo/uvo.h"

namespace kfdb_script {

struct Op {
  std::string kind;  // create add erase clear cov reloc loop haloc end
  int64_t id = 0;
  int a = 0, b = 0, c = 0;  // create: max_keyframes, max_words, hash_len; erase / cov: a = slot
  std::vector<uint32_t> ids;
  std::vector<double> vals;
  bool has_hash = false;
  std::vector<float> hash;
  std::vector<int32_t> slots;  // cov: the neighbours; loop: the connected slots
  std::vector<int64_t> excl;
  float score = 0.0f;          // minScore / maxScore
};

inline float f32_of(uint32_t b) {
  float f;
  memcpy(&f, &b, 4);
  return f;
}
inline uint32_t bits_of(float f) {
  uint32_t b;
  memcpy(&b, &f, 4);
  return b;
}

inline void read_bow(std::istream& in, int n, Op& op) {
  op.ids.resize((size_t)n), op.vals.resize((size_t)n);
  for (auto& x : op.ids) in >> x;
  for (auto& v : op.vals) {
    uint64_t b;
    in >> b;
    memcpy(&v, &b, 8);
  }
}
inline void read_hash(std::istream& in, int len, Op& op) {
  op.hash.assign((size_t)len, 0.0f);
  if (!op.has_hash) return;
  for (auto& h : op.hash) {
    uint32_t b;
    in >> b;
    h = f32_of(b);
  }
}
inline float read_f32(std::istream& in) {
  uint32_t b;
  in >> b;
  return f32_of(b);
}

inline bool read_op(std::istream& in, int hash_len, Op& op) {
  op = Op();
  if (!(in >> op.kind) || op.kind == "end") return false;
  int n = 0, h = 0;
  if (op.kind == "create") {
    in >> op.a >> op.b >> op.c;
  } else if (op.kind == "add") {
    in >> op.id >> n >> h;
    op.has_hash = h != 0;
    read_bow(in, n, op);
    read_hash(in, hash_len, op);
  } else if (op.kind == "erase") {
    in >> op.a;
  } else if (op.kind == "cov") {
    in >> op.a >> n;
    op.slots.resize((size_t)n);
    for (auto& s : op.slots) in >> s;
  } else if (op.kind == "reloc" || op.kind == "loop") {
    in >> op.id >> n;
    read_bow(in, n, op);
    if (op.kind == "loop") {
      in >> n;
      op.slots.resize((size_t)n);
      for (auto& s : op.slots) in >> s;
      op.score = read_f32(in);
    }
  } else if (op.kind == "haloc") {
    in >> op.id >> h;
    op.has_hash = h != 0;
    read_hash(in, hash_len, op);
    in >> n;
    op.excl.resize((size_t)n);
    for (auto& e : op.excl) in >> e;
    op.score = read_f32(in);
  }
  return (bool)in;
}

inline void print_cand(const int32_t* cand, int n) {
  printf("cand %d", n);
  for (int i = 0; i < n; ++i) printf(" %d", cand[i]);
  printf("\n");
}
inline void print_table(int maxc, int minc, const uvo_kfdb_query_row* rows, int n) {
  printf("table %d %d %d\n", maxc, minc, n);
  for (int i = 0; i < n; ++i)
    printf("row %d %d %d %d %u %u\n", rows[i].slot, rows[i].words, rows[i].flags, rows[i].best, bits_of(rows[i].score), bits_of(rows[i].acc));
}
inline void print_haloc(const float* m, const uint8_t* kept, int n) {
  printf("haloc %d\n", n);
  for (int i = 0; i < n; ++i) printf("h %u %d\n", bits_of(m[i]), (int)kept[i]);
}
inline void print_state(const uvo_kfdb_fields* st, int n) {
  printf("state %d\n", n);
  for (int i = 0; i < n; ++i)
    printf("st %lld %lld %d %d %u %u\n", (long long)st[i].loop_query, (long long)st[i].reloc_query, st[i].loop_words, st[i].reloc_words, bits_of(st[i].loop_score),
           bits_of(st[i].reloc_score));
}

}  // namespace kfdb_script
