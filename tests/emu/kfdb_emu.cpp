// Host build of the keyframe database's rules (u-vip-slam_amd/csrc/kfdb_core.hpp): the functions the kernels of kfdb.hip call, run by a
// serial loop over the slots, with std::sort where the device sorts by the same unique key.  A stand-alone program: it reads a case
// as text (tests/kfdb_cases.py: to_script) from the file named on the command line and prints what parse_output reads; the CPU suite
// holds that to the literal model bit for bit (tests/test_kfdb_emu.py), once more in a build with the address and undefined-behaviour
// sanitizers.  `--time N`: instead of printing, repeat every query N times and print the mean seconds per query kind (one core; the
// figure tools/kfdb_latency.py sets beside the device's).
#include <algorithm>
#include <chrono>
#include <fstream>
#include <iostream>

#include "../../u-vip-slam_amd/csrc/kfdb_core.hpp"
#include "kfdb_script.hpp"

using namespace uvo::kfdb;

struct HostDb {
  int max_kf = 0, max_words = 0, hash_len = 0, n = 0;
  std::vector<int64_t> id;
  std::vector<uint32_t> seq;
  std::vector<uint8_t> in_file, has_hash;
  std::vector<int32_t> kf_n, cov;
  std::vector<uint32_t> bow_id;
  std::vector<double> bow_val;
  std::vector<float> hash_t;  // transposed like the device's
  std::vector<uvo_kfdb_fields> state;
  // last query
  std::vector<uvo_kfdb_query_row> rows;
  int maxc = 0, minc = 0;
  std::vector<float> hm;
  std::vector<uint8_t> hkept;

  void create(int k, int w, int h) {
    max_kf = k, max_words = w, hash_len = h, n = 0;
    id.assign(k, 0), seq.assign(k, 0), in_file.assign(k, 0), has_hash.assign(k, 0), kf_n.assign(k, 0), cov.assign((size_t)k * kCovisibles, -1);
    bow_id.assign((size_t)k * w, 0), bow_val.assign((size_t)k * w, 0.0), hash_t.assign((size_t)k * h, 0.0f), state.assign(k, uvo_kfdb_fields());
  }
  int add(const kfdb_script::Op& op) {
    const int k = n++;
    id[k] = op.id, seq[k] = (uint32_t)k, in_file[k] = 1, has_hash[k] = op.has_hash, kf_n[k] = (int)op.ids.size();
    std::copy(op.ids.begin(), op.ids.end(), bow_id.begin() + (size_t)k * max_words);
    std::copy(op.vals.begin(), op.vals.end(), bow_val.begin() + (size_t)k * max_words);
    for (int i = 0; i < hash_len; ++i) hash_t[(size_t)i * max_kf + k] = op.hash[i];
    state[k] = uvo_kfdb_fields();
    for (int c = 0; c < kCovisibles; ++c) cov[(size_t)k * kCovisibles + c] = -1;
    return k;
  }
  void set_cov(int slot, const std::vector<int32_t>& nb) {
    for (int c = 0; c < kCovisibles; ++c) cov[(size_t)slot * kCovisibles + c] = c < (int)nb.size() ? nb[c] : -1;
  }

  std::vector<int32_t> bow_query(int mode, int64_t qid, const std::vector<uint32_t>& qi, const std::vector<double>& qv, const std::vector<int32_t>& connected,
                                 float min_score) {
    const int nq = (int)qi.size();
    std::vector<uint8_t> conn((size_t)std::max(n, 1), 0);
    for (int s : connected) conn[s] = 1;
    std::vector<float> score(n, 0.0f);
    std::vector<uint64_t> keys;
    std::vector<uint8_t> listed(n, 0);
    maxc = 0, minc = 0, rows.clear();
    // per slot: what k_kfdb_words computes, then the walk's effect on the stored fields
    for (int s = 0; s < n; ++s) {
      int cnt = 0, first = -1;
      double sum = 0.0;
      if (in_file[s])
        for (int j = 0; j < kf_n[s]; ++j) {
          const int q = find_word(qi.data(), nq, bow_id[(size_t)s * max_words + j]);
          if (q < 0) continue;
          if (first < 0) first = q;
          ++cnt;
          sum += l1_term(qv[q], bow_val[(size_t)s * max_words + j]);
        }
      score[s] = l1_finish(sum);
      if (cnt <= 0) continue;
      const bool loop = mode == kLoop;
      int64_t& q = loop ? state[s].loop_query : state[s].reloc_query;
      int32_t& w = loop ? state[s].loop_words : state[s].reloc_words;
      if (touch(mode, qid, cnt, loop && conn[s], q, w)) {
        listed[s] = 1;
        keys.push_back(list_key(first, seq[s]));
        maxc = std::max(maxc, (int)w);
      }
    }
    std::vector<int32_t> cand;
    if (keys.empty()) return cand;
    minc = min_common_words(maxc);
    for (int s = 0; s < n; ++s) {
      if (!listed[s]) continue;
      if (mode == kLoop) {
        if (state[s].loop_words > minc) state[s].loop_score = score[s];
      } else if (state[s].reloc_words > minc) {
        state[s].reloc_score = score[s];
      }
    }
    std::sort(keys.begin(), keys.end());
    float best_acc = mode == kLoop ? min_score : 0.0f;
    for (uint64_t key : keys) {
      const int s = (int)(uint32_t)key;  // slot == add sequence: slots are handed out in add order
      uvo_kfdb_query_row r;
      r.slot = s, r.words = mode == kLoop ? state[s].loop_words : state[s].reloc_words, r.flags = UVO_KFDB_LISTED, r.best = -1;
      r.score = mode == kLoop ? state[s].loop_score : state[s].reloc_score, r.acc = 0.0f;
      if (r.words > minc) {
        r.flags |= UVO_KFDB_SCORED;
        if (mode != kLoop || r.score >= min_score) {
          r.flags |= UVO_KFDB_ENTERED;
          accumulate(mode, qid, minc, r.score, s, cov.data() + (size_t)s * kCovisibles, state.data(), r.acc, r.best);
          if (r.acc > best_acc) best_acc = r.acc;
        }
      }
      rows.push_back(r);
    }
    const float min_retain = 0.75f * best_acc;
    std::vector<uint8_t> taken(n, 0);
    for (auto& r : rows)
      if ((r.flags & UVO_KFDB_ENTERED) && r.acc > min_retain) {
        r.flags |= UVO_KFDB_RETAINED;
        if (!taken[r.best]) taken[r.best] = 1, cand.push_back(r.best);
      }
    return cand;
  }

  std::vector<int32_t> haloc_query(int64_t qid, bool q_has, const std::vector<float>& q, const std::vector<int64_t>& excl, float max_score) {
    hm.assign(n, 0.0f), hkept.assign(n, 0);
    std::vector<uint64_t> keys;
    for (int s = 0; s < n; ++s) {
      if (id[s] == qid || std::find(excl.begin(), excl.end(), id[s]) != excl.end()) continue;
      hm[s] = hash_match(q.data(), q_has, hash_t.data() + s, max_kf, has_hash[s] != 0, hash_len);
      if (haloc_keep(hm[s], max_score)) hkept[s] = 1, keys.push_back(haloc_key(hm[s], seq[s]));
    }
    std::sort(keys.begin(), keys.end());
    std::vector<int32_t> cand;
    if (keys.size() >= 3)
      for (int i = 0; i < 3; ++i) cand.push_back((int32_t)(uint32_t)keys[i]);
    return cand;
  }
};

int main(int argc, char** argv) {
  int reps = 0;
  const char* path = nullptr;
  for (int i = 1; i < argc; ++i) {
    if (std::string(argv[i]) == "--time" && i + 1 < argc) reps = atoi(argv[++i]);
    else path = argv[i];
  }
  if (!path) {
    fprintf(stderr, "usage: kfdb_emu [--time N] script\n");
    return 2;
  }
  std::ifstream in(path);
  if (!in) {
    fprintf(stderr, "cannot read %s\n", path);
    return 2;
  }
  HostDb db;
  kfdb_script::Op op;
  double t_sum[3] = {0, 0, 0};
  int t_n[3] = {0, 0, 0};
  while (kfdb_script::read_op(in, db.hash_len, op)) {
    if (op.kind == "create") {
      db.create(op.a, op.b, op.c);
    } else if (op.kind == "add") {
      const int k = db.add(op);
      if (!reps) printf("slot %d\n", k);
    } else if (op.kind == "erase") {
      db.in_file[op.a] = 0;
      if (!reps) printf("ok\n");
    } else if (op.kind == "clear") {
      db.n = 0;
      if (!reps) printf("ok\n");
    } else if (op.kind == "cov") {
      db.set_cov(op.a, op.slots);
      if (!reps) printf("ok\n");
    } else if (op.kind == "reloc" || op.kind == "loop" || op.kind == "haloc") {
      const int kind = op.kind == "reloc" ? 0 : op.kind == "loop" ? 1 : 2;
      if (reps) {
        const std::vector<uvo_kfdb_fields> saved = db.state;  // every repetition starts from the same stored fields
        for (int r = 0; r < reps; ++r) {
          db.state = saved;
          const auto t0 = std::chrono::steady_clock::now();
          const auto cand = kind == 2 ? db.haloc_query(op.id, op.has_hash, op.hash, op.excl, op.score)
                                      : db.bow_query(kind == 1 ? kLoop : kReloc, op.id, op.ids, op.vals, op.slots, op.score);
          t_sum[kind] += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
          ++t_n[kind];
          if (cand.size() > (size_t)db.n) return 3;
        }
        continue;
      }
      if (kind == 2) {
        const auto cand = db.haloc_query(op.id, op.has_hash, op.hash, op.excl, op.score);
        kfdb_script::print_cand(cand.data(), (int)cand.size());
        kfdb_script::print_haloc(db.hm.data(), db.hkept.data(), db.n);
      } else {
        const auto cand = db.bow_query(kind == 1 ? kLoop : kReloc, op.id, op.ids, op.vals, op.slots, op.score);
        kfdb_script::print_cand(cand.data(), (int)cand.size());
        kfdb_script::print_table(db.maxc, db.minc, db.rows.data(), (int)db.rows.size());
      }
      kfdb_script::print_state(db.state.data(), db.n);
    }
  }
  if (reps) printf("{\"reloc_s\": %.9g, \"loop_s\": %.9g, \"haloc_s\": %.9g}\n", t_n[0] ? t_sum[0] / t_n[0] : 0.0, t_n[1] ? t_sum[1] / t_n[1] : 0.0,
                   t_n[2] ? t_sum[2] / t_n[2] : 0.0);
  return 0;
}
