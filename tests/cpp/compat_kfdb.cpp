// Drives USLAM::KeyFrameDatabase (include/uvo/compat/KeyFrameDatabase.h) from C++ with stand-ins for the reference's KeyFrame and
// FrameKTL, the way Tracking::Relocalisation and LoopClosing::DetectLoop call it.  Reads a case as text (tests/kfdb_cases.py:
// to_script; reader shared with the host build, tests/emu/kfdb_script.hpp) and prints what parse_output reads.  `--hook`: covisible rows
// are refreshed only for the key frames named through NotifyCovisibilityChanged.
#include <deque>
#include <fstream>
#include <iostream>
#include <map>
#include <set>

#include "../emu/kfdb_script.hpp"
#include "uvo/compat/KeyFrameDatabase.h"

namespace haloc {
class Hash {};
}  // namespace haloc

struct KeyFrame {
  long unsigned int mnId;
  std::map<unsigned int, double> mBowVec;
  std::vector<float> hash;
  std::vector<KeyFrame*> ordered;  // mvpOrderedConnectedKeyFrames
  std::set<KeyFrame*> connected;
  std::vector<float> GetHalocVector() { return hash; }
  std::vector<KeyFrame*> GetBestCovisibilityKeyFrames(const int& N) {
    return (int)ordered.size() < N ? ordered : std::vector<KeyFrame*>(ordered.begin(), ordered.begin() + N);
  }
  std::set<KeyFrame*> GetConnectedKeyFrames() { return connected; }
  std::vector<KeyFrame*> GetVectorCovisibleKeyFrames() { return ordered; }
};
struct FrameKTL {
  long unsigned int mnId;
  std::map<unsigned int, double> mBowVec;
};

template <class T>
static void fill(T& x, const kfdb_script::Op& op) {
  x.mnId = (long unsigned int)op.id;
  for (size_t i = 0; i < op.ids.size(); ++i) x.mBowVec[op.ids[i]] = op.vals[i];
}

typedef USLAM::KeyFrameDatabase<KeyFrame, FrameKTL> Database;

static void answer(Database& db, const std::vector<KeyFrame*>& cand, bool haloc) {
  std::vector<int32_t> slots;
  for (size_t i = 0; i < cand.size(); ++i) slots.push_back(db.SlotOf(cand[i]));
  kfdb_script::print_cand(slots.data(), (int)slots.size());
  const int n = uvo_kfdb_size(db.handle());
  if (haloc) {
    std::vector<float> m((size_t)n + 1);
    std::vector<uint8_t> kept((size_t)n + 1);
    int k = 0;
    uvo_kfdb_last_haloc(db.handle(), m.data(), kept.data(), n, &k);
    kfdb_script::print_haloc(m.data(), kept.data(), k);
  } else {
    std::vector<uvo_kfdb_query_row> rows((size_t)n + 1);
    int k = 0, maxc = 0, minc = 0;
    uvo_kfdb_last_query(db.handle(), rows.data(), n, &k, &maxc, &minc);
    kfdb_script::print_table(maxc, minc, rows.data(), k);
  }
  std::vector<uvo_kfdb_fields> st((size_t)n + 1);
  uvo_kfdb_state(db.handle(), 0, n, st.data());
  kfdb_script::print_state(st.data(), n);
}

int main(int argc, char** argv) {
  bool hook = false;
  const char* path = 0;
  for (int i = 1; i < argc; ++i) {
    if (std::string(argv[i]) == "--hook") hook = true;
    else path = argv[i];
  }
  std::ifstream in(path ? path : "");
  if (!in) {
    fprintf(stderr, "usage: compat_kfdb [--hook] script\n");
    return 2;
  }
  Database* db = 0;
  std::deque<KeyFrame> owned;  // stable addresses
  KeyFrame outsider;           // a covisible the database never saw
  outsider.mnId = 1u << 30;
  haloc::Hash haloc;
  int hash_len = 0;
  kfdb_script::Op op;
  while (kfdb_script::read_op(in, hash_len, op)) {
    if (op.kind == "create") {
      hash_len = op.c;
      db = new Database(op.a, op.b, op.c);
      if (!db->ok()) {
        fprintf(stderr, "create failed: %s\n", uvo_last_error());
        return 1;
      }
      db->UseCovisibilityHook(hook);
    } else if (op.kind == "add") {
      owned.push_back(KeyFrame());
      KeyFrame* kf = &owned.back();
      fill(*kf, op);
      if (op.has_hash) kf->hash = op.hash;
      if (!db->add(kf)) {
        fprintf(stderr, "add failed: %s\n", uvo_last_error());
        return 1;
      }
      printf("slot %d\n", db->SlotOf(kf));
    } else if (op.kind == "erase") {
      db->erase(db->kfVec[(size_t)op.a]);
      printf("ok\n");
    } else if (op.kind == "clear") {
      db->clear();
      printf("ok\n");
    } else if (op.kind == "cov") {  // KeyFrame::UpdateBestCovisibles
      KeyFrame* kf = db->kfVec[(size_t)op.a];
      kf->ordered.clear();
      for (size_t i = 0; i < op.slots.size(); ++i) kf->ordered.push_back(op.slots[i] < 0 ? &outsider : db->kfVec[(size_t)op.slots[i]]);
      if (hook) db->NotifyCovisibilityChanged(kf);
      printf("ok\n");
    } else if (op.kind == "reloc") {
      FrameKTL F;
      fill(F, op);
      answer(*db, db->DetectRelocalisationCandidates(&F), false);
    } else if (op.kind == "loop") {
      KeyFrame cur;
      fill(cur, op);
      for (size_t i = 0; i < op.slots.size(); ++i) cur.connected.insert(db->kfVec[(size_t)op.slots[i]]);
      cur.connected.insert(&outsider);
      answer(*db, db->DetectLoopCandidates(&cur, op.score), false);
    } else if (op.kind == "haloc") {
      KeyFrame cur;
      cur.mnId = (long unsigned int)op.id;
      if (op.has_hash) cur.hash = op.hash;
      // no_candidates: the first excluded id as an earlier loop closure of this key frame, the others as its covisibles
      std::deque<KeyFrame> covis;
      db->cluster_lc_found_.clear();
      for (size_t i = 0; i < op.excl.size(); ++i) {
        if (i == 0) {
          db->cluster_lc_found_.push_back(std::make_pair((int)op.excl[i], (int)op.id));
          db->cluster_lc_found_.push_back(std::make_pair(12345, 54321));
        } else {
          covis.push_back(KeyFrame());
          covis.back().mnId = (long unsigned int)op.excl[i];
          cur.ordered.push_back(&covis.back());
        }
      }
      answer(*db, db->DetectLoopCandidatesHaloc(&cur, op.score, &haloc), true);
    }
  }
  delete db;
  return 0;
}
