// USLAM::KeyFrameDatabase (include/KeyFrameDatabase.h, src/KeyFrameDatabase.cc) over the C ABI's device database (uvo_kfdb_* in
// uvo/uvo.h), with the reference's method set, so that Tracking::Relocalisation (src/Tracking.cc:2379) and LoopClosing::DetectLoop
// (src/LoopClosing.cc:195-196) compile unchanged against it:
//
//     - KeyFrameDatabase* mpKeyFrameDB = new KeyFrameDatabase(*mpVocabulary);
//     + USLAM::KeyFrameDatabase<KeyFrame, FrameKTL>* mpKeyFrameDB = new USLAM::KeyFrameDatabase<KeyFrame, FrameKTL>(max_keyframes, max_words, hash_len);
//       mpKeyFrameDB->add(pKF);  mpKeyFrameDB->erase(pKF);  mpKeyFrameDB->clear();
//       vpCandidateKFs = mpKeyFrameDB->DetectRelocalisationCandidates(&mCurrentFrame);
//       vpCandidateKFs = mpKeyFrameDB->DetectLoopCandidates(mpCurrentKF, minScore);
//       vpCandidateKFsHaloc = mpKeyFrameDB->DetectLoopCandidatesHaloc(mpCurrentKF, maxHalocScore, &haloc);
//
// The key frame type needs mnId, mBowVec (a map from word id to value: begin()/end(), ->first, ->second), GetHalocVector(),
// GetBestCovisibilityKeyFrames(10), GetConnectedKeyFrames() and GetVectorCovisibleKeyFrames(); the frame type mnId and mBowVec.  kfVec
// and cluster_lc_found_ stay public members as in the reference; kfVec[slot] is the key frame of a device slot.
//
// The six query fields (mnLoopQuery, mnLoopWords, mLoopScore, mnRelocQuery, mnRelocWords, mRelocScore) live on the device, not in the
// key frames: nothing outside KeyFrameDatabase.cc reads them.  The covisible rows the accumulation reads are refreshed in front of
// every BoW query: by default from every key frame in the inverted file (exact with no change to the host); after
// UseCovisibilityHook(true) only from the key frames named through NotifyCovisibilityChanged since the last query (and the newly added
// ones) -- one line at the end of KeyFrame::UpdateBestCovisibles (src/KeyFrame.cc:420-439): mpKeyFrameDB->NotifyCovisibilityChanged(this);
// A key frame beyond max_keyframes is not added (add returns false; the reference's add returns nothing).  clear() also drops kfVec,
// where the reference keeps its pointers (dangling after Tracking::Reset).  Header only, C++11, no OpenCV, no boost.
#ifndef UVO_COMPAT_KEYFRAMEDATABASE_H_
#define UVO_COMPAT_KEYFRAMEDATABASE_H_
#include <stdint.h>

#include <map>
#include <mutex>
#include <set>
#include <utility>
#include <vector>

#include "uvo/uvo.h"

namespace USLAM {

template <class KeyFrame, class Frame>
class KeyFrameDatabase {
 public:
  KeyFrameDatabase(int max_keyframes, int max_words, int hash_len, int device = 0) : db_(0), hash_len_(hash_len), hook_(false) {
    uvo_kfdb_create(max_keyframes, max_words, hash_len, device, &db_);
    cand_.resize((size_t)(max_keyframes > 3 ? max_keyframes : 3));
  }
  ~KeyFrameDatabase() { uvo_kfdb_destroy(db_); }
  bool ok() const { return db_ != 0; }
  uvo_kfdb* handle() { return db_; }
  // the device slot of a key frame, -1 when it has none
  int SlotOf(KeyFrame* pKF) const {
    typename std::map<KeyFrame*, int>::const_iterator it = slot_.find(pKF);
    return it == slot_.end() ? -1 : it->second;
  }

  bool add(KeyFrame* pKF) {
    std::lock_guard<std::mutex> lock(mMutex);
    Bow(pKF->mBowVec);
    const std::vector<float> h = pKF->GetHalocVector();
    int slot = -1;
    if (uvo_kfdb_add(db_, (int64_t)pKF->mnId, ids_.data(), vals_.data(), (int)ids_.size(), (int)h.size() == hash_len_ ? h.data() : 0, &slot) != UVO_OK) return false;
    kfVec.push_back(pKF);  // slot == kfVec.size() - 1: slots are handed out in add order
    slot_[pKF] = slot;
    in_file_.push_back(1);
    changed_.insert(slot);
    return true;
  }

  void erase(KeyFrame* pKF) {
    std::lock_guard<std::mutex> lock(mMutex);
    const int slot = SlotOf(pKF);
    if (slot < 0) return;
    uvo_kfdb_erase(db_, slot);
    in_file_[(size_t)slot] = 0;
  }

  void clear() {
    std::lock_guard<std::mutex> lock(mMutex);
    uvo_kfdb_clear(db_);
    kfVec.clear(), slot_.clear(), in_file_.clear(), changed_.clear(), unresolved_.clear();
  }

  // the hook of the optional refresh mode; harmless in the default mode
  void UseCovisibilityHook(bool on) { hook_ = on; }
  void NotifyCovisibilityChanged(KeyFrame* pKF) {
    std::lock_guard<std::mutex> lock(mMutex);
    const int slot = SlotOf(pKF);
    if (slot >= 0) changed_.insert(slot);
  }

  std::vector<KeyFrame*> DetectRelocalisationCandidates(Frame* F) {
    std::lock_guard<std::mutex> lock(mMutex);
    RefreshCovisibles();
    Bow(F->mBowVec);
    int n = 0;
    if (uvo_kfdb_detect_reloc(db_, (int64_t)F->mnId, ids_.data(), vals_.data(), (int)ids_.size(), cand_.data(), (int)cand_.size(), &n) != UVO_OK) n = 0;
    return KeyFrames(n);
  }

  std::vector<KeyFrame*> DetectLoopCandidates(KeyFrame* pKF, float minScore) {
    const std::set<KeyFrame*> spConnectedKeyFrames = pKF->GetConnectedKeyFrames();
    std::lock_guard<std::mutex> lock(mMutex);
    RefreshCovisibles();
    Bow(pKF->mBowVec);
    std::vector<int32_t> connected;
    for (typename std::set<KeyFrame*>::const_iterator it = spConnectedKeyFrames.begin(); it != spConnectedKeyFrames.end(); ++it) {
      const int s = SlotOf(*it);
      if (s >= 0) connected.push_back(s);
    }
    int n = 0;
    if (uvo_kfdb_detect_loop(db_, (int64_t)pKF->mnId, ids_.data(), vals_.data(), (int)ids_.size(), connected.data(), (int)connected.size(), minScore, cand_.data(),
                             (int)cand_.size(), &n) != UVO_OK)
      n = 0;
    return KeyFrames(n);
  }

  // the third argument is the reference's haloc::Hash*, whose match() runs on the device here
  template <class Hash>
  std::vector<KeyFrame*> DetectLoopCandidatesHaloc(KeyFrame* pKF, float maxScore, Hash*) {
    const std::vector<KeyFrame*> ConnectedKeyFrames = pKF->GetVectorCovisibleKeyFrames();
    std::lock_guard<std::mutex> lock(mMutex);
    std::vector<int64_t> no_candidates;  // :81-92
    for (size_t i = 0; i < cluster_lc_found_.size(); i++) {
      if ((int64_t)cluster_lc_found_[i].first == (int64_t)pKF->mnId) no_candidates.push_back(cluster_lc_found_[i].second);
      if ((int64_t)cluster_lc_found_[i].second == (int64_t)pKF->mnId) no_candidates.push_back(cluster_lc_found_[i].first);
    }
    for (size_t i = 0; i < ConnectedKeyFrames.size(); i++) no_candidates.push_back((int64_t)ConnectedKeyFrames[i]->mnId);
    const std::vector<float> hash_q = pKF->GetHalocVector();
    int n = 0;
    if (uvo_kfdb_detect_loop_haloc(db_, (int64_t)pKF->mnId, (int)hash_q.size() == hash_len_ ? hash_q.data() : 0, no_candidates.data(), (int)no_candidates.size(),
                                   maxScore, cand_.data(), &n) != UVO_OK)
      n = 0;
    return KeyFrames(n);
  }

  std::vector<KeyFrame*> kfVec;
  std::vector<std::pair<int, int> > cluster_lc_found_;
  static const int LC_DISCARD_WINDOW = 10;

 protected:
  template <class BowVector>
  void Bow(const BowVector& v) {
    ids_.clear(), vals_.clear();
    for (typename BowVector::const_iterator it = v.begin(); it != v.end(); ++it) ids_.push_back((uint32_t)it->first), vals_.push_back((double)it->second);
    if (ids_.empty()) ids_.reserve(1), vals_.reserve(1);
  }
  void RefreshOne(int slot) {
    const std::vector<KeyFrame*> vpNeighs = kfVec[(size_t)slot]->GetBestCovisibilityKeyFrames(10);
    int32_t row[UVO_KFDB_COVISIBLES];
    int n = 0;
    bool unresolved = false;  // a neighbour without a slot may get one later without this key frame's covisibility changing again
    for (size_t i = 0; i < vpNeighs.size() && n < UVO_KFDB_COVISIBLES; ++i) {
      row[n] = SlotOf(vpNeighs[i]);
      unresolved = unresolved || row[n] < 0;
      ++n;
    }
    uvo_kfdb_set_covisibles(db_, slot, row, n);
    if (unresolved) unresolved_.insert(slot); else unresolved_.erase(slot);
  }
  void RefreshCovisibles() {
    if (hook_) {
      changed_.insert(unresolved_.begin(), unresolved_.end());
      for (std::set<int>::const_iterator it = changed_.begin(); it != changed_.end(); ++it)
        if (in_file_[(size_t)*it]) RefreshOne(*it);
    } else {
      for (size_t s = 0; s < kfVec.size(); ++s)
        if (in_file_[s]) RefreshOne((int)s);  // only a listed key frame's neighbours are read, and only those in the inverted file are listed
    }
    changed_.clear();
  }
  std::vector<KeyFrame*> KeyFrames(int n) const {
    std::vector<KeyFrame*> out;
    out.reserve((size_t)n);
    for (int i = 0; i < n; ++i) out.push_back(kfVec[(size_t)cand_[(size_t)i]]);
    return out;
  }

  uvo_kfdb* db_;
  int hash_len_;
  bool hook_;
  std::map<KeyFrame*, int> slot_;
  std::vector<uint8_t> in_file_;
  std::set<int> changed_, unresolved_;
  std::vector<uint32_t> ids_;
  std::vector<double> vals_;
  std::vector<int32_t> cand_;
  std::mutex mMutex;
};

}  // namespace USLAM
#endif  // UVO_COMPAT_KEYFRAMEDATABASE_H_
