// USLAM::PnPsolver (include/PnPsolver.h, src/PnPsolver.cc) over the C ABI's solver sets (uvo_pnpsolver_* in uvo/uvo.h), for the one
// place the reference uses it from the tracker: Tracking::Relocalisation, src/Tracking.cc:2415-2441.
//
//     - PnPsolver* pSolver = new PnPsolver(mCurrentFrame, vvpMapPointMatches[i]);
//     + USLAM::PnPsolver* pSolver = new USLAM::PnPsolver(solvers, mCurrentFrame, vvpMapPointMatches[i]);    // solvers: a PnPsolverSet
//       pSolver->SetRansacParameters(0.99,10,300,4,0.5,5.991);
//       ...
//     - cv::Mat Tcw = pSolver->iterate(5,bNoMore,vbInliers,nInliers);            // per candidate, inside for(i) inside while(...)
//     + USLAM::PnPsolver::Tcw Tcw = pSolver->iterate(5,bNoMore,vbInliers,nInliers);   // the same, one device call per candidate
//   or, the loop of :2428-2517 up to the first pose as ONE device call over all candidates that are not discarded:
//     + int i = USLAM::IterateCandidates(solvers, vpPnPsolvers, vbDiscarded, nCandidates, 5, Tcw, vbInliers, nInliers);
//
// The frame type needs mvKeysUn (cv::KeyPoint layout), mvLevelSigma2, fx, fy, cx, cy; the map point type isBad() and GetWorldPos()
// returning something with at<float>(i) (cv::Mat) or operator[] -- see world_pos below.  The random stream: the reference draws from
// libc's rand(), never seeded; the set owns the restated generator (srand(1) at construction) and every iterate call advances it by
// exactly the draws the reference would have made, so solvers iterated in the reference's order see the reference's subsets.
// Header only, C++11, no OpenCV.
#ifndef UVO_COMPAT_PNPSOLVER_H_
#define UVO_COMPAT_PNPSOLVER_H_
#include <vector>

#include "uvo/uvo.h"

namespace USLAM {

// the set every PnPsolver of one relocalisation lives in, and the generator state they share (the process-wide rand() of the reference)
class PnPsolverSet {
 public:
  PnPsolverSet(uvo_klt* klt, int max_solvers, int max_points) : s_(0) {
    uvo_pnpsolver_set_create(klt, max_solvers, max_points, &s_);
    uvo_glibc_srand(&rng_, 1);
  }
  ~PnPsolverSet() { uvo_pnpsolver_set_destroy(s_); }
  bool ok() const { return s_ != 0; }
  void clear() {  // a new relocalisation: forget the solvers, keep the stream
    if (s_) uvo_pnpsolver_set_clear(s_);
  }
  uvo_pnpsolver_set* handle() { return s_; }
  uvo_glibc_rand* rng() { return &rng_; }

 private:
  PnPsolverSet(const PnPsolverSet&);
  PnPsolverSet& operator=(const PnPsolverSet&);
  uvo_pnpsolver_set* s_;
  uvo_glibc_rand rng_;
};

class PnPsolver {
 public:
  // what iterate() / find() return in place of cv::Mat: empty() or a row-major float 4 x 4
  struct Tcw {
    float m[16];
    bool valid;
    Tcw() : valid(false) {
      for (int i = 0; i < 16; ++i) m[i] = 0.f;
    }
    bool empty() const { return !valid; }
    float at(int r, int c) const { return m[4 * r + c]; }
    const float* data() const { return m; }
  };

  // PnPsolver::PnPsolver(F, vpMapPointMatches), :68-111
  template <class Frame, class MapPointPtr>
  PnPsolver(PnPsolverSet& set, const Frame& F, const std::vector<MapPointPtr>& vpMapPointMatches)
      : set_(&set), id_(-1), n_matches_((int)vpMapPointMatches.size()), fx_(F.fx), fy_(F.fy), cx_(F.cx), cy_(F.cy) {
    static_assert(sizeof(F.mvKeysUn[0]) == sizeof(uvo_keypoint), "keypoint layout must be cv::KeyPoint");
    for (size_t i = 0, iend = vpMapPointMatches.size(); i < iend; i++) {
      const MapPointPtr& pMP = vpMapPointMatches[i];
      if (!pMP || pMP->isBad()) continue;
      const uvo_keypoint& kp = reinterpret_cast<const uvo_keypoint&>(F.mvKeysUn[i]);
      p2d_.push_back(kp.x), p2d_.push_back(kp.y);
      sigma2_.push_back(F.mvLevelSigma2[kp.octave]);
      float X[3];
      world_pos(pMP->GetWorldPos(), X);
      p3d_.insert(p3d_.end(), X, X + 3);
      kp_index_.push_back((int32_t)i);
    }
    SetRansacParameters();
  }

  // Takes effect until the solver first iterates: the library derives nMinInliers, mRansacMaxIts and mvMaxError when the solver joins
  // its set (the reference's caller sets parameters once, right after construction).
  void SetRansacParameters(double probability = 0.99, int minInliers = 8, int maxIterations = 300, int minSet = 4, float epsilon = 0.4f,
                           float th2 = 5.991f) {
    prm_.probability = probability, prm_.min_inliers = minInliers, prm_.max_iterations = maxIterations, prm_.min_set = minSet;
    prm_.epsilon = epsilon, prm_.th2 = th2;
  }

  Tcw find(std::vector<bool>& vbInliers, int& nInliers) {
    bool bFlag;
    uvo_pnpsolver_info info;
    if (!join() || uvo_pnpsolver_query(set_->handle(), id_, &info) != UVO_OK) return none(vbInliers, nInliers);
    return iterate(info.max_its, bFlag, vbInliers, nInliers);
  }

  Tcw iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers) {
    bNoMore = false;
    if (!join()) return none(vbInliers, nInliers);
    const int32_t id = id_;
    uvo_pnpsolver_status st = {0, 0, 0};
    std::vector<uint8_t> mask(n_matches_ > 0 ? n_matches_ : 1);
    uvo_pnpsolver_result r = uvo_pnpsolver_result();
    r.status = &st, r.inliers = &mask[0], r.inliers_cap = (int32_t)mask.size();
    if (uvo_pnpsolver_iterate(set_->handle(), &id, 1, nIterations, set_->rng(), &r) != UVO_OK) return none(vbInliers, nInliers);
    bNoMore = st.no_more != 0;
    return unpack(r, mask, vbInliers, nInliers);
  }

  int id() {  // the solver's id in its set (joins it if need be), -1 on failure
    return join() ? id_ : -1;
  }
  int n_matches() const { return n_matches_; }

  static Tcw unpack(const uvo_pnpsolver_result& r, const std::vector<uint8_t>& mask, std::vector<bool>& vbInliers, int& nInliers) {
    if (r.returned < 0) return none(vbInliers, nInliers);
    Tcw T;
    T.valid = true;
    for (int i = 0; i < 16; ++i) T.m[i] = r.Tcw[i];
    nInliers = r.n_inliers;
    vbInliers.assign(mask.begin(), mask.end());
    return T;
  }

 private:
  static Tcw none(std::vector<bool>& vbInliers, int& nInliers) {
    vbInliers.clear();
    nInliers = 0;
    return Tcw();
  }
  bool join() {
    if (id_ >= 0) return true;
    if (!set_->ok()) return false;
    int id = -1;
    const int n = (int)kp_index_.size();
    if (uvo_pnpsolver_add(set_->handle(), n ? &p3d_[0] : 0, n ? &p2d_[0] : 0, n ? &sigma2_[0] : 0, n ? &kp_index_[0] : 0, n, n_matches_, fx_, fy_, cx_,
                          cy_, &prm_, &id) != UVO_OK)
      return false;
    id_ = id;
    return true;
  }
  // cv::Mat (3 x 1 float) or anything indexable
  template <class M>
  static auto world_pos(const M& p, float* X) -> decltype(p.template at<float>(0), void()) {
    X[0] = p.template at<float>(0), X[1] = p.template at<float>(1), X[2] = p.template at<float>(2);
  }
  template <class M>
  static auto world_pos(const M& p, float* X) -> decltype(p[0], void()) {
    X[0] = p[0], X[1] = p[1], X[2] = p[2];
  }

  PnPsolverSet* set_;
  int id_, n_matches_;
  float fx_, fy_, cx_, cy_;
  uvo_pnpsolver_params prm_;
  std::vector<float> p3d_, p2d_, sigma2_;
  std::vector<int32_t> kp_index_;
};

// The loop of Tracking::Relocalisation :2428-2517 up to its first pose, as one library call: iterate(nIterations) on every candidate
// that is not discarded, in order, until one returns a non-empty Tcw.  Candidates that report bNoMore are discarded and counted off
// nCandidates exactly as :2444-2448 does; candidates behind the returning one are not touched.  Returns the index of the candidate
// that returned (Tcw, vbInliers, nInliers are its), or -1: then every remaining candidate has run nIterations more and the caller's
// while(nCandidates>0 && !bMatch) goes round again.  vpPnPsolvers[i] may be null where vbDiscarded[i] is set.
inline int IterateCandidates(PnPsolverSet& set, const std::vector<PnPsolver*>& vpPnPsolvers, std::vector<bool>& vbDiscarded, int& nCandidates,
                             int nIterations, PnPsolver::Tcw& Tcw, std::vector<bool>& vbInliers, int& nInliers) {
  std::vector<int32_t> ids, which;
  size_t cap = 1;
  for (size_t i = 0; i < vpPnPsolvers.size(); i++) {
    if (vbDiscarded[i] || !vpPnPsolvers[i]) continue;
    const int id = vpPnPsolvers[i]->id();
    if (id < 0) continue;
    ids.push_back(id), which.push_back((int32_t)i);
    if ((size_t)vpPnPsolvers[i]->n_matches() > cap) cap = (size_t)vpPnPsolvers[i]->n_matches();
  }
  Tcw = PnPsolver::Tcw();
  vbInliers.clear();
  nInliers = 0;
  if (ids.empty()) return -1;
  std::vector<uvo_pnpsolver_status> st(ids.size());
  std::vector<uint8_t> mask(cap);
  uvo_pnpsolver_result r = uvo_pnpsolver_result();
  r.status = &st[0], r.inliers = &mask[0], r.inliers_cap = (int32_t)cap;
  if (uvo_pnpsolver_iterate(set.handle(), &ids[0], (int)ids.size(), nIterations, set.rng(), &r) != UVO_OK) return -1;
  for (size_t j = 0; j < ids.size(); j++)
    if (st[j].touched && st[j].no_more) {
      vbDiscarded[which[j]] = true;
      nCandidates--;
    }
  if (r.returned < 0) return -1;
  mask.resize(vpPnPsolvers[which[r.returned]]->n_matches());
  Tcw = PnPsolver::unpack(r, mask, vbInliers, nInliers);
  return which[r.returned];
}

}  // namespace USLAM
#endif  // UVO_COMPAT_PNPSOLVER_H_
