// USLAM::Sim3Solver (include/Sim3Solver.h, src/Sim3Solver.cc) over the C ABI's solver sets (uvo_sim3solver_* in uvo/uvo.h), for the one
// place the reference uses it: LoopClosing::ComputeSim3, src/LoopClosing.cc:373-479.
//
//     - Sim3Solver* pSolver = new Sim3Solver(mpCurrentKF,pKF,vvpMapPointMatches[i]);
//     + USLAM::Sim3Solver* pSolver = new USLAM::Sim3Solver(solvers,mpCurrentKF,pKF,vvpMapPointMatches[i]);    // solvers: a Sim3SolverSet
//       pSolver->SetRansacParameters(0.99,2,300);
//       ...
//     - cv::Mat Scm = pSolver->iterate(5,bNoMore,vbInliers,nInliers);             // per candidate, inside for(i) inside while(...)
//     + USLAM::Sim3Solver::T12 Scm = pSolver->iterate(5,bNoMore,vbInliers,nInliers);   // the same, one device call per candidate
//   or, the for(i) of :423-478 from candidate `first` up to the first transform as ONE device call:
//     + int i = USLAM::IterateCandidates(solvers, vpSim3Solvers, vbDiscarded, nCandidates, first, 5, Scm, vbInliers, nInliers);
//
// The key frame type needs GetMapPointMatches(), GetRotation(), GetTranslation(), GetCalibrationMatrix(), GetKeyPointUn(i) (cv::KeyPoint
// layout) and GetSigma2(octave); the map point type isBad(), GetIndexInKeyFrame(pKF) and GetWorldPos().  Matrices and vectors may be
// cv::Mat (at<float>) or anything indexable row-major with operator[] -- see el() below.  The random stream: the reference draws from
// libc's rand(), never seeded; the set owns the restated generator (srand(1) at construction) and every iterate call advances it by
// exactly the draws the reference would have made.  GetEstimatedRotation / Translation / Scale give the transform of the solver's last
// call that returned one (in the reference they also move with every new best of a call that returns nothing, which ComputeSim3 never
// reads).  Header only, C++11, no OpenCV.
#ifndef UVO_COMPAT_SIM3SOLVER_H_
#define UVO_COMPAT_SIM3SOLVER_H_
#include <vector>

#include "uvo/uvo.h"

namespace USLAM {

// the set every Sim3Solver of one ComputeSim3 lives in, and the generator state they share (the process-wide rand() of the reference)
class Sim3SolverSet {
 public:
  Sim3SolverSet(uvo_matcher* matcher, int max_solvers, int max_points) : s_(0) {
    uvo_sim3solver_set_create(matcher, max_solvers, max_points, &s_);
    uvo_glibc_srand(&rng_, 1);
  }
  ~Sim3SolverSet() { uvo_sim3solver_set_destroy(s_); }
  bool ok() const { return s_ != 0; }
  void clear() {  // a new ComputeSim3: forget the solvers, keep the stream
    if (s_) uvo_sim3solver_set_clear(s_);
  }
  uvo_sim3solver_set* handle() { return s_; }
  uvo_glibc_rand* rng() { return &rng_; }

 private:
  Sim3SolverSet(const Sim3SolverSet&);
  Sim3SolverSet& operator=(const Sim3SolverSet&);
  uvo_sim3solver_set* s_;
  uvo_glibc_rand rng_;
};

class Sim3Solver {
 public:
  // what the members return in place of cv::Mat: empty() or row-major floats
  template <int R, int C>
  struct Mat {
    float m[R * C];
    bool valid;
    Mat() : valid(false) {
      for (int i = 0; i < R * C; ++i) m[i] = 0.f;
    }
    bool empty() const { return !valid; }
    float at(int r, int c = 0) const { return m[C * r + c]; }
    const float* data() const { return m; }
  };
  typedef Mat<4, 4> T12;
  typedef Mat<3, 3> Rotation;
  typedef Mat<3, 1> Translation;

  // Sim3Solver::Sim3Solver(pKF1, pKF2, vpMatched12), :37-112
  template <class KeyFramePtr, class MapPointPtr>
  Sim3Solver(Sim3SolverSet& set, KeyFramePtr pKF1, KeyFramePtr pKF2, const std::vector<MapPointPtr>& vpMatched12)
      : set_(&set), id_(-1), n_matches_((int)vpMatched12.size()), scale_(0.f) {
    const std::vector<MapPointPtr> vpKeyFrameMP1 = pKF1->GetMapPointMatches();
    for (int i1 = 0; i1 < n_matches_; i1++) {
      if (!vpMatched12[i1]) continue;
      const MapPointPtr& pMP1 = vpKeyFrameMP1[i1];
      const MapPointPtr& pMP2 = vpMatched12[i1];
      if (!pMP1) continue;
      if (pMP1->isBad() || pMP2->isBad()) continue;
      const int indexKF1 = pMP1->GetIndexInKeyFrame(pKF1);
      const int indexKF2 = pMP2->GetIndexInKeyFrame(pKF2);
      if (indexKF1 < 0 || indexKF2 < 0) continue;
      static_assert(sizeof(pKF1->GetKeyPointUn(0)) == sizeof(uvo_keypoint), "keypoint layout must be cv::KeyPoint");
      const auto& kp1 = pKF1->GetKeyPointUn(indexKF1);
      const auto& kp2 = pKF2->GetKeyPointUn(indexKF2);
      sigma2_1_.push_back(pKF1->GetSigma2(reinterpret_cast<const uvo_keypoint&>(kp1).octave));
      sigma2_2_.push_back(pKF2->GetSigma2(reinterpret_cast<const uvo_keypoint&>(kp2).octave));
      const auto X1 = pMP1->GetWorldPos();
      const auto X2 = pMP2->GetWorldPos();
      for (int k = 0; k < 3; ++k) x1w_.push_back(el(X1, k, 0, 1)), x2w_.push_back(el(X2, k, 0, 1));
      index1_.push_back((int32_t)i1);
    }
    keyframe(pKF1, kf1_), keyframe(pKF2, kf2_);
    prm_.probability = 0.99, prm_.min_inliers = 6, prm_.max_iterations = 300;
  }

  // :114-138.  Before the solver first iterates it sets what the solver joins its set with; afterwards it is SetRansacParameters again:
  // mRansacMaxIts anew, mnIterations zeroed, the best kept.
  void SetRansacParameters(double probability = 0.99, int minInliers = 6, int maxIterations = 300) {
    prm_.probability = probability, prm_.min_inliers = minInliers, prm_.max_iterations = maxIterations;
    if (id_ >= 0) uvo_sim3solver_set_ransac_parameters(set_->handle(), id_, &prm_);
  }

  T12 find(std::vector<bool>& vbInliers12, int& nInliers) {
    uvo_sim3solver_info info;
    bool bFlag;
    if (!join() || uvo_sim3solver_query(set_->handle(), id_, &info) != UVO_OK) return none(vbInliers12, nInliers);
    return iterate(info.max_its, bFlag, vbInliers12, nInliers);
  }

  T12 iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers) {
    bNoMore = false;
    if (!join()) return none(vbInliers, nInliers);
    const int32_t id = id_;
    uvo_sim3solver_status st = {0, 0, 0};
    std::vector<uint8_t> mask(n_matches_ > 0 ? n_matches_ : 1);
    uvo_sim3solver_result r = uvo_sim3solver_result();
    r.status = &st, r.inliers = &mask[0], r.inliers_cap = (int32_t)mask.size();
    if (uvo_sim3solver_iterate(set_->handle(), &id, 1, nIterations, set_->rng(), &r) != UVO_OK) return none(vbInliers, nInliers);
    bNoMore = st.no_more != 0;
    mask.resize(n_matches_);
    return unpack(r, mask, vbInliers, nInliers);
  }

  Rotation GetEstimatedRotation() const { return R_; }
  Translation GetEstimatedTranslation() const { return t_; }
  float GetEstimatedScale() const { return scale_; }

  int id() {  // the solver's id in its set (joins it if need be), -1 on failure
    return join() ? id_ : -1;
  }
  int n_matches() const { return n_matches_; }

  // the result of a call in which this solver returned (or none did): its transform becomes the estimate
  T12 unpack(const uvo_sim3solver_result& r, const std::vector<uint8_t>& mask, std::vector<bool>& vbInliers, int& nInliers) {
    if (r.returned < 0) return none(vbInliers, nInliers);
    T12 T;
    T.valid = R_.valid = t_.valid = true;
    for (int i = 0; i < 16; ++i) T.m[i] = r.T12[i];
    for (int i = 0; i < 9; ++i) R_.m[i] = r.R12[i];
    for (int i = 0; i < 3; ++i) t_.m[i] = r.t12[i];
    scale_ = r.scale;
    nInliers = r.n_inliers;
    vbInliers.assign(mask.begin(), mask.end());
    return T;
  }

  static T12 none(std::vector<bool>& vbInliers, int& nInliers) {
    vbInliers.clear();
    nInliers = 0;
    return T12();
  }

 private:
  bool join() {
    if (id_ >= 0) return true;
    if (!set_->ok()) return false;
    int id = -1;
    const int n = (int)index1_.size();
    if (uvo_sim3solver_add(set_->handle(), n ? &x1w_[0] : 0, n ? &x2w_[0] : 0, n ? &sigma2_1_[0] : 0, n ? &sigma2_2_[0] : 0, n ? &index1_[0] : 0, n,
                           n_matches_, &kf1_, &kf2_, &prm_, &id) != UVO_OK)
      return false;
    id_ = id;
    return true;
  }
  // element (r, c) of a cv::Mat (float) or of anything indexable row-major with `cols` columns
  template <class M>
  static auto el(const M& p, int r, int c, int cols) -> decltype(p.template at<float>(0, 0), float()) {
    return cols == 1 ? p.template at<float>(r) : p.template at<float>(r, c);
  }
  template <class M>
  static auto el(const M& p, int r, int c, int cols) -> decltype(p[0], float()) {
    return p[cols * r + c];
  }
  template <class KeyFramePtr>
  static void keyframe(KeyFramePtr pKF, uvo_sim3_keyframe& kf) {
    const auto R = pKF->GetRotation();
    const auto t = pKF->GetTranslation();
    const auto K = pKF->GetCalibrationMatrix();
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) kf.Rcw[3 * r + c] = el(R, r, c, 3);
      kf.tcw[r] = el(t, r, 0, 1);
    }
    kf.fx = el(K, 0, 0, 3), kf.fy = el(K, 1, 1, 3), kf.cx = el(K, 0, 2, 3), kf.cy = el(K, 1, 2, 3);
  }

  Sim3SolverSet* set_;
  int id_, n_matches_;
  uvo_sim3_keyframe kf1_, kf2_;
  uvo_sim3solver_params prm_;
  std::vector<float> x1w_, x2w_, sigma2_1_, sigma2_2_;
  std::vector<int32_t> index1_;
  Rotation R_;
  Translation t_;
  float scale_;
};

// The for(i) of LoopClosing::ComputeSim3 :423-478 from candidate `first` up to its first transform, as one library call:
// iterate(nIterations) on every candidate from `first` on that is not discarded, in order, until one returns a transform.  Candidates
// that report bNoMore are discarded and counted off nCandidates exactly as :439-443 does; candidates behind the returning one are not
// touched.  Returns the index of the candidate that returned (Scm, vbInliers, nInliers are its, and its GetEstimated* are set), or -1:
// then the for(i) has run to its end.  The caller resumes at the returned index + 1 when OptimizeSim3 rejects the transform, and at 0
// for the next round of the while.  vpSim3Solvers[i] may be null where vbDiscarded[i] is set.
inline int IterateCandidates(Sim3SolverSet& set, const std::vector<Sim3Solver*>& vpSim3Solvers, std::vector<bool>& vbDiscarded, int& nCandidates,
                             int first, int nIterations, Sim3Solver::T12& Scm, std::vector<bool>& vbInliers, int& nInliers) {
  std::vector<int32_t> ids, which;
  size_t cap = 1;
  for (size_t i = first < 0 ? 0 : (size_t)first; i < vpSim3Solvers.size(); i++) {
    if (vbDiscarded[i] || !vpSim3Solvers[i]) continue;
    const int id = vpSim3Solvers[i]->id();
    if (id < 0) continue;
    ids.push_back(id), which.push_back((int32_t)i);
    if ((size_t)vpSim3Solvers[i]->n_matches() > cap) cap = (size_t)vpSim3Solvers[i]->n_matches();
  }
  Scm = Sim3Solver::none(vbInliers, nInliers);
  if (ids.empty()) return -1;
  std::vector<uvo_sim3solver_status> st(ids.size());
  std::vector<uint8_t> mask(cap);
  uvo_sim3solver_result r = uvo_sim3solver_result();
  r.status = &st[0], r.inliers = &mask[0], r.inliers_cap = (int32_t)cap;
  if (uvo_sim3solver_iterate(set.handle(), &ids[0], (int)ids.size(), nIterations, set.rng(), &r) != UVO_OK) return -1;
  for (size_t j = 0; j < ids.size(); j++)
    if (st[j].touched && st[j].no_more) {
      vbDiscarded[which[j]] = true;
      nCandidates--;
    }
  if (r.returned < 0) return -1;
  Sim3Solver* pSolver = vpSim3Solvers[which[r.returned]];
  mask.resize(pSolver->n_matches());
  Scm = pSolver->unpack(r, mask, vbInliers, nInliers);
  return which[r.returned];
}

}  // namespace USLAM
#endif  // UVO_COMPAT_SIM3SOLVER_H_
