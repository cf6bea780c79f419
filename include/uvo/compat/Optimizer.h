// Optimizer::PoseOptimization(Frame*) (include/Optimizer.h, src/Optimizer.cc:2012-2145: the vision-only overload) over the C ABI's
// pose optimizer (uvo_pose_* in uvo/uvo.h), for the places the tracker calls it: Tracking::TrackWithPnP (src/Tracking.cc:1884),
// TrackLocalMap (:1925), TrackwithMotionModel (:867) and Relocalisation (:2468, :2484, :2499).
//
//     - int nmatchesMap = Optimizer::PoseOptimization(&mCurrentFrame);
//     + int nmatchesMap = USLAM::Optimizer::PoseOptimization(poseopt, &mCurrentFrame);     // poseopt: a USLAM::PoseOptimizer
//
// With it none of these functions links g2o or Eigen.  The IMU overloads (:319, :779), OptimizeSim3 and the bundle adjustments stay
// with the reference's Optimizer.
//
// The frame type needs mvpMapPoints (pointers; null where there is no map point; GetWorldPos() returning something with at<float>(i)
// or operator[]), mvKeysUn (cv::KeyPoint layout), mvInvLevelSigma2, mvbOutlier (std::vector<bool> or anything indexable and
// assignable from bool), fx, fy, cx, cy, and the pose as 16 row-major floats reachable through pose_data(frame): the default looks for
// mTcw.ptr<float>() (cv::Mat, CV_32F, continuous) or a float mTcw[16]; overload USLAM::pose_data for anything else.
// The reference's effects are kept: mvbOutlier[i] = false for every index with a map point before the optimisation, the flags of the
// last round scattered back to those indices, indices without a map point untouched, the pose written, the count returned.
// MapPoint::mGlobalMutex is the caller's to hold around the call, as :2049 holds it around the gathering.
// Header only, C++11, no OpenCV.
#ifndef UVO_COMPAT_OPTIMIZER_H_
#define UVO_COMPAT_OPTIMIZER_H_
#include <vector>

#include "uvo/uvo.h"

namespace USLAM {

// the owner of the device set: one per tracker thread, sized for the most correspondences a frame can carry
class PoseOptimizer {
 public:
  PoseOptimizer(uvo_klt* klt, int max_points, int max_problems = 1) : o_(0) { uvo_pose_optimizer_create(klt, max_problems, max_points, &o_); }
  ~PoseOptimizer() { uvo_pose_optimizer_destroy(o_); }
  bool ok() const { return o_ != 0; }
  uvo_pose_optimizer* handle() { return o_; }
  // gathering buffers, kept between calls so that a call allocates nothing once they have grown
  std::vector<float> p3d, p2d, inv_sigma2;
  std::vector<int32_t> index;
  std::vector<uint8_t> outlier;

 private:
  PoseOptimizer(const PoseOptimizer&);
  PoseOptimizer& operator=(const PoseOptimizer&);
  uvo_pose_optimizer* o_;
};

namespace detail {
// cv::Mat (3 x 1 float) or anything indexable
template <class M>
auto world_pos(const M& p, float* X) -> decltype(p.template at<float>(0), void()) {
  X[0] = p.template at<float>(0), X[1] = p.template at<float>(1), X[2] = p.template at<float>(2);
}
template <class M>
auto world_pos(const M& p, float* X) -> decltype(p[0], void()) {
  X[0] = p[0], X[1] = p[1], X[2] = p[2];
}
template <class M>
auto mat_data(M& m, int) -> decltype(m.template ptr<float>()) {
  return m.template ptr<float>();
}
template <class M>
auto mat_data(M& m, long) -> decltype(&m[0]) {
  return &m[0];
}
}  // namespace detail

// the 16 row-major floats of the frame's pose
template <class Frame>
float* pose_data(Frame& F) {
  return detail::mat_data(F.mTcw, 0);
}

namespace Optimizer {

// int Optimizer::PoseOptimization(Frame* pFrame).  Returns nInitialCorrespondences - nBad, or -1 when the library call fails (the
// frame is then as the gathering left it: mvbOutlier cleared for the indices with a map point, the pose untouched).
template <class Frame>
int PoseOptimization(PoseOptimizer& opt, Frame* pFrame) {
  static_assert(sizeof(pFrame->mvKeysUn[0]) == sizeof(uvo_keypoint), "keypoint layout must be cv::KeyPoint");
  opt.p3d.clear(), opt.p2d.clear(), opt.inv_sigma2.clear(), opt.index.clear();
  const int N = (int)pFrame->mvpMapPoints.size();
  for (int i = 0; i < N; i++) {
    if (!pFrame->mvpMapPoints[i]) continue;
    float X[3];
    detail::world_pos(pFrame->mvpMapPoints[i]->GetWorldPos(), X);
    opt.p3d.insert(opt.p3d.end(), X, X + 3);
    pFrame->mvbOutlier[i] = false;
    const uvo_keypoint& kp = reinterpret_cast<const uvo_keypoint&>(pFrame->mvKeysUn[i]);
    opt.p2d.push_back(kp.x), opt.p2d.push_back(kp.y);
    opt.inv_sigma2.push_back(pFrame->mvInvLevelSigma2[kp.octave]);
    opt.index.push_back((int32_t)i);
  }
  const int n = (int)opt.index.size();
  if (!opt.ok()) return -1;
  opt.outlier.assign(n > 0 ? n : 1, 0);
  float* T = pose_data(*pFrame);
  uvo_pose_problem p = uvo_pose_problem();
  p.p3d = n ? &opt.p3d[0] : 0, p.p2d = n ? &opt.p2d[0] : 0, p.inv_sigma2 = n ? &opt.inv_sigma2[0] : 0, p.n = n;
  p.fx = pFrame->fx, p.fy = pFrame->fy, p.cx = pFrame->cx, p.cy = pFrame->cy;
  for (int e = 0; e < 16; ++e) p.Tcw[e] = T[e];
  uvo_pose_result r = uvo_pose_result();
  r.outlier = &opt.outlier[0], r.outlier_cap = (int32_t)opt.outlier.size();
  if (uvo_pose_optimize(opt.handle(), &p, 1, &r) != UVO_OK) return -1;
  for (int j = 0; j < n; ++j) pFrame->mvbOutlier[opt.index[j]] = opt.outlier[j] != 0;
  for (int e = 0; e < 16; ++e) T[e] = r.Tcw[e];
  return r.n_inliers;
}

}  // namespace Optimizer
}  // namespace USLAM
#endif  // UVO_COMPAT_OPTIMIZER_H_
