// Optimizer::PoseOptimization(Frame*) (include/Optimizer.h, src/Optimizer.cc:2012-2145: the vision-only overload) over the C ABI's
// pose optimizer (uvo_pose_* in uvo/uvo.h), for the places the tracker calls it: Tracking::TrackWithPnP (src/Tracking.cc:1884),
// TrackLocalMap (:1925), TrackwithMotionModel (:867) and Relocalisation (:2468, :2484, :2499).
//
//     - int nmatchesMap = Optimizer::PoseOptimization(&mCurrentFrame);
//     + int nmatchesMap = USLAM::Optimizer::PoseOptimization(poseopt, &mCurrentFrame);     // poseopt: a USLAM::PoseOptimizer
//
// With it none of these functions links g2o or Eigen.
//
// Optimizer::OptimizeSim3(pKF1, pKF2, vpMatches1, g2oS12, th2) (src/Optimizer.cc:2660-2856) over the C ABI's Sim3 optimizer
// (uvo_sim3_opt* in uvo/uvo.h), for LoopClosing::ComputeSim3 (src/LoopClosing.cc:463):
//
//     - g2o::Sim3 gScm(Converter::toMatrix3d(R), Converter::toVector3d(t), s);
//     - const int nInliers = Optimizer::OptimizeSim3(mpCurrentKF, pKF, vpMapPointMatches, gScm, 10);
//     + USLAM::Sim3 gScm(R.ptr<float>(), t.ptr<float>(), s);
//     + const int nInliers = USLAM::Optimizer::OptimizeSim3(sim3opt, mpCurrentKF, pKF, vpMapPointMatches, gScm, 10);  // a USLAM::Sim3Optimizer
//
// and an overload over the list of candidates that issues ONE device call; the caller takes the first candidate in order with
// nInliers >= 10.  With it the path from loop candidate to accepted loop links nothing of the reference's Optimizer.
// GlobalBundleAdjustmentNavState and the initialisation optimisers stay with the reference's Optimizer (the first has no caller).
//
// Optimizer::OptimizeEssentialGraph(pMap, pLoopKF, pCurKF, Scurw, NonCorrectedSim3, CorrectedSim3, LoopConnections)
// (src/Optimizer.cc:2409-2658, called at src/LoopClosing.cc:678) over the C ABI's essential graph (uvo_essential_graph_* in uvo/uvo.h):
//
//     - Optimizer::OptimizeEssentialGraph(mpMap, mpMatchedKF, mpCurrentKF, mg2oScw, NonCorrectedSim3, CorrectedSim3, LoopConnections);
//     + USLAM::Optimizer::OptimizeEssentialGraph(graph, mpMap, mpMatchedKF, mpCurrentKF, mScw, NonCorrectedSim3, CorrectedSim3, LoopConnections);
//
// graph: a USLAM::EssentialGraphOptimizer; KeyFrameAndPose: any std::map<KF*, USLAM::Sim3>.  It needs of the map GetAllKeyFrames() and
// GetAllMapPoints(); of the key-frame type mnId, isBad(), GetRotation(), GetTranslation(), GetParent(), GetLoopEdges() (a std::set<KF*>),
// GetCovisiblesByWeight(w), GetWeight(pKF), hasChild(pKF); of the map-point type isBad(), mnCorrectedByKF, mnCorrectedReference,
// GetReferenceKeyFrame(), GetWorldPos(), UpdateNormalAndDepth().  The reference's walk is kept (:2437-2598): the vertices are the key
// frames that are not bad, in ascending mnId (the order the envelope solver is given); the edges in the order of insertion -- those of
// LoopConnections in the map's and the sets' iteration order under the weight rule of :2489, then per key frame of GetAllKeyFrames()
// the parent edge, the loop edges to smaller ids and the covisibility edges of GetCovisiblesByWeight(100) under the conditions of
// :2574-2579 with the inserted-pairs set -- and its effects (:2605-2657): ba_set_pose with [R | t / s], ba_set_world_pos +
// UpdateNormalAndDepth() per map point that is not bad, nIDr chosen as :2635-2643 choose it.  Departures: a bad key frame is no vertex,
// and where the reference dereferences the null optimizer.vertex(id) for it the adaptor skips that edge or key frame; the normal-edge
// loop skips bad key frames; a point whose reference key frame is no vertex keeps its position (the reference maps it through two
// default-constructed similarities, the identity) and is still set and updated; on a failed library call, or when pLoopKF is no
// vertex, -1 is returned and nothing of the caller's is touched.  Scurw is taken and not read, as in the reference.
//
// The two IMU overloads of Optimizer::PoseOptimization (src/Optimizer.cc:779-1103 over a key frame, :319-777 over the last frame) over
// the C ABI's nav optimizer (uvo_nav_* in uvo/uvo.h), for Tracking::TrackWithIMU (src/Tracking.cc:1099, :1105), TrackLocalMapWithIMU
// (:1996, :2006) and IMU_Relocalisation (:3035):
//
//     - Optimizer::PoseOptimization(&mCurrentFrame, mpLastKeyFrame, imupreint, mpLocalMapper->GetGravityVec(), grot, true, d0, dcov);
//     + USLAM::Optimizer::PoseOptimization(navopt, navprm, &mCurrentFrame, mpLastKeyFrame, imupreint, mpLocalMapper->GetGravityVec(), grot, true, d0, dcov);
//
// navopt: a USLAM::NavOptimizer; navprm: a USLAM::NavParams, what the reference reads from statics (ConfigParam::GetEigTbc(),
// IMUData::getGyrBiasRW2() / getAccBiasRW2()).  The overload is chosen as the reference's is, by the type of the second argument: one
// with a member mNavStatePrior is a frame (30 unknowns, its correspondences and its prior enter), any other a key frame (15 unknowns).
// Needed of the frame type besides PoseOptimization(Frame*)'s members: GetNavState(), SetNavState(ns), mNavStatePrior, mMargCovInv
// ((i, j) access), mHas_depth, mDepth, mDepth_time, mTimeStamp; of the key frame GetNavState() and mTimeStamp; of NavState Get_P(),
// Get_V(), Get_R().unit_quaternion() (x(), y(), z(), w()), Get_RotMatrix(), Get_BiasGyr(), Get_BiasAcc(), Get_dBias_Gyr(),
// Get_dBias_Acc() ((i) access) and Set_Pos, Set_Vel, Set_Rot(SO3), Set_DeltaBiasGyr, Set_DeltaBiasAcc, the SO3 constructible from its
// quaternion type and that from (w, x, y, z); of the preintegration the getters of uvo_nav_problem's fields ((i), (i, j) access).
// The reference's effects are kept: mvbOutlier of BOTH frames cleared only where a map point exists and rewritten there; SetNavState
// with the recovered P, V, R and delta biases; the pose of UpdatePoseFromNS written through pose_data(frame); with bComputeMarg
// mMargCovInv and mNavStatePrior of the frame.  On the early return (fewer than 3 or 4 correspondences) 0 is returned and nothing but
// the cleared flags is changed.  The depth edge's information is 1 / cov1^2, cov1 = shi^2 depth_cov^2 + e3^T Rwb^T CovPos Rwb e3 with
// CovPos the 3 x 3 POSITION block of CovPVPhi: the reference writes block(0,0,2,2) into a 3 x 3 matrix there (:470, :913), which
// Eigen does not define.  grot is taken and not read, as in the reference.
//
// Optimizer::LocalBundleAdjustment(pKF, pbStopFlag, pMap, pLM) (src/Optimizer.cc:2147-2405, called at src/LocalMapping.cc:807) and
// Optimizer::BundleAdjustment / GlobalBundleAdjustemnt / RecoveryBundleAdjustemnt (:1879-2010, src/Tracking.cc:1480, :1807) over the C
// ABI's bundle adjuster (uvo_bundle_adjust* in uvo/uvo.h):
//
//     - Optimizer::LocalBundleAdjustment(mpCurrentKeyFrame, &mbAbortBA, mpMap, this);
//     + USLAM::Optimizer::LocalBundleAdjustment(mpCurrentKeyFrame, &mbAbortBA, mpMap, this, adjuster);   // a USLAM::BundleAdjuster
//
// They need of the key-frame type mnId, mnBALocalForKF, mnBAFixedForKF, isBad(), GetVectorCovisibleKeyFrames(), GetMapPointMatches(),
// GetRotation() and GetTranslation() (the floats of GetPose()), GetKeyPointUn(i), GetInvSigma2(octave), fx, fy, cx, cy,
// EraseMapPointMatch(pMP) and EraseMapPointMatch(idx); of the map-point type mnBALocalForKF, isBad(), GetObservations() (a
// std::map<KF*, size_t>), GetWorldPos(), EraseObservation(pKF), GetIndexInKeyFrame(pKF), UpdateNormalAndDepth(); of the map
// mMutexMapUpdate (lock() / unlock()), GetAllKeyFrames(), GetAllMapPoints(); of the local mapper SetMapUpdateFlagInTracking(bool).
// Poses and positions are written through USLAM::ba_set_pose(pKF, const float T[16]) and USLAM::ba_set_world_pos(pMP, const float
// X[3]), whose defaults call pKF->SetPose(T) and pMP->SetWorldPos(X) with the float pointers: a cv::Mat host overloads the two (wrap
// the floats in a cv::Mat header and clone).  The reference's effects are kept: the gathering of :2149-2198 with both marks, a
// point's edges in the order its GetObservations() iterates, the erasures of both checks, SetPose / SetWorldPos /
// UpdateNormalAndDepth and the map-update flag.  Departures: pbStopFlag is read once, before the call (1 is returned and nothing is
// optimised when it is set); the erasures of the first check and the write-back happen once, after the call and under
// mMutexMapUpdate, not in between the two rounds.
//
// Optimizer::LocalBundleAdjustmentNavState(pCurKF, lLocalKeyFrames, pbStopFlag, pMap, gw, grot, pLM, ini_depth, depth_cov, fixedKF_id)
// (src/Optimizer.cc:1105-1732, called at src/LocalMapping.cc:811 once the IMU is initialised) over the C ABI's nav bundle adjuster
// (uvo_nav_bundle_adjust* in uvo/uvo.h):
//
//     - Optimizer::LocalBundleAdjustmentNavState(mpCurrentKeyFrame, mlLocalKeyFrames, &mbAbortBA, mpMap, mGravityVec, grot, this, d0, dcov, fixed_id);
//     + USLAM::Optimizer::LocalBundleAdjustmentNavState(mpCurrentKeyFrame, mlLocalKeyFrames, &mbAbortBA, mpMap, mGravityVec, grot, this, d0, dcov, fixed_id,
//     +                                                 navprm, navadjuster);       // a USLAM::NavParams and a USLAM::NavBundleAdjuster
//
// It needs of the key-frame type, besides LocalBundleAdjustment's members: GetPrevKeyFrame(), GetNavState(), GetIMUPreInt() (the getters
// of uvo_nav_ba_link's fields), Depth_Vec and Depth_Vec_Time (size(), [i]), mTimeStamp, SetNavStatePos, SetNavStateVel, SetNavStateRot,
// SetNavStateDeltaBg, SetNavStateDeltaBa; of NavState what the IMU overloads of PoseOptimization need.  The local key frames come as any
// container with begin() / end() / front() / back().  The reference's effects are kept: the gathering of :1121-1182 with both marks (the
// key frame before the window first among the fixed ones), a point's edges in the order its GetObservations() iterates, per entry of
// Depth_Vec the forward edge when (t1 - td) < (td - t0), else the backward edge when minKFID + 1 < pKF0->mnId, else none; the erasures of
// the FINAL check only (EraseMapPointMatch(pMP), EraseObservation(pKF)), P, V, R and the delta biases set, the pose of UpdatePoseFromNS
// written through ba_set_pose, SetWorldPos / UpdateNormalAndDepth and the map-update flag, all under mMutexMapUpdate.  The depth entry's
// information is computed with the 3 x 3 position block, as for the pose overloads.  Departures: pbStopFlag is read once, before the
// call; -1 is returned, and nothing but the marks touched, when the window's first key frame has no previous key frame (the reference
// reads pKFPrevLocal->mnId before its null test at :1149), when that key frame is bad (the reference then looks up a vertex that is not
// there), or when the library call fails; a backward entry whose pKF_1 is not a key frame of the window is skipped (likewise).  grot is
// taken and not read.
//
// The frame type needs mvpMapPoints (pointers; null where there is no map point; GetWorldPos() returning something with at<float>(i)
// or operator[]), mvKeysUn (cv::KeyPoint layout), mvInvLevelSigma2, mvbOutlier (std::vector<bool> or anything indexable and
// assignable from bool), fx, fy, cx, cy, and the pose as 16 row-major floats reachable through pose_data(frame): the default looks for
// mTcw.ptr<float>() (cv::Mat, CV_32F, continuous) or a float mTcw[16]; overload USLAM::pose_data for anything else.
// The reference's effects are kept: mvbOutlier[i] = false for every index with a map point before the optimisation, the flags of the
// last round scattered back to those indices, indices without a map point untouched, the pose written, the count returned.
// MapPoint::mGlobalMutex is the caller's to hold around the call, as :2049 holds it around the gathering.
// OptimizeSim3 needs of the key-frame type GetRotation() and GetTranslation() (3 x 3 and 3 x 1 floats, at<float>(i) or operator[] in
// row-major order), fx, fy, cx, cy (the members GetCalibrationMatrix() is built from), GetMapPointMatches(), GetKeyPointUn(i)
// (cv::KeyPoint layout), GetInvSigma2(octave) and GetSigma2(octave); of the map-point type isBad(), GetWorldPos() and
// GetIndexInKeyFrame(pKF).  The reference's effects are kept: the walk of :2713-2792 (a match is skipped -- and its entry in vpMatches1
// LEFT AS IT IS -- when pMP1 is null, when either point is bad, or when i2 < 0); e12 weighted with pKF1->GetInvSigma2(octave1) and e21
// with pKF2->GetSigma2(octave2), the variance, as :2781 has it; vpMatches1[idx] nulled for every pair bad in either check; S12 written
// only when the second round ran, so on the early return (fewer than 10 pairs left: 0 is returned) it is untouched.
// Header only, C++11, no OpenCV.
#ifndef UVO_COMPAT_OPTIMIZER_H_
#define UVO_COMPAT_OPTIMIZER_H_
#include <algorithm>
#include <cmath>
#include <map>
#include <set>
#include <type_traits>
#include <utility>
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

// the owner of a nav optimizer set and of the gathering buffers of both frames
class NavOptimizer {
 public:
  NavOptimizer(uvo_klt* klt, int max_points, int max_problems = 1) : o_(0) { uvo_nav_optimizer_create(klt, max_problems, max_points, &o_); }
  ~NavOptimizer() { uvo_nav_optimizer_destroy(o_); }
  bool ok() const { return o_ != 0; }
  uvo_nav_optimizer* handle() { return o_; }
  struct Gathered {
    std::vector<float> p3d, p2d, inv_sigma2;
    std::vector<int32_t> index;
    std::vector<uint8_t> outlier;
  };
  Gathered cur, last;

 private:
  NavOptimizer(const NavOptimizer&);
  NavOptimizer& operator=(const NavOptimizer&);
  uvo_nav_optimizer* o_;
};

// what the reference's IMU overloads read from statics
struct NavParams {
  double Tbc[16];  // ConfigParam::GetEigTbc(), row-major
  double gyr_bias_rw2, acc_bias_rw2;  // IMUData::getGyrBiasRW2(), getAccBiasRW2()
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

// g2o::Sim3 as far as ComputeSim3 uses it: quaternion (x y z w, not normalised), translation and scale in double.  Built from the
// solver's floats as g2o::Sim3(Converter::toMatrix3d(R), Converter::toVector3d(t), s) is; those floats are what the optimiser starts
// from.  A Sim3 that is not built from floats (an optimised one, or one set by hand) starts from its own values rounded to float.
class Sim3 {
 public:
  struct Matrix3 {
    double m[9];  // row-major
    double operator()(int r, int c) const { return m[3 * r + c]; }
  };
  struct Vector3 {
    double v[3];
    double operator[](int i) const { return v[i]; }
  };
  Sim3() : s_(1.) { q_[0] = q_[1] = q_[2] = 0., q_[3] = 1., t_[0] = t_[1] = t_[2] = 0., sync(); }
  Sim3(const float* R, const float* t, float s) : s_(s) {
    for (int e = 0; e < 9; ++e) Rf_[e] = R[e];
    for (int e = 0; e < 3; ++e) tf_[e] = t[e], t_[e] = t[e];
    sf_ = s;
    // Eigen's Quaternion(Matrix3) on the widened matrix; the optimiser computes the same from the same floats
    const double m00 = R[0], m11 = R[4], m22 = R[8];
    double tr = m00 + m11 + m22;
    if (tr > 0.) {
      tr = std::sqrt(tr + 1.);
      q_[3] = 0.5 * tr, tr = 0.5 / tr;
      q_[0] = ((double)R[7] - R[5]) * tr, q_[1] = ((double)R[2] - R[6]) * tr, q_[2] = ((double)R[3] - R[1]) * tr;
    } else {
      int i = 0;
      if (m11 > m00) i = 1;
      if (m22 > (double)R[4 * i]) i = 2;
      const int j = (i + 1) % 3, k = (j + 1) % 3;
      tr = std::sqrt((double)R[4 * i] - R[4 * j] - R[4 * k] + 1.);
      q_[i] = 0.5 * tr, tr = 0.5 / tr;
      q_[3] = ((double)R[3 * k + j] - R[3 * j + k]) * tr;
      q_[j] = ((double)R[3 * j + i] + R[3 * i + j]) * tr;
      q_[k] = ((double)R[3 * k + i] + R[3 * i + k]) * tr;
    }
  }
  Sim3(const double* q_xyzw, const double* t, double s) : s_(s) {
    for (int e = 0; e < 4; ++e) q_[e] = q_xyzw[e];
    for (int e = 0; e < 3; ++e) t_[e] = t[e];
    sync();
  }
  // Eigen's toRotationMatrix
  Matrix3 rotation_matrix() const {
    Matrix3 R;
    const double tx = 2. * q_[0], ty = 2. * q_[1], tz = 2. * q_[2];
    const double twx = tx * q_[3], twy = ty * q_[3], twz = tz * q_[3], txx = tx * q_[0], txy = ty * q_[0], txz = tz * q_[0];
    const double tyy = ty * q_[1], tyz = tz * q_[1], tzz = tz * q_[2];
    R.m[0] = 1. - (tyy + tzz), R.m[1] = txy - twz, R.m[2] = txz + twy;
    R.m[3] = txy + twz, R.m[4] = 1. - (txx + tzz), R.m[5] = tyz - twx;
    R.m[6] = txz - twy, R.m[7] = tyz + twx, R.m[8] = 1. - (txx + tyy);
    return R;
  }
  Vector3 translation() const {
    Vector3 t;
    t.v[0] = t_[0], t.v[1] = t_[1], t.v[2] = t_[2];
    return t;
  }
  double scale() const { return s_; }
  const double* quaternion() const { return q_; }  // x y z w
  // what the optimiser starts from
  const float* start_rotation() const { return Rf_; }
  const float* start_translation() const { return tf_; }
  float start_scale() const { return sf_; }

 private:
  void sync() {
    const Matrix3 R = rotation_matrix();
    for (int e = 0; e < 9; ++e) Rf_[e] = (float)R.m[e];
    for (int e = 0; e < 3; ++e) tf_[e] = (float)t_[e];
    sf_ = (float)s_;
  }
  double q_[4], t_[3], s_;
  float Rf_[9], tf_[3], sf_;
};

// the owner of the device set: one on the loop-closing thread's matcher handle, sized for the candidates of one ComputeSim3 and the most
// matches a key frame can carry
class Sim3Optimizer {
 public:
  // the sizes in the order of uvo_sim3_optimizer_create and of the Python class: problems first, then pairs
  Sim3Optimizer(uvo_matcher* m, int max_problems, int max_pairs) : o_(0) { uvo_sim3_optimizer_create(m, max_problems, max_pairs, &o_); }
  ~Sim3Optimizer() { uvo_sim3_optimizer_destroy(o_); }
  bool ok() const { return o_ != 0; }
  uvo_sim3_optimizer* handle() { return o_; }
  // gathering buffers of all problems of a call, kept between calls so that a call allocates nothing once they have grown
  std::vector<float> x1w, x2w, obs1, obs2, info1, info2;
  std::vector<int32_t> index;    // vnIndexEdge
  std::vector<int32_t> offset;   // first pair of each problem, and the total
  std::vector<uint8_t> removed;
  std::vector<uvo_sim3_opt_problem> problems;
  std::vector<uvo_sim3_opt_result> results;

 private:
  Sim3Optimizer(const Sim3Optimizer&);
  Sim3Optimizer& operator=(const Sim3Optimizer&);
  uvo_sim3_optimizer* o_;
};

namespace detail {
template <class M>
auto mat_elem(const M& m, int i, int) -> decltype(m.template at<float>(i)) {
  return m.template at<float>(i);
}
template <class M>
auto mat_elem(const M& m, int i, long) -> decltype(m[i] + 0.f) {
  return m[i];
}
template <class KF>
void keyframe_of(KF* pKF, uvo_sim3_keyframe& k) {
  const auto R = pKF->GetRotation();
  const auto t = pKF->GetTranslation();
  for (int e = 0; e < 9; ++e) k.Rcw[e] = mat_elem(R, e, 0);
  for (int e = 0; e < 3; ++e) k.tcw[e] = mat_elem(t, e, 0);
  k.fx = pKF->fx, k.fy = pKF->fy, k.cx = pKF->cx, k.cy = pKF->cy;
}
// :2713-2792: the pairs of one candidate appended to the buffers
template <class KF, class MP>
void gather_sim3(Sim3Optimizer& opt, KF* pKF1, KF* pKF2, const std::vector<MP*>& vpMatches1) {
  const int N = (int)vpMatches1.size();
  const std::vector<MP*> vpMapPoints1 = pKF1->GetMapPointMatches();
  for (int i = 0; i < N; i++) {
    if (!vpMatches1[i]) continue;
    MP* pMP1 = vpMapPoints1[i];
    MP* pMP2 = vpMatches1[i];
    const int i2 = pMP2->GetIndexInKeyFrame(pKF2);
    if (!(pMP1 && pMP2)) continue;
    if (!(!pMP1->isBad() && !pMP2->isBad() && i2 >= 0)) continue;
    float X[3];
    world_pos(pMP1->GetWorldPos(), X);
    opt.x1w.insert(opt.x1w.end(), X, X + 3);
    world_pos(pMP2->GetWorldPos(), X);
    opt.x2w.insert(opt.x2w.end(), X, X + 3);
    const auto kp1 = pKF1->GetKeyPointUn(i);
    const auto kp2 = pKF2->GetKeyPointUn(i2);
    static_assert(sizeof(kp1) == sizeof(uvo_keypoint), "keypoint layout must be cv::KeyPoint");
    const uvo_keypoint& k1 = reinterpret_cast<const uvo_keypoint&>(kp1);
    const uvo_keypoint& k2 = reinterpret_cast<const uvo_keypoint&>(kp2);
    opt.obs1.push_back(k1.x), opt.obs1.push_back(k1.y);
    opt.obs2.push_back(k2.x), opt.obs2.push_back(k2.y);
    opt.info1.push_back(pKF1->GetInvSigma2(k1.octave));
    opt.info2.push_back(pKF2->GetSigma2(k2.octave));  // :2781: the variance, as the reference passes it
    opt.index.push_back((int32_t)i);
  }
}
}  // namespace detail

// the owner of the device adjuster: one on the mapping thread's matcher handle
class BundleAdjuster {
 public:
  BundleAdjuster(uvo_matcher* m, int max_free, int max_fixed, int max_points, int max_edges) : a_(0) {
    uvo_bundle_adjuster_create(m, max_free, max_fixed, max_points, max_edges, &a_);
  }
  ~BundleAdjuster() { uvo_bundle_adjuster_destroy(a_); }
  bool ok() const { return a_ != 0; }
  uvo_bundle_adjuster* handle() { return a_; }
  // gathering buffers, kept between calls so that a call allocates nothing once they have grown
  std::vector<float> Tcw, points, obs, inv_sigma2, cameras, Tcw_out, points_out;
  std::vector<uint8_t> fixed, point_bad, removed1, removed2;
  std::vector<int32_t> begin, edge_kf, edge_camera, edge_index;  // edge_index: the observation's index in its key frame
  uvo_ba_result result;                                          // of the last call: counts, iterations, trials

 private:
  BundleAdjuster(const BundleAdjuster&);
  BundleAdjuster& operator=(const BundleAdjuster&);
  uvo_bundle_adjuster* a_;
};

template <class KF>
void ba_set_pose(KF* pKF, const float T[16]) {
  pKF->SetPose(T);
}
template <class MP>
void ba_set_world_pos(MP* pMP, const float X[3]) {
  pMP->SetWorldPos(X);
}

namespace detail {
template <class M>
struct LockGuard {
  explicit LockGuard(M& m) : m_(m) { m_.lock(); }
  ~LockGuard() { m_.unlock(); }
  M& m_;
};
inline void ba_clear(BundleAdjuster& a) {
  a.Tcw.clear(), a.points.clear(), a.obs.clear(), a.inv_sigma2.clear(), a.cameras.clear(), a.fixed.clear(), a.point_bad.clear();
  a.begin.assign(1, 0), a.edge_kf.clear(), a.edge_camera.clear(), a.edge_index.clear();
}
template <class KF>
void ba_add_keyframe(BundleAdjuster& a, KF* pKF, bool fixed) {
  const auto R = pKF->GetRotation();
  const auto t = pKF->GetTranslation();
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) a.Tcw.push_back(mat_elem(R, 3 * r + c, 0));
    a.Tcw.push_back(mat_elem(t, r, 0));
  }
  a.fixed.push_back(fixed ? 1 : 0);
}
template <class KF>
int ba_camera(BundleAdjuster& a, KF* pKF) {
  const float k[4] = {(float)pKF->fx, (float)pKF->fy, (float)pKF->cx, (float)pKF->cy};
  const int n = (int)a.cameras.size() / 4;
  for (int i = 0; i < n; ++i)
    if (a.cameras[4 * i] == k[0] && a.cameras[4 * i + 1] == k[1] && a.cameras[4 * i + 2] == k[2] && a.cameras[4 * i + 3] == k[3]) return i;
  a.cameras.insert(a.cameras.end(), k, k + 4);
  return n;
}
// a point and its edges (:2261-2307, :1934-1978): the observations in the order GetObservations() iterates, those of bad key frames and
// of key frames that are no vertex skipped.  edge_kfs receives the key frame of every edge.
template <class KF, class MP>
void ba_add_point(BundleAdjuster& a, MP* pMP, const std::vector<KF*>& vertices, std::vector<KF*>& edge_kfs) {
  float X[3];
  world_pos(pMP->GetWorldPos(), X);
  a.points.insert(a.points.end(), X, X + 3);
  a.point_bad.push_back(pMP->isBad() ? 1 : 0);
  const auto observations = pMP->GetObservations();
  for (auto mit = observations.begin(); mit != observations.end(); ++mit) {
    KF* pKFi = mit->first;
    if (pKFi->isBad()) continue;
    int k = -1;
    for (size_t v = 0; v < vertices.size() && k < 0; ++v)
      if (vertices[v] == pKFi) k = (int)v;
    if (k < 0) continue;
    const auto kp = pKFi->GetKeyPointUn(mit->second);
    static_assert(sizeof(kp) == sizeof(uvo_keypoint), "keypoint layout must be cv::KeyPoint");
    const uvo_keypoint& u = reinterpret_cast<const uvo_keypoint&>(kp);
    a.edge_kf.push_back(k), a.obs.push_back(u.x), a.obs.push_back(u.y);
    a.inv_sigma2.push_back(pKFi->GetInvSigma2(u.octave));
    a.edge_camera.push_back(ba_camera(a, pKFi));
    a.edge_index.push_back((int32_t)mit->second);
    edge_kfs.push_back(pKFi);
  }
  a.begin.push_back((int32_t)a.edge_kf.size());
}
inline int ba_call(BundleAdjuster& a, int mode, int n_iterations) {
  const size_t K = a.fixed.size(), P = a.point_bad.size(), E = a.edge_kf.size();
  a.Tcw_out.assign(16 * K + 1, 0.f), a.points_out.assign(3 * P + 1, 0.f), a.removed1.assign(E + 1, 0), a.removed2.assign(E + 1, 0);
  a.Tcw.push_back(0.f), a.points.push_back(0.f), a.obs.push_back(0.f), a.inv_sigma2.push_back(0.f), a.cameras.push_back(0.f);
  a.fixed.push_back(0), a.point_bad.push_back(0), a.edge_kf.push_back(0), a.edge_camera.push_back(0);  // no empty vector is indexed
  uvo_ba_problem q = uvo_ba_problem();
  q.mode = mode, q.n_iterations = n_iterations;
  q.n_keyframes = (int32_t)K, q.n_points = (int32_t)P, q.n_edges = (int32_t)E, q.n_cameras = (int32_t)(a.cameras.size() / 4);
  q.kf_Tcw = &a.Tcw[0], q.kf_fixed = &a.fixed[0], q.points = &a.points[0], q.point_bad = &a.point_bad[0], q.point_edge_begin = &a.begin[0];
  q.edge_kf = &a.edge_kf[0], q.edge_obs = &a.obs[0], q.edge_inv_sigma2 = &a.inv_sigma2[0], q.edge_camera = &a.edge_camera[0], q.cameras = &a.cameras[0];
  a.result = uvo_ba_result();
  a.result.kf_Tcw = &a.Tcw_out[0], a.result.points = &a.points_out[0], a.result.removed1 = &a.removed1[0], a.result.removed2 = &a.removed2[0];
  return a.ok() && uvo_bundle_adjust(a.handle(), &q, &a.result) == UVO_OK ? 0 : -1;
}
}  // namespace detail

namespace Optimizer {

// The candidates of one ComputeSim3 in ONE device call: candidate j is (pKF1, vpKF2[j], vvpMatches1[j], vS12[j]); vnInliers[j] is what
// the reference's OptimizeSim3 returns for it.  Every candidate is treated as the single call treats it: its matches nulled, its S12
// written unless it returned early.  Returns 0, or -1 when the library call fails (nothing of the caller's is then touched, vnInliers
// included).
template <class KF, class MP>
int OptimizeSim3(Sim3Optimizer& opt, KF* pKF1, const std::vector<KF*>& vpKF2, std::vector<std::vector<MP*> >& vvpMatches1, std::vector<Sim3>& vS12,
                 float th2, std::vector<int>& vnInliers) {
  const int P = (int)vpKF2.size();
  if (!opt.ok() || (int)vvpMatches1.size() != P || (int)vS12.size() != P) return -1;
  opt.x1w.clear(), opt.x2w.clear(), opt.obs1.clear(), opt.obs2.clear(), opt.info1.clear(), opt.info2.clear(), opt.index.clear(), opt.offset.clear();
  for (int j = 0; j < P; ++j) {
    opt.offset.push_back((int32_t)opt.index.size());
    detail::gather_sim3(opt, pKF1, vpKF2[j], vvpMatches1[j]);
  }
  opt.offset.push_back((int32_t)opt.index.size());
  opt.removed.assign(opt.index.size() + 1, 0);
  opt.problems.assign(P, uvo_sim3_opt_problem());
  opt.results.assign(P, uvo_sim3_opt_result());
  for (int j = 0; j < P; ++j) {
    uvo_sim3_opt_problem& p = opt.problems[j];
    const int off = opt.offset[j], n = opt.offset[j + 1] - off;
    p.n = n, p.th2 = th2;
    if (n) {
      p.x1w = &opt.x1w[3 * off], p.x2w = &opt.x2w[3 * off], p.obs1 = &opt.obs1[2 * off], p.obs2 = &opt.obs2[2 * off];
      p.info1 = &opt.info1[off], p.info2 = &opt.info2[off];
    }
    detail::keyframe_of(pKF1, p.kf1);
    detail::keyframe_of(vpKF2[j], p.kf2);
    for (int e = 0; e < 9; ++e) p.R12[e] = vS12[j].start_rotation()[e];
    for (int e = 0; e < 3; ++e) p.t12[e] = vS12[j].start_translation()[e];
    p.s12 = vS12[j].start_scale();
    opt.results[j].removed = &opt.removed[off], opt.results[j].removed_cap = n;
  }
  if (P > 0 && uvo_sim3_optimize(opt.handle(), &opt.problems[0], P, &opt.results[0]) != UVO_OK) return -1;
  vnInliers.assign(P, 0);
  for (int j = 0; j < P; ++j) {
    const uvo_sim3_opt_result& r = opt.results[j];
    const int off = opt.offset[j], n = opt.offset[j + 1] - off;
    for (int e = 0; e < n; ++e)
      if (opt.removed[off + e]) vvpMatches1[j][opt.index[off + e]] = static_cast<MP*>(0);
    if (r.more_iterations != 0) vS12[j] = Sim3(r.q, r.t, r.s);  // the early return runs no second round and leaves g2oS12 as it was
    vnInliers[j] = r.n_inliers;
  }
  return 0;
}

// int Optimizer::OptimizeSim3(KeyFrame* pKF1, KeyFrame* pKF2, vector<MapPoint*>& vpMatches1, g2o::Sim3& g2oS12, float th2).  Returns
// nIn, 0 on the early return, or -1 when the library call fails (nothing is then touched).
template <class KF, class MP>
int OptimizeSim3(Sim3Optimizer& opt, KF* pKF1, KF* pKF2, std::vector<MP*>& vpMatches1, Sim3& S12, float th2) {
  std::vector<KF*> kfs(1, pKF2);
  std::vector<std::vector<MP*> > matches(1);
  matches[0].swap(vpMatches1);
  std::vector<Sim3> sims(1, S12);
  std::vector<int> inl;
  const int rc = OptimizeSim3(opt, pKF1, kfs, matches, sims, th2, inl);
  vpMatches1.swap(matches[0]);
  if (rc != 0) return -1;
  S12 = sims[0];
  return inl[0];
}


}  // namespace Optimizer

namespace detail {
template <class NS>
void nav_state_of(const NS& ns, uvo_nav_state& s) {
  for (int i = 0; i < 3; ++i) {
    s.P[i] = ns.Get_P()(i), s.V[i] = ns.Get_V()(i), s.bg[i] = ns.Get_BiasGyr()(i), s.ba[i] = ns.Get_BiasAcc()(i);
    s.dbg[i] = ns.Get_dBias_Gyr()(i), s.dba[i] = ns.Get_dBias_Acc()(i);
  }
  s.q[0] = ns.Get_R().unit_quaternion().x(), s.q[1] = ns.Get_R().unit_quaternion().y(), s.q[2] = ns.Get_R().unit_quaternion().z();
  s.q[3] = ns.Get_R().unit_quaternion().w();
}
// ns_recov: P, V, R and the delta biases of the result; the biases stay
template <class NS>
void nav_state_to(const uvo_nav_state& s, NS& ns) {
  typedef typename std::decay<decltype(ns.Get_P())>::type Vec;
  typedef typename std::decay<decltype(ns.Get_R())>::type Rot;
  typedef typename std::decay<decltype(ns.Get_R().unit_quaternion())>::type Quat;
  Vec P = ns.Get_P(), V = ns.Get_V(), dbg = ns.Get_dBias_Gyr(), dba = ns.Get_dBias_Acc();
  for (int i = 0; i < 3; ++i) P(i) = s.P[i], V(i) = s.V[i], dbg(i) = s.dbg[i], dba(i) = s.dba[i];
  ns.Set_Pos(P), ns.Set_Vel(V), ns.Set_DeltaBiasGyr(dbg), ns.Set_DeltaBiasAcc(dba);
  ns.Set_Rot(Rot(Quat(s.q[3], s.q[0], s.q[1], s.q[2])));
}
template <class M>
void mat3_of(const M& m, double* o) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) o[i * 3 + j] = m(i, j);
}
template <class V>
void vec3_of(const V& v, double* o) {
  for (int i = 0; i < 3; ++i) o[i] = v(i);
}
// the walk of :937-991 and :518-624 over one frame: mvbOutlier cleared where a map point exists, and only there
template <class Frame>
void gather_nav(NavOptimizer::Gathered& g, Frame* pFrame) {
  static_assert(sizeof(pFrame->mvKeysUn[0]) == sizeof(uvo_keypoint), "keypoint layout must be cv::KeyPoint");
  g.p3d.clear(), g.p2d.clear(), g.inv_sigma2.clear(), g.index.clear();
  const int N = (int)pFrame->mvpMapPoints.size();
  for (int i = 0; i < N; i++) {
    if (!pFrame->mvpMapPoints[i]) continue;
    float X[3];
    world_pos(pFrame->mvpMapPoints[i]->GetWorldPos(), X);
    g.p3d.insert(g.p3d.end(), X, X + 3);
    pFrame->mvbOutlier[i] = false;
    const uvo_keypoint& kp = reinterpret_cast<const uvo_keypoint&>(pFrame->mvKeysUn[i]);
    g.p2d.push_back(kp.x), g.p2d.push_back(kp.y);
    g.inv_sigma2.push_back(pFrame->mvInvLevelSigma2[kp.octave]);
    g.index.push_back((int32_t)i);
  }
  g.outlier.assign(g.index.empty() ? 1 : g.index.size(), 0);
}
// the frame form's part: the last frame's correspondences, its prior and its information
template <class L>
auto nav_last(NavOptimizer& opt, L* pLast, uvo_nav_problem& p, uvo_nav_result& r, int) -> decltype((void)pLast->mNavStatePrior, void()) {
  p.form = UVO_NAV_FRAME;
  gather_nav(opt.last, pLast);
  const int n = (int)opt.last.index.size();
  p.n_last = n;
  if (n) p.p3d_last = &opt.last.p3d[0], p.p2d_last = &opt.last.p2d[0], p.inv_sigma2_last = &opt.last.inv_sigma2[0];
  r.outlier_last = &opt.last.outlier[0], r.outlier_last_cap = (int32_t)opt.last.outlier.size();
  nav_state_of(pLast->mNavStatePrior, p.prior);
  for (int i = 0; i < 15; ++i)
    for (int j = 0; j < 15; ++j) p.prior_info[i * 15 + j] = pLast->mMargCovInv(i, j);
}
template <class L>
void nav_last(NavOptimizer&, L*, uvo_nav_problem& p, uvo_nav_result&, long) {
  p.form = UVO_NAV_KEYFRAME;
}
template <class L>
auto nav_scatter_last(NavOptimizer& opt, L* pLast, int) -> decltype((void)pLast->mNavStatePrior, void()) {
  for (size_t j = 0; j < opt.last.index.size(); ++j) pLast->mvbOutlier[opt.last.index[j]] = opt.last.outlier[j] != 0;
}
template <class L>
void nav_scatter_last(NavOptimizer&, L*, long) {}
}  // namespace detail

// the owner of the device nav adjuster: one on the mapping thread's matcher handle
class NavBundleAdjuster {
 public:
  NavBundleAdjuster(uvo_matcher* m, int max_free, int max_fixed, int max_points, int max_edges, int max_depth) : a_(0) {
    uvo_nav_bundle_adjuster_create(m, max_free, max_fixed, max_points, max_edges, max_depth, &a_);
  }
  ~NavBundleAdjuster() { uvo_nav_bundle_adjuster_destroy(a_); }
  bool ok() const { return a_ != 0; }
  uvo_nav_bundle_adjuster* handle() { return a_; }
  // gathering buffers, kept between calls so that a call allocates nothing once they have grown
  std::vector<uvo_nav_state> states, states_out;
  std::vector<uvo_nav_ba_link> links;
  std::vector<uvo_nav_ba_depth> depth;
  std::vector<float> points, obs, inv_sigma2, cameras, Tcw_out, points_out;
  std::vector<uint8_t> fixed, has_bias, point_bad, excluded, erased;
  std::vector<int32_t> begin, edge_kf, edge_camera, edge_index;  // edge_index: the observation's index in its key frame
  uvo_nav_ba_result result;                                      // of the last call: counts, iterations, trials

 private:
  NavBundleAdjuster(const NavBundleAdjuster&);
  NavBundleAdjuster& operator=(const NavBundleAdjuster&);
  uvo_nav_bundle_adjuster* a_;
};

namespace detail {
template <class KF>
int index_of(const std::vector<KF*>& v, const KF* p) {
  for (size_t i = 0; i < v.size(); ++i)
    if (v[i] == p) return (int)i;
  return -1;
}
inline void navba_clear(NavBundleAdjuster& a) {
  a.states.clear(), a.links.clear(), a.depth.clear(), a.points.clear(), a.obs.clear(), a.inv_sigma2.clear(), a.cameras.clear(), a.fixed.clear(), a.has_bias.clear();
  a.point_bad.clear(), a.begin.assign(1, 0), a.edge_kf.clear(), a.edge_camera.clear(), a.edge_index.clear();
}
template <class KF>
void navba_add_keyframe(NavBundleAdjuster& a, KF* pKF, bool fixed, bool has_bias) {
  a.states.push_back(uvo_nav_state());
  nav_state_of(pKF->GetNavState(), a.states.back());
  a.fixed.push_back(fixed ? 1 : 0), a.has_bias.push_back(has_bias ? 1 : 0);
}
template <class Pre>
void navba_link(uvo_nav_ba_link& l, int kf0, int kf1, const Pre& pre) {
  l.kf0 = kf0, l.kf1 = kf1, l.dT = pre.getDeltaTime();
  vec3_of(pre.getDeltaP(), l.dP), vec3_of(pre.getDeltaV(), l.dV), mat3_of(pre.getDeltaR(), l.dR);
  mat3_of(pre.getJPBiasg(), l.JPg), mat3_of(pre.getJPBiasa(), l.JPa), mat3_of(pre.getJVBiasg(), l.JVg), mat3_of(pre.getJVBiasa(), l.JVa), mat3_of(pre.getJRBiasg(), l.JRg);
  for (int i = 0; i < 9; ++i)
    for (int j = 0; j < 9; ++j) l.cov_pvphi[i * 9 + j] = pre.getCovPVPhi()(i, j);
}
template <class A, class KF>
int navba_camera(A& a, KF* pKF) {
  const float k[4] = {(float)pKF->fx, (float)pKF->fy, (float)pKF->cx, (float)pKF->cy};
  const int n = (int)a.cameras.size() / 4;
  for (int i = 0; i < n; ++i)
    if (a.cameras[4 * i] == k[0] && a.cameras[4 * i + 1] == k[1] && a.cameras[4 * i + 2] == k[2] && a.cameras[4 * i + 3] == k[3]) return i;
  a.cameras.insert(a.cameras.end(), k, k + 4);
  return n;
}
// a point and its edges (:1498-1559): as ba_add_point
template <class KF, class MP>
void navba_add_point(NavBundleAdjuster& a, MP* pMP, const std::vector<KF*>& vertices, std::vector<KF*>& edge_kfs) {
  float X[3];
  world_pos(pMP->GetWorldPos(), X);
  a.points.insert(a.points.end(), X, X + 3);
  a.point_bad.push_back(pMP->isBad() ? 1 : 0);
  const auto observations = pMP->GetObservations();
  for (auto mit = observations.begin(); mit != observations.end(); ++mit) {
    KF* pKFi = mit->first;
    if (pKFi->isBad()) continue;
    const int k = index_of(vertices, pKFi);
    if (k < 0) continue;
    const auto kp = pKFi->GetKeyPointUn(mit->second);
    static_assert(sizeof(kp) == sizeof(uvo_keypoint), "keypoint layout must be cv::KeyPoint");
    const uvo_keypoint& u = reinterpret_cast<const uvo_keypoint&>(kp);
    a.edge_kf.push_back(k), a.obs.push_back(u.x), a.obs.push_back(u.y);
    a.inv_sigma2.push_back(pKFi->GetInvSigma2(u.octave));
    a.edge_camera.push_back(navba_camera(a, pKFi));
    a.edge_index.push_back((int32_t)mit->second);
    edge_kfs.push_back(pKFi);
  }
  a.begin.push_back((int32_t)a.edge_kf.size());
}
template <class Mat>
int navba_call(NavBundleAdjuster& a, const NavParams& prm, const Mat& gw) {
  const size_t K = a.fixed.size(), P = a.point_bad.size(), E = a.edge_kf.size();
  a.states_out.assign(K + 1, uvo_nav_state()), a.Tcw_out.assign(16 * K + 1, 0.f), a.points_out.assign(3 * P + 1, 0.f), a.excluded.assign(E + 1, 0), a.erased.assign(E + 1, 0);
  uvo_nav_ba_problem q = uvo_nav_ba_problem();
  q.n_keyframes = (int32_t)K, q.n_points = (int32_t)P, q.n_edges = (int32_t)E, q.n_cameras = (int32_t)(a.cameras.size() / 4);
  q.n_links = (int32_t)a.links.size(), q.n_depth = (int32_t)a.depth.size();
  a.states.push_back(uvo_nav_state()), a.links.push_back(uvo_nav_ba_link()), a.depth.push_back(uvo_nav_ba_depth());
  a.points.push_back(0.f), a.obs.push_back(0.f), a.inv_sigma2.push_back(0.f), a.cameras.push_back(0.f);
  a.fixed.push_back(0), a.has_bias.push_back(0), a.point_bad.push_back(0), a.edge_kf.push_back(0), a.edge_camera.push_back(0);  // no empty vector is indexed
  q.kf_state = &a.states[0], q.kf_fixed = &a.fixed[0], q.kf_has_bias = &a.has_bias[0], q.points = &a.points[0], q.point_bad = &a.point_bad[0];
  q.point_edge_begin = &a.begin[0], q.edge_kf = &a.edge_kf[0], q.edge_obs = &a.obs[0], q.edge_inv_sigma2 = &a.inv_sigma2[0], q.edge_camera = &a.edge_camera[0];
  q.cameras = &a.cameras[0], q.links = &a.links[0], q.depth = &a.depth[0];
  float g[3];
  world_pos(gw, g);
  for (int i = 0; i < 3; ++i) {
    q.gw[i] = g[i], q.Pbc[i] = prm.Tbc[i * 4 + 3];
    for (int j = 0; j < 3; ++j) q.Rbc[i * 3 + j] = prm.Tbc[i * 4 + j];
  }
  q.gyr_bias_rw2 = prm.gyr_bias_rw2, q.acc_bias_rw2 = prm.acc_bias_rw2;
  a.result = uvo_nav_ba_result();
  a.result.kf_state = &a.states_out[0], a.result.kf_Tcw = &a.Tcw_out[0], a.result.points = &a.points_out[0], a.result.excluded = &a.excluded[0], a.result.erased = &a.erased[0];
  return uvo_nav_bundle_adjust(a.handle(), &q, &a.result) == UVO_OK ? 0 : -1;
}
}  // namespace detail

namespace Optimizer {

// int Optimizer::PoseOptimization(FrameKTL* pFrame, KeyFrame* pLastKF, const IMUPreintegrator&, const cv::Mat& gw, const cv::Mat& grot,
// const bool& bComputeMarg, double ini_depth, double depth_cov) and the overload over FrameKTL* pLastFrame.  Returns
// nInitialCorrespondences - nBad, 0 on the early return, or -1 when the library call fails (the frames are then as the gathering left
// them).
template <class Frame, class Last, class Pre, class Mat>
int PoseOptimization(NavOptimizer& opt, const NavParams& prm, Frame* pFrame, Last* pLast, const Pre& imupreint, const Mat& gw, const Mat& grot,
                     const bool& bComputeMarg, double ini_depth, double depth_cov) {
  (void)grot;
  if (!opt.ok()) return -1;
  uvo_nav_problem p = uvo_nav_problem();
  uvo_nav_result r = uvo_nav_result();
  detail::gather_nav(opt.cur, pFrame);
  detail::nav_last(opt, pLast, p, r, 0);
  const int n = (int)opt.cur.index.size();
  p.n = n;
  if (n) p.p3d = &opt.cur.p3d[0], p.p2d = &opt.cur.p2d[0], p.inv_sigma2 = &opt.cur.inv_sigma2[0];
  r.outlier = &opt.cur.outlier[0], r.outlier_cap = (int32_t)opt.cur.outlier.size();
  p.has_depth = pFrame->mHas_depth ? 1 : 0, p.compute_marg = bComputeMarg ? 1 : 0;
  detail::nav_state_of(pFrame->GetNavState(), p.cur);
  detail::nav_state_of(pLast->GetNavState(), p.last);
  p.dT = imupreint.getDeltaTime();
  detail::vec3_of(imupreint.getDeltaP(), p.dP), detail::vec3_of(imupreint.getDeltaV(), p.dV), detail::mat3_of(imupreint.getDeltaR(), p.dR);
  detail::mat3_of(imupreint.getJPBiasg(), p.JPg), detail::mat3_of(imupreint.getJPBiasa(), p.JPa), detail::mat3_of(imupreint.getJVBiasg(), p.JVg);
  detail::mat3_of(imupreint.getJVBiasa(), p.JVa), detail::mat3_of(imupreint.getJRBiasg(), p.JRg);
  for (int i = 0; i < 9; ++i)
    for (int j = 0; j < 9; ++j) p.cov_pvphi[i * 9 + j] = imupreint.getCovPVPhi()(i, j);
  float g[3];
  detail::world_pos(gw, g);
  for (int i = 0; i < 3; ++i) {
    p.gw[i] = g[i], p.Pbc[i] = prm.Tbc[i * 4 + 3];
    for (int j = 0; j < 3; ++j) p.Rbc[i * 3 + j] = prm.Tbc[i * 4 + j];
  }
  p.fx = pFrame->fx, p.fy = pFrame->fy, p.cx = pFrame->cx, p.cy = pFrame->cy;
  p.gyr_bias_rw2 = prm.gyr_bias_rw2, p.acc_bias_rw2 = prm.acc_bias_rw2;
  if (p.has_depth) {
    p.shi = (pFrame->mTimeStamp - pLast->mTimeStamp) / (pFrame->mDepth_time - pLast->mTimeStamp);
    p.depth_meas = pFrame->mDepth - ini_depth;
    double R[9], cov3 = 0.;
    detail::mat3_of(pLast->GetNavState().Get_RotMatrix(), R);
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) cov3 = cov3 + (R[i * 3 + 2] * p.cov_pvphi[i * 9 + j]) * R[j * 3 + 2];  // the 3 x 3 position block
    const double cov1 = (p.shi * p.shi * depth_cov * depth_cov) + cov3;
    p.depth_info = 1 / (cov1 * cov1);
  }
  if (uvo_nav_optimize(opt.handle(), &p, 1, &r) != UVO_OK) return -1;
  if (r.rounds == 0) return 0;
  for (int j = 0; j < n; ++j) pFrame->mvbOutlier[opt.cur.index[j]] = opt.cur.outlier[j] != 0;
  detail::nav_scatter_last(opt, pLast, 0);
  typename std::decay<decltype(pFrame->GetNavState())>::type ns = pFrame->GetNavState();
  detail::nav_state_to(r.ns, ns);
  pFrame->SetNavState(ns);
  float* T = pose_data(*pFrame);
  for (int e = 0; e < 16; ++e) T[e] = r.Tcw[e];
  if (bComputeMarg) {
    for (int i = 0; i < 15; ++i)
      for (int j = 0; j < 15; ++j) pFrame->mMargCovInv(i, j) = r.marg_cov_inv[i * 15 + j];
    pFrame->mNavStatePrior = ns;
  }
  return r.n_inliers;
}

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

// void Optimizer::LocalBundleAdjustment(KeyFrame* pKF, bool* pbStopFlag, Map* pMap, LocalMapping* pLM).  Returns 0; 1 when *pbStopFlag
// was set (the marks of the gathering are left, nothing else is touched); -1 when the library call fails (likewise).
template <class KF, class Map, class LM>
int LocalBundleAdjustment(KF* pKF, bool* pbStopFlag, Map* pMap, LM* pLM, BundleAdjuster& adj) {
  typedef typename std::remove_pointer<typename std::remove_reference<decltype(pKF->GetMapPointMatches()[0])>::type>::type MP;
  // Local KeyFrames: First Breath Search from Current Keyframe (:2149-2162)
  std::vector<KF*> lLocalKeyFrames(1, pKF);
  pKF->mnBALocalForKF = pKF->mnId;
  const std::vector<KF*> vNeighKFs = pKF->GetVectorCovisibleKeyFrames();
  for (int i = 0, iend = (int)vNeighKFs.size(); i < iend; i++) {
    KF* pKFi = vNeighKFs[i];
    pKFi->mnBALocalForKF = pKF->mnId;
    if (!pKFi->isBad()) lLocalKeyFrames.push_back(pKFi);
  }
  // Local MapPoints seen in Local KeyFrames (:2164-2180)
  std::vector<MP*> lLocalMapPoints;
  for (size_t l = 0; l < lLocalKeyFrames.size(); ++l) {
    const std::vector<MP*> vpMPs = lLocalKeyFrames[l]->GetMapPointMatches();
    for (size_t v = 0; v < vpMPs.size(); ++v) {
      MP* pMP = vpMPs[v];
      if (pMP)
        if (!pMP->isBad())
          if (pMP->mnBALocalForKF != pKF->mnId) {
            lLocalMapPoints.push_back(pMP);
            pMP->mnBALocalForKF = pKF->mnId;
          }
    }
  }
  // Fixed Keyframes. Keyframes that see Local MapPoints but that are not Local Keyframes (:2182-2198)
  std::vector<KF*> lFixedCameras;
  for (size_t l = 0; l < lLocalMapPoints.size(); ++l) {
    const auto observations = lLocalMapPoints[l]->GetObservations();
    for (auto mit = observations.begin(); mit != observations.end(); ++mit) {
      KF* pKFi = mit->first;
      if (pKFi->mnBALocalForKF != pKF->mnId && pKFi->mnBAFixedForKF != pKF->mnId) {
        pKFi->mnBAFixedForKF = pKF->mnId;
        if (!pKFi->isBad()) lFixedCameras.push_back(pKFi);
      }
    }
  }
  if (pbStopFlag && *pbStopFlag) return 1;
  detail::ba_clear(adj);
  std::vector<KF*> vertices(lLocalKeyFrames);
  vertices.insert(vertices.end(), lFixedCameras.begin(), lFixedCameras.end());
  for (size_t l = 0; l < lLocalKeyFrames.size(); ++l) detail::ba_add_keyframe(adj, lLocalKeyFrames[l], lLocalKeyFrames[l]->mnId == 0);
  for (size_t l = 0; l < lFixedCameras.size(); ++l) detail::ba_add_keyframe(adj, lFixedCameras[l], true);
  std::vector<KF*> vpEdgeKF;
  for (size_t l = 0; l < lLocalMapPoints.size(); ++l) detail::ba_add_point(adj, lLocalMapPoints[l], vertices, vpEdgeKF);
  if (detail::ba_call(adj, UVO_BA_LOCAL, 0) != 0) return -1;
  {
    detail::LockGuard<decltype(pMap->mMutexMapUpdate)> lock(pMap->mMutexMapUpdate);
    // Check inlier observations: the first check's erasures (:2316-2333), then the second's (:2361-2379)
    for (size_t j = 0; j < lLocalMapPoints.size(); ++j) {
      MP* pMP = lLocalMapPoints[j];
      for (int e = adj.begin[j]; e < adj.begin[j + 1]; ++e)
        if (adj.removed1[e]) {
          vpEdgeKF[e]->EraseMapPointMatch(pMP);
          pMP->EraseObservation(vpEdgeKF[e]);
        }
    }
    for (size_t j = 0; j < lLocalMapPoints.size(); ++j) {
      MP* pMP = lLocalMapPoints[j];
      for (int e = adj.begin[j]; e < adj.begin[j + 1]; ++e)
        if (adj.removed2[e]) {
          vpEdgeKF[e]->EraseMapPointMatch(pMP->GetIndexInKeyFrame(vpEdgeKF[e]));
          pMP->EraseObservation(vpEdgeKF[e]);
        }
    }
    // Recover optimized data (:2381-2399)
    for (size_t l = 0; l < lLocalKeyFrames.size(); ++l) ba_set_pose(lLocalKeyFrames[l], &adj.Tcw_out[16 * l]);
    for (size_t j = 0; j < lLocalMapPoints.size(); ++j) {
      ba_set_world_pos(lLocalMapPoints[j], &adj.points_out[3 * j]);
      lLocalMapPoints[j]->UpdateNormalAndDepth();
    }
  }
  if (pLM) pLM->SetMapUpdateFlagInTracking(true);
  return 0;
}

// void Optimizer::BundleAdjustment(const vector<KeyFrame*>& vpKFs, const vector<MapPoint*>& vpMP, int nIterations, bool* pbStopFlag):
// every key frame free but mnId == 0, one optimize(nIterations), no check, nothing erased.  Returns 0, 1 (stop flag set) or -1.
template <class KF, class MP>
int BundleAdjustment(const std::vector<KF*>& vpKFs, const std::vector<MP*>& vpMP, int nIterations, bool* pbStopFlag, BundleAdjuster& adj) {
  if (pbStopFlag && *pbStopFlag) return 1;
  detail::ba_clear(adj);
  std::vector<KF*> vertices;
  for (size_t i = 0; i < vpKFs.size(); i++) {
    KF* pKF = vpKFs[i];
    if (pKF->isBad()) continue;
    vertices.push_back(pKF);
    detail::ba_add_keyframe(adj, pKF, pKF->mnId == 0);
  }
  std::vector<MP*> points;
  std::vector<KF*> vpEdgeKF;
  for (size_t i = 0; i < vpMP.size(); i++) {
    MP* pMP = vpMP[i];
    if (!pMP || pMP->isBad()) continue;
    points.push_back(pMP);
    detail::ba_add_point(adj, pMP, vertices, vpEdgeKF);
  }
  if (detail::ba_call(adj, UVO_BA_FULL, nIterations) != 0) return -1;
  // Recover optimized data (:1986-2008)
  for (size_t l = 0; l < vertices.size(); ++l) ba_set_pose(vertices[l], &adj.Tcw_out[16 * l]);
  for (size_t j = 0; j < points.size(); ++j) {
    ba_set_world_pos(points[j], &adj.points_out[3 * j]);
    points[j]->UpdateNormalAndDepth();
  }
  return 0;
}

// void Optimizer::GlobalBundleAdjustemnt(Map* pMap, int nIterations, bool* pbStopFlag), with the reference's spelling
template <class Map>
int GlobalBundleAdjustemnt(Map* pMap, int nIterations, bool* pbStopFlag, BundleAdjuster& adj) {
  const auto vpKFs = pMap->GetAllKeyFrames();
  const auto vpMP = pMap->GetAllMapPoints();
  return BundleAdjustment(vpKFs, vpMP, nIterations, pbStopFlag, adj);
}

// void Optimizer::RecoveryBundleAdjustemnt(KeyFrame* pKFini, KeyFrame* pKFcur, int nIterations, bool* pbStopFlag)
template <class KF>
int RecoveryBundleAdjustemnt(KF* pKFini, KF* pKFcur, int nIterations, bool* pbStopFlag, BundleAdjuster& adj) {
  std::vector<KF*> vpKFs;
  vpKFs.push_back(pKFini);
  vpKFs.push_back(pKFcur);
  const auto vpMP = pKFcur->getmvpMappoints();
  return BundleAdjustment(vpKFs, vpMP, nIterations, pbStopFlag, adj);
}

// void Optimizer::LocalBundleAdjustmentNavState(KeyFrame* pCurKF, const std::list<KeyFrame*>& lLocalKeyFrames, bool* pbStopFlag, Map* pMap,
// const cv::Mat& gw, const cv::Mat& grot, LocalMapping* pLM, double ini_depth, double depth_cov, int fixedKF_id).  Returns 0; 1 when
// *pbStopFlag was set (the marks of the gathering are left, nothing else is touched); -1 when there is no usable key frame before the window
// or the library call fails (likewise).
template <class KF, class List, class Map, class Mat, class LM>
int LocalBundleAdjustmentNavState(KF* pCurKF, const List& lLocalKeyFrames, bool* pbStopFlag, Map* pMap, const Mat& gw, const Mat& grot, LM* pLM, double ini_depth,
                                  double depth_cov, int fixedKF_id, const NavParams& prm, NavBundleAdjuster& adj) {
  typedef typename std::remove_pointer<typename std::remove_reference<decltype(pCurKF->GetMapPointMatches()[0])>::type>::type MP;
  (void)grot;
  if (!adj.ok()) return -1;
  // All KeyFrames in Local window are optimized (:1121-1125)
  std::vector<KF*> window(lLocalKeyFrames.begin(), lLocalKeyFrames.end());
  if (window.empty()) return -1;
  for (size_t l = 0; l < window.size(); ++l) window[l]->mnBALocalForKF = pCurKF->mnId;
  // Local MapPoints seen in Local KeyFrames (:1127-1143)
  std::vector<MP*> lLocalMapPoints;
  for (size_t l = 0; l < window.size(); ++l) {
    const std::vector<MP*> vpMPs = window[l]->GetMapPointMatches();
    for (size_t v = 0; v < vpMPs.size(); ++v) {
      MP* pMP = vpMPs[v];
      if (pMP)
        if (!pMP->isBad())
          if (pMP->mnBALocalForKF != pCurKF->mnId) {
            lLocalMapPoints.push_back(pMP);
            pMP->mnBALocalForKF = pCurKF->mnId;
          }
    }
  }
  // Fixed Keyframes: the KeyFrame before local window, then the covisible ones (:1145-1182)
  std::vector<KF*> lFixedCameras;
  KF* pKFPrevLocal = window.front()->GetPrevKeyFrame();
  if (!pKFPrevLocal) return -1;
  const long unsigned int minKFID = pKFPrevLocal->mnId;
  pKFPrevLocal->mnBAFixedForKF = pCurKF->mnId;
  if (pKFPrevLocal->isBad()) return -1;
  lFixedCameras.push_back(pKFPrevLocal);
  for (size_t l = 0; l < lLocalMapPoints.size(); ++l) {
    const auto observations = lLocalMapPoints[l]->GetObservations();
    for (auto mit = observations.begin(); mit != observations.end(); ++mit) {
      KF* pKFi = mit->first;
      if (pKFi->mnBALocalForKF != pCurKF->mnId && pKFi->mnBAFixedForKF != pCurKF->mnId) {
        pKFi->mnBAFixedForKF = pCurKF->mnId;
        if (!pKFi->isBad()) lFixedCameras.push_back(pKFi);
      }
    }
  }
  if (pbStopFlag && *pbStopFlag) return 1;
  detail::navba_clear(adj);
  std::vector<KF*> vertices(window);
  vertices.insert(vertices.end(), lFixedCameras.begin(), lFixedCameras.end());
  for (size_t l = 0; l < window.size(); ++l) detail::navba_add_keyframe(adj, window[l], (long)window[l]->mnId == (long)fixedKF_id, true);
  for (size_t l = 0; l < lFixedCameras.size(); ++l) detail::navba_add_keyframe(adj, lFixedCameras[l], true, lFixedCameras[l] == pKFPrevLocal);
  // the inertial links and the depth entries (:1273-1482)
  for (size_t l = 0; l < window.size(); ++l) {
    KF* pKF1 = window[l];
    KF* pKF0 = pKF1->GetPrevKeyFrame();
    const int k0 = pKF0 ? detail::index_of(vertices, pKF0) : -1;
    if (k0 < 0 || !adj.has_bias[k0]) return -1;
    adj.links.push_back(uvo_nav_ba_link());
    detail::navba_link(adj.links.back(), k0, (int)l, pKF1->GetIMUPreInt());
    for (size_t i = 0; i < pKF1->Depth_Vec.size(); i++) {
      const double depth_time = pKF1->Depth_Vec_Time[i];
      uvo_nav_ba_depth d = uvo_nav_ba_depth();
      KF* pRot = 0;
      if ((pKF1->mTimeStamp - depth_time) < (depth_time - pKF0->mTimeStamp)) {      // forward
        d.ka = (int32_t)l, d.kb = k0, d.kc = k0, d.link = (int32_t)l;
        d.shi = (pKF1->mTimeStamp - pKF0->mTimeStamp) / (depth_time - pKF0->mTimeStamp);
        pRot = pKF0;
      } else if (minKFID + 1 < pKF0->mnId) {                                        // backward
        KF* pKF_1 = pKF0->GetPrevKeyFrame();
        const int k_1 = pKF_1 ? detail::index_of(window, pKF_1) : -1;
        if (k_1 < 0 || k_1 >= (int)l) continue;     // its preintegration is the link of a window key frame listed before
        d.ka = k0, d.kb = k_1, d.kc = k_1, d.link = k_1;
        d.shi = (pKF0->mTimeStamp - pKF_1->mTimeStamp) / (depth_time - pKF_1->mTimeStamp);
        pRot = pKF_1;
      } else {
        continue;
      }
      d.meas = pKF1->Depth_Vec[i] - ini_depth;
      double R[9], cov3 = 0.;
      detail::mat3_of(pRot->GetNavState().Get_RotMatrix(), R);
      const double* cov = adj.links[d.link].cov_pvphi;
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) cov3 = cov3 + (R[r * 3 + 2] * cov[r * 9 + c]) * R[c * 3 + 2];  // the 3 x 3 position block
      const double cov1 = (d.shi * d.shi * depth_cov * depth_cov) + cov3;
      d.info = 1 / (cov1 * cov1);
      adj.depth.push_back(d);
    }
  }
  std::vector<KF*> vpEdgeKF;
  for (size_t l = 0; l < lLocalMapPoints.size(); ++l) detail::navba_add_point(adj, lLocalMapPoints[l], vertices, vpEdgeKF);
  if (detail::navba_call(adj, prm, gw) != 0) return -1;
  {
    detail::LockGuard<decltype(pMap->mMutexMapUpdate)> lock(pMap->mMutexMapUpdate);
    // vToErase: the final check's (:1624-1678)
    for (size_t j = 0; j < lLocalMapPoints.size(); ++j) {
      MP* pMP = lLocalMapPoints[j];
      for (int e = adj.begin[j]; e < adj.begin[j + 1]; ++e)
        if (adj.erased[e]) {
          vpEdgeKF[e]->EraseMapPointMatch(pMP);
          pMP->EraseObservation(vpEdgeKF[e]);
        }
    }
    // Keyframes (:1680-1716)
    for (size_t l = 0; l < window.size(); ++l) {
      KF* pKFi = window[l];
      typename std::decay<decltype(pKFi->GetNavState())>::type ns = pKFi->GetNavState();
      detail::nav_state_to(adj.states_out[l], ns);
      pKFi->SetNavStatePos(ns.Get_P()), pKFi->SetNavStateVel(ns.Get_V()), pKFi->SetNavStateRot(ns.Get_R());
      pKFi->SetNavStateDeltaBg(ns.Get_dBias_Gyr()), pKFi->SetNavStateDeltaBa(ns.Get_dBias_Acc());
      ba_set_pose(pKFi, &adj.Tcw_out[16 * l]);
    }
    // Points (:1718-1725)
    for (size_t j = 0; j < lLocalMapPoints.size(); ++j) {
      ba_set_world_pos(lLocalMapPoints[j], &adj.points_out[3 * j]);
      lLocalMapPoints[j]->UpdateNormalAndDepth();
    }
  }
  if (pLM) pLM->SetMapUpdateFlagInTracking(true);
  return 0;
}

}  // namespace Optimizer

// the owner of the device graph: one on the loop-closing thread's matcher handle; the sizes in the order of uvo_essential_graph_create
class EssentialGraphOptimizer {
 public:
  EssentialGraphOptimizer(uvo_matcher* m, int max_keyframes, int max_edges, int max_envelope_blocks, int max_points) : g_(0) {
    uvo_essential_graph_create(m, max_keyframes, max_edges, max_envelope_blocks, max_points, &g_);
  }
  ~EssentialGraphOptimizer() { uvo_essential_graph_destroy(g_); }
  bool ok() const { return g_ != 0; }
  uvo_essential_graph* handle() { return g_; }
  // gathering buffers, kept between calls so that a call allocates nothing once they have grown
  std::vector<uvo_sim3d> Scw, Scw_normal, Scw_out;
  std::vector<int32_t> edge_i, edge_j, point_ref;
  std::vector<uint8_t> edge_connection;
  std::vector<float> points, Tcw_out, points_out;
  uvo_essential_result result;  // of the last call: iterations, trials, envelope blocks

 private:
  EssentialGraphOptimizer(const EssentialGraphOptimizer&);
  EssentialGraphOptimizer& operator=(const EssentialGraphOptimizer&);
  uvo_essential_graph* g_;
};

namespace detail {
inline uvo_sim3d sim3d_of(const Sim3& S) {
  uvo_sim3d o;
  for (int e = 0; e < 4; ++e) o.q[e] = S.quaternion()[e];
  for (int e = 0; e < 3; ++e) o.t[e] = S.translation()[e];
  o.s = S.scale();
  return o;
}
// g2o::Sim3 Siw(Rcw, tcw, 1.0) of the key frame's float pose
template <class KF>
uvo_sim3d sim3d_of_pose(KF* pKF) {
  const auto R = pKF->GetRotation();
  const auto t = pKF->GetTranslation();
  float Rf[9], tf[3];
  for (int e = 0; e < 9; ++e) Rf[e] = mat_elem(R, e, 0);
  for (int e = 0; e < 3; ++e) tf[e] = mat_elem(t, e, 0);
  return sim3d_of(Sim3(Rf, tf, 1.f));
}
template <class KF>
struct ById {
  bool operator()(const KF* a, const KF* b) const { return a->mnId < b->mnId; }
};
}  // namespace detail

namespace Optimizer {

template <class Map, class KF, class KeyFrameAndPose, class Connections>
int OptimizeEssentialGraph(EssentialGraphOptimizer& g, Map* pMap, KF* pLoopKF, KF* pCurKF, const Sim3& /*Scurw*/, const KeyFrameAndPose& NonCorrectedSim3,
                           const KeyFrameAndPose& CorrectedSim3, const Connections& LoopConnections) {
  const auto vpKFs = pMap->GetAllKeyFrames();
  const auto vpMPs = pMap->GetAllMapPoints();
  const int minFeat = 100;
  // SET KEYFRAME VERTICES (:2437-2470), in ascending mnId
  std::vector<KF*> vertices;
  for (size_t i = 0; i < vpKFs.size(); i++)
    if (!vpKFs[i]->isBad()) vertices.push_back(vpKFs[i]);
  std::sort(vertices.begin(), vertices.end(), detail::ById<KF>());
  std::map<KF*, int32_t> index;
  g.Scw.clear(), g.Scw_normal.clear(), g.edge_i.clear(), g.edge_j.clear(), g.edge_connection.clear(), g.points.clear(), g.point_ref.clear();
  for (size_t k = 0; k < vertices.size(); ++k) {
    KF* pKF = vertices[k];
    index[pKF] = (int32_t)k;
    const auto c = CorrectedSim3.find(pKF);
    g.Scw.push_back(c != CorrectedSim3.end() ? detail::sim3d_of(c->second) : detail::sim3d_of_pose(pKF));
    const auto n = NonCorrectedSim3.find(pKF);
    g.Scw_normal.push_back(n != NonCorrectedSim3.end() ? detail::sim3d_of(n->second) : g.Scw.back());
  }
  if (!index.count(pLoopKF)) return -1;
  struct Add {
    EssentialGraphOptimizer& g;
    const std::map<KF*, int32_t>& index;
    bool operator()(KF* i, KF* j, bool connection) const {  // vertex 0 = i, vertex 1 = j; false: one of them is no vertex
      const typename std::map<KF*, int32_t>::const_iterator a = index.find(i), b = index.find(j);
      if (a == index.end() || b == index.end()) return false;
      g.edge_i.push_back(a->second), g.edge_j.push_back(b->second), g.edge_connection.push_back(connection ? 1 : 0);
      return true;
    }
  } add = {g, index};
  std::set<std::pair<long unsigned int, long unsigned int> > sInsertedEdges;
  // SET LOOP EDGES (:2477-2506)
  for (auto mit = LoopConnections.begin(), mend = LoopConnections.end(); mit != mend; mit++) {
    KF* pKF = mit->first;
    const long unsigned int nIDi = pKF->mnId;
    const auto& spConnections = mit->second;
    for (auto sit = spConnections.begin(), send = spConnections.end(); sit != send; sit++) {
      const long unsigned int nIDj = (*sit)->mnId;
      if ((nIDi != pCurKF->mnId || nIDj != pLoopKF->mnId) && pKF->GetWeight(*sit) < minFeat) continue;
      if (!add(pKF, *sit, true)) continue;
      sInsertedEdges.insert(std::make_pair(std::min(nIDi, nIDj), std::max(nIDi, nIDj)));
    }
  }
  // SET NORMAL EDGES (:2508-2598)
  for (size_t i = 0, iend = vpKFs.size(); i < iend; i++) {
    KF* pKF = vpKFs[i];
    if (pKF->isBad()) continue;
    KF* pParentKF = pKF->GetParent();
    if (pParentKF) add(pKF, pParentKF, false);  // Spanning tree edge
    const std::set<KF*> sLoopEdges = pKF->GetLoopEdges();
    for (auto sit = sLoopEdges.begin(), send = sLoopEdges.end(); sit != send; sit++) {
      KF* pLKF = *sit;
      if (pLKF->mnId < pKF->mnId) add(pKF, pLKF, false);
    }
    const std::vector<KF*> vpConnectedKFs = pKF->GetCovisiblesByWeight(minFeat);
    for (auto vit = vpConnectedKFs.begin(); vit != vpConnectedKFs.end(); vit++) {
      KF* pKFn = *vit;
      if (pKFn && pKFn != pParentKF && !pKF->hasChild(pKFn) && !sLoopEdges.count(pKFn)) {
        if (!pKFn->isBad() && pKFn->mnId < pKF->mnId) {
          if (sInsertedEdges.count(std::make_pair(std::min(pKF->mnId, pKFn->mnId), std::max(pKF->mnId, pKFn->mnId)))) continue;
          add(pKF, pKFn, false);
        }
      }
    }
  }
  // the points that are corrected (:2627-2647); a point whose reference key frame is no vertex stays where it is
  typedef typename std::remove_pointer<typename std::remove_reference<decltype(vpMPs[0])>::type>::type MPc;
  typedef typename std::remove_const<MPc>::type MP;
  std::vector<MP*> points, kept;
  for (size_t i = 0, iend = vpMPs.size(); i < iend; i++) {
    MP* pMP = vpMPs[i];
    if (pMP->isBad()) continue;
    KF* pRefKF = 0;
    long unsigned int nIDr;
    if (pMP->mnCorrectedByKF == pCurKF->mnId) nIDr = pMP->mnCorrectedReference;
    else pRefKF = pMP->GetReferenceKeyFrame(), nIDr = pRefKF->mnId;
    int32_t ref = -1;
    for (size_t k = 0; k < vertices.size() && ref < 0; ++k)
      if (vertices[k]->mnId == nIDr) ref = (int32_t)k;
    if (ref < 0) {
      kept.push_back(pMP);
      continue;
    }
    float X[3];
    detail::world_pos(pMP->GetWorldPos(), X);
    g.points.insert(g.points.end(), X, X + 3);
    g.point_ref.push_back(ref);
    points.push_back(pMP);
  }
  // OPTIMIZE (:2602-2603)
  const int32_t K = (int32_t)vertices.size(), E = (int32_t)g.edge_i.size(), P = (int32_t)points.size();
  g.Scw_out.resize((size_t)K), g.Tcw_out.resize(16 * (size_t)K), g.points_out.resize(3 * (size_t)P + 1);
  uvo_essential_problem q;
  q.n_keyframes = K, q.n_edges = E, q.n_points = P, q.fixed = index[pLoopKF];
  q.Scw = g.Scw.data(), q.Scw_normal = g.Scw_normal.data(), q.edge_i = g.edge_i.data(), q.edge_j = g.edge_j.data(), q.edge_connection = g.edge_connection.data();
  q.points = g.points.data(), q.point_ref = g.point_ref.data(), q.n_iterations = 20;
  g.result.Scw = g.Scw_out.data(), g.result.kf_Tcw = g.Tcw_out.data(), g.result.points = g.points_out.data();
  if (!g.ok() || uvo_essential_graph_optimize(g.handle(), &q, &g.result) != UVO_OK) return -1;
  // SE3 Pose Recovering and the points (:2605-2657)
  for (size_t k = 0; k < vertices.size(); ++k) ba_set_pose(vertices[k], &g.Tcw_out[16 * k]);
  for (size_t j = 0; j < points.size(); ++j) {
    ba_set_world_pos(points[j], &g.points_out[3 * j]);
    points[j]->UpdateNormalAndDepth();
  }
  for (size_t j = 0; j < kept.size(); ++j) {
    float X[3];
    detail::world_pos(kept[j]->GetWorldPos(), X);
    ba_set_world_pos(kept[j], X);
    kept[j]->UpdateNormalAndDepth();
  }
  return 0;
}

}  // namespace Optimizer
}  // namespace USLAM
#endif  // UVO_COMPAT_OPTIMIZER_H_
