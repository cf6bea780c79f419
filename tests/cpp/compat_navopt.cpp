// Drives the two IMU overloads of USLAM::Optimizer::PoseOptimization (include/uvo/compat/Optimizer.h) the way Tracking::TrackWithIMU
// and TrackLocalMapWithIMU would: frames whose mvpMapPoints have gaps, mvbOutlier pre-set to a pattern, the overload chosen by the type
// of the second argument; in the frame form a second call follows in which the first call's frame is the last frame, so that the prior
// the first call wrote is the one the second reads.  Everything touched is written out for tests/test_gpu_cpp_navopt.py.
// Built as C++11 with -Wall -Werror, no OpenCV, no Eigen: the stand-ins below have the members the adaptor names.
//
//   compat_navopt scene.bin out.bin
// scene.bin: the problem record of tests/navopt_model.py (PROBLEM_DTYPE); double depth_cov; float invLevelSigma2[8]; then for the
//            current and the last frame: int32 nkeys; uvo_keypoint keys[nkeys]; {int32 has; float xyz[3]} [nkeys]; uint8 before[nkeys]
// out.bin:   per call: int32 ret; double ns[22]; float Tcw[16]; double mMargCovInv[225]; double mNavStatePrior[22];
//            uint8 after[nkeys]; uint8 after_last[nkeys_last]
#include <cstdio>
#include <cstring>
#include <vector>

#include "uvo/compat/Optimizer.h"

namespace {
struct Vec3 {
  double v[3];
  double operator()(int i) const { return v[i]; }
  double& operator()(int i) { return v[i]; }
};
template <int N>
struct MatN {
  double m[N * N];
  double operator()(int i, int j) const { return m[i * N + j]; }
  double& operator()(int i, int j) { return m[i * N + j]; }
};
struct Quat {
  double c[4];  // x y z w
  Quat() {}
  Quat(double w, double x, double y, double z) { c[0] = x, c[1] = y, c[2] = z, c[3] = w; }
  double x() const { return c[0]; }
  double y() const { return c[1]; }
  double z() const { return c[2]; }
  double w() const { return c[3]; }
};
struct SO3 {
  Quat q;
  SO3() {}
  explicit SO3(const Quat& q_) : q(q_) {}
  const Quat& unit_quaternion() const { return q; }
};
struct NavState {
  Vec3 P, V, bg, ba, dbg, dba;
  SO3 R;
  Vec3 Get_P() const { return P; }
  Vec3 Get_V() const { return V; }
  SO3 Get_R() const { return R; }
  MatN<3> Get_RotMatrix() const {  // Eigen's toRotationMatrix
    const double* q = R.q.c;
    const double tx = 2. * q[0], ty = 2. * q[1], tz = 2. * q[2];
    const double twx = tx * q[3], twy = ty * q[3], twz = tz * q[3], txx = tx * q[0], txy = ty * q[0], txz = tz * q[0], tyy = ty * q[1], tyz = tz * q[1], tzz = tz * q[2];
    MatN<3> M = {{1. - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1. - (txx + tzz), tyz - twx, txz - twy, tyz + twx, 1. - (txx + tyy)}};
    return M;
  }
  Vec3 Get_BiasGyr() const { return bg; }
  Vec3 Get_BiasAcc() const { return ba; }
  Vec3 Get_dBias_Gyr() const { return dbg; }
  Vec3 Get_dBias_Acc() const { return dba; }
  void Set_Pos(const Vec3& v) { P = v; }
  void Set_Vel(const Vec3& v) { V = v; }
  void Set_Rot(const SO3& r) { R = r; }
  void Set_DeltaBiasGyr(const Vec3& v) { dbg = v; }
  void Set_DeltaBiasAcc(const Vec3& v) { dba = v; }
  void from(const double* s) {
    std::memcpy(P.v, s, 24), std::memcpy(V.v, s + 3, 24), std::memcpy(R.q.c, s + 6, 32), std::memcpy(bg.v, s + 10, 24), std::memcpy(ba.v, s + 13, 24);
    std::memcpy(dbg.v, s + 16, 24), std::memcpy(dba.v, s + 19, 24);
  }
  void to(double* s) const {
    std::memcpy(s, P.v, 24), std::memcpy(s + 3, V.v, 24), std::memcpy(s + 6, R.q.c, 32), std::memcpy(s + 10, bg.v, 24), std::memcpy(s + 13, ba.v, 24);
    std::memcpy(s + 16, dbg.v, 24), std::memcpy(s + 19, dba.v, 24);
  }
};
struct Pos {
  float v[3];
  float operator[](int i) const { return v[i]; }
};
struct MapPoint {
  Pos pos;
  Pos GetWorldPos() const { return pos; }
};
struct KeyFrame {
  NavState ns;
  double mTimeStamp;
  const NavState& GetNavState() const { return ns; }
};
struct Frame {
  std::vector<MapPoint*> mvpMapPoints;
  std::vector<MapPoint> store;
  std::vector<uvo_keypoint> mvKeysUn;
  std::vector<float> mvInvLevelSigma2;
  std::vector<bool> mvbOutlier;
  float mTcw[16];
  float fx, fy, cx, cy;
  NavState mNavState, mNavStatePrior;
  MatN<15> mMargCovInv;
  bool mHas_depth;
  double mDepth, mDepth_time, mTimeStamp;
  const NavState& GetNavState() const { return mNavState; }
  void SetNavState(const NavState& ns) { mNavState = ns; }
};
struct Preint {
  double dT;
  Vec3 dP, dV;
  MatN<3> dR, JPg, JPa, JVg, JVa, JRg;
  MatN<9> cov;
  double getDeltaTime() const { return dT; }
  Vec3 getDeltaP() const { return dP; }
  Vec3 getDeltaV() const { return dV; }
  MatN<3> getDeltaR() const { return dR; }
  MatN<3> getJPBiasg() const { return JPg; }
  MatN<3> getJPBiasa() const { return JPa; }
  MatN<3> getJVBiasg() const { return JVg; }
  MatN<3> getJVBiasa() const { return JVa; }
  MatN<3> getJRBiasg() const { return JRg; }
  const MatN<9>& getCovPVPhi() const { return cov; }
};
// navopt::Problem as tests/navopt_model.py writes it
struct Record {
  int32_t form, has_depth, compute_marg, n, n_last, off, pad_[2];
  double cur[22], last[22], prior[22];
  double dT, dP[3], dV[3], dR[9], JPg[9], JPa[9], JVg[9], JVa[9], JRg[9], cov[81];
  double gw[3], Rbc[9], Pbc[3], fx, fy, cx, cy, gyr_rw2, acc_rw2;
  double prior_info[225];
  double depth_meas, shi, depth_info;
};
bool rd(FILE* f, void* p, size_t n) { return std::fread(p, 1, n, f) == n; }
bool read_frame(FILE* f, Frame& F, const float* inv_levels, const Record& R) {
  int32_t nkeys = 0;
  if (!rd(f, &nkeys, 4) || nkeys < 0) return false;
  F.mvInvLevelSigma2.assign(inv_levels, inv_levels + 8);
  F.mvKeysUn.resize(nkeys), F.store.resize(nkeys), F.mvpMapPoints.assign(nkeys, (MapPoint*)0);
  if (nkeys && !rd(f, &F.mvKeysUn[0], sizeof(uvo_keypoint) * (size_t)nkeys)) return false;
  for (int i = 0; i < nkeys; ++i) {
    struct {
      int32_t has;
      float p[3];
    } rec;
    if (!rd(f, &rec, sizeof rec)) return false;
    std::memcpy(F.store[i].pos.v, rec.p, 12);
    if (rec.has) F.mvpMapPoints[i] = &F.store[i];
  }
  std::vector<uint8_t> before(nkeys ? nkeys : 1);
  if (nkeys && !rd(f, &before[0], (size_t)nkeys)) return false;
  F.mvbOutlier.assign(before.begin(), before.begin() + nkeys);
  F.fx = (float)R.fx, F.fy = (float)R.fy, F.cx = (float)R.cx, F.cy = (float)R.cy;
  std::memset(F.mTcw, 0, sizeof F.mTcw);
  std::memset(&F.mMargCovInv, 0, sizeof F.mMargCovInv);
  F.mHas_depth = false, F.mDepth = 0., F.mDepth_time = 1., F.mTimeStamp = 0.;
  return true;
}
void write_call(FILE* o, int32_t ret, const Frame& F, const Frame* L) {
  double s[22];
  std::fwrite(&ret, 4, 1, o);
  F.mNavState.to(s);
  std::fwrite(s, 8, 22, o);
  std::fwrite(F.mTcw, 4, 16, o);
  std::fwrite(F.mMargCovInv.m, 8, 225, o);
  F.mNavStatePrior.to(s);
  std::fwrite(s, 8, 22, o);
  for (size_t i = 0; i < F.mvbOutlier.size(); ++i) std::fputc(F.mvbOutlier[i] ? 1 : 0, o);
  if (L)
    for (size_t i = 0; i < L->mvbOutlier.size(); ++i) std::fputc(L->mvbOutlier[i] ? 1 : 0, o);
}
}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  static Record R;
  double depth_cov = 0.;
  float inv_levels[8];
  Frame F, L;
  if (!rd(f, &R, sizeof R) || !rd(f, &depth_cov, 8) || !rd(f, inv_levels, 32) || !read_frame(f, F, inv_levels, R) || !read_frame(f, L, inv_levels, R)) return 2;
  std::fclose(f);
  // times and depth chosen so that the adaptor's shi and measurement are the record's exactly: (shi - 0) / (1 - 0), depth - 0
  F.mNavState.from(R.cur), F.mNavStatePrior.from(R.cur), F.mHas_depth = R.has_depth != 0, F.mDepth = R.depth_meas, F.mTimeStamp = R.shi;
  L.mNavState.from(R.last), L.mNavStatePrior.from(R.prior);
  std::memcpy(L.mMargCovInv.m, R.prior_info, sizeof R.prior_info);
  Preint M;
  M.dT = R.dT;
  std::memcpy(M.dP.v, R.dP, 24), std::memcpy(M.dV.v, R.dV, 24), std::memcpy(M.dR.m, R.dR, 72), std::memcpy(M.JPg.m, R.JPg, 72), std::memcpy(M.JPa.m, R.JPa, 72);
  std::memcpy(M.JVg.m, R.JVg, 72), std::memcpy(M.JVa.m, R.JVa, 72), std::memcpy(M.JRg.m, R.JRg, 72), std::memcpy(M.cov.m, R.cov, 648);
  USLAM::NavParams prm;
  std::memset(&prm, 0, sizeof prm);
  for (int i = 0; i < 3; ++i) {
    prm.Tbc[i * 4 + 3] = R.Pbc[i];
    for (int j = 0; j < 3; ++j) prm.Tbc[i * 4 + j] = R.Rbc[i * 3 + j];
  }
  prm.Tbc[15] = 1., prm.gyr_bias_rw2 = R.gyr_rw2, prm.acc_bias_rw2 = R.acc_rw2;
  const Pos gw = {{(float)R.gw[0], (float)R.gw[1], (float)R.gw[2]}}, grot = {{0.f, 0.f, 0.f}};

  uvo_klt_cfg cfg = {64, 64, 3, 21, 21, 16, 2, 0};
  uvo_klt* klt = 0;
  if (uvo_klt_create(&cfg, &klt) != UVO_OK) {
    std::fprintf(stderr, "%s\n", uvo_last_error());
    return 1;
  }
  FILE* o = std::fopen(argv[2], "wb");
  if (!o) return 2;
  int32_t ret = -1, ret2 = -1;
  {
    const int cap = (int)(F.mvKeysUn.size() > L.mvKeysUn.size() ? F.mvKeysUn.size() : L.mvKeysUn.size());
    USLAM::NavOptimizer opt(klt, cap > 0 ? cap : 1);
    if (!opt.ok()) {
      std::fprintf(stderr, "%s\n", uvo_last_error());
      return 1;
    }
    const Frame F0 = F;  // the current frame as it came, for the second call
    if (R.form == UVO_NAV_KEYFRAME) {
      KeyFrame K;
      K.ns = L.mNavState, K.mTimeStamp = 0.;
      ret = USLAM::Optimizer::PoseOptimization(opt, prm, &F, &K, M, gw, grot, R.compute_marg != 0, 0., depth_cov);
      write_call(o, ret, F, 0);
    } else {
      ret = USLAM::Optimizer::PoseOptimization(opt, prm, &F, &L, M, gw, grot, R.compute_marg != 0, 0., depth_cov);
      write_call(o, ret, F, &L);
      // the next frame: the frame just optimised is the last frame now, its prior and information those the call wrote
      Frame N = F0;
      for (size_t i = 0; i < N.mvpMapPoints.size(); ++i)
        if (N.mvpMapPoints[i]) N.mvpMapPoints[i] = &N.store[i];
      F.mTimeStamp = 0.;
      ret2 = USLAM::Optimizer::PoseOptimization(opt, prm, &N, &F, M, gw, grot, R.compute_marg != 0, 0., depth_cov);
      write_call(o, ret2, N, &F);
    }
    if (ret < 0) {
      std::fprintf(stderr, "%s\n", uvo_last_error());
      return 1;
    }
  }
  uvo_klt_destroy(klt);
  std::fclose(o);
  std::printf("{\"ret\": %d, \"ret2\": %d}\n", ret, ret2);
  return 0;
}
