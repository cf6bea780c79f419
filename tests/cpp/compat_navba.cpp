// Drives USLAM::Optimizer::LocalBundleAdjustmentNavState (include/uvo/compat/Optimizer.h) the way LocalMapping::Run would after the IMU is
// initialised: key frames, map points, the map and the local mapper as stub types, a hand-built map with everything the gathering of
// src/Optimizer.cc:1121-1182 and the depth rule of :1371-1465 distinguish; everything the call touched is written out for
// tests/test_gpu_cpp_navba.py.  Built as C++11 with -Wall -Werror, no OpenCV, no Eigen.
//
//   compat_navba scene.bin out.bin
// scene.bin: int32 current, nKF, nMP, nWindow, fixedKF_id, stop; double ini_depth, depth_cov, Tbc[16], gyr_rw2, acc_rw2; float gw[3], invLevelSigma2[8];
//            int32 window[nWindow]; per key frame: int32 mnId, bad, prev; double ns[22], t; float K[4]; double preint[142]; int32 ndepth;
//            double depth[ndepth], depth_time[ndepth]; int32 nkeys; {float x, y; int32 octave, mp} [nkeys]; per map point: int32 bad, late; float pos[3]
// out.bin:   int32 ret, map flag, locks, K, P, E, L, D; int32 begin[P + 1], edge_kf[E], edge_index[E]; uint8 excluded[E], erased[E];
//            {int32 kf0, kf1} [L]; uvo_nav_ba_depth [D]; per key frame: int32 mnBALocalForKF, mnBAFixedForKF, poses set, states set; double ns[22];
//            float T[16]; int32 mp[nkeys]; per map point: int32 mnBALocalForKF, positions set, normal updates; float pos[3]; int32 nobs, observer[nobs]
#include <cstdio>
#include <cstring>
#include <map>
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
struct Pos {
  float v[3];
  float operator[](int i) const { return v[i]; }
};
struct KeyFrame;
struct MapPoint {
  long unsigned int mnBALocalForKF;
  bool bad, late;  // late: reports bad once the gathering has marked it, as a point culled by another thread in between would
  Pos pos;
  int n_set, n_updates;
  std::map<KeyFrame*, size_t> obs;
  bool isBad() const { return bad || (late && mnBALocalForKF != 1000000); }
  Pos GetWorldPos() const { return pos; }
  void SetWorldPos(const float* X) { pos.v[0] = X[0], pos.v[1] = X[1], pos.v[2] = X[2], ++n_set; }
  void UpdateNormalAndDepth() { ++n_updates; }
  std::map<KeyFrame*, size_t> GetObservations() const { return obs; }
  void EraseObservation(KeyFrame* kf) { obs.erase(kf); }
  int GetIndexInKeyFrame(KeyFrame* kf) const {
    std::map<KeyFrame*, size_t>::const_iterator it = obs.find(kf);
    return it == obs.end() ? -1 : (int)it->second;
  }
};
struct KeyFrame {
  long unsigned int mnId, mnBALocalForKF, mnBAFixedForKF;
  bool bad;
  KeyFrame* prev;
  NavState ns;
  Preint pre;
  double mTimeStamp;
  std::vector<double> Depth_Vec, Depth_Vec_Time;
  float T[16];
  float fx, fy, cx, cy;
  int n_pose, n_ns;
  std::vector<uvo_keypoint> keys;
  std::vector<MapPoint*> points;
  const float* inv_sigma2;
  bool isBad() const { return bad; }
  KeyFrame* GetPrevKeyFrame() const { return prev; }
  const NavState& GetNavState() const { return ns; }
  const Preint& GetIMUPreInt() const { return pre; }
  void SetNavStatePos(const Vec3& v) { ns.Set_Pos(v), ++n_ns; }
  void SetNavStateVel(const Vec3& v) { ns.Set_Vel(v), ++n_ns; }
  void SetNavStateRot(const SO3& r) { ns.Set_Rot(r), ++n_ns; }
  void SetNavStateDeltaBg(const Vec3& v) { ns.Set_DeltaBiasGyr(v), ++n_ns; }
  void SetNavStateDeltaBa(const Vec3& v) { ns.Set_DeltaBiasAcc(v), ++n_ns; }
  void SetPose(const float* M) { std::memcpy(T, M, sizeof T), ++n_pose; }
  std::vector<MapPoint*> GetMapPointMatches() const { return points; }
  uvo_keypoint GetKeyPointUn(size_t i) const { return keys[i]; }
  float GetInvSigma2(int octave) const { return inv_sigma2[octave]; }
  void EraseMapPointMatch(MapPoint* p) {
    const int idx = p->GetIndexInKeyFrame(this);
    if (idx >= 0) points[idx] = 0;
  }
};
struct Mutex {
  int locks, held;
  void lock() { ++locks, ++held; }
  void unlock() { --held; }
};
struct Map {
  Mutex mMutexMapUpdate;
};
struct LocalMapping {
  int flag;
  void SetMapUpdateFlagInTracking(bool b) { flag = b ? 1 : 0; }
};
bool rd(FILE* f, void* p, size_t n) { return std::fread(p, 1, n, f) == n; }
void wr(FILE* f, const void* p, size_t n) { std::fwrite(p, 1, n, f); }
void wi(FILE* f, int32_t v) { wr(f, &v, 4); }
}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t h[6];
  double dd[20];
  float gw[3], inv_sigma2[8];
  if (!rd(f, h, sizeof h) || !rd(f, dd, sizeof dd) || !rd(f, gw, sizeof gw) || !rd(f, inv_sigma2, sizeof inv_sigma2)) return 2;
  const int nKF = h[1], nMP = h[2], nW = h[3];
  std::vector<int32_t> window(nW);
  if (!rd(f, &window[0], 4 * (size_t)nW)) return 2;
  std::vector<KeyFrame> kfs(nKF);
  std::vector<MapPoint> mps(nMP);
  std::vector<std::vector<int32_t> > mp_of(nKF);
  std::vector<int32_t> prev(nKF);
  for (int k = 0; k < nKF; ++k) {
    KeyFrame& kf = kfs[k];
    int32_t id[3], n;
    double ns[22], t, pre[142];
    float K[4];
    if (!rd(f, id, 12) || !rd(f, ns, sizeof ns) || !rd(f, &t, 8) || !rd(f, K, 16) || !rd(f, pre, sizeof pre) || !rd(f, &n, 4)) return 2;
    kf.mnId = (long unsigned int)id[0], kf.bad = id[1] != 0, prev[k] = id[2], kf.mnBALocalForKF = kf.mnBAFixedForKF = 1000000, kf.n_pose = kf.n_ns = 0;
    kf.inv_sigma2 = inv_sigma2, kf.mTimeStamp = t, kf.fx = K[0], kf.fy = K[1], kf.cx = K[2], kf.cy = K[3];
    kf.ns.from(ns);
    std::memset(kf.T, 0, sizeof kf.T);
    Preint& p = kf.pre;
    p.dT = pre[0];
    std::memcpy(p.dP.v, pre + 1, 24), std::memcpy(p.dV.v, pre + 4, 24), std::memcpy(p.dR.m, pre + 7, 72), std::memcpy(p.JPg.m, pre + 16, 72), std::memcpy(p.JPa.m, pre + 25, 72);
    std::memcpy(p.JVg.m, pre + 34, 72), std::memcpy(p.JVa.m, pre + 43, 72), std::memcpy(p.JRg.m, pre + 52, 72), std::memcpy(p.cov.m, pre + 61, 648);
    kf.Depth_Vec.resize(n), kf.Depth_Vec_Time.resize(n);
    if (n && (!rd(f, &kf.Depth_Vec[0], 8 * (size_t)n) || !rd(f, &kf.Depth_Vec_Time[0], 8 * (size_t)n))) return 2;
    if (!rd(f, &n, 4)) return 2;
    for (int i = 0; i < n; ++i) {
      float xy[2];
      int32_t om[2];
      if (!rd(f, xy, 8) || !rd(f, om, 8)) return 2;
      uvo_keypoint kp;
      std::memset(&kp, 0, sizeof kp);
      kp.x = xy[0], kp.y = xy[1], kp.octave = om[0];
      kf.keys.push_back(kp);
      mp_of[k].push_back(om[1]);
    }
  }
  for (int j = 0; j < nMP; ++j) {
    int32_t b[2];
    if (!rd(f, b, 8) || !rd(f, mps[j].pos.v, 12)) return 2;
    mps[j].bad = b[0] != 0, mps[j].late = b[1] != 0, mps[j].mnBALocalForKF = 1000000, mps[j].n_set = mps[j].n_updates = 0;
  }
  std::fclose(f);
  for (int k = 0; k < nKF; ++k) {
    kfs[k].prev = prev[k] >= 0 ? &kfs[prev[k]] : 0;
    for (size_t i = 0; i < mp_of[k].size(); ++i) {
      MapPoint* p = mp_of[k][i] >= 0 ? &mps[mp_of[k][i]] : 0;
      kfs[k].points.push_back(p);
      if (p) p->obs[&kfs[k]] = i;
    }
  }
  Map map;
  map.mMutexMapUpdate.locks = map.mMutexMapUpdate.held = 0;
  LocalMapping lm;
  lm.flag = 0;
  bool stop = h[5] != 0;
  std::vector<KeyFrame*> local;
  for (int l = 0; l < nW; ++l) local.push_back(&kfs[window[l]]);
  USLAM::NavParams prm;
  std::memcpy(prm.Tbc, dd + 2, sizeof prm.Tbc);
  prm.gyr_bias_rw2 = dd[18], prm.acc_bias_rw2 = dd[19];
  Pos g = {{gw[0], gw[1], gw[2]}};

  uvo_matcher_cfg cfg = {64, 64, 1, 64, 0};
  uvo_matcher* m = 0;
  if (uvo_matcher_create(&cfg, &m) != UVO_OK) return 3;
  {
    USLAM::NavBundleAdjuster adj(m, 8, 16, 512, 4096, 16);
    if (!adj.ok()) return 3;
    const int ret = USLAM::Optimizer::LocalBundleAdjustmentNavState(&kfs[h[0]], local, &stop, &map, g, g, &lm, dd[0], dd[1], h[4], prm, adj);
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    const int32_t K = ret == 0 ? (int32_t)adj.states_out.size() - 1 : 0, P = ret == 0 ? (int32_t)adj.begin.size() - 1 : 0, E = ret == 0 ? adj.begin[P] : 0;
    const int32_t L = ret == 0 ? (int32_t)adj.links.size() - 1 : 0, D = ret == 0 ? (int32_t)adj.depth.size() - 1 : 0;
    wi(o, ret), wi(o, lm.flag), wi(o, map.mMutexMapUpdate.locks * 10 + map.mMutexMapUpdate.held), wi(o, K), wi(o, P), wi(o, E), wi(o, L), wi(o, D);
    if (ret == 0) {
      wr(o, &adj.begin[0], 4 * (size_t)(P + 1));
      if (E) wr(o, &adj.edge_kf[0], 4 * (size_t)E), wr(o, &adj.edge_index[0], 4 * (size_t)E), wr(o, &adj.excluded[0], (size_t)E), wr(o, &adj.erased[0], (size_t)E);
      for (int l = 0; l < L; ++l) wi(o, adj.links[l].kf0), wi(o, adj.links[l].kf1);
      if (D) wr(o, &adj.depth[0], sizeof(uvo_nav_ba_depth) * (size_t)D);
    }
    for (int k = 0; k < nKF; ++k) {
      wi(o, (int32_t)kfs[k].mnBALocalForKF), wi(o, (int32_t)kfs[k].mnBAFixedForKF), wi(o, kfs[k].n_pose), wi(o, kfs[k].n_ns);
      double ns[22];
      kfs[k].ns.to(ns);
      wr(o, ns, sizeof ns), wr(o, kfs[k].T, sizeof kfs[k].T);
      for (size_t i = 0; i < kfs[k].points.size(); ++i) wi(o, kfs[k].points[i] ? (int32_t)(kfs[k].points[i] - &mps[0]) : -1);
    }
    for (int j = 0; j < nMP; ++j) {
      wi(o, (int32_t)mps[j].mnBALocalForKF), wi(o, mps[j].n_set), wi(o, mps[j].n_updates);
      wr(o, mps[j].pos.v, 12);
      wi(o, (int32_t)mps[j].obs.size());
      for (std::map<KeyFrame*, size_t>::const_iterator it = mps[j].obs.begin(); it != mps[j].obs.end(); ++it) wi(o, (int32_t)(it->first - &kfs[0]));
    }
    std::fclose(o);
  }
  uvo_matcher_destroy(m);
  return 0;
}
