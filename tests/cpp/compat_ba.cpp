// Drives USLAM::Optimizer::LocalBundleAdjustment, BundleAdjustment, GlobalBundleAdjustemnt and RecoveryBundleAdjustemnt
// (include/uvo/compat/Optimizer.h) the way LocalMapping::Run and Tracking would: key frames, map points, the map and the local mapper as
// stub types, a graph with everything the gathering of src/Optimizer.cc:2149-2198 distinguishes (a bad covisible key frame, a bad map
// point, a null match, a key frame with mnId 0, fixed cameras, a bad observer); everything the call touched is written out for
// tests/test_gpu_cpp_ba.py.  Built as C++11 with -Wall -Werror, no OpenCV.
//
//   compat_ba scene.bin out.bin
// scene.bin: int32 what (0 local, 1 BundleAdjustment, 2 Global, 3 Recovery), current, other, nIterations, stop, nKF, nMP; float invLevelSigma2[8];
//            per key frame: int32 mnId, bad; float R[9] t[3] K[4]; int32 nkeys; {float x, y; int32 octave, mp} [nkeys]; int32 ncov; int32 cov[ncov];
//            per map point: int32 bad; float pos[3]
// out.bin:   int32 ret, map flag, locks, K, P, E; int32 begin[P + 1]; int32 edge_kf[E]; int32 edge_index[E]; uint8 removed1[E], removed2[E];
//            per key frame: int32 mnBALocalForKF, mnBAFixedForKF, poses set; float T[16]; int32 mp[nkeys];
//            per map point: int32 mnBALocalForKF, positions set, normal updates; float pos[3]; int32 nobs; int32 observer[nobs]
#include <cstdio>
#include <cstring>
#include <map>
#include <vector>

#include "uvo/compat/Optimizer.h"

namespace {
struct Vec {
  std::vector<float> v;
  float operator[](int i) const { return v[i]; }
};
struct KeyFrame;
struct MapPoint {
  long unsigned int mnBALocalForKF;
  bool bad;
  float pos[3];
  int n_set, n_updates;
  std::map<KeyFrame*, size_t> obs;
  bool isBad() const { return bad; }
  Vec GetWorldPos() const {
    Vec p;
    p.v.assign(pos, pos + 3);
    return p;
  }
  void SetWorldPos(const float* X) { pos[0] = X[0], pos[1] = X[1], pos[2] = X[2], ++n_set; }
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
  float T[16];
  float fx, fy, cx, cy;
  int n_set;
  std::vector<uvo_keypoint> keys;
  std::vector<MapPoint*> points;
  std::vector<KeyFrame*> cov;
  const float* inv_sigma2;
  bool isBad() const { return bad; }
  Vec GetRotation() const {
    Vec m;
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) m.v.push_back(T[4 * r + c]);
    return m;
  }
  Vec GetTranslation() const {
    Vec m;
    for (int r = 0; r < 3; ++r) m.v.push_back(T[4 * r + 3]);
    return m;
  }
  void SetPose(const float* M) { std::memcpy(T, M, sizeof T), ++n_set; }
  std::vector<KeyFrame*> GetVectorCovisibleKeyFrames() const { return cov; }
  std::vector<MapPoint*> GetMapPointMatches() const { return points; }
  std::vector<MapPoint*> getmvpMappoints() const { return points; }
  uvo_keypoint GetKeyPointUn(size_t i) const { return keys[i]; }
  float GetInvSigma2(int octave) const { return inv_sigma2[octave]; }
  void EraseMapPointMatch(MapPoint* p) {
    const int idx = p->GetIndexInKeyFrame(this);
    if (idx >= 0) points[idx] = 0;
  }
  void EraseMapPointMatch(int idx) { points[idx] = 0; }
};
struct Mutex {
  int locks, held;
  void lock() { ++locks, ++held; }
  void unlock() { --held; }
};
struct Map {
  Mutex mMutexMapUpdate;
  std::vector<KeyFrame*> kfs;
  std::vector<MapPoint*> mps;
  std::vector<KeyFrame*> GetAllKeyFrames() const { return kfs; }
  std::vector<MapPoint*> GetAllMapPoints() const { return mps; }
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
  int32_t h[7];
  float inv_sigma2[8];
  if (!rd(f, h, sizeof h) || !rd(f, inv_sigma2, sizeof inv_sigma2)) return 2;
  const int what = h[0], nKF = h[5], nMP = h[6];
  std::vector<KeyFrame> kfs(nKF);
  std::vector<MapPoint> mps(nMP);
  std::vector<std::vector<int32_t> > cov(nKF), mp_of(nKF);
  for (int k = 0; k < nKF; ++k) {
    KeyFrame& kf = kfs[k];
    int32_t id[2], n;
    float R[9], t[3], K[4];
    if (!rd(f, id, 8) || !rd(f, R, 36) || !rd(f, t, 12) || !rd(f, K, 16) || !rd(f, &n, 4)) return 2;
    kf.mnId = (long unsigned int)id[0], kf.bad = id[1] != 0, kf.mnBALocalForKF = kf.mnBAFixedForKF = 1000000, kf.n_set = 0, kf.inv_sigma2 = inv_sigma2;
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) kf.T[4 * r + c] = R[3 * r + c];
      kf.T[4 * r + 3] = t[r];
    }
    kf.T[12] = kf.T[13] = kf.T[14] = 0.f, kf.T[15] = 1.f;
    kf.fx = K[0], kf.fy = K[1], kf.cx = K[2], kf.cy = K[3];
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
    if (!rd(f, &n, 4)) return 2;
    cov[k].resize(n);
    if (n && !rd(f, &cov[k][0], 4 * (size_t)n)) return 2;
  }
  for (int j = 0; j < nMP; ++j) {
    int32_t bad;
    if (!rd(f, &bad, 4) || !rd(f, mps[j].pos, 12)) return 2;
    mps[j].bad = bad != 0, mps[j].mnBALocalForKF = 1000000, mps[j].n_set = mps[j].n_updates = 0;
  }
  std::fclose(f);
  for (int k = 0; k < nKF; ++k) {
    for (size_t c = 0; c < cov[k].size(); ++c) kfs[k].cov.push_back(&kfs[cov[k][c]]);
    for (size_t i = 0; i < mp_of[k].size(); ++i) {
      MapPoint* p = mp_of[k][i] >= 0 ? &mps[mp_of[k][i]] : 0;
      kfs[k].points.push_back(p);
      if (p) p->obs[&kfs[k]] = i;
    }
  }
  Map map;
  map.mMutexMapUpdate.locks = map.mMutexMapUpdate.held = 0;
  for (int k = 0; k < nKF; ++k) map.kfs.push_back(&kfs[k]);
  for (int j = 0; j < nMP; ++j) map.mps.push_back(&mps[j]);
  LocalMapping lm;
  lm.flag = 0;
  bool stop = h[4] != 0;

  uvo_matcher_cfg cfg = {64, 64, 1, 64, 0};
  uvo_matcher* m = 0;
  if (uvo_matcher_create(&cfg, &m) != UVO_OK) return 3;
  int ret;
  {
    USLAM::BundleAdjuster adj(m, 16, 16, 512, 4096);
    if (!adj.ok()) return 3;
    if (what == 0) ret = USLAM::Optimizer::LocalBundleAdjustment(&kfs[h[1]], &stop, &map, &lm, adj);
    else if (what == 1) ret = USLAM::Optimizer::BundleAdjustment(map.kfs, map.mps, h[3], &stop, adj);
    else if (what == 2) ret = USLAM::Optimizer::GlobalBundleAdjustemnt(&map, h[3], &stop, adj);
    else ret = USLAM::Optimizer::RecoveryBundleAdjustemnt(&kfs[h[2]], &kfs[h[1]], h[3], &stop, adj);
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    const int32_t K = ret == 0 ? adj.result.kf_Tcw ? (int32_t)(adj.Tcw_out.size() / 16) : 0 : 0;
    const int32_t P = ret == 0 ? (int32_t)adj.begin.size() - 1 : 0, E = ret == 0 ? adj.begin[P] : 0;
    wi(o, ret), wi(o, lm.flag), wi(o, map.mMutexMapUpdate.locks * 10 + map.mMutexMapUpdate.held), wi(o, K), wi(o, P), wi(o, E);
    if (ret == 0) {
      wr(o, &adj.begin[0], 4 * (size_t)(P + 1));
      if (E) wr(o, &adj.edge_kf[0], 4 * (size_t)E), wr(o, &adj.edge_index[0], 4 * (size_t)E), wr(o, &adj.removed1[0], (size_t)E), wr(o, &adj.removed2[0], (size_t)E);
    }
    for (int k = 0; k < nKF; ++k) {
      wi(o, (int32_t)kfs[k].mnBALocalForKF), wi(o, (int32_t)kfs[k].mnBAFixedForKF), wi(o, kfs[k].n_set);
      wr(o, kfs[k].T, sizeof kfs[k].T);
      for (size_t i = 0; i < kfs[k].points.size(); ++i) wi(o, kfs[k].points[i] ? (int32_t)(kfs[k].points[i] - &mps[0]) : -1);
    }
    for (int j = 0; j < nMP; ++j) {
      wi(o, (int32_t)mps[j].mnBALocalForKF), wi(o, mps[j].n_set), wi(o, mps[j].n_updates);
      wr(o, mps[j].pos, 12);
      wi(o, (int32_t)mps[j].obs.size());
      for (std::map<KeyFrame*, size_t>::const_iterator it = mps[j].obs.begin(); it != mps[j].obs.end(); ++it) wi(o, (int32_t)(it->first - &kfs[0]));
    }
    std::fclose(o);
  }
  uvo_matcher_destroy(m);
  return 0;
}
