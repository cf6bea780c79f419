// Drives USLAM::Optimizer::OptimizeSim3 (include/uvo/compat/Optimizer.h) the way LoopClosing::ComputeSim3 would: key frames and map
// points as stub types, vpMatches1 with every kind of entry the walk of src/Optimizer.cc:2713-2792 distinguishes, first all candidates
// through the list overload (one device call), then each through the single call on a fresh copy; everything they touched is written
// out for tests/test_gpu_cpp_sim3opt.py.  Built as C++11 with -Wall -Werror, no OpenCV.
//
//   compat_sim3opt scene.bin out.bin
// scene.bin: int32 candidates; float th2; float levelSigma2[8]; float invLevelSigma2[8]; key frame 1: float R[9] t[3] K[4]; int32 N;
//            {int32 kind; float x1w[3]; float kp1[2]; int32 octave1} [N]          kind: 1 a point, 2 pMP1 null, 3 pMP1 bad
//            per candidate: key frame 2: float R[9] t[3] K[4]; float R12[9] t12[3] s12;
//            {int32 kind; float x2w[3]; float kp2[2]; int32 octave2} [N]          kind: 0 vpMatches1[i] null, 1 a match, 4 pMP2 bad,
//                                                                                        5 pMP2 not in key frame 2 (i2 = -1)
// out.bin:   twice (list overload, single calls), per candidate: int32 ret; double q[4] t[3] s; uint8 is_null[N]
#include <cstdio>
#include <cstring>
#include <vector>

#include "uvo/compat/Optimizer.h"

namespace {
struct Vec {
  std::vector<float> v;
  float operator[](int i) const { return v[i]; }
};
struct KeyFrame;
struct MapPoint {
  float pos[3];
  bool bad;
  const KeyFrame* in;  // the key frame it is observed in
  int index;           // and where
  bool isBad() const { return bad; }
  Vec GetWorldPos() const {
    Vec p;
    p.v.assign(pos, pos + 3);
    return p;
  }
  int GetIndexInKeyFrame(const KeyFrame* kf) const { return kf == in ? index : -1; }
};
struct KeyFrame {
  float R[9], t[3];
  float fx, fy, cx, cy;
  std::vector<uvo_keypoint> keys;
  std::vector<MapPoint*> points;
  const float *sigma2, *inv_sigma2;
  Vec GetRotation() const {
    Vec m;
    m.v.assign(R, R + 9);
    return m;
  }
  Vec GetTranslation() const {
    Vec m;
    m.v.assign(t, t + 3);
    return m;
  }
  std::vector<MapPoint*> GetMapPointMatches() const { return points; }
  uvo_keypoint GetKeyPointUn(int i) const { return keys[i]; }
  float GetSigma2(int octave) const { return sigma2[octave]; }
  float GetInvSigma2(int octave) const { return inv_sigma2[octave]; }
};
struct Rec {
  int32_t kind;
  float xw[3], kp[2];
  int32_t octave;
};
struct Candidate {
  KeyFrame kf2;
  std::vector<MapPoint> mp2;
  std::vector<MapPoint*> matches;
  float R12[9], t12[3], s12;
};
bool rd(FILE* f, void* p, size_t n) { return std::fread(p, 1, n, f) == n; }
bool read_kf(FILE* f, KeyFrame& k) {
  float K[4];
  if (!rd(f, k.R, 36) || !rd(f, k.t, 12) || !rd(f, K, 16)) return false;
  k.fx = K[0], k.fy = K[1], k.cx = K[2], k.cy = K[3];
  return true;
}
void write_out(FILE* o, int32_t ret, const USLAM::Sim3& S, const std::vector<MapPoint*>& m) {
  std::fwrite(&ret, 4, 1, o);
  std::fwrite(S.quaternion(), 8, 4, o);
  const USLAM::Sim3::Vector3 t = S.translation();
  std::fwrite(t.v, 8, 3, o);
  const double s = S.scale();
  std::fwrite(&s, 8, 1, o);
  for (size_t i = 0; i < m.size(); ++i) {
    const uint8_t b = m[i] ? 0 : 1;
    std::fwrite(&b, 1, 1, o);
  }
}
}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t count = 0, N = 0;
  float th2, sigma2[8], inv_sigma2[8];
  KeyFrame kf1;
  if (!rd(f, &count, 4) || count < 0 || count > 64 || !rd(f, &th2, 4) || !rd(f, sigma2, 32) || !rd(f, inv_sigma2, 32) || !read_kf(f, kf1)) return 2;
  if (!rd(f, &N, 4) || N < 0 || N > 16384) return 2;
  kf1.sigma2 = sigma2, kf1.inv_sigma2 = inv_sigma2;
  std::vector<MapPoint> mp1(N);
  kf1.keys.resize(N), kf1.points.assign(N, (MapPoint*)0);
  for (int i = 0; i < N; ++i) {
    Rec r;
    if (!rd(f, &r, sizeof r)) return 2;
    std::memcpy(mp1[i].pos, r.xw, 12);
    mp1[i].bad = r.kind == 3, mp1[i].in = &kf1, mp1[i].index = i;
    uvo_keypoint k = uvo_keypoint();
    k.x = r.kp[0], k.y = r.kp[1], k.octave = r.octave;
    kf1.keys[i] = k;
    if (r.kind != 2) kf1.points[i] = &mp1[i];
  }
  std::vector<Candidate> C(count);
  for (int j = 0; j < count; ++j) {
    Candidate& c = C[j];
    if (!read_kf(f, c.kf2) || !rd(f, c.R12, 36) || !rd(f, c.t12, 12) || !rd(f, &c.s12, 4)) return 2;
    c.kf2.sigma2 = sigma2, c.kf2.inv_sigma2 = inv_sigma2;
    c.mp2.resize(N), c.matches.assign(N, (MapPoint*)0), c.kf2.keys.resize(N);
    for (int i = 0; i < N; ++i) {
      Rec r;
      if (!rd(f, &r, sizeof r)) return 2;
      std::memcpy(c.mp2[i].pos, r.xw, 12);
      c.mp2[i].bad = r.kind == 4, c.mp2[i].in = r.kind == 5 ? (const KeyFrame*)0 : &c.kf2, c.mp2[i].index = i;
      uvo_keypoint k = uvo_keypoint();
      k.x = r.kp[0], k.y = r.kp[1], k.octave = r.octave;
      c.kf2.keys[i] = k;
      if (r.kind != 0) c.matches[i] = &c.mp2[i];
    }
  }
  std::fclose(f);

  uvo_matcher_cfg cfg = {64, 64, 1, 64, 0};
  uvo_matcher* m = 0;
  if (uvo_matcher_create(&cfg, &m) != UVO_OK) {
    std::fprintf(stderr, "%s\n", uvo_last_error());
    return 1;
  }
  FILE* o = std::fopen(argv[2], "wb");
  if (!o) return 2;
  int rets = 0;
  {
    USLAM::Sim3Optimizer opt(m, count > 0 ? count : 1, N > 0 ? N : 1);
    if (!opt.ok()) {
      std::fprintf(stderr, "%s\n", uvo_last_error());
      return 1;
    }
    // the list overload: one call
    std::vector<std::vector<MapPoint*> > matches(count);
    std::vector<USLAM::Sim3> sims;
    std::vector<KeyFrame*> kf2s;
    std::vector<int> inl;
    for (int j = 0; j < count; ++j) {
      matches[j] = C[j].matches;
      sims.push_back(USLAM::Sim3(C[j].R12, C[j].t12, C[j].s12));
      kf2s.push_back(&C[j].kf2);
    }
    if (USLAM::Optimizer::OptimizeSim3(opt, &kf1, kf2s, matches, sims, th2, inl) != 0) {
      std::fprintf(stderr, "%s\n", uvo_last_error());
      return 1;
    }
    for (int j = 0; j < count; ++j) write_out(o, inl[j], sims[j], matches[j]), rets += inl[j];
    // the single calls, on fresh copies
    for (int j = 0; j < count; ++j) {
      std::vector<MapPoint*> mj = C[j].matches;
      USLAM::Sim3 S(C[j].R12, C[j].t12, C[j].s12);
      const int ret = USLAM::Optimizer::OptimizeSim3(opt, &kf1, &C[j].kf2, mj, S, th2);
      if (ret < 0) {
        std::fprintf(stderr, "%s\n", uvo_last_error());
        return 1;
      }
      write_out(o, ret, S, mj);
    }
  }
  uvo_matcher_destroy(m);
  std::fclose(o);
  std::printf("{\"candidates\": %d, \"inliers\": %d}\n", count, rets);
  return 0;
}
