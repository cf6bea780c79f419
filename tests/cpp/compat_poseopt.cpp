// Drives USLAM::Optimizer::PoseOptimization (include/uvo/compat/Optimizer.h) the way Tracking::TrackLocalMap would: a frame whose
// mvpMapPoints has gaps, mvbOutlier pre-set to a pattern, one call, everything it touched written out for tests/test_gpu_cpp_poseopt.py.
// Built as C++11 with -Wall -Werror, no OpenCV.
//
//   compat_poseopt scene.bin out.bin
// scene.bin: int32 nkeys; float fx fy cx cy; float invLevelSigma2[8]; float Tcw[16]; uvo_keypoint keys[nkeys];
//            {int32 has; float xyz[3]} [nkeys]; uint8 outlier_before[nkeys]
// out.bin:   int32 ret; float Tcw[16]; uint8 outlier_after[nkeys]
#include <cstdio>
#include <cstring>
#include <vector>

#include "uvo/compat/Optimizer.h"

namespace {
struct Pos {
  float v[3];
  float operator[](int i) const { return v[i]; }
};
struct MapPoint {
  Pos pos;
  Pos GetWorldPos() const { return pos; }
};
struct Frame {
  std::vector<MapPoint*> mvpMapPoints;
  std::vector<uvo_keypoint> mvKeysUn;
  std::vector<float> mvInvLevelSigma2;
  std::vector<bool> mvbOutlier;
  float mTcw[16];
  float fx, fy, cx, cy;
};
bool rd(FILE* f, void* p, size_t n) { return std::fread(p, 1, n, f) == n; }
}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t nkeys = 0;
  Frame F;
  F.mvInvLevelSigma2.resize(8);
  float K[4];
  if (!rd(f, &nkeys, 4) || nkeys < 0 || !rd(f, K, 16) || !rd(f, &F.mvInvLevelSigma2[0], 32) || !rd(f, F.mTcw, 64)) return 2;
  F.fx = K[0], F.fy = K[1], F.cx = K[2], F.cy = K[3];
  F.mvKeysUn.resize(nkeys);
  std::vector<MapPoint> store(nkeys);
  F.mvpMapPoints.assign(nkeys, (MapPoint*)0);
  if (nkeys && !rd(f, &F.mvKeysUn[0], sizeof(uvo_keypoint) * (size_t)nkeys)) return 2;
  for (int i = 0; i < nkeys; ++i) {
    struct {
      int32_t has;
      float p[3];
    } rec;
    if (!rd(f, &rec, sizeof rec)) return 2;
    std::memcpy(store[i].pos.v, rec.p, 12);
    if (rec.has) F.mvpMapPoints[i] = &store[i];
  }
  std::vector<uint8_t> before(nkeys ? nkeys : 1);
  if (nkeys && !rd(f, &before[0], (size_t)nkeys)) return 2;
  std::fclose(f);
  F.mvbOutlier.assign(before.begin(), before.begin() + nkeys);

  uvo_klt_cfg cfg = {64, 64, 3, 21, 21, 16, 2, 0};
  uvo_klt* klt = 0;
  if (uvo_klt_create(&cfg, &klt) != UVO_OK) {
    std::fprintf(stderr, "%s\n", uvo_last_error());
    return 1;
  }
  int32_t ret;
  {
    USLAM::PoseOptimizer opt(klt, nkeys > 0 ? nkeys : 1);
    if (!opt.ok()) {
      std::fprintf(stderr, "%s\n", uvo_last_error());
      return 1;
    }
    ret = USLAM::Optimizer::PoseOptimization(opt, &F);
    if (ret < 0) {
      std::fprintf(stderr, "%s\n", uvo_last_error());
      return 1;
    }
  }
  uvo_klt_destroy(klt);
  FILE* o = std::fopen(argv[2], "wb");
  if (!o) return 2;
  std::fwrite(&ret, 4, 1, o);
  std::fwrite(F.mTcw, 4, 16, o);
  for (int i = 0; i < nkeys; ++i) {
    const uint8_t b = F.mvbOutlier[i] ? 1 : 0;
    std::fwrite(&b, 1, 1, o);
  }
  std::fclose(o);
  std::printf("{\"ret\": %d}\n", ret);
  return 0;
}
