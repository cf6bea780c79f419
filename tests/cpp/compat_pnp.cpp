// Drives USLAM::solvePnPRansac (include/uvo/compat/SolvePnPRansac.h) the way Tracking::TrackWithPnP would, on a scene written by
// tests/test_gpu_cpp_pnp.py.
//   compat_pnp scene.bin out.bin
// scene.bin: int32 n, n_dist; float fx, fy, cx, cy, dist[8]; n x float[3] map points; n x float[2] image points.
// out.bin: int32 ok, n_inliers; double rvec[3], tvec[3]; float Tcw[16]; n_inliers x int32.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "uvo/compat/SolvePnPRansac.h"

namespace {
struct Point3f {
  float x, y, z;
};
struct Point2f {
  float x, y;
};
}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t n = 0, n_dist = 0;
  uvo_camera_model cam = uvo_camera_model();
  bool ok = std::fread(&n, 4, 1, f) == 1 && std::fread(&n_dist, 4, 1, f) == 1 && std::fread(&cam.fx, 4, 4, f) == 4 && std::fread(cam.dist, 4, 8, f) == 8;
  cam.n_dist = n_dist;
  std::vector<Point3f> mappts(n);
  std::vector<Point2f> pts(n);
  ok = ok && (n == 0 || (std::fread(&mappts[0], 12, n, f) == (size_t)n && std::fread(&pts[0], 8, n, f) == (size_t)n));
  std::fclose(f);
  if (!ok) return 2;
  uvo_klt_cfg cfg = {64, 64, 3, 21, 21, n > 16 ? n : 16, 2, 0};
  uvo_klt* klt = 0;
  if (uvo_klt_create(&cfg, &klt) != UVO_OK) {
    std::fprintf(stderr, "%s\n", uvo_last_error());
    return 1;
  }
  double Rvec[3], Tvec[3];
  float Tcw[16];
  std::vector<int> mask_pnp;
  const bool found = USLAM::solvePnPRansac(klt, mappts, pts, cam, Rvec, Tvec, false, 300, 3, 0.99, mask_pnp, Tcw);
  uvo_klt_destroy(klt);
  FILE* o = std::fopen(argv[2], "wb");
  if (!o) return 2;
  const int32_t head[2] = {found ? 1 : 0, (int32_t)mask_pnp.size()};
  std::fwrite(head, 4, 2, o);
  std::fwrite(Rvec, 8, 3, o);
  std::fwrite(Tvec, 8, 3, o);
  std::fwrite(Tcw, 4, 16, o);
  if (!mask_pnp.empty()) std::fwrite(&mask_pnp[0], 4, mask_pnp.size(), o);
  std::fclose(o);
  std::printf("{\"ok\": %d, \"inliers\": %d}\n", head[0], head[1]);
  return 0;
}
