// Drives USLAM::Initializer (include/uvo/compat/Initializer.h) the way Tracking::Initialize would (src/Tracking.cc:1340), on scenes
// written by tests/test_gpu_cpp_initializer.py: the constructor on the reference frame, then Initialize on each current frame in turn,
// all on one device object, so the generator runs on from call to call.
//   compat_initializer scene.bin out.bin
// scene.bin: int32 n1, calls; float fx, fy, cx, cy; n1 x (x, y); per call: int32 n2; n2 x (x, y); n2 x int32 vMatches12.
// out.bin, per call: int32 ok, R21 empty, t21 empty, n2; float R21[9], t21[3] (zeros when empty); n2 x float[3] vP3D; n2 x uint8 vbTriangulated.
//
// Compiled against tests/cpp/opencv_decl_stub, which only DECLARES cv::Mat: the members this program calls are defined below, and
// cv::Point3f, which the stub lacks, is declared before the adaptor is read.
#include <opencv2/core/core.hpp>

namespace cv {
template <class T>
struct Point3_ {
  T x, y, z;
};
typedef Point3_<float> Point3f;
}  // namespace cv

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "uvo/compat/Initializer.h"

namespace cv {
// a Mat of floats that owns nothing: the driver's few matrices live until it exits
Mat::Mat() : rows(0), cols(0), data(0) {}
Mat::Mat(int r, int c, int) : rows(r), cols(c), data(reinterpret_cast<uchar*>(new float[(size_t)r * c]())) {}
bool Mat::empty() const { return data == 0; }
template <>
float& Mat::at<float>(int r) {
  return reinterpret_cast<float*>(data)[r];
}
template <>
float& Mat::at<float>(int r, int c) {
  return reinterpret_cast<float*>(data)[r * cols + c];
}
template <>
const float& Mat::at<float>(int r, int c) const {
  return reinterpret_cast<const float*>(data)[r * cols + c];
}
}  // namespace cv

namespace {
struct FrameKTL {
  cv::Mat mK;
  std::vector<cv::KeyPoint> mvKeysUn;
};
bool get(FILE* f, void* p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }
void read_keys(FILE* f, int n, std::vector<cv::KeyPoint>& out) {
  std::vector<float> xy(2 * (size_t)n + 1);
  if (!get(f, &xy[0], (size_t)n * 8)) exit(3);
  out.assign(n, cv::KeyPoint());
  for (int i = 0; i < n; ++i) out[i].pt.x = xy[2 * i], out[i].pt.y = xy[2 * i + 1];
}
}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  int32_t n1, calls;
  float k[4];
  if (!get(in, &n1, 4) || !get(in, &calls, 4) || !get(in, k, 16)) return 3;
  FrameKTL mInitialFrame;
  mInitialFrame.mK = cv::Mat(3, 3, CV_32F);
  mInitialFrame.mK.at<float>(0, 0) = k[0], mInitialFrame.mK.at<float>(1, 1) = k[1], mInitialFrame.mK.at<float>(0, 2) = k[2], mInitialFrame.mK.at<float>(1, 2) = k[3];
  mInitialFrame.mK.at<float>(2, 2) = 1.f;
  read_keys(in, n1, mInitialFrame.mvKeysUn);
  uvo_klt_cfg cfg = {64, 64, 1, 21, 21, 256, 2, 0};
  uvo_klt* klt = 0;
  if (uvo_klt_create(&cfg, &klt) != UVO_OK) {
    fprintf(stderr, "uvo_klt_create: %s\n", uvo_last_error());
    return 4;
  }
  {
    USLAM::InitializerDevice initDevice(klt, 2048);
    USLAM::Initializer* mpInitializer = new USLAM::Initializer(initDevice, mInitialFrame, 1.0, 200);
    for (int c = 0; c < calls; ++c) {
      int32_t n2;
      if (!get(in, &n2, 4)) return 3;
      FrameKTL mCurrentFrame;
      read_keys(in, n2, mCurrentFrame.mvKeysUn);
      std::vector<int32_t> m(n2 + 1);
      if (!get(in, &m[0], (size_t)n2 * 4)) return 3;
      std::vector<int> mvIniMatches(m.begin(), m.begin() + n2);
      cv::Mat Rcw, tcw;
      std::vector<cv::Point3f> mvIniP3D(n2);
      std::vector<bool> vbTriangulated(n2, false);
      for (int i = 0; i < n2; ++i) mvIniP3D[i].x = mvIniP3D[i].y = mvIniP3D[i].z = 0.f;
      const bool ok = mpInitializer->Initialize(mCurrentFrame, mvIniMatches, Rcw, tcw, mvIniP3D, vbTriangulated);
      const int32_t head[4] = {ok ? 1 : 0, Rcw.empty() ? 1 : 0, tcw.empty() ? 1 : 0, n2};
      float pose[12] = {0};
      if (!Rcw.empty() && !tcw.empty())
        for (int r = 0; r < 3; ++r) {
          for (int cc = 0; cc < 3; ++cc) pose[3 * r + cc] = Rcw.at<float>(r, cc);
          pose[9 + r] = tcw.at<float>(r);
        }
      fwrite(head, 4, 4, out);
      fwrite(pose, 4, 12, out);
      for (int i = 0; i < n2; ++i) fwrite(&mvIniP3D[i], 4, 3, out);
      for (int i = 0; i < n2; ++i) fputc(vbTriangulated[i] ? 1 : 0, out);
      printf("call %d: ok %d, nGood %d %d %d %d\n", c, (int)ok, mpInitializer->last().n_good[0], mpInitializer->last().n_good[1], mpInitializer->last().n_good[2],
             mpInitializer->last().n_good[3]);
    }
    delete mpInitializer;
  }
  uvo_klt_destroy(klt);
  fclose(in);
  fclose(out);
  return 0;
}
