// Drives USLAM::ORBmatcher::CreateNewMapPoints (include/uvo/compat/ORBmatcher.h) the way LocalMapping::CreateNewMapPoints would, on a
// scene written by tests/test_gpu_cpp_newpoints.py, and -- for comparison and timing -- the loop the adaptors offered before it:
// SearchForTriangulationBegin, then per neighbour SearchForTriangulationNext + the triangulation of src/LocalMapping.cc:1096-1180 on
// the host in fp32 (the same restatement of OpenCV's one-sided Jacobi SVD as csrc/triangulate.hip) + AddMapPoint.
//
//   compat_newpoints scene.bin out.bin [reps]
// scene.bin: int32 check_orientation, n_kf; per key frame (the first is key frame 1): int32 n, nlevels; float R[9], t[3], ow[3], fx, fy,
//   cx, cy; float scale[nlevels], sigma2[nlevels]; n key points (28 B); n descriptors (32 B); n has-map-point bytes; n int32 vocabulary
//   nodes; float F12[9] (unused for key frame 1).
// out.bin: for the one call, then for the host loop: per neighbour int32 count, count x {int32 idx1, idx2; float x3D[3]}.
// stdout: one JSON line with the median wall time of both ways over `reps` repetitions.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>

#include "uvo/compat/ORBmatcher.h"

namespace {
struct Mat {  // cv::Mat stand-in: up to 3x3 CV_32F
  float m[3][3];
  template <class T>
  T at(int r, int c) const { return m[r][c]; }
  template <class T>
  T at(int r) const { return m[r][0]; }
};
struct Desc1 {
  const uint8_t* p;
  const uint8_t* ptr(int) const { return p; }
};
struct MapPoint {};
struct KeyFrame {
  int N = 0;
  std::vector<uvo_keypoint> keys;
  std::vector<uint8_t> desc;
  std::vector<MapPoint*> mps;
  std::map<unsigned, std::vector<unsigned> > featvec;
  std::vector<float> scale, sigma2;
  Mat R, t3, ow, F12;
  float fx, fy, cx, cy;
  std::vector<MapPoint*> GetMapPointMatches() const { return mps; }
  std::vector<uvo_keypoint> GetKeyPointsUn() const { return keys; }
  uvo_keypoint GetKeyPointUn(int i) const { return keys[i]; }
  Desc1 GetDescriptor(int i) const { return Desc1{&desc[(size_t)i * 32]}; }
  const std::map<unsigned, std::vector<unsigned> >& GetFeatureVector() const { return featvec; }
  int GetScaleLevels() const { return (int)scale.size(); }
  float GetSigma2(int l) const { return sigma2[l]; }
  std::vector<float> GetScaleFactors() const { return scale; }
  Mat GetRotation() const { return R; }
  Mat GetTranslation() const { return t3; }
  Mat GetCameraCenter() const { return ow; }
  void AddMapPoint(MapPoint* p, int i) { mps[i] = p; }
};

template <class T>
bool rd(FILE* f, T* dst, size_t n) { return fread(dst, sizeof(T), n, f) == n; }

// vt.row(3) of OpenCV 3.4's JacobiSVDImpl_<float> on a 4 x 4 matrix [OCV-RECALL]; as svd4_last_row in csrc/triangulate.hip
void svd4_last_row(const float A[4][4], float v[4]) {
  float At[4][4], Vt[4][4];
  double W[4];
  const float eps = 1.1920928955078125e-7f * 2;
  for (int i = 0; i < 4; ++i) {
    double sd = 0;
    for (int k = 0; k < 4; ++k) {
      At[i][k] = A[k][i];
      sd += (double)At[i][k] * (double)At[i][k];
      Vt[i][k] = i == k ? 1.f : 0.f;
    }
    W[i] = sd;
  }
  for (int iter = 0; iter < 30; ++iter) {
    bool changed = false;
    for (int i = 0; i < 3; ++i)
      for (int j = i + 1; j < 4; ++j) {
        double a = W[i], p = 0, b = W[j];
        for (int k = 0; k < 4; ++k) p += (double)At[i][k] * (double)At[j][k];
        if (std::fabs(p) <= (double)eps * std::sqrt(a * b)) continue;
        p *= 2;
        const double beta = a - b, gamma = hypot(p, beta);
        float c, s;
        if (beta < 0) {
          const double delta = (gamma - beta) * 0.5;
          s = (float)std::sqrt(delta / gamma);
          c = (float)(p / (gamma * (double)s * 2));
        } else {
          c = (float)std::sqrt((gamma + beta) / (gamma * 2));
          s = (float)(p / (gamma * (double)c * 2));
        }
        a = b = 0;
        for (int k = 0; k < 4; ++k) {
          const float t0 = c * At[i][k] + s * At[j][k], t1 = -s * At[i][k] + c * At[j][k];
          At[i][k] = t0, At[j][k] = t1;
          a += (double)t0 * (double)t0, b += (double)t1 * (double)t1;
        }
        W[i] = a, W[j] = b;
        changed = true;
        for (int k = 0; k < 4; ++k) {
          const float t0 = c * Vt[i][k] + s * Vt[j][k], t1 = -s * Vt[i][k] + c * Vt[j][k];
          Vt[i][k] = t0, Vt[j][k] = t1;
        }
      }
    if (!changed) break;
  }
  for (int i = 0; i < 4; ++i) {
    double sd = 0;
    for (int k = 0; k < 4; ++k) sd += (double)At[i][k] * (double)At[i][k];
    W[i] = std::sqrt(sd);
  }
  for (int i = 0; i < 3; ++i) {
    int j = i;
    for (int k = i + 1; k < 4; ++k)
      if (W[j] < W[k]) j = k;
    if (i != j) {
      std::swap(W[i], W[j]);
      for (int k = 0; k < 4; ++k) std::swap(Vt[i][k], Vt[j][k]);
    }
  }
  for (int k = 0; k < 4; ++k) v[k] = Vt[3][k];
}
double dot3(const float* a, const float* b) { return (double)a[0] * (double)b[0] + (double)a[1] * (double)b[1] + (double)a[2] * (double)b[2]; }

// src/LocalMapping.cc:1106-1180 on the host in fp32: true = "Triangulation is succesfull"
bool triangulate(const KeyFrame& K1, const KeyFrame& K2, const uvo_keypoint& kp1, const uvo_keypoint& kp2, float ratioFactor, float* X) {
  const float invfx1 = 1.0f / K1.fx, invfy1 = 1.0f / K1.fy, invfx2 = 1.0f / K2.fx, invfy2 = 1.0f / K2.fy;
  const float xn1[3] = {(kp1.x - K1.cx) * invfx1, (kp1.y - K1.cy) * invfy1, 1.0f}, xn2[3] = {(kp2.x - K2.cx) * invfx2, (kp2.y - K2.cy) * invfy2, 1.0f};
  float ray1[3], ray2[3];
  for (int i = 0; i < 3; ++i) {
    ray1[i] = K1.R.m[0][i] * xn1[0] + K1.R.m[1][i] * xn1[1] + K1.R.m[2][i] * xn1[2];
    ray2[i] = K2.R.m[0][i] * xn2[0] + K2.R.m[1][i] * xn2[1] + K2.R.m[2][i] * xn2[2];
  }
  const float cosParallaxRays = (float)(dot3(ray1, ray2) / (std::sqrt(dot3(ray1, ray1)) * std::sqrt(dot3(ray2, ray2))));
  if (cosParallaxRays < 0 || cosParallaxRays > 0.9998) return false;
  float A[4][4];
  for (int k = 0; k < 4; ++k) {
    const float a0 = k < 3 ? K1.R.m[0][k] : K1.t3.m[0][0], a1 = k < 3 ? K1.R.m[1][k] : K1.t3.m[1][0], a2 = k < 3 ? K1.R.m[2][k] : K1.t3.m[2][0];
    const float b0 = k < 3 ? K2.R.m[0][k] : K2.t3.m[0][0], b1 = k < 3 ? K2.R.m[1][k] : K2.t3.m[1][0], b2 = k < 3 ? K2.R.m[2][k] : K2.t3.m[2][0];
    A[0][k] = xn1[0] * a2 - a0, A[1][k] = xn1[1] * a2 - a1, A[2][k] = xn2[0] * b2 - b0, A[3][k] = xn2[1] * b2 - b1;
  }
  float v[4];
  svd4_last_row(A, v);
  if (v[3] == 0) return false;
  const float rinv = (float)(1.0 / (double)v[3]);
  X[0] = v[0] * rinv, X[1] = v[1] * rinv, X[2] = v[2] * rinv;
  const KeyFrame* K[2] = {&K1, &K2};
  const uvo_keypoint* kp[2] = {&kp1, &kp2};
  float z[2];
  for (int c = 0; c < 2; ++c) {
    z[c] = (float)(dot3(K[c]->R.m[2], X) + (double)K[c]->t3.m[2][0]);
    if (z[c] <= 0) return false;
  }
  for (int c = 0; c < 2; ++c) {
    const float x = (float)(dot3(K[c]->R.m[0], X) + (double)K[c]->t3.m[0][0]), y = (float)(dot3(K[c]->R.m[1], X) + (double)K[c]->t3.m[1][0]);
    const float invz = (float)(1.0 / (double)z[c]);
    const float u = K[c]->fx * x * invz + K[c]->cx, w = K[c]->fy * y * invz + K[c]->cy;
    const float ex = u - kp[c]->x, ey = w - kp[c]->y;
    if ((ex * ex + ey * ey) > 5.991 * K[c]->sigma2[kp[c]->octave]) return false;
  }
  const float n1[3] = {X[0] - K1.ow.m[0][0], X[1] - K1.ow.m[1][0], X[2] - K1.ow.m[2][0]}, n2[3] = {X[0] - K2.ow.m[0][0], X[1] - K2.ow.m[1][0], X[2] - K2.ow.m[2][0]};
  const float dist1 = (float)std::sqrt(dot3(n1, n1)), dist2 = (float)std::sqrt(dot3(n2, n2));
  if (dist1 == 0 || dist2 == 0) return false;
  const float ratioDist = dist1 / dist2, ratioOctave = K1.scale[kp1.octave] / K2.scale[kp2.octave];
  return !(ratioDist * ratioFactor < ratioOctave || ratioDist > ratioOctave * ratioFactor);
}

typedef USLAM::ORBmatcher::NewMapPoint NewMapPoint;
void dump(FILE* f, const std::vector<std::vector<NewMapPoint> >& v) {
  for (size_t k = 0; k < v.size(); ++k) {
    const int32_t n = (int32_t)v[k].size();
    fwrite(&n, 4, 1, f);
    for (int j = 0; j < n; ++j) {
      const int32_t ij[2] = {(int32_t)v[k][j].idx1, (int32_t)v[k][j].idx2};
      fwrite(ij, 4, 2, f);
      fwrite(v[k][j].x3D, 4, 3, f);
    }
  }
}
double median(std::vector<double> v) {
  std::sort(v.begin(), v.end());
  return v[v.size() / 2];
}
}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  const int reps = argc > 3 ? atoi(argv[3]) : 1;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t ori = 0, nkf = 0;
  if (!rd(f, &ori, 1) || !rd(f, &nkf, 1) || nkf < 1 || nkf > 4097) return 2;
  std::vector<KeyFrame> kfs(nkf);
  for (int k = 0; k < nkf; ++k) {
    KeyFrame& K = kfs[k];
    int32_t n = 0, nl = 0;
    if (!rd(f, &n, 1) || !rd(f, &nl, 1) || n < 0 || n > 65535 || nl < 1 || nl > 64) return 2;
    float pose[19];
    if (!rd(f, pose, 19)) return 2;
    memset(&K.R, 0, sizeof(Mat)), memset(&K.t3, 0, sizeof(Mat)), memset(&K.ow, 0, sizeof(Mat));
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) K.R.m[r][c] = pose[3 * r + c];
      K.t3.m[r][0] = pose[9 + r], K.ow.m[r][0] = pose[12 + r];
    }
    K.fx = pose[15], K.fy = pose[16], K.cx = pose[17], K.cy = pose[18];
    K.N = n, K.scale.resize(nl), K.sigma2.resize(nl), K.keys.resize(n), K.desc.resize((size_t)n * 32), K.mps.assign(n, nullptr);
    std::vector<uint8_t> has(n);
    std::vector<int32_t> node(n);
    if (!rd(f, K.scale.data(), nl) || !rd(f, K.sigma2.data(), nl) || !rd(f, K.keys.data(), n) || !rd(f, K.desc.data(), (size_t)n * 32) || !rd(f, has.data(), n) ||
        !rd(f, node.data(), n) || !rd(f, &K.F12.m[0][0], 9))
      return 2;
    static MapPoint some_point;
    for (int i = 0; i < n; ++i) {
      if (has[i]) K.mps[i] = &some_point;
      K.featvec[(unsigned)node[i]].push_back((unsigned)i);
    }
  }
  fclose(f);
  std::vector<KeyFrame*> neigh;
  std::vector<Mat> vF12;
  for (int k = 1; k < nkf; ++k) neigh.push_back(&kfs[k]), vF12.push_back(kfs[k].F12);
  const std::vector<MapPoint*> mps0 = kfs[0].mps;
  const float ratioFactor = 1.5f * kfs[0].scale[1];
  USLAM::ORBmatcher matcher(0.6f, ori != 0);
  std::vector<std::vector<NewMapPoint> > one, host;
  std::vector<double> t_one, t_host;
  static MapPoint created;
  for (int rep = 0; rep < reps + 1; ++rep) {  // the first repetition warms the handle up and is not timed
    // ---- the one call
    kfs[0].mps = mps0;
    auto t0 = std::chrono::steady_clock::now();
    const int n_new = matcher.CreateNewMapPoints(&kfs[0], neigh, vF12, one);
    if (n_new < 0) {
      fprintf(stderr, "CreateNewMapPoints: %d %s\n", n_new, uvo_last_error());
      return 1;
    }
    for (size_t k = 0; k < one.size(); ++k)
      for (size_t j = 0; j < one[k].size(); ++j) kfs[0].AddMapPoint(&created, (int)one[k][j].idx1);  // :1188, the caller's loop over the output
    auto t1 = std::chrono::steady_clock::now();
    // ---- Begin + per neighbour Next, host triangulation, AddMapPoint
    kfs[0].mps = mps0;
    host.assign(neigh.size(), std::vector<NewMapPoint>());
    auto t2 = std::chrono::steady_clock::now();
    if (matcher.SearchForTriangulationBegin(&kfs[0], neigh, vF12) != UVO_OK) {
      fprintf(stderr, "SearchForTriangulationBegin: %s\n", uvo_last_error());
      return 1;
    }
    for (size_t k = 0; k < neigh.size(); ++k) {
      std::vector<uvo_keypoint> k1, k2;
      std::vector<std::pair<size_t, size_t> > idx;
      matcher.SearchForTriangulationNext(&kfs[0], neigh[k], (int)k, k1, k2, idx);
      for (size_t j = 0; j < idx.size(); ++j) {
        NewMapPoint P;
        if (!triangulate(kfs[0], *neigh[k], k1[j], k2[j], ratioFactor, P.x3D)) continue;
        P.idx1 = idx[j].first, P.idx2 = idx[j].second;
        host[k].push_back(P);
        kfs[0].AddMapPoint(&created, (int)P.idx1);
      }
    }
    auto t3 = std::chrono::steady_clock::now();
    if (rep) {
      t_one.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count());
      t_host.push_back(std::chrono::duration<double, std::milli>(t3 - t2).count());
    }
  }
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 2;
  dump(o, one);
  dump(o, host);
  fclose(o);
  size_t n_one = 0, n_host = 0;
  for (size_t k = 0; k < one.size(); ++k) n_one += one[k].size(), n_host += host[k].size();
  printf("{\"pairs\": %d, \"n1\": %d, \"new_points_one_call\": %zu, \"new_points_host_loop\": %zu, \"reps\": %d, \"one_call_ms\": %.4f, \"begin_next_host_svd_ms\": %.4f}\n",
         nkf - 1, kfs[0].N, n_one, n_host, reps, t_one.empty() ? 0.0 : median(t_one), t_host.empty() ? 0.0 : median(t_host));
  return 0;
}
