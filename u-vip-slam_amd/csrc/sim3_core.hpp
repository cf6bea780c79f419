// Sim3Solver (src/Sim3Solver.cc of the reference: the RANSAC around Horn's closed form that LoopClosing::ComputeSim3 runs per loop
// candidate) as plain C++.  sim3solver.hip runs this on the device, tests/emu/sim3solver_emu.cpp on the host; the two are held to each
// other bit for bit under the rules of epnp_core.hpp's header: IEEE + - * / sqrt and fabs only, no contraction, every lane owns whole
// scalars, no reduction tree over floating-point values.  The generator and the subset draw are glibc_rand.hpp's pnps::GlibcRand /
// pnps::draw_subset at a minimal set of 3.
//
// computeT needs atan2, sin and cos in double, which are not shared-source functions.  atan2_pos and sincos below are built from IEEE
// operations only (two-part constants, Taylor polynomials on a reduced range); they do not reproduce libm's bits, they are accurate to
// about 2^-51 absolute, which is below what the float roundings that follow them resolve (tests/test_sim3solver_emu.py, layer 6).
//
// The roundings of the OpenCV calls the source makes are restated from recall, OpenCV not being available to the project [OCV-RECALL]
// (DESIGN.md section 4 carries the same list; tests/sim3_model.py restates it independently):
//   1. CV_32F products A*B, A*B+C, alpha*A*B, C - alpha*A*B are one gemm each: products and sums in double in index order, alpha and
//      the added term applied in double, one rounding to float per element.
//   2. cv::reduce(SUM) on 32F accumulates in float in column order; C / P.cols multiplies by the double 1./3 and rounds once.
//   3. The entries of N are float expressions evaluated left to right.
//   4. cv::eigen on a symmetric CV_32F matrix is JacobiImpl_<float>: eps = FLT_EPSILON, at most n*n*30 rotations, the pivot through
//      the indR / indC bookkeeping, OpenCV's own hypot, eigenvalues sorted descending with the rows of V, signs as they fall.
//   5. norm(vec) sums squares in double; ang = atan2(double, (double)float); vec = 2*ang*vec/norm(vec) is one scale
//      (2*ang) * (1./norm) applied in double and rounded to float.
//   6. cv::Rodrigues on the float vector computes in double: theta = sqrt(sum of squares), identity below DBL_EPSILON, c, s, 1 - c,
//      r * (1/theta), R = c I + (1 - c) r r^T + s [r]x summed in that order, rounded to float.
//   7. Pr1.dot(P3) multiplies the floats as doubles and sums in double in row-major order (a vectorised OpenCV may group the sum
//      differently); cv::pow(P3, 2) gives float squares, den is their double sum in row-major order; ms12i = (float)(nom / den);
//      sRinv = (1.0 / ms12i) * R^T is applied in double.
//   8. Project: invz = 1 / z, x * invz and fx * x + cx are float; dist.dot(dist) is a double narrowed to the float err.
// derive_max_its uses pow / log / ceil and is HOST ONLY, as pnps::derive_params is.
#pragma once
#include <float.h>
#include <math.h>

#include "glibc_rand.hpp"

#if defined(__HIPCC__)
#define SIM3_HD __host__ __device__ __forceinline__  // outputs through pointers must not force the caller's locals into memory
#else
#define SIM3_HD inline
#endif
#if defined(__clang__)
#define SIM3_UNROLL _Pragma("unroll")
#else
#define SIM3_UNROLL
#endif

namespace uvo {
namespace sim3 {

constexpr int kMinSet = 3;
constexpr int kWsFloats = 36, kWsInts = 8;  // per lane: A[16], V[16], W[4]; indR[4], indC[4]

// The 4 x 4 Jacobi indexes A and V by a run-time pivot: its arrays live where the caller puts them (LDS on the device, L lanes
// interleaved), never in private arrays.
template <int L>
struct Ws {
  float* f;
  int32_t* i;
  PNP_HD float& A(int r, int c) const { return f[(r * 4 + c) * L]; }
  PNP_HD float& V(int r, int c) const { return f[(16 + r * 4 + c) * L]; }
  PNP_HD float& W(int k) const { return f[(32 + k) * L]; }
  PNP_HD int32_t& indR(int k) const { return i[k * L]; }
  PNP_HD int32_t& indC(int k) const { return i[(4 + k) * L]; }
};

// ---- SetRansacParameters :114-138 (host only) ------------------------------------------------------------------------------------
struct Params {
  double probability;
  int min_inliers, max_iterations;
};
// mRansacMaxIts.  Where the ratio is no int the conventions are pnps::derive_params': too large means maxIterations, NaN (and anything
// below 1) gives 1.
inline int derive_max_its(int n, const Params& p) {
  const float eps = (float)p.min_inliers / (float)n;
  double its = 1.;
  if (p.min_inliers != n) its = ceil(log(1. - p.probability) / log(1. - pow((double)eps, 3.)));
  if (!(its >= 1.)) return 1;  // NaN, -inf, anything below 1: before the conversion, which is undefined for them
  return its < (double)p.max_iterations ? (int)its : p.max_iterations;
}

// mvnMaxError1/2 are vector<size_t>: 9.210 * sigma2 is truncated, then compared as a float
inline float max_error(float sigma2) { return (float)(uint64_t)(9.210 * (double)sigma2); }

// ---- sin, cos on [0, 2 pi] and atan2 for y >= 0, from IEEE operations --------------------------------------------------------------
SIM3_HD void sincos(double th, double* sn, double* cs) {
  if (!(th >= 0. && th <= 7.)) {  // NaN, infinity: no quadrant to pick
    *sn = *cs = (th - th) / (th - th);
    return;
  }
  const int k = (int)(th * 0x1.45f306dc9c883p-1 + 0.5);  // nearest multiple of pi/2: 0..4
  const double kd = (double)k;
  const double r = (th - kd * 0x1.921fb54400000p+0) - kd * 0x1.0b4611a626331p-34;  // pi/2 in two parts, the first of 33 bits: kd * it is exact
  const double z = r * r;
  // Taylor on |r| <= pi/4: the first terms left out are r^19/19! < 1e-19 and r^20/20! < 1e-20
  double p = 0x1.952c77030ad4ap-49;
  p = 0x1.ae7f3e733b81fp-41 - z * p;
  p = 0x1.6124613a86d09p-33 - z * p;
  p = 0x1.ae64567f544e4p-26 - z * p;
  p = 0x1.71de3a556c734p-19 - z * p;
  p = 0x1.a01a01a01a01ap-13 - z * p;
  p = 0x1.1111111111111p-7 - z * p;
  p = 0x1.5555555555555p-3 - z * p;
  const double s = r - r * (z * p);
  double q = 0x1.6827863b97d97p-53;
  q = 0x1.ae7f3e733b81fp-45 - z * q;
  q = 0x1.93974a8c07c9dp-37 - z * q;
  q = 0x1.1eed8eff8d898p-29 - z * q;
  q = 0x1.27e4fb7789f5cp-22 - z * q;
  q = 0x1.a01a01a01a01ap-16 - z * q;
  q = 0x1.6c16c16c16c17p-10 - z * q;
  q = 0x1.5555555555555p-5 - z * q;
  const double c = (1. - 0.5 * z) + (z * z) * q;
  const int quad = k & 3;
  *sn = quad == 0 ? s : quad == 1 ? c : quad == 2 ? -s : -c;
  *cs = quad == 0 ? c : quad == 1 ? -s : quad == 2 ? -c : s;
}

// atan2(y, x) for y >= 0: in [0, pi]
SIM3_HD double atan2_pos(double y, double x) {
  const double ax = fabs(x);
  const bool steep = y > ax;
  const double num = steep ? ax : y, den = steep ? y : ax;
  const double a = den == 0. ? 0. : num / den;  // in [0, 1]
  if (!(a >= 0. && a <= 1.)) return a - a + (a - a) / (a - a);  // NaN in, NaN out
  // atan a = atan(i/8) + atan t, t = (a - i/8) / (1 + a i/8), |t| <= 1/16: Taylor to t^15, the next term is below 1e-21
  const int i = (int)(a * 8. + 0.5);
  const double c = (double)i * 0.125;
  const double t = (a - c) / (1. + a * c);
  const double z = t * t;
  double p = 0x1.1111111111111p-4;
  p = 0x1.3b13b13b13b14p-4 - z * p;
  p = 0x1.745d1745d1746p-4 - z * p;
  p = 0x1.c71c71c71c71cp-4 - z * p;
  p = 0x1.2492492492492p-3 - z * p;
  p = 0x1.999999999999ap-3 - z * p;
  p = 0x1.5555555555555p-2 - z * p;
  const double at = t - t * (z * p);
  const double hi = i == 0 ? 0. : i == 1 ? 0x1.fd5ba9aac2f6ep-4 : i == 2 ? 0x1.f5b75f92c80ddp-3 : i == 3 ? 0x1.6f61941e4def1p-2 : i == 4 ? 0x1.dac670561bb4fp-2
                   : i == 5 ? 0x1.1e00babdefeb4p-1 : i == 6 ? 0x1.4978fa3269ee1p-1 : i == 7 ? 0x1.700a7c5784634p-1 : 0x1.921fb54442d18p-1;
  const double lo = i == 0 ? 0. : i == 1 ? -0x1.cd37686760c17p-59 : i == 2 ? 0x1.8ab6e3cf7afbdp-57 : i == 3 ? -0x1.c63aae6f6e918p-56 : i == 4 ? 0x1.a2b7f222f65e2p-56
                   : i == 5 ? -0x1.928df287a668fp-58 : i == 6 ? 0x1.2419a87f2a458p-56 : i == 7 ? -0x1.8c34d25aadef6p-56 : 0x1.1a62633145c07p-55;
  const double v = hi + (lo + at);  // atan(num / den) in [0, pi/4]
  if (!steep) return x >= 0. ? v : 0x1.921fb54442d18p+1 - (v - 0x1.1a62633145c07p-53);
  return x >= 0. ? 0x1.921fb54442d18p+0 - (v - 0x1.1a62633145c07p-54) : 0x1.921fb54442d18p+0 + (v + 0x1.1a62633145c07p-54);
}

// acos on [-1, 1] from IEEE operations: atan2(sqrt((1 - x)(1 + x)), x)
SIM3_HD double acos_ieee(double x) {
  if (!(x >= -1. && x <= 1.)) return (x - x) / (x - x) + (1. - 1.) / (x - x);  // NaN
  return atan2_pos(sqrt((1. - x) * (1. + x)), x);
}

// ---- cv::eigen of a symmetric 4 x 4 CV_32F matrix [OCV-RECALL 4] ---------------------------------------------------------------------
PNP_HD float ocv_hypot(float a, float b) {
  a = fabsf(a), b = fabsf(b);
  if (a > b) {
    b /= a;
    return a * sqrtf(1 + b * b);
  }
  if (b > 0) {
    a /= b;
    return b * sqrtf(1 + a * a);
  }
  return 0;
}

template <class WS>
PNP_HD void jacobi_row_max(const WS& w, int k) {  // largest off-diagonal entry right of the diagonal in row k
  int m = k + 1;
  float mv = fabsf(w.A(k, m));
  for (int i = k + 2; i < 4; ++i) {
    const float val = fabsf(w.A(k, i));
    if (mv < val) mv = val, m = i;
  }
  w.indR(k) = m;
}
template <class WS>
PNP_HD void jacobi_col_max(const WS& w, int k) {  // and above the diagonal in column k
  int m = 0;
  float mv = fabsf(w.A(0, k));
  for (int i = 1; i < k; ++i) {
    const float val = fabsf(w.A(i, k));
    if (mv < val) mv = val, m = i;
  }
  w.indC(k) = m;
}

// in: w.A (upper triangle read).  out: w.W descending, w.V the eigenvectors as rows
template <class WS>
PNP_HD void jacobi4(const WS& w) {
  constexpr int n = 4;
  const float eps = FLT_EPSILON;
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) w.V(i, j) = i == j ? 1.f : 0.f;
  for (int k = 0; k < n; ++k) {
    w.W(k) = w.A(k, k);
    if (k < n - 1) jacobi_row_max(w, k);
    if (k > 0) jacobi_col_max(w, k);
  }
  for (int iters = 0; iters < n * n * 30; ++iters) {
    int k = 0;
    float mv = fabsf(w.A(0, w.indR(0)));
    for (int i = 1; i < n - 1; ++i) {
      const float val = fabsf(w.A(i, w.indR(i)));
      if (mv < val) mv = val, k = i;
    }
    int l = w.indR(k);
    for (int i = 1; i < n; ++i) {
      const float val = fabsf(w.A(w.indC(i), i));
      if (mv < val) mv = val, k = w.indC(i), l = i;
    }
    const float p = w.A(k, l);
    if (fabsf(p) <= eps) break;
    const float y = (w.W(l) - w.W(k)) * 0.5f;
    float t = fabsf(y) + ocv_hypot(p, y);
    float s = ocv_hypot(p, t);
    const float c = t / s;
    s = p / s;
    t = (p / t) * p;
    if (y < 0) s = -s, t = -t;
    w.A(k, l) = 0;
    w.W(k) -= t;
    w.W(l) += t;
    float a0, b0;
#define UVO_SIM3_ROTATE(v0, v1) a0 = v0, b0 = v1, v0 = a0 * c - b0 * s, v1 = a0 * s + b0 * c
    for (int i = 0; i < k; ++i) UVO_SIM3_ROTATE(w.A(i, k), w.A(i, l));
    for (int i = k + 1; i < l; ++i) UVO_SIM3_ROTATE(w.A(k, i), w.A(i, l));
    for (int i = l + 1; i < n; ++i) UVO_SIM3_ROTATE(w.A(k, i), w.A(l, i));
    for (int i = 0; i < n; ++i) UVO_SIM3_ROTATE(w.V(k, i), w.V(l, i));
#undef UVO_SIM3_ROTATE
    for (int j = 0; j < 2; ++j) {
      const int idx = j == 0 ? k : l;
      if (idx < n - 1) jacobi_row_max(w, idx);
      if (idx > 0) jacobi_col_max(w, idx);
    }
  }
  for (int k = 0; k < n - 1; ++k) {
    int m = k;
    for (int i = k + 1; i < n; ++i)
      if (w.W(m) < w.W(i)) m = i;
    if (k != m) {
      const float tw = w.W(m);
      w.W(m) = w.W(k), w.W(k) = tw;
      for (int i = 0; i < n; ++i) {
        const float tv = w.V(m, i);
        w.V(m, i) = w.V(k, i), w.V(k, i) = tv;
      }
    }
  }
}

// ---- the rotation of a quaternion (w, x, y, z) as computeT makes it: angle-axis in float, cv::Rodrigues [OCV-RECALL 5, 6] ------------
SIM3_HD void quaternion_to_rotation(float e0, float v0, float v1, float v2, float* R) {
  const double nrm = sqrt((double)v0 * (double)v0 + (double)v1 * (double)v1 + (double)v2 * (double)v2);
  const double ang = atan2_pos(nrm, (double)e0);
  const double alpha = (2. * ang) * (1. / nrm);
  const float r0 = (float)(alpha * (double)v0), r1 = (float)(alpha * (double)v1), r2 = (float)(alpha * (double)v2);
  double rx = r0, ry = r1, rz = r2;
  const double theta = sqrt(rx * rx + ry * ry + rz * rz);
  const bool ident = theta < DBL_EPSILON;  // the identity; selected per element below, so that no store depends on a branch
  double s, c;
  sincos(theta, &s, &c);
  const double c1 = 1. - c, itheta = 1. / theta;
  rx *= itheta, ry *= itheta, rz *= itheta;
  R[0] = ident ? 1.f : (float)(c + c1 * (rx * rx) + s * 0.);
  R[1] = ident ? 0.f : (float)(c * 0. + c1 * (rx * ry) + s * -rz);
  R[2] = ident ? 0.f : (float)(c * 0. + c1 * (rx * rz) + s * ry);
  R[3] = ident ? 0.f : (float)(c * 0. + c1 * (rx * ry) + s * rz);
  R[4] = ident ? 1.f : (float)(c + c1 * (ry * ry) + s * 0.);
  R[5] = ident ? 0.f : (float)(c * 0. + c1 * (ry * rz) + s * -rx);
  R[6] = ident ? 0.f : (float)(c * 0. + c1 * (rx * rz) + s * -ry);
  R[7] = ident ? 0.f : (float)(c * 0. + c1 * (ry * rz) + s * rx);
  R[8] = ident ? 1.f : (float)(c + c1 * (rz * rz) + s * 0.);
}

// ---- computeT :226-332 ---------------------------------------------------------------------------------------------------------------
struct Hyp {
  float T12[16], T21[16];  // row-major 4 x 4
  float R[9], t[3], s;     // mR12i, mt12i, ms12i
  int32_t finite;          // every element of T12 and T21 is finite
};

SIM3_HD void centroid(const float P[3][3], float Pr[3][3], float C[3]) {  // [OCV-RECALL 2]
  SIM3_UNROLL
  for (int r = 0; r < 3; ++r) {
    const float sum = (P[r][0] + P[r][1]) + P[r][2];
    C[r] = (float)((double)sum * (1. / 3));
    SIM3_UNROLL
    for (int c = 0; c < 3; ++c) Pr[r][c] = P[r][c] - C[r];
  }
}

// P1, P2: [coordinate][point], the columns being the three drawn points in camera 1 and camera 2
template <class WS>
SIM3_HD void compute_t(const WS& w, const float P1[3][3], const float P2[3][3], Hyp& H) {
  float Pr1[3][3], Pr2[3][3], O1[3], O2[3], M[3][3];
  centroid(P1, Pr1, O1);
  centroid(P2, Pr2, O2);
  SIM3_UNROLL
  for (int i = 0; i < 3; ++i)
    SIM3_UNROLL
    for (int j = 0; j < 3; ++j) {  // M = Pr2 * Pr1^T
      double d = 0.;
      SIM3_UNROLL
      for (int k = 0; k < 3; ++k) d += (double)Pr2[i][k] * (double)Pr1[j][k];
      M[i][j] = (float)d;
    }
  const float N11 = M[0][0] + M[1][1] + M[2][2], N12 = M[1][2] - M[2][1], N13 = M[2][0] - M[0][2], N14 = M[0][1] - M[1][0];
  const float N22 = M[0][0] - M[1][1] - M[2][2], N23 = M[0][1] + M[1][0], N24 = M[2][0] + M[0][2];
  const float N33 = -M[0][0] + M[1][1] - M[2][2], N34 = M[1][2] + M[2][1], N44 = -M[0][0] - M[1][1] + M[2][2];
  w.A(0, 0) = N11, w.A(0, 1) = N12, w.A(0, 2) = N13, w.A(0, 3) = N14;
  w.A(1, 0) = N12, w.A(1, 1) = N22, w.A(1, 2) = N23, w.A(1, 3) = N24;
  w.A(2, 0) = N13, w.A(2, 1) = N23, w.A(2, 2) = N33, w.A(2, 3) = N34;
  w.A(3, 0) = N14, w.A(3, 1) = N24, w.A(3, 2) = N34, w.A(3, 3) = N44;
  jacobi4(w);
  float* R = H.R;
  quaternion_to_rotation(w.V(0, 0), w.V(0, 1), w.V(0, 2), w.V(0, 3), R);
  float P3[3][3];
  SIM3_UNROLL
  for (int i = 0; i < 3; ++i)
    SIM3_UNROLL
    for (int j = 0; j < 3; ++j) {  // P3 = R * Pr2
      double d = 0.;
      SIM3_UNROLL
      for (int k = 0; k < 3; ++k) d += (double)R[3 * i + k] * (double)Pr2[k][j];
      P3[i][j] = (float)d;
    }
  double nom = 0., den = 0.;
  SIM3_UNROLL
  for (int i = 0; i < 3; ++i)
    SIM3_UNROLL
    for (int j = 0; j < 3; ++j) nom += (double)Pr1[i][j] * (double)P3[i][j];
  SIM3_UNROLL
  for (int i = 0; i < 3; ++i)
    SIM3_UNROLL
    for (int j = 0; j < 3; ++j) den += (double)(P3[i][j] * P3[i][j]);
  const float s = (float)(nom / den);
  H.s = s;
  SIM3_UNROLL
  for (int i = 0; i < 3; ++i) {  // t = O1 - s R O2
    double d = 0.;
    SIM3_UNROLL
    for (int k = 0; k < 3; ++k) d += (double)R[3 * i + k] * (double)O2[k];
    H.t[i] = (float)(-(double)s * d + (double)O1[i]);
  }
  const double sinv = 1.0 / (double)s;
  float sRinv[9];
  SIM3_UNROLL
  for (int i = 0; i < 3; ++i)
    SIM3_UNROLL
    for (int j = 0; j < 3; ++j) {
      H.T12[4 * i + j] = (float)((double)s * (double)R[3 * i + j]);
      sRinv[3 * i + j] = (float)(sinv * (double)R[3 * j + i]);
      H.T21[4 * i + j] = sRinv[3 * i + j];
    }
  SIM3_UNROLL
  for (int i = 0; i < 3; ++i) {
    double d = 0.;
    SIM3_UNROLL
    for (int k = 0; k < 3; ++k) d += (double)sRinv[3 * i + k] * (double)H.t[k];
    H.T12[4 * i + 3] = H.t[i];
    H.T21[4 * i + 3] = (float)(-d);
  }
  H.T12[12] = H.T12[13] = H.T12[14] = 0.f, H.T12[15] = 1.f;
  H.T21[12] = H.T21[13] = H.T21[14] = 0.f, H.T21[15] = 1.f;
  bool fin = true;
  SIM3_UNROLL
  for (int e = 0; e < 12; ++e) fin &= (H.T12[e] - H.T12[e] == 0.f) & (H.T21[e] - H.T21[e] == 0.f);
  H.finite = fin ? 1 : 0;
}

// ---- the constructor's Rcw * X + tcw, FromCameraToImage, Project, CheckInliers [OCV-RECALL 1, 8] -------------------------------------
// T: row-major with row stride `ld` (a 4 x 4 transform: ld = 4; Rcw and tcw apart: R with ld = 3 and t)
PNP_HD void transform(const float* R, int ld, float t0, float t1, float t2, const float* X, float* out) {
  out[0] = (float)(((double)R[0] * (double)X[0] + (double)R[1] * (double)X[1] + (double)R[2] * (double)X[2]) + (double)t0);
  out[1] = (float)(((double)R[ld] * (double)X[0] + (double)R[ld + 1] * (double)X[1] + (double)R[ld + 2] * (double)X[2]) + (double)t1);
  out[2] = (float)(((double)R[2 * ld] * (double)X[0] + (double)R[2 * ld + 1] * (double)X[1] + (double)R[2 * ld + 2] * (double)X[2]) + (double)t2);
}

struct Cam {
  float fx, fy, cx, cy;
};

PNP_HD void to_image(const float* Xc, const Cam& K, float* uv) {
  const float invz = 1 / Xc[2];
  const float x = Xc[0] * invz, y = Xc[1] * invz;
  uv[0] = K.fx * x + K.cx;
  uv[1] = K.fy * y + K.cy;
}

PNP_HD float reprojection_error(const float* T, const float* X, const Cam& K, const float* uv, bool uv_first) {
  float Xc[3], p[2];
  transform(T, 4, T[3], T[7], T[11], X, Xc);
  to_image(Xc, K, p);
  const float dx = uv_first ? uv[0] - p[0] : p[0] - uv[0], dy = uv_first ? uv[1] - p[1] : p[1] - uv[1];
  return (float)((double)dx * (double)dx + (double)dy * (double)dy);
}

// one correspondence: X1c, X2c its position in either camera, p1, p2 its image there, e1, e2 the thresholds as floats
PNP_HD bool check_inlier(const float* T12, const float* T21, const float* X1c, const float* X2c, const float* p1, const float* p2, const Cam& K1, const Cam& K2,
                         float e1, float e2) {
  const float err1 = reprojection_error(T12, X2c, K1, p1, true);   // mvP1im1 - vP2im1
  const float err2 = reprojection_error(T21, X1c, K2, p2, false);  // vP1im2 - mvP2im2
  return err1 < e1 && err2 < e2;
}

// ---- iterate :140-207 over hypotheses that were all evaluated beforehand -----------------------------------------------------------
// the iterations one call runs unless it returns: the loop condition is an AND
PNP_HD int iterations_ahead(int iterations_so_far, int max_its, int n_iterations) {
  const int a = max_its - iterations_so_far;
  const int k = a < n_iterations ? a : n_iterations;
  return k > 0 ? k : 0;
}

struct State {
  int32_t iterations;  // mnIterations
  int32_t best_count;  // mnBestInliers
};
struct Outcome {
  int32_t performed;  // iterations of this call = hypotheses consumed
  int32_t returned;   // the hypothesis returned, -1: none
  int32_t no_more;    // bNoMore
  int32_t inliers;    // nInliers
  int32_t best_from;  // the hypothesis that is the best now, -1: the one carried from earlier calls
};

PNP_HD Outcome replay(State& st, const int32_t* counts, int n_iterations, int max_its, int min_inliers) {
  Outcome o = {0, -1, 0, 0, -1};
  int cur = 0;
  while (st.iterations < max_its && cur < n_iterations) {
    const int c = counts[cur];
    ++cur, ++st.iterations;
    if (c >= st.best_count) {
      st.best_count = c, o.best_from = cur - 1;
      if (c > min_inliers) {
        o.performed = cur, o.returned = cur - 1, o.inliers = c;
        return o;
      }
    }
  }
  o.performed = cur;
  if (st.iterations >= max_its) o.no_more = 1;
  return o;
}

}  // namespace sim3
}  // namespace uvo
