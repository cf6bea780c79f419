// Initializer (src/Initializer.cc of the reference: the two-view initialisation every monocular session starts with) as plain C++:
// the F path that Initialize really executes (:44-113 returns ReconstructF unconditionally; the ReconstructH branch is commented out
// and nothing FindHomography produces leaves the function).  FindHomography, ComputeH21, CheckHomography, ReconstructH and Re_CheckRT
// are NOT restated.  initializer.hip runs this on the device, tests/emu/initializer_emu.cpp on the host; the two are held to each other
// bit for bit under the rules of epnp_core.hpp's header: IEEE + - * / sqrt and fabs only, no contraction, every lane owns whole
// scalars, no reduction tree over floating-point values.  acos is restated from IEEE operations through sim3::atan2_pos.
//
// The roundings of the OpenCV calls the source makes are restated from recall, OpenCV not being available to the project [OCV-RECALL]
// (DESIGN.md section 4 carries the same list; tests/initializer_model.py restates it independently):
//   1. cv::SVDecomp / cv::SVD::compute on CV_32F is JacobiSVDImpl_<float> on the n rows of length m of At (m >= n; the 8 x 9 matrix
//      has fewer rows than columns, so its rows are taken as they are, a square matrix is transposed first): the squared row norms W
//      in double; at most max(m, 30) sweeps over the pairs i < j in index order; p = the rows' dot product in double; the pair is
//      skipped when |p| <= eps sqrt(W_i W_j), eps = 2 FLT_EPSILON; c and s are floats made from double expressions with hypot;
//      the rotated elements are float expressions, the new W their squares summed in double; afterwards W = the row norms, a
//      selection sort descending (first largest) that swaps the rows of At and Vt.  std::hypot is restated as a sqrt(1 + (b/a)^2).
//   2. The completion loop of the same function: rows whose norm is <= FLT_MIN, and the rows n .. n1-1 that FULL_UV asks for, start
//      from +-1/m by bit 8 of cv::RNG(0x12345678)'s outputs (state = (uint32)state * 4294883355 + (state >> 32)); two Gram-Schmidt
//      passes against the rows before them (the dot product sums float products in a double, the subtraction is double, rounded to
//      float), each followed by a division by the float L1 norm (0 where that is <= 200 FLT_EPSILON); then the L2 norm in double.
//      Every row is then scaled by the float 1 / norm.  vt.row(8) of ComputeF21 is the row this loop builds.
//   3. A * B of CV_32F matrices with an inner dimension of 2..4 and no transposition flag is cv::gemm's small-matrix path: the float
//      row sum, left to right; with an added matrix (R * x + t) the sum and the added term are joined in double and rounded once.
//      A product with a transposed operand inside the expression (K.t() * F, u * W.t(), -R.t() * t) takes the general path: products
//      and sums in double in index order, alpha applied in double, one rounding to float.
//   4. a * row - row is float arithmetic; Mat / s multiplies by the float (1 / s); cv::norm and cv::Mat::dot are double sums;
//      cv::determinant of a 3 x 3 CV_32F is evaluated in double.
//   5. acos(float) is the float overload; * 180 is a float product, / CV_PI a double division narrowed to the float parallax.
#pragma once
#include <string.h>

#include "sim3_core.hpp"

namespace uvo {
namespace twoview {

constexpr int kSet = 8;                        // points of a minimal set
constexpr int kWsFloats = 81, kWsDoubles = 8;  // per lane: nine rows of nine floats (At; Vt in rows 4..7), W

// The Jacobi indexes its rows by run-time pair and sort position: its arrays live where the caller puts them (LDS on the device, L
// lanes interleaved), never in private arrays.
template <int L>
struct Ws {
  float* f;
  double* d;
  SIM3_HD float& A(int r, int c) const { return f[(r * 9 + c) * L]; }
  SIM3_HD float& V(int r, int c) const { return f[((r + 4) * 9 + c) * L]; }
  SIM3_HD double& W(int k) const { return d[k * L]; }
};

// ---- Initialize :73-90: one minimal set; RandomInt on the live length, swap with the back --------------------------------------------
PNP_HD void draw_set(pnps::GlibcRand& g, int n, int32_t* avail, int32_t* out) {
  for (int i = 0; i < n; ++i) avail[i] = i;
  int live = n;
  for (int j = 0; j < kSet; ++j) {
    const int randi = pnps::random_int(g, 0, live - 1);
    out[j] = avail[randi];
    avail[randi] = avail[live - 1];
    --live;
  }
}

// ---- Normalize :741-787 over ALL keys of a frame: serial float sums (host only), T as four numbers ------------------------------------
struct Norm {
  float meanX, meanY, sX, sY;
};
inline Norm normalize(const float* xy, int n) {
  float meanX = 0, meanY = 0;
  for (int i = 0; i < n; ++i) meanX += xy[2 * i], meanY += xy[2 * i + 1];
  meanX = meanX / (float)n, meanY = meanY / (float)n;
  float devX = 0, devY = 0;
  for (int i = 0; i < n; ++i) devX += fabsf(xy[2 * i] - meanX), devY += fabsf(xy[2 * i + 1] - meanY);
  devX = devX / (float)n, devY = devY / (float)n;
  return Norm{meanX, meanY, (float)(1.0 / (double)devX), (float)(1.0 / (double)devY)};
}
SIM3_HD void normalized(const Norm& T, float x, float y, float* ox, float* oy) {
  *ox = (x - T.meanX) * T.sX;
  *oy = (y - T.meanY) * T.sY;
}

// ---- JacobiSVDImpl_<float> [OCV-RECALL 1, 2] -------------------------------------------------------------------------------------------
SIM3_HD double hypot_ieee(double a, double b) {
  a = fabs(a), b = fabs(b);
  if (a < b) {
    const double t = a;
    a = b, b = t;
  }
  if (a == 0.) return 0.;
  const double r = b / a;
  return a * sqrt(1. + r * r);
}

struct CvRng {
  uint64_t s;
  SIM3_HD uint32_t next() {
    s = (uint64_t)(uint32_t)s * 4294883355u + (uint32_t)(s >> 32);
    return (uint32_t)s;
  }
};

// in: n rows of length m in w.A.  out: n1 rows of w.A orthonormal (the left vectors of At's decomposition), w.W the singular values
// descending, and, with_v, w.V = the accumulated rotations (n x n)
template <class WS>
SIM3_HD void jacobi_svd(const WS& w, int m, int n, int n1, bool with_v) {
  const float eps = FLT_EPSILON * 2;
  const double minval = FLT_MIN;
  for (int i = 0; i < n; ++i) {
    double sd = 0;
    for (int k = 0; k < m; ++k) {
      const float t = w.A(i, k);
      sd += (double)t * (double)t;
    }
    w.W(i) = sd;
    if (with_v)
      for (int k = 0; k < n; ++k) w.V(i, k) = i == k ? 1.f : 0.f;
  }
  for (int iter = 0; iter < 30; ++iter) {  // max(m, 30) with m <= 9
    bool changed = false;
    for (int i = 0; i < n - 1; ++i)
      for (int j = i + 1; j < n; ++j) {
        double a = w.W(i), p = 0, b = w.W(j);
        for (int k = 0; k < m; ++k) p += (double)w.A(i, k) * (double)w.A(j, k);
        if (fabs(p) <= (double)eps * sqrt(a * b)) continue;
        p *= 2;
        const double beta = a - b, gamma = hypot_ieee(p, beta);
        float c, s;
        if (beta < 0) {
          const double delta = (gamma - beta) * 0.5;
          s = (float)sqrt(delta / gamma);
          c = (float)(p / (gamma * (double)s * 2));
        } else {
          c = (float)sqrt((gamma + beta) / (gamma * 2));
          s = (float)(p / (gamma * (double)c * 2));
        }
        a = b = 0;
        for (int k = 0; k < m; ++k) {
          const float x = w.A(i, k), y = w.A(j, k);
          const float t0 = c * x + s * y;
          const float t1 = -s * x + c * y;
          w.A(i, k) = t0, w.A(j, k) = t1;
          a += (double)t0 * (double)t0, b += (double)t1 * (double)t1;
        }
        w.W(i) = a, w.W(j) = b;
        changed = true;
        if (with_v)
          for (int k = 0; k < n; ++k) {
            const float x = w.V(i, k), y = w.V(j, k);
            w.V(i, k) = c * x + s * y, w.V(j, k) = -s * x + c * y;
          }
      }
    if (!changed) break;
  }
  for (int i = 0; i < n; ++i) {
    double sd = 0;
    for (int k = 0; k < m; ++k) {
      const float t = w.A(i, k);
      sd += (double)t * (double)t;
    }
    w.W(i) = sqrt(sd);
  }
  for (int i = 0; i < n - 1; ++i) {
    int j = i;
    for (int k = i + 1; k < n; ++k)
      if (w.W(j) < w.W(k)) j = k;
    if (i != j) {
      const double tw = w.W(i);
      w.W(i) = w.W(j), w.W(j) = tw;
      for (int k = 0; k < m; ++k) {
        const float t = w.A(i, k);
        w.A(i, k) = w.A(j, k), w.A(j, k) = t;
      }
      if (with_v)
        for (int k = 0; k < n; ++k) {
          const float t = w.V(i, k);
          w.V(i, k) = w.V(j, k), w.V(j, k) = t;
        }
    }
  }
  CvRng rng{0x12345678u};
  for (int i = 0; i < n1; ++i) {
    double sd = i < n ? w.W(i) : 0.;
    for (int ii = 0; ii < 100 && sd <= minval; ++ii) {
      const float val0 = (float)(1. / (double)m);
      for (int k = 0; k < m; ++k) w.A(i, k) = (rng.next() & 256u) != 0 ? val0 : -val0;
      for (int pass = 0; pass < 2; ++pass)
        for (int j = 0; j < i; ++j) {
          sd = 0;
          for (int k = 0; k < m; ++k) sd += (double)(w.A(i, k) * w.A(j, k));
          float asum = 0;
          for (int k = 0; k < m; ++k) {
            const float t = (float)((double)w.A(i, k) - sd * (double)w.A(j, k));
            w.A(i, k) = t;
            asum += fabsf(t);
          }
          asum = asum > eps * 100 ? 1 / asum : 0;
          for (int k = 0; k < m; ++k) w.A(i, k) *= asum;
        }
      sd = 0;
      for (int k = 0; k < m; ++k) {
        const float t = w.A(i, k);
        sd += (double)t * (double)t;
      }
      sd = sqrt(sd);
    }
    const float s = (float)(sd > minval ? 1 / sd : 0.);
    for (int k = 0; k < m; ++k) w.A(i, k) *= s;
  }
}

// ---- cv::gemm on 3 x 3 CV_32F [OCV-RECALL 3] --------------------------------------------------------------------------------------------
SIM3_HD void mul33(const float* a, const float* b, float* d) {  // the small-matrix path
  SIM3_UNROLL
  for (int i = 0; i < 3; ++i)
    SIM3_UNROLL
    for (int j = 0; j < 3; ++j) d[3 * i + j] = a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j] + a[3 * i + 2] * b[6 + j];
}
SIM3_HD void mul33_at(const float* a, const float* b, float* d) {  // a^T * b, the general path
  SIM3_UNROLL
  for (int i = 0; i < 3; ++i)
    SIM3_UNROLL
    for (int j = 0; j < 3; ++j) {
      double s = 0.;
      SIM3_UNROLL
      for (int k = 0; k < 3; ++k) s += (double)a[3 * k + i] * (double)b[3 * k + j];
      d[3 * i + j] = (float)s;
    }
}
SIM3_HD void mul33_bt(const float* a, const float* b, float* d) {  // a * b^T, the general path
  SIM3_UNROLL
  for (int i = 0; i < 3; ++i)
    SIM3_UNROLL
    for (int j = 0; j < 3; ++j) {
      double s = 0.;
      SIM3_UNROLL
      for (int k = 0; k < 3; ++k) s += (double)a[3 * i + k] * (double)b[3 * j + k];
      d[3 * i + j] = (float)s;
    }
}

// SVDecomp of a 3 x 3 CV_32F matrix: u, w, vt (row-major); the workspace holds At = M^T
template <class WS>
SIM3_HD void svd33(const WS& w, const float* M, float* u, float* sv, float* vt) {
  SIM3_UNROLL
  for (int i = 0; i < 3; ++i)
    SIM3_UNROLL
    for (int k = 0; k < 3; ++k) w.A(i, k) = M[3 * k + i];
  jacobi_svd(w, 3, 3, 3, true);
  SIM3_UNROLL
  for (int r = 0; r < 3; ++r) {
    sv[r] = (float)w.W(r);
    SIM3_UNROLL
    for (int c = 0; c < 3; ++c) u[3 * r + c] = w.A(c, r), vt[3 * r + c] = w.V(r, c);
  }
}

// ---- ComputeF21 :260-295 and FindFundamental :204 ---------------------------------------------------------------------------------------
template <class WS>
SIM3_HD void set_row(const WS& w, int i, float u1, float v1, float u2, float v2) {
  w.A(i, 0) = u2 * u1, w.A(i, 1) = u2 * v1, w.A(i, 2) = u2;
  w.A(i, 3) = v2 * u1, w.A(i, 4) = v2 * v1, w.A(i, 5) = v2;
  w.A(i, 6) = u1, w.A(i, 7) = v1, w.A(i, 8) = 1.f;
}
// the eight rows are in w.A; F = T2^T Fn T1
template <class WS>
SIM3_HD void f21_from_rows(const WS& w, const Norm& N1, const Norm& N2, float* F) {
  jacobi_svd(w, 9, kSet, 9, false);
  float Fpre[9], u[9], sv[3], vt[9], tmp[9], Fn[9];
  SIM3_UNROLL
  for (int e = 0; e < 9; ++e) Fpre[e] = w.A(8, e);
  svd33(w, Fpre, u, sv, vt);
  const float D[9] = {sv[0], 0.f, 0.f, 0.f, sv[1], 0.f, 0.f, 0.f, 0.f};  // w.at<float>(2) = 0
  mul33(u, D, tmp);
  mul33(tmp, vt, Fn);
  const float T2t[9] = {N2.sX, 0.f, 0.f, 0.f, N2.sY, 0.f, -N2.meanX * N2.sX, -N2.meanY * N2.sY, 1.f};
  const float T1[9] = {N1.sX, 0.f, -N1.meanX * N1.sX, 0.f, N1.sY, -N1.meanY * N1.sY, 0.f, 0.f, 1.f};
  mul33(T2t, Fn, tmp);
  mul33(tmp, T1, F);
}

// ---- CheckFundamental :381-460 for one match: the two terms the score gains (+0 where it gains none), -> bIn ----------------------------
SIM3_HD float inv_sigma_square(float sigma) { return (float)(1.0 / (double)(sigma * sigma)); }
SIM3_HD bool score_terms(const float* F, float u1, float v1, float u2, float v2, float invSigmaSquare, float* term1, float* term2) {
  const float th = 3.841f, thScore = 5.991f;
  bool bIn = true;
  const float a2 = F[0] * u1 + F[1] * v1 + F[2];
  const float b2 = F[3] * u1 + F[4] * v1 + F[5];
  const float c2 = F[6] * u1 + F[7] * v1 + F[8];
  const float num2 = a2 * u2 + b2 * v2 + c2;
  const float squareDist1 = num2 * num2 / (a2 * a2 + b2 * b2);
  const float chiSquare1 = squareDist1 * invSigmaSquare;
  if (chiSquare1 > th) bIn = false, *term1 = 0.f;
  else *term1 = thScore - chiSquare1;
  const float a1 = F[0] * u2 + F[3] * v2 + F[6];
  const float b1 = F[1] * u2 + F[4] * v2 + F[7];
  const float c1 = F[2] * u2 + F[5] * v2 + F[8];
  const float num1 = a1 * u1 + b1 * v1 + c1;
  const float squareDist2 = num1 * num1 / (a1 * a1 + b1 * b1);
  const float chiSquare2 = squareDist2 * invSigmaSquare;
  if (chiSquare2 > th) bIn = false, *term2 = 0.f;
  else *term2 = thScore - chiSquare2;
  return bIn;
}

// ---- ReconstructF :471-479, DecomposeE :1062-1082 ----------------------------------------------------------------------------------------
struct Cam {
  float fx, fy, cx, cy;
};
struct Motion {
  float R1[9], R2[9], t[3];
};
SIM3_HD double det33(const float* m) {  // [OCV-RECALL 4]
  return (double)m[0] * ((double)m[4] * (double)m[8] - (double)m[5] * (double)m[7]) - (double)m[1] * ((double)m[3] * (double)m[8] - (double)m[5] * (double)m[6]) +
         (double)m[2] * ((double)m[3] * (double)m[7] - (double)m[4] * (double)m[6]);
}
template <class WS>
SIM3_HD void decompose_e(const WS& w, const float* F, const Cam& C, Motion& M) {
  const float K[9] = {C.fx, 0.f, C.cx, 0.f, C.fy, C.cy, 0.f, 0.f, 1.f};
  float KtF[9], E[9], u[9], sv[3], vt[9], tmp[9];
  mul33_at(K, F, KtF);
  mul33(KtF, K, E);
  svd33(w, E, u, sv, vt);
  const double nrm = sqrt((double)u[2] * (double)u[2] + (double)u[5] * (double)u[5] + (double)u[8] * (double)u[8]);
  const float sc = (float)(1.0 / nrm);
  M.t[0] = u[2] * sc, M.t[1] = u[5] * sc, M.t[2] = u[8] * sc;
  const float Wm[9] = {0.f, -1.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f};
  mul33(u, Wm, tmp);
  mul33(tmp, vt, M.R1);
  const bool neg1 = det33(M.R1) < 0;
  SIM3_UNROLL
  for (int e = 0; e < 9; ++e) M.R1[e] = neg1 ? -M.R1[e] : M.R1[e];
  mul33_bt(u, Wm, tmp);
  mul33(tmp, vt, M.R2);
  const bool neg2 = det33(M.R2) < 0;
  SIM3_UNROLL
  for (int e = 0; e < 9; ++e) M.R2[e] = neg2 ? -M.R2[e] : M.R2[e];
}
// CheckRT's argument pair k = 0..3: (R1, t), (R2, t), (R1, -t), (R2, -t)
SIM3_HD void motion_of(const Motion& M, int k, float* R, float* t) {
  SIM3_UNROLL
  for (int e = 0; e < 9; ++e) R[e] = (k & 1) ? M.R2[e] : M.R1[e];
  SIM3_UNROLL
  for (int e = 0; e < 3; ++e) t[e] = (k & 2) ? -M.t[e] : M.t[e];
}

// ---- CheckRT :790-904 for one inlier match, Triangulate :726-739 --------------------------------------------------------------------------
constexpr int kCounted = 1, kGood = 2;  // nGood++ ; vbGood = true
SIM3_HD float th2_of(float sigma) { return (float)(4.0 * (double)(sigma * sigma)); }
SIM3_HD bool finite_f(float x) { return x - x == 0.f; }
template <class WS>
SIM3_HD int check_rt_one(const WS& w, const float* R, const float* t, const Cam& C, float k1x, float k1y, float k2x, float k2y, float th2, float* X, float* cosp) {
  X[0] = X[1] = X[2] = 0.f, *cosp = 0.f;
  const float K[9] = {C.fx, 0.f, C.cx, 0.f, C.fy, C.cy, 0.f, 0.f, 1.f};
  float P1[12], P2[12], O2[3];
  SIM3_UNROLL
  for (int i = 0; i < 3; ++i)
    SIM3_UNROLL
    for (int j = 0; j < 4; ++j) {
      const float m0 = j < 3 ? R[j] : t[0], m1 = j < 3 ? R[3 + j] : t[1], m2 = j < 3 ? R[6 + j] : t[2];
      P1[4 * i + j] = j < 3 ? K[3 * i + j] : 0.f;
      P2[4 * i + j] = K[3 * i] * m0 + K[3 * i + 1] * m1 + K[3 * i + 2] * m2;
    }
  SIM3_UNROLL
  for (int i = 0; i < 3; ++i) O2[i] = (float)(-((double)R[i] * (double)t[0] + (double)R[3 + i] * (double)t[1] + (double)R[6 + i] * (double)t[2]));
  SIM3_UNROLL
  for (int k = 0; k < 4; ++k) {  // At = A^T: row k of At is column k of A
    w.A(k, 0) = k1x * P1[8 + k] - P1[k];
    w.A(k, 1) = k1y * P1[8 + k] - P1[4 + k];
    w.A(k, 2) = k2x * P2[8 + k] - P2[k];
    w.A(k, 3) = k2y * P2[8 + k] - P2[4 + k];
  }
  jacobi_svd(w, 4, 4, 4, true);
  const float rinv = (float)(1.0 / (double)w.V(3, 3));
  const float x = w.V(3, 0) * rinv, y = w.V(3, 1) * rinv, z = w.V(3, 2) * rinv;
  if (!finite_f(x) || !finite_f(y) || !finite_f(z)) return 0;
  const float n2x = x - O2[0], n2y = y - O2[1], n2z = z - O2[2];
  const float dist1 = (float)sqrt((double)x * (double)x + (double)y * (double)y + (double)z * (double)z);
  const float dist2 = (float)sqrt((double)n2x * (double)n2x + (double)n2y * (double)n2y + (double)n2z * (double)n2z);
  const float cosParallax = (float)(((double)x * (double)n2x + (double)y * (double)n2y + (double)z * (double)n2z) / (double)(dist1 * dist2));
  const bool low = (double)cosParallax < 0.99998;
  if (z <= 0 && low) return 0;
  const float x2 = (float)((double)(R[0] * x + R[1] * y + R[2] * z) + (double)t[0]);
  const float y2 = (float)((double)(R[3] * x + R[4] * y + R[5] * z) + (double)t[1]);
  const float z2 = (float)((double)(R[6] * x + R[7] * y + R[8] * z) + (double)t[2]);
  if (z2 <= 0 && low) return 0;
  const float invZ1 = (float)(1.0 / (double)z);
  const float im1x = C.fx * x * invZ1 + C.cx, im1y = C.fy * y * invZ1 + C.cy;
  const float squareError1 = (im1x - k1x) * (im1x - k1x) + (im1y - k1y) * (im1y - k1y);
  if (squareError1 > th2) return 0;
  const float invZ2 = (float)(1.0 / (double)z2);
  const float im2x = C.fx * x2 * invZ2 + C.cx, im2y = C.fy * y2 * invZ2 + C.cy;
  const float squareError2 = (im2x - k2x) * (im2x - k2x) + (im2y - k2y) * (im2y - k2y);
  if (squareError2 > th2) return 0;
  X[0] = x, X[1] = y, X[2] = z, *cosp = cosParallax;
  return kCounted | (low ? kGood : 0);
}

using sim3::acos_ieee;  // sim3_core.hpp: essential_core.hpp takes it from there too
// :898 acos(c) * 180 / CV_PI [OCV-RECALL 5]
SIM3_HD float parallax_deg(float c) {
  const float a = (float)acos_ieee((double)c);
  return (float)((double)(a * 180.f) / 3.1415926535897932384626433832795);
}
// The order statistic of :895-897 is a value, not a sum: the device selects it bit by bit over this key, which orders floats as
// operator< does (-0 below +0 and NaN above everything, where std::sort sees equals and undefined behaviour).
SIM3_HD uint32_t ordered_key(float v) {
  uint32_t b;
  memcpy(&b, &v, 4);
  return (b & 0x80000000u) ? ~b : b | 0x80000000u;
}
SIM3_HD float from_ordered_key(uint32_t k) {
  const uint32_t b = (k & 0x80000000u) ? k & 0x7fffffffu : ~k;
  float v;
  memcpy(&v, &b, 4);
  return v;
}

// ---- ReconstructF's verdict :491-561 -----------------------------------------------------------------------------------------------------
struct Verdict {
  int32_t ok, deciding;
};
SIM3_HD Verdict verdict_of(int N, const int32_t* nGood, const float* parallax) {
  const float minParallax = 1.f;
  const int minTriangulated = 50;
  int maxGood = nGood[0];
  SIM3_UNROLL
  for (int k = 1; k < 4; ++k) maxGood = nGood[k] > maxGood ? nGood[k] : maxGood;
  const int n09 = (int)(0.9 * (double)N);
  const int nMinGood = n09 > minTriangulated ? n09 : minTriangulated;
  int nsimilar = 0, deciding = 3;
  SIM3_UNROLL
  for (int k = 3; k >= 0; --k) {
    if ((double)nGood[k] > 0.7 * (double)maxGood) ++nsimilar;
    if (nGood[k] == maxGood) deciding = k;
  }
  const bool rejected = maxGood < nMinGood || nsimilar > 1;
  float par = parallax[0];
  SIM3_UNROLL
  for (int k = 1; k < 4; ++k) par = deciding == k ? parallax[k] : par;
  return Verdict{!rejected && par > minParallax ? 1 : 0, deciding};
}

}  // namespace twoview
}  // namespace uvo
