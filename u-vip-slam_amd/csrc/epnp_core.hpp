// cv::solvePnPRansac(..., SOLVEPNP_EPNP) as plain C++ in double: the one statement of everything in the call that is arithmetic.
// pnp.hip runs it on the device, tests/emu/pnp_emu.cpp on the host; the two are held to each other bit for bit, which is only
// possible because (a) nothing here calls a library function other than sqrt and fabs (IEEE, correctly rounded on both sides), the
// build contracts no multiply-add on either side, and (b) work is shared between lanes only by giving every lane whole scalars:
// solve() is a sequence of phases, phase p computes K_p scalars, scalar k is one serial loop over the points in list order, and a
// caller with L lanes lets lane l take k = l, l + L, ...  A host build is the caller with one lane.
//
// EPnP after Lepetit, Moreno-Noguer, Fua (IJCV 2009), the variant OpenCV ships: four control points from the principal axes of the
// map points, barycentric coordinates, the 12 x 12 normal matrix MtM of the 2n x 12 projection system, its four smallest
// eigenvectors, the 6 x 10 distance system, three closed-form starts for the betas each refined by five Gauss-Newton steps, an
// absolute-orientation fit per start, the smallest mean reprojection error wins.  Factorizations are this file's own (cyclic
// Jacobi for the symmetric eigenproblems, one-sided Jacobi for the 3 x 3 SVD, Householder QR for the small least-squares solves):
// from 6 points on the pose is determined by the data and agrees with any other correct EPnP to rounding; at 5 points MtM has a
// two-dimensional null space and the pose depends on the basis the eigen-solver happens to return.
//
// The exception to (a): rodrigues() uses acos, and update_iters() pow / log.  rodrigues runs on the host only (library and
// emulation alike, on the same R).  update_iters runs on the device in the library, as the F-matrix RANSAC's does, and with glibc in
// the host build: the iteration count is therefore OUTSIDE the shared-source guarantee -- two libms have to agree after rint(), which
// they do unless num / denom lands within an ulp or so of a half -- and is held to the numpy replay separately (layer 3).
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PNP_HD __host__ __device__ inline
#else
#define PNP_HD inline
#endif

namespace uvo {
namespace pnp {

constexpr int kModelPoints = 5;

struct Cam {
  double fx, fy, cx, cy, k[8];  // k1 k2 p1 p2 k3 k4 k5 k6
};

// ---- cv::RNG and getSubset without checkSubset ---------------------------------------------------------------------------------
struct Rng {
  uint64_t s = ~0ull;
  uint32_t draws = 0;
  PNP_HD uint32_t next() {
    s = (s & 0xffffffffull) * 4164903690ull + (s >> 32);
    ++draws;
    return (uint32_t)s;
  }
};

PNP_HD void draw_subset(Rng& r, int n, int32_t* out) {
  int32_t ch[kModelPoints];
#pragma unroll
  for (int i = 0; i < kModelPoints; ++i) {
    int32_t v;
    bool dup;
    do {
      v = (int32_t)(r.next() % (uint32_t)n);
      dup = false;
#pragma unroll
      for (int j = 0; j < kModelPoints; ++j) dup |= j < i && v == ch[j];
    } while (dup);
    ch[i] = v;
  }
#pragma unroll
  for (int i = 0; i < kModelPoints; ++i) out[i] = ch[i];
}

// RANSACUpdateNumIters
PNP_HD int update_iters(double p, double ep, int model_points, int max_iters) {
  p = p < 0. ? 0. : p;
  p = p > 1. ? 1. : p;
  ep = ep < 0. ? 0. : ep;
  ep = ep > 1. ? 1. : ep;
  double num = 1. - p < DBL_MIN ? DBL_MIN : 1. - p;
  double denom = 1. - pow(1. - ep, (double)model_points);
  if (denom < DBL_MIN) return 0;
  num = log(num);
  denom = log(denom);
  return denom >= 0 || -num >= max_iters * (-denom) ? max_iters : (int)rint(num / denom);
}

// RANSACPointSetRegistrator::run over the counts of hypotheses that were all evaluated in advance: a hypothesis is taken iff its
// count exceeds max(best, modelPoints - 1); returns the winner (-1: none) and the iteration count at loop exit
PNP_HD int replay(const int32_t* counts, int n, double conf, int max_iters, int* iterations) {
  int niters = max_iters, best = -1, best_count = 0, it = 0;
  for (; it < niters; ++it) {
    const int c = counts[it];
    if (c > (best_count > kModelPoints - 1 ? best_count : kModelPoints - 1)) {
      best_count = c, best = it;
      niters = update_iters(conf, (double)(n - c) / n, kModelPoints, niters);
    }
  }
  *iterations = it;
  return best;
}

// ---- cv::undistortPoints without P (normalised coordinates): five fixed-point iterations of the Brown model -----------------------
PNP_HD void undistort_norm(const Cam& C, double u, double v, double* xo, double* yo) {
  const double ifx = 1. / C.fx, ify = 1. / C.fy;
  double x = (u - C.cx) * ifx, y = (v - C.cy) * ify;
  const double x0 = x, y0 = y;
  const double* k = C.k;
  for (int j = 0; j < 5; ++j) {
    const double r2 = x * x + y * y;
    const double icdist = (1 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2) / (1 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2);
    const double deltaX = 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x);
    const double deltaY = k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y;
    x = (x0 - deltaX) * icdist;
    y = (y0 - deltaY) * icdist;
  }
  *xo = x, *yo = y;
}

// ---- computeError: cv::projectPoints in double, the projection stored as float, the squared distance to the float image point ----
PNP_HD float project_error(const Cam& C, const double* R, const double* t, const float* P, const float* m) {
  const double X = P[0], Y = P[1], Z = P[2];
  double x = R[0] * X + R[1] * Y + R[2] * Z + t[0];
  double y = R[3] * X + R[4] * Y + R[5] * Z + t[1];
  double z = R[6] * X + R[7] * Y + R[8] * Z + t[2];
  z = z ? 1. / z : 1.;
  x *= z, y *= z;
  const double* k = C.k;
  const double r2 = x * x + y * y, r4 = r2 * r2, r6 = r4 * r2;
  const double a1 = 2 * x * y, a2 = r2 + 2 * x * x, a3 = r2 + 2 * y * y;
  const double cdist = 1 + k[0] * r2 + k[1] * r4 + k[4] * r6;
  const double icdist2 = 1. / (1 + k[5] * r2 + k[6] * r4 + k[7] * r6);
  const double xd = x * cdist * icdist2 + k[2] * a1 + k[3] * a2;
  const double yd = y * cdist * icdist2 + k[2] * a3 + k[3] * a1;
  const float pu = (float)(xd * C.fx + C.cx), pv = (float)(yd * C.fy + C.cy);
  const float dx = m[0] - pu, dy = m[1] - pv;
  return (float)((double)dx * (double)dx + (double)dy * (double)dy);
}

PNP_HD bool finite12(const double* p) {
  bool ok = true;
  for (int i = 0; i < 12; ++i) ok &= fabs(p[i]) <= DBL_MAX;  // false for NaN and infinities
  return ok;
}

// ---- the points of one EPnP call: list entry i is point idx[i]; image side = normalised coordinates (float-stored for the RANSAC
// subsets, double for the refit), brought back to pixels with fu, uc, fv, vc in double as epnp's init_points does ----------------------
struct Points {
  const float* obj;     // [.][3]
  const float* und_f;   // [.][2], used when und_d is null
  const double* und_d;  // [.][2]
  const int32_t* idx;
  int n;
  double fu, fv, uc, vc;
  PNP_HD void world(int i, double* p) const {
    const int j = idx[i];
    p[0] = obj[3 * j], p[1] = obj[3 * j + 1], p[2] = obj[3 * j + 2];
  }
  PNP_HD void pixel(int i, double* u, double* v) const {
    const int j = idx[i];
    const double x = und_d ? und_d[2 * j] : (double)und_f[2 * j], y = und_d ? und_d[2 * j + 1] : (double)und_f[2 * j + 1];
    *u = x * fu + uc, *v = y * fv + vc;
  }
};

// the same for a caller that holds pixel coordinates as they are (pnpsolver_core.hpp: PnPsolver::add_correspondence takes the
// undistorted key point's float u, v): solve() and what it calls take either form
struct PixelPoints {
  const float* obj;  // [.][3]
  const float* pix;  // [.][2]
  const int32_t* idx;
  int n;
  double fu, fv, uc, vc;
  PNP_HD void world(int i, double* p) const {
    const int j = idx[i];
    p[0] = obj[3 * j], p[1] = obj[3 * j + 1], p[2] = obj[3 * j + 2];
  }
  PNP_HD void pixel(int i, double* u, double* v) const {
    const int j = idx[i];
    *u = pix[2 * j], *v = pix[2 * j + 1];
  }
};

// workspace of one solve, in doubles; element e of a workspace with stride S lives at w[e * S] (S > 1: the workspaces of S lanes
// interleaved in LDS, so that the lanes of a wavefront touch neighbouring banks)
enum : int {
  W_CWS = 0,            // [4][3] control points, world
  W_CINV = 12,          // [3][3] inverse of the control-point axes
  W_MTM = 21,           // [12][12], after the eigen-solve its diagonal holds the eigenvalues
  W_EV = 165,           // [12][12] eigenvectors in columns
  W_L = 309,            // [6][10]
  W_RHO = 369,          // [6]
  W_LSA = 375,          // [6][5] least-squares system
  W_LSB = 405,          // [6]
  W_LSX = 411,          // [5]
  W_BETA = 416,         // [4]
  W_CCS = 420,          // [3 starts][4][3] control points, camera
  W_PC0 = 456,          // [3][3] centroid of the camera-frame points
  W_ABT = 465,          // [3][3][3] (first block doubles as the covariance of the map points)
  W_U3 = 492,           // [3][3][3]
  W_V3 = 519,           // [3][3][3]
  W_RT = 546,           // [3][12] R, t per start
  W_ERR = 582,          // [3]
  W_SEL = 585,          // [4] columns of W_EV with the four smallest eigenvalues, smallest first
  W_SIZE = 589
};

template <int S>
struct Ws {
  double* w;
  PNP_HD double& operator[](int e) const { return w[e * S]; }
};

struct NoSync {
  PNP_HD void operator()() const {}
};

// cyclic Jacobi for the symmetric n x n matrix at a (row-major, leading dimension n): eigenvalues on the diagonal, vectors in the
// columns of v.  A rotation is skipped once apq^2 <= 1e-32 app aqq or |apq| <= 1e-18 trace; at most 30 sweeps.
template <int S>
PNP_HD void jacobi_eig(const Ws<S>& W, int a, int v, int n) {
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) W[v + i * n + j] = i == j ? 1. : 0.;
  double scale = 0.;  // the trace: entries below 1e-18 of it are rounding noise of a matrix of this size whatever their diagonal
  for (int i = 0; i < n; ++i) scale += fabs(W[a + i * n + i]);
  const double floor_ = 1e-18 * scale;
  for (int sweep = 0; sweep < 30; ++sweep) {
    int rotated = 0;
    for (int p = 0; p < n - 1; ++p)
      for (int q = p + 1; q < n; ++q) {
        const double apq = W[a + p * n + q], app = W[a + p * n + p], aqq = W[a + q * n + q];
        // the relative test alone never ends inside a null space (two zero eigenvalues at five points): their diagonals are noise
        if (apq * apq <= 1e-32 * fabs(app * aqq) || fabs(apq) <= floor_) continue;
        ++rotated;
        const double theta = (aqq - app) / (2. * apq);
        const double t = (theta < 0. ? -1. : 1.) / (fabs(theta) + sqrt(theta * theta + 1.));
        const double c = 1. / sqrt(t * t + 1.), s = t * c;
        for (int k = 0; k < n; ++k) {
          if (k != p && k != q) {
            const double akp = W[a + k * n + p], akq = W[a + k * n + q];
            const double np_ = c * akp - s * akq, nq_ = s * akp + c * akq;
            W[a + k * n + p] = np_, W[a + p * n + k] = np_;
            W[a + k * n + q] = nq_, W[a + q * n + k] = nq_;
          }
          const double vkp = W[v + k * n + p], vkq = W[v + k * n + q];
          W[v + k * n + p] = c * vkp - s * vkq;
          W[v + k * n + q] = s * vkp + c * vkq;
        }
        W[a + p * n + p] = app - t * apq;
        W[a + q * n + q] = aqq + t * apq;
        W[a + p * n + q] = 0., W[a + q * n + p] = 0.;
      }
    if (!rotated) break;
  }
}

// one-sided Jacobi SVD of the 3 x 3 matrix at g (overwritten): g = U diag V^T with U at u, V at v (columns).  A column of g that
// vanishes against the largest gets the cross product of the other two as its U column (rank-2 input: coplanar points).
template <int S>
PNP_HD void svd3(const Ws<S>& W, int g, int u, int v) {
  for (int i = 0; i < 9; ++i) W[v + i] = (i & 3) == 0 ? 1. : 0.;
  for (int sweep = 0; sweep < 30; ++sweep) {
    int rotated = 0;
    for (int p = 0; p < 2; ++p)
      for (int q = p + 1; q < 3; ++q) {
        double al = 0., be = 0., ga = 0.;
        for (int k = 0; k < 3; ++k) {
          const double gp = W[g + 3 * k + p], gq = W[g + 3 * k + q];
          al += gp * gp, be += gq * gq, ga += gp * gq;
        }
        if (ga * ga <= 1e-32 * (al * be)) continue;
        ++rotated;
        const double zeta = (be - al) / (2. * ga);
        const double t = (zeta < 0. ? -1. : 1.) / (fabs(zeta) + sqrt(zeta * zeta + 1.));
        const double c = 1. / sqrt(t * t + 1.), s = t * c;
        for (int k = 0; k < 3; ++k) {
          const double gp = W[g + 3 * k + p], gq = W[g + 3 * k + q];
          W[g + 3 * k + p] = c * gp - s * gq, W[g + 3 * k + q] = s * gp + c * gq;
          const double vp = W[v + 3 * k + p], vq = W[v + 3 * k + q];
          W[v + 3 * k + p] = c * vp - s * vq, W[v + 3 * k + q] = s * vp + c * vq;
        }
      }
    if (!rotated) break;
  }
  const double n0 = sqrt(W[g] * W[g] + W[g + 3] * W[g + 3] + W[g + 6] * W[g + 6]);
  const double n1 = sqrt(W[g + 1] * W[g + 1] + W[g + 4] * W[g + 4] + W[g + 7] * W[g + 7]);
  const double n2 = sqrt(W[g + 2] * W[g + 2] + W[g + 5] * W[g + 5] + W[g + 8] * W[g + 8]);
  const double big = n0 > n1 ? (n0 > n2 ? n0 : n2) : (n1 > n2 ? n1 : n2);
  const int jmin = n0 <= n1 ? (n0 <= n2 ? 0 : 2) : (n1 <= n2 ? 1 : 2);
  const double small = jmin == 0 ? n0 : jmin == 1 ? n1 : n2;
  const double i0 = 1. / n0, i1 = 1. / n1, i2 = 1. / n2;
  for (int k = 0; k < 3; ++k) W[u + 3 * k] = W[g + 3 * k] * i0, W[u + 3 * k + 1] = W[g + 3 * k + 1] * i1, W[u + 3 * k + 2] = W[g + 3 * k + 2] * i2;
  if (small <= 1e-12 * big) {
    const int a = (jmin + 1) % 3, b = (jmin + 2) % 3;
    W[u + 0 + jmin] = W[u + 3 + a] * W[u + 6 + b] - W[u + 6 + a] * W[u + 3 + b];
    W[u + 3 + jmin] = W[u + 6 + a] * W[u + 0 + b] - W[u + 0 + a] * W[u + 6 + b];
    W[u + 6 + jmin] = W[u + 0 + a] * W[u + 3 + b] - W[u + 3 + a] * W[u + 0 + b];
  }
}

// least squares of the 6 x nc system at W_LSA (leading dimension 5) / W_LSB by Householder QR; the solution goes to W_LSX
template <int S>
PNP_HD void qr_solve6(const Ws<S>& W, int nc) {
  const int m = 6, ld = 5;
  for (int c = 0; c < nc; ++c) {
    double sigma = 0.;
    for (int r = c + 1; r < m; ++r) sigma += W[W_LSA + r * ld + c] * W[W_LSA + r * ld + c];
    const double x = W[W_LSA + c * ld + c];
    if (sigma == 0.) continue;
    const double mu = sqrt(x * x + sigma);
    const double v0 = x <= 0. ? x - mu : -sigma / (x + mu);
    const double beta = 2. * v0 * v0 / (sigma + v0 * v0), iv0 = 1. / v0;
    for (int r = c + 1; r < m; ++r) W[W_LSA + r * ld + c] *= iv0;  // the Householder vector, v[c] = 1
    for (int j = c + 1; j <= nc; ++j) {                             // column nc stands for the right-hand side
      const int col = j < nc ? W_LSA + j : W_LSB, st = j < nc ? ld : 1;
      double w = W[col + c * st];
      for (int r = c + 1; r < m; ++r) w += W[W_LSA + r * ld + c] * W[col + r * st];
      w *= beta;
      W[col + c * st] -= w;
      for (int r = c + 1; r < m; ++r) W[col + r * st] -= w * W[W_LSA + r * ld + c];
    }
    W[W_LSA + c * ld + c] = mu;  // H x = mu e_c for either form of v0
  }
  for (int c = nc - 1; c >= 0; --c) {
    double s = W[W_LSB + c];
    for (int j = c + 1; j < nc; ++j) s -= W[W_LSA + c * ld + j] * W[W_LSX + j];
    W[W_LSX + c] = s / W[W_LSA + c * ld + c];
  }
}

PNP_HD double pick3(const double* p, int k) { return k == 0 ? p[0] : k == 1 ? p[1] : p[2]; }
PNP_HD double pick(const double* p, int k) { return k == 0 ? p[0] : k == 1 ? p[1] : k == 2 ? p[2] : p[3]; }

template <int S>
PNP_HD void alphas_of(const Ws<S>& W, const double* p, double* a) {
  const double d0 = p[0] - W[W_CWS], d1 = p[1] - W[W_CWS + 1], d2 = p[2] - W[W_CWS + 2];
  a[1] = W[W_CINV + 0] * d0 + W[W_CINV + 1] * d1 + W[W_CINV + 2] * d2;
  a[2] = W[W_CINV + 3] * d0 + W[W_CINV + 4] * d1 + W[W_CINV + 5] * d2;
  a[3] = W[W_CINV + 6] * d0 + W[W_CINV + 7] * d1 + W[W_CINV + 8] * d2;
  a[0] = 1. - a[1] - a[2] - a[3];
}

// point i in the camera frame of start c: the barycentric combination of that start's control points
template <int S, class Pts>
PNP_HD void camera_point(const Ws<S>& W, const Pts& P, int c, int i, double* pc, double* pw) {
  double a[4];
  P.world(i, pw);
  alphas_of(W, pw, a);
  const int cc = W_CCS + 12 * c;
  for (int j = 0; j < 3; ++j) pc[j] = a[0] * W[cc + j] + a[1] * W[cc + 3 + j] + a[2] * W[cc + 6 + j] + a[3] * W[cc + 9 + j];
}

// the closed-form start `c` for the betas from the 6 x 10 system, then five Gauss-Newton steps; leaves W_BETA
template <int S>
PNP_HD void betas_of_start(const Ws<S>& W, int c) {
  const int nc = c == 0 ? 4 : c == 1 ? 3 : 5;
  for (int r = 0; r < 6; ++r) {
    for (int j = 0; j < nc; ++j) W[W_LSA + r * 5 + j] = W[W_L + r * 10 + (c != 0 ? j : j < 2 ? j : j == 2 ? 3 : 6)];
    W[W_LSB + r] = W[W_RHO + r];
  }
  qr_solve6(W, nc);
  const double b0 = W[W_LSX], b1 = W[W_LSX + 1], b2 = W[W_LSX + 2], b3 = W[W_LSX + 3];
  if (c == 0) {
    const double r0 = sqrt(b0 < 0. ? -b0 : b0), sg = b0 < 0. ? -1. : 1.;
    W[W_BETA] = r0, W[W_BETA + 1] = sg * b1 / r0, W[W_BETA + 2] = sg * b2 / r0, W[W_BETA + 3] = sg * b3 / r0;
  } else {
    double x0, x1;
    if (b0 < 0.)
      x0 = sqrt(-b0), x1 = b2 < 0. ? sqrt(-b2) : 0.;
    else
      x0 = sqrt(b0), x1 = b2 > 0. ? sqrt(b2) : 0.;
    if (b1 < 0.) x0 = -x0;
    W[W_BETA] = x0, W[W_BETA + 1] = x1, W[W_BETA + 2] = c == 2 ? b3 / x0 : 0., W[W_BETA + 3] = 0.;
  }
  for (int it = 0; it < 5; ++it) {
    const double e0 = W[W_BETA], e1 = W[W_BETA + 1], e2 = W[W_BETA + 2], e3 = W[W_BETA + 3];
    for (int r = 0; r < 6; ++r) {
      const int l = W_L + r * 10;
      W[W_LSA + r * 5 + 0] = 2 * W[l] * e0 + W[l + 1] * e1 + W[l + 3] * e2 + W[l + 6] * e3;
      W[W_LSA + r * 5 + 1] = W[l + 1] * e0 + 2 * W[l + 2] * e1 + W[l + 4] * e2 + W[l + 7] * e3;
      W[W_LSA + r * 5 + 2] = W[l + 3] * e0 + W[l + 4] * e1 + 2 * W[l + 5] * e2 + W[l + 8] * e3;
      W[W_LSA + r * 5 + 3] = W[l + 6] * e0 + W[l + 7] * e1 + W[l + 8] * e2 + 2 * W[l + 9] * e3;
      W[W_LSB + r] = W[W_RHO + r] - (W[l] * e0 * e0 + W[l + 1] * e0 * e1 + W[l + 2] * e1 * e1 + W[l + 3] * e0 * e2 + W[l + 4] * e1 * e2 +
                                     W[l + 5] * e2 * e2 + W[l + 6] * e0 * e3 + W[l + 7] * e1 * e3 + W[l + 8] * e2 * e3 + W[l + 9] * e3 * e3);
    }
    qr_solve6(W, 4);
    for (int j = 0; j < 4; ++j) W[W_BETA + j] += W[W_LSX + j];
  }
}

// everything between MtM and the three candidate sets of camera-frame control points; one lane
template <int S, class Pts>
PNP_HD void solve_from_mtm(const Ws<S>& W, const Pts& P) {
  jacobi_eig(W, W_MTM, W_EV, 12);
  unsigned used = 0;
  for (int s = 0; s < 4; ++s) {  // the four smallest eigenvalues, smallest first (always four valid columns, NaN or not)
    int sel = -1;
    for (int i = 0; i < 12; ++i)
      if (!(used >> i & 1) && (sel < 0 || W[W_MTM + i * 13] < W[W_MTM + sel * 13])) sel = i;
    used |= 1u << sel;
    W[W_SEL + s] = (double)sel;
  }
  if (P.n == kModelPoints) {
    // Five points: M is 10 x 12, the two smallest eigenvalues are both zero and any rotation of their two vectors is as good an answer
    // of the eigen-solver as what it returned.  The closed-form starts are not indifferent to it: when the solution happens to lie
    // along one of the two, b00 or b11 of the N = 2 start is zero up to noise, its square root takes the wrong branch and a subset of
    // five good points yields a useless pose (about one in a hundred, with any solver).  So the basis is chosen, not inherited: the
    // second vector gets no net depth (its four z components sum to zero), the first all of it -- every point in front of the camera
    // then needs a first coefficient that is safely away from zero.
    const int c0 = (int)W[W_SEL], c1 = (int)W[W_SEL + 1];
    const double z0 = W[W_EV + 2 * 12 + c0] + W[W_EV + 5 * 12 + c0] + W[W_EV + 8 * 12 + c0] + W[W_EV + 11 * 12 + c0];
    const double z1 = W[W_EV + 2 * 12 + c1] + W[W_EV + 5 * 12 + c1] + W[W_EV + 8 * 12 + c1] + W[W_EV + 11 * 12 + c1];
    const double r = sqrt(z0 * z0 + z1 * z1);
    if (r > 0.) {
      const double c = z0 / r, s = z1 / r;
      for (int e = 0; e < 12; ++e) {
        const double a = W[W_EV + e * 12 + c0], b = W[W_EV + e * 12 + c1];
        W[W_EV + e * 12 + c0] = c * a + s * b;
        W[W_EV + e * 12 + c1] = c * b - s * a;
      }
    }
  }
  for (int r = 0; r < 6; ++r) {  // the six pairs of control points: (0,1) (0,2) (0,3) (1,2) (1,3) (2,3)
    const int pa = r < 3 ? 0 : r < 5 ? 1 : 2, pb = r < 3 ? r + 1 : r < 5 ? r - 1 : 3;
    const int dv = W_LSA;  // [4][3]: the pair's difference in each of the four eigenvectors
    for (int i = 0; i < 4; ++i) {
      const int col = (int)W[W_SEL + i];
      for (int k = 0; k < 3; ++k) W[dv + 3 * i + k] = W[W_EV + (3 * pa + k) * 12 + col] - W[W_EV + (3 * pb + k) * 12 + col];
    }
    int e = 0;  // columns: b00 b01 b11 b02 b12 b22 b03 b13 b23 b33
    for (int j = 0; j < 4; ++j)
      for (int i = 0; i <= j; ++i, ++e) {
        const double d = W[dv + 3 * i] * W[dv + 3 * j] + W[dv + 3 * i + 1] * W[dv + 3 * j + 1] + W[dv + 3 * i + 2] * W[dv + 3 * j + 2];
        W[W_L + r * 10 + e] = i == j ? d : 2. * d;
      }
    double rho = 0.;
    for (int k = 0; k < 3; ++k) {
      const double d = W[W_CWS + 3 * pa + k] - W[W_CWS + 3 * pb + k];
      rho += d * d;
    }
    W[W_RHO + r] = rho;
  }
  for (int c = 0; c < 3; ++c) {
    betas_of_start(W, c);
    for (int e = 0; e < 12; ++e) {
      double s = 0.;
      for (int i = 0; i < 4; ++i) s += W[W_BETA + i] * W[W_EV + e * 12 + (int)W[W_SEL + i]];
      W[W_CCS + 12 * c + e] = s;
    }
    double pc[3], pw[3];  // the sign: the first point has to lie in front of the camera
    camera_point(W, P, c, 0, pc, pw);
    if (pc[2] < 0.)
      for (int e = 0; e < 12; ++e) W[W_CCS + 12 * c + e] = -W[W_CCS + 12 * c + e];
  }
}

// R, t of start c from the 3 x 3 correlation of the centred camera-frame and world points
template <int S>
PNP_HD void orientation(const Ws<S>& W, int c) {
  const int g = W_ABT + 9 * c, u = W_U3 + 9 * c, v = W_V3 + 9 * c, rt = W_RT + 12 * c;
  svd3(W, g, u, v);
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) W[rt + 3 * i + j] = W[u + 3 * i] * W[v + 3 * j] + W[u + 3 * i + 1] * W[v + 3 * j + 1] + W[u + 3 * i + 2] * W[v + 3 * j + 2];
  const double det = W[rt] * W[rt + 4] * W[rt + 8] + W[rt + 1] * W[rt + 5] * W[rt + 6] + W[rt + 2] * W[rt + 3] * W[rt + 7] -
                     W[rt + 2] * W[rt + 4] * W[rt + 6] - W[rt + 1] * W[rt + 3] * W[rt + 8] - W[rt] * W[rt + 5] * W[rt + 7];
  if (det < 0.)
    for (int j = 0; j < 3; ++j) W[rt + 6 + j] = -W[rt + 6 + j];
  for (int i = 0; i < 3; ++i)
    W[rt + 9 + i] = W[W_PC0 + 3 * c + i] - (W[rt + 3 * i] * W[W_CWS] + W[rt + 3 * i + 1] * W[W_CWS + 1] + W[rt + 3 * i + 2] * W[W_CWS + 2]);
}

// EPnP on the points P with `lanes` cooperating callers (this one is `lane`), `sync` between phases.  out: R (9, row-major), t (3) of
// the start with the smallest mean reprojection error whose pose is finite; returns whether there is one (out untouched if not).
// Every lane returns the same value; lane 0 writes out.
template <int S, class Sync, class Pts>
PNP_HD bool solve(const Ws<S>& W, const Pts& P, int lane, int lanes, const Sync& sync, double* out) {
  const int n = P.n;
  const double inv_n = 1. / (double)n;
  // 1. centroid = control point 0
  for (int k = lane; k < 3; k += lanes) {
    double s = 0.;
    for (int i = 0; i < n; ++i) {
      double p[3];
      P.world(i, p);
      s += pick3(p, k);
    }
    W[W_CWS + k] = s * inv_n;
  }
  sync();
  // 2. covariance (upper triangle, mirrored)
  for (int k = lane; k < 6; k += lanes) {
    const int a = k < 3 ? 0 : k < 5 ? 1 : 2, b = k < 3 ? k : k < 5 ? k - 2 : 2;
    const double ca = W[W_CWS + a], cb = W[W_CWS + b];
    double s = 0.;
    for (int i = 0; i < n; ++i) {
      double p[3];
      P.world(i, p);
      s += (pick3(p, a) - ca) * (pick3(p, b) - cb);
    }
    W[W_ABT + 3 * a + b] = s, W[W_ABT + 3 * b + a] = s;
  }
  sync();
  // 3. principal axes -> control points 1..3 and the inverse of their axes (an axis of no extent contributes nothing)
  if (lane == 0) {
    jacobi_eig(W, W_ABT, W_V3, 3);
    const double e0 = W[W_ABT], e1 = W[W_ABT + 4], e2 = W[W_ABT + 8];
    const double emax = e0 > e1 ? (e0 > e2 ? e0 : e2) : (e1 > e2 ? e1 : e2);
    for (int j = 0; j < 3; ++j) {
      const double ev = W[W_ABT + 4 * j];
      const double len = sqrt((ev > 0. ? ev : 0.) * inv_n);
      const double inv = ev > 1e-18 * emax ? 1. / len : 0.;
      // the axis's sign by convention: its largest component positive.  With noisy data the pose depends on it (the control points
      // c0 + axis and c0 - axis give systems that are no orthogonal transform of each other), so it has to be fixed, not inherited
      const double a0 = W[W_V3 + j], a1 = W[W_V3 + 3 + j], a2 = W[W_V3 + 6 + j];
      const double big = fabs(a0) >= fabs(a1) ? (fabs(a0) >= fabs(a2) ? a0 : a2) : (fabs(a1) >= fabs(a2) ? a1 : a2);
      const double sg = big < 0. ? -1. : 1.;
      for (int k = 0; k < 3; ++k) {
        const double ax = sg * W[W_V3 + 3 * k + j];
        W[W_CWS + 3 * (j + 1) + k] = W[W_CWS + k] + len * ax;
        W[W_CINV + 3 * j + k] = inv * ax;
      }
    }
  }
  sync();
  // 4. MtM: entry (r, c), r <= c, summed over the points in list order
  for (int k = lane; k < 78; k += lanes) {
    int r = 0, c = k;
    while (c >= 12 - r) c -= 12 - r, ++r;
    c += r;
    const int jr = r / 3, kr = r - 3 * jr, jc = c / 3, kc = c - 3 * jc;
    double s = 0.;
    for (int i = 0; i < n; ++i) {
      double p[3], a[4], u, v;
      P.world(i, p);
      alphas_of(W, p, a);
      P.pixel(i, &u, &v);
      const double ar = pick(a, jr), ac = pick(a, jc);
      const double m0r = kr == 0 ? ar * P.fu : kr == 2 ? ar * (P.uc - u) : 0., m1r = kr == 1 ? ar * P.fv : kr == 2 ? ar * (P.vc - v) : 0.;
      const double m0c = kc == 0 ? ac * P.fu : kc == 2 ? ac * (P.uc - u) : 0., m1c = kc == 1 ? ac * P.fv : kc == 2 ? ac * (P.vc - v) : 0.;
      s += m0r * m0c + m1r * m1c;
    }
    W[W_MTM + r * 12 + c] = s, W[W_MTM + c * 12 + r] = s;
  }
  sync();
  // 5. null space, betas, the three sets of camera-frame control points
  if (lane == 0) solve_from_mtm(W, P);
  sync();
  // 6. centroid of the camera-frame points per start
  for (int k = lane; k < 9; k += lanes) {
    const int c = k / 3, j = k - 3 * c;
    double s = 0.;
    for (int i = 0; i < n; ++i) {
      double pc[3], pw[3];
      camera_point(W, P, c, i, pc, pw);
      s += pick3(pc, j);
    }
    W[W_PC0 + k] = s * inv_n;
  }
  sync();
  // 7. correlation per start
  for (int k = lane; k < 27; k += lanes) {
    const int c = k / 9, j = (k - 9 * c) / 3, l = k - 9 * c - 3 * j;
    const double pcj = W[W_PC0 + 3 * c + j], pwl = W[W_CWS + l];
    double s = 0.;
    for (int i = 0; i < n; ++i) {
      double pc[3], pw[3];
      camera_point(W, P, c, i, pc, pw);
      s += (pick3(pc, j) - pcj) * (pick3(pw, l) - pwl);
    }
    W[W_ABT + k] = s;
  }
  sync();
  // 8. R, t per start
  for (int c = lane; c < 3; c += lanes) orientation(W, c);
  sync();
  // 9. mean reprojection error per start
  for (int c = lane; c < 3; c += lanes) {
    const int rt = W_RT + 12 * c;
    double s = 0.;
    for (int i = 0; i < n; ++i) {
      double p[3], u, v;
      P.world(i, p);
      P.pixel(i, &u, &v);
      const double xc = W[rt] * p[0] + W[rt + 1] * p[1] + W[rt + 2] * p[2] + W[rt + 9];
      const double yc = W[rt + 3] * p[0] + W[rt + 4] * p[1] + W[rt + 5] * p[2] + W[rt + 10];
      const double iz = 1. / (W[rt + 6] * p[0] + W[rt + 7] * p[1] + W[rt + 8] * p[2] + W[rt + 11]);
      const double du = u - (P.uc + P.fu * xc * iz), dv = v - (P.vc + P.fv * yc * iz);
      s += sqrt(du * du + dv * dv);
    }
    W[W_ERR + c] = s * inv_n;
  }
  sync();
  // 10. the best start
  int best = -1;
  for (int c = 0; c < 3; ++c) {
    bool fin = fabs(W[W_ERR + c]) <= DBL_MAX;
    for (int e = 0; e < 12; ++e) fin &= fabs(W[W_RT + 12 * c + e]) <= DBL_MAX;
    if (fin && (best < 0 || W[W_ERR + c] < W[W_ERR + best])) best = c;
  }
  if (best >= 0 && lane == 0)
    for (int e = 0; e < 12; ++e) out[e] = W[W_RT + 12 * best + e];
  return best >= 0;
}

// cv::Rodrigues, matrix -> vector: R is first replaced by U V^T of its SVD.  Host only (acos).
inline void rodrigues(const double* Rin, double* rvec) {
  double buf[27];
  Ws<1> W{buf};
  for (int i = 0; i < 9; ++i) buf[i] = Rin[i];
  svd3(W, 0, 9, 18);
  double R[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) R[3 * i + j] = buf[9 + 3 * i] * buf[18 + 3 * j] + buf[9 + 3 * i + 1] * buf[18 + 3 * j + 1] + buf[9 + 3 * i + 2] * buf[18 + 3 * j + 2];
  double rx = R[7] - R[5], ry = R[2] - R[6], rz = R[3] - R[1];
  const double s = sqrt((rx * rx + ry * ry + rz * rz) * 0.25);
  double c = (R[0] + R[4] + R[8] - 1) * 0.5;
  c = c > 1. ? 1. : c < -1. ? -1. : c;
  double theta = acos(c);
  if (s < 1e-5) {
    if (c > 0) {
      rx = ry = rz = 0;
    } else {
      double t = (R[0] + 1) * 0.5;
      rx = sqrt(t > 0. ? t : 0.);
      t = (R[4] + 1) * 0.5;
      ry = sqrt(t > 0. ? t : 0.) * (R[1] < 0 ? -1. : 1.);
      t = (R[8] + 1) * 0.5;
      rz = sqrt(t > 0. ? t : 0.) * (R[2] < 0 ? -1. : 1.);
      if (fabs(rx) < fabs(ry) && fabs(rx) < fabs(rz) && (R[5] > 0) != (ry * rz > 0)) rz = -rz;
      theta /= sqrt(rx * rx + ry * ry + rz * rz);
      rx *= theta, ry *= theta, rz *= theta;
    }
  } else {
    const double vth = 1. / (2 * s) * theta;
    rx *= vth, ry *= vth, rz *= vth;
  }
  rvec[0] = rx, rvec[1] = ry, rvec[2] = rz;
}

}  // namespace pnp
}  // namespace uvo
