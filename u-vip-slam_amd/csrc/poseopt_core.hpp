// Optimizer::PoseOptimization(Frame*) (src/Optimizer.cc:2012-2145 of the reference, with the parts of g2o it runs: the Levenberg
// driver, EdgeSE3ProjectXYZ, the Huber kernel, SE3Quat, the dense 6 x 6 solve) as plain C++ in double.  poseopt.hip runs this on the
// device, tests/emu/poseopt_emu.cpp on the host; the two are held to each other bit for bit under the rules of epnp_core.hpp's
// header: IEEE + - * / sqrt and fabs only, no contraction (-ffp-contract=off on both sides), no library function.
//
// One rule is new here.  The other cores give every lane whole scalars and never reduce a floating-point value across lanes; this
// one has to, so: SUMS OVER EDGES ARE REDUCED IN ONE FIXED SHAPE.
//   1. Lane l of kLanes = 256 adds the terms of its edges l, l + 256, l + 512, ... in ascending order onto 0.0, skipping the edges
//      that are not active (level 1).
//   2. The 64 lane sums of a wavefront combine in a butterfly: for m = 32, 16, 8, 4, 2, 1 every lane replaces its value v by
//      v + (the value of lane l ^ m).  IEEE addition commutes, so all 64 lanes hold the same bits afterwards, those of the fold
//      s[l] = s[l] + s[l + m] for l < m.
//   3. The four wavefront sums w0..w3 combine as (w0 + w1) + (w2 + w3).
// The sums of a linearisation go to a place all members read (Team::shared(): 28 words of LDS on the device), so that they do not
// occupy 56 registers of every lane for the ten trials that use them; a trial's one sum comes back in a register.
// The shape depends on nothing but the edge index: not on n, not on the values, not on how many edges are active.  A Team does the
// walking: the device's (LaneTeam) is the 256 lanes of a workgroup, the host's (HostLaneTeam) one thread that plays lane 0..255
// in turn and folds as in 2 and 3; both are lane_team.hpp's, which sim3opt and ba walk too.  There are 21 + 6 + 1 sums per linearisation (H's upper triangle, b, the robust chi2) and one
// per trial (the robust chi2 at the tried pose).  Counts are integers and need no rule.
//
// Everything that is not a sum over edges -- the 6 x 6 solve, exp, the pose product, the Levenberg decision -- is computed by every
// lane from the same reduced values, so every branch below is uniform over the team.
//
// Departures from the reference, stated in uvo.h and DESIGN.md section 4:
//   * the solve is an unpivoted LDL^T (solve6), "ok" meaning every pivot is finite and > 0; Eigen's LDLT pivots and accepts
//     semi-definite matrices.  On a failed solve dx keeps its previous value (zero at the start of a round), as the reference's x does.
//   * sin, cos are sim3::sincos (IEEE operations only, about 2^-51 absolute), pow(x, 3) is x * x * x.  sim3::sincos answers NaN above
//     7 rad: a step with |omega| > 7 makes the tried pose NaN, its chi2 NaN, and the trial is rejected as any NaN trial is
//     (rho > 0 is false; the pose is restored; the trial loop ends because rho < 0 is false as well).
//   * where the reference multiplies by the zeros of a matrix (information's off-diagonal, skew's diagonal) this file keeps the
//     products that decide a class (chi2: 0 * inf is NaN) and drops those inside H and b, where a non-finite term ends in a failed
//     solve either way.
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>

#include "lane_team.hpp"
#include "sim3_core.hpp"

#if defined(__HIPCC__)
#define PO_HD __host__ __device__ __forceinline__
#else
#define PO_HD inline
#endif

#if defined(__clang__)
#define PO_NOUNROLL _Pragma("nounroll")  // the loops over rounds, iterations, trials and a lane's edges: one body each
#else
#define PO_NOUNROLL
#endif

namespace uvo {
namespace poseopt {

constexpr int kLanes = kTeamLanes;
constexpr int kRounds = 4;
constexpr int kMaxTrials = 10;        // _maxTrialsAfterFailure
constexpr int kSums = 28;             // 21 of H, 6 of b, the robust chi2
constexpr int kMaxLin = 32;           // 10 + 10 + 7 + 5 linearisations at the most
constexpr int kMaxTrialRecs = 320;    // ten trials each

// seeded mutations, for the host build only (tests/emu/poseopt_emu.cpp); the library instantiates MUT = 0
constexpr int kMutNone = 0, kMutHuberB = 1, kMutNoReeval = 2, kMutBreakActive = 3, kMutLambdaOnce = 4, kMutNoRestore = 5,
              kMutScale = 6;

PO_HD int its_of(int round) { return round == 0 ? 10 : round == 1 ? 10 : round == 2 ? 7 : 5; }
PO_HD float th_of(int round) { return round == 0 ? 9.210f : round == 1 ? 7.378f : 5.991f; }
// const float delta = sqrt(5.991): the double root, rounded to float; setDelta widens it again
constexpr double kDelta = (double)0x1.394ca8p+1f;

struct Pose {
  double q[4];  // x y z w, unit, w >= 0
  double t[3];
};

struct Cam {
  double fx, fy, cx, cy;  // the frame's floats, widened (EdgeSE3ProjectXYZ's members are doubles)
};

// per-edge state bits
constexpr uint8_t kLevel = 1, kFlag = 2;

struct Edges {
  const float* in;   // [n][6]: the point, the observation, invSigma2
  double* chi2;      // [n] chi2 of the stored error: that of the last evaluation, accepted or not
  uint8_t* state;    // [n] kLevel | kFlag
  uint8_t* mask;     // [n] the flag after the last round run, for the caller
  int n;
};

// the layout of uvo_pose_trace (uvo.h); poseopt.hip asserts the sizes equal
struct TraceLin {
  int32_t round, iteration;
  double H[21], b[6], chi2;
};
struct TraceTrial {
  int32_t lin, ok, accepted, pad_;
  double lambda, cur, tmp, scale;
};
struct Trace {
  int32_t n_lin, n_trials;
  double R[9], t[3];
  TraceLin lin[kMaxLin];
  TraceTrial trial[kMaxTrialRecs];
};

struct Out {
  float Tcw[16];
  int32_t n_inliers, rounds;
};

// ---- SE3Quat -------------------------------------------------------------------------------------------------------------------------
// normalizeRotation: w < 0 flips every coefficient, then coeffs / norm
PO_HD void normalize_rotation(double q[4]) {
  if (q[3] < 0.) q[0] = q[0] * -1., q[1] = q[1] * -1., q[2] = q[2] * -1., q[3] = q[3] * -1.;
  const double nrm = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  q[0] = q[0] / nrm, q[1] = q[1] / nrm, q[2] = q[2] / nrm, q[3] = q[3] / nrm;
}

// Eigen's Quaternion(Matrix3): R row-major
PO_HD void quat_of(const double R[9], double q[4]) {
  double t = R[0] + R[4] + R[8];
  if (t > 0.) {
    t = sqrt(t + 1.);
    q[3] = 0.5 * t;
    t = 0.5 / t;
    q[0] = (R[7] - R[5]) * t, q[1] = (R[2] - R[6]) * t, q[2] = (R[3] - R[1]) * t;
  } else if (R[4] > R[0] ? R[8] > R[4] : R[8] > R[0]) {  // i = 2, j = 0, k = 1
    t = sqrt(R[8] - R[0] - R[4] + 1.);
    q[2] = 0.5 * t;
    t = 0.5 / t;
    q[3] = (R[3] - R[1]) * t, q[0] = (R[2] + R[6]) * t, q[1] = (R[5] + R[7]) * t;
  } else if (R[4] > R[0]) {  // i = 1, j = 2, k = 0
    t = sqrt(R[4] - R[8] - R[0] + 1.);
    q[1] = 0.5 * t;
    t = 0.5 / t;
    q[3] = (R[2] - R[6]) * t, q[2] = (R[7] + R[5]) * t, q[0] = (R[1] + R[3]) * t;
  } else {  // i = 0, j = 1, k = 2
    t = sqrt(R[0] - R[4] - R[8] + 1.);
    q[0] = 0.5 * t;
    t = 0.5 / t;
    q[3] = (R[7] - R[5]) * t, q[1] = (R[3] + R[1]) * t, q[2] = (R[6] + R[2]) * t;
  }
}

// Eigen's toRotationMatrix
PO_HD void rotation_of(const double q[4], double R[9]) {
  const double tx = 2. * q[0], ty = 2. * q[1], tz = 2. * q[2];
  const double twx = tx * q[3], twy = ty * q[3], twz = tz * q[3];
  const double txx = tx * q[0], txy = ty * q[0], txz = tz * q[0];
  const double tyy = ty * q[1], tyz = tz * q[1], tzz = tz * q[2];
  R[0] = 1. - (tyy + tzz), R[1] = txy - twz, R[2] = txz + twy;
  R[3] = txy + twz, R[4] = 1. - (txx + tzz), R[5] = tyz - twx;
  R[6] = txz - twy, R[7] = tyz + twx, R[8] = 1. - (txx + tyy);
}

// Eigen's quaternion * vector: uv = 2 (q.vec x v); v + w uv + q.vec x uv
PO_HD void rotate(const double q[4], double v0, double v1, double v2, double o[3]) {
  double u0 = q[1] * v2 - q[2] * v1, u1 = q[2] * v0 - q[0] * v2, u2 = q[0] * v1 - q[1] * v0;
  u0 = u0 + u0, u1 = u1 + u1, u2 = u2 + u2;
  o[0] = (v0 + q[3] * u0) + (q[1] * u2 - q[2] * u1);
  o[1] = (v1 + q[3] * u1) + (q[2] * u0 - q[0] * u2);
  o[2] = (v2 + q[3] * u2) + (q[0] * u1 - q[1] * u0);
}

// toSE3Quat: the float matrix widened, SE3Quat(R, t)
PO_HD void pose_of(const float T[16], Pose& P) {
  const double R[9] = {(double)T[0], (double)T[1], (double)T[2], (double)T[4], (double)T[5], (double)T[6], (double)T[8], (double)T[9], (double)T[10]};
  quat_of(R, P.q);
  normalize_rotation(P.q);
  P.t[0] = (double)T[3], P.t[1] = (double)T[7], P.t[2] = (double)T[11];
}

// toCvMat(to_homogeneous_matrix()), and the double R, t for the trace
PO_HD void matrix_of(const Pose& P, float T[16], double R[9]) {
  rotation_of(P.q, R);
  T[0] = (float)R[0], T[1] = (float)R[1], T[2] = (float)R[2], T[3] = (float)P.t[0];
  T[4] = (float)R[3], T[5] = (float)R[4], T[6] = (float)R[5], T[7] = (float)P.t[1];
  T[8] = (float)R[6], T[9] = (float)R[7], T[10] = (float)R[8], T[11] = (float)P.t[2];
  T[12] = 0.f, T[13] = 0.f, T[14] = 0.f, T[15] = 1.f;
}

// oplusImpl: exp(dx) * estimate.  dx = (omega, upsilon).
PO_HD void oplus(const double dx[6], const Pose& P, Pose& out) {
  const double o0 = dx[0], o1 = dx[1], o2 = dx[2];
  const double theta = sqrt(o0 * o0 + o1 * o1 + o2 * o2);
  const double Om[9] = {0., -o2, o1, o2, 0., -o0, -o1, o0, 0.};
  double Om2[9];
  SIM3_UNROLL
  for (int i = 0; i < 3; ++i)
    SIM3_UNROLL
    for (int j = 0; j < 3; ++j) Om2[i * 3 + j] = (Om[i * 3] * Om[j] + Om[i * 3 + 1] * Om[3 + j]) + Om[i * 3 + 2] * Om[6 + j];
  double R[9], V[9];
  if (theta < 0.00001) {
    SIM3_UNROLL
    for (int e = 0; e < 9; ++e) R[e] = ((e % 4 == 0 ? 1. : 0.) + Om[e]) + Om2[e], V[e] = R[e];
  } else {
    double sn, cs;
    sim3::sincos(theta, &sn, &cs);
    const double a = sn / theta, b = (1. - cs) / (theta * theta), c = (theta - sn) / (theta * theta * theta);
    SIM3_UNROLL
    for (int e = 0; e < 9; ++e) {
      const double id = e % 4 == 0 ? 1. : 0.;
      R[e] = (id + a * Om[e]) + b * Om2[e];
      V[e] = (id + b * Om[e]) + c * Om2[e];
    }
  }
  Pose E;
  quat_of(R, E.q);
  SIM3_UNROLL
  for (int i = 0; i < 3; ++i) E.t[i] = (V[i * 3] * dx[3] + V[i * 3 + 1] * dx[4]) + V[i * 3 + 2] * dx[5];
  normalize_rotation(E.q);
  // E * P: t = E.t + E.r * P.t; r = E.r * P.r; normalizeRotation
  double rt[3];
  rotate(E.q, P.t[0], P.t[1], P.t[2], rt);
  const double *a = E.q, *b = P.q;
  out.t[0] = E.t[0] + rt[0], out.t[1] = E.t[1] + rt[1], out.t[2] = E.t[2] + rt[2];
  const double w = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
  const double x = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
  const double y = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2];
  const double z = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0];
  out.q[0] = x, out.q[1] = y, out.q[2] = z, out.q[3] = w;
  normalize_rotation(out.q);
}

// ---- one edge ------------------------------------------------------------------------------------------------------------------------
struct EdgeEval {
  double x, y, z;   // the point in the camera
  double e0, e1;    // computeError
  double w;         // invSigma2, widened
  double chi2;      // _error . (information * _error)
};

PO_HD void edge_error(const Pose& P, const Cam& C, const float* in, EdgeEval& E) {
  double p[3];
  rotate(P.q, (double)in[0], (double)in[1], (double)in[2], p);
  E.x = p[0] + P.t[0], E.y = p[1] + P.t[1], E.z = p[2] + P.t[2];
  E.e0 = (double)in[3] - ((E.x / E.z) * C.fx + C.cx);
  E.e1 = (double)in[4] - ((E.y / E.z) * C.fy + C.cy);
  E.w = (double)in[5];
  E.chi2 = E.e0 * (E.w * E.e0 + 0. * E.e1) + E.e1 * (0. * E.e0 + E.w * E.e1);
}

// RobustKernelHuber::robustify: rho[0], rho[1]
PO_HD void huber(double e, double* rho0, double* rho1) {
  const double dsqr = kDelta * kDelta;
  if (e <= dsqr) {
    *rho0 = e, *rho1 = 1.;
  } else {
    const double sqrte = sqrt(e);
    *rho0 = 2. * sqrte * kDelta - dsqr, *rho1 = kDelta / sqrte;
  }
}

// linearizeOplus: _jacobianOplusXj, 2 x 6
PO_HD void jacobian(const EdgeEval& E, const Cam& C, double J0[6], double J1[6]) {
  const double x = E.x, y = E.y, z = E.z, z_2 = z * z;
  J0[0] = x * y / z_2 * C.fx;
  J0[1] = -(1. + (x * x / z_2)) * C.fx;
  J0[2] = y / z * C.fx;
  J0[3] = -1. / z * C.fx;
  J0[4] = 0.;
  J0[5] = x / z_2 * C.fx;
  J1[0] = (1. + y * y / z_2) * C.fy;
  J1[1] = -x * y / z_2 * C.fy;
  J1[2] = -x / z * C.fy;
  J1[3] = 0.;
  J1[4] = -1. / z * C.fy;
  J1[5] = y / z_2 * C.fy;
}

// constructQuadraticForm with the Huber kernel: the edge's terms of H (upper triangle, row-major), b and the robust chi2
template <int MUT>
PO_HD void edge_terms(const EdgeEval& E, const Cam& C, double term[kSums]) {
  double rho0, rho1, J0[6], J1[6];
  huber(E.chi2, &rho0, &rho1);
  jacobian(E, C, J0, J1);
  const double wo = rho1 * E.w;  // robustInformation: rho[1] * information, the rho[2] term dropped
  double r0 = -(E.w * E.e0), r1 = -(E.w * E.e1);
  if (MUT != kMutHuberB) r0 = r0 * rho1, r1 = r1 * rho1;
  int k = 0;
  SIM3_UNROLL
  for (int i = 0; i < 6; ++i)
    SIM3_UNROLL
    for (int j = i; j < 6; ++j) term[k++] = (J0[i] * wo) * J0[j] + (J1[i] * wo) * J1[j];
  SIM3_UNROLL
  for (int i = 0; i < 6; ++i) term[21 + i] = J0[i] * r0 + J1[i] * r1;
  term[27] = rho0;
}

// ---- the 6 x 6 solve -------------------------------------------------------------------------------------------------------------------
// (H + lambda I) x = b by an unpivoted LDL^T.  H: the 21 upper entries, row-major.  Returns whether every pivot is finite and > 0;
// x is written only then.
PO_HD bool solve6(const double H[21], double lambda, const double b[6], double x[6]) {
  // in place on the lower triangle: L[i][j] (i > j) starts as the matrix entry and ends as the factor's, d[j] likewise
  double L[6][6], d[6];
  {
    int k = 0;
    SIM3_UNROLL
    for (int i = 0; i < 6; ++i)
      SIM3_UNROLL
      for (int j = i; j < 6; ++j, ++k) {
        if (i == j) d[i] = H[k] + lambda;
        else L[j][i] = H[k];
      }
  }
  bool ok = true;
  SIM3_UNROLL
  for (int j = 0; j < 6; ++j) {
    double dj = d[j];
    SIM3_UNROLL
    for (int k = 0; k < j; ++k) dj = dj - (L[j][k] * L[j][k]) * d[k];
    d[j] = dj;
    ok = ok && dj > 0. && dj <= DBL_MAX;
    SIM3_UNROLL
    for (int i = j + 1; i < 6; ++i) {
      double v = L[i][j];
      SIM3_UNROLL
      for (int k = 0; k < j; ++k) v = v - (L[i][k] * L[j][k]) * d[k];
      L[i][j] = v / dj;
    }
  }
  if (!ok) return false;
  double y[6];
  SIM3_UNROLL
  for (int i = 0; i < 6; ++i) {
    double v = b[i];
    SIM3_UNROLL
    for (int k = 0; k < i; ++k) v = v - L[i][k] * y[k];
    y[i] = v;
  }
  SIM3_UNROLL
  for (int i = 0; i < 6; ++i) y[i] = y[i] / d[i];
  SIM3_UNROLL
  for (int i = 5; i >= 0; --i) {
    double v = y[i];
    SIM3_UNROLL
    for (int k = i + 1; k < 6; ++k) v = v - L[k][i] * x[k];
    x[i] = v;
  }
  return true;
}

// ---- one trial's two scalars -----------------------------------------------------------------------------------------------------------
// activeRobustChi2 after computeActiveErrors at pose P: lane `lane`'s share, its edges' stored chi2 rewritten on the way
PO_HD void lane_robust_chi2(const Pose& P, const Cam& C, const Edges& E, int lane, double* acc) {
  PO_NOUNROLL
  for (int i = lane; i < E.n; i += kLanes) {
    if (E.state[i] & kLevel) continue;
    EdgeEval ev;
    edge_error(P, C, E.in + 6 * i, ev);
    E.chi2[i] = ev.chi2;
    double rho0, rho1;
    huber(ev.chi2, &rho0, &rho1);
    acc[0] = acc[0] + rho0;
  }
}

// computeScale() + 1e-3: the denominator of rho = (currentChi - tempChi) / scale
template <int MUT>
PO_HD double trial_scale(const double dx[6], double lambda, const double* b) {
  double scale = 0.;
  SIM3_UNROLL
  for (int j = 0; j < 6; ++j) scale = scale + dx[j] * (lambda * dx[j] + b[j]);
  return MUT == kMutScale ? scale : scale + 1e-3;
}

// ---- the host's team -----------------------------------------------------------------------------------------------------------------
#if !defined(__HIP_DEVICE_COMPILE__)
using HostTeam = HostLaneTeam<kSums>;
#endif

// ---- the call --------------------------------------------------------------------------------------------------------------------------
// Every member of the team calls this with the same arguments.  tr may be null.
template <int MUT, class Team>
PO_HD void run(Team& T, const Edges& E, const Cam& C, const float* Tcw, Out* out, Trace* tr) {
  Pose P;
  pose_of(Tcw, P);
  const int n = E.n;
  (void)T.count([&](int lane) {
    for (int i = lane; i < n; i += kLanes) E.chi2[i] = 0., E.state[i] = 0, E.mask[i] = 0;
    return 0;
  });
  int n_lin = 0, n_trials = 0, n_active = n, n_bad = 0, rounds = 0;
  double lambda = 0.;
  PO_NOUNROLL
  for (int round = 0; round < kRounds; ++round) {
    rounds = round + 1;
    // optimize(its): nothing to do without an active edge (initializeOptimization finds no vertex)
    double ni = 2., dx[6] = {0., 0., 0., 0., 0., 0.};
    int stalled = 0;
    const int its = n_active > 0 ? its_of(round) : 0;
    bool go = true;
    PO_NOUNROLL
    for (int it = 0; it < 10; ++it) {
      if (!(go && it < its)) continue;  // compile-time bound; uniform
      // computeActiveErrors, activeRobustChi2, buildSystem
      double* const S = T.shared();
      T.template sum_shared<kSums>(
          [&](int lane, double* acc) {
            PO_NOUNROLL
            for (int i = lane; i < n; i += kLanes) {
              if (E.state[i] & kLevel) continue;
              EdgeEval ev;
              edge_error(P, C, E.in + 6 * i, ev);
              E.chi2[i] = ev.chi2;
              double term[kSums];
              edge_terms<MUT>(ev, C, term);
              SIM3_UNROLL
              for (int k = 0; k < kSums; ++k) acc[k] = acc[k] + term[k];
            }
          },
          S);
      double cur = S[27];
      const double ini = cur;
      if (it == 0 && (MUT != kMutLambdaOnce || round == 0)) {  // computeLambdaInit: tau * max |H_jj|
        double mx = 0.;
        const double dg[6] = {S[0], S[6], S[11], S[15], S[18], S[20]};
        SIM3_UNROLL
        for (int j = 0; j < 6; ++j) mx = fabs(dg[j]) < mx ? mx : fabs(dg[j]);  // std::max(fabs(h), max): a NaN entry is taken
        lambda = 1e-5 * mx;
      }
      if (it == 0) ni = 2., stalled = 0;
      const int lin = n_lin;
      if (tr && T.lead() && lin < kMaxLin) {
        TraceLin& r = tr->lin[lin];
        r.round = round, r.iteration = it;
        for (int k = 0; k < 21; ++k) r.H[k] = S[k];
        for (int k = 0; k < 6; ++k) r.b[k] = S[21 + k];
        r.chi2 = S[27];
      }
      ++n_lin;
      double rho = 0.;
      int q = 0;
      bool again = true;
      PO_NOUNROLL
      for (int trial = 0; trial < kMaxTrials; ++trial) {
        if (!again) continue;
        const Pose backup = P;
        const bool ok = solve6(S, lambda, S + 21, dx);
        Pose Q;
        oplus(dx, P, Q);
        P = Q;
        double tmp;
        T.template sum<1>([&](int lane, double* acc) { lane_robust_chi2(P, C, E, lane, acc); }, &tmp);
        if (!ok) tmp = DBL_MAX;
        const double scale = trial_scale<MUT>(dx, lambda, S + 21);
        rho = (cur - tmp) / scale;
        const bool accept = rho > 0. && fabs(tmp) <= DBL_MAX;
        if (tr && T.lead() && n_trials < kMaxTrialRecs) {
          TraceTrial& r = tr->trial[n_trials];
          r.lin = lin, r.ok = ok ? 1 : 0, r.accepted = accept ? 1 : 0, r.pad_ = 0;
          r.lambda = lambda, r.cur = cur, r.tmp = tmp, r.scale = scale;
        }
        ++n_trials;
        if (accept) {
          const double u = 2. * rho - 1.;
          double alpha = 1. - u * u * u;
          alpha = 2. / 3. < alpha ? 2. / 3. : alpha;             // std::min(alpha, _goodStepUpperScale)
          const double sf = 1. / 3. < alpha ? alpha : 1. / 3.;   // std::max(_goodStepLowerScale, alpha)
          lambda = lambda * sf;
          ni = 2.;
          cur = tmp;
        } else {
          lambda = lambda * ni;
          ni = ni * 2.;
          P = backup;
        }
        ++q;
        again = rho < 0. && q < kMaxTrials;
      }
      if (q == kMaxTrials || rho == 0.) {  // Terminate
        go = false;
        continue;
      }
      if ((ini - cur) * 1e3 < ini) ++stalled;
      else stalled = 0;
      if (stalled >= 3) go = false;
    }
    // classification.  The counts travel packed: flagged edges in the low 15 bits' worth, level-1 edges above (n <= 16384).
    const double th = (double)th_of(round);
    const int packed = T.count([&](int lane) {
      int c = 0;
      PO_NOUNROLL
      for (int i = lane; i < n; i += kLanes) {
        uint8_t st = E.state[i];
        if ((st & kFlag) && MUT != kMutNoReeval) {
          EdgeEval ev;
          edge_error(P, C, E.in + 6 * i, ev);
          E.chi2[i] = ev.chi2;
        }
        const double c2 = E.chi2[i];
        if (c2 > th) {
          st = kFlag | kLevel;
          c += 1;
        } else if (c2 <= th) {
          st = MUT == kMutNoRestore ? (uint8_t)(st & kLevel) : (uint8_t)0;
        }
        E.state[i] = st;
        E.mask[i] = (st & kFlag) ? 1 : 0;
        c += (st & kLevel) ? 1 << 15 : 0;
      }
      return c;
    });
    n_bad = packed & 0x7fff;
    n_active = n - (packed >> 15);
    if ((MUT == kMutBreakActive ? n_active : n) < 10) break;
  }
  if (T.lead()) {
    double R[9];
    matrix_of(P, out->Tcw, R);
    out->n_inliers = n - n_bad, out->rounds = rounds;
    if (tr) {
      tr->n_lin = n_lin, tr->n_trials = n_trials;
      for (int e = 0; e < 9; ++e) tr->R[e] = R[e];
      for (int e = 0; e < 3; ++e) tr->t[e] = P.t[e];
    }
  }
}

}  // namespace poseopt
}  // namespace uvo
