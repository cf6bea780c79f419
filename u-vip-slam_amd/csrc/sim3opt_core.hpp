// Optimizer::OptimizeSim3 (src/Optimizer.cc:2660-2856 of the reference, with the parts of g2o it runs: the Levenberg driver,
// EdgeSim3ProjectXYZ and EdgeInverseSim3ProjectXYZ with BaseBinaryEdge's NUMERIC Jacobian, the Huber kernel, g2o::Sim3, the dense 7 x 7
// solve) as plain C++ in double.  sim3opt.hip runs this on the device, tests/emu/sim3opt_emu.cpp on the host; the two are held to each
// other bit for bit under the rules of epnp_core.hpp's and poseopt_core.hpp's headers: IEEE + - * / sqrt and fabs only, no contraction
// (-ffp-contract=off on both sides), no library function.
//
// SUMS OVER PAIRS ARE REDUCED IN THE FIXED SHAPE OF poseopt_core.hpp: lane l of 256 adds the terms of its pairs l, l + 256, ... in
// ascending order onto 0.0, skipping removed pairs; a butterfly within the wavefront; then (w0 + w1) + (w2 + w3).  A correspondence is
// a PAIR of edges, and the order inside a pair is part of the contract: A LANE ADDS THE TERMS OF THE PAIR'S e12 (through the
// similarity) FIRST AND THOSE OF ITS e21 (through the inverse) SECOND, each onto the running lane sum.  One linearisation takes
// 28 + 7 + 1 sums (H's upper triangle row-major, b, the robust chi2), one trial takes one.
//
// The Jacobian is the central difference of BaseBinaryEdge::linearizeOplus (core/base_binary_edge.hpp:131-205): delta = 1e-9,
// column d = (1 / 2e-9) * (e(+) - e(-)) at the estimates Sim3(+-delta e_d) * estimate.  Those 14 similarities and their inverses depend
// on the estimate alone: member k < 14 of the team computes number k (dimension k / 2, sign + for even k), member 14 the unperturbed
// pair, each as 24 words "s R | t" forward and inverse, into a place all members read (Team::sims(): LDS on the device).  Every word
// is produced by one member with the operations the host build uses, so bit identity holds.  A pair then costs 30 projections per
// linearisation and keeps one edge's 2 x 7 Jacobian in registers at a time.
//
// Everything that is not a sum over pairs -- the 7 x 7 solve, exp, the product, the Levenberg decision -- is computed by every
// member from the same reduced values, so every branch of run() is uniform over the team.
//
// Departures from the reference, stated in uvo.h and DESIGN.md section 4:
//   * the fixed tree in place of serial sums;
//   * the solve is an unpivoted LDL^T (solve7), "ok" meaning every pivot is finite and > 0; Eigen's LDLT pivots and accepts
//     semi-definite matrices.  On a failed solve dx keeps its previous value (zero at the start of a round);
//   * sin, cos are sim3::sincos (NaN above 7 rad), exp is exp_ below (NaN beyond |x| = 40): such a trial is NaN and is rejected;
//   * map() multiplies by the matrix s R (one rotation matrix per similarity) where g2o evaluates s * (r * xyz) with the quaternion
//     per point: the same function, other roundings;
//   * the zeros of the information matrix are kept in chi2 (0 * inf is NaN decides a class) and dropped inside H and b.
#pragma once
#include "poseopt_core.hpp"

namespace uvo {
namespace sim3opt {

using poseopt::kLanes;
using poseopt::kMaxTrials;
constexpr int kSums = 36;            // 28 of H, 7 of b, the robust chi2
constexpr int kHalf = 18;            // sums per pass of a linearisation
constexpr int kMaxLin = 15;          // 5 + 10 linearisations at the most
constexpr int kMaxTrialRecs = 150;   // ten trials each
constexpr int kSims = 15;            // 14 perturbed similarities and the estimate
constexpr int kSimWords = 24;        // s R | t of a similarity, then of its inverse
constexpr int kPairFloats = 12;      // X1c, X2c, obs1, obs2, info1, info2
constexpr double kStep = 1e-9;                 // delta of linearizeOplus
constexpr double kScalar = 1.0 / (2 * 1e-9);   // its scalar

// seeded mutations, for the host build only (tests/emu/sim3opt_emu.cpp); the library instantiates MUT = 0
constexpr int kMutNone = 0, kMutForward21 = 1, kMutOneSided = 2, kMutAlways10 = 3, kMutReadmit = 4, kMutInfo2 = 5, kMutExp = 6,
              kMutWriteEarly = 7, kMutScale = 8, kMutNiOnce = 9;

struct Sim {
  double q[4];  // x y z w, NOT normalised: g2o::Sim3 never normalises
  double t[3];
  double s;
};

struct Cams {
  const float *K1, *K2;  // fx fy cx cy of either key frame: floats, widened where they are used (the vertex's members are doubles)
};

constexpr uint8_t kRemoved = 1;

struct Pairs {
  const float* in;  // [n][12]
  double* chi2;     // [n][2] chi2 of the stored errors of e12 and e21: those of the last evaluation, accepted or not
  uint8_t* state;   // [n] kRemoved
  uint8_t* mask;    // [n] 1 where the reference nulls vpMatches1[idx]
  int n;
};

// the layout of uvo_sim3_opt_trace (uvo.h); sim3opt.hip asserts the sizes equal
struct TraceLin {
  int32_t round, iteration;
  double H[28], b[7], chi2;
};
struct Trace {
  int32_t n_lin, n_trials;
  double q[4], t[3], s;
  TraceLin lin[kMaxLin];
  poseopt::TraceTrial trial[kMaxTrialRecs];
};

struct Out {
  double q[4], t[3], s;
  float R12[9], t12[3], scale;
  int32_t n_inliers, n_correspondences, n_bad, more_iterations, pad_;
};

// ---- exp ---------------------------------------------------------------------------------------------------------------------------
// exp(x) = 2^k exp(r), k = nearest integer to x / ln 2, r = (x - k L1) - k L2 with ln 2 = L1 + L2 in two parts.  NaN for |x| > 40 and
// for NaN.  Error bound, from the construction: |exp_(x) - exp(x)| <= 2^-51 exp(x).
//   * L1 has 32 significant bits, |k| <= 58: k L1 is exact, and x - k L1 is exact (below 1/2 in magnitude and a multiple of
//     2^-54 when k != 0; x itself when k = 0).  k L2 and the second subtraction round once each: r is off by at most 2^-55 + 2^-80,
//     |r| <= ln 2 / 2 + 2^-30 < 0.3466.
//   * Taylor to r^13: the first term left out is r^14 / 14! < 4.2e-18 < 2^-57.
//   * Horner: an error made at depth j reaches the result multiplied by r^j; what matters is y = r + r^2 p (half an ulp of a value
//     below 1/2: 2^-55, plus 3 roundings on r^2 p < 0.07: 2^-55) and 1 + y in [0.70, 1.42]: 2^-53.
//   * together below 2^-53 + 3 * 2^-55 + 2^-57 < 2^-52 absolute on exp(r) >= 0.707: 2^-51 relative with room; 2^k is a product of
//     exact powers and scales exactly (no subnormal at |x| <= 40).
// At |x| < 0.3466 (k = 0, r = x exactly) the bound is 2^-52 absolute, which is what the scale column of the Jacobian sees at +-1e-9.
constexpr double kExpLimit = 40.;
template <int MUT>
PO_HD double exp_(double x) {
  if (MUT == kMutExp) return 1. + x;
  if (!(fabs(x) <= kExpLimit)) return (x - x) / (x - x);
  const int k = (int)(x * 0x1.71547652b82fep+0 + (x < 0. ? -0.5 : 0.5));
  const double kd = (double)k;
  const double r = (x - kd * 0x1.62e42fee00000p-1) - kd * 0x1.a39ef35793c76p-33;
  double p = 1. / 6227020800.;
  p = 1. / 479001600. + r * p;
  p = 1. / 39916800. + r * p;
  p = 1. / 3628800. + r * p;
  p = 1. / 362880. + r * p;
  p = 1. / 40320. + r * p;
  p = 1. / 5040. + r * p;
  p = 1. / 720. + r * p;
  p = 1. / 120. + r * p;
  p = 1. / 24. + r * p;
  p = 1. / 6. + r * p;
  p = 0.5 + r * p;
  const double e = 1. + (r + (r * r) * p);
  // 2^k from exact products: |k| <= 58 < 64
  const int a = k < 0 ? -k : k;
  double f = k < 0 ? 0.5 : 2., two_k = 1.;
  SIM3_UNROLL
  for (int bit = 0; bit < 6; ++bit) {
    two_k = ((a >> bit) & 1) ? two_k * f : two_k;
    f = f * f;
  }
  return e * two_k;
}

// ---- g2o::Sim3 -----------------------------------------------------------------------------------------------------------------------
// Sim3(Matrix3d, Vector3d, double) from the caller's floats: Eigen's Quaternion(Matrix3), no normalisation
PO_HD void sim_of(const float* R12, const float* t12, float s12, Sim& S) {
  double R[9];
  SIM3_UNROLL
  for (int e = 0; e < 9; ++e) R[e] = (double)R12[e];
  poseopt::quat_of(R, S.q);
  S.t[0] = (double)t12[0], S.t[1] = (double)t12[1], S.t[2] = (double)t12[2];
  S.s = (double)s12;
}

// quat_of where the trace is known to be positive: its first branch
PO_HD void quat_of_positive_trace(const double R[9], double q[4]) {
  double t = sqrt((R[0] + R[4] + R[8]) + 1.);
  q[3] = 0.5 * t;
  t = 0.5 / t;
  q[0] = (R[7] - R[5]) * t, q[1] = (R[2] - R[6]) * t, q[2] = (R[3] - R[1]) * t;
}

// Sim3(update) * estimate (VertexSim3Expmap::oplusImpl; sim3.h:70-142 and :266-272).  update = (omega, upsilon, sigma).
// TINY: the caller knows that |sigma| and theta are below eps (the +-1e-9 steps of the numeric Jacobian), and only that branch is
// compiled: the same operations as the general function performs on such an update (R = I + Omega + Omega2 then has the trace
// 3 - 2 theta^2 > 0, so Quaternion(R) takes its first branch).
template <int MUT, bool TINY = false>
PO_HD void oplus(const double dx[7], const Sim& P, Sim& out) {
  const double o0 = dx[0], o1 = dx[1], o2 = dx[2], sigma = dx[6];
  const double theta = sqrt(o0 * o0 + o1 * o1 + o2 * o2);
  const double Om[9] = {0., -o2, o1, o2, 0., -o0, -o1, o0, 0.};
  double Om2[9];
  SIM3_UNROLL
  for (int i = 0; i < 3; ++i)
    SIM3_UNROLL
    for (int j = 0; j < 3; ++j) Om2[i * 3 + j] = (Om[i * 3] * Om[j] + Om[i * 3 + 1] * Om[3 + j]) + Om[i * 3 + 2] * Om[6 + j];
  const double s = exp_<MUT>(sigma);
  const double eps = 0.00001;
  const bool small_sigma = TINY || fabs(sigma) < eps, small_theta = TINY || theta < eps;
  double A, B, C, ra = 1., rb = 1.;  // R = I + ra Omega + rb Omega2
  if (small_theta) {
    if (small_sigma) {
      A = 1. / 2., B = 1. / 6., C = 1.;
    } else {
      const double sigma2 = sigma * sigma;
      C = (s - 1.) / sigma;
      A = ((sigma - 1.) * s + 1.) / sigma2;
      B = ((0.5 * sigma2 - sigma + 1.) * s) / (sigma2 * sigma);
    }
  } else {
    double sn, cs;
    sim3::sincos(theta, &sn, &cs);
    const double theta2 = theta * theta;
    ra = sn / theta, rb = (1. - cs) / (theta * theta);
    if (small_sigma) {
      C = 1.;
      A = (1. - cs) / theta2;
      B = (theta - sn) / (theta2 * theta);
    } else {
      C = (s - 1.) / sigma;
      const double a = s * sn, b = s * cs, sigma2 = sigma * sigma, c = theta2 + sigma2;
      A = (a * sigma + (1. - b) * theta) / (theta * c);
      B = (C - ((b - 1.) * sigma + a * theta) / c) * 1. / theta2;
    }
  }
  double R[9], W[9];
  SIM3_UNROLL
  for (int e = 0; e < 9; ++e) {
    const double id = e % 4 == 0 ? 1. : 0.;
    R[e] = small_theta ? (id + Om[e]) + Om2[e] : (id + ra * Om[e]) + rb * Om2[e];
    W[e] = (A * Om[e] + B * Om2[e]) + C * id;
  }
  Sim E;
  if (TINY) quat_of_positive_trace(R, E.q);
  else poseopt::quat_of(R, E.q);
  SIM3_UNROLL
  for (int i = 0; i < 3; ++i) E.t[i] = (W[i * 3] * dx[3] + W[i * 3 + 1] * dx[4]) + W[i * 3 + 2] * dx[5];
  // E * P: r = E.r * P.r (not normalised); t = s (E.r * P.t) + E.t; s = s * P.s
  double rt[3];
  poseopt::rotate(E.q, P.t[0], P.t[1], P.t[2], rt);
  const double *a = E.q, *b = P.q;
  out.t[0] = s * rt[0] + E.t[0], out.t[1] = s * rt[1] + E.t[1], out.t[2] = s * rt[2] + E.t[2];
  const double w = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
  const double x = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
  const double y = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2];
  const double z = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0];
  out.q[0] = x, out.q[1] = y, out.q[2] = z, out.q[3] = w;
  out.s = s * P.s;
}

// the 24 words of a similarity: s R | t of map(), then of inverse() = (r*, r* ((-1 / s) t), 1 / s)
PO_HD void mats_of(const Sim& S, double* M) {
  double R[9];
  poseopt::rotation_of(S.q, R);
  SIM3_UNROLL
  for (int e = 0; e < 9; ++e) M[e] = S.s * R[e];
  M[9] = S.t[0], M[10] = S.t[1], M[11] = S.t[2];
  const double qc[4] = {-S.q[0], -S.q[1], -S.q[2], S.q[3]};
  const double si = 1. / S.s, ms = -1. / S.s;
  double ti[3];
  poseopt::rotate(qc, ms * S.t[0], ms * S.t[1], ms * S.t[2], ti);
  poseopt::rotation_of(qc, R);
  SIM3_UNROLL
  for (int e = 0; e < 9; ++e) M[12 + e] = si * R[e];
  M[21] = ti[0], M[22] = ti[1], M[23] = ti[2];
}

// member k's words of a linearisation: k < 14 the estimate perturbed along dimension k / 2 (even k: +delta), k = 14 the estimate
template <int MUT>
PO_HD void build_sim(const Sim& S, int k, double* M) {
  Sim Q = S;
  if (k < 14) {
    double dx[7];
    SIM3_UNROLL
    for (int j = 0; j < 7; ++j) dx[j] = j == (k >> 1) ? ((k & 1) ? -kStep : kStep) : 0.;
    oplus<MUT, true>(dx, S, Q);
  }
  mats_of(Q, M);
}

// ---- one edge ------------------------------------------------------------------------------------------------------------------------
// what one edge of a pair reads of its 12 floats, widened: SECOND = false e12 (X2c, obs1, info1), true e21 (X1c, obs2, info2)
struct Edge {
  double X[3], o[2], w;
};
template <int MUT, bool SECOND>
PO_HD void load_edge(const float* in, Edge& P) {
  SIM3_UNROLL
  for (int e = 0; e < 3; ++e) P.X[e] = (double)in[(SECOND ? 0 : 3) + e];
  P.o[0] = (double)in[SECOND ? 8 : 6], P.o[1] = (double)in[SECOND ? 9 : 7];
  P.w = (double)in[SECOND ? 11 : 10];
  if (MUT == kMutInfo2 && SECOND) P.w = 1. / P.w;
}

// The 12 floats of a pair as the host gathers them: P3D1c = R1w * P3D1w + t1w and P3D2c = R2w * P3D2w + t2w are the float products of the
// reference's cv::Mat arithmetic (sim3::transform), the rest is copied.
inline void pack_pair(const float* R1w, const float* t1w, const float* R2w, const float* t2w, const float* x1w, const float* x2w, const float* obs1,
                      const float* obs2, float info1, float info2, float* e) {
  sim3::transform(R1w, 3, t1w[0], t1w[1], t1w[2], x1w, e);
  sim3::transform(R2w, 3, t2w[0], t2w[1], t2w[2], x2w, e + 3);
  e[6] = obs1[0], e[7] = obs1[1], e[8] = obs2[0], e[9] = obs2[1], e[10] = info1, e[11] = info2;
}

// computeError: obs - cam_map(project(map(X))), M the 12 words s R | t
PO_HD void edge_error(const double* M, const double* X, const float* K, const double* obs, double* e0, double* e1) {
  const double fx = (double)K[0], fy = (double)K[1], cx = (double)K[2], cy = (double)K[3];
  const double x = ((M[0] * X[0] + M[1] * X[1]) + M[2] * X[2]) + M[9];
  const double y = ((M[3] * X[0] + M[4] * X[1]) + M[5] * X[2]) + M[10];
  const double z = ((M[6] * X[0] + M[7] * X[1]) + M[8] * X[2]) + M[11];
  *e0 = obs[0] - ((x / z) * fx + cx);
  *e1 = obs[1] - ((y / z) * fy + cy);
}
PO_HD double chi2_of(double e0, double e1, double w) { return e0 * (w * e0 + 0. * e1) + e1 * (0. * e0 + w * e1); }

// RobustKernelHuber::robustify with delta = (double)(float)sqrt(th2)
PO_HD void huber(double e, double delta, double* rho0, double* rho1) {
  const double dsqr = delta * delta;
  if (e <= dsqr) {
    *rho0 = e, *rho1 = 1.;
  } else {
    const double sqrte = sqrt(e);
    *rho0 = 2. * sqrte * delta - dsqr, *rho1 = delta / sqrte;
  }
}
// const float deltaHuber = sqrt(th2) on a float: the float root.  The double root rounded to float is the same number (53 >= 2 * 24 + 2
// bits make the second rounding harmless), so it does not matter which overload the reference's translation unit picks.
PO_HD double delta_of(float th2) { return (double)(float)sqrt((double)th2); }

// linearizeOplus + constructQuadraticForm of one edge: its terms added onto the lane's sums; returns the chi2 of its error.
// sims: the team's 15 x 24 words; off: 0 for the forward map, 12 for the inverse.
// The 36 sums are taken in TWO PASSES of 18 (kHalf) so that a lane's sums and the Jacobian fit its registers: PART 0 adds rows 0..2 of
// H (sums 0..17), PART 1 rows 3..6, b and the robust chi2 (sums 18..35).  Both passes compute the same errors and the same Jacobian.
template <int MUT, int PART>
PO_HD double edge_terms(const double* sims, int off, const double* X, const float* K, const double* obs, double w,
                        double delta, double* acc) {
  double e0, e1;
  edge_error(sims + 14 * kSimWords + off, X, K, obs, &e0, &e1);
  const double chi2 = chi2_of(e0, e1, w);
  double rho0, rho1, J0[7], J1[7];
  huber(chi2, delta, &rho0, &rho1);
  PO_NOUNROLL
  for (int d = 0; d < 7; ++d) {
    double p0, p1, m0, m1;
    edge_error(sims + (2 * d) * kSimWords + off, X, K, obs, &p0, &p1);
    edge_error(sims + (2 * d + 1) * kSimWords + off, X, K, obs, &m0, &m1);
    if (MUT == kMutOneSided) m0 = e0, m1 = e1;
    J0[d] = kScalar * (p0 - m0), J1[d] = kScalar * (p1 - m1);
  }
  const double wo = rho1 * w;  // robustInformation: rho[1] * information
  const double r0 = -(w * e0) * rho1, r1 = -(w * e1) * rho1;
  int k = 0;
  SIM3_UNROLL
  for (int i = PART == 0 ? 0 : 3; i < (PART == 0 ? 3 : 7); ++i)
    SIM3_UNROLL
    for (int j = i; j < 7; ++j, ++k) acc[k] = acc[k] + ((J0[i] * wo) * J0[j] + (J1[i] * wo) * J1[j]);
  if (PART == 1) {
    SIM3_UNROLL
    for (int i = 0; i < 7; ++i) acc[10 + i] = acc[10 + i] + (J0[i] * r0 + J1[i] * r1);
    acc[17] = acc[17] + rho0;
  }
  return chi2;
}

// a lane's share of one linearisation: e12 first, e21 second, the stored chi2 rewritten
template <int MUT, int PART>
PO_HD void lane_linearise(const double* sims, const Cams& C, const Pairs& E, double delta, int lane, double* acc) {
  PO_NOUNROLL
  for (int i = lane; i < E.n; i += kLanes) {
    if (E.state[i] & kRemoved) continue;
    Edge P;
    load_edge<MUT, false>(E.in + kPairFloats * i, P);
    E.chi2[2 * i] = edge_terms<MUT, PART>(sims, 0, P.X, C.K1, P.o, P.w, delta, acc);
    load_edge<MUT, true>(E.in + kPairFloats * i, P);
    E.chi2[2 * i + 1] = edge_terms<MUT, PART>(sims, MUT == kMutForward21 ? 0 : 12, P.X, C.K2, P.o, P.w, delta, acc);
  }
}

// activeRobustChi2 after computeActiveErrors at the similarity whose 24 words are M: a lane's share, e12 then e21
template <int MUT>
PO_HD void lane_robust_chi2(const double* M, const Cams& C, const Pairs& E, double delta, int lane, double* acc) {
  PO_NOUNROLL
  for (int i = lane; i < E.n; i += kLanes) {
    if (E.state[i] & kRemoved) continue;
    Edge P;
    load_edge<MUT, false>(E.in + kPairFloats * i, P);
    double e0, e1, rho0, rho1;
    edge_error(M, P.X, C.K1, P.o, &e0, &e1);
    const double c12 = chi2_of(e0, e1, P.w);
    E.chi2[2 * i] = c12;
    huber(c12, delta, &rho0, &rho1);
    acc[0] = acc[0] + rho0;
    load_edge<MUT, true>(E.in + kPairFloats * i, P);
    edge_error(M + (MUT == kMutForward21 ? 0 : 12), P.X, C.K2, P.o, &e0, &e1);
    const double c21 = chi2_of(e0, e1, P.w);
    E.chi2[2 * i + 1] = c21;
    huber(c21, delta, &rho0, &rho1);
    acc[0] = acc[0] + rho0;
  }
}

// ---- the 7 x 7 solve -------------------------------------------------------------------------------------------------------------------
// (H + lambda I) x = b by an unpivoted LDL^T: solve6 at 7.  H: the 28 upper entries, row-major.  Returns whether every pivot is finite
// and > 0; x is written only then.
PO_HD bool solve7(const double H[28], double lambda, const double b[7], double x[7]) {
  double L[7][7], d[7];
  {
    int k = 0;
    SIM3_UNROLL
    for (int i = 0; i < 7; ++i)
      SIM3_UNROLL
      for (int j = i; j < 7; ++j, ++k) {
        if (i == j) d[i] = H[k] + lambda;
        else L[j][i] = H[k];
      }
  }
  bool ok = true;
  SIM3_UNROLL
  for (int j = 0; j < 7; ++j) {
    double dj = d[j];
    SIM3_UNROLL
    for (int k = 0; k < j; ++k) dj = dj - (L[j][k] * L[j][k]) * d[k];
    d[j] = dj;
    ok = ok && dj > 0. && dj <= DBL_MAX;
    SIM3_UNROLL
    for (int i = j + 1; i < 7; ++i) {
      double v = L[i][j];
      SIM3_UNROLL
      for (int k = 0; k < j; ++k) v = v - (L[i][k] * L[j][k]) * d[k];
      L[i][j] = v / dj;
    }
  }
  if (!ok) return false;
  double y[7];
  SIM3_UNROLL
  for (int i = 0; i < 7; ++i) {
    double v = b[i];
    SIM3_UNROLL
    for (int k = 0; k < i; ++k) v = v - L[i][k] * y[k];
    y[i] = v;
  }
  SIM3_UNROLL
  for (int i = 0; i < 7; ++i) y[i] = y[i] / d[i];
  SIM3_UNROLL
  for (int i = 6; i >= 0; --i) {
    double v = y[i];
    SIM3_UNROLL
    for (int k = i + 1; k < 7; ++k) v = v - L[k][i] * x[k];
    x[i] = v;
  }
  return true;
}

// computeScale() + 1e-3
template <int MUT>
PO_HD double trial_scale(const double dx[7], double lambda, const double* b) {
  double scale = 0.;
  SIM3_UNROLL
  for (int j = 0; j < 7; ++j) scale = scale + dx[j] * (lambda * dx[j] + b[j]);
  return MUT == kMutScale ? scale : scale + 1e-3;
}

// ---- the host's team -----------------------------------------------------------------------------------------------------------------
// lane_team.hpp's walk of the reduction shape, with this core's 36 shared words and the similarities' 360
#if !defined(__HIP_DEVICE_COMPILE__)
struct HostTeam : HostLaneTeam<kSums> {
  double simw[kSims * kSimWords];
  double uni(double v) const { return v; }
  double* sims() { return simw; }
  template <class F>
  void each(F f) {
    for (int l = 0; l < kLanes; ++l) f(l);
  }
};
#endif

// Values every member holds alike may be said to be so (Team::uni: on the device a move to the scalar register file, which spares a
// vector register pair per value over the whole call; on the host nothing).  The bits do not change.
template <class Team>
PO_HD void uni_sim(const Team& T, Sim& S) {
  SIM3_UNROLL
  for (int e = 0; e < 4; ++e) S.q[e] = T.uni(S.q[e]);
  SIM3_UNROLL
  for (int e = 0; e < 3; ++e) S.t[e] = T.uni(S.t[e]);
  S.s = T.uni(S.s);
}

// the estimate as the result and the trace carry it
PO_HD void write_estimate(const Sim& F, Out* out, Trace* tr) {
  double R[9];
  poseopt::rotation_of(F.q, R);
  for (int e = 0; e < 4; ++e) out->q[e] = F.q[e];
  for (int e = 0; e < 3; ++e) out->t[e] = F.t[e], out->t12[e] = (float)F.t[e];
  for (int e = 0; e < 9; ++e) out->R12[e] = (float)R[e];
  out->s = F.s, out->scale = (float)F.s;
  if (tr) {
    for (int e = 0; e < 4; ++e) tr->q[e] = F.q[e];
    for (int e = 0; e < 3; ++e) tr->t[e] = F.t[e];
    tr->s = F.s;
  }
}

// ---- the call --------------------------------------------------------------------------------------------------------------------------
// Every member of the team calls this with the same arguments.  tr may be null.
template <int MUT, class Team>
PO_HD void run(Team& T, const Pairs& E, const Cams& C, const float* R12, const float* t12, float s12, float th2f, Out* out, Trace* tr) {
  Sim S;
  sim_of(R12, t12, s12, S);
  if (T.lead()) write_estimate(S, out, tr);  // the input's round trip: the answer of the early return
  uni_sim(T, S);
  const int n = E.n;
  const double delta = T.uni(delta_of(th2f)), th2 = T.uni((double)th2f);
  (void)T.count([&](int lane) {
    for (int i = lane; i < n; i += kLanes) E.chi2[2 * i] = 0., E.chi2[2 * i + 1] = 0., E.state[i] = 0, E.mask[i] = 0;
    return 0;
  });
  int n_lin = 0, n_trials = 0, n_active = n, n_bad = 0, n_in = 0, more = 0;
  bool early = false;
  double lambda = 0.;
  PO_NOUNROLL
  for (int round = 0; round < 2; ++round) {
    // optimize(its): nothing to do without an active edge (initializeOptimization finds no vertex)
    double ni = 2., dx[7] = {0., 0., 0., 0., 0., 0., 0.};
    int stalled = 0;
    const int its = n_active > 0 ? (round == 0 ? 5 : more) : 0;
    bool go = true;
    PO_NOUNROLL
    for (int it = 0; it < 10; ++it) {
      if (!(go && it < its)) continue;  // compile-time bound; uniform
      double* const W = T.sims();
      T.each([&](int lane) {
        if (lane < kSims) build_sim<MUT>(S, lane, W + lane * kSimWords);
      });
      double* const Sm = T.shared();
      T.template sum_shared<kHalf>([&](int lane, double* acc) { lane_linearise<MUT, 0>(W, C, E, delta, lane, acc); }, Sm);
      T.template sum_shared<kHalf>([&](int lane, double* acc) { lane_linearise<MUT, 1>(W, C, E, delta, lane, acc); }, Sm + kHalf);
      double cur = Sm[35];
      const double ini = cur;
      if (it == 0) {  // computeLambdaInit: tau * max |H_jj|
        double mx = 0.;
        const double dg[7] = {Sm[0], Sm[7], Sm[13], Sm[18], Sm[22], Sm[25], Sm[27]};
        SIM3_UNROLL
        for (int j = 0; j < 7; ++j) mx = fabs(dg[j]) < mx ? mx : fabs(dg[j]);
        lambda = T.uni(1e-5 * mx);
        ni = 2., stalled = 0;
      }
      const int lin = n_lin;
      if (tr && T.lead() && lin < kMaxLin) {
        TraceLin& r = tr->lin[lin];
        r.round = round, r.iteration = it;
        for (int k = 0; k < 28; ++k) r.H[k] = Sm[k];
        for (int k = 0; k < 7; ++k) r.b[k] = Sm[28 + k];
        r.chi2 = Sm[35];
      }
      ++n_lin;
      double rho = 0.;
      int q = 0;
      bool again = true;
      PO_NOUNROLL
      for (int trial = 0; trial < kMaxTrials; ++trial) {
        if (!again) continue;
        const Sim backup = S;
        const bool ok = solve7(Sm, lambda, Sm + 28, dx);
        SIM3_UNROLL
        for (int j = 0; j < 7; ++j) dx[j] = T.uni(dx[j]);
        Sim Q;
        oplus<MUT>(dx, S, Q);
        S = Q;
        double M[kSimWords], tmp;
        mats_of(S, M);
        SIM3_UNROLL
        for (int e = 0; e < kSimWords; ++e) M[e] = T.uni(M[e]);
        T.template sum<1>([&](int lane, double* acc) { lane_robust_chi2<MUT>(M, C, E, delta, lane, acc); }, &tmp);
        if (!ok) tmp = DBL_MAX;
        const double scale = trial_scale<MUT>(dx, lambda, Sm + 28);
        rho = (cur - tmp) / scale;
        const bool accept = rho > 0. && fabs(tmp) <= DBL_MAX;
        if (tr && T.lead() && n_trials < kMaxTrialRecs) {
          poseopt::TraceTrial& r = tr->trial[n_trials];
          r.lin = lin, r.ok = ok ? 1 : 0, r.accepted = accept ? 1 : 0, r.pad_ = 0;
          r.lambda = lambda, r.cur = cur, r.tmp = tmp, r.scale = scale;
        }
        ++n_trials;
        if (accept) {
          const double u = 2. * rho - 1.;
          double alpha = 1. - u * u * u;
          alpha = 2. / 3. < alpha ? 2. / 3. : alpha;
          const double sf = 1. / 3. < alpha ? alpha : 1. / 3.;
          lambda = lambda * sf;
          ni = 2.;
          cur = tmp;
        } else {
          lambda = lambda * ni;
          ni = MUT == kMutNiOnce ? ni : ni * 2.;
          S = backup;
        }
        uni_sim(T, S);
        lambda = T.uni(lambda), ni = T.uni(ni), cur = T.uni(cur), rho = T.uni(rho);
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
    // the inlier check on the stored errors; a NaN chi2 satisfies neither comparison: the pair stays and counts as an inlier
    const int bad = T.count([&](int lane) {
      int c = 0;
      PO_NOUNROLL
      for (int i = lane; i < n; i += kLanes) {
        if (E.state[i] & kRemoved) continue;
        if (E.chi2[2 * i] > th2 || E.chi2[2 * i + 1] > th2) {
          E.mask[i] = 1;
          if (round == 0 && MUT != kMutReadmit) E.state[i] = kRemoved;  // removeEdge: for good
          c += 1;
        }
      }
      return c;
    });
    if (round == 0) {
      n_bad = bad;
      n_active = n - bad;
      more = (bad > 0 || MUT == kMutAlways10) ? 10 : 5;
      if (n - bad < 10) {  // return 0 without writing g2oS12
        early = true;
        more = 0;
        break;
      }
    } else {
      n_in = n_active - bad;
    }
  }
  if (T.lead()) {
    if (!early || MUT == kMutWriteEarly) write_estimate(S, out, tr);  // else what was written at the start stands
    out->n_inliers = early ? 0 : n_in, out->n_correspondences = n, out->n_bad = n_bad, out->more_iterations = more, out->pad_ = 0;
    if (tr) tr->n_lin = n_lin, tr->n_trials = n_trials;
  }
}

}  // namespace sim3opt
}  // namespace uvo
