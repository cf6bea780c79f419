// The two visual-inertial overloads of Optimizer::PoseOptimization of the reference -- (FrameKTL*, KeyFrame*, IMUPreintegrator, ...)
// src/Optimizer.cc:779-1103, the KEY-FRAME FORM: 15 unknowns, the last key frame fixed; and (FrameKTL*, FrameKTL*, IMUPreintegrator, ...)
// :319-777, the FRAME FORM: 30 unknowns, the last frame free and tied by a prior -- with the parts of src/IMU/g2otypes.{h,cpp},
// NavState.cpp, so3.cpp and the vendored g2o they run, as plain C++ in double.  navopt.hip runs this on the device,
// tests/emu/navopt_emu.cpp on the host; the two are held to each other bit for bit under the rules of poseopt_core.hpp's header: IEEE
// + - * / sqrt and fabs only, no contraction, no library function, sums over edges reduced in lane_team.hpp's one shape.
//
// What is new against poseopt_core.hpp:
//   * THE STATE LIVES IN MEMORY ALL MEMBERS READ (Work: LDS on the device), not in every lane's registers: two NavStates, their
//     backups, H (30 x 30), the factor, b, the step, and the few SINGLE EDGES (prior, IMU, bias, depth) as 31 stacked rows of a dense
//     Jacobian J[31][30].  Work that is not a sum over reprojection edges is handed out by Team::each(count, f): f(0..count-1), the
//     device's lanes taking one index each (then one barrier), the host's thread all in turn.  Every f(i) writes words no other f(k)
//     of the same each reads or writes, and every written word's sequence of operations is fixed by its indices alone, so who runs
//     which index cannot show in the result.
//   * One linearisation is: the reprojection edges of the current frame reduced to poseopt's 21 + 6 + 1 sums, those of the last frame
//     (frame form) to a second set in a second reduction; the four single edges evaluated by each(4); WJ = (rho1 Omega) J and
//     We = (rho1 Omega) e row by row; then for a <= b
//         H[a][b] = (the reduced sum, where a and b are P or Phi of one frame, else 0) + sum over the active rows r ASCENDING of J[r][a] * WJ[r][b]
//         b[a]    = (the reduced sum) - sum over the active rows r ascending of J[r][a] * We[r]
//     and chi2 = (sum of the current frame + sum of the last frame) + rho0 of prior, IMU, bias, depth in that order.
//   * The solve is a dense unpivoted LDL^T of 15 or 30 unknowns, RIGHT-LOOKING: at column j every entry below the diagonal is divided
//     by the pivot, then every entry (i, k), j < k <= i, loses (L[i][j] * L[k][j]) * d[j].  "ok": every pivot finite and > 0.
//
// Hessian order (g2o orders by vertex id): frame PVR 0..8 (dP, dV, dPhi), frame bias 9..14 (dbg, dba); frame form: last PVR 15..23,
// last bias 24..29.
//
// Departures from the reference, stated in uvo.h and DESIGN.md section 4:
//   * Cholmod's ordered supernodal factorisation is the LDL^T above; on a failed solve dx keeps its previous value.
//   * CovPVPhi.inverse() (Eigen: partial-pivot LU), computeMarginals and the inverses behind mMargCovInv are the same LDL^T, column by
//     column of the identity.
//   * sin, cos are sim3::sincos, atan is built on sim3::atan2_pos: atan(n / w) = +-atan2_pos(n, |w|), the sign that of w.
//   * SO3's copy constructor normalises its quaternion on every copy; here a quaternion is normalised where it is made (exp, a
//     product, inverse(), a rotation matrix read) and once when the input state is read.
//   * structural zeros of the single edges' Jacobians are multiplied like any entry (0 * inf is NaN in H where g2o never formed the
//     product): a non-finite term ends in a failed solve either way.
//   * UpdatePoseFromNS multiplies CV_32F matrices; here Rwb, Pwb, Rbc, Pbc are rounded to float as there, the products run in double
//     and are rounded to float once.
//   * two defects of the reference are not reproduced: see marginals() and Problem::depth_info.
#pragma once
#include "poseopt_core.hpp"

#define NV_HD PO_HD

namespace uvo {
namespace navopt {

constexpr int kLanes = kTeamLanes;
constexpr int kRounds = 4, kIts = 10, kMaxTrials = 10;
constexpr int kSums = 28;                    // per frame: 21 of H, 6 of b, the robust chi2
constexpr int kND = 30, kTri = kND * (kND + 1) / 2;
constexpr int kRows = 31;                    // prior 0..14, IMU 15..23, bias 24..29, depth 30
constexpr int kMaxLin = 40, kMaxTrialRecs = 400;
constexpr int kKeyFrame = 0, kFrame = 1;
constexpr int kPrior = 0, kImu = 1, kBias = 2, kDepth = 3;   // the single edges, in the order their rho0 is added

// seeded mutations, for the host build only (tests/emu/navopt_emu.cpp); the library instantiates MUT = 0
constexpr int kMutNone = 0, kMutNoReset = 1, kMutBreakActive = 2, kMutImuNoKernel = 3, kMutDepthSwap = 4, kMutDepthHalf = 5, kMutMargFresh = 6,
              kMutMargSwap = 7, kMutOrder = 8, kMutHuberB = 9, kMutJrInv = 10;

// (float)sqrt(x) widened, as `const float thHuber... = sqrt(x); rk->setDelta(...)` leaves them
constexpr double kDeltaPrior = (double)0x1.61e714p+2f;   // 30.5779
constexpr double kDeltaImu = (double)0x1.29e632p+2f;     // 21.666
constexpr double kDeltaBias = (double)0x1.066a66p+2f;    // 16.812
constexpr double kDeltaDepth = (double)0x1.066a66p+2f;   // 16.812
constexpr double kDeltaMono = (double)0x1.394ca8p+1f;    // 5.991
constexpr float kChi2Mono = 5.991f;                      // const float chi2Mono[4], every round

struct State {
  double P[3], V[3], q[4], bg[3], ba[3], dbg[3], dba[3];  // q: x y z w
};
constexpr int kStateWords = 22;

// one problem, as the host writes it and every member reads it
struct Problem {
  int32_t form, has_depth, compute_marg, n, n_last, off;  // off: index of its first edge among the call's (the last frame's follow)
  int32_t pad_[2];
  State cur, last, prior;   // prior: mNavStatePrior of the last frame (frame form)
  double dT, dP[3], dV[3], dR[9], JPg[9], JPa[9], JVg[9], JVa[9], JRg[9], cov[81];
  double gw[3], Rbc[9], Pbc[3], fx, fy, cx, cy, gyr_rw2, acc_rw2;
  double prior_info[225];   // mMargCovInv of the last frame (frame form)
  double depth_meas, shi, depth_info;  // depth_info: the caller's scalar (the reference's own cannot be pinned: DESIGN.md section 4)
};

struct Out {
  State ns;
  float Tcw[16];
  int32_t n_inliers, rounds, marg_ok, pad_;
  double marg_cov[225], marg_cov_inv[225];
};

struct TraceLin {
  int32_t round, iteration;
  double H[kTri], b[kND], chi2;  // H: the upper triangle of the nd x nd matrix, row-major, packed; zero beyond
};
using TraceTrial = poseopt::TraceTrial;
struct Trace {
  int32_t n_lin, n_trials;
  TraceLin lin[kMaxLin];
  TraceTrial trial[kMaxTrialRecs];
};

constexpr uint8_t kLevel = 1, kFlag = 2;
struct Edges {
  const float* in;   // [n + n_last][6]: the point, the observation, invSigma2; the current frame's first
  double* chi2;      // [n + n_last]
  uint8_t* state;    // [n + n_last]
  uint8_t* mask;     // [n + n_last]
};

// what all members read and each() writes: LDS on the device
struct Work {
  double H[kND * kND];    // the last linearisation, upper triangle valid
  double A[kND * kND];    // the factorisation's work: lower triangle
  double J[kRows * kND], WJ[kRows * kND];
  double X[kND * 15];     // right-hand sides of the inverses
  double e[kRows], We[kRows];
  double b[kND], dx[kND], y[kND];
  double oimu[81];        // inverse of CovPVPhi
  double M15[225];        // marginals: the 15 x 15 block of inv(H)
  double sing[3][4];      // chi2, rho0, rho1 of the single edges
  State est[2], backup[2];  // 0 the current frame, 1 the last
  double cam[2][12];      // per frame: Rcb Rwb^T, Pwb
  double camc[3];         // Rcb Pbc
};

// ---- small matrix helpers, Eigen's order: a row times a column is ((a0 b0 + a1 b1) + a2 b2) --------------------------------------------
NV_HD void mat3_mul(const double* A, const double* B, double* C) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) C[i * 3 + j] = (A[i * 3] * B[j] + A[i * 3 + 1] * B[3 + j]) + A[i * 3 + 2] * B[6 + j];
}
NV_HD void mat3_vec(const double* A, const double* v, double* o) {
  for (int i = 0; i < 3; ++i) o[i] = (A[i * 3] * v[0] + A[i * 3 + 1] * v[1]) + A[i * 3 + 2] * v[2];
}
NV_HD void mat3_t(const double* A, double* T) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) T[i * 3 + j] = A[j * 3 + i];
}
NV_HD void hat(const double* v, double* O) {
  O[0] = 0., O[1] = -v[2], O[2] = v[1], O[3] = v[2], O[4] = 0., O[5] = -v[0], O[6] = -v[1], O[7] = v[0], O[8] = 0.;
}

// ---- Sophus::SO3 (src/IMU/so3.cpp) as a unit quaternion x y z w ---------------------------------------------------------------------------
NV_HD void q_normalize(double* q) {  // Eigen's normalize(): coeffs / norm, no sign rule
  const double nrm = sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
  q[0] = q[0] / nrm, q[1] = q[1] / nrm, q[2] = q[2] / nrm, q[3] = q[3] / nrm;
}
// operator*: the quaternion product, normalised
NV_HD void q_mul(const double* a, const double* b, double* o) {
  const double w = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
  const double x = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
  const double y = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2];
  const double z = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0];
  o[0] = x, o[1] = y, o[2] = z, o[3] = w;
  q_normalize(o);
}
// inverse(): SO3(conjugate), normalised
NV_HD void q_inv(const double* q, double* o) {
  o[0] = -q[0], o[1] = -q[1], o[2] = -q[2], o[3] = q[3];
  q_normalize(o);
}
// SO3(Matrix3d): Eigen's Quaternion(Matrix3), normalised
NV_HD void q_of_matrix(const double* R, double* q) {
  poseopt::quat_of(R, q);
  q_normalize(q);
}
// expAndTheta :256-280
NV_HD void so3_exp(const double* om, double* q) {
  const double theta = sqrt((om[0] * om[0] + om[1] * om[1]) + om[2] * om[2]);
  const double half = 0.5 * theta;
  double sn, cs;
  sim3::sincos(half, &sn, &cs);
  double imag;
  if (theta < 1e-10) {
    const double sq = theta * theta, po4 = sq * sq;
    imag = (0.5 - 0.0208333 * sq) + 0.000260417 * po4;
  } else {
    imag = sn / theta;
  }
  q[0] = imag * om[0], q[1] = imag * om[1], q[2] = imag * om[2], q[3] = cs;
  q_normalize(q);
}
// logAndTheta :205-247.  The fabs(w) < SMALL_EPS branch of the reference is overwritten by the line after it: 2 atan(n / w) / n holds
// whenever n >= SMALL_EPS.
NV_HD void so3_log(const double* q, double* o) {
  const double n = sqrt((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]);
  const double w = q[3];
  double f;
  if (n < 1e-10) {
    f = 2. / w - 2. * (n * n) / (w * (w * w));
  } else {
    const double at = sim3::atan2_pos(n, fabs(w));
    f = 2. * (w < 0. ? -at : at) / n;
  }
  o[0] = f * q[0], o[1] = f * q[1], o[2] = f * q[2];
}
// JacobianR :32-49, JacobianRInv :50-69
NV_HD void so3_jr(const double* w, double* Jr) {
  const double theta = sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);
  for (int e = 0; e < 9; ++e) Jr[e] = e % 4 == 0 ? 1. : 0.;
  if (theta < 0.00001) return;
  const double k[3] = {w[0] / theta, w[1] / theta, w[2] / theta};
  double K[9], K2[9], sn, cs;
  hat(k, K);
  mat3_mul(K, K, K2);
  sim3::sincos(theta, &sn, &cs);
  const double a = (1. - cs) / theta, c = 1. - sn / theta;
  for (int e = 0; e < 9; ++e) Jr[e] = (Jr[e] - a * K[e]) + c * K2[e];
}
template <int MUT>
NV_HD void so3_jrinv(const double* w, double* Ji) {
  const double theta = sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);
  for (int e = 0; e < 9; ++e) Ji[e] = e % 4 == 0 ? 1. : 0.;
  if (theta < 0.00001) return;
  const double k[3] = {w[0] / theta, w[1] / theta, w[2] / theta};
  double K[9], K2[9], W[9], sn, cs;
  hat(k, K);
  hat(w, W);
  mat3_mul(K, K, K2);
  sim3::sincos(theta, &sn, &cs);
  const double c = 1.0 - (1.0 + cs) * theta / (2.0 * sn);
  const double half = MUT == kMutJrInv ? -0.5 : 0.5;
  for (int e = 0; e < 9; ++e) Ji[e] = (Ji[e] + half * W[e]) + c * K2[e];
}

// RobustKernelHuber::robustify, or no kernel
NV_HD void robustify(double e, double delta, bool robust, double* rho0, double* rho1) {
  const double dsqr = delta * delta;
  if (!robust || e <= dsqr) {
    *rho0 = e, *rho1 = 1.;
  } else {
    const double sqrte = sqrt(e);
    *rho0 = 2. * sqrte * delta - dsqr, *rho1 = delta / sqrte;
  }
}

// ---- the Hessian's columns -------------------------------------------------------------------------------------------------------------
template <int MUT>
NV_HD int col_pvr(int frame) { return MUT == kMutOrder ? 15 * frame + 6 : 15 * frame; }
template <int MUT>
NV_HD int col_bias(int frame) { return MUT == kMutOrder ? 15 * frame : 15 * frame + 9; }

// ---- EdgeNavStatePVRPointXYZOnlyPose g2otypes.h:283-358, g2otypes.cpp:451-502 ------------------------------------------------------------
// cam: Rcb Rwb^T (9), Pwb (3); camc: Rcb Pbc
NV_HD void frame_camera(const State& s, const double* Rbc, double* cam) {
  double Rwb[9], Rcb[9], RwbT[9];
  poseopt::rotation_of(s.q, Rwb);
  mat3_t(Rbc, Rcb);
  mat3_t(Rwb, RwbT);
  mat3_mul(Rcb, RwbT, cam);
  cam[9] = s.P[0], cam[10] = s.P[1], cam[11] = s.P[2];
}
struct ReprojEval {
  double a[3];      // Rcb Rwb^T (Pw - Pwb): Paux
  double x, y, z;   // Pc
  double e0, e1, w, chi2;
};
NV_HD void reproj_error(const double* cam, const double* camc, const Problem& p, const float* in, ReprojEval& E) {
  const double d[3] = {(double)in[0] - cam[9], (double)in[1] - cam[10], (double)in[2] - cam[11]};
  mat3_vec(cam, d, E.a);
  E.x = E.a[0] - camc[0], E.y = E.a[1] - camc[1], E.z = E.a[2] - camc[2];
  E.e0 = (double)in[3] - ((E.x / E.z) * p.fx + p.cx);
  E.e1 = (double)in[4] - ((E.y / E.z) * p.fy + p.cy);
  E.w = (double)in[5];
  E.chi2 = E.e0 * (E.w * E.e0 + 0. * E.e1) + E.e1 * (0. * E.e0 + E.w * E.e1);
}
// the 2 x 6 Jacobian over (dP, dPhi): the dV columns are zero
NV_HD void reproj_jacobian(const ReprojEval& E, const Problem& p, double J0[6], double J1[6]) {
  const double x = E.x, y = E.y, z = E.z;
  // Jpi = Maux / z, then -Jpi
  const double m00 = -(p.fx / z), m02 = -((-x / z * p.fx) / z), m11 = -(p.fy / z), m12 = -((-y / z * p.fy) / z);
  // the zeros of Maux and of hat() are not multiplied (poseopt_core.hpp's header: a product with a zero inside H and b is dropped)
  const double* a = E.a;
  const double* B = p.Rbc;  // Rcb[i][j] = B[j * 3 + i]
  for (int j = 0; j < 3; ++j) {
    const double c0 = B[j * 3], c1 = B[j * 3 + 1], c2 = B[j * 3 + 2];  // column j of Rcb
    J0[j] = m00 * -c0 + m02 * -c2;
    J1[j] = m11 * -c1 + m12 * -c2;
    // hat(Paux) Rcb, column j
    const double h0 = a[1] * c2 - a[2] * c1, h1 = a[2] * c0 - a[0] * c2, h2 = a[0] * c1 - a[1] * c0;
    J0[3 + j] = m00 * h0 + m02 * h2;
    J1[3 + j] = m11 * h1 + m12 * h2;
  }
}
template <int MUT>
NV_HD void reproj_terms(const ReprojEval& E, const Problem& p, bool robust, double acc[kSums]) {
  double rho0, rho1, J0[6], J1[6];
  robustify(E.chi2, kDeltaMono, robust, &rho0, &rho1);
  reproj_jacobian(E, p, J0, J1);
  const double wo = rho1 * E.w;
  double r0 = -(E.w * E.e0), r1 = -(E.w * E.e1);
  if (MUT != kMutHuberB) r0 = r0 * rho1, r1 = r1 * rho1;
  int k = 0;
  SIM3_UNROLL
  for (int i = 0; i < 6; ++i)
    SIM3_UNROLL
    for (int j = i; j < 6; ++j, ++k) acc[k] = acc[k] + ((J0[i] * wo) * J0[j] + (J1[i] * wo) * J1[j]);
  SIM3_UNROLL
  for (int i = 0; i < 6; ++i) acc[21 + i] = acc[21 + i] + (J0[i] * r0 + J1[i] * r1);
  acc[27] = acc[27] + rho0;
}

// ---- the single edges: error rows into W.e, chi2 / rho into W.sing; with `lin` the Jacobian rows into W.J (zeroed before) ------------------
NV_HD double quad_form(const double* e, const double* Om, int m) {  // _error . (information * _error)
  double c = 0.;
  PO_NOUNROLL
  for (int r = 0; r < m; ++r) {
    double v = 0.;
    PO_NOUNROLL
    for (int s = 0; s < m; ++s) v = v + Om[r * m + s] * e[s];
    c = c + e[r] * v;
  }
  return c;
}
NV_HD void put3(double* J, int row, int col, const double* B, double sign) {  // a 3 x 3 block
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) J[(row + i) * kND + col + j] = sign * B[i * 3 + j];
}

// EdgeNavStatePriorPVRBias g2otypes.cpp:504-559: vertex 0 the last frame's PVR, vertex 1 its bias
template <int MUT>
NV_HD void edge_prior(const Problem& p, Work& W, bool lin) {
  const State& s = W.est[1];
  const State& pr = p.prior;
  double* e = W.e;
  for (int i = 0; i < 3; ++i) e[i] = pr.P[i] - s.P[i], e[3 + i] = pr.V[i] - s.V[i];
  double qi[4], qp[4], qr[4];
  for (int i = 0; i < 4; ++i) qp[i] = pr.q[i];
  q_normalize(qp);
  q_inv(qp, qi);
  q_mul(qi, s.q, qr);
  so3_log(qr, e + 6);
  for (int i = 0; i < 3; ++i) e[9 + i] = (pr.bg[i] + pr.dbg[i]) - (s.bg[i] + s.dbg[i]), e[12 + i] = (pr.ba[i] + pr.dba[i]) - (s.ba[i] + s.dba[i]);
  const double c = quad_form(e, p.prior_info, 15);
  W.sing[0][kPrior] = c;
  robustify(c, kDeltaPrior, true, &W.sing[1][kPrior], &W.sing[2][kPrior]);
  if (!lin) return;
  const int cp = col_pvr<MUT>(1), cb = col_bias<MUT>(1);
  double R[9], Ji[9];
  const double I[9] = {1., 0., 0., 0., 1., 0., 0., 0., 1.};
  poseopt::rotation_of(s.q, R);
  so3_jrinv<MUT>(e + 6, Ji);
  put3(W.J, 0, cp, R, -1.);
  put3(W.J, 3, cp + 3, I, -1.);
  put3(W.J, 6, cp + 6, Ji, 1.);
  put3(W.J, 9, cb, I, -1.);
  put3(W.J, 12, cb + 3, I, -1.);
}

// the IMU term both edges share: dPij + JPg dBg + JPa dBa
NV_HD void corrected(const double* d, const double* Jg, const double* Ja, const State& b, double* o) {
  double g[3], a[3];
  mat3_vec(Jg, b.dbg, g);
  mat3_vec(Ja, b.dba, a);
  for (int i = 0; i < 3; ++i) o[i] = (d[i] + g[i]) + a[i];
}

// EdgeNavStatePVR g2otypes.cpp:8-213: vertex 0 the last (key) frame's PVR, vertex 1 the current frame's, vertex 2 the last's bias
template <int MUT>
NV_HD void edge_imu(const Problem& p, Work& W, bool lin) {
  const State& si = W.est[1];
  const State& sj = W.est[0];
  double* e = W.e + 15;
  const double dT = p.dT, dT2 = dT * dT;
  double RiT[4], u[3], v[3], cP[3], cV[3], r[3];
  q_inv(si.q, RiT);
  for (int i = 0; i < 3; ++i) {
    u[i] = ((sj.P[i] - si.P[i]) - si.V[i] * dT) - (0.5 * p.gw[i]) * dT2;
    v[i] = (sj.V[i] - si.V[i]) - p.gw[i] * dT;
  }
  corrected(p.dP, p.JPg, p.JPa, si, cP);
  corrected(p.dV, p.JVg, p.JVa, si, cV);
  poseopt::rotate(RiT, u[0], u[1], u[2], r);
  for (int i = 0; i < 3; ++i) e[i] = r[i] - cP[i];
  poseopt::rotate(RiT, v[0], v[1], v[2], r);
  for (int i = 0; i < 3; ++i) e[3 + i] = r[i] - cV[i];
  double jb[3], qd[4], qb[4], qdb[4], qdi[4], t[4], rR[4];
  mat3_vec(p.JRg, si.dbg, jb);
  so3_exp(jb, qb);
  q_of_matrix(p.dR, qd);
  q_mul(qd, qb, qdb);
  q_inv(qdb, qdi);
  q_mul(qdi, RiT, t);
  q_mul(t, sj.q, rR);
  so3_log(rR, e + 6);
  const double c = quad_form(e, W.oimu, 9);
  W.sing[0][kImu] = c;
  robustify(c, kDeltaImu, MUT != kMutImuNoKernel, &W.sing[1][kImu], &W.sing[2][kImu]);
  if (!lin) return;
  double Ri[9], Rj[9], RiTm[9], RjT[9], Ji[9], B[9], C[9], hu[3], hv[3];
  poseopt::rotation_of(si.q, Ri);
  poseopt::rotation_of(sj.q, Rj);
  mat3_t(Ri, RiTm);
  mat3_t(Rj, RjT);
  so3_jrinv<MUT>(e + 6, Ji);
  const int cj = col_pvr<MUT>(0);
  // vertex j, the current frame
  mat3_mul(RiTm, Rj, B);
  put3(W.J, 15, cj, B, 1.);
  put3(W.J, 18, cj + 3, RiTm, 1.);
  put3(W.J, 21, cj + 6, Ji, 1.);
  if (p.form != kFrame) return;
  // vertex i, the last frame
  const int ci = col_pvr<MUT>(1), cb = col_bias<MUT>(1);
  const double I[9] = {1., 0., 0., 0., 1., 0., 0., 0., 1.};
  put3(W.J, 15, ci, I, -1.);
  for (int k = 0; k < 9; ++k) B[k] = RiTm[k] * dT;
  put3(W.J, 15, ci + 3, B, -1.);
  mat3_vec(RiTm, u, hu);
  hat(hu, B);
  put3(W.J, 15, ci + 6, B, 1.);
  put3(W.J, 18, ci + 3, RiTm, -1.);
  mat3_vec(RiTm, v, hv);
  hat(hv, B);
  put3(W.J, 18, ci + 6, B, 1.);
  for (int k = 0; k < 9; ++k) C[k] = -Ji[k];
  mat3_mul(C, RjT, B);
  mat3_mul(B, Ri, C);
  put3(W.J, 21, ci + 6, C, 1.);
  // vertex 2, the last frame's bias
  put3(W.J, 15, cb, p.JPg, -1.);
  put3(W.J, 15, cb + 3, p.JPa, -1.);
  put3(W.J, 18, cb, p.JVg, -1.);
  put3(W.J, 18, cb + 3, p.JVa, -1.);
  double qe[4], qei[4], Et[9], Jr[9];
  so3_exp(e + 6, qe);
  q_inv(qe, qei);
  poseopt::rotation_of(qei, Et);
  so3_jr(jb, Jr);
  for (int k = 0; k < 9; ++k) C[k] = -Ji[k];
  mat3_mul(C, Et, B);
  mat3_mul(B, Jr, C);
  mat3_mul(C, p.JRg, B);
  put3(W.J, 21, cb, B, 1.);
}

// EdgeNavStateBias g2otypes.cpp:215-263: vertex 0 the last (key) frame's bias, vertex 1 the current frame's
template <int MUT>
NV_HD void edge_bias(const Problem& p, Work& W, bool lin) {
  const State& si = W.est[1];
  const State& sj = W.est[0];
  double* e = W.e + 24;
  for (int i = 0; i < 3; ++i) e[i] = (sj.bg[i] + sj.dbg[i]) - (si.bg[i] + si.dbg[i]), e[3 + i] = (sj.ba[i] + sj.dba[i]) - (si.ba[i] + si.dba[i]);
  // InvCovBgaRW / dT: diagonal, the zeros of the matrix multiplied as in chi2()
  const double wg = (1. / p.gyr_rw2) / p.dT, wa = (1. / p.acc_rw2) / p.dT, z = 0. / p.dT;
  double c = 0.;
  for (int r = 0; r < 6; ++r) {
    double v = 0.;
    for (int s = 0; s < 6; ++s) v = v + (r == s ? (r < 3 ? wg : wa) : z) * e[s];
    c = c + e[r] * v;
  }
  W.sing[0][kBias] = c;
  robustify(c, kDeltaBias, true, &W.sing[1][kBias], &W.sing[2][kBias]);
  if (!lin) return;
  const int cj = col_bias<MUT>(0), ci = col_bias<MUT>(1);
  for (int i = 0; i < 6; ++i) {
    W.J[(24 + i) * kND + cj + i] = 1.;
    if (p.form == kFrame) W.J[(24 + i) * kND + ci + i] = -1.;
  }
}

// EdgeNavStateDepthProjected g2otypes.cpp:292-392, literally.  Key-frame form: vertex 0 the key frame, vertex 1 the current frame, vertex 2
// the key frame's bias (Optimizer.cc:904-906).  Frame form: vertex 0 the CURRENT frame, vertex 1 the last, vertex 2 the last's bias (:461-463).
template <int MUT>
NV_HD void edge_depth(const Problem& p, Work& W, bool lin) {
  const bool cur_first = (p.form == kFrame) != (MUT == kMutDepthSwap && p.form == kFrame);
  const State& s0 = cur_first ? W.est[0] : W.est[1];
  const State& s1 = cur_first ? W.est[1] : W.est[0];
  const State& sb = W.est[1];
  const double dT = p.dT, dT2 = dT * dT;
  const double proj = p.shi * (p.depth_meas - s0.P[2]) + s0.P[2];
  const double r1 = proj - s1.P[2];
  double R0[9], c[3], Rc[3], kf[3];
  poseopt::rotation_of(s0.q, R0);
  corrected(p.dP, p.JPg, p.JPa, sb, c);
  mat3_vec(R0, c, Rc);
  const double G[3] = {0., 0., 9.81};
  for (int i = 0; i < 3; ++i) kf[i] = ((s0.P[i] + dT * s0.V[i]) + (MUT == kMutDepthHalf ? 0.5 * dT2 : dT2) * G[i]) + Rc[i];
  const double r2 = proj - kf[2];
  const double e = r1 + r2;
  W.e[30] = e;
  const double chi = e * (p.depth_info * e);
  W.sing[0][kDepth] = chi;
  robustify(chi, kDeltaDepth, true, &W.sing[1][kDepth], &W.sing[2][kDepth]);
  if (!lin) return;
  double* J = W.J + 30 * kND;
  const int f0 = cur_first ? 0 : 1, f1 = cur_first ? 1 : 0;
  if (f1 == 0 || p.form == kFrame) J[col_pvr<MUT>(f1) + 2] = -1.;
  if (f0 == 0 || p.form == kFrame) {
    const int c0 = col_pvr<MUT>(f0);
    J[c0 + 2] = 2. * (1. - p.shi) - 1.;
    J[c0 + 5] = -dT;
    // (hat(Ri c) e3)^T: the third column of hat
    J[c0 + 6] = Rc[1], J[c0 + 7] = -Rc[0], J[c0 + 8] = 0.;
  }
  if (p.form == kFrame) {
    const int cb = col_bias<MUT>(1);
    double nR[9], Bg[9], Ba[9];
    for (int k = 0; k < 9; ++k) nR[k] = -R0[k];
    mat3_mul(nR, p.JPg, Bg);
    mat3_mul(nR, p.JPa, Ba);
    for (int k = 0; k < 3; ++k) J[cb + k] = Bg[k * 3 + 2], J[cb + 3 + k] = Ba[k * 3 + 2];
  }
}

NV_HD bool edge_active(const Problem& p, int k) { return k == kPrior ? p.form == kFrame : k == kDepth ? p.has_depth != 0 : true; }
NV_HD int row_edge(int r) { return r < 15 ? kPrior : r < 24 ? kImu : r < 30 ? kBias : kDepth; }
NV_HD int edge_row0(int k) { return k == kPrior ? 0 : k == kImu ? 15 : k == kBias ? 24 : 30; }
NV_HD int edge_dim(int k) { return k == kPrior ? 15 : k == kImu ? 9 : k == kBias ? 6 : 1; }
// information of edge k, entry (r, s) inside the edge
NV_HD double edge_info(const Problem& p, const Work& W, int k, int r, int s) {
  if (k == kPrior) return p.prior_info[r * 15 + s];
  if (k == kImu) return W.oimu[r * 9 + s];
  if (k == kBias) return r == s ? (1. / (r < 3 ? p.gyr_rw2 : p.acc_rw2)) / p.dT : 0. / p.dT;
  return p.depth_info;
}

template <int MUT>
NV_HD void single_edge(const Problem& p, Work& W, int k, bool lin) {
  if (!edge_active(p, k)) {
    W.sing[0][k] = 0., W.sing[1][k] = 0., W.sing[2][k] = 0.;
    return;
  }
  if (k == kPrior) edge_prior<MUT>(p, W, lin);
  else if (k == kImu) edge_imu<MUT>(p, W, lin);
  else if (k == kBias) edge_bias<MUT>(p, W, lin);
  else edge_depth<MUT>(p, W, lin);
}
// rho0 of the single edges, in their order
NV_HD double single_chi2(const Problem& p, const Work& W, double sum) {
  PO_NOUNROLL
  for (int k = 0; k < 4; ++k)
    if (edge_active(p, k)) sum = sum + W.sing[1][k];
  return sum;
}

// ---- the dense LDL^T ---------------------------------------------------------------------------------------------------------------------
// A (leading dimension ld): the lower triangle of a symmetric n x n matrix; on return the unit factor below the diagonal, d on it.
// Returns whether every pivot is finite and > 0.
template <class Team>
NV_HD bool ldl_factor(Team& T, double* A, int n, int ld) {
  bool ok = true;
  PO_NOUNROLL
  for (int j = 0; j < n; ++j) {
    const double d = A[j * ld + j];
    ok = ok && d > 0. && d <= DBL_MAX;
    const int m = n - 1 - j;
    T.each(m, [&](int t) {
      const int i = j + 1 + t;
      A[i * ld + j] = A[i * ld + j] / d;
    });
    T.each(m * (m + 1) / 2, [&](int t) {
      // t -> (i, k), j < k <= i < n, rows in turn
      int r = 0;
      while ((r + 1) * (r + 2) / 2 <= t) ++r;
      const int i = j + 1 + r, k = j + 1 + (t - r * (r + 1) / 2);
      A[i * ld + k] = A[i * ld + k] - (A[i * ld + j] * A[k * ld + j]) * d;
    });
  }
  return ok;
}
// X (n x m, leading dimension ldx) <- inv(L D L^T) X, column-oriented: every entry loses its terms in ascending (forward) or descending
// (backward) order of the other index
template <class Team>
NV_HD void ldl_solve(Team& T, const double* A, int n, int ld, double* X, int m, int ldx) {
  PO_NOUNROLL
  for (int j = 0; j < n - 1; ++j)
    T.each((n - 1 - j) * m, [&](int t) {
      const int i = j + 1 + t / m, c = t % m;
      X[i * ldx + c] = X[i * ldx + c] - A[i * ld + j] * X[j * ldx + c];
    });
  T.each(n * m, [&](int t) {
    const int i = t / m, c = t % m;
    X[i * ldx + c] = X[i * ldx + c] / A[i * ld + i];
  });
  PO_NOUNROLL
  for (int j = n - 1; j > 0; --j)
    T.each(j * m, [&](int t) {
      const int i = t / m, c = t % m;
      X[i * ldx + c] = X[i * ldx + c] - A[j * ld + i] * X[j * ldx + c];
    });
}
// X[0..n)[0..m) <- the first m columns of the inverse of the symmetric matrix whose lower triangle src(i, k) gives; A is the work
template <class Team, class F>
NV_HD bool ldl_inverse(Team& T, F src, double* A, int n, int ld, double* X, int m, int ldx) {
  T.each(n * n, [&](int t) {
    const int i = t / n, k = t % n;
    if (k <= i) A[i * ld + k] = src(i, k);
    if (k < m) X[i * ldx + k] = i == k ? 1. : 0.;
  });
  const bool ok = ldl_factor(T, A, n, ld);
  ldl_solve(T, A, n, ld, X, m, ldx);
  return ok;
}

// ---- oplus: IncSmallPVR NavState.cpp:71-100, IncSmallBias :102-123 ----------------------------------------------------------------------
template <int MUT>
NV_HD void oplus(const double* dx, int frame, State& s) {
  const double* u = dx + col_pvr<MUT>(frame);
  const double* ub = dx + col_bias<MUT>(frame);
  double R[9], Rp[3], dq[4], q[4];
  poseopt::rotation_of(s.q, R);  // the rotation before the update
  mat3_vec(R, u, Rp);
  for (int i = 0; i < 3; ++i) s.P[i] = s.P[i] + Rp[i], s.V[i] = s.V[i] + u[3 + i];
  so3_exp(u + 6, dq);
  q_mul(s.q, dq, q);
  for (int i = 0; i < 4; ++i) s.q[i] = q[i];
  for (int i = 0; i < 3; ++i) s.dbg[i] = s.dbg[i] + ub[i], s.dba[i] = s.dba[i] + ub[3 + i];
}

// UpdatePoseFromNS FrameKTL.cc:160-181 (CV_32F products: see the header)
NV_HD void pose_from_ns(const State& s, const Problem& p, float* Tcw) {
  double Rd[9], Rwb[9], Rbc[9], Pbc[3], Pwb[3], RR[9], Rcw[9], Pwc[3], t[3];
  poseopt::rotation_of(s.q, Rd);
  for (int k = 0; k < 9; ++k) Rwb[k] = (double)(float)Rd[k], Rbc[k] = (double)(float)p.Rbc[k];
  for (int k = 0; k < 3; ++k) Pwb[k] = (double)(float)s.P[k], Pbc[k] = (double)(float)p.Pbc[k];
  mat3_mul(Rwb, Rbc, RR);
  mat3_t(RR, Rcw);
  for (int k = 0; k < 9; ++k) Rcw[k] = (double)(float)Rcw[k];
  mat3_vec(Rwb, Pbc, Pwc);
  for (int k = 0; k < 3; ++k) Pwc[k] = (double)(float)(Pwc[k] + Pwb[k]);
  mat3_vec(Rcw, Pwc, t);
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) Tcw[i * 4 + j] = (float)Rcw[i * 3 + j];
    Tcw[i * 4 + 3] = -(float)t[i];
  }
  Tcw[12] = 0.f, Tcw[13] = 0.f, Tcw[14] = 0.f, Tcw[15] = 1.f;
}

NV_HD int tri_index(int a, int b, int nd) { return a * nd - a * (a - 1) / 2 + (b - a); }  // a <= b

// ---- the host's team -----------------------------------------------------------------------------------------------------------------
#if !defined(__HIP_DEVICE_COMPILE__)
struct HostTeam : HostLaneTeam<kSums> {
  template <class F>
  void each(int count, F f) {
    for (int i = 0; i < count; ++i) f(i);
  }
};
#endif

// ---- one linearisation: computeActiveErrors, activeRobustChi2, buildSystem -> W.H, W.b, S[27] + S[55] and the single edges' rho0 ----------
template <int MUT, class Team>
NV_HD double linearise(Team& T, const Problem& p, const Edges& E, Work& W, bool robust, int nd) {
  double* const S = T.shared();
  T.each(kRows * kND + 2, [&](int t) {
    if (t < kRows * kND) W.J[t] = 0.;
    else frame_camera(W.est[t - kRows * kND], p.Rbc, W.cam[t - kRows * kND]);
  });
  T.each(nd * nd + nd, [&](int t) {
    if (t < nd * nd) W.H[(t / nd) * kND + t % nd] = 0.;
    else W.b[t - nd * nd] = 0.;
  });
  T.each(4, [&](int k) { single_edge<MUT>(p, W, k, true); });
  double chi[2] = {0., 0.};
  PO_NOUNROLL
  for (int f = 0; f < 2; ++f) {
    if (f == 1 && p.form != kFrame) continue;
    const int i0 = f == 0 ? 0 : p.n, i1 = f == 0 ? p.n : p.n + p.n_last;
    const double* cam = W.cam[f];
    T.template sum_shared<kSums>(
        [&](int lane, double* acc) {
          PO_NOUNROLL
          for (int i = i0 + lane; i < i1; i += kLanes) {
            if (E.state[i] & kLevel) continue;
            ReprojEval ev;
            reproj_error(cam, W.camc, p, E.in + 6 * i, ev);
            E.chi2[i] = ev.chi2;
            reproj_terms<MUT>(ev, p, robust, acc);  // adds the edge's terms of H (upper triangle, row-major), b and the robust chi2
          }
        },
        S);
    chi[f] = S[27];
    // the frame's sums into its P and Phi rows and columns
    const int cp = col_pvr<MUT>(f);
    T.each(27, [&](int t) {
      if (t < 21) {
        int a = 0, k = t;
        while (k >= 6 - a) k -= 6 - a, ++a;
        const int b = a + k;
        W.H[(cp + (a < 3 ? a : a + 3)) * kND + cp + (b < 3 ? b : b + 3)] = S[t];
      } else {
        const int a = t - 21;
        W.b[cp + (a < 3 ? a : a + 3)] = S[t];
      }
    });
  }
  // WJ = (rho1 Omega) J, We = (rho1 Omega) e, row by row inside each edge
  T.each(kRows * (nd + 1), [&](int t) {
    const int r = t / (nd + 1), c = t % (nd + 1), k = row_edge(r);
    if (!edge_active(p, k)) return;
    const int r0 = edge_row0(k), m = edge_dim(k);
    const double rho1 = W.sing[2][k];
    double v = 0.;
    PO_NOUNROLL
    for (int s = 0; s < m; ++s) v = v + (rho1 * edge_info(p, W, k, r - r0, s)) * (c < nd ? W.J[(r0 + s) * kND + c] : W.e[r0 + s]);
    if (c < nd) W.WJ[r * kND + c] = v;
    else W.We[r] = v;
  });
  T.each(nd * (nd + 1) / 2 + nd, [&](int t) {
    const int ntri = nd * (nd + 1) / 2;
    if (t < ntri) {
      int a = 0, k = t;
      while (k >= nd - a) k -= nd - a, ++a;
      const int b = a + k;
      double v = 0.;
      PO_NOUNROLL
      for (int r = 0; r < kRows; ++r)
        if (edge_active(p, row_edge(r))) v = v + W.J[r * kND + a] * W.WJ[r * kND + b];
      W.H[a * kND + b] = W.H[a * kND + b] + v;
    } else {
      const int a = t - ntri;
      double v = 0.;
      PO_NOUNROLL
      for (int r = 0; r < kRows; ++r)
        if (edge_active(p, row_edge(r))) v = v + W.J[r * kND + a] * W.We[r];
      W.b[a] = W.b[a] - v;
    }
  });
  return single_chi2(p, W, chi[0] + chi[1]);
}

// activeRobustChi2 after computeActiveErrors at the tried estimate
template <int MUT, class Team>
NV_HD double trial_chi2(Team& T, const Problem& p, const Edges& E, Work& W, bool robust) {
  T.each(6, [&](int t) {
    if (t < 4) single_edge<MUT>(p, W, t, false);
    else frame_camera(W.est[t - 4], p.Rbc, W.cam[t - 4]);
  });
  double chi[2] = {0., 0.};
  PO_NOUNROLL
  for (int f = 0; f < 2; ++f) {
    if (f == 1 && p.form != kFrame) continue;
    const int i0 = f == 0 ? 0 : p.n, i1 = f == 0 ? p.n : p.n + p.n_last;
    const double* cam = W.cam[f];
    T.template sum<1>(
        [&](int lane, double* acc) {
          PO_NOUNROLL
          for (int i = i0 + lane; i < i1; i += kLanes) {
            if (E.state[i] & kLevel) continue;
            ReprojEval ev;
            reproj_error(cam, W.camc, p, E.in + 6 * i, ev);
            E.chi2[i] = ev.chi2;
            double rho0, rho1;
            robustify(ev.chi2, kDeltaMono, robust, &rho0, &rho1);
            acc[0] = acc[0] + rho0;
          }
        },
        &chi[f]);
  }
  return single_chi2(p, W, chi[0] + chi[1]);
}

// one Levenberg trial from W.H, W.b and W.est: push, (H + lambda I) x = b, oplus, the robust chi2 at the tried estimate (DBL_MAX after a
// failed solve, when W.dx keeps its previous value), computeScale() + 1e-3.  W.backup holds the estimates for the pop.
template <int MUT, class Team>
NV_HD bool try_step(Team& T, const Problem& p, const Edges& E, Work& W, bool robust, int nd, double lambda, double* tmp, double* scale) {
  T.each(nd * nd + 2, [&](int t) {
    if (t < nd * nd) {
      const int i = t / nd, k = t % nd;
      if (k <= i) W.A[i * kND + k] = i == k ? W.H[i * kND + i] + lambda : W.H[k * kND + i];
      if (k == 0) W.y[i] = W.b[i];
    } else {
      W.backup[t - nd * nd] = W.est[t - nd * nd];
    }
  });
  const bool ok = ldl_factor(T, W.A, nd, kND);
  ldl_solve(T, W.A, nd, kND, W.y, 1, 1);
  if (ok) T.each(nd, [&](int t) { W.dx[t] = W.y[t]; });
  T.each(p.form == kFrame ? 2 : 1, [&](int t) { oplus<MUT>(W.dx, t, W.est[t]); });
  const double chi = trial_chi2<MUT>(T, p, E, W, robust);
  *tmp = ok ? chi : DBL_MAX;
  double s = 0.;
  PO_NOUNROLL
  for (int j = 0; j < nd; ++j) s = s + W.dx[j] * (lambda * W.dx[j] + W.b[j]);
  *scale = s + 1e-3;
  return ok;
}

// computeMarginals on H as the last buildSystem left it, and mMargCovInv as the overload stores it.  The frame form of the reference
// reads spinv.block(0,1), which computeMarginals(vertices) never fills: the joint 15 x 15 block is what the line means and what this is.
template <int MUT, class Team>
NV_HD bool marginals(Team& T, const Problem& p, Work& W, int nd, Out* out) {
  bool ok = ldl_inverse(T, [&](int i, int k) { return W.H[k * kND + i]; }, W.A, nd, kND, W.X, 15, 15);
  // the current frame's (PVR, bias) in the ABI's order whatever the Hessian's
  const int cp = col_pvr<MUT>(0), cb = col_bias<MUT>(0);
  T.each(225, [&](int t) {
    const int i = t / 15, k = t % 15;
    const int hi = i < 9 ? cp + i : cb + i - 9, hk = k < 9 ? cp + k : cb + k - 9;
    W.M15[t] = W.X[hi * 15 + hk];
  });
  const bool joint = (p.form == kFrame) != (MUT == kMutMargSwap);
  double* C = W.WJ;  // 15 x 15 scratch for the inverse's columns
  if (joint) {
    ok = ldl_inverse(T, [&](int i, int k) { return W.M15[i * 15 + k]; }, W.A, 15, kND, C, 15, 15) && ok;
  } else {
    T.each(225, [&](int t) { C[t] = 0.; });
    ok = ldl_inverse(T, [&](int i, int k) { return W.M15[i * 15 + k]; }, W.A, 9, kND, C, 9, 15) && ok;
    ok = ldl_inverse(T, [&](int i, int k) { return W.M15[(9 + i) * 15 + 9 + k]; }, W.A, 6, kND, C + 9 * 15 + 9, 6, 15) && ok;
  }
  T.each(225, [&](int t) { out->marg_cov[t] = W.M15[t], out->marg_cov_inv[t] = C[t]; });
  return ok;
}

// ---- the call --------------------------------------------------------------------------------------------------------------------------
// Every member of the team calls this with the same arguments.  tr may be null.
template <int MUT, class Team>
NV_HD void run(Team& T, const Problem& p, const Edges& E, Work& W, Out* out, Trace* tr) {
  const int n = p.n, nl = p.form == kFrame ? p.n_last : 0, nall = n + nl;
  const int nd = p.form == kFrame ? 30 : 15;
  const int n_edges = nall + 2 + (p.form == kFrame ? 1 : 0) + (p.has_depth ? 1 : 0);  // optimizer.edges().size()
  (void)T.count([&](int lane) {
    for (int i = lane; i < nall; i += kLanes) E.chi2[i] = 0., E.state[i] = 0, E.mask[i] = 0;
    return 0;
  });
  T.each(3, [&](int t) {
    if (t < 2) {
      W.est[t] = t == 0 ? p.cur : p.last;
      q_normalize(W.est[t].q);
    } else {
      double Rcb[9];
      mat3_t(p.Rbc, Rcb);
      mat3_vec(Rcb, p.Pbc, W.camc);
    }
  });
  int n_lin = 0, n_trials = 0, n_bad = 0, rounds = 0, marg_ok = 0;
  const bool run_it = n >= (p.form == kFrame ? 4 : 3);  // the early return: 0, nothing changed
  if (run_it) {
    const bool cov_ok = ldl_inverse(T, [&](int i, int k) { return p.cov[i * 9 + k]; }, W.A, 9, kND, W.X, 9, 15);
    (void)cov_ok;  // a covariance that is not positive definite leaves non-finite information: every solve fails
    T.each(81, [&](int t) { W.oimu[t] = W.X[(t / 9) * 15 + t % 9]; });
    double lambda = 0.;
    PO_NOUNROLL
    for (int round = 0; round < kRounds; ++round) {
      rounds = round + 1;
      const bool robust = round < 3;  // setRobustKernel(0) after the classification of round index 2, reprojection edges only
      if (MUT != kMutNoReset || round == 0)
        T.each(2, [&](int t) {  // Reset estimates
          W.est[t] = t == 0 ? p.cur : p.last;
          q_normalize(W.est[t].q);
        });
      T.each(nd, [&](int t) { W.dx[t] = 0.; });
      double ni = 2.;
      int stalled = 0;
      bool go = true;
      PO_NOUNROLL
      for (int it = 0; it < kIts; ++it) {
        if (!go) continue;
        double cur = linearise<MUT>(T, p, E, W, robust, nd);
        const double ini = cur;
        if (it == 0) {  // computeLambdaInit: tau * max |H_jj| over all free vertices
          double mx = 0.;
          PO_NOUNROLL
          for (int j = 0; j < nd; ++j) {
            const double h = fabs(W.H[j * kND + j]);
            mx = h < mx ? mx : h;
          }
          lambda = 1e-5 * mx;
          ni = 2., stalled = 0;
        }
        const int lin = n_lin;
        if (tr && lin < kMaxLin) {
          TraceLin& r = tr->lin[lin];
          T.each(kTri + kND + 1, [&](int t) {
            if (t < kTri) {
              double v = 0.;
              if (t < nd * (nd + 1) / 2) {
                int a = 0, k = t;
                while (k >= nd - a) k -= nd - a, ++a;
                v = W.H[a * kND + a + k];
              }
              r.H[t] = v;
            } else if (t < kTri + kND) {
              r.b[t - kTri] = t - kTri < nd ? W.b[t - kTri] : 0.;
            } else {
              r.round = round, r.iteration = it, r.chi2 = cur;
            }
          });
        }
        ++n_lin;
        double rho = 0.;
        int q = 0;
        bool again = true;
        PO_NOUNROLL
        for (int trial = 0; trial < kMaxTrials; ++trial) {
          if (!again) continue;
          double tmp, scale;
          const bool ok = try_step<MUT>(T, p, E, W, robust, nd, lambda, &tmp, &scale);
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
            alpha = 2. / 3. < alpha ? 2. / 3. : alpha;
            const double sf = 1. / 3. < alpha ? alpha : 1. / 3.;
            lambda = lambda * sf;
            ni = 2.;
            cur = tmp;
          } else {
            lambda = lambda * ni;
            ni = ni * 2.;
            T.each(2, [&](int t) { W.est[t] = W.backup[t]; });  // pop
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
      // classification of both frames' edges: const float chi2 = e->chi2(); chi2 > chi2Mono[it]
      T.each(2, [&](int t) { frame_camera(W.est[t], p.Rbc, W.cam[t]); });
      const int packed = T.count([&](int lane) {
        int c = 0;
        PO_NOUNROLL
        for (int i = lane; i < nall; i += kLanes) {
          uint8_t st = E.state[i];
          if (st & kFlag) {
            ReprojEval ev;
            reproj_error(W.cam[i < n ? 0 : 1], W.camc, p, E.in + 6 * i, ev);
            E.chi2[i] = ev.chi2;
          }
          const float c2 = (float)E.chi2[i];
          if (c2 > kChi2Mono) {
            st = kFlag | kLevel;
            c += i < n ? 1 : 0;
          } else {
            st = 0;  // `else`: a NaN chi2 is an inlier here (the vision-only overload leaves it as it was)
          }
          E.state[i] = st;
          E.mask[i] = (st & kFlag) ? 1 : 0;
          if (MUT == kMutBreakActive) c += (st & kLevel) ? 1 << 16 : 0;  // the mutation's count; its scenes are small
        }
        return c;
      });
      n_bad = packed & 0xffff;
      const int n_active = nall - (packed >> 16);
      if ((MUT == kMutBreakActive ? n_active : n_edges) < 10) break;
    }
    if (p.compute_marg) {
      if (MUT == kMutMargFresh) (void)linearise<MUT>(T, p, E, W, rounds - 1 < 3, nd);
      marg_ok = marginals<MUT>(T, p, W, nd, out) ? 1 : 0;
    }
  }
  if (!(run_it && p.compute_marg)) T.each(225, [&](int t) { out->marg_cov[t] = 0., out->marg_cov_inv[t] = 0.; });
  if (T.lead()) {
    out->ns = W.est[0];
    pose_from_ns(W.est[0], p, out->Tcw);
    out->n_inliers = run_it ? n - n_bad : 0, out->rounds = rounds, out->marg_ok = marg_ok, out->pad_ = 0;
    if (tr) tr->n_lin = n_lin, tr->n_trials = n_trials;
  }
}

}  // namespace navopt
}  // namespace uvo
