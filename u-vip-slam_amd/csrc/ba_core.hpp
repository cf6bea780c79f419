// Optimizer::LocalBundleAdjustment (src/Optimizer.cc:2147-2405 of the reference) and Optimizer::BundleAdjustment (:1896-2010), with the
// parts of g2o they run: EdgeSE3ProjectXYZ, the Huber kernel, BlockSolver's Schur complement, the Levenberg driver.  Plain C++ in
// double under the rules of poseopt_core.hpp: IEEE + - * / sqrt and fabs only, no contraction (-ffp-contract=off on both sides), no
// library function.  ba.hip runs this on the device, tests/emu/ba_emu.cpp on the host; the two are held to each other bit for bit.
//
// The work is cut into PHASES.  A phase is a function of (workspace, team, block index); a block is what one workgroup of 256 lanes
// does.  The device launches one kernel per phase with one workgroup per block, the host build calls the blocks one after the other.
// Which phases run is decided by drive() below, host code shared by both builds; the Levenberg decision itself is made in the
// phases lin_ctl and trial_ctl (one block each), which leave a status word for drive() to read.  Nothing waits for another block
// inside a phase.
//
// EVERY FLOATING-POINT SUM HAS ONE FIXED SHAPE THAT DEPENDS ON INDICES ALONE:
//   1. per point (Hll's 6 entries, b_l's 3; b_l - W^T x_p): one lane walks the point's edges serially in edge order onto 0.0 (or b_l),
//      skipping the removed ones.
//   2. per free key frame (Hpp_ii's 21 entries, b_p's 6): the block of that key frame walks the key frame's edge list (ascending edge
//      index, built at upload) in poseopt_core.hpp's shape: lane l takes entries l, l + 256, ..., the butterfly, (w0 + w1) + (w2 + w3).
//   3. per Schur block (i1 <= i2): the block walks key frame i1's edge list in the same shape; an entry contributes when its point
//      also has an edge to i2 (a table key frame x point -> edge built at upload) and both edges are active.  The position of a
//      term is its position in i1's list, so no second list is needed.  bschur's correction is 6 more sums of the diagonal block.
//   4. scalars (robust chi2, x . (lambda x + b) over the points): per chunk of 256 edges or points in the shape of 2 with one entry
//      a lane, then the chunk sums folded in ascending order onto 0.0 (chi2) or onto the poses' serial sum (scale).
//   5. the reduced system: a dense unpivoted LDL^T in natural key-frame order, in place on the lower triangle; every entry receives its
//      updates in ascending k as v - (L_ik * L_jk) * d_k; forward substitution in ascending k, back substitution in descending k.
// No floating-point atomics.  The largest diagonal entry is a maximum: any order; a NaN entry makes it NaN.
// These shapes are also navba_core.hpp's, over its own key-frame unknowns.  What both cores run is written once, in the section "the
// Schur pieces" below, templated on the workspace; this file owns it, navba_core.hpp calls it.
//
// Departures from the reference, stated in uvo.h and DESIGN.md section 4: the dense LDL^T in place of SimplicialLDLT under an AMD
// ordering ("ok" = every pivot finite and > 0); the sums' shapes above in place of g2o's serial order over its own edge and vertex
// containers; sin, cos as in poseopt_core.hpp; on a failed solve the step keeps its previous value (zero at the start of an
// optimize()); a free key frame or a point without an active edge is outside the system, as after initializeOptimization().
#pragma once
#include "poseopt_core.hpp"

namespace uvo {
namespace ba {

using poseopt::Pose;
using poseopt::kLanes;

constexpr int kMaxFree = 64, kMaxFixed = 256, kMaxPoints = 32768, kMaxEdges = 262144, kMaxCams = 64;
constexpr int kMaxIterations = 32;              // full mode; local mode runs 5 + 10
constexpr int kMaxTrials = 10;
constexpr int kMaxLin = kMaxIterations, kMaxTrialRecs = kMaxIterations * kMaxTrials;
constexpr int kSchurSums = 42;                  // 36 of W Dinv W^T, 6 of W Dinv b_l
constexpr int kEdgeWords = 22;                  // per edge: Jp[2][6], Jl[2][3], wo, r0, r1, rho0
constexpr int kModeLocal = 0, kModeFull = 1;

// seeded mutations, for the host build only (tests/emu/ba_emu.cpp); the library instantiates MUT = 0
constexpr int kMutNone = 0, kMutLambdaPoseOnly = 1, kMutDinvPlain = 2, kMutFixedW = 3, kMutSchurAdd = 4, kMutNoWx = 5, kMutReeval = 6,
              kMutReturn = 7, kMutStepIdle = 8, kMutTauPoses = 9;

enum Phase { kInit = 0, kBegin, kEdgeLin, kPointSum, kKfSum, kLinCtl, kDinv, kSchur, kSolve, kStep, kEdgeErr, kTrialCtl, kCheck, kFinish, kPhases };
// status left by kBegin / kLinCtl / kTrialCtl
constexpr int kStTrial = 1, kStLinearise = 2, kStStop = 3;

struct TraceLin {
  int32_t round, iteration, n_edges, n_free, n_points, pad_;
  double chi2, maxdiag;
};
struct Trace {
  int32_t n_lin, n_trials;
  TraceLin lin[kMaxLin];
  poseopt::TraceTrial trial[kMaxTrialRecs];
};

struct Ctl {
  double lambda, ni, cur, ini, rho;
  int32_t round, it, q, stalled, status, solve_ok, n_lin, n_trials;
  int32_t its[2];
};

struct Ws {
  int32_t K, F, P, E, C, pad_;
  // the upload
  const float* kf_T;        // [K][12]
  const int32_t* kf_free;   // [K] index among the free key frames, -1: fixed
  const int32_t* free_kf;   // [F]
  const float* pts;         // [P][3]
  const uint8_t* pt_bad;    // [P]
  const int32_t* pt_begin;  // [P + 1]
  const int32_t* e_kf;      // [E]
  const int32_t* e_pt;      // [E]
  const int32_t* e_cam;     // [E]
  const float* e_obs;       // [E][3]: x y invSigma2
  const float* cams;        // [C][4]: fx fy cx cy
  const int32_t* kl_begin;  // [F + 1]
  const int32_t* kl_edge;   // [<= E] a free key frame's edges, ascending
  const int32_t* fp_edge;   // [F][P] the edge of (free key frame, point), -1: none
  // state
  Pose *pose, *pose_try;    // [K]
  double *X, *X_try;        // [P][3]
  uint8_t* e_off;           // [E] 1: removed
  double* e_chi2;           // [E] chi2 of the stored error: that of the last evaluation, accepted or not
  double* e_lin;            // [E][kEdgeWords]
  double* Hll;              // [P][9]: the 6 upper entries, b_l
  double* Dinv;             // [P][9]: the 6 upper entries of (Hll + lambda I)^-1, Dinv b_l
  uint8_t* p_on;            // [P] has an active edge
  double* Hpp;              // [F][27]: the 21 upper entries, b_p
  uint8_t* f_on;            // [F]
  double* Hs;               // [6F][6F], the lower triangle
  double *bs, *xp;          // [6F]
  double* xl;               // [P][3]
  double *chunk_chi2, *chunk_scale, *chunk_max;  // [chunks of E], [chunks of P], [chunks of P + F]
  int32_t* chunk_n;         // [chunks of E] active edges
  Ctl* ctl;
  Trace* trace;
  uint8_t *removed1, *removed2;  // [E]
  // the download
  double* kf_est;           // [K][7] q (x y z w), t
  float* kf_T_out;          // [K][16]
  double* pt_est;           // [P][3]
  float* pt_out;            // [P][3]
};

PO_HD int chunks(int n) { return (n + kLanes - 1) / kLanes; }
PO_HD int schur_blocks(int F) { return F * (F + 1) / 2; }

// ---- one edge ------------------------------------------------------------------------------------------------------------------------
// computeError: obs - cam_project(T.map(X)), chi2 with the information invSigma2 * I
PO_HD void edge_error(const Ws& W, int e, const Pose* poses, const double* X, poseopt::EdgeEval& E, poseopt::Cam& C) {
  const Pose& P = poses[W.e_kf[e]];
  const double* x = X + 3 * (size_t)W.e_pt[e];
  double p[3];
  poseopt::rotate(P.q, x[0], x[1], x[2], p);
  E.x = p[0] + P.t[0], E.y = p[1] + P.t[1], E.z = p[2] + P.t[2];
  const float* c = W.cams + 4 * W.e_cam[e];
  C.fx = (double)c[0], C.fy = (double)c[1], C.cx = (double)c[2], C.cy = (double)c[3];
  const float* o = W.e_obs + 3 * (size_t)e;
  E.e0 = (double)o[0] - ((E.x / E.z) * C.fx + C.cx);
  E.e1 = (double)o[1] - ((E.y / E.z) * C.fy + C.cy);
  E.w = (double)o[2];
  E.chi2 = E.e0 * (E.w * E.e0 + 0. * E.e1) + E.e1 * (0. * E.e0 + E.w * E.e1);
}

// linearizeOplus and the robustified weights: what constructQuadraticForm needs of the edge.  Returns rho[0].
PO_HD double edge_linearise(const Ws& W, int e) {
  poseopt::EdgeEval E;
  poseopt::Cam C;
  edge_error(W, e, W.pose, W.X, E, C);
  W.e_chi2[e] = E.chi2;
  double rho0, rho1;
  poseopt::huber(E.chi2, &rho0, &rho1);
  double* L = W.e_lin + (size_t)e * kEdgeWords;
  poseopt::jacobian(E, C, L, L + 6);
  // _jacobianOplusXi = (-1./z * tmp) * R
  double R[9];
  poseopt::rotation_of(W.pose[W.e_kf[e]].q, R);
  const double s = -1. / E.z;
  const double a00 = s * C.fx, a02 = s * (-E.x / E.z * C.fx), a11 = s * C.fy, a12 = s * (-E.y / E.z * C.fy), a01 = s * 0., a10 = s * 0.;
  SIM3_UNROLL
  for (int j = 0; j < 3; ++j) {
    L[12 + j] = (a00 * R[j] + a01 * R[3 + j]) + a02 * R[6 + j];
    L[15 + j] = (a10 * R[j] + a11 * R[3 + j]) + a12 * R[6 + j];
  }
  L[18] = rho1 * E.w;  // robustInformation: rho[1] * information
  L[19] = -(E.w * E.e0) * rho1, L[20] = -(E.w * E.e1) * rho1;
  L[21] = rho0;
  return rho0;
}

// Hpl's block of the edge: W[a][b] = Jp^T (rho1 Omega) Jl, 6 x 3
PO_HD void edge_W(const double* L, double Wm[18]) {
  SIM3_UNROLL
  for (int a = 0; a < 6; ++a)
    SIM3_UNROLL
    for (int b = 0; b < 3; ++b) Wm[a * 3 + b] = (L[a] * L[18]) * L[12 + b] + (L[6 + a] * L[18]) * L[15 + b];
}

PO_HD double max_nan(double a, double b) { return a != a ? a : b != b ? b : a < b ? b : a; }

// whether the edge reaches a free key frame that is in the system
template <int MUT>
PO_HD int free_of(const Ws& W, int e) {
  const int kf = W.e_kf[e];
  const int f = W.kf_free[kf];
  if (MUT == kMutFixedW && f < 0) return kf % W.F;  // a fixed key frame's W kept: it lands in some free key frame's rows
  return f;
}

// ---- the Schur pieces ------------------------------------------------------------------------------------------------------------------
// What does not depend on what a key frame's unknowns are, stated once for this core and navba_core.hpp: WS is either core's
// workspace, whose fields of one name have one meaning.  A mono edge's pose Jacobian is 2 x 6 in both.  No mutation lives in here: a
// core's switches stay at its call sites.

// shape 1: Hll's 6 entries and b_l of point j into H, stored with p_on.  Returns whether the point has an active edge.
template <class WS>
PO_HD bool point_sum(const WS& W, int j, double H[9]) {
  SIM3_UNROLL
  for (int k = 0; k < 9; ++k) H[k] = 0.;
  int on = 0;
  PO_NOUNROLL
  for (int e = W.pt_begin[j]; e < W.pt_begin[j + 1]; ++e) {
    if (W.e_off[e]) continue;
    on = 1;
    const double* L = W.e_lin + (size_t)e * kEdgeWords;
    int k = 0;
    SIM3_UNROLL
    for (int a = 0; a < 3; ++a)
      SIM3_UNROLL
      for (int b = a; b < 3; ++b, ++k) H[k] = H[k] + ((L[12 + a] * L[18]) * L[12 + b] + (L[15 + a] * L[18]) * L[15 + b]);
    SIM3_UNROLL
    for (int a = 0; a < 3; ++a) H[6 + a] = H[6 + a] + (L[12 + a] * L[19] + L[15 + a] * L[20]);
  }
  SIM3_UNROLL
  for (int k = 0; k < 9; ++k) W.Hll[9 * (size_t)j + k] = H[k];
  W.p_on[j] = (uint8_t)on;
  return on != 0;
}
PO_HD double point_maxdiag(const double H[9]) { return max_nan(max_nan(fabs(H[0]), fabs(H[3])), fabs(H[5])); }

// shape 2, lane l's share: entries l, l + 256, ... of the n edges listed from kl_edge[b0] onto the 21 + 6 sums
template <class WS>
PO_HD void kf_accumulate(const WS& W, int b0, int n, int l, double* acc) {
  PO_NOUNROLL
  for (int i = l; i < n; i += kLanes) {
    const int e = W.kl_edge[b0 + i];
    if (W.e_off[e]) continue;
    const double* L = W.e_lin + (size_t)e * kEdgeWords;
    int k = 0;
    SIM3_UNROLL
    for (int a = 0; a < 6; ++a)
      SIM3_UNROLL
      for (int b = a; b < 6; ++b, ++k) acc[k] = acc[k] + ((L[a] * L[18]) * L[b] + (L[6 + a] * L[18]) * L[6 + b]);
    SIM3_UNROLL
    for (int a = 0; a < 6; ++a) acc[21 + a] = acc[21 + a] + (L[a] * L[19] + L[6 + a] * L[20]);
  }
}

// Dinv = (Hll + lambda I)^-1 as the adjugate over the determinant, written out as Eigen's fixed-size inverse() is; Dinv b_l
template <class WS>
PO_HD void point_dinv(const WS& W, int j, double lambda) {
  const double* H = W.Hll + 9 * (size_t)j;
  const double m00 = H[0] + lambda, m01 = H[1], m02 = H[2], m11 = H[3] + lambda, m12 = H[4], m22 = H[5] + lambda;
  const double c00 = m11 * m22 - m12 * m12, c01 = m12 * m02 - m01 * m22, c02 = m01 * m12 - m11 * m02;
  const double c11 = m00 * m22 - m02 * m02, c12 = m01 * m02 - m00 * m12, c22 = m00 * m11 - m01 * m01;
  const double det = (m00 * c00 + m01 * c01) + m02 * c02;
  const double inv = 1. / det;
  double* D = W.Dinv + 9 * (size_t)j;
  D[0] = c00 * inv, D[1] = c01 * inv, D[2] = c02 * inv, D[3] = c11 * inv, D[4] = c12 * inv, D[5] = c22 * inv;
  D[6] = (D[0] * H[6] + D[1] * H[7]) + D[2] * H[8];
  D[7] = (D[1] * H[6] + D[3] * H[7]) + D[4] * H[8];
  D[8] = (D[2] * H[6] + D[4] * H[7]) + D[5] * H[8];
}

// Schur block blk is (i1, i2), i1 <= i2, in the order (0,0) (0,1) .. (0,F-1) (1,1) ..
PO_HD void block_of(int blk, int F, int* i1, int* i2) {
  int i = 0, rest = blk;
  while (rest >= F - i) rest -= F - i, ++i;
  *i1 = i, *i2 = i + rest;
}

PO_HD int tri6(int a, int b) {  // index of (a, b), a <= b, among the 21 upper entries
  int idx = 0;
  for (int r = 0; r < a; ++r) idx += 6 - r;
  return idx + (b - a);
}

// shape 3, lane l's share of block (i1, i2): the 36 sums of W_i1j Dinv_j W_i2j^T and, in a diagonal block, the 6 of W_i1j Dinv_j b_lj
template <class WS>
PO_HD void schur_accumulate(const WS& W, int i1, int i2, int l, double* acc) {
  const int b0 = W.kl_begin[i1], n = W.kl_begin[i1 + 1] - b0;
  const bool diag = i1 == i2;
  PO_NOUNROLL
  for (int i = l; i < n; i += kLanes) {
    const int e1 = W.kl_edge[b0 + i];
    if (W.e_off[e1]) continue;
    const int j = W.e_pt[e1];
    const int e2 = diag ? e1 : W.fp_edge[(size_t)i2 * W.P + j];
    if (e2 < 0 || W.e_off[e2]) continue;
    const double* D = W.Dinv + 9 * (size_t)j;
    double W1[18], Y[18];
    edge_W(W.e_lin + (size_t)e1 * kEdgeWords, W1);
    SIM3_UNROLL
    for (int a = 0; a < 6; ++a) {
      const double w0 = W1[a * 3], w1 = W1[a * 3 + 1], w2 = W1[a * 3 + 2];
      Y[a * 3] = (w0 * D[0] + w1 * D[1]) + w2 * D[2];
      Y[a * 3 + 1] = (w0 * D[1] + w1 * D[3]) + w2 * D[4];
      Y[a * 3 + 2] = (w0 * D[2] + w1 * D[4]) + w2 * D[5];
      if (diag) acc[36 + a] = acc[36 + a] + ((w0 * D[6] + w1 * D[7]) + w2 * D[8]);
    }
    double W2[18];
    edge_W(W.e_lin + (size_t)e2 * kEdgeWords, W2);
    SIM3_UNROLL
    for (int a = 0; a < 6; ++a)
      SIM3_UNROLL
      for (int b = 0; b < 6; ++b) acc[a * 6 + b] = acc[a * 6 + b] + ((Y[a * 3] * W2[b * 3] + Y[a * 3 + 1] * W2[b * 3 + 1]) + Y[a * 3 + 2] * W2[b * 3 + 2]);
  }
}

// shape 5: A x = b for the N x N system whose lower triangle is A, factorised in place; col and y are the team's two vectors of N words.
// Returns whether every pivot was finite and > 0; y holds x (whatever the pivots were).
template <class Team>
PO_HD bool ldlt_solve(Team& T, double* A, int N, const double* b, double* col, double* y) {
  bool ok = true;
  T.par(N, [&](int i) { y[i] = b[i]; });
  PO_NOUNROLL
  for (int k = 0; k < N; ++k) {
    const double dk = A[(size_t)k * N + k];
    ok = ok && dk > 0. && dk <= DBL_MAX;
    T.par(N - k - 1, [&](int r) {
      const int i = k + 1 + r;
      const double v = A[(size_t)i * N + k] / dk;
      A[(size_t)i * N + k] = v, col[i] = v;
    });
    T.par2(N - k - 1, N - k - 1, [&](int r, int c) {
      if (c > r) return;
      const int i = k + 1 + r, j = k + 1 + c;
      A[(size_t)i * N + j] = A[(size_t)i * N + j] - (col[i] * col[j]) * dk;
    });
  }
  PO_NOUNROLL
  for (int k = 0; k < N; ++k) {
    const double yk = y[k];
    T.par(N - k - 1, [&](int r) {
      const int i = k + 1 + r;
      y[i] = y[i] - A[(size_t)i * N + k] * yk;
    });
  }
  T.par(N, [&](int i) { y[i] = y[i] / A[(size_t)i * N + i]; });
  PO_NOUNROLL
  for (int k = N - 1; k >= 1; --k) {
    const double xk = y[k];
    T.par(k, [&](int i) { y[i] = y[i] - A[(size_t)k * N + i] * xk; });
  }
  return ok;
}

// Point j of the system: x_l = Dinv (b_l - W^T x_p) when the solve succeeded (else x_l keeps its value), X_try = X + x_l.  Returns the
// point's share of x . (lambda x + b).  step6(e, x) says whether edge e reaches a free key frame of the system and, if so, gives the six
// entries of x_p that belong to the edge's (dP, dPhi) or pose columns.
template <class WS, class Step6>
PO_HD double point_step(const WS& W, int j, bool ok, double lambda, Step6 step6) {
  double* xl = W.xl + 3 * (size_t)j;
  const double* H = W.Hll + 9 * (size_t)j;
  if (ok) {
    double c[3] = {H[6], H[7], H[8]};
    PO_NOUNROLL
    for (int e = W.pt_begin[j]; e < W.pt_begin[j + 1]; ++e) {
      if (W.e_off[e]) continue;
      double x[6];
      if (!step6(e, x)) continue;
      double Wm[18];
      edge_W(W.e_lin + (size_t)e * kEdgeWords, Wm);
      SIM3_UNROLL
      for (int b = 0; b < 3; ++b) {
        double t = Wm[b] * -x[0];
        SIM3_UNROLL
        for (int a = 1; a < 6; ++a) t = t + Wm[a * 3 + b] * -x[a];
        c[b] = c[b] + t;
      }
    }
    const double* D = W.Dinv + 9 * (size_t)j;
    xl[0] = (D[0] * c[0] + D[1] * c[1]) + D[2] * c[2];
    xl[1] = (D[1] * c[0] + D[3] * c[1]) + D[4] * c[2];
    xl[2] = (D[2] * c[0] + D[4] * c[1]) + D[5] * c[2];
  }
  double t = 0.;
  SIM3_UNROLL
  for (int b = 0; b < 3; ++b) {
    W.X_try[3 * (size_t)j + b] = W.X[3 * (size_t)j + b] + xl[b];
    t = t + xl[b] * (lambda * xl[b] + H[6 + b]);
  }
  return t;
}

// ---- the Levenberg driver's control block: the lead lane's parts of init, lin_ctl and trial_ctl -------------------------------------------
template <class WS>
PO_HD void ctl_reset(const WS& W) {
  Ctl& c = *W.ctl;
  c.lambda = 0., c.ni = 2., c.cur = 0., c.ini = 0., c.rho = 0.;
  c.round = -1, c.it = 0, c.q = 0, c.stalled = 0, c.status = 0, c.solve_ok = 0, c.n_lin = 0, c.n_trials = 0;
  c.its[0] = c.its[1] = 0;
  W.trace->n_lin = 0, W.trace->n_trials = 0;
}

// a linearisation with chi2 `chi` and largest diagonal entry `mx`: computeLambdaInit at the first iteration of an optimize(), the
// trace record, and on to the trials
template <class WS>
PO_HD void levenberg_linearised(const WS& W, double chi, double mx, int n_edges, int n_free, int n_points) {
  Ctl& c = *W.ctl;
  c.cur = chi, c.ini = chi;
  if (c.it == 0) c.lambda = 1e-5 * mx, c.ni = 2., c.stalled = 0;
  c.q = 0, c.rho = 0.;
  if (c.n_lin < kMaxLin) {
    TraceLin& r = W.trace->lin[c.n_lin];
    r.round = c.round, r.iteration = c.it, r.n_edges = n_edges, r.n_free = n_free, r.n_points = n_points, r.pad_ = 0;
    r.chi2 = chi, r.maxdiag = mx;
  }
  c.n_lin = c.n_lin + 1;
  W.trace->n_lin = c.n_lin;
  c.its[c.round] = c.its[c.round] + 1;
  c.status = kStTrial;
}

// a trial that started from (lambda, cur) and gave (ok, tmp, scale, rho): the trace record, lambda and ni, and what comes next
template <class WS>
PO_HD void levenberg_decide(const WS& W, double lambda, double cur, bool ok, double tmp, double scale, double rho, bool accept) {
  Ctl& c = *W.ctl;
  if (c.n_trials < kMaxTrialRecs) {
    poseopt::TraceTrial& r = W.trace->trial[c.n_trials];
    r.lin = c.n_lin - 1, r.ok = ok ? 1 : 0, r.accepted = accept ? 1 : 0, r.pad_ = 0;
    r.lambda = lambda, r.cur = cur, r.tmp = tmp, r.scale = scale;
  }
  c.n_trials = c.n_trials + 1;
  W.trace->n_trials = c.n_trials;
  double ni = c.ni, lam = lambda, now = cur;
  if (accept) {
    const double u = 2. * rho - 1.;
    double alpha = 1. - u * u * u;
    alpha = 2. / 3. < alpha ? 2. / 3. : alpha;
    const double sf = 1. / 3. < alpha ? alpha : 1. / 3.;
    lam = lam * sf, ni = 2., now = tmp;
  } else {
    lam = lam * ni, ni = ni * 2.;
  }
  const int q = c.q + 1;
  c.lambda = lam, c.ni = ni, c.cur = now, c.rho = rho, c.q = q;
  if (rho < 0. && q < kMaxTrials) {
    c.status = kStTrial;
  } else if (q == kMaxTrials || rho == 0.) {  // Terminate
    c.status = kStStop;
  } else {
    if ((c.ini - now) * 1e3 < c.ini) c.stalled = c.stalled + 1;
    else c.stalled = 0;
    c.status = c.stalled >= 3 ? kStStop : kStLinearise;
    c.it = c.it + 1;
  }
}

// ---- phases --------------------------------------------------------------------------------------------------------------------------
template <int MUT, class Team>
PO_HD void phase_init(const Ws& W, Team& T, int blk) {
  T.par(kLanes, [&](int l) {
    const int i = blk * kLanes + l;
    if (i < W.K) {
      float M[16];
      SIM3_UNROLL
      for (int k = 0; k < 12; ++k) M[k] = W.kf_T[12 * i + k];
      M[12] = M[13] = M[14] = 0.f, M[15] = 1.f;
      poseopt::pose_of(M, W.pose[i]);
      W.pose_try[i] = W.pose[i];
    }
    if (i < W.P) {
      SIM3_UNROLL
      for (int k = 0; k < 3; ++k) W.X[3 * (size_t)i + k] = W.X_try[3 * (size_t)i + k] = (double)W.pts[3 * (size_t)i + k];
    }
    if (i < W.E) W.e_off[i] = 0, W.e_chi2[i] = 0., W.removed1[i] = 0, W.removed2[i] = 0;
    if (i == 0) ctl_reset(W);
  });
}

// the start of an optimize(): lambda and ni are set anew (at its first linearisation), the step is zero, the estimates stay
template <int MUT, class Team>
PO_HD void phase_begin(const Ws& W, Team& T, int) {
  if (MUT != kMutStepIdle) {
    T.par(3 * W.P, [&](int i) { W.xl[i] = 0.; });
    T.par(6 * W.F, [&](int i) { W.xp[i] = 0.; });
  }
  if (MUT == kMutReturn) T.par(W.E, [&](int e) { W.e_off[e] = 0; });
  if (T.lead()) {
    Ctl& c = *W.ctl;
    c.round = c.round + 1, c.it = 0, c.status = kStLinearise;
  }
}

template <int MUT, class Team>
PO_HD void phase_edge_lin(const Ws& W, Team& T, int blk) {
  double s;
  T.template sum<1>(
      [&](int l, double* acc) {
        const int e = blk * kLanes + l;
        if (e < W.E && !W.e_off[e]) acc[0] = acc[0] + edge_linearise(W, e);
      },
      &s);
  const int n = T.count([&](int l) {
    const int e = blk * kLanes + l;
    return e < W.E && !W.e_off[e] ? 1 : 0;
  });
  if (T.lead()) W.chunk_chi2[blk] = s, W.chunk_n[blk] = n;
}

template <int MUT, class Team>
PO_HD void phase_point_sum(const Ws& W, Team& T, int blk) {
  const double mx = T.maxr([&](int l) {
    const int j = blk * kLanes + l;
    if (j >= W.P) return 0.;
    double H[9];
    point_sum(W, j, H);
    if (MUT == kMutTauPoses) return 0.;
    return point_maxdiag(H);
  });
  if (T.lead()) W.chunk_max[blk] = mx;
}

template <int MUT, class Team>
PO_HD void phase_kf_sum(const Ws& W, Team& T, int f) {
  const int b0 = W.kl_begin[f], n = W.kl_begin[f + 1] - b0;
  double S[27];
  T.template sum<27>([&](int l, double* acc) { kf_accumulate(W, b0, n, l, acc); }, S);
  const int on = T.count([&](int l) {
    int c = 0;
    for (int i = l; i < n; i += kLanes) c += W.e_off[W.kl_edge[b0 + i]] ? 0 : 1;
    return c;
  });
  if (T.lead()) {
    SIM3_UNROLL
    for (int k = 0; k < 27; ++k) W.Hpp[27 * f + k] = S[k];
    W.f_on[f] = on > 0 ? 1 : 0;
    const double dg[6] = {S[0], S[6], S[11], S[15], S[18], S[20]};
    double mx = 0.;
    SIM3_UNROLL
    for (int k = 0; k < 6; ++k) mx = max_nan(mx, fabs(dg[k]));
    W.chunk_max[chunks(W.P) + f] = mx;
  }
}

// computeActiveErrors' chi2, computeLambdaInit at the first iteration of an optimize()
template <int MUT, class Team>
PO_HD void phase_lin_ctl(const Ws& W, Team& T, int) {
  const int ce = chunks(W.E), cm = chunks(W.P) + W.F;
  const double mx = T.maxr([&](int l) {
    double m = 0.;
    for (int i = l; i < cm; i += kLanes) m = max_nan(m, W.chunk_max[i]);
    return m;
  });
  const int n_edges = T.count([&](int l) {
    int c = 0;
    for (int i = l; i < ce; i += kLanes) c += W.chunk_n[i];
    return c;
  });
  const int n_points = T.count([&](int l) {
    int c = 0;
    for (int i = l; i < W.P; i += kLanes) c += W.p_on[i];
    return c;
  });
  if (T.lead()) {
    Ctl& c = *W.ctl;
    if (n_edges == 0) {  // initializeOptimization() finds no vertex: optimize() returns at once
      c.status = kStStop;
    } else {
      double chi = 0.;
      PO_NOUNROLL
      for (int i = 0; i < ce; ++i) chi = chi + W.chunk_chi2[i];
      int nf = 0;
      for (int f = 0; f < W.F; ++f) nf += W.f_on[f];
      levenberg_linearised(W, chi, mx, n_edges, nf, n_points);
    }
  }
}

template <int MUT, class Team>
PO_HD void phase_dinv(const Ws& W, Team& T, int blk) {
  const double lambda = MUT == kMutLambdaPoseOnly || MUT == kMutDinvPlain ? 0. : W.ctl->lambda;
  T.par(kLanes, [&](int l) {
    const int j = blk * kLanes + l;
    if (j < W.P && W.p_on[j]) point_dinv(W, j, lambda);
  });
}

// block (i1, i2), i1 <= i2, of Hschur = Hpp + lambda I - sum_j W_i1j Dinv_j W_i2j^T, written to the lower triangle (transposed);
// the diagonal blocks also give bschur = b_p - sum_j W_ij Dinv_j b_lj
template <int MUT, class Team>
PO_HD void phase_schur(const Ws& W, Team& T, int blk) {
  int i1, i2;
  block_of(blk, W.F, &i1, &i2);
  const bool diag = i1 == i2;
  double* S = T.shared();
  T.template sum_shared<kSchurSums>([&](int l, double* acc) { schur_accumulate(W, i1, i2, l, acc); }, S);
  const int N = 6 * W.F;
  const double lambda = W.ctl->lambda;
  const bool on = W.f_on[i1] && W.f_on[i2];
  T.par(kSchurSums, [&](int k) {
    if (k < 36) {
      const int a = k / 6, b = k - 6 * a;
      if (diag && a > b) return;
      double v;
      if (!on) {
        v = diag && a == b ? 1. : 0.;  // a key frame without an active edge is outside the system: an identity row
      } else {
        double h = 0.;
        if (diag) {
          h = W.Hpp[27 * i1 + tri6(a, b)];
          if (a == b) h = h + lambda;
        }
        v = MUT == kMutSchurAdd ? h + S[k] : h - S[k];
      }
      W.Hs[(size_t)(6 * i2 + b) * N + (6 * i1 + a)] = v;
    } else if (diag) {
      const int a = k - 36;
      W.bs[6 * i1 + a] = on ? W.Hpp[27 * i1 + 21 + a] - S[k] : 0.;
    }
  });
}

// the pose solve and the key frames' oplus
template <int MUT, class Team>
PO_HD void phase_solve(const Ws& W, Team& T, int) {
  const int N = 6 * W.F;
  double* y = T.vec() + 6 * kMaxFree;  // [N]; T.vec(): [N] column k of L
  const bool ok = ldlt_solve(T, W.Hs, N, W.bs, T.vec(), y);
  if (ok) T.par(N, [&](int i) { W.xp[i] = y[i]; });
  // on a failed solve the step keeps its previous value and is applied all the same, as update(_solver->x()) is
  T.par(W.K, [&](int kf) {
    const int f = W.kf_free[kf];
    if (f >= 0 && (W.f_on[f] || MUT == kMutStepIdle)) poseopt::oplus(W.xp + 6 * f, W.pose[kf], W.pose_try[kf]);
    else W.pose_try[kf] = W.pose[kf];
  });
  if (T.lead()) W.ctl->solve_ok = ok ? 1 : 0;
}

// x_l = Dinv (b_l - W^T x_p), the point's oplus, its share of x . (lambda x + b)
template <int MUT, class Team>
PO_HD void phase_step(const Ws& W, Team& T, int blk) {
  const double lambda = W.ctl->lambda;
  const double lambda_l = MUT == kMutLambdaPoseOnly ? 0. : lambda;  // the mutation: the points never see lambda, here or in Dinv
  const bool ok = W.ctl->solve_ok != 0;
  double s;
  T.template sum<1>(
      [&](int l, double* acc) {
        const int j = blk * kLanes + l;
        if (j >= W.P) return;
        if (!W.p_on[j]) {
          // outside the system: it keeps its estimate (the mutation applies the step the last optimize() left)
          SIM3_UNROLL
          for (int b = 0; b < 3; ++b) W.X_try[3 * (size_t)j + b] = MUT == kMutStepIdle ? W.X[3 * (size_t)j + b] + W.xl[3 * (size_t)j + b] : W.X[3 * (size_t)j + b];
          return;
        }
        acc[0] = acc[0] + point_step(W, j, ok, lambda_l, [&](int e, double* x) {
          const int f = free_of<MUT>(W, e);
          if (MUT == kMutNoWx || f < 0 || !W.f_on[f]) return false;
          SIM3_UNROLL
          for (int a = 0; a < 6; ++a) x[a] = W.xp[6 * f + a];
          return true;
        });
      },
      &s);
  if (T.lead()) W.chunk_scale[blk] = s;
}

template <int MUT, class Team>
PO_HD void phase_edge_err(const Ws& W, Team& T, int blk) {
  double s;
  T.template sum<1>(
      [&](int l, double* acc) {
        const int e = blk * kLanes + l;
        if (e >= W.E || W.e_off[e]) return;
        poseopt::EdgeEval E;
        poseopt::Cam C;
        edge_error(W, e, W.pose_try, W.X_try, E, C);
        W.e_chi2[e] = E.chi2;
        double rho0, rho1;
        poseopt::huber(E.chi2, &rho0, &rho1);
        acc[0] = acc[0] + rho0;
      },
      &s);
  if (T.lead()) W.chunk_chi2[blk] = s;
}

// the Levenberg decision of one trial
template <int MUT, class Team>
PO_HD void phase_trial_ctl(const Ws& W, Team& T, int) {
  Ctl& c = *W.ctl;
  const int ce = chunks(W.E), cp = chunks(W.P);
  const double lambda = c.lambda, cur = c.cur;
  const bool ok = c.solve_ok != 0;
  double tmp = 0.;
  PO_NOUNROLL
  for (int i = 0; i < ce; ++i) tmp = tmp + W.chunk_chi2[i];
  if (!ok) tmp = DBL_MAX;
  double scale = 0.;
  PO_NOUNROLL
  for (int f = 0; f < W.F; ++f) {
    if (!W.f_on[f]) continue;
    for (int a = 0; a < 6; ++a) scale = scale + W.xp[6 * f + a] * (lambda * W.xp[6 * f + a] + W.Hpp[27 * f + 21 + a]);
  }
  PO_NOUNROLL
  for (int i = 0; i < cp; ++i) scale = scale + W.chunk_scale[i];
  scale = scale + 1e-3;
  const double rho = (cur - tmp) / scale;
  const bool accept = rho > 0. && fabs(tmp) <= DBL_MAX;
  T.par(0, [&](int) {});  // every lane has read the control block before the lead rewrites it
  if (accept) {
    T.par(W.K, [&](int i) { W.pose[i] = W.pose_try[i]; });
    T.par(3 * W.P, [&](int i) { W.X[i] = W.X_try[i]; });
  } else if (MUT == kMutReeval) {
    // the stored error re-evaluated after a rejected trial: chi2 of the restored estimates
    T.par(W.E, [&](int e) {
      if (W.e_off[e]) return;
      poseopt::EdgeEval E;
      poseopt::Cam C;
      edge_error(W, e, W.pose, W.X, E, C);
      W.e_chi2[e] = E.chi2;
    });
  }
  if (T.lead()) levenberg_decide(W, lambda, cur, ok, tmp, scale, rho, accept);
}

// chi2() > 5.991 || !isDepthPositive(): chi2 of the stored error, the depth at the current estimates; edges of points flagged bad are
// not examined; a bad edge is removed for good
template <int MUT, class Team>
PO_HD void phase_check(const Ws& W, Team& T, int blk) {
  const int round = W.ctl->round;
  T.par(kLanes, [&](int l) {
    const int e = blk * kLanes + l;
    if (e >= W.E || W.e_off[e] || W.pt_bad[W.e_pt[e]]) return;
    poseopt::EdgeEval E;
    poseopt::Cam C;
    edge_error(W, e, W.pose, W.X, E, C);
    const bool bad = W.e_chi2[e] > 5.991 || !(E.z > 0.);
    if (!bad) return;
    (round == 0 ? W.removed1 : W.removed2)[e] = 1;
    W.e_off[e] = 1;
  });
}

template <int MUT, class Team>
PO_HD void phase_finish(const Ws& W, Team& T, int blk) {
  T.par(kLanes, [&](int l) {
    const int i = blk * kLanes + l;
    if (i < W.K) {
      const Pose& P = W.pose[i];
      double R[9];
      poseopt::matrix_of(P, W.kf_T_out + 16 * i, R);
      SIM3_UNROLL
      for (int k = 0; k < 4; ++k) W.kf_est[7 * i + k] = P.q[k];
      SIM3_UNROLL
      for (int k = 0; k < 3; ++k) W.kf_est[7 * i + 4 + k] = P.t[k];
    }
    if (i < W.P) {
      SIM3_UNROLL
      for (int k = 0; k < 3; ++k) W.pt_est[3 * (size_t)i + k] = W.X[3 * (size_t)i + k], W.pt_out[3 * (size_t)i + k] = (float)W.X[3 * (size_t)i + k];
    }
  });
}

template <int MUT, class Team>
PO_HD void run_phase(int ph, const Ws& W, Team& T, int blk) {
  switch (ph) {
    case kInit: phase_init<MUT>(W, T, blk); break;
    case kBegin: phase_begin<MUT>(W, T, blk); break;
    case kEdgeLin: phase_edge_lin<MUT>(W, T, blk); break;
    case kPointSum: phase_point_sum<MUT>(W, T, blk); break;
    case kKfSum: phase_kf_sum<MUT>(W, T, blk); break;
    case kLinCtl: phase_lin_ctl<MUT>(W, T, blk); break;
    case kDinv: phase_dinv<MUT>(W, T, blk); break;
    case kSchur: phase_schur<MUT>(W, T, blk); break;
    case kSolve: phase_solve<MUT>(W, T, blk); break;
    case kStep: phase_step<MUT>(W, T, blk); break;
    case kEdgeErr: phase_edge_err<MUT>(W, T, blk); break;
    case kTrialCtl: phase_trial_ctl<MUT>(W, T, blk); break;
    case kCheck: phase_check<MUT>(W, T, blk); break;
    default: phase_finish<MUT>(W, T, blk); break;
  }
}

// ---- host side: the launch sequence, and what the upload derives from the caller's lists ------------------------------------------------
struct Dims {
  int K, F, P, E;
};

// X.launch(phase, blocks) queues a phase; X.status(&st) waits for what is queued and reads the status word.  Both return 0 or an error
// code, after which nothing more is launched.  The loop is bounded by rounds x iterations x 10 trials.  *syncs counts the status reads.
template <class X>
int drive(X& x, const Dims& d, int mode, int n_iterations, int* syncs) {
  const int ce = chunks(d.E), cp = chunks(d.P);
  int rc = x.launch(kInit, chunks(d.K > d.P ? (d.K > d.E ? d.K : d.E) : (d.P > d.E ? d.P : d.E)));
  const int rounds = mode == kModeLocal ? 2 : 1;
  for (int round = 0; round < rounds && !rc; ++round) {
    const int its = mode == kModeLocal ? (round == 0 ? 5 : 10) : n_iterations;
    rc = x.launch(kBegin, 1);
    int st = kStLinearise;
    for (int it = 0; it < its && !rc && st == kStLinearise; ++it) {
      if (!rc) rc = x.launch(kEdgeLin, ce);
      if (!rc) rc = x.launch(kPointSum, cp);
      if (!rc) rc = x.launch(kKfSum, d.F);
      if (!rc) rc = x.launch(kLinCtl, 1);
      st = kStTrial;
      if (it == 0 && !rc) rc = x.status(&st), ++*syncs;
      for (int trial = 0; trial < kMaxTrials && !rc && st == kStTrial; ++trial) {
        if (!rc) rc = x.launch(kDinv, cp);
        if (!rc) rc = x.launch(kSchur, schur_blocks(d.F));
        if (!rc) rc = x.launch(kSolve, 1);
        if (!rc) rc = x.launch(kStep, cp);
        if (!rc) rc = x.launch(kEdgeErr, ce);
        if (!rc) rc = x.launch(kTrialCtl, 1);
        if (!rc) rc = x.status(&st), ++*syncs;
      }
      if (st == kStTrial) st = kStStop;  // cannot happen: the tenth trial never asks for another
    }
    if (mode == kModeLocal && !rc) rc = x.launch(kCheck, ce);
  }
  if (!rc) rc = x.launch(kFinish, chunks(d.K > d.P ? d.K : d.P));
  return rc;
}

// What the upload derives from the caller's lists (integer work, g2o's buildStructure): the free key frames' numbering in key-frame
// order, every edge's point, the free key frames' edge lists in ascending edge index, the table (free key frame, point) -> edge.
// Returns 0, or 1 when there are more than kMaxFree free key frames, an edge names a key frame or a camera out of range, the
// point_edge_begin list is not ascending from 0 to E, or a point has two edges to one free key frame.  fp_edge has F x P entries.
inline int derive(int K, const uint8_t* fixed, int P, const int32_t* pt_begin, int E, const int32_t* e_kf, const int32_t* e_cam, int C, int32_t* kf_free,
                  int32_t* free_kf, int* F_out, int32_t* e_pt, int32_t* kl_begin, int32_t* kl_edge, int32_t* fp_edge) {
  int F = 0;
  for (int k = 0; k < K; ++k) F += fixed[k] ? 0 : 1;
  if (F > kMaxFree) return 1;
  F = 0;
  for (int k = 0; k < K; ++k) {
    kf_free[k] = fixed[k] ? -1 : F;
    if (!fixed[k]) free_kf[F++] = k;
  }
  *F_out = F;
  if (pt_begin[0] != 0 || pt_begin[P] != E) return 1;
  for (int j = 0; j < P; ++j)
    if (pt_begin[j + 1] < pt_begin[j] || pt_begin[j + 1] > E) return 1;
  for (int f = 0; f <= F; ++f) kl_begin[f] = 0;
  for (int e = 0; e < E; ++e) {
    if (e_kf[e] < 0 || e_kf[e] >= K || e_cam[e] < 0 || e_cam[e] >= C) return 1;
    const int f = kf_free[e_kf[e]];
    if (f >= 0) ++kl_begin[f + 1];
  }
  for (int f = 0; f < F; ++f) kl_begin[f + 1] += kl_begin[f];
  for (size_t i = 0; i < (size_t)F * (size_t)P; ++i) fp_edge[i] = -1;
  int32_t fill[kMaxFree];
  for (int f = 0; f < F; ++f) fill[f] = kl_begin[f];
  for (int j = 0; j < P; ++j)
    for (int e = pt_begin[j]; e < pt_begin[j + 1]; ++e) {
      e_pt[e] = j;
      const int f = kf_free[e_kf[e]];
      if (f < 0) continue;
      kl_edge[fill[f]++] = e;
      int32_t& slot = fp_edge[(size_t)f * (size_t)P + j];
      if (slot >= 0) return 1;
      slot = e;
    }
  return 0;
}

// the host's team, of this core and of navba_core.hpp: lane_team.hpp's walk of the reduction shape, one thread that plays lanes
// 0..255 in turn
#if !defined(__HIP_DEVICE_COMPILE__)
struct HostTeam : HostLaneTeam<kSchurSums> {
  double v[2 * 6 * kMaxFree];  // the solve's two vectors; navba_core.hpp asserts that its own fit
  double* vec() { return v; }
  template <class F>
  double maxr(F f) {
    double m = f(0);
    for (int l = 1; l < kLanes; ++l) m = max_nan(m, f(l));
    return m;
  }
  template <class F>
  void par(int n, F f) {
    for (int i = 0; i < n; ++i) f(i);
  }
  template <class F>
  void each(int n, F f) {  // navopt_core.hpp's name for par
    par(n, f);
  }
  template <class F>
  void par2(int rows, int cols, F f) {
    for (int r = 0; r < rows; ++r)
      for (int c = 0; c < cols; ++c) f(r, c);
  }
};
#endif

}  // namespace ba
}  // namespace uvo
