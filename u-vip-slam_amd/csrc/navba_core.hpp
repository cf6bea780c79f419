// Optimizer::LocalBundleAdjustmentNavState (src/Optimizer.cc:1105-1732 of the reference) with the parts of src/IMU/g2otypes.{h,cpp},
// NavState.cpp, so3.cpp and g2o it runs: a window of key frames with 15 unknowns each (VertexNavStatePVR dP dV dPhi, VertexNavStateBias
// dbg dba), chained by EdgeNavStatePVR and EdgeNavStateBias, with EdgeNavStateDepthProjected entries, under marginalised points seen
// through EdgeNavStatePVRPointXYZ.  It joins ba_core.hpp (points eliminated, the Schur complement rebuilt per trial, the dense LDL^T,
// the Levenberg driver as launches) and navopt_core.hpp (NavState, SO3, the inertial edges) BY CALLING THEM: the per-point and
// per-key-frame sums, Dinv, the Schur block's sums, the solve, the point back-substitution and the Levenberg bookkeeping are
// ba_core.hpp's "Schur pieces", stated there once; this file owns the mono edge through the NavState camera, the inertial edges,
// inert_lin / inert_add / inert_err, the 15-block scatter, hdiag, bfull and the two checks.  Plain C++ in
// double under poseopt_core.hpp's rules: IEEE + - * / sqrt fabs only, no contraction, no library function.  navba.hip runs this on the
// device, tests/emu/navba_emu.cpp on the host; the two are held to each other bit for bit.
//
// PHASES as in ba_core.hpp: a phase is a function of (workspace, team, block); the device launches one kernel per phase with one
// workgroup of 256 lanes per block.  drive() below decides which run; lin_ctl and trial_ctl make the Levenberg decision and leave a
// status word.
//
// THE REDUCED SYSTEM is 15F x 15F: free key frames in the caller's order, PVR (columns 0..8) before bias (9..14) in each.  A mono edge
// touches only dP and dPhi of its key frame, so its pose Jacobian is 2 x 6 and everything ba_core.hpp does per edge, per point, per
// key frame (21 + 6 sums, shape 2) and per Schur block (36 + 6 sums, shape 3) keeps its shape; a 6 x 6 block lands in rows and columns
// {0,1,2,6,7,8} of the two 15-blocks.
//
// THE INERTIAL EDGES are few (two per link, and the depth entries).  Edge g is: g < 2L: link g / 2, its EdgeNavStatePVR (g even) or
// its EdgeNavStateBias (g odd); else depth entry g - 2L.  inert_lin gives EACH EDGE A LANE: the lane writes the error and a dense
// Jacobian J[m][30] to global memory (m = 9, 6, 1 rows; columns: slot A 0..8 the first PVR vertex, B 9..17 the second, C 18..23 the first
// bias vertex, D 24..29 the second), then the block's lanes share out WJ = (rho1 Omega) J and We = (rho1 Omega) e entry by entry, each
// a sum over s ascending.  inert_add gives each entry (r >= c) of a 15-block pair a lane, which adds onto what schur left
//     sum over the edges g ASCENDING (so: a link's PVR edge, its bias edge, the next link's ..., then the depth entries in list order),
//     each over its rows ascending, of J[row][c] * WJ[row][r]
// and onto b the same with We, subtracted.  Each entry is written by exactly one lane.  No floating-point atomics anywhere.
// The chi2 of a linearisation or a trial is ba_core.hpp's shape 4 over the mono edges, then rho0 of the inertial edges added in
// ascending g.  Lambda's tau x max-diagonal runs over the 15-blocks' diagonal (mono sum + the inertial terms in the order above) and
// the points.  The solve is ba_core.hpp's shape 5 at n = 15F <= 360.
//
// The first check takes the kernel off every mono edge of an unflagged point and puts the edges with chi2 > 5.991 (in double) or
// a non-positive depth at level 1 (`excluded`); the final check runs over all mono edges of unflagged points, excluded ones too, on
// the stored chi2 (for an excluded edge: what round one's last evaluation left) and the depth at the final estimates (`erased`).
//
// Departures from the reference (uvo.h): those of ba_core.hpp and navopt_core.hpp; a free key frame is always
// in the system (a link ends in it); the information of a depth entry is the caller's scalar.
#pragma once
#include "ba_core.hpp"
#include "navopt_core.hpp"

namespace uvo {
namespace navba {

using navopt::State;
using poseopt::kLanes;
using ba::chunks;
using ba::max_nan;
using ba::schur_blocks;
using ba::tri6;

constexpr int kMaxFree = 24, kMaxFixed = 256, kMaxPoints = 32768, kMaxEdges = 262144, kMaxCams = 64, kMaxDepth = 256;
constexpr int kMaxLinks = 2 * kMaxFree;        // one per window key frame, the ones fixed by fixedKF_id included
constexpr int kMaxTrials = ba::kMaxTrials;
constexpr int kMaxLin = ba::kMaxLin, kMaxTrialRecs = ba::kMaxTrialRecs;
constexpr int kSchurSums = ba::kSchurSums, kEdgeWords = ba::kEdgeWords;
constexpr int kJ = 30;                           // columns of an inertial edge's Jacobian
constexpr int kIeJ = 0, kIeWJ = 9 * kJ, kIeE = 2 * 9 * kJ, kIeWe = kIeE + 9, kIeChi = kIeWe + 9, kIeWords = kIeChi + 4;  // chi2 rho0 rho1

// seeded mutations, for the host build only (tests/emu/navba_emu.cpp); the library instantiates MUT = 0
constexpr int kMutNone = 0, kMutVCols = 1, kMutScatter05 = 2, kMutBackPre = 3, kMutCheckFloat = 4, kMutKeepKernel = 5, kMutFlaggedOff = 6,
              kMutFinalSkip = 7, kMutOrder = 8, kMutBiasNoDt = 9, kMutTauPoses = 10;

enum Phase { kInit = 0, kBegin, kEdgeLin, kInertLin, kPointSum, kKfSum, kLinCtl, kDinv, kSchur, kInertAdd, kSolve, kStep, kEdgeErr, kInertErr,
             kTrialCtl, kCheck, kFinish, kPhases };
constexpr int kStTrial = ba::kStTrial, kStLinearise = ba::kStLinearise, kStStop = ba::kStStop;

using TraceLin = ba::TraceLin;   // n_edges counts the inertial edges too; n_free is F
using Trace = ba::Trace;
using Ctl = ba::Ctl;

struct Link {    // one inertial link: kf1's preintegration, measured from kf0
  int32_t kf0, kf1;
  double dT, dP[3], dV[3], dR[9], JPg[9], JPa[9], JVg[9], JVa[9], JRg[9], cov[81];
};
struct Depth {   // one EdgeNavStateDepthProjected: vertices PVR(ka), PVR(kb), Bias(kc); the preintegration of `link`
  int32_t ka, kb, kc, link;
  double shi, meas, info;
};
struct Params {
  double Rbc[9], Pbc[3], gw[3], gyr_rw2, acc_rw2;
};

struct Ws {
  int32_t K, F, P, E, C, L, D, pad_;
  // the upload
  const State* kf_in;       // [K]
  const int32_t* kf_free;   // [K] index among the free key frames, -1: fixed
  const uint8_t* kf_bias;   // [K] carries a bias vertex
  const int32_t* free_kf;   // [F]
  const float* pts;         // [P][3]
  const uint8_t* pt_bad;    // [P]
  const int32_t* pt_begin;  // [P + 1]
  const int32_t* e_kf;      // [E]
  const int32_t* e_pt;      // [E]
  const int32_t* e_cam;     // [E]
  const float* e_obs;       // [E][3]: x y invSigma2
  const float* cams;        // [C][4]
  const int32_t* kl_begin;  // [F + 1]
  const int32_t* kl_edge;   // [<= E]
  const int32_t* fp_edge;   // [F][P]
  const Link* links;        // [L]
  const Depth* depths;      // [D]
  const Params* prm;
  // state
  State *ns, *ns_try;       // [K]
  double *cam, *cam_try;    // [K][12]: Rcb Rwb^T, Pwb
  double* camc;             // [3]: Rcb Pbc
  double *X, *X_try;        // [P][3]
  uint8_t* e_off;           // [E] 1: at level 1
  uint8_t* e_rob;           // [E] 1: carries the Huber kernel
  double* e_chi2;           // [E] chi2 of the stored error
  double* e_lin;            // [E][kEdgeWords]
  double *Hll, *Dinv;       // [P][9]
  uint8_t* p_on;            // [P]
  double* Hpp;              // [F][27] the mono edges' 21 + 6 sums over (dP, dPhi)
  double* hdiag;            // [15F] the diagonal of the 15-blocks before lambda
  double* link_info;        // [L][81] inverse of CovPVPhi
  double* ie_lin;           // [2L + D][kIeWords]
  int32_t* ie_col;          // [2L + D][4] column of the slot's vertex in the reduced system, -1: fixed or unused
  double* ie_try;           // [2L + D] rho0 at the tried estimates
  double* ie_etry;          // [2L + D][9] the error there
  double* Hs;               // [15F][15F], the lower triangle
  double *bs, *bfull, *xp;  // [15F]; bfull: b before the points' correction
  double* xl;               // [P][3]
  double *chunk_chi2, *chunk_scale, *chunk_max;  // [chunks of E], [chunks of P], [chunks of P + F]
  int32_t* chunk_n;         // [chunks of E]
  Ctl* ctl;
  Trace* trace;
  uint8_t *excluded, *erased;  // [E]
  // the download
  State* kf_out;            // [K]
  float* kf_T_out;          // [K][16]
  double* pt_est;           // [P][3]
  float* pt_out;            // [P][3]
};

PO_HD int n_inert(const Ws& W) { return 2 * W.L + W.D; }

// ---- the Hessian's columns --------------------------------------------------------------------------------------------------------------
template <int MUT>
PO_HD int col_pvr(int f) { return MUT == kMutOrder ? 15 * f + 6 : 15 * f; }
template <int MUT>
PO_HD int col_bias(int f) { return MUT == kMutOrder ? 15 * f : 15 * f + 9; }
// entry a of a mono edge's (dP, dPhi) inside the PVR vertex's 9
template <int MUT>
PO_HD int pvr_of6(int a) { return MUT == kMutScatter05 ? a : a < 3 ? a : a + 3; }
// the (dP, dPhi) entry that column a of a 15-block is, -1: none
template <int MUT>
PO_HD int mono_of(int a) {
  const int p = a - col_pvr<MUT>(0);
  if (p < 0 || p >= 9) return -1;
  if (MUT == kMutScatter05) return p < 6 ? p : -1;
  return p < 3 ? p : p >= 6 ? p - 3 : -1;
}

// ---- EdgeNavStatePVRPointXYZ g2otypes.h:207-281, g2otypes.cpp:394-449 ------------------------------------------------------------------
struct MonoEval {
  double a[3];      // Paux = Rcb Rwb^T (Pw - Pwb)
  double x, y, z;   // Pc
  double e0, e1, w, chi2;
  double fx, fy;
};
// cam: Rcb Rwb^T (9), Pwb (3) of the edge's key frame
PO_HD void mono_error(const Ws& W, int e, const double* cams, const double* X, MonoEval& E) {
  const double* cam = cams + 12 * W.e_kf[e];
  const double* x = X + 3 * (size_t)W.e_pt[e];
  const double d[3] = {x[0] - cam[9], x[1] - cam[10], x[2] - cam[11]};
  navopt::mat3_vec(cam, d, E.a);
  E.x = E.a[0] - W.camc[0], E.y = E.a[1] - W.camc[1], E.z = E.a[2] - W.camc[2];
  const float* c = W.cams + 4 * W.e_cam[e];
  E.fx = (double)c[0], E.fy = (double)c[1];
  const float* o = W.e_obs + 3 * (size_t)e;
  E.e0 = (double)o[0] - ((E.x / E.z) * E.fx + (double)c[2]);
  E.e1 = (double)o[1] - ((E.y / E.z) * E.fy + (double)c[3]);
  E.w = (double)o[2];
  E.chi2 = E.e0 * (E.w * E.e0 + 0. * E.e1) + E.e1 * (0. * E.e0 + E.w * E.e1);
}

// linearizeOplus and the robustified weights, in ba_core.hpp's words: Jp[2][6] over (dP, dPhi), Jl[2][3], wo, r0, r1, rho0
PO_HD double mono_linearise(const Ws& W, int e) {
  MonoEval E;
  mono_error(W, e, W.cam, W.X, E);
  W.e_chi2[e] = E.chi2;
  double rho0, rho1;
  navopt::robustify(E.chi2, navopt::kDeltaMono, W.e_rob[e] != 0, &rho0, &rho1);
  double* L = W.e_lin + (size_t)e * kEdgeWords;
  const double x = E.x, y = E.y, z = E.z;
  // -Jpi, Jpi = Maux / z
  const double m00 = -(E.fx / z), m02 = -((-x / z * E.fx) / z), m11 = -(E.fy / z), m12 = -((-y / z * E.fy) / z);
  const double* a = E.a;
  const double* B = W.prm->Rbc;  // Rcb[i][j] = B[j * 3 + i]
  const double* M = W.cam + 12 * W.e_kf[e];
  SIM3_UNROLL
  for (int j = 0; j < 3; ++j) {
    const double c0 = B[j * 3], c1 = B[j * 3 + 1], c2 = B[j * 3 + 2];  // column j of Rcb
    // JdPwb = -Jpi (-Rcb)
    L[j] = m00 * -c0 + m02 * -c2;
    L[6 + j] = m11 * -c1 + m12 * -c2;
    // JdRwb = -Jpi (hat(Paux) Rcb)
    const double h0 = a[1] * c2 - a[2] * c1, h1 = a[2] * c0 - a[0] * c2, h2 = a[0] * c1 - a[1] * c0;
    L[3 + j] = m00 * h0 + m02 * h2;
    L[9 + j] = m11 * h1 + m12 * h2;
    // _jacobianOplusXi = -Jpi Rcb Rwb^T
    L[12 + j] = m00 * M[j] + m02 * M[6 + j];
    L[15 + j] = m11 * M[3 + j] + m12 * M[6 + j];
  }
  L[18] = rho1 * E.w;
  L[19] = -(E.w * E.e0) * rho1, L[20] = -(E.w * E.e1) * rho1;
  L[21] = rho0;
  return rho0;
}

// ---- the inertial edges ---------------------------------------------------------------------------------------------------------------------
PO_HD int ie_rows(const Ws& W, int g) { return g >= 2 * W.L ? 1 : (g & 1) ? 6 : 9; }

// information of edge g, entry (r, s)
template <int MUT>
PO_HD double ie_info(const Ws& W, int g, int r, int s) {
  if (g >= 2 * W.L) return W.depths[g - 2 * W.L].info;
  if (!(g & 1)) return W.link_info[81 * (g >> 1) + r * 9 + s];
  const double dT = MUT == kMutBiasNoDt ? 1. : W.links[g >> 1].dT;
  return r == s ? (1. / (r < 3 ? W.prm->gyr_rw2 : W.prm->acc_rw2)) / dT : 0. / dT;
}

// EdgeNavStatePVR g2otypes.cpp:8-213: vertex 0 PVR(kf0) slot A, vertex 1 PVR(kf1) slot B, vertex 2 Bias(kf0) slot C
template <int MUT>
PO_HD void edge_pvr(const Ws& W, int l, const State* S, double* e, double* J) {
  const Link& p = W.links[l];
  const State& si = S[p.kf0];
  const State& sj = S[p.kf1];
  const double dT = p.dT, dT2 = dT * dT;
  const double* gw = W.prm->gw;
  double RiT[4], u[3], v[3], cP[3], cV[3], r[3];
  navopt::q_inv(si.q, RiT);
  for (int i = 0; i < 3; ++i) {
    u[i] = ((sj.P[i] - si.P[i]) - si.V[i] * dT) - (0.5 * gw[i]) * dT2;
    v[i] = (sj.V[i] - si.V[i]) - gw[i] * dT;
  }
  navopt::corrected(p.dP, p.JPg, p.JPa, si, cP);
  navopt::corrected(p.dV, p.JVg, p.JVa, si, cV);
  poseopt::rotate(RiT, u[0], u[1], u[2], r);
  for (int i = 0; i < 3; ++i) e[i] = r[i] - cP[i];
  poseopt::rotate(RiT, v[0], v[1], v[2], r);
  for (int i = 0; i < 3; ++i) e[3 + i] = r[i] - cV[i];
  double jb[3], qd[4], qb[4], qdb[4], qdi[4], t[4], rR[4], er[3];
  navopt::mat3_vec(p.JRg, si.dbg, jb);
  navopt::so3_exp(jb, qb);
  navopt::q_of_matrix(p.dR, qd);
  navopt::q_mul(qd, qb, qdb);
  navopt::q_inv(qdb, qdi);
  navopt::q_mul(qdi, RiT, t);
  navopt::q_mul(t, sj.q, rR);
  navopt::so3_log(rR, er);
  for (int i = 0; i < 3; ++i) e[6 + i] = er[i];
  if (!J) return;
  double Ri[9], Rj[9], RiTm[9], RjT[9], Ji[9], B[9], Cm[9], hu[3], hv[3];
  poseopt::rotation_of(si.q, Ri);
  poseopt::rotation_of(sj.q, Rj);
  navopt::mat3_t(Ri, RiTm);
  navopt::mat3_t(Rj, RjT);
  navopt::so3_jrinv<0>(er, Ji);
  const double I[9] = {1., 0., 0., 0., 1., 0., 0., 0., 1.};
  // vertex 1
  navopt::mat3_mul(RiTm, Rj, B);
  navopt::put3(J, 0, 9, B, 1.);
  navopt::put3(J, 3, 12, RiTm, 1.);
  navopt::put3(J, 6, 15, Ji, 1.);
  // vertex 0
  navopt::put3(J, 0, 0, I, -1.);
  for (int k = 0; k < 9; ++k) B[k] = RiTm[k] * dT;
  navopt::put3(J, 0, 3, B, -1.);
  navopt::mat3_vec(RiTm, u, hu);
  navopt::hat(hu, B);
  navopt::put3(J, 0, 6, B, 1.);
  navopt::put3(J, 3, 3, RiTm, -1.);
  navopt::mat3_vec(RiTm, v, hv);
  navopt::hat(hv, B);
  navopt::put3(J, 3, 6, B, 1.);
  for (int k = 0; k < 9; ++k) Cm[k] = -Ji[k];
  navopt::mat3_mul(Cm, RjT, B);
  navopt::mat3_mul(B, Ri, Cm);
  navopt::put3(J, 6, 6, Cm, 1.);
  // vertex 2
  navopt::put3(J, 0, 18, p.JPg, -1.);
  navopt::put3(J, 0, 21, p.JPa, -1.);
  navopt::put3(J, 3, 18, p.JVg, -1.);
  navopt::put3(J, 3, 21, p.JVa, -1.);
  double qe[4], qei[4], Et[9], Jr[9];
  navopt::so3_exp(er, qe);
  navopt::q_inv(qe, qei);
  poseopt::rotation_of(qei, Et);
  navopt::so3_jr(jb, Jr);
  for (int k = 0; k < 9; ++k) Cm[k] = -Ji[k];
  navopt::mat3_mul(Cm, Et, B);
  navopt::mat3_mul(B, Jr, Cm);
  navopt::mat3_mul(Cm, p.JRg, B);
  navopt::put3(J, 6, 18, B, 1.);
}

// EdgeNavStateBias g2otypes.cpp:215-263: vertex 0 Bias(kf0) slot C, vertex 1 Bias(kf1) slot D
PO_HD void edge_bias(const Ws& W, int l, const State* S, double* e, double* J) {
  const Link& p = W.links[l];
  const State& si = S[p.kf0];
  const State& sj = S[p.kf1];
  for (int i = 0; i < 3; ++i) e[i] = (sj.bg[i] + sj.dbg[i]) - (si.bg[i] + si.dbg[i]), e[3 + i] = (sj.ba[i] + sj.dba[i]) - (si.ba[i] + si.dba[i]);
  if (!J) return;
  for (int i = 0; i < 6; ++i) J[i * kJ + 18 + i] = -1., J[i * kJ + 24 + i] = 1.;
}

// EdgeNavStateDepthProjected g2otypes.cpp:292-392: vertex 0 PVR(ka) slot A, vertex 1 PVR(kb) slot B, vertex 2 Bias(kc) slot C
PO_HD void edge_depth(const Ws& W, int d, const State* S, double* e, double* J) {
  const Depth& q = W.depths[d];
  const Link& p = W.links[q.link];
  const State& s0 = S[q.ka];
  const State& s1 = S[q.kb];
  const State& sb = S[q.kc];
  const double dT = p.dT, dT2 = dT * dT;
  const double proj = q.shi * (q.meas - s0.P[2]) + s0.P[2];
  const double r1 = proj - s1.P[2];
  double R0[9], c[3], Rc[3], kf[3];
  poseopt::rotation_of(s0.q, R0);
  navopt::corrected(p.dP, p.JPg, p.JPa, sb, c);
  navopt::mat3_vec(R0, c, Rc);
  const double G[3] = {0., 0., 9.81};
  for (int i = 0; i < 3; ++i) kf[i] = ((s0.P[i] + dT * s0.V[i]) + dT2 * G[i]) + Rc[i];
  const double r2 = proj - kf[2];
  e[0] = r1 + r2;
  if (!J) return;
  J[2] = 2. * (1. - q.shi) - 1.;
  J[5] = -dT;
  J[6] = Rc[1], J[7] = -Rc[0], J[8] = 0.;
  J[9 + 2] = -1.;
  double nR[9], Bg[9], Ba[9];
  for (int k = 0; k < 9; ++k) nR[k] = -R0[k];
  navopt::mat3_mul(nR, p.JPg, Bg);
  navopt::mat3_mul(nR, p.JPa, Ba);
  for (int k = 0; k < 3; ++k) J[18 + k] = Bg[k * 3 + 2], J[21 + k] = Ba[k * 3 + 2];
}

PO_HD double ie_delta(const Ws& W, int g) { return g >= 2 * W.L ? navopt::kDeltaDepth : (g & 1) ? navopt::kDeltaBias : navopt::kDeltaImu; }

// error into e (9 words), the Jacobian into J when given (zeroed here); returns chi2
template <int MUT>
PO_HD double ie_eval(const Ws& W, int g, const State* S, double* e, double* J) {
  if (J) {
    PO_NOUNROLL
    for (int k = 0; k < 9 * kJ; ++k) J[k] = 0.;
  }
  const int m = ie_rows(W, g);
  if (g >= 2 * W.L) edge_depth(W, g - 2 * W.L, S, e, J);
  else if (g & 1) edge_bias(W, g >> 1, S, e, J);
  else edge_pvr<MUT>(W, g >> 1, S, e, J);
  double c = 0.;
  PO_NOUNROLL
  for (int r = 0; r < m; ++r) {
    double v = 0.;
    PO_NOUNROLL
    for (int s = 0; s < m; ++s) v = v + ie_info<MUT>(W, g, r, s) * e[s];
    c = c + e[r] * v;
  }
  return c;
}

// the column of edge g's Jacobian that column `col` of the reduced system is, -1: none
PO_HD int ie_local(const Ws& W, int g, int col) {
  const int32_t* c0 = W.ie_col + 4 * g;
  if (c0[0] >= 0 && col >= c0[0] && col < c0[0] + 9) return col - c0[0];
  if (c0[1] >= 0 && col >= c0[1] && col < c0[1] + 9) return 9 + col - c0[1];
  if (c0[2] >= 0 && col >= c0[2] && col < c0[2] + 6) return 18 + col - c0[2];
  if (c0[3] >= 0 && col >= c0[3] && col < c0[3] + 6) return 24 + col - c0[3];
  return -1;
}
// the inertial edges' share of H[c][r], c <= r, and (r < 0) of b[c]
PO_HD double ie_sum(const Ws& W, int c, int r) {
  double v = 0.;
  const int G = n_inert(W);
  PO_NOUNROLL
  for (int g = 0; g < G; ++g) {
    const int lc = ie_local(W, g, c);
    if (lc < 0) continue;
    const double* I = W.ie_lin + (size_t)g * kIeWords;
    const int m = ie_rows(W, g);
    if (r < 0) {
      PO_NOUNROLL
      for (int k = 0; k < m; ++k) v = v + I[kIeJ + k * kJ + lc] * I[kIeWe + k];
    } else {
      const int lr = ie_local(W, g, r);
      if (lr < 0) continue;
      PO_NOUNROLL
      for (int k = 0; k < m; ++k) v = v + I[kIeJ + k * kJ + lc] * I[kIeWJ + k * kJ + lr];
    }
  }
  return v;
}

// UpdatePoseFromNS FrameKTL.cc:160-181, as navopt::pose_from_ns with the window's Rbc and Pbc
PO_HD void pose_from_ns(const State& s, const Params& p, float* Tcw) {
  double Rd[9], Rwb[9], Rbc[9], Pbc[3], Pwb[3], RR[9], Rcw[9], Pwc[3], t[3];
  poseopt::rotation_of(s.q, Rd);
  for (int k = 0; k < 9; ++k) Rwb[k] = (double)(float)Rd[k], Rbc[k] = (double)(float)p.Rbc[k];
  for (int k = 0; k < 3; ++k) Pwb[k] = (double)(float)s.P[k], Pbc[k] = (double)(float)p.Pbc[k];
  navopt::mat3_mul(Rwb, Rbc, RR);
  navopt::mat3_t(RR, Rcw);
  for (int k = 0; k < 9; ++k) Rcw[k] = (double)(float)Rcw[k];
  navopt::mat3_vec(Rwb, Pbc, Pwc);
  for (int k = 0; k < 3; ++k) Pwc[k] = (double)(float)(Pwc[k] + Pwb[k]);
  navopt::mat3_vec(Rcw, Pwc, t);
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) Tcw[i * 4 + j] = (float)Rcw[i * 3 + j];
    Tcw[i * 4 + 3] = -(float)t[i];
  }
  Tcw[12] = 0.f, Tcw[13] = 0.f, Tcw[14] = 0.f, Tcw[15] = 1.f;
}

// IncSmallPVR NavState.cpp:71-100, IncSmallBias :102-123 on the key frame's columns of the step
template <int MUT>
PO_HD void oplus(const double* xp, int f, State& s) {
  const double* u = xp + col_pvr<MUT>(f);
  const double* ub = xp + col_bias<MUT>(f);
  double R[9], Rp[3], dq[4], q[4];
  poseopt::rotation_of(s.q, R);
  navopt::mat3_vec(R, u, Rp);
  for (int i = 0; i < 3; ++i) s.P[i] = s.P[i] + Rp[i], s.V[i] = s.V[i] + u[3 + i];
  navopt::so3_exp(u + 6, dq);
  navopt::q_mul(s.q, dq, q);
  for (int i = 0; i < 4; ++i) s.q[i] = q[i];
  for (int i = 0; i < 3; ++i) s.dbg[i] = s.dbg[i] + ub[i], s.dba[i] = s.dba[i] + ub[3 + i];
}

// ---- phases --------------------------------------------------------------------------------------------------------------------------
template <int MUT, class Team>
PO_HD void phase_init(const Ws& W, Team& T, int blk) {
  T.par(kLanes, [&](int l) {
    const int i = blk * kLanes + l;
    if (i < W.K) {
      W.ns[i] = W.kf_in[i];
      navopt::q_normalize(W.ns[i].q);
      W.ns_try[i] = W.ns[i];
      navopt::frame_camera(W.ns[i], W.prm->Rbc, W.cam + 12 * i);
      SIM3_UNROLL
      for (int k = 0; k < 12; ++k) W.cam_try[12 * i + k] = W.cam[12 * i + k];
    }
    if (i < W.P) {
      SIM3_UNROLL
      for (int k = 0; k < 3; ++k) W.X[3 * (size_t)i + k] = W.X_try[3 * (size_t)i + k] = (double)W.pts[3 * (size_t)i + k];
    }
    if (i < W.E) W.e_off[i] = 0, W.e_rob[i] = 1, W.e_chi2[i] = 0., W.excluded[i] = 0, W.erased[i] = 0;
    if (i < n_inert(W)) {
      // the slots' columns
      int32_t* c = W.ie_col + 4 * i;
      int ka = -1, kb = -1, kc = -1, kd = -1;
      if (i >= 2 * W.L) {
        const Depth& q = W.depths[i - 2 * W.L];
        ka = q.ka, kb = q.kb, kc = q.kc;
      } else if (i & 1) {
        kc = W.links[i >> 1].kf0, kd = W.links[i >> 1].kf1;
      } else {
        ka = W.links[i >> 1].kf0, kb = W.links[i >> 1].kf1, kc = ka;
      }
      c[0] = ka >= 0 && W.kf_free[ka] >= 0 ? col_pvr<MUT>(W.kf_free[ka]) : -1;
      c[1] = kb >= 0 && W.kf_free[kb] >= 0 ? col_pvr<MUT>(W.kf_free[kb]) : -1;
      c[2] = kc >= 0 && W.kf_free[kc] >= 0 ? col_bias<MUT>(W.kf_free[kc]) : -1;
      c[3] = kd >= 0 && W.kf_free[kd] >= 0 ? col_bias<MUT>(W.kf_free[kd]) : -1;
    }
    if (i == 0) {
      double Rcb[9];
      navopt::mat3_t(W.prm->Rbc, Rcb);
      navopt::mat3_vec(Rcb, W.prm->Pbc, W.camc);
      ba::ctl_reset(W);
    }
  });
  if (blk < W.L) {  // CovPVPhi.inverse() of link blk: navopt_core.hpp's LDL^T, column by column of the identity
    double* A = T.vec();
    double* Xi = T.vec() + 81;
    const double* cov = W.links[blk].cov;
    (void)navopt::ldl_inverse(T, [&](int i, int k) { return cov[i * 9 + k]; }, A, 9, 9, Xi, 9, 9);
    T.par(81, [&](int t) { W.link_info[81 * blk + t] = Xi[t]; });
  }
}

template <int MUT, class Team>
PO_HD void phase_begin(const Ws& W, Team& T, int) {
  T.par(3 * W.P, [&](int i) { W.xl[i] = 0.; });
  T.par(15 * W.F, [&](int i) { W.xp[i] = 0.; });
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
        if (e < W.E && !W.e_off[e]) acc[0] = acc[0] + mono_linearise(W, e);
      },
      &s);
  const int n = T.count([&](int l) {
    const int e = blk * kLanes + l;
    return e < W.E && !W.e_off[e] ? 1 : 0;
  });
  if (T.lead()) W.chunk_chi2[blk] = s, W.chunk_n[blk] = n;
}

// each edge a lane; then WJ and We entry by entry
template <int MUT, class Team>
PO_HD void phase_inert_lin(const Ws& W, Team& T, int blk) {
  const int G = n_inert(W);
  T.par(kLanes, [&](int l) {
    const int g = blk * kLanes + l;
    if (g >= G) return;
    double* I = W.ie_lin + (size_t)g * kIeWords;
    const double c = ie_eval<MUT>(W, g, W.ns, I + kIeE, I + kIeJ);
    I[kIeChi] = c;
    navopt::robustify(c, ie_delta(W, g), true, I + kIeChi + 1, I + kIeChi + 2);
  });
  T.par(kLanes * 9 * (kJ + 1), [&](int t) {
    const int g = blk * kLanes + t / (9 * (kJ + 1)), rc = t % (9 * (kJ + 1)), r = rc / (kJ + 1), c = rc % (kJ + 1);
    if (g >= G) return;
    const int m = ie_rows(W, g);
    if (r >= m) return;
    double* I = W.ie_lin + (size_t)g * kIeWords;
    const double rho1 = I[kIeChi + 2];
    double v = 0.;
    PO_NOUNROLL
    for (int s = 0; s < m; ++s) v = v + (rho1 * ie_info<MUT>(W, g, r, s)) * (c < kJ ? I[kIeJ + s * kJ + c] : I[kIeE + s]);
    if (c < kJ) I[kIeWJ + r * kJ + c] = v;
    else I[kIeWe + r] = v;
  });
}

template <int MUT, class Team>
PO_HD void phase_point_sum(const Ws& W, Team& T, int blk) {
  const double mx = T.maxr([&](int l) {
    const int j = blk * kLanes + l;
    if (j >= W.P) return 0.;
    double H[9];
    const bool on = ba::point_sum(W, j, H);
    if (MUT == kMutTauPoses || !on) return 0.;
    return ba::point_maxdiag(H);
  });
  if (T.lead()) W.chunk_max[blk] = mx;
}

template <int MUT, class Team>
PO_HD void phase_kf_sum(const Ws& W, Team& T, int f) {
  const int b0 = W.kl_begin[f], n = W.kl_begin[f + 1] - b0;
  double S[27];
  T.template sum<27>([&](int l, double* acc) { ba::kf_accumulate(W, b0, n, l, acc); }, S);
  if (T.lead()) {
    SIM3_UNROLL
    for (int k = 0; k < 27; ++k) W.Hpp[27 * f + k] = S[k];
  }
  T.par(0, [&](int) {});
  // the diagonal of the 15-block before lambda: the mono sum, then the inertial terms
  T.par(15, [&](int a) {
    const int a6 = mono_of<MUT>(a);
    const double h = a6 >= 0 ? W.Hpp[27 * f + tri6(a6, a6)] : 0.;
    W.hdiag[15 * f + a] = h + ie_sum(W, 15 * f + a, 15 * f + a);
  });
  if (T.lead()) {
    double mx = 0.;
    PO_NOUNROLL
    for (int k = 0; k < 15; ++k) mx = max_nan(mx, fabs(W.hdiag[15 * f + k]));
    W.chunk_max[chunks(W.P) + f] = mx;
  }
}

template <int MUT, class Team>
PO_HD void phase_lin_ctl(const Ws& W, Team& T, int) {
  const int ce = chunks(W.E), cm = chunks(W.P) + W.F;
  const double mx = T.maxr([&](int l) {
    double m = 0.;
    for (int i = l; i < cm; i += kLanes) m = max_nan(m, W.chunk_max[i]);
    return m;
  });
  const int n_mono = T.count([&](int l) {
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
    const int G = n_inert(W);
    double chi = 0.;
    PO_NOUNROLL
    for (int i = 0; i < ce; ++i) chi = chi + W.chunk_chi2[i];
    PO_NOUNROLL
    for (int g = 0; g < G; ++g) chi = chi + W.ie_lin[(size_t)g * kIeWords + kIeChi + 1];
    ba::levenberg_linearised(W, chi, mx, n_mono + G, W.F, n_points);
  }
}

template <int MUT, class Team>
PO_HD void phase_dinv(const Ws& W, Team& T, int blk) {
  const double lambda = W.ctl->lambda;
  T.par(kLanes, [&](int l) {
    const int j = blk * kLanes + l;
    if (j < W.P && W.p_on[j]) ba::point_dinv(W, j, lambda);
  });
}

// block (i1, i2), i1 <= i2: the 36 + 6 sums of ba_core.hpp's shape 3 over (dP, dPhi), then the whole 15 x 15 block of
// Hpp + lambda I - sum_j W_i1j Dinv_j W_i2j^T written to the lower triangle: the mono part where both entries are dP or dPhi, lambda
// on the diagonal, zero elsewhere.  inert_add adds the inertial edges.
template <int MUT, class Team>
PO_HD void phase_schur(const Ws& W, Team& T, int blk) {
  int i1, i2;
  ba::block_of(blk, W.F, &i1, &i2);
  const bool diag = i1 == i2;
  double* S = T.shared();
  T.template sum_shared<kSchurSums>([&](int l, double* acc) { ba::schur_accumulate(W, i1, i2, l, acc); }, S);
  const int N = 15 * W.F;
  const double lambda = W.ctl->lambda;
  T.par(225 + 15, [&](int k) {
    if (k < 225) {
      const int a = k / 15, b = k - 15 * a;  // a: column inside block i1, b: row inside block i2
      if (diag && a > b) return;
      const int a6 = mono_of<MUT>(a), b6 = mono_of<MUT>(b);
      double v = 0.;
      if (a6 >= 0 && b6 >= 0) {
        double h = 0.;
        if (diag) h = W.Hpp[27 * i1 + (a6 <= b6 ? tri6(a6, b6) : tri6(b6, a6))];
        if (diag && a == b) h = h + lambda;
        v = h - S[a6 * 6 + b6];
      } else if (diag && a == b) {
        v = lambda;
      }
      W.Hs[(size_t)(15 * i2 + b) * N + (15 * i1 + a)] = v;
    } else if (diag) {
      const int a = k - 225, a6 = mono_of<MUT>(a);
      const double h = a6 >= 0 ? W.Hpp[27 * i1 + 21 + a6] : 0.;
      W.bfull[15 * i1 + a] = h;
      W.bs[15 * i1 + a] = a6 >= 0 ? h - S[36 + a6] : 0.;
    }
  });
}

// the inertial edges' J^T (rho1 Omega) J and J^T (rho1 Omega) e into block (i1, i2): one lane an entry
template <int MUT, class Team>
PO_HD void phase_inert_add(const Ws& W, Team& T, int blk) {
  // ba::block_of, written out: behind the call the compiler no longer sees that the columns below are not negative, and the
  // walks of ie_sum cost this kernel 7 to 10 % (profiles/LOG.md)
  int i1 = 0, rest = blk;
  while (rest >= W.F - i1) rest -= W.F - i1, ++i1;
  const int i2 = i1 + rest;
  const bool diag = i1 == i2;
  const int N = 15 * W.F;
  T.par(225 + 15, [&](int k) {
    if (k < 225) {
      const int a = k / 15, b = k - 15 * a;
      if (diag && a > b) return;
      const int c = 15 * i1 + a, r = 15 * i2 + b;
      double v = W.Hs[(size_t)r * N + c] + ie_sum(W, c, r);
      if (MUT == kMutVCols && diag) {  // the mutation: the V columns of the mono Jacobian a copy of the P columns
        const int pa = a - col_pvr<MUT>(0), pb = b - col_pvr<MUT>(0);
        if (pa >= 3 && pa < 6 && pb >= 3 && pb < 6) v = v + W.Hpp[27 * i1 + tri6(pa - 3, pb - 3)];
      }
      W.Hs[(size_t)r * N + c] = v;
    } else if (diag) {
      const int c = 15 * i1 + (k - 225);
      const double v = ie_sum(W, c, -1);
      W.bfull[c] = W.bfull[c] - v;
      W.bs[c] = W.bs[c] - v;
    }
  });
}

// the solve (ba_core.hpp's shape 5 at N = 15F) and the key frames' oplus
template <int MUT, class Team>
PO_HD void phase_solve(const Ws& W, Team& T, int) {
  const int N = 15 * W.F;
  double* y = T.vec() + 15 * kMaxFree;
  const bool ok = ba::ldlt_solve(T, W.Hs, N, W.bs, T.vec(), y);
  if (ok) T.par(N, [&](int i) { W.xp[i] = y[i]; });
  T.par(W.K, [&](int kf) {
    const int f = W.kf_free[kf];
    W.ns_try[kf] = W.ns[kf];
    if (f >= 0) navba::oplus<MUT>(W.xp, f, W.ns_try[kf]);
    navopt::frame_camera(W.ns_try[kf], W.prm->Rbc, W.cam_try + 12 * kf);
  });
  if (T.lead()) W.ctl->solve_ok = ok ? 1 : 0;
}

template <int MUT, class Team>
PO_HD void phase_step(const Ws& W, Team& T, int blk) {
  const double lambda = W.ctl->lambda;
  const bool ok = W.ctl->solve_ok != 0;
  double s;
  T.template sum<1>(
      [&](int l, double* acc) {
        const int j = blk * kLanes + l;
        if (j >= W.P) return;
        if (!W.p_on[j]) {
          SIM3_UNROLL
          for (int b = 0; b < 3; ++b) W.X_try[3 * (size_t)j + b] = W.X[3 * (size_t)j + b];
          return;
        }
        acc[0] = acc[0] + ba::point_step(W, j, ok, lambda, [&](int e, double* x) {
          const int f = W.kf_free[W.e_kf[e]];
          if (f < 0) return false;
          SIM3_UNROLL
          for (int a = 0; a < 6; ++a) x[a] = W.xp[col_pvr<MUT>(f) + pvr_of6<MUT>(a)];
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
        MonoEval E;
        mono_error(W, e, W.cam_try, W.X_try, E);
        W.e_chi2[e] = E.chi2;
        double rho0, rho1;
        navopt::robustify(E.chi2, navopt::kDeltaMono, W.e_rob[e] != 0, &rho0, &rho1);
        acc[0] = acc[0] + rho0;
      },
      &s);
  if (T.lead()) W.chunk_chi2[blk] = s;
}

template <int MUT, class Team>
PO_HD void phase_inert_err(const Ws& W, Team& T, int blk) {
  const int G = n_inert(W);
  T.par(kLanes, [&](int l) {
    const int g = blk * kLanes + l;
    if (g >= G) return;
    double rho0, rho1;
    const double c = ie_eval<MUT>(W, g, W.ns_try, W.ie_etry + 9 * (size_t)g, nullptr);
    navopt::robustify(c, ie_delta(W, g), true, &rho0, &rho1);
    W.ie_try[g] = rho0;
  });
}

template <int MUT, class Team>
PO_HD void phase_trial_ctl(const Ws& W, Team& T, int) {
  Ctl& c = *W.ctl;
  const int ce = chunks(W.E), cp = chunks(W.P), G = n_inert(W);
  const double lambda = c.lambda, cur = c.cur;
  const bool ok = c.solve_ok != 0;
  double tmp = 0.;
  PO_NOUNROLL
  for (int i = 0; i < ce; ++i) tmp = tmp + W.chunk_chi2[i];
  PO_NOUNROLL
  for (int g = 0; g < G; ++g) tmp = tmp + W.ie_try[g];
  if (!ok) tmp = DBL_MAX;
  double scale = 0.;
  PO_NOUNROLL
  for (int i = 0; i < 15 * W.F; ++i) scale = scale + W.xp[i] * (lambda * W.xp[i] + W.bfull[i]);
  PO_NOUNROLL
  for (int i = 0; i < cp; ++i) scale = scale + W.chunk_scale[i];
  scale = scale + 1e-3;
  const double rho = (cur - tmp) / scale;
  const bool accept = rho > 0. && fabs(tmp) <= DBL_MAX;
  T.par(0, [&](int) {});  // every lane has read the control block before the lead rewrites it
  if (accept) {
    T.par(W.K, [&](int i) { W.ns[i] = W.ns_try[i]; });
    T.par(12 * W.K, [&](int i) { W.cam[i] = W.cam_try[i]; });
    T.par(3 * W.P, [&](int i) { W.X[i] = W.X_try[i]; });
  }
  if (T.lead()) ba::levenberg_decide(W, lambda, cur, ok, tmp, scale, rho, accept);
}

// chi2() > 5.991 || !isDepthPositive() on the stored chi2 and the depth at the current estimates; edges of flagged points are not
// examined.  Round 0: level 1 and `excluded`, and the kernel off whatever the verdict.  Round 1: `erased`, over excluded edges too.
template <int MUT, class Team>
PO_HD void phase_check(const Ws& W, Team& T, int blk) {
  const int round = W.ctl->round;
  T.par(kLanes, [&](int l) {
    const int e = blk * kLanes + l;
    if (e >= W.E) return;
    if (W.pt_bad[W.e_pt[e]]) {
      if (MUT == kMutFlaggedOff && round == 0) W.e_rob[e] = 0;
      return;
    }
    if (MUT == kMutFinalSkip && round == 1 && W.e_off[e]) return;
    MonoEval E;
    mono_error(W, e, W.cam, W.X, E);
    const bool over = MUT == kMutCheckFloat ? (float)W.e_chi2[e] > 5.991f : W.e_chi2[e] > 5.991;
    const bool bad = over || !(E.z > 0.);
    if (round == 0) {
      if (bad) W.excluded[e] = 1, W.e_off[e] = 1;
      if (MUT != kMutKeepKernel) W.e_rob[e] = 0;
    } else if (bad) {
      W.erased[e] = 1;
    }
  });
}

template <int MUT, class Team>
PO_HD void phase_finish(const Ws& W, Team& T, int blk) {
  T.par(kLanes, [&](int l) {
    const int i = blk * kLanes + l;
    if (i < W.K) {
      W.kf_out[i] = W.ns[i];
      pose_from_ns(W.ns[i], *W.prm, W.kf_T_out + 16 * i);
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
    case kInertLin: phase_inert_lin<MUT>(W, T, blk); break;
    case kPointSum: phase_point_sum<MUT>(W, T, blk); break;
    case kKfSum: phase_kf_sum<MUT>(W, T, blk); break;
    case kLinCtl: phase_lin_ctl<MUT>(W, T, blk); break;
    case kDinv: phase_dinv<MUT>(W, T, blk); break;
    case kSchur: phase_schur<MUT>(W, T, blk); break;
    case kInertAdd: phase_inert_add<MUT>(W, T, blk); break;
    case kSolve: phase_solve<MUT>(W, T, blk); break;
    case kStep: phase_step<MUT>(W, T, blk); break;
    case kEdgeErr: phase_edge_err<MUT>(W, T, blk); break;
    case kInertErr: phase_inert_err<MUT>(W, T, blk); break;
    case kTrialCtl: phase_trial_ctl<MUT>(W, T, blk); break;
    case kCheck: phase_check<MUT>(W, T, blk); break;
    default: phase_finish<MUT>(W, T, blk); break;
  }
}

// ---- host side: the launch sequence -----------------------------------------------------------------------------------------------------
struct Dims {
  int K, F, P, E, L, D;
};

PO_HD int imax(int a, int b) { return a > b ? a : b; }

// as ba::drive: X.launch(phase, blocks), X.status(&st).  optimize(5), the first check, optimize(10), the final check.
template <class X>
int drive(X& x, const Dims& d, int* syncs) {
  const int ce = chunks(d.E), cp = chunks(d.P), cg = chunks(2 * d.L + d.D), sb = schur_blocks(d.F);
  int rc = x.launch(kInit, imax(chunks(imax(imax(d.K, d.P), imax(d.E, 2 * d.L + d.D))), d.L));
  for (int round = 0; round < 2 && !rc; ++round) {
    const int its = round == 0 ? 5 : 10;
    rc = x.launch(kBegin, 1);
    int st = kStLinearise;
    for (int it = 0; it < its && !rc && st == kStLinearise; ++it) {
      if (!rc) rc = x.launch(kEdgeLin, ce);
      if (!rc) rc = x.launch(kInertLin, cg);
      if (!rc) rc = x.launch(kPointSum, cp);
      if (!rc) rc = x.launch(kKfSum, d.F);
      if (!rc) rc = x.launch(kLinCtl, 1);
      st = kStTrial;
      for (int trial = 0; trial < kMaxTrials && !rc && st == kStTrial; ++trial) {
        if (!rc) rc = x.launch(kDinv, cp);
        if (!rc) rc = x.launch(kSchur, sb);
        if (!rc) rc = x.launch(kInertAdd, sb);
        if (!rc) rc = x.launch(kSolve, 1);
        if (!rc) rc = x.launch(kStep, cp);
        if (!rc) rc = x.launch(kEdgeErr, ce);
        if (!rc) rc = x.launch(kInertErr, cg);
        if (!rc) rc = x.launch(kTrialCtl, 1);
        if (!rc) rc = x.status(&st), ++*syncs;
      }
      if (st == kStTrial) st = kStStop;  // cannot happen: the tenth trial never asks for another
    }
    if (!rc) rc = x.launch(kCheck, ce);
  }
  if (!rc) rc = x.launch(kFinish, chunks(imax(d.K, d.P)));
  return rc;
}

// What the call checks of the inertial lists before anything is written.  Returns 0, or 1 when a link or a depth entry names a key
// frame or a link out of range or one key frame twice, names the bias vertex of a key frame that carries none, or a free key frame has
// no link ending in it.
inline int check_inertial(int K, const uint8_t* fixed, const uint8_t* has_bias, int L, const Link* links, int D, const Depth* depths) {
  uint8_t linked[kMaxFree + kMaxFixed];
  for (int k = 0; k < K; ++k) linked[k] = 0;
  for (int l = 0; l < L; ++l) {
    const Link& q = links[l];
    if (q.kf0 < 0 || q.kf0 >= K || q.kf1 < 0 || q.kf1 >= K || q.kf0 == q.kf1) return 1;
    if (!has_bias[q.kf0] || !has_bias[q.kf1]) return 1;
    linked[q.kf1] = 1;
  }
  for (int d = 0; d < D; ++d) {
    const Depth& q = depths[d];
    if (q.ka < 0 || q.ka >= K || q.kb < 0 || q.kb >= K || q.kc < 0 || q.kc >= K || q.link < 0 || q.link >= L || q.ka == q.kb) return 1;
    if (!has_bias[q.kc]) return 1;
  }
  for (int k = 0; k < K; ++k)
    if (!fixed[k] && (!linked[k] || !has_bias[k])) return 1;
  return 0;
}

#if !defined(__HIP_DEVICE_COMPILE__)
using HostTeam = ba::HostTeam;
static_assert(2 * 15 * kMaxFree <= 2 * 6 * ba::kMaxFree, "the solve's two vectors fit ba::HostTeam's");
#endif

}  // namespace navba
}  // namespace uvo
