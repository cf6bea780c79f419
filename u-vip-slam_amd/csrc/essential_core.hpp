// Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:2409-2658 of the reference) with the parts of g2o it runs: g2o::Sim3 (product,
// inverse, log), VertexSim3Expmap (_fix_scale stays false, as its constructor leaves it: the scale is optimised), EdgeSim3 with
// BaseBinaryEdge's NUMERIC Jacobian, the Levenberg driver under setUserLambdaInit(1e-16), the pose recovery and the map points'
// correction.  Plain C++ in double under the rules of poseopt_core.hpp: IEEE + - * / sqrt and fabs only, no contraction
// (-ffp-contract=off on both sides), no library function.  essential.hip runs this on the device, tests/emu/essential_emu.cpp on the
// host; the two are held to each other bit for bit.
//
// The work is cut into PHASES as ba_core.hpp cuts it: a phase is a function of (workspace, team, block index), a block is what one
// workgroup of 256 lanes does, the device launches one kernel per phase, the host build calls the blocks in turn.  drive() below, host
// code shared by both builds, chooses the phases; the Levenberg decision is made in the phases lin_ctl and trial_ctl, which leave a
// status word.  Nothing waits for another block inside a phase.
//
// EVERY FLOATING-POINT SUM HAS ONE FIXED SHAPE THAT DEPENDS ON INDICES ALONE:
//   1. per edge: the seven products of J^T J and of J^T (-e) are summed over the error's rows in ascending row onto the first product.
//   2. per free key frame (the 28 upper entries of its diagonal block, its 7 entries of b): one lane per entry walks the key frame's
//      incidence list (ascending edge index, built at upload) serially onto 0.0.
//   3. per off-diagonal block that has edges (the pair list, sorted at upload; several edges may join one pair): one lane per entry of
//      the 49 walks the pair's edges in ascending edge index onto 0.0.
//   4. scalars (chi2 over the edges, x . (lambda x + b) over the 7 F unknowns): chunks of 256 in lane_team.hpp's shape, the chunk sums
//      folded in ascending order onto 0.0: shape 4 of ba_core.hpp.
//   5. the system: shape 5 of ba_core.hpp RESTRICTED TO THE BLOCK ENVELOPE.  Free key frames stand in key-frame order (ascending mnId:
//      the caller's order); row i of blocks holds the blocks first[i] .. i, first[i] the smallest free index an edge joins to i.  The
//      unpivoted LDL^T runs in place; every entry receives its updates in ascending scalar k as v - (L_ik * L_jk) * d_k; forward
//      substitution in ascending k, back substitution in descending k; "ok" = every pivot finite and > 0.  Outside the envelope the
//      dense factor holds zeros, whose updates change nothing: on one matrix the envelope solve and ba::ldlt_solve give the same bits
//      (as long as no pivot is zero or not finite: a dense factor then fills with NaN where the envelope stores nothing).
//      The factorisation is right-looking over BLOCK columns, three barriers a key frame: the 7 x 7 diagonal block by one lane, a lane
//      per scalar row below it through the block's seven columns in order, the trailing update over all pairs of rows in the column's
//      structure with its seven terms in ascending k.
// No floating-point atomics.
//
// Departures from the reference, stated in uvo.h and DESIGN.md section 4: the block-envelope LDL^T in key-frame order in place of
// SimplicialLDLT under an AMD ordering; the sums' shapes above in place of g2o's order over its containers; sin, cos, acos, exp and log
// are the library's own (sim3::sincos, sim3::acos_ieee, sim3opt::exp_, log_ below); on a failed solve the step keeps its previous value
// (zero at the start); W.lu() is restated as a 3 x 3 partial-pivot LU with the first largest pivot.
#pragma once
#include "ba_core.hpp"
#include "sim3opt_core.hpp"

namespace uvo {
namespace essential {

using poseopt::kLanes;
using sim3opt::Sim;
using ba::Ctl;
using ba::Trace;
using ba::kStTrial;
using ba::kStLinearise;
using ba::kStStop;
using ba::kMaxTrials;

constexpr int kMaxKeyframes = 8192, kMaxEdges = 262144, kMaxPoints = 1 << 20, kMaxBlocks = 1 << 22;
constexpr int kMaxIterations = ba::kMaxIterations;  // the reference passes 20
constexpr int kEdgeWords = 105;                     // per edge: e[7], Ji[7][7], Jj[7][7] (row: the error's, column: the update's)
constexpr int kKfPerBlock = 7, kKfEntries = 35;     // assemble: 28 + 7 lanes a key frame
constexpr int kPairsPerBlock = 5;                   // 49 lanes a pair
constexpr int kTeamWords = 64;                      // the solve's words of the team: d[7] at 0, the diagonal block's L at 8
constexpr double kStep = 1e-9, kScalar = 1.0 / (2 * 1e-9);
constexpr double kLambdaInit = 1e-16;

// seeded mutations, for the host build only (tests/emu/essential_emu.cpp); the library instantiates MUT = 0
constexpr int kMutNone = 0, kMutMeasureScw = 1, kMutOneSided = 2, kMutSwapped = 3, kMutLambdaTau = 4, kMutFixedKept = 5, kMutEnvelopeShort = 6,
              kMutOrderReversed = 7, kMutPointsUncorrected = 8;

enum Phase { kInit = 0, kMeasure, kEdgeLin, kKfSum, kPairSum, kLinCtl, kCopy, kSolve, kStepPh, kEdgeErr, kTrialCtl, kFinishKf, kFinishPts, kPhases };

struct Ws {
  int32_t K, F, P, E, NP, NB, fixed, pad_;
  // the upload
  const Sim *Scw, *Scwn;     // [K]
  const int32_t *e_i, *e_j;  // [E]
  const uint8_t* e_conn;     // [E]
  const float* pts;          // [P][3]
  const int32_t* pt_ref;     // [P]
  const int32_t* kf_free;    // [K] index among the free key frames, -1: fixed
  const int32_t* inc_begin;  // [F + 1]
  const int32_t* inc_edge;   // [<= 2E] a free key frame's edges, ascending: 2 * edge + (1: the key frame is the edge's vertex 1)
  const int32_t* pair_begin; // [NP + 1]
  const int32_t* pair_rc;    // [NP][2] block row > block column
  const int32_t* pair_edge;  // [<= E] 2 * edge + (1: the block's row is the edge's vertex 1)
  const int32_t* first;      // [F]
  const int32_t* env_off;    // [F + 1] block offset of row i's block first[i]
  const int32_t* col_begin;  // [F + 1]
  const int32_t* col_rows;   // [NB - F] the rows below the diagonal that hold block column j, ascending
  const int32_t* blk_row;    // [NB] the row of a stored block
  // state
  Sim *est, *est_try;        // [K]
  Sim* meas;                 // [E]
  double* e_lin;             // [E][kEdgeWords]
  double *H, *L;             // [NB][49] the envelope: H as assembled, L the factor's storage
  double *b, *x, *y;         // [7F]
  double *chunk_chi2, *chunk_scale, *chunk_max;  // [chunks of E], [chunks of max(K, 7F)], [blocks of kf_sum]
  Ctl* ctl;
  Trace* trace;
  // the download
  Sim* Scw_out;              // [K]
  float* kf_T_out;           // [K][16]
  float* pt_out;             // [P][3]
};

PO_HD int chunks(int n) { return (n + kLanes - 1) / kLanes; }
PO_HD int kf_blocks(int F) { return (F + kKfPerBlock - 1) / kKfPerBlock; }
PO_HD int pair_blocks(int NP) { return (NP + kPairsPerBlock - 1) / kPairsPerBlock; }
PO_HD int step_items(int K, int F) { return K > 7 * F ? K : 7 * F; }
PO_HD double* block_at(double* A, const Ws& W, int row, int col) { return A + 49 * (size_t)(W.env_off[row] + col - W.first[row]); }

// ---- log -------------------------------------------------------------------------------------------------------------------------------
// log(x) = e ln 2 + log(m), x = m 2^e with m in [sqrt(1/2), sqrt 2], log(m) = 2 atanh(f), f = (m - 1) / (m + 1), ln 2 = L1 + L2 as in
// sim3opt::exp_.  NaN outside [2^-60, 2^60] and for NaN.  Error bound, from the construction: |log_(x) - log(x)| <= 2^-50 |log(x)|.
//   * m and e come from products with exact powers of two (no subnormal in the range): exact.  m - 1 is exact (Sterbenz), m + 1 and the
//     quotient round once each: f is off by 2^-52 relative, |f| <= 0.1716, and atanh passes a relative error on multiplied by at most
//     1 / (1 - f^2) <= 1.031.
//   * z = f^2 <= 0.02944; the series 1/3 + z/5 + ... + z^9/21 leaves out z^10/23 < 2e-17 relative to a term of 1: below 2^-55.  Its
//     Horner roundings and those of f (z p) enter at the weight z/3 < 0.01: below 2^-58 together.  f + f z p: 2^-53.
//     log(m) is off by at most (1.031 + 0.5 + 0.04) 2^-52 < 2^-51 relative.
//   * e L1 is exact (32 bits times |e| <= 60); e L2 + log(m) and the last sum round once each: 2^-53 of at most |log x| each, and
//     |log m| <= |log x|.  Together below (1 + 1/4 + 1/4) 2^-51 |log x| < 2^-50 |log x|.
// At x = 1 + eps (e = 0) the value is 2 atanh(eps / (2 + eps)) within 2^-51 relative: what the scale row of the Jacobian sees.
PO_HD double log_(double x) {
  if (!(x >= 0x1p-60 && x <= 0x1p+60)) return (x - x) / (x - x) + (1. - 1.) / (x - x);
  double m = x;
  int e = 0;
  double up = 0x1p+32, dn = 0x1p-32, lim = 0x1p-31;
  SIM3_UNROLL
  for (int bit = 32; bit >= 1; bit >>= 1) {
    if (m >= up) m = m * dn, e += bit;
    up = bit == 32 ? 0x1p+16 : bit == 16 ? 0x1p+8 : bit == 8 ? 0x1p+4 : bit == 4 ? 0x1p+2 : 0x1p+1;
    dn = bit == 32 ? 0x1p-16 : bit == 16 ? 0x1p-8 : bit == 8 ? 0x1p-4 : bit == 4 ? 0x1p-2 : 0x1p-1;
  }
  up = 0x1p+32;
  SIM3_UNROLL
  for (int bit = 32; bit >= 1; bit >>= 1) {
    if (m < lim) m = m * up, e -= bit;
    lim = bit == 32 ? 0x1p-15 : bit == 16 ? 0x1p-7 : bit == 8 ? 0x1p-3 : bit == 4 ? 0x1p-1 : 0x1p+0;
    up = bit == 32 ? 0x1p+16 : bit == 16 ? 0x1p+8 : bit == 8 ? 0x1p+4 : bit == 4 ? 0x1p+2 : 0x1p+1;
  }
  if (m > 0x1.6a09e667f3bcdp+0) m = m * 0.5, e += 1;  // now in [sqrt(1/2), sqrt 2]
  const double f = (m - 1.) / (m + 1.), z = f * f;
  double p = 1. / 21.;
  p = 1. / 19. + z * p;
  p = 1. / 17. + z * p;
  p = 1. / 15. + z * p;
  p = 1. / 13. + z * p;
  p = 1. / 11. + z * p;
  p = 1. / 9. + z * p;
  p = 1. / 7. + z * p;
  p = 1. / 5. + z * p;
  p = 1. / 3. + z * p;
  const double lm = 2. * (f + f * (z * p));
  const double ed = (double)e;
  return ed * 0x1.62e42fee00000p-1 + (ed * 0x1.a39ef35793c76p-33 + lm);
}

// ---- g2o::Sim3 -------------------------------------------------------------------------------------------------------------------------
// operator*: r = a.r * b.r (Eigen's quaternion product, not normalised), t = a.s (a.r * b.t) + a.t, s = a.s * b.s
PO_HD void sim_mul(const Sim& A, const Sim& B, Sim& o) {
  const double *a = A.q, *b = B.q;
  double rt[3];
  poseopt::rotate(A.q, B.t[0], B.t[1], B.t[2], rt);
  const double w = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
  const double x = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
  const double y = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2];
  const double z = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0];
  o.t[0] = A.s * rt[0] + A.t[0], o.t[1] = A.s * rt[1] + A.t[1], o.t[2] = A.s * rt[2] + A.t[2];
  o.q[0] = x, o.q[1] = y, o.q[2] = z, o.q[3] = w;
  o.s = A.s * B.s;
}

// inverse(): (r*, r* ((-1 / s) t), 1 / s)
PO_HD void sim_inv(const Sim& A, Sim& o) {
  const double qc[4] = {-A.q[0], -A.q[1], -A.q[2], A.q[3]};
  const double ms = -1. / A.s;
  double ti[3];
  poseopt::rotate(qc, ms * A.t[0], ms * A.t[1], ms * A.t[2], ti);
  o.q[0] = qc[0], o.q[1] = qc[1], o.q[2] = qc[2], o.q[3] = qc[3];
  o.t[0] = ti[0], o.t[1] = ti[1], o.t[2] = ti[2];
  o.s = 1. / A.s;
}

// map(): s (r * xyz) + t
PO_HD void sim_map(const Sim& A, const double X[3], double o[3]) {
  double r[3];
  poseopt::rotate(A.q, X[0], X[1], X[2], r);
  o[0] = A.s * r[0] + A.t[0], o[1] = A.s * r[1] + A.t[1], o[2] = A.s * r[2] + A.t[2];
}

// W.lu().solve(t) at 3 x 3: Eigen's PartialPivLU (the first entry of largest magnitude in the column is the pivot), the unit lower and
// the upper triangular solves, a row's products summed before they are subtracted
PO_HD void lu3_solve(const double Win[9], const double t[3], double x[3]) {
  double a00 = Win[0], a01 = Win[1], a02 = Win[2], a10 = Win[3], a11 = Win[4], a12 = Win[5], a20 = Win[6], a21 = Win[7], a22 = Win[8];
  double c0 = t[0], c1 = t[1], c2 = t[2];
#define ESS_SWAP(u, v) \
  {                    \
    const double s_ = u; \
    u = v, v = s_;     \
  }
  {
    const bool p1 = fabs(a10) > fabs(a00) && !(fabs(a20) > fabs(a10)), p2 = fabs(a20) > fabs(a00) && fabs(a20) > fabs(a10);
    if (p1) {
      ESS_SWAP(a00, a10) ESS_SWAP(a01, a11) ESS_SWAP(a02, a12) ESS_SWAP(c0, c1)
    } else if (p2) {
      ESS_SWAP(a00, a20) ESS_SWAP(a01, a21) ESS_SWAP(a02, a22) ESS_SWAP(c0, c2)
    }
  }
  a10 = a10 / a00, a20 = a20 / a00;
  a11 = a11 - a10 * a01, a12 = a12 - a10 * a02, a21 = a21 - a20 * a01, a22 = a22 - a20 * a02;
  if (fabs(a21) > fabs(a11)) {
    ESS_SWAP(a10, a20) ESS_SWAP(a11, a21) ESS_SWAP(a12, a22) ESS_SWAP(c1, c2)
  }
#undef ESS_SWAP
  a21 = a21 / a11;
  a22 = a22 - a21 * a12;
  c1 = c1 - a10 * c0;
  c2 = c2 - (a20 * c0 + a21 * c1);
  x[2] = c2 / a22;
  x[1] = (c1 - a12 * x[2]) / a11;
  x[0] = (c0 - (a01 * x[1] + a02 * x[2])) / a00;
}

// log(): sim3.h:148-230, its four branches
PO_HD void sim_log(const Sim& S, double res[7]) {
  const double sigma = log_(S.s);
  double R[9];
  poseopt::rotation_of(S.q, R);
  const double d = 0.5 * (((R[0] + R[4]) + R[8]) - 1.);
  const double dR[3] = {R[7] - R[5], R[2] - R[6], R[3] - R[1]};
  const double eps = 0.00001;
  const bool small_sigma = fabs(sigma) < eps, near = d > 1. - eps;
  double om[3], A, B, C;
  if (near) {
    om[0] = 0.5 * dR[0], om[1] = 0.5 * dR[1], om[2] = 0.5 * dR[2];
    if (small_sigma) {
      C = 1., A = 1. / 2., B = 1. / 6.;
    } else {
      const double sigma2 = sigma * sigma;
      C = (S.s - 1.) / sigma;
      A = ((sigma - 1.) * S.s + 1.) / sigma2;
      B = ((0.5 * sigma2 - sigma + 1.) * S.s) / (sigma2 * sigma);
    }
  } else {
    const double theta = sim3::acos_ieee(d);
    const double f = theta / (2. * sqrt(1. - d * d));
    om[0] = f * dR[0], om[1] = f * dR[1], om[2] = f * dR[2];
    const double theta2 = theta * theta;
    double sn, cs;
    sim3::sincos(theta, &sn, &cs);
    if (small_sigma) {
      C = 1.;
      A = (1. - cs) / theta2;
      B = (theta - sn) / (theta2 * theta);
    } else {
      C = (S.s - 1.) / sigma;
      const double a = S.s * sn, b = S.s * cs, c = theta2 + sigma * sigma;
      A = (a * sigma + (1. - b) * theta) / (theta * c);
      B = (C - ((b - 1.) * sigma + a * theta) / c) * 1. / theta2;
    }
  }
  const double Om[9] = {0., -om[2], om[1], om[2], 0., -om[0], -om[1], om[0], 0.};
  double Wm[9];
  SIM3_UNROLL
  for (int i = 0; i < 3; ++i)
    SIM3_UNROLL
    for (int j = 0; j < 3; ++j) {
      // A * Omega + B * Omega * Omega + C * I: (B Omega) Omega as a product, summed in index order
      const double bo = ((B * Om[i * 3]) * Om[j] + (B * Om[i * 3 + 1]) * Om[3 + j]) + (B * Om[i * 3 + 2]) * Om[6 + j];
      Wm[i * 3 + j] = (A * Om[i * 3 + j] + bo) + C * (i == j ? 1. : 0.);
    }
  double up[3];
  lu3_solve(Wm, S.t, up);
  res[0] = om[0], res[1] = om[1], res[2] = om[2], res[3] = up[0], res[4] = up[1], res[5] = up[2], res[6] = sigma;
}

// EdgeSim3::computeError: log(C * S_i * S_j^-1), vertex 0 = i, vertex 1 = j; Sjinv = S_j.inverse()
PO_HD void edge_error(const Sim& C, const Sim& Si, const Sim& Sjinv, double e[7]) {
  Sim a, b;
  sim_mul(C, Si, a);
  sim_mul(a, Sjinv, b);
  sim_log(b, e);
}

// the edge's two estimates as computeError reads them (the mutation: the edge's direction swapped)
template <int MUT>
PO_HD void edge_ends(const Ws& W, int e, int* vi, int* vj) {
  *vi = MUT == kMutSwapped ? W.e_j[e] : W.e_i[e];
  *vj = MUT == kMutSwapped ? W.e_i[e] : W.e_j[e];
}

// chi2 = e . e under the information I_7: e^T (I e), the zeros of I dropped
PO_HD double chi2_of(const double e[7]) {
  double c = e[0] * e[0];
  SIM3_UNROLL
  for (int k = 1; k < 7; ++k) c = c + e[k] * e[k];
  return c;
}

// computeError and linearizeOplus of edge e at W.est: e[7] and the Jacobians of the vertices that are not fixed (central difference,
// delta 1e-9, scalar 1 / 2e-9, the estimate Sim3(+-delta e_d) * S) into e_lin.  Returns chi2.
template <int MUT>
PO_HD double edge_linearise(const Ws& W, int e) {
  int vi, vj;
  edge_ends<MUT>(W, e, &vi, &vj);
  const Sim C = W.meas[e];
  const Sim Si = W.est[vi], Sj = W.est[vj];
  Sim Sjinv;
  sim_inv(Sj, Sjinv);
  double* L = W.e_lin + (size_t)e * kEdgeWords;
  double e0[7];
  edge_error(C, Si, Sjinv, e0);
  SIM3_UNROLL
  for (int k = 0; k < 7; ++k) L[k] = e0[k];
  PO_NOUNROLL
  for (int side = 0; side < 2; ++side) {
    // the edge's vertex `side` is W.e_i / W.e_j whatever the mutation swaps: the lists of the assembly name the edge's own ends
    const int v = side == 0 ? W.e_i[e] : W.e_j[e];
    if (W.kf_free[v] < 0 && MUT != kMutFixedKept) continue;  // a fixed vertex's columns are not computed
    const bool first_of_error = v == vi;
    const Sim S = W.est[v];
    double* J = L + 7 + 49 * side;
    PO_NOUNROLL
    for (int d = 0; d < 7; ++d) {
      double dx[7], ep[7], em[7];
      Sim Q, Qinv;
      SIM3_UNROLL
      for (int j = 0; j < 7; ++j) dx[j] = j == d ? kStep : 0.;
      sim3opt::oplus<sim3opt::kMutNone, true>(dx, S, Q);
      if (first_of_error) edge_error(C, Q, Sjinv, ep);
      else sim_inv(Q, Qinv), edge_error(C, Si, Qinv, ep);
      if (MUT == kMutOneSided) {
        SIM3_UNROLL
        for (int k = 0; k < 7; ++k) em[k] = e0[k];
      } else {
        SIM3_UNROLL
        for (int j = 0; j < 7; ++j) dx[j] = j == d ? -kStep : 0.;
        sim3opt::oplus<sim3opt::kMutNone, true>(dx, S, Q);
        if (first_of_error) edge_error(C, Q, Sjinv, em);
        else sim_inv(Q, Qinv), edge_error(C, Si, Qinv, em);
      }
      SIM3_UNROLL
      for (int k = 0; k < 7; ++k) J[k * 7 + d] = kScalar * (ep[k] - em[k]);
    }
  }
  return chi2_of(e0);
}

// shape 1: sum over the error's rows of Ja[k][a] * Jb[k][b], and of Ja[k][a] * -e[k]
PO_HD double jtj(const double* Ja, int a, const double* Jb, int b) {
  double s = Ja[a] * Jb[b];
  SIM3_UNROLL
  for (int k = 1; k < 7; ++k) s = s + Ja[k * 7 + a] * Jb[k * 7 + b];
  return s;
}
PO_HD double jte(const double* Ja, int a, const double* e) {
  double s = Ja[a] * -e[0];
  SIM3_UNROLL
  for (int k = 1; k < 7; ++k) s = s + Ja[k * 7 + a] * -e[k];
  return s;
}

PO_HD void tri7(int idx, int* a, int* b) {  // entry idx of the 28 upper entries, row-major -> (a, b), a <= b
  int r = 0, rest = idx;
  while (rest >= 7 - r) rest -= 7 - r, ++r;
  *a = r, *b = r + rest;
}

// ---- shape 5 on the block envelope ---------------------------------------------------------------------------------------------------------
// (A) x = b for the envelope A of W (the factor's storage: a row's blocks first[i] .. i, 49 words each, row-major; of the diagonal
// blocks the lower triangle counts), factorised in place; y [7F] holds x afterwards (whatever the pivots were).  Returns whether every
// pivot was finite and > 0.  T.vec(): kTeamWords words all lanes read.
template <int MUT, class Team>
PO_HD bool envelope_solve(Team& T, const Ws& W, double* A, const double* b, double* y) {
  const int F = W.F;
  double* sh = T.vec();
  bool ok = true;
  T.par(7 * F, [&](int i) { y[i] = b[i]; });
  PO_NOUNROLL
  for (int J = 0; J < F; ++J) {
    double* D = block_at(A, W, J, J);
    if (T.lead()) {
      // the diagonal block, serially; its forward substitution (y of this block has every earlier column's term)
      double Lb[49];
      SIM3_UNROLL
      for (int i = 0; i < 7; ++i)
        SIM3_UNROLL
        for (int j = 0; j <= i; ++j) Lb[i * 7 + j] = D[i * 7 + j];
      SIM3_UNROLL
      for (int k = 0; k < 7; ++k) {
        const double dk = Lb[k * 7 + k];
        sh[k] = dk;
        SIM3_UNROLL
        for (int i = k + 1; i < 7; ++i) Lb[i * 7 + k] = Lb[i * 7 + k] / dk;
        SIM3_UNROLL
        for (int i = k + 1; i < 7; ++i)
          SIM3_UNROLL
          for (int j = k + 1; j <= i; ++j) Lb[i * 7 + j] = Lb[i * 7 + j] - (Lb[i * 7 + k] * Lb[j * 7 + k]) * dk;
      }
      double yb[7];
      SIM3_UNROLL
      for (int i = 0; i < 7; ++i) yb[i] = y[7 * J + i];
      SIM3_UNROLL
      for (int k = 0; k < 7; ++k)
        SIM3_UNROLL
        for (int i = k + 1; i < 7; ++i) yb[i] = yb[i] - Lb[i * 7 + k] * yb[k];
      SIM3_UNROLL
      for (int i = 0; i < 7; ++i) {
        y[7 * J + i] = yb[i];
        SIM3_UNROLL
        for (int j = 0; j <= i; ++j) D[i * 7 + j] = Lb[i * 7 + j], sh[8 + i * 7 + j] = Lb[i * 7 + j];
      }
    }
    T.par(0, [&](int) {});
    SIM3_UNROLL
    for (int k = 0; k < 7; ++k) ok = ok && sh[k] > 0. && sh[k] <= DBL_MAX;
    const int cb = W.col_begin[J], m = W.col_begin[J + 1] - cb;
    // a lane per scalar row below: its seven entries through the block's columns in order, then its term of the forward substitution
    T.par(7 * m, [&](int r) {
      const int I = W.col_rows[cb + r / 7], a = r % 7;
      double* Lr = block_at(A, W, I, J) + 7 * a;
      double v[7];
      SIM3_UNROLL
      for (int c = 0; c < 7; ++c) v[c] = Lr[c];
      SIM3_UNROLL
      for (int k = 0; k < 7; ++k) {
        v[k] = v[k] / sh[k];
        SIM3_UNROLL
        for (int c = k + 1; c < 7; ++c) v[c] = v[c] - (v[k] * sh[8 + c * 7 + k]) * sh[k];
      }
      double yr = y[7 * I + a];
      SIM3_UNROLL
      for (int k = 0; k < 7; ++k) Lr[k] = v[k], yr = yr - v[k] * y[7 * J + k];
      y[7 * I + a] = yr;
    });
    // the trailing update over all pairs of rows of the column's structure
    const int n = 7 * m;
    auto update = [&](int r, int c) {
      if (c > r) return;
      const int p = r / 7, a = r - 7 * p, q = c / 7, bb = c - 7 * q;
      const int I = W.col_rows[cb + p], I2 = W.col_rows[cb + q];
      const double* Lr = block_at(A, W, I, J) + 7 * a;
      const double* Lc = block_at(A, W, I2, J) + 7 * bb;
      double* dst = block_at(A, W, I, I2) + 7 * a + bb;
      double v = *dst;
      if (MUT == kMutOrderReversed) {
        SIM3_UNROLL
        for (int k = 6; k >= 0; --k) v = v - (Lr[k] * Lc[k]) * sh[k];
      } else {
        SIM3_UNROLL
        for (int k = 0; k < 7; ++k) v = v - (Lr[k] * Lc[k]) * sh[k];
      }
      *dst = v;
    };
    // one entry a lane; which lane takes which entry changes no value
    if (n <= 4096) T.par(n * n, [&](int idx) { update(idx / n, idx % n); });
    else T.par2(n, n, update);
  }
  T.par(7 * F, [&](int i) {
    const int I = i / 7, a = i - 7 * I;
    y[i] = y[i] / block_at(A, W, I, I)[a * 7 + a];
  });
  PO_NOUNROLL
  for (int I = F - 1; I >= 0; --I) {
    if (T.lead()) {
      const double* D = block_at(A, W, I, I);
      double yb[7];
      SIM3_UNROLL
      for (int i = 0; i < 7; ++i) yb[i] = y[7 * I + i];
      SIM3_UNROLL
      for (int k = 6; k >= 1; --k)
        SIM3_UNROLL
        for (int i = 0; i < k; ++i) yb[i] = yb[i] - D[k * 7 + i] * yb[k];
      SIM3_UNROLL
      for (int i = 0; i < 7; ++i) y[7 * I + i] = yb[i], sh[i] = yb[i];
    }
    T.par(0, [&](int) {});
    const int f0 = W.first[I];
    T.par(7 * (I - f0), [&](int c) {
      const int j = f0 + c / 7, bb = c % 7;
      const double* Bk = block_at(A, W, I, j);
      double yc = y[7 * j + bb];
      SIM3_UNROLL
      for (int a = 6; a >= 0; --a) yc = yc - Bk[a * 7 + bb] * sh[a];
      y[7 * j + bb] = yc;
    });
  }
  return ok;
}

// ---- phases ----------------------------------------------------------------------------------------------------------------------------
template <int MUT, class Team>
PO_HD void phase_init(const Ws& W, Team& T, int blk) {
  const size_t words = 49 * (size_t)W.NB;
  T.par(kLanes, [&](int l) {
    const size_t i = (size_t)blk * kLanes + l;
    if (i < words) W.H[i] = 0.;
    if (i < (size_t)W.K) W.est[i] = W.Scw[i], W.est_try[i] = W.Scw[i];
    if (i < 7 * (size_t)W.F) W.x[i] = 0., W.b[i] = 0.;
    if (i == 0) ba::ctl_reset(W), W.ctl->round = 0;
  });
}

// setMeasurement(Sjw * Swi): S_j * S_i^-1 from CorrectedSim3 / the poses for an edge of LoopConnections, from NonCorrectedSim3 else
template <int MUT, class Team>
PO_HD void phase_measure(const Ws& W, Team& T, int blk) {
  T.par(kLanes, [&](int l) {
    const int e = blk * kLanes + l;
    if (e >= W.E) return;
    const Sim* from = W.e_conn[e] || MUT == kMutMeasureScw ? W.Scw : W.Scwn;
    Sim inv, m;
    sim_inv(from[W.e_i[e]], inv);
    sim_mul(from[W.e_j[e]], inv, m);
    W.meas[e] = m;
  });
}

template <int MUT, class Team>
PO_HD void phase_edge_lin(const Ws& W, Team& T, int blk) {
  double s;
  T.template sum<1>(
      [&](int l, double* acc) {
        const int e = blk * kLanes + l;
        if (e < W.E) acc[0] = acc[0] + edge_linearise<MUT>(W, e);
      },
      &s);
  if (T.lead()) W.chunk_chi2[blk] = s;
}

// shape 2: kKfPerBlock key frames a block, 35 lanes each
template <int MUT, class Team>
PO_HD void phase_kf_sum(const Ws& W, Team& T, int blk) {
  const double mx = T.maxr([&](int l) {
    const int f = blk * kKfPerBlock + l / kKfEntries, k = l % kKfEntries;
    if (l >= kKfPerBlock * kKfEntries || f >= W.F) return 0.;
    int a = k - 28, b = 0;
    if (k < 28) tri7(k, &a, &b);
    double s = 0.;
    PO_NOUNROLL
    for (int i = W.inc_begin[f]; i < W.inc_begin[f + 1]; ++i) {
      const int w = W.inc_edge[i];
      const double* L = W.e_lin + (size_t)(w >> 1) * kEdgeWords;
      const double* J = L + 7 + 49 * (w & 1);
      s = s + (k < 28 ? jtj(J, a, J, b) : jte(J, a, L));
    }
    if (k >= 28) {
      W.b[7 * f + a] = s;
      return 0.;
    }
    double* D = block_at(W.H, W, f, f);
    D[a * 7 + b] = s, D[b * 7 + a] = s;
    return a == b ? fabs(s) : 0.;
  });
  if (T.lead()) W.chunk_max[blk] = mx;
}

// shape 3: kPairsPerBlock pairs a block, 49 lanes each; block (row, column), row > column, entry (a, b) = sum J_row[.][a] J_column[.][b]
template <int MUT, class Team>
PO_HD void phase_pair_sum(const Ws& W, Team& T, int blk) {
  T.par(kLanes, [&](int l) {
    const int p = blk * kPairsPerBlock + l / 49, k = l % 49;
    if (l >= kPairsPerBlock * 49 || p >= W.NP) return;
    const int a = k / 7, b = k - 7 * a;
    double s = 0.;
    PO_NOUNROLL
    for (int i = W.pair_begin[p]; i < W.pair_begin[p + 1]; ++i) {
      const int w = W.pair_edge[i];
      const double* L = W.e_lin + (size_t)(w >> 1) * kEdgeWords + 7;
      s = s + jtj(L + 49 * (w & 1), a, L + 49 * (1 - (w & 1)), b);
    }
    block_at(W.H, W, W.pair_rc[2 * p], W.pair_rc[2 * p + 1])[k] = s;
  });
}

// computeActiveErrors' chi2; the user's lambda at the first iteration; the trace record
template <int MUT, class Team>
PO_HD void phase_lin_ctl(const Ws& W, Team& T, int) {
  if (!T.lead()) return;
  Ctl& c = *W.ctl;
  double chi = 0.;
  PO_NOUNROLL
  for (int i = 0; i < chunks(W.E); ++i) chi = chi + W.chunk_chi2[i];
  double mx = 0.;
  PO_NOUNROLL
  for (int i = 0; i < kf_blocks(W.F); ++i) mx = ba::max_nan(mx, W.chunk_max[i]);
  c.cur = chi, c.ini = chi;
  if (c.it == 0) c.lambda = MUT == kMutLambdaTau ? 1e-5 * mx : kLambdaInit, c.ni = 2., c.stalled = 0;
  c.q = 0, c.rho = 0.;
  if (c.n_lin < ba::kMaxLin) {
    ba::TraceLin& r = W.trace->lin[c.n_lin];
    r.round = 0, r.iteration = c.it, r.n_edges = W.E, r.n_free = W.F, r.n_points = W.P, r.pad_ = 0;
    r.chi2 = chi, r.maxdiag = mx;
  }
  c.n_lin = c.n_lin + 1;
  W.trace->n_lin = c.n_lin;
  c.its[0] = c.its[0] + 1;
  c.status = kStTrial;
}

// H into the factor's storage, lambda onto the diagonal: a rejected trial refactors from H
template <int MUT, class Team>
PO_HD void phase_copy(const Ws& W, Team& T, int blk) {
  const double lambda = W.ctl->lambda;
  const size_t words = 49 * (size_t)W.NB;
  T.par(kLanes, [&](int l) {
    const size_t i = (size_t)blk * kLanes + l;
    if (i >= words) return;
    const int bi = (int)(i / 49), k = (int)(i - 49 * (size_t)bi);
    const bool diagonal = k % 8 == 0 && bi == W.env_off[W.blk_row[bi] + 1] - 1;
    W.L[i] = diagonal ? W.H[i] + lambda : W.H[i];
  });
}

template <int MUT, class Team>
PO_HD void phase_solve(const Ws& W, Team& T, int) {
  const bool ok = envelope_solve<MUT>(T, W, W.L, W.b, W.y);
  if (ok) T.par(7 * W.F, [&](int i) { W.x[i] = W.y[i]; });
  // on a failed solve the step keeps its previous value and is applied all the same, as update(_solver->x()) is
  if (T.lead()) W.ctl->solve_ok = ok ? 1 : 0;
}

// oplusImpl of every free key frame; a chunk's share of x . (lambda x + b)
template <int MUT, class Team>
PO_HD void phase_step(const Ws& W, Team& T, int blk) {
  const double lambda = W.ctl->lambda;
  double s;
  T.template sum<1>(
      [&](int l, double* acc) {
        const int i = blk * kLanes + l;
        if (i < W.K) {
          const int f = W.kf_free[i];
          if (f >= 0) {
            Sim Q;
            sim3opt::oplus<sim3opt::kMutNone>(W.x + 7 * f, W.est[i], Q);
            W.est_try[i] = Q;
          } else {
            W.est_try[i] = W.est[i];
          }
        }
        if (i < 7 * W.F) acc[0] = acc[0] + W.x[i] * (lambda * W.x[i] + W.b[i]);
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
        if (e >= W.E) return;
        int vi, vj;
        edge_ends<MUT>(W, e, &vi, &vj);
        Sim inv;
        sim_inv(W.est_try[vj], inv);
        double err[7];
        edge_error(W.meas[e], W.est_try[vi], inv, err);
        acc[0] = acc[0] + chi2_of(err);
      },
      &s);
  if (T.lead()) W.chunk_chi2[blk] = s;
}

template <int MUT, class Team>
PO_HD void phase_trial_ctl(const Ws& W, Team& T, int) {
  Ctl& c = *W.ctl;
  const double lambda = c.lambda, cur = c.cur;
  const bool ok = c.solve_ok != 0;
  double tmp = 0.;
  PO_NOUNROLL
  for (int i = 0; i < chunks(W.E); ++i) tmp = tmp + W.chunk_chi2[i];
  if (!ok) tmp = DBL_MAX;
  double scale = 0.;
  PO_NOUNROLL
  for (int i = 0; i < chunks(step_items(W.K, W.F)); ++i) scale = scale + W.chunk_scale[i];
  scale = scale + 1e-3;
  const double rho = (cur - tmp) / scale;
  const bool accept = rho > 0. && fabs(tmp) <= DBL_MAX;
  T.par(0, [&](int) {});  // every lane has read the control block before the lead rewrites it
  if (accept) T.par(W.K, [&](int i) { W.est[i] = W.est_try[i]; });
  if (T.lead()) ba::levenberg_decide(W, lambda, cur, ok, tmp, scale, rho, accept);
}

// SE3 pose recovery [R | t / s] as Converter::toCvSE3 narrows it, and the estimate
template <int MUT, class Team>
PO_HD void phase_finish_kf(const Ws& W, Team& T, int blk) {
  T.par(kLanes, [&](int l) {
    const int i = blk * kLanes + l;
    if (i >= W.K) return;
    const Sim S = W.est[i];
    W.Scw_out[i] = S;
    double R[9];
    poseopt::rotation_of(S.q, R);
    const double is = 1. / S.s;
    float* M = W.kf_T_out + 16 * (size_t)i;
    M[0] = (float)R[0], M[1] = (float)R[1], M[2] = (float)R[2], M[3] = (float)(S.t[0] * is);
    M[4] = (float)R[3], M[5] = (float)R[4], M[6] = (float)R[5], M[7] = (float)(S.t[1] * is);
    M[8] = (float)R[6], M[9] = (float)R[7], M[10] = (float)R[8], M[11] = (float)(S.t[2] * is);
    M[12] = 0.f, M[13] = 0.f, M[14] = 0.f, M[15] = 1.f;
  });
}

// correctedSwr.map(Srw.map(X)): Srw = vScw[nIDr], correctedSwr the inverse of the reference key frame's estimate
template <int MUT, class Team>
PO_HD void phase_finish_pts(const Ws& W, Team& T, int blk) {
  T.par(kLanes, [&](int l) {
    const int j = blk * kLanes + l;
    if (j >= W.P) return;
    const int r = W.pt_ref[j];
    const double X[3] = {(double)W.pts[3 * (size_t)j], (double)W.pts[3 * (size_t)j + 1], (double)W.pts[3 * (size_t)j + 2]};
    Sim inv;
    sim_inv(MUT == kMutPointsUncorrected ? W.Scw[r] : W.est[r], inv);
    double c[3], o[3];
    sim_map(W.Scw[r], X, c);
    sim_map(inv, c, o);
    W.pt_out[3 * (size_t)j] = (float)o[0], W.pt_out[3 * (size_t)j + 1] = (float)o[1], W.pt_out[3 * (size_t)j + 2] = (float)o[2];
  });
}

template <int MUT, class Team>
PO_HD void run_phase(int ph, const Ws& W, Team& T, int blk) {
  switch (ph) {
    case kInit: phase_init<MUT>(W, T, blk); break;
    case kMeasure: phase_measure<MUT>(W, T, blk); break;
    case kEdgeLin: phase_edge_lin<MUT>(W, T, blk); break;
    case kKfSum: phase_kf_sum<MUT>(W, T, blk); break;
    case kPairSum: phase_pair_sum<MUT>(W, T, blk); break;
    case kLinCtl: phase_lin_ctl<MUT>(W, T, blk); break;
    case kCopy: phase_copy<MUT>(W, T, blk); break;
    case kSolve: phase_solve<MUT>(W, T, blk); break;
    case kStepPh: phase_step<MUT>(W, T, blk); break;
    case kEdgeErr: phase_edge_err<MUT>(W, T, blk); break;
    case kTrialCtl: phase_trial_ctl<MUT>(W, T, blk); break;
    case kFinishKf: phase_finish_kf<MUT>(W, T, blk); break;
    default: phase_finish_pts<MUT>(W, T, blk); break;
  }
}

// ---- host side: the launch sequence, and what the upload derives from the caller's lists ------------------------------------------------
struct Dims {
  int K, F, P, E, NP, NB;
};

// X as ba::drive's.  Without a free key frame or an edge nothing is optimised: the answer is the input's.  *syncs counts the status reads.
template <class X>
int drive(X& x, const Dims& d, int n_iterations, int* syncs) {
  const int ce = chunks(d.E);
  const size_t words = 49 * (size_t)d.NB;
  size_t most = words > (size_t)d.K ? words : (size_t)d.K;
  if (most < 7 * (size_t)d.F) most = 7 * (size_t)d.F;
  int rc = x.launch(kInit, (int)((most + kLanes - 1) / kLanes));
  const bool go = d.F > 0 && d.E > 0;
  if (go && !rc) rc = x.launch(kMeasure, ce);
  int st = kStLinearise;
  for (int it = 0; go && it < n_iterations && !rc && st == kStLinearise; ++it) {
    if (!rc) rc = x.launch(kEdgeLin, ce);
    if (!rc) rc = x.launch(kKfSum, kf_blocks(d.F));
    if (!rc) rc = x.launch(kPairSum, pair_blocks(d.NP));
    if (!rc) rc = x.launch(kLinCtl, 1);
    st = kStTrial;
    for (int trial = 0; trial < kMaxTrials && !rc && st == kStTrial; ++trial) {
      if (!rc) rc = x.launch(kCopy, (int)((words + kLanes - 1) / kLanes));
      if (!rc) rc = x.launch(kSolve, 1);
      if (!rc) rc = x.launch(kStepPh, chunks(step_items(d.K, d.F)));
      if (!rc) rc = x.launch(kEdgeErr, ce);
      if (!rc) rc = x.launch(kTrialCtl, 1);
      if (!rc) rc = x.status(&st), ++*syncs;
    }
    if (st == kStTrial) st = kStStop;  // cannot happen: the tenth trial never asks for another
  }
  if (!rc) rc = x.launch(kFinishKf, chunks(d.K));
  if (!rc) rc = x.launch(kFinishPts, chunks(d.P));
  return rc;
}

// What the upload derives from the caller's lists (integer work, g2o's buildStructure).  The arrays hold: kf_free K, inc_begin F + 1,
// inc_edge 2E, pair_begin E + 1, pair_rc 2E, pair_edge E, first F, env_off F + 1, col_begin F + 1, col_rows and blk_row max_blocks; scratch max(E, F) words.
constexpr int kDeriveOk = 0, kDeriveRange = 1, kDeriveSelf = 2, kDeriveCapacity = 3;
template <int MUT>
inline int derive(int K, int fixed, int E, const int32_t* e_i, const int32_t* e_j, int max_blocks, int32_t* kf_free, int32_t* inc_begin, int32_t* inc_edge,
                  int32_t* pair_begin, int32_t* pair_rc, int32_t* pair_edge, int32_t* first, int32_t* env_off, int32_t* col_begin, int32_t* col_rows,
                  int32_t* blk_row, int64_t* scratch, Dims* out) {
  if (fixed < 0 || fixed >= K) return kDeriveRange;
  for (int e = 0; e < E; ++e) {
    if (e_i[e] < 0 || e_i[e] >= K || e_j[e] < 0 || e_j[e] >= K) return kDeriveRange;
    if (e_i[e] == e_j[e]) return kDeriveSelf;
  }
  const int F = K - 1;
  for (int k = 0; k < K; ++k) kf_free[k] = k == fixed ? -1 : k < fixed ? k : k - 1;
  // where a vertex's columns land: its own free index; the mutation keeps the fixed vertex's and lands them in some free key frame's
  auto lands = [&](int v) { return kf_free[v] >= 0 ? kf_free[v] : (MUT == kMutFixedKept && F > 0 ? fixed % F : -1); };
  for (int f = 0; f <= F; ++f) inc_begin[f] = 0;
  for (int e = 0; e < E; ++e) {
    const int a = lands(e_i[e]), b = lands(e_j[e]);
    if (a >= 0) ++inc_begin[a + 1];
    if (b >= 0) ++inc_begin[b + 1];
  }
  for (int f = 0; f < F; ++f) inc_begin[f + 1] += inc_begin[f];
  {
    int32_t* fill = col_begin;  // borrowed: F + 1 words
    for (int f = 0; f < F; ++f) fill[f] = inc_begin[f];
    for (int e = 0; e < E; ++e) {
      const int a = lands(e_i[e]), b = lands(e_j[e]);
      if (a >= 0) inc_edge[fill[a]++] = 2 * e;
      if (b >= 0) inc_edge[fill[b]++] = 2 * e + 1;
    }
  }
  for (int f = 0; f < F; ++f) first[f] = f;
  int n = 0;
  for (int e = 0; e < E; ++e) {
    const int a = kf_free[e_i[e]], b = kf_free[e_j[e]];
    if (a < 0 || b < 0) continue;
    const int row = a > b ? a : b, col = a > b ? b : a;
    if (col < first[row]) first[row] = col;
    // the key sorts by (row, column, edge); the low bit: the block's row is the edge's vertex 1
    scratch[n++] = ((int64_t)row << 44) | ((int64_t)col << 24) | ((int64_t)e << 1) | (b > a ? 1 : 0);
  }
  if (MUT == kMutEnvelopeShort)
    for (int f = 0; f < F; ++f)
      if (first[f] < f) ++first[f];
  // an insertion-free sort: shell sort on the keys (host only; E log^2 E)
  for (int gap = n / 2; gap > 0; gap /= 2)
    for (int i = gap; i < n; ++i) {
      const int64_t v = scratch[i];
      int j = i;
      for (; j >= gap && scratch[j - gap] > v; j -= gap) scratch[j] = scratch[j - gap];
      scratch[j] = v;
    }
  int NP = 0, ne = 0;
  pair_begin[0] = 0;
  for (int i = 0; i < n; ++i) {
    const int row = (int)(scratch[i] >> 44), col = (int)((scratch[i] >> 24) & 0xfffff);
    if (col < first[row]) continue;  // only under the mutation
    if (NP == 0 || pair_rc[2 * (NP - 1)] != row || pair_rc[2 * (NP - 1) + 1] != col) {
      pair_rc[2 * NP] = row, pair_rc[2 * NP + 1] = col;
      ++NP;
    }
    pair_edge[ne++] = (int32_t)(scratch[i] & 0xffffff);
    pair_begin[NP] = ne;
  }
  int64_t nb = 0;
  for (int f = 0; f < F; ++f) env_off[f] = (int32_t)nb, nb += f - first[f] + 1;
  env_off[F] = (int32_t)(nb > INT32_MAX ? INT32_MAX : nb);
  if (nb > max_blocks) {
    out->NB = (int)(nb > INT32_MAX ? INT32_MAX : nb);
    return kDeriveCapacity;
  }
  for (int f = 0; f <= F; ++f) col_begin[f] = 0;
  for (int i = 0; i < F; ++i)
    for (int j = first[i]; j < i; ++j) ++col_begin[j + 1];
  for (int f = 0; f < F; ++f) col_begin[f + 1] += col_begin[f];
  for (int f = 0; f < F; ++f) scratch[f] = col_begin[f];
  for (int i = 0; i < F; ++i)
    for (int j = first[i]; j <= i; ++j) {
      blk_row[env_off[i] + j - first[i]] = i;
      if (j < i) col_rows[scratch[j]++] = i;
    }
  out->K = K, out->F = F, out->E = E, out->NP = NP, out->NB = (int)nb;
  return kDeriveOk;
}

}  // namespace essential
}  // namespace uvo
