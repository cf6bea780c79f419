// Host build of the essential-graph optimisation: csrc/essential_core.hpp compiled by the host compiler with -ffp-contract=off, the same
// source the k_essential_* kernels run, with ba::HostTeam walking the reduction shape of 256 lanes and essential::drive choosing the
// phases as it does on the device.  tests/essential_checks.py holds it to the numpy model (tests/essential_model.py) layer by layer;
// tests/test_gpu_essential.py holds the device to it bit for bit.
//
// Eight seeded mutations exist behind -DESSENTIAL_MUT=k of THIS file only (the library has none), to show that the checks can fail:
// 1 every measurement taken from Scw (the normal edges too), 2 a one-sided difference in the numeric Jacobian, 3 the edge's direction
// swapped in computeError, 4 lambda starts at tau * maxdiag, 5 the fixed vertex's columns kept (they land in a free key frame's rows),
// 6 an envelope one block short (the farthest block of a row and its edges dropped), 7 the seven terms of a trailing update in
// descending k, 8 the points mapped back with the uncorrected similarity.
//
// With -DESSENTIAL_EMU_MAIN the file is a stand-alone program that runs the committed scene list (the file named by its argument:
// tests/golden/essential_scenes.bin) once: the form in which it is run under -fsanitize=address,undefined.
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/uvo/uvo.h"
#include "../../u-vip-slam_amd/csrc/essential_core.hpp"

#ifndef ESSENTIAL_MUT
#define ESSENTIAL_MUT 0
#endif

using namespace uvo;
using essential::Sim;

static_assert(sizeof(uvo_essential_trace) == sizeof(ba::Trace), "uvo_essential_trace is ba::Trace");
static_assert(sizeof(uvo_sim3d) == sizeof(Sim), "uvo_sim3d is sim3opt::Sim");

namespace {

// the arrays of a call, owned
struct HostWs {
  essential::Ws W;
  essential::Dims d;
  ba::Ctl ctl;
  ba::Trace trace;
  std::vector<Sim> Scw, Scwn, est, est_try, meas, Scw_out;
  std::vector<int32_t> e_i, e_j, pt_ref, kf_free, inc_begin, inc_edge, pair_begin, pair_rc, pair_edge, first, env_off, col_begin, col_rows, blk_row;
  std::vector<uint8_t> e_conn;
  std::vector<float> pts, kf_T_out, pt_out;
  std::vector<double> e_lin, H, L, b, x, y, chunk_chi2, chunk_scale, chunk_max;
  std::vector<int64_t> scratch;

  // the integer part: 0, or essential::derive's code
  int structure(int K, int fixed, int E, const int32_t* ei, const int32_t* ej, int max_blocks) {
    const size_t k = (size_t)K, e = (size_t)E;
    kf_free.assign(k + 1, 0), inc_begin.assign(k + 2, 0), inc_edge.assign(2 * e + 1, 0), pair_begin.assign(e + 2, 0), pair_rc.assign(2 * e + 2, 0);
    pair_edge.assign(e + 1, 0), first.assign(k + 1, 0), env_off.assign(k + 2, 0), col_begin.assign(k + 2, 0);
    col_rows.assign((size_t)max_blocks + 1, 0), blk_row.assign((size_t)max_blocks + 1, 0), scratch.assign((e > k ? e : k) + 1, 0);
    std::memset(&d, 0, sizeof d);
    const int rc = essential::derive<ESSENTIAL_MUT>(K, fixed, E, ei, ej, max_blocks, kf_free.data(), inc_begin.data(), inc_edge.data(), pair_begin.data(), pair_rc.data(),
                                                    pair_edge.data(), first.data(), env_off.data(), col_begin.data(), col_rows.data(), blk_row.data(), scratch.data(), &d);
    if (rc) return rc;
    W.kf_free = kf_free.data(), W.inc_begin = inc_begin.data(), W.inc_edge = inc_edge.data(), W.pair_begin = pair_begin.data(), W.pair_rc = pair_rc.data();
    W.pair_edge = pair_edge.data(), W.first = first.data(), W.env_off = env_off.data(), W.col_begin = col_begin.data(), W.col_rows = col_rows.data();
    W.blk_row = blk_row.data();
    W.K = K, W.F = d.F, W.E = E, W.NP = d.NP, W.NB = d.NB, W.fixed = fixed, W.pad_ = 0;
    const size_t nb = 49 * (size_t)d.NB + 1, n = 7 * (size_t)d.F + 7;
    H.assign(nb, 0.), L.assign(nb, 0.), b.assign(n, 0.), x.assign(n, 0.), y.assign(n, 0.);
    W.H = H.data(), W.L = L.data(), W.b = b.data(), W.x = x.data(), W.y = y.data();
    return 0;
  }

  int load(const uvo_essential_problem& q, int max_blocks) {
    std::memset(&W, 0, sizeof W);
    const size_t K = (size_t)q.n_keyframes, E = (size_t)q.n_edges, P = (size_t)q.n_points;
    const int rc = structure(q.n_keyframes, q.fixed, q.n_edges, q.edge_i, q.edge_j, max_blocks);
    if (rc) return rc;
    d.P = q.n_points, W.P = q.n_points;
    Scw.assign((const Sim*)q.Scw, (const Sim*)q.Scw + K), Scwn.assign((const Sim*)q.Scw_normal, (const Sim*)q.Scw_normal + K);
    est = Scw, est_try = Scw, Scw_out = Scw;
    meas.assign(E + 1, Sim());
    e_i.assign(q.edge_i, q.edge_i + E), e_j.assign(q.edge_j, q.edge_j + E), e_conn.assign(q.edge_connection, q.edge_connection + E);
    e_i.push_back(0), e_j.push_back(0), e_conn.push_back(0);
    pts.assign(3 * P + 3, 0.f), pt_ref.assign(P + 1, 0), pt_out.assign(3 * P + 3, 0.f), kf_T_out.assign(16 * K + 16, 0.f);
    if (P > 0) std::memcpy(pts.data(), q.points, 12 * P), std::memcpy(pt_ref.data(), q.point_ref, 4 * P);
    e_lin.assign((E + 1) * essential::kEdgeWords, 0.);
    chunk_chi2.assign((size_t)essential::chunks(q.n_edges) + 1, 0.);
    chunk_scale.assign((size_t)essential::chunks(essential::step_items(q.n_keyframes, d.F)) + 1, 0.);
    chunk_max.assign((size_t)essential::kf_blocks(d.F) + 1, 0.);
    std::memset(&ctl, 0, sizeof ctl), std::memset(&trace, 0, sizeof trace);
    W.Scw = Scw.data(), W.Scwn = Scwn.data(), W.e_i = e_i.data(), W.e_j = e_j.data(), W.e_conn = e_conn.data(), W.pts = pts.data(), W.pt_ref = pt_ref.data();
    W.est = est.data(), W.est_try = est_try.data(), W.meas = meas.data(), W.e_lin = e_lin.data();
    W.chunk_chi2 = chunk_chi2.data(), W.chunk_scale = chunk_scale.data(), W.chunk_max = chunk_max.data(), W.ctl = &ctl, W.trace = &trace;
    W.Scw_out = Scw_out.data(), W.kf_T_out = kf_T_out.data(), W.pt_out = pt_out.data();
    return 0;
  }

  // the envelope A (H or L) as the dense lower triangle [7F][7F], zeros outside
  void dense(const std::vector<double>& A, double* out) const {
    const size_t N = 7 * (size_t)d.F;
    std::memset(out, 0, sizeof(double) * N * N);
    for (int i = 0; i < d.F; ++i)
      for (int j = first[i]; j <= i; ++j) {
        const double* B = A.data() + 49 * (size_t)(env_off[i] + j - first[i]);
        for (int a = 0; a < 7; ++a)
          for (int c = 0; c < 7; ++c)
            if (j < i || c <= a) out[(size_t)(7 * i + a) * N + 7 * j + c] = B[a * 7 + c];
      }
  }
};

struct HostExec {
  HostWs* h;
  ba::HostTeam T;
  int launch(int ph, int blocks) {
    for (int b = 0; b < blocks; ++b) essential::run_phase<ESSENTIAL_MUT>(ph, h->W, T, b);
    return 0;
  }
  int status(int* out) {
    *out = h->ctl.status;
    return 0;
  }
};

constexpr int kAnyBlocks = 1 << 22;

}  // namespace

extern "C" {

int emu_essential_mutation() { return ESSENTIAL_MUT; }

double emu_essential_log(double x) { return essential::log_(x); }
double emu_essential_acos(double x) { return sim3::acos_ieee(x); }
void emu_essential_mul(const double* a, const double* b, double* out) { essential::sim_mul(*(const Sim*)a, *(const Sim*)b, *(Sim*)out); }
void emu_essential_inv(const double* a, double* out) { essential::sim_inv(*(const Sim*)a, *(Sim*)out); }
void emu_essential_log7(const double* a, double* out) { essential::sim_log(*(const Sim*)a, out); }
void emu_essential_oplus(const double* dx, const double* a, double* out) { sim3opt::oplus<sim3opt::kMutNone>(dx, *(const Sim*)a, *(Sim*)out); }

// the call, as uvo_essential_graph_optimize answers it.  Returns 0 or essential::derive's code (1 range, 2 i == j, 3 capacity).
int emu_essential_optimize(const uvo_essential_problem* q, int max_blocks, uvo_essential_result* r, uvo_essential_trace* trace) {
  static HostWs h;
  const int rc = h.load(*q, max_blocks);
  if (rc) return rc;
  HostExec x = {&h, {}};
  int syncs = 0;
  essential::drive(x, h.d, q->n_iterations, &syncs);
  const size_t K = (size_t)q->n_keyframes, P = (size_t)q->n_points;
  if (r->Scw) std::memcpy(r->Scw, h.Scw_out.data(), sizeof(Sim) * K);
  if (r->kf_Tcw) std::memcpy(r->kf_Tcw, h.kf_T_out.data(), sizeof(float) * 16 * K);
  if (r->points && P > 0) std::memcpy(r->points, h.pt_out.data(), sizeof(float) * 3 * P);
  r->iterations = h.ctl.its[0], r->n_trials = h.ctl.n_trials, r->n_syncs = syncs + 1, r->envelope_blocks = h.d.NB;
  if (trace) std::memcpy(trace, &h.trace, sizeof h.trace);
  return 0;
}

// One linearisation and one trial at GIVEN estimates est [K][8] and lambda.  Out: dims [4] = F, NP, NB, ok; meas [E][8]; lin [E][105];
// H [7F][7F] the dense lower triangle of the assembled envelope; first [F]; b [7F]; x [7F]; est_try [K][8]; scal [4] = chi2 at the
// linearisation, the largest diagonal entry, tmp, scale.  Returns 0 or essential::derive's code.
int emu_essential_one_trial(const uvo_essential_problem* q, const double* est, double lambda, int32_t* dims, double* meas, double* lin, double* H, int32_t* first,
                            double* b, double* x, double* est_try, double* scal) {
  static HostWs h;
  const int rc = h.load(*q, kAnyBlocks);
  if (rc) return rc;
  const size_t K = (size_t)q->n_keyframes, E = (size_t)q->n_edges, N = 7 * (size_t)h.d.F;
  HostExec X = {&h, {}};
  const size_t words = 49 * (size_t)h.d.NB;
  const size_t most = words > K ? (words > N ? words : N) : (K > N ? K : N);
  X.launch(essential::kInit, (int)((most + 255) / 256));
  X.launch(essential::kMeasure, essential::chunks((int)E));
  std::memcpy(h.est.data(), est, sizeof(Sim) * K);
  X.launch(essential::kEdgeLin, essential::chunks((int)E)), X.launch(essential::kKfSum, essential::kf_blocks(h.d.F));
  X.launch(essential::kPairSum, essential::pair_blocks(h.d.NP)), X.launch(essential::kLinCtl, 1);
  std::memcpy(meas, h.meas.data(), sizeof(Sim) * E), std::memcpy(lin, h.e_lin.data(), sizeof(double) * E * essential::kEdgeWords);
  h.dense(h.H, H);
  std::memcpy(first, h.first.data(), 4 * (size_t)h.d.F), std::memcpy(b, h.b.data(), sizeof(double) * N);
  scal[0] = h.ctl.cur, scal[1] = h.trace.lin[0].maxdiag;
  h.ctl.lambda = lambda;
  X.launch(essential::kCopy, (int)((words + 255) / 256)), X.launch(essential::kSolve, 1);
  const int ok = h.ctl.solve_ok;
  X.launch(essential::kStepPh, essential::chunks(essential::step_items((int)K, h.d.F))), X.launch(essential::kEdgeErr, essential::chunks((int)E));
  X.launch(essential::kTrialCtl, 1);
  std::memcpy(x, h.x.data(), sizeof(double) * N), std::memcpy(est_try, h.est_try.data(), sizeof(Sim) * K);
  dims[0] = h.d.F, dims[1] = h.d.NP, dims[2] = h.d.NB, dims[3] = ok;
  scal[2] = h.trace.trial[0].tmp, scal[3] = h.trace.trial[0].scale;
  return 0;
}

// The envelope solve on a GIVEN matrix: A [7F][7F] (the lower triangle is read, entries outside the envelope of first [F] are not), rhs
// [7F] -> x [7F], Lout [7F][7F] the factor (dense lower triangle, zeros outside the envelope).  Returns ok.
int emu_essential_envelope_solve(int F, const int32_t* first, const double* A, const double* rhs, double* x, double* Lout) {
  static HostWs h;
  std::memset(&h.W, 0, sizeof h.W);
  // a chain of edges that gives exactly this envelope: key frame 0 fixed, free f = key frame f + 1, one edge (f, first[f]) where below
  std::vector<int32_t> ei, ej;
  for (int f = 0; f < F; ++f) {
    if (first[f] < 0 || first[f] > f) return -1;
    if (first[f] < f) ei.push_back(f + 1), ej.push_back(first[f] + 1);
  }
  ei.push_back(0), ej.push_back(0);
  if (h.structure(F + 1, 0, (int)ei.size() - 1, ei.data(), ej.data(), kAnyBlocks)) return -1;
  const size_t N = 7 * (size_t)F;
  for (int i = 0; i < F; ++i)
    for (int j = h.first[i]; j <= i; ++j) {
      double* B = h.L.data() + 49 * (size_t)(h.env_off[i] + j - h.first[i]);
      for (int a = 0; a < 7; ++a)
        for (int c = 0; c < 7; ++c) B[a * 7 + c] = j < i || c <= a ? A[(size_t)(7 * i + a) * N + 7 * j + c] : A[(size_t)(7 * j + c) * N + 7 * i + a];
    }
  ba::HostTeam T;
  const bool ok = essential::envelope_solve<ESSENTIAL_MUT>(T, h.W, h.L.data(), rhs, h.y.data());
  std::memcpy(x, h.y.data(), sizeof(double) * N);
  h.dense(h.L, Lout);
  return ok ? 1 : 0;
}

// ba::ldlt_solve on the dense lower triangle A [N][N], in place; x [N].  Returns ok.
int emu_essential_dense_solve(int N, double* A, const double* rhs, double* x) {
  ba::HostTeam T;
  std::vector<double> col((size_t)N + 1);
  return ba::ldlt_solve(T, A, N, rhs, col.data(), x) ? 1 : 0;
}

}  // extern "C"

#ifdef ESSENTIAL_EMU_MAIN
#include <cstdio>

// the committed scene list (tests/golden/essential_scenes.bin, written by tests/essential_model.py's dump): int32 count; per scene int32
// K, E, P, fixed, n_iterations; int32 mnId [K]; double Scw [K][8]; double Scw_normal [K][8]; int32 i [E]; int32 j [E]; uint8 connection [E];
// float points [P][3]; int32 ref [P]
int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t count = 0;
  int bad = std::fread(&count, 4, 1, f) != 1 || count < 0 || count > 1000;
  for (int s = 0; s < count && !bad; ++s) {
    int32_t h[5];
    if (std::fread(h, 4, 5, f) != 5 || h[0] < 1 || h[0] > essential::kMaxKeyframes || h[1] < 0 || h[1] > essential::kMaxEdges || h[2] < 0 || h[2] > 100000) {
      bad = 1;
      break;
    }
    const size_t K = (size_t)h[0], E = (size_t)h[1], P = (size_t)h[2];
    std::vector<int32_t> id(K), ei(E + 1), ej(E + 1), ref(P + 1);
    std::vector<uvo_sim3d> S(K), Sn(K), So(K);
    std::vector<uint8_t> conn(E + 1);
    std::vector<float> pts(3 * P + 1), To(16 * K), po(3 * P + 1);
    bad = std::fread(id.data(), 4, K, f) != K || std::fread(S.data(), 64, K, f) != K || std::fread(Sn.data(), 64, K, f) != K || std::fread(ei.data(), 4, E, f) != E ||
          std::fread(ej.data(), 4, E, f) != E || std::fread(conn.data(), 1, E, f) != E || std::fread(pts.data(), 12, P, f) != P || std::fread(ref.data(), 4, P, f) != P;
    if (bad) break;
    const uvo_essential_problem q = {h[0], h[1], h[2], h[3], S.data(), Sn.data(), ei.data(), ej.data(), conn.data(), pts.data(), ref.data(), h[4]};
    uvo_essential_result r = {So.data(), To.data(), po.data(), -1, -1, -1, -1};
    static uvo_essential_trace tr;
    const int rc = emu_essential_optimize(&q, kAnyBlocks, &r, &tr);
    std::printf("scene %d: K %d E %d P %d rc %d blocks %d iterations %d trials %d\n", s, h[0], h[1], h[2], rc, r.envelope_blocks, r.iterations, r.n_trials);
    bad = rc != 0 || r.iterations < 0 || r.iterations > 32 || r.n_trials > 320 || tr.n_trials != r.n_trials || r.envelope_blocks < h[0] - 1;
  }
  std::fclose(f);
  std::printf("%s\n", bad ? "FAILED" : "ok");
  return bad ? 1 : 0;
}
#endif
