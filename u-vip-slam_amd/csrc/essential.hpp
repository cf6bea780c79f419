// The essential-graph optimiser's host exchange (essential.hip; arithmetic and launch sequence in essential_core.hpp): one
// description of the arrays a call sends up -- the caller's lists and what essential::derive works out of them -- and of what it brings
// down, placed alike on the device and in the page-locked mirror.  The device's team, the kernel of a phase and the executor are
// ba.hpp's.
#pragma once
#include "ba.hpp"
#include "essential_core.hpp"

namespace uvo {

#define UVO_ESS_COPY(dst, src, field, count, kind) \
  if ((size_t)(count) > 0) UVO_HIP_CHECK(hipMemcpyAsync((dst).field, (src).field, sizeof(*(src).field) * (size_t)(count), kind, st))

struct EssGraph {
  essential::Sim *Scw, *Scwn;
  int32_t *e_i, *e_j;
  uint8_t* e_conn;
  float* pts;
  int32_t *pt_ref, *kf_free, *inc_begin, *inc_edge, *pair_begin, *pair_rc, *pair_edge, *first, *env_off, *col_begin, *col_rows, *blk_row;

  void layout(Carve& c, size_t K, size_t E, size_t P, size_t NB) {
    c.take(Scw, K).take(Scwn, K).take(e_i, E).take(e_j, E).take(e_conn, E).take(pts, 3 * P).take(pt_ref, P).take(kf_free, K);
    c.take(inc_begin, K + 1).take(inc_edge, 2 * E).take(pair_begin, E + 1).take(pair_rc, 2 * E).take(pair_edge, E);
    c.take(first, K).take(env_off, K + 1).take(col_begin, K + 1).take(col_rows, NB).take(blk_row, NB);
  }
  void bind(essential::Ws& W) const {
    W.Scw = Scw, W.Scwn = Scwn, W.e_i = e_i, W.e_j = e_j, W.e_conn = e_conn, W.pts = pts, W.pt_ref = pt_ref, W.kf_free = kf_free;
    W.inc_begin = inc_begin, W.inc_edge = inc_edge, W.pair_begin = pair_begin, W.pair_rc = pair_rc, W.pair_edge = pair_edge;
    W.first = first, W.env_off = env_off, W.col_begin = col_begin, W.col_rows = col_rows, W.blk_row = blk_row;
  }
  // the mirror (this) to the device: one copy per array that is not empty
  int send(const EssGraph& dev, const essential::Dims& d, hipStream_t st) const {
    const size_t K = (size_t)d.K, E = (size_t)d.E, P = (size_t)d.P, F = (size_t)d.F, NB = (size_t)d.NB;
    UVO_ESS_COPY(dev, *this, Scw, K, hipMemcpyHostToDevice);
    UVO_ESS_COPY(dev, *this, Scwn, K, hipMemcpyHostToDevice);
    UVO_ESS_COPY(dev, *this, e_i, E, hipMemcpyHostToDevice);
    UVO_ESS_COPY(dev, *this, e_j, E, hipMemcpyHostToDevice);
    UVO_ESS_COPY(dev, *this, e_conn, E, hipMemcpyHostToDevice);
    UVO_ESS_COPY(dev, *this, pts, 3 * P, hipMemcpyHostToDevice);
    UVO_ESS_COPY(dev, *this, pt_ref, P, hipMemcpyHostToDevice);
    UVO_ESS_COPY(dev, *this, kf_free, K, hipMemcpyHostToDevice);
    UVO_ESS_COPY(dev, *this, inc_begin, F + 1, hipMemcpyHostToDevice);
    UVO_ESS_COPY(dev, *this, inc_edge, 2 * E, hipMemcpyHostToDevice);
    UVO_ESS_COPY(dev, *this, pair_begin, (size_t)d.NP + 1, hipMemcpyHostToDevice);
    UVO_ESS_COPY(dev, *this, pair_rc, 2 * (size_t)d.NP, hipMemcpyHostToDevice);
    UVO_ESS_COPY(dev, *this, pair_edge, E, hipMemcpyHostToDevice);
    UVO_ESS_COPY(dev, *this, first, F, hipMemcpyHostToDevice);
    UVO_ESS_COPY(dev, *this, env_off, F + 1, hipMemcpyHostToDevice);
    UVO_ESS_COPY(dev, *this, col_begin, F + 1, hipMemcpyHostToDevice);
    UVO_ESS_COPY(dev, *this, col_rows, NB > F ? NB - F : 0, hipMemcpyHostToDevice);
    UVO_ESS_COPY(dev, *this, blk_row, NB, hipMemcpyHostToDevice);
    return UVO_OK;
  }
};

struct EssAnswer {
  essential::Sim* Scw_out;
  float *kf_T_out, *pt_out;
  ba::Ctl* ctl;

  void layout(Carve& c, size_t K, size_t P) { c.take(Scw_out, K).take(kf_T_out, 16 * K).take(pt_out, 3 * P).take(ctl, 1); }
  // the device's (dev) to the mirror (this); the caller synchronises
  int receive(const EssAnswer& dev, int K, int P, hipStream_t st) const {
    UVO_ESS_COPY(*this, dev, Scw_out, K, hipMemcpyDeviceToHost);
    UVO_ESS_COPY(*this, dev, kf_T_out, 16 * (size_t)K, hipMemcpyDeviceToHost);
    UVO_ESS_COPY(*this, dev, pt_out, 3 * (size_t)P, hipMemcpyDeviceToHost);
    UVO_ESS_COPY(*this, dev, ctl, 1, hipMemcpyDeviceToHost);
    return UVO_OK;
  }
};

#undef UVO_ESS_COPY

}  // namespace uvo
