// cv::findFundamentalMat(pts0_Un, pts1_Un, cv::FM_RANSAC, 1, 0.999, mask_rsc), src/Tracking.cc:1062 (OpenCV 3.4 calib3d fundam.cpp,
// ptsetreg.cpp, core mathfuncs.cpp; recalled, not read: tests/fundamental_model.py lists every recalled detail [OCV-RECALL]).
// Four steps in the tracker handle's stream, all scratch sized at uvo_klt_create:
//   k_fm_subsets : the RNG stream and getSubset, one workgroup.  cv::RNG is a multiply-with-carry generator whose states from the
//       third on are A^k * S_2 mod M (M = A * 2^32 - 1), so every lane starts its run of draws with one modular product by a jump
//       constant the host computed once.  For every position of a window of draws the attempt starting there is parsed (its
//       length with the duplicate redraws, the collinearity verdict); the chain of attempts from the window's first position is
//       found by pointer jumping in LDS, and one wave walks it with ballots: consecutive failures against the attempt limit, passes
//       become hypotheses.  All hypotheses up to maxIters are drawn (speculatively: the replay decides how many count).
//   k_fm_models  : run7Point, one lane per hypothesis, in double.  The null space of the 7 x 9 system comes from a Householder QR
//       of its transpose -- backward stable like OpenCV's SVD; the normal equations A^T A are not -- then OpenCV's cubic and
//       root scaling.  A different basis of the same null space: F agrees to rounding, the order of the roots may not.
//   k_fm_score_ransac / _lmeds : one wave per model over all points: inlier count by ballot, or (n <= 14) the median by ranking
//       the error bits across the lanes (std::nth_element on the floats read as int).
//   k_fm_replay  : one wave walks the models in draw order.  Acceptances are the strict running maxima above 6 (RANSAC) or the
//       strict running minima (LMedS), so a prefix scan finds them; the few records are then replayed in order with
//       RANSACUpdateNumIters, which fixes the stop, the iteration count and the draws consumed.  Then the winner's mask, F, info.
#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>

#include "devmem.hpp"
#include "fundamental.hpp"

namespace uvo {

constexpr uint64_t kMwcA = 4164903690ull;
constexpr uint64_t kMwcM = (kMwcA << 32) - 1;
constexpr int kFmT = 1024;           // k_fm_subsets workgroup
constexpr int kFmP = 2;              // draws per lane and window
constexpr int kFmD = kFmT * kFmP;    // draws per window
constexpr int kFmMaxAtt = kFmD / 7;  // attempts per window (each takes >= 7 draws)
constexpr int kFmRounds = 9;         // pointer-jumping rounds: 2^9 > kFmMaxAtt
static_assert(kFmP == 2, "the compaction in k_fm_subsets handles two positions per lane");
static_assert((1 << kFmRounds) > kFmMaxAtt, "pointer jumping must cover a window's chain");

struct FmState {
  int32_t n_hyp;      // subsets drawn
  int32_t fail;       // getSubset ran out of attempts after n_hyp subsets
  uint32_t fail_end;  // draws consumed when it did
  int32_t overflow;   // an attempt needed more draws than a window holds (the call fails)
};

__device__ __forceinline__ uint64_t mwc_next(uint64_t s) { return (s & 0xffffffffull) * kMwcA + (s >> 32); }

__device__ __forceinline__ uint64_t addmod_m(uint64_t a, uint64_t b) {  // a, b < M
  const uint64_t s = a + b;
  return (s < a || s >= kMwcM) ? s - kMwcM : s;
}

__device__ uint64_t mulmod_m(uint64_t a, uint64_t b) {  // a, b < M: a * b mod M by doubling (no 128-bit division on the device)
  uint64_t r = 0;
  for (int bit = 63; bit >= 0; --bit) {
    r = addmod_m(r, r);
    if ((b >> bit) & 1) r = addmod_m(r, a);
  }
  return r;
}

// getSubset's seven indices for the attempt starting at window position p (each index redrawn while it repeats an earlier one);
// returns the draws it takes, 0 when it runs past the window
__device__ __forceinline__ int fm_parse_attempt(const int32_t* s_idx, int p, int (&ch)[7]) {
  int q = p;
  ch[0] = s_idx[q++];
#pragma unroll
  for (int i = 1; i < 7; ++i) {
    int v = -1;
    for (;;) {
      if (q >= kFmD) return 0;
      v = s_idx[q++];
      bool dup = false;
#pragma unroll
      for (int j = 0; j < i; ++j) dup |= v == ch[j];
      if (!dup) break;
    }
    ch[i] = v;
  }
  return q - p;
}

// haveCollinearPoints: the last point against every pair of the six before it; Point2f differences (float), double products
__device__ __forceinline__ bool fm_collinear(const float (&x)[7], const float (&y)[7]) {
  bool col = false;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    const double dx1 = (double)(x[j] - x[6]), dy1 = (double)(y[j] - y[6]);
#pragma unroll
    for (int k = 0; k < j; ++k) {
      const double dx2 = (double)(x[k] - x[6]), dy2 = (double)(y[k] - y[6]);
      col |= fabs(dx2 * dy1 - dy2 * dx1) <= (double)FLT_EPSILON * (fabs(dx1) + fabs(dy1) + fabs(dx2) + fabs(dy2));
    }
  }
  return col;
}

__global__ __launch_bounds__(kFmT) void k_fm_subsets(const float2* __restrict__ p0, const float2* __restrict__ p1, int n, int cap, int max_att,
                                                     int seven, const uint64_t* __restrict__ jump, int32_t* __restrict__ subsets,
                                                     uint32_t* __restrict__ hyp_end, FmState* __restrict__ st) {
  __shared__ uint64_t s_st[kFmD];    // RNG state behind each draw of the window
  __shared__ int32_t s_idx[kFmD];    // the draw % n
  __shared__ uint16_t s_info[kFmD];  // length of the attempt starting here | passes << 15; 0: it runs past the window
  __shared__ int16_t s_jmp[2][kFmD];
  __shared__ uint8_t s_mark[kFmD];
  __shared__ int16_t s_att[kFmMaxAtt + 1];
  __shared__ int32_t s_wsum[kFmT / 64];
  __shared__ int32_t s_next, s_done;
  const int t = threadIdx.x, lane = t & 63, wave = wave_in_block();
  if (seven) {  // n == 7: the kernel runs once on all points
    if (t < 7) subsets[t] = t;
    if (t == 0) *st = FmState{1, 0, 0, 0};
    return;
  }
  uint64_t base = mwc_next(~0ull);  // the state behind draw 0 (S_1 > M: it is the only one)
  uint32_t ws = 0;                  // first draw of the window
  int n_hyp = 0, run = 0;           // wave 0: hypotheses so far, failed attempts since the last pass
  for (;;) {
    {  // 1. the window's draws: lane t owns positions t*P .. t*P + P-1
      uint64_t s = base;
      if (t > 0) s = mulmod_m(jump[t], base >= kMwcM ? base - kMwcM : base);
      for (int q = 0; q < kFmP; ++q) {
        s_st[t * kFmP + q] = s;
        s_idx[t * kFmP + q] = (int32_t)((uint32_t)s % (uint32_t)n);
        s = mwc_next(s);
      }
    }
    __syncthreads();
    // 2. the attempt starting at every position
    for (int q = 0; q < kFmP; ++q) {
      const int p = t * kFmP + q;
      int ch[7];
      const int len = fm_parse_attempt(s_idx, p, ch);
      int pass = 0;
      if (len) {
        float x0[7], y0[7], x1[7], y1[7];
#pragma unroll
        for (int i = 0; i < 7; ++i) {
          const float2 a = p0[ch[i]], b = p1[ch[i]];
          x0[i] = a.x, y0[i] = a.y, x1[i] = b.x, y1[i] = b.y;
        }
        pass = !fm_collinear(x0, y0) && !fm_collinear(x1, y1);
      }
      s_info[p] = (uint16_t)(len | pass << 15);
      s_jmp[0][p] = (int16_t)((len && p + len < kFmD) ? p + len : kFmD);
      s_mark[p] = p == 0;
    }
    __syncthreads();
    // 3. the chain of attempts from position 0: after round r every position fewer than 2^(r+1) attempts away is marked
    int cur = 0;
    for (int r = 0; r < kFmRounds; ++r) {
      int nj[kFmP];
      for (int q = 0; q < kFmP; ++q) {
        const int p = t * kFmP + q, j = s_jmp[cur][p];
        nj[q] = kFmD;
        if (j < kFmD) {
          if (s_mark[p]) s_mark[j] = 1;
          nj[q] = s_jmp[cur][j];
        }
      }
      for (int q = 0; q < kFmP; ++q) s_jmp[cur ^ 1][t * kFmP + q] = (int16_t)nj[q];
      cur ^= 1;
      __syncthreads();
    }
    // 4. the attempts on the chain in draw order, and where the next window starts
    int c[kFmP];
    for (int q = 0; q < kFmP; ++q) {
      const int p = t * kFmP + q, len = s_info[p] & 0x7fff;
      c[q] = s_mark[p] && len;
      if (s_mark[p] && (!len || p + len >= kFmD)) s_next = len ? p + len : p;  // the chain's last position
    }
    const uint64_t lt = (1ull << lane) - 1;
    const uint64_t b0 = __ballot(c[0]), b1 = __ballot(c[1]);
    int off = __builtin_popcountll(b0 & lt) + __builtin_popcountll(b1 & lt);
    if (lane == 0) s_wsum[wave] = __builtin_popcountll(b0) + __builtin_popcountll(b1);
    __syncthreads();
    int total = 0;
    for (int w = 0; w < kFmT / 64; ++w) {
      const int v = s_wsum[w];
      if (w < wave) off += v;
      total += v;
    }
    if (c[0]) s_att[off] = (int16_t)(t * kFmP);
    if (c[1]) s_att[off + c[0]] = (int16_t)(t * kFmP + 1);
    __syncthreads();
    // 5. wave 0 walks them: passes become hypotheses until the cap; max_att failures in a row end getSubset
    if (wave == 0) {
      int done = 0, fail = 0, overflow = 0;
      uint32_t fail_end = 0;
      for (int a0 = 0; a0 < total && !done; a0 += 64) {
        const int a = a0 + lane;
        const bool valid = a < total;
        const int p = valid ? s_att[a] : 0;
        const int info = valid ? s_info[p] : 0;
        const bool pass = valid && (info >> 15);
        const uint64_t pm = __ballot(pass), vm = __ballot(valid);
        const uint64_t upto = pm & (lane == 63 ? ~0ull : ((2ull << lane) - 1));
        const int runl = upto ? lane - (63 - __builtin_clzll(upto)) : run + lane + 1;  // failures in a row up to this attempt
        const uint64_t hm = __ballot(valid && !pass && runl >= max_att);
        const int hl = hm ? __builtin_ctzll(hm) : 64;  // getSubset gives up at this attempt
        const int rank = __builtin_popcountll(pm & lt);
        const bool take = pass && lane < hl && rank < cap - n_hyp;
        if (take) {
          const int h = n_hyp + rank;
          int ch[7];
          const int len = fm_parse_attempt(s_idx, p, ch);
#pragma unroll
          for (int i = 0; i < 7; ++i) subsets[h * 7 + i] = ch[i];
          hyp_end[h] = ws + (uint32_t)(p + len);
        }
        n_hyp += __builtin_popcountll(__ballot(take));
        const int hp = __shfl(p, hl & 63), hlen = __shfl(info & 0x7fff, hl & 63);
        if (n_hyp >= cap) {
          done = 1;
        } else if (hm) {
          done = 1, fail = 1, fail_end = ws + (uint32_t)(hp + hlen);
        } else {
          run = pm ? (63 - __builtin_clzll(vm)) - (63 - __builtin_clzll(pm)) : run + __builtin_popcountll(vm);
        }
      }
      if (!done && s_next == 0) done = 1, overflow = 1;  // the window's first attempt alone is longer than the window
      if (lane == 0) {
        s_done = done;
        if (done) *st = FmState{n_hyp, fail, fail_end, overflow};
      }
    }
    __syncthreads();
    if (s_done) return;
    const int nx = s_next;
    base = nx < kFmD ? s_st[nx] : mwc_next(s_st[kFmD - 1]);
    ws += (uint32_t)nx;
    __syncthreads();  // the next window overwrites s_st
  }
}

__device__ int fm_solve_cubic(double a0, double a1, double a2, double a3, double (&x)[3]) {  // cv::solveCubic, double coefficients
  int n = 0;
  double x0 = 0., x1 = 0., x2 = 0.;
  if (a0 == 0) {
    if (a1 == 0) {
      if (a2 == 0)
        n = a3 == 0 ? -1 : 0;
      else
        x0 = -a3 / a2, n = 1;
    } else {
      double d = a2 * a2 - 4 * a1 * a3;
      if (d >= 0) {
        d = sqrt(d);
        const double q1 = (-a2 + d) * 0.5, q2 = (a2 + d) * -0.5;
        if (fabs(q1) > fabs(q2))
          x0 = q1 / a1, x1 = a3 / q1;
        else
          x0 = q2 / a1, x1 = a3 / q2;
        n = d > 0 ? 2 : 1;
      }
    }
  } else {
    a0 = 1. / a0;
    a1 *= a0, a2 *= a0, a3 *= a0;
    const double Q = (a1 * a1 - 3 * a2) * (1. / 9);
    const double R = (2 * a1 * a1 * a1 - 9 * a1 * a2 + 27 * a3) * (1. / 54);
    const double Qcubed = Q * Q * Q;
    double d = Qcubed - R * R;
    const double pi = 3.1415926535897932384626433832795;
    if (d > 0) {
      const double theta = acos(R / sqrt(Qcubed));
      const double sqrtQ = sqrt(Q);
      const double t0 = -2 * sqrtQ, t1 = theta * (1. / 3), t2 = a1 * (1. / 3);
      x0 = t0 * cos(t1) - t2;
      x1 = t0 * cos(t1 + (2. * pi / 3)) - t2;
      x2 = t0 * cos(t1 - (2. * pi / 3)) - t2;
      n = 3;
    } else if (d == 0) {
      if (R >= 0) {
        x0 = -2 * pow(R, 1. / 3) - a1 / 3;
        x1 = pow(R, 1. / 3) - a1 / 3;
      } else {
        x0 = 2 * pow(-R, 1. / 3) - a1 / 3;
        x1 = -pow(-R, 1. / 3) - a1 / 3;
      }
      x2 = 0;
      n = x0 == x1 ? 1 : 2;
      x1 = x0 == x1 ? 0 : x1;
    } else {
      d = sqrt(-d);
      double e = pow(d + fabs(R), 1. / 3);
      if (R > 0) e = -e;
      x0 = (e + Q / e) - a1 * (1. / 3);
      n = 1;
    }
  }
  x[0] = x0, x[1] = x1, x[2] = x2;
  return n;
}

__global__ __launch_bounds__(64) void k_fm_models(const float2* __restrict__ p0, const float2* __restrict__ p1, const int32_t* __restrict__ subsets,
                                                  const FmState* __restrict__ st, int cap, double* __restrict__ models, int32_t* __restrict__ nmodels) {
  const int h = blockIdx.x * 64 + threadIdx.x;
  if (h >= cap || h >= st->n_hyp) return;
  double m[9][7];  // the transpose of OpenCV's 7 x 9 system: column c = the row of point c
#pragma unroll
  for (int c = 0; c < 7; ++c) {
    const int i = subsets[h * 7 + c];
    const double x0 = p0[i].x, y0 = p0[i].y, x1 = p1[i].x, y1 = p1[i].y;
    m[0][c] = x1 * x0, m[1][c] = x1 * y0, m[2][c] = x1, m[3][c] = y1 * x0, m[4][c] = y1 * y0, m[5][c] = y1;
    m[6][c] = x0, m[7][c] = y0, m[8][c] = 1.;
  }
  // Householder QR: H_c = I - beta_c v v^T zeroes m[c+1..8][c]; v[c] = 1, v[c+1..8] kept in m[c+1..8][c]
  double beta[7];
#pragma unroll
  for (int c = 0; c < 7; ++c) {
    double sigma = 0.;
#pragma unroll
    for (int r = c + 1; r < 9; ++r) sigma += m[r][c] * m[r][c];
    const double x = m[c][c];
    double b = 0.;
    if (sigma != 0.) {
      const double mu = sqrt(x * x + sigma);
      const double v0 = x <= 0. ? x - mu : -sigma / (x + mu);
      b = 2. * v0 * v0 / (sigma + v0 * v0);
      const double iv0 = 1. / v0;
#pragma unroll
      for (int r = c + 1; r < 9; ++r) m[r][c] *= iv0;
#pragma unroll
      for (int j = c + 1; j < 7; ++j) {
        double w = m[c][j];
#pragma unroll
        for (int r = c + 1; r < 9; ++r) w += m[r][c] * m[r][j];
        w *= b;
        m[c][j] -= w;
#pragma unroll
        for (int r = c + 1; r < 9; ++r) m[r][j] -= w * m[r][c];
      }
    }
    beta[c] = b;
  }
  // columns 7 and 8 of Q = H_0 ... H_6: a basis of the null space (OpenCV: the last two rows of Vt)
  double f1[9], f2[9];
#pragma unroll
  for (int r = 0; r < 9; ++r) f1[r] = r == 7 ? 1. : 0., f2[r] = r == 8 ? 1. : 0.;
#pragma unroll
  for (int c = 6; c >= 0; --c) {
    double w1 = f1[c], w2 = f2[c];
#pragma unroll
    for (int r = c + 1; r < 9; ++r) w1 += m[r][c] * f1[r], w2 += m[r][c] * f2[r];
    w1 *= beta[c], w2 *= beta[c];
    f1[c] -= w1, f2[c] -= w2;
#pragma unroll
    for (int r = c + 1; r < 9; ++r) f1[r] -= w1 * m[r][c], f2[r] -= w2 * m[r][c];
  }
  // run7Point from here on, operation for operation
#pragma unroll
  for (int i = 0; i < 9; ++i) f1[i] -= f2[i];
  double t0 = f2[4] * f2[8] - f2[5] * f2[7];
  double t1 = f2[3] * f2[8] - f2[5] * f2[6];
  double t2 = f2[3] * f2[7] - f2[4] * f2[6];
  const double c3 = f2[0] * t0 - f2[1] * t1 + f2[2] * t2;
  const double c2 = f1[0] * t0 - f1[1] * t1 + f1[2] * t2 - f1[3] * (f2[1] * f2[8] - f2[2] * f2[7]) + f1[4] * (f2[0] * f2[8] - f2[2] * f2[6]) -
                    f1[5] * (f2[0] * f2[7] - f2[1] * f2[6]) + f1[6] * (f2[1] * f2[5] - f2[2] * f2[4]) - f1[7] * (f2[0] * f2[5] - f2[2] * f2[3]) +
                    f1[8] * (f2[0] * f2[4] - f2[1] * f2[3]);
  t0 = f1[4] * f1[8] - f1[5] * f1[7];
  t1 = f1[3] * f1[8] - f1[5] * f1[6];
  t2 = f1[3] * f1[7] - f1[4] * f1[6];
  const double c1 = f2[0] * t0 - f2[1] * t1 + f2[2] * t2 - f2[3] * (f1[1] * f1[8] - f1[2] * f1[7]) + f2[4] * (f1[0] * f1[8] - f1[2] * f1[6]) -
                    f2[5] * (f1[0] * f1[7] - f1[1] * f1[6]) + f2[6] * (f1[1] * f1[5] - f1[2] * f1[4]) - f2[7] * (f1[0] * f1[5] - f1[2] * f1[3]) +
                    f2[8] * (f1[0] * f1[4] - f1[1] * f1[3]);
  const double c0 = f1[0] * t0 - f1[1] * t1 + f1[2] * t2;
  double r[3];
  const int nr = fm_solve_cubic(c0, c1, c2, c3, r);
  if (nr >= 1 && nr <= 3) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      if (k >= nr) break;
      double lambda = r[k], mu = 1.;
      const double s = f1[8] * r[k] + f2[8];
      double* F = models + ((size_t)h * 3 + k) * 9;
      if (fabs(s) > DBL_EPSILON) {
        mu = 1. / s;
        lambda *= mu;
        F[8] = 1.;
      } else {
        F[8] = 0.;
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) F[i] = f1[i] * lambda + f2[i] * mu;
    }
  }
  nmodels[h] = nr;
}

// FMEstimatorCallback::computeError for one pair, in double; std::max(a, b) = a < b ? b : a
__device__ __forceinline__ float fm_error(const double* __restrict__ F, float2 m1, float2 m2) {
  double a = F[0] * m1.x + F[1] * m1.y + F[2];
  double b = F[3] * m1.x + F[4] * m1.y + F[5];
  double c = F[6] * m1.x + F[7] * m1.y + F[8];
  const double s2 = 1. / (a * a + b * b);
  const double d2 = m2.x * a + m2.y * b + c;
  a = F[0] * m2.x + F[3] * m2.y + F[6];
  b = F[1] * m2.x + F[4] * m2.y + F[7];
  c = F[2] * m2.x + F[5] * m2.y + F[8];
  const double s1 = 1. / (a * a + b * b);
  const double d1 = m1.x * a + m1.y * b + c;
  const double e1 = d1 * d1 * s1, e2 = d2 * d2 * s2;
  return (float)(e1 < e2 ? e2 : e1);
}

// one wave per (hypothesis, model): the number of errors <= t
__global__ __launch_bounds__(256) void k_fm_score_ransac(const float2* __restrict__ p0, const float2* __restrict__ p1, int n, float t,
                                                         const FmState* __restrict__ st, int cap, const int32_t* __restrict__ nmodels,
                                                         const double* __restrict__ models, double* __restrict__ scores) {
  const int g = blockIdx.x * 4 + wave_in_block(), lane = threadIdx.x & 63;
  const int h = g / 3, k = g - 3 * h;
  if (h >= cap || h >= st->n_hyp) return;
  if (k >= nmodels[h]) {
    if (lane == 0) scores[g] = -1.;
    return;
  }
  const double* F = models + (size_t)g * 9;
  int cnt = 0;
  for (int i0 = 0; i0 < n; i0 += 64) {
    const int i = i0 + lane;
    cnt += __builtin_popcountll(__ballot(i < n && fm_error(F, p0[i], p1[i]) <= t));
  }
  if (lane == 0) scores[g] = (double)cnt;
}

// n <= 14: one wave per (hypothesis, model), lane i holds error i; the median is the error of rank n/2 in int order
__global__ __launch_bounds__(256) void k_fm_score_lmeds(const float2* __restrict__ p0, const float2* __restrict__ p1, int n,
                                                        const FmState* __restrict__ st, int cap, const int32_t* __restrict__ nmodels,
                                                        const double* __restrict__ models, double* __restrict__ scores) {
  const int g = blockIdx.x * 4 + wave_in_block(), lane = threadIdx.x & 63;
  const int h = g / 3, k = g - 3 * h;
  if (h >= cap || h >= st->n_hyp) return;
  if (k >= nmodels[h]) {
    if (lane == 0) scores[g] = -1.;
    return;
  }
  const double* F = models + (size_t)g * 9;
  const int32_t e = lane < n ? __float_as_int(fm_error(F, p0[lane], p1[lane])) : INT_MAX;
  int rank = 0;
  for (int j = 0; j < n; ++j) {
    const int32_t o = __shfl(e, j);
    rank += (o < e) || (o == e && j < lane);
  }
  const uint64_t m = __ballot(lane < n && rank == n / 2);
  const int32_t med = __shfl(e, __builtin_ctzll(m));
  if (lane == 0) scores[g] = (double)__int_as_float(med);
}

// RANSACUpdateNumIters (MAX / MIN as OpenCV's macros)
__host__ __device__ int fm_update_iters(double p, double ep, int model_points, int max_iters) {
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

struct FmReplay {
  const float2 *p0, *p1;
  const uint8_t* status;
  const FmState* st;
  const int32_t* nmodels;
  const double *models, *scores;
  const uint32_t* hyp_end;
  FmOut* out;
  uint8_t* mask;
  int n, method, niters0;
  float t;
  double conf;
};

__global__ __launch_bounds__(64) void k_fm_replay(FmReplay a) {
  const int lane = threadIdx.x;
  const FmState st = *a.st;
  const bool ransac = a.method == UVO_FM_RANSAC, lmeds = a.method == UVO_FM_LMEDS, seven = !ransac && !lmeds;
  int best = -1, iterations = 0;
  uint32_t draws = 0;
  if (seven) {
    best = a.nmodels[0] >= 1 ? 0 : -1;
  } else if (!st.overflow) {
    const int nh = st.n_hyp;
    int niters = a.niters0, hcur = -1;
    double carry = ransac ? 6. : DBL_MAX;  // the level a score must beat: max(best, modelPoints - 1), resp. minMedian
    bool stopped = false;
    // past hypothesis max(niters, hcur + 1) the loop has ended whatever comes later: the walk stops there
    for (int s0 = 0; s0 < 3 * min(nh, max(niters, hcur + 1)) && !stopped; s0 += 64) {
      const int s = s0 + lane, h = s / 3, k = s - 3 * h;
      double sc = ransac ? -1. : INFINITY;
      if (h < nh && k < a.nmodels[h]) {
        const double v = a.scores[s];
        sc = ransac || v == v ? v : INFINITY;  // a NaN median never wins
      }
      double pm = sc;  // running max (RANSAC) / min (LMedS) over the lanes up to this one
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const double o = __shfl_up(pm, off);
        if (lane >= off) pm = ransac ? (o > pm ? o : pm) : (o < pm ? o : pm);
      }
      double ex = __shfl_up(pm, 1);
      ex = lane == 0 ? carry : ransac ? (ex > carry ? ex : carry) : (ex < carry ? ex : carry);
      uint64_t rec = __ballot(ransac ? sc > ex : sc < ex);
      while (rec) {  // the acceptances of this chunk, in order
        const int r = __builtin_ctzll(rec);
        const int hr = __shfl(h, r);
        const double cr = __shfl(sc, r);
        if (hr != hcur && hr >= niters) {  // the loop ended before this hypothesis
          stopped = true;
          break;
        }
        best = s0 + r, hcur = hr;
        if (ransac) niters = fm_update_iters(a.conf, (double)(a.n - (int)cr) / a.n, 7, niters);
        rec &= rec - 1;
      }
      const double last = __shfl(pm, 63);
      carry = ransac ? (last > carry ? last : carry) : (last < carry ? last : carry);
    }
    const int it = ransac ? max(niters, hcur + 1) : niters;
    if (st.fail && nh < it) {
      iterations = nh, draws = st.fail_end;
    } else {
      iterations = it, draws = a.hyp_end[it - 1];
    }
  }
  const double* Fb = best >= 0 ? a.models + (size_t)best * 9 : nullptr;
  float thr = a.t;
  if (lmeds && best >= 0) {
    double sigma = 2.5 * 1.4826 * (1 + 5. / (a.n - 7)) * sqrt(a.scores[best]);
    sigma = sigma < 0.001 ? 0.001 : sigma;
    thr = (float)(sigma * sigma);
  }
  int cnt = 0;
  for (int i0 = 0; i0 < a.n; i0 += 64) {
    const int i = i0 + lane;
    bool inl = false;
    if (i < a.n) {
      inl = seven || (Fb && fm_error(Fb, a.p0[i], a.p1[i]) <= thr);
      a.mask[i] = (inl && (!a.status || a.status[i])) ? 1 : 0;
    }
    cnt += __builtin_popcountll(__ballot(inl));
  }
  const bool hasF = best >= 0 && (!lmeds || cnt >= 7);
  if (lane < 9) a.out->F[lane] = hasF ? Fb[lane] : 0.;
  if (lane == 0) {
    a.out->method = a.method, a.out->iterations = iterations, a.out->inliers = seven || best >= 0 ? cnt : 0;
    a.out->rng_draws = draws, a.out->overflow = st.overflow;
  }
}

int fm_alloc(DevMem& m, FmScratch& f) {
  RC(alloc_carved(m, [&](Carve& c) {
    c.take(f.state, 1, 64).take(f.subsets, kFmCap * 7, 64).take(f.hyp_end, kFmCap, alignof(uint32_t)).take(f.nmodels, kFmCap, alignof(int32_t));
    c.take(f.models, kFmCap * 27, 64).take(f.scores, kFmCap * 3, alignof(double)).take(f.jump, kFmT, alignof(uint64_t));
  }));
  // lane t of k_fm_subsets starts kFmP * t draws into the window: A^(kFmP * t) mod M, with 128-bit host arithmetic
  uint64_t jump[kFmT];
  unsigned __int128 step = 1;
  for (int i = 0; i < kFmP; ++i) step = step * kMwcA % kMwcM;
  unsigned __int128 j = 1;
  for (int t = 0; t < kFmT; ++t) {
    jump[t] = (uint64_t)j;
    j = j * step % kMwcM;
  }
  UVO_HIP_CHECK(hipMemcpy(f.jump, jump, sizeof jump, hipMemcpyHostToDevice));
  return UVO_OK;
}

int fm_fixup(double& thr, double& conf) {
  if (!(thr == thr) || !(conf == conf)) return fail(UVO_E_BADARG, "NaN threshold or confidence");
  if (thr <= 0) thr = 3;
  if (conf < DBL_EPSILON || conf > 1 - DBL_EPSILON) conf = 0.99;
  return UVO_OK;
}

int fm_enqueue(hipStream_t s, const FmScratch& f, const float* d_p0, const float* d_p1, int n, double thr, double conf, const uint8_t* d_status,
               FmOut* d_out, uint8_t* d_mask) {
  const int method = n == 7 ? UVO_FM_SEVEN_POINT : n <= 14 ? UVO_FM_LMEDS : UVO_FM_RANSAC;
  const int cap = method == UVO_FM_SEVEN_POINT ? 1 : method == UVO_FM_LMEDS ? std::max(fm_update_iters(conf, 0.45, 7, kFmCap), 3) : kFmCap;
  const float2* a = reinterpret_cast<const float2*>(d_p0);
  const float2* b = reinterpret_cast<const float2*>(d_p1);
  hipLaunchKernelGGL(k_fm_subsets, dim3(1), dim3(kFmT), 0, s, a, b, n, cap, method == UVO_FM_RANSAC ? 10000 : 1000, method == UVO_FM_SEVEN_POINT ? 1 : 0,
                     f.jump, f.subsets, f.hyp_end, f.state);
  hipLaunchKernelGGL(k_fm_models, dim3((cap + 63) / 64), dim3(64), 0, s, a, b, f.subsets, f.state, cap, f.models, f.nmodels);
  const dim3 gs((cap * 3 + 3) / 4);
  const float t = (float)(thr * thr);
  if (method == UVO_FM_RANSAC)
    hipLaunchKernelGGL(k_fm_score_ransac, gs, dim3(256), 0, s, a, b, n, t, f.state, cap, f.nmodels, f.models, f.scores);
  else if (method == UVO_FM_LMEDS)
    hipLaunchKernelGGL(k_fm_score_lmeds, gs, dim3(256), 0, s, a, b, n, f.state, cap, f.nmodels, f.models, f.scores);
  const FmReplay r{a, b, d_status, f.state, f.nmodels, f.models, f.scores, f.hyp_end, d_out, d_mask, n, method, cap, t, conf};
  hipLaunchKernelGGL(k_fm_replay, dim3(1), dim3(64), 0, s, r);
  UVO_HIP_CHECK(hipGetLastError());
  return UVO_OK;
}

}  // namespace uvo
