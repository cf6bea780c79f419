// Triangulation of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:1096-1180), and the whole pair loop of :1058-1199 on the device.
//
//   triangulate_one        : one match -> verdict + x3D, the reference's expressions in its operation order and types: everything fp32
//                            except where the reference's expression is double (cv::norm and cv::Mat::dot return double, `1.0 / z`, the
//                            comparisons against 0.9998 and 5.991 * sigma2).  OpenCV's evaluation of the cv::Mat expressions is recalled
//                            [OCV-RECALL]: 3x3 * 3x1 on cv::gemm's small-matrix path (fp32 row sum, as k_project), `a * row - row` as
//                            cv::addWeighted in fp32, `v / w` as a multiplication by the fp32 reciprocal (cvtScale32f), cv::SVD::compute
//                            as JacobiSVDImpl_<float> on A^T (one-sided Jacobi: fp32 rotations, double norms / dot products, eps =
//                            2 FLT_EPSILON, at most 30 sweeps, rows sorted by singular value descending).
//   k_triangulate          : one lane per match of a caller-given list (uvo_triangulate_matches)
//   k_create_new_map_points: ONE workgroup walks the pairs in order; per pair: the acceptance loop of SearchForTriangulation
//                            (src/ORBmatcher.cc:886-960, the fixed point of k_match_resolve's UVO_RULE_TRIANGULATION with the queries that
//                            hold a map point BY NOW switched off), the rotation filter (:966-984, as k_rot_filter), the match list in
//                            ascending idx1 (what vMatchedIndices holds), triangulate_one per match, has_mp1 = 1 for the accepted ones.
//                            Pair k + 1 starts behind a workgroup barrier: no launch, no host visit between pairs.
// The 4 x 4 Jacobi is unrolled over compile-time indices so that the matrices stay in registers (no scratch, no LDS).
#include "triangulate.hpp"

namespace uvo {

namespace {

// cv::Mat 3x3 * 3x1 in fp32 on cv::gemm's small-matrix path, alpha = 1, no C: the fp32 row sum
__device__ __forceinline__ float row3(float a, float b, float c, const float* p) { return a * p[0] + b * p[1] + c * p[2]; }
// cv::Mat::dot of a 1x3 row with a 3x1 vector: double accumulator over fp32 inputs
__device__ __forceinline__ double dot3d(const float* r, const float* p) {
  double s = 0.0;
  s += (double)r[0] * (double)p[0];
  s += (double)r[1] * (double)p[1];
  s += (double)r[2] * (double)p[2];
  return s;
}
__device__ __forceinline__ double norm3d(const float* p) { return sqrt(dot3d(p, p)); }  // cv::norm (NORM_L2): double

// One Jacobi rotation of rows I, J of At (and Vt) -- the body of JacobiSVDImpl_<float>'s (i, j) loop, m = n = 4.
#define UVO_JACOBI_PAIR(I, J)                                                               \
  {                                                                                         \
    double a = W[I], p = 0, b = W[J];                                                       \
    _Pragma("unroll") for (int k = 0; k < 4; ++k) p += (double)At[I][k] * (double)At[J][k]; \
    if (!(fabs(p) <= (double)eps * sqrt(a * b))) {                                          \
      p *= 2;                                                                               \
      const double beta = a - b, gamma = hypot(p, beta);                                    \
      float c, s;                                                                           \
      if (beta < 0) {                                                                       \
        const double delta = (gamma - beta) * 0.5;                                          \
        s = (float)sqrt(delta / gamma);                                                     \
        c = (float)(p / (gamma * (double)s * 2));                                           \
      } else {                                                                              \
        c = (float)sqrt((gamma + beta) / (gamma * 2));                                      \
        s = (float)(p / (gamma * (double)c * 2));                                           \
      }                                                                                     \
      a = b = 0;                                                                            \
      _Pragma("unroll") for (int k = 0; k < 4; ++k) {                                       \
        const float t0 = c * At[I][k] + s * At[J][k];                                       \
        const float t1 = -s * At[I][k] + c * At[J][k];                                      \
        At[I][k] = t0, At[J][k] = t1;                                                       \
        a += (double)t0 * (double)t0, b += (double)t1 * (double)t1;                         \
      }                                                                                     \
      W[I] = a, W[J] = b;                                                                   \
      changed = true;                                                                       \
      _Pragma("unroll") for (int k = 0; k < 4; ++k) {                                       \
        const float t0 = c * Vt[I][k] + s * Vt[J][k];                                       \
        const float t1 = -s * Vt[I][k] + c * Vt[J][k];                                      \
        Vt[I][k] = t0, Vt[J][k] = t1;                                                       \
      }                                                                                     \
    }                                                                                       \
  }
// selection step of the final sort: rows I and JJ change places when the largest of W[I..3] was found at JJ
#define UVO_SORT_SWAP(I, JJ)                        \
  if (j == JJ) {                                    \
    const double tw = W[I];                         \
    W[I] = W[JJ], W[JJ] = tw;                       \
    _Pragma("unroll") for (int k = 0; k < 4; ++k) { \
      const float tv = Vt[I][k];                    \
      Vt[I][k] = Vt[JJ][k], Vt[JJ][k] = tv;         \
    }                                               \
  }

// vt.row(3) of cv::SVD::compute(A, w, u, vt, MODIFY_A | FULL_UV) for a 4 x 4 fp32 A (rows a0..a3)
__device__ __forceinline__ void svd4_last_row(const float* a0, const float* a1, const float* a2, const float* a3, float* v) {
  float At[4][4], Vt[4][4];
  double W[4];
  const float eps = 1.1920928955078125e-7f * 2;  // FLT_EPSILON * 2
#pragma unroll
  for (int i = 0; i < 4; ++i) {  // At = A^T: row i of At is column i of A
    At[i][0] = a0[i], At[i][1] = a1[i], At[i][2] = a2[i], At[i][3] = a3[i];
    double sd = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      sd += (double)At[i][k] * (double)At[i][k];
      Vt[i][k] = i == k ? 1.f : 0.f;
    }
    W[i] = sd;
  }
  for (int iter = 0; iter < 30; ++iter) {  // max_iter = max(m, 30)
    bool changed = false;
    UVO_JACOBI_PAIR(0, 1)
    UVO_JACOBI_PAIR(0, 2)
    UVO_JACOBI_PAIR(0, 3)
    UVO_JACOBI_PAIR(1, 2)
    UVO_JACOBI_PAIR(1, 3)
    UVO_JACOBI_PAIR(2, 3)
    if (!changed) break;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    double sd = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) sd += (double)At[i][k] * (double)At[i][k];
    W[i] = sqrt(sd);
  }
  {  // i = 0: j = the first largest of W[0..3]
    int j = 0;
    double wj = W[0];
    if (wj < W[1]) j = 1, wj = W[1];
    if (wj < W[2]) j = 2, wj = W[2];
    if (wj < W[3]) j = 3;
    UVO_SORT_SWAP(0, 1)
    UVO_SORT_SWAP(0, 2)
    UVO_SORT_SWAP(0, 3)
  }
  {  // i = 1
    int j = 1;
    double wj = W[1];
    if (wj < W[2]) j = 2, wj = W[2];
    if (wj < W[3]) j = 3;
    UVO_SORT_SWAP(1, 2)
    UVO_SORT_SWAP(1, 3)
  }
  {  // i = 2
    const int j = W[2] < W[3] ? 3 : 2;
    UVO_SORT_SWAP(2, 3)
  }
  v[0] = Vt[3][0], v[1] = Vt[3][1], v[2] = Vt[3][2], v[3] = Vt[3][3];
}
#undef UVO_JACOBI_PAIR
#undef UVO_SORT_SWAP

// src/LocalMapping.cc:1106-1180 for one match.  x3d holds the point whenever the homogeneous coordinate is non-zero (verdict >=
// UVO_TRI_BEHIND_1 or accepted), zeros otherwise.
__device__ __forceinline__ int triangulate_one(const TriCam& C1, const TriCam& C2, float ratioFactor, float k1x, float k1y, int oct1, float k2x,
                                               float k2y, int oct2, float* x3d) {
  x3d[0] = x3d[1] = x3d[2] = 0.f;
  const float invfx1 = 1.0f / C1.fx, invfy1 = 1.0f / C1.fy, invfx2 = 1.0f / C2.fx, invfy2 = 1.0f / C2.fy;  // :1052-1053, :1093-1094
  // :1106-1110 parallax between the rays (Rwc = Rcw^T: row i of Rwc is column i of Rcw)
  const float xn1[3] = {(k1x - C1.cx) * invfx1, (k1y - C1.cy) * invfy1, 1.0f};
  const float xn2[3] = {(k2x - C2.cx) * invfx2, (k2y - C2.cy) * invfy2, 1.0f};
  const float ray1[3] = {row3(C1.r[0], C1.r[3], C1.r[6], xn1), row3(C1.r[1], C1.r[4], C1.r[7], xn1), row3(C1.r[2], C1.r[5], C1.r[8], xn1)};
  const float ray2[3] = {row3(C2.r[0], C2.r[3], C2.r[6], xn2), row3(C2.r[1], C2.r[4], C2.r[7], xn2), row3(C2.r[2], C2.r[5], C2.r[8], xn2)};
  const float cosParallaxRays = (float)(dot3d(ray1, ray2) / (norm3d(ray1) * norm3d(ray2)));
  if (cosParallaxRays < 0 || (double)cosParallaxRays > 0.9998) return UVO_TRI_PARALLAX;  // :1112
  // :1116-1120 rows of A: xn * Tcw.row(2) - Tcw.row(i), Tcw = [Rcw | tcw]
  float A0[4], A1[4], A2[4], A3[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float t1r0 = k < 3 ? C1.r[k] : C1.t[0], t1r1 = k < 3 ? C1.r[3 + k] : C1.t[1], t1r2 = k < 3 ? C1.r[6 + k] : C1.t[2];
    const float t2r0 = k < 3 ? C2.r[k] : C2.t[0], t2r1 = k < 3 ? C2.r[3 + k] : C2.t[1], t2r2 = k < 3 ? C2.r[6 + k] : C2.t[2];
    A0[k] = xn1[0] * t1r2 - t1r0;
    A1[k] = xn1[1] * t1r2 - t1r1;
    A2[k] = xn2[0] * t2r2 - t2r0;
    A3[k] = xn2[1] * t2r2 - t2r1;
  }
  float v[4];
  svd4_last_row(A0, A1, A2, A3, v);  // :1122-1125
  if (v[3] == 0) return UVO_TRI_W_ZERO;  // :1127
  const float rinv = (float)(1.0 / (double)v[3]);  // :1131 Mat / double = Mat * (1 / s), scaled in fp32
  const float X[3] = {v[0] * rinv, v[1] * rinv, v[2] * rinv};
  x3d[0] = X[0], x3d[1] = X[1], x3d[2] = X[2];
  const float z1 = (float)(dot3d(C1.r + 6, X) + (double)C1.t[2]);  // :1135
  if (z1 <= 0) return UVO_TRI_BEHIND_1;
  const float z2 = (float)(dot3d(C2.r + 6, X) + (double)C2.t[2]);  // :1139
  if (z2 <= 0) return UVO_TRI_BEHIND_2;
  {  // :1144-1153
    const float sigmaSquare1 = C1.sigma2[oct1];
    const float x1 = (float)(dot3d(C1.r, X) + (double)C1.t[0]);
    const float y1 = (float)(dot3d(C1.r + 3, X) + (double)C1.t[1]);
    const float invz1 = (float)(1.0 / (double)z1);
    const float u1 = C1.fx * x1 * invz1 + C1.cx;
    const float v1 = C1.fy * y1 * invz1 + C1.cy;
    const float errX1 = u1 - k1x, errY1 = v1 - k1y;
    if ((double)(errX1 * errX1 + errY1 * errY1) > 5.991 * (double)sigmaSquare1) return UVO_TRI_REPROJ_1;
  }
  {  // :1156-1165
    const float sigmaSquare2 = C2.sigma2[oct2];
    const float x2 = (float)(dot3d(C2.r, X) + (double)C2.t[0]);
    const float y2 = (float)(dot3d(C2.r + 3, X) + (double)C2.t[1]);
    const float invz2 = (float)(1.0 / (double)z2);
    const float u2 = C2.fx * x2 * invz2 + C2.cx;
    const float v2 = C2.fy * y2 * invz2 + C2.cy;
    const float errX2 = u2 - k2x, errY2 = v2 - k2y;
    if ((double)(errX2 * errX2 + errY2 * errY2) > 5.991 * (double)sigmaSquare2) return UVO_TRI_REPROJ_2;
  }
  // :1168-1180 scale consistency
  const float n1[3] = {X[0] - C1.ow[0], X[1] - C1.ow[1], X[2] - C1.ow[2]};
  const float n2[3] = {X[0] - C2.ow[0], X[1] - C2.ow[1], X[2] - C2.ow[2]};
  const float dist1 = (float)norm3d(n1), dist2 = (float)norm3d(n2);
  if (dist1 == 0 || dist2 == 0) return UVO_TRI_ZERO_DIST;
  const float ratioDist = dist1 / dist2;
  const float ratioOctave = C1.sf[oct1] / C2.sf[oct2];
  if (ratioDist * ratioFactor < ratioOctave || ratioDist > ratioOctave * ratioFactor) return UVO_TRI_SCALE;
  return UVO_TRI_ACCEPTED;
}

__device__ __forceinline__ void store_result(int v, const float* X, int32_t* verdict, float* x3d, int64_t j) {
  verdict[j] = v;
  x3d[3 * j] = X[0], x3d[3 * j + 1] = X[1], x3d[3 * j + 2] = X[2];
}

constexpr int HISTO_LENGTH = 30;  // src/ORBmatcher.cc:42
constexpr int TH_LOW = 50;        // src/ORBmatcher.cc:41

// Choice of query i of a pair (src/ORBmatcher.cc:893-935), given the ownership of the pair's targets so far: free candidates with
// d <= TH_LOW, sorted by (d, idx2); walk while d <= round(2 * best); the first one on the epipolar line.  The same rule as
// rule_choice(UVO_RULE_TRIANGULATION) in match_engine.hip.
__device__ __forceinline__ int tri_choice(int i, const int32_t* cand_start, const uint32_t* cand, const int32_t* owner) {
  const int b = cand_start[i], e = cand_start[i + 1];
  int best = 0x7fffffff;
  for (int c = b; c < e; ++c) {
    const uint32_t v = cand[c];
    if (owner[v & 0xffffu] < i) continue;
    const int d = (int)((v >> 16) & 0x1ffu);
    if (d > TH_LOW) continue;
    best = d < best ? d : best;
  }
  if (best == 0x7fffffff) return -1;
  const int dist_th = 2 * best;
  uint32_t pick = 0xffffffffu;  // (d << 16 | idx2): the sort order of vector<pair<int, size_t>>
  for (int c = b; c < e; ++c) {
    const uint32_t v = cand[c];
    if (!(v >> 31)) continue;
    if (owner[v & 0xffffu] < i) continue;
    const int d = (int)((v >> 16) & 0x1ffu);
    if (d > TH_LOW || d > dist_th) continue;
    const uint32_t key = ((uint32_t)d << 16) | (v & 0xffffu);
    pick = key < pick ? key : pick;
  }
  return pick == 0xffffffffu ? -1 : (int)(pick & 0xffffu);
}

// rotation bin of a match (src/ORBmatcher.cc:936-944), as k_rot_filter: -2 = lands in no bin (the reference asserts the range)
__device__ __forceinline__ int rot_bin(float a1, float a2) {
  float rot = a1 - a2;
  if (rot < 0.0) rot += 360.0f;
  if (!(rot >= 0.0f && rot < 360.0f * 1.05f)) return -2;
  int bin = (int)roundf(rot * (1.0f / HISTO_LENGTH));
  if (bin == HISTO_LENGTH) bin = 0;
  return bin >= 0 && bin < HISTO_LENGTH ? bin : -2;
}

}  // namespace

__global__ __launch_bounds__(256) void k_triangulate(int n, const TriCam* __restrict__ cams, float ratio_factor, const uvo_keypoint* __restrict__ kp1,
                                                     const uvo_keypoint* __restrict__ kp2, int32_t* __restrict__ verdict, float* __restrict__ x3d) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  float X[3];
  const int v = triangulate_one(cams[0], cams[1], ratio_factor, kp1[j].x, kp1[j].y, kp1[j].octave, kp2[j].x, kp2[j].y, kp2[j].octave, X);
  store_result(v, X, verdict, x3d, j);
}

// One workgroup of 512 lanes (a 256-register budget per lane: the unrolled Jacobi spills at 128).  A.pair[p] = {q_begin, q_end, n2, base}: the pair's queries are [q_begin, q_end) of q_idx1 / cand_start (the
// reference's visiting order), its key frame 2 holds n2 key points whose coordinates start at element `base` of tx / ty / tlevel / tangle.
// Outputs of pair p start at element q_begin of out_idx1 / out_idx2 / verdict / x3d (a pair has at most as many matches as queries).
__global__ __launch_bounds__(512) void k_create_new_map_points(TriChain A) {
  __shared__ int32_t s_owner[4096], s_owner_next[4096];
  __shared__ int s_part[512];
  __shared__ int s_hist[HISTO_LENGTH];
  __shared__ int s_keep[3];
  __shared__ int s_changed, s_accepted;
  const int INF = 0x7fffffff;
  const int tid = threadIdx.x, nth = blockDim.x;
  const TriCam& C1 = A.cams[0];
  for (int p = 0; p < A.n_pairs; ++p) {
    const int qb = A.pair[4 * p], nq = A.pair[4 * p + 1] - qb, n2 = A.pair[4 * p + 2], base = A.pair[4 * p + 3];
    const int32_t* cand_start = A.cand_start + qb;
    const int32_t* q_idx1 = A.q_idx1 + qb;
    int32_t* choice = A.choice;
    int32_t* owner = n2 <= 4096 ? s_owner : A.owner;
    int32_t* owner_next = n2 <= 4096 ? s_owner_next : A.owner_next;
    // ---- SearchForTriangulation's acceptance loop as a fixed point (k_match_resolve), queries with a map point by now switched off
    for (int k = tid; k < n2; k += nth) owner[k] = INF;
    for (int i = tid; i < nq; i += nth) choice[i] = -2;
    for (int i = tid; i < A.n1; i += nth) A.match12[i] = -1;
    if (tid < HISTO_LENGTH) s_hist[tid] = 0;
    if (tid == 0) s_accepted = 0;
    __syncthreads();
    for (int iter = 0; iter <= nq; ++iter) {
      if (tid == 0) s_changed = 0;
      for (int k = tid; k < n2; k += nth) owner_next[k] = INF;
      __syncthreads();
      for (int i = tid; i < nq; i += nth) {
        const int ch = A.has_mp1[q_idx1[i]] ? -1 : tri_choice(i, cand_start, A.cand, owner);
        if (ch != choice[i]) {
          choice[i] = ch;
          s_changed = 1;
        }
        if (ch >= 0) atomicMin(&owner_next[ch], i);
      }
      __syncthreads();
      for (int k = tid; k < n2; k += nth) owner[k] = owner_next[k];
      const int changed = s_changed;
      __syncthreads();
      if (!changed) break;
    }
    // ---- rotation consistency (:966-984)
    if (A.check_orientation) {
      for (int i = tid; i < nq; i += nth)
        if (choice[i] >= 0) {
          const int b = rot_bin(A.kp1[q_idx1[i]].angle, A.tangle[base + choice[i]]);
          if (b >= 0) atomicAdd(&s_hist[b], 1);
        }
      __syncthreads();
      if (tid == 0) {  // ComputeThreeMaxima (:1748-1789)
        int max1 = 0, max2 = 0, max3 = 0, ind1 = -1, ind2 = -1, ind3 = -1;
        for (int i = 0; i < HISTO_LENGTH; i++) {
          const int s = s_hist[i];
          if (s > max1) {
            max3 = max2, max2 = max1, max1 = s;
            ind3 = ind2, ind2 = ind1, ind1 = i;
          } else if (s > max2) {
            max3 = max2, max2 = s;
            ind3 = ind2, ind2 = i;
          } else if (s > max3) {
            max3 = s, ind3 = i;
          }
        }
        if (max2 < 0.1f * (float)max1) {
          ind2 = -1, ind3 = -1;
        } else if (max3 < 0.1f * (float)max1) {
          ind3 = -1;
        }
        s_keep[0] = ind1, s_keep[1] = ind2, s_keep[2] = ind3;
      }
      __syncthreads();
      for (int i = tid; i < nq; i += nth)
        if (choice[i] >= 0) {
          const int b = rot_bin(A.kp1[q_idx1[i]].angle, A.tangle[base + choice[i]]);
          if (b != s_keep[0] && b != s_keep[1] && b != s_keep[2]) choice[i] = -1;
        }
      __syncthreads();
    }
    // ---- vMatchedIndices: the pairs with match12[idx1] >= 0, ascending idx1 (:986-1000)
    for (int i = tid; i < nq; i += nth)
      if (choice[i] >= 0) A.match12[q_idx1[i]] = choice[i];
    __syncthreads();
    const int per = (A.n1 + nth - 1) / nth;
    const int cb = min(tid * per, A.n1), ce = min(cb + per, A.n1);
    int cnt = 0;
    for (int i = cb; i < ce; ++i) cnt += A.match12[i] >= 0;
    s_part[tid] = cnt;
    __syncthreads();
    for (int off = 1; off < nth; off <<= 1) {  // inclusive scan over the lanes' counts
      const int v = tid >= off ? s_part[tid - off] : 0;
      __syncthreads();
      s_part[tid] += v;
      __syncthreads();
    }
    const int n_matches = s_part[nth - 1];
    int run = qb + (tid ? s_part[tid - 1] : 0);
    for (int i = cb; i < ce; ++i) {
      const int t = A.match12[i];
      if (t >= 0) {
        A.out_idx1[run] = i, A.out_idx2[run] = t;
        ++run;
      }
    }
    __syncthreads();
    // ---- triangulate the pair's matches (:1096-1180); the accepted ones give their key-frame-1 feature a map point (:1188)
    const TriCam& C2 = A.cams[1 + p];
    int acc = 0;
    for (int j = tid; j < n_matches; j += nth) {
      const int i1 = A.out_idx1[qb + j], i2 = base + A.out_idx2[qb + j];
      float X[3];
      const int v = triangulate_one(C1, C2, A.ratio_factor, A.kp1[i1].x, A.kp1[i1].y, A.kp1[i1].octave, A.tx[i2], A.ty[i2], A.tlevel[i2], X);
      store_result(v, X, A.verdict, A.x3d, qb + j);
      if (v == UVO_TRI_ACCEPTED) {
        A.has_mp1[i1] = 1;
        ++acc;
      }
    }
    if (acc) atomicAdd(&s_accepted, acc);
    __syncthreads();
    if (tid == 0) A.n_matches[p] = n_matches, A.n_accepted[p] = s_accepted;
    __syncthreads();
  }
}

void launch_triangulate(hipStream_t s, int n, const TriCam* d_cams, float ratio_factor, const uvo_keypoint* d_kp1, const uvo_keypoint* d_kp2,
                        int32_t* d_verdict, float* d_x3d) {
  if (n > 0) hipLaunchKernelGGL(k_triangulate, dim3((n + 255) / 256), dim3(256), 0, s, n, d_cams, ratio_factor, d_kp1, d_kp2, d_verdict, d_x3d);
}

void launch_create_new_map_points(hipStream_t s, const TriChain& A) {
  if (A.n_pairs > 0) hipLaunchKernelGGL(k_create_new_map_points, dim3(1), dim3(512), 0, s, A);
}

}  // namespace uvo
