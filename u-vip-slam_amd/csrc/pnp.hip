// cv::solvePnPRansac(mappts, pts, mK, mDistCoef, Rvec, Tvec, false, 300, 3, 0.99, mask_pnp, cv::SOLVEPNP_EPNP), src/Tracking.cc:1864
// (OpenCV 3.4 calib3d solvepnp.cpp, epnp.cpp, ptsetreg.cpp; recalled, not read: tests/pnp_model.py lists every recalled detail
// [OCV-RECALL]).  All arithmetic is epnp_core.hpp, shared with the host build tests/emu/pnp_emu.cpp; this file decides which lane
// computes which scalar.  Four launches in the tracker handle's stream, all scratch sized at uvo_klt_create:
//   k_pnp_prepare    : one thread per point: cv::undistortPoints to normalised coordinates, kept in double (the refit's) and rounded
//                      to float (what solvePnP sees for the float subsets).  One extra workgroup: a single lane walks the cv::RNG
//                      stream and draws every hypothesis's five indices (no checkSubset for this estimator: only repeated indices
//                      are redrawn, 5 to 6 draws per hypothesis).
//   k_pnp_hypotheses : EPnP on five points, one lane per hypothesis, eight lanes per workgroup.  The lane's workspace (589 doubles:
//                      MtM, its eigenvectors, the 6 x 10 system, ...) lives in LDS, interleaved with the other lanes' so that the
//                      eight touch neighbouring banks; nothing is indexed dynamically in registers.  All hypotheses up to
//                      min(iterations, kFmCap) are solved speculatively, as the F-matrix stage does.
//                      At five points the core chooses the basis of MtM's two-dimensional null space itself (epnp_core.hpp).
//   k_pnp_score      : one workgroup per hypothesis over all points: projectPoints + the float error, count by ballot.
//   k_pnp_finish     : one workgroup.  Lane 0 replays the RANSAC loop over the counts (winner, niters updates, stop); all lanes
//                      compact the winner's inliers in ascending order; then the EPnP core once more on the inliers, the 256 lanes
//                      sharing its phases scalar by scalar (epnp_core.hpp), with the double-precision undistorted points.
#include <cfloat>
#include <cmath>

#include "devmem.hpp"
#include "pnp.hpp"

namespace uvo {

constexpr int kPnpHypLanes = 8;

struct SyncThreads {
  __device__ void operator()() const { __syncthreads(); }
};

__global__ __launch_bounds__(256) void k_pnp_prepare(pnp::Cam C, const float* __restrict__ img, int n, int hyp, float* __restrict__ und_f,
                                                     double* __restrict__ und_d, int32_t* __restrict__ subsets, uint32_t* __restrict__ hyp_end) {
  if (blockIdx.x == gridDim.x - 1) {
    if (threadIdx.x != 0) return;
    if (n == pnp::kModelPoints) {  // the direct path: one solve on all points, nothing drawn
      for (int i = 0; i < pnp::kModelPoints; ++i) subsets[i] = i;
      hyp_end[0] = 0;
      return;
    }
    pnp::Rng rng;
    for (int h = 0; h < hyp; ++h) {
      pnp::draw_subset(rng, n, subsets + h * pnp::kModelPoints);
      hyp_end[h] = rng.draws;
    }
    return;
  }
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double x, y;
  pnp::undistort_norm(C, (double)img[2 * i], (double)img[2 * i + 1], &x, &y);
  und_d[2 * i] = x, und_d[2 * i + 1] = y;
  und_f[2 * i] = (float)x, und_f[2 * i + 1] = (float)y;
}

__global__ __launch_bounds__(kPnpHypLanes) void k_pnp_hypotheses(pnp::Cam C, const float* __restrict__ obj, const float* __restrict__ und_f,
                                                                 const int32_t* __restrict__ subsets, int hyp, double* __restrict__ poses,
                                                                 int32_t* __restrict__ counts) {
  __shared__ double s_ws[pnp::W_SIZE * kPnpHypLanes];
  const int h = blockIdx.x * kPnpHypLanes + threadIdx.x;
  if (h >= hyp) return;
  const pnp::Ws<kPnpHypLanes> W{s_ws + threadIdx.x};
  const pnp::Points P{obj, und_f, nullptr, subsets + h * pnp::kModelPoints, pnp::kModelPoints, C.fx, C.fy, C.cx, C.cy};
  double* out = poses + (size_t)h * 12;
  for (int e = 0; e < 12; ++e) out[e] = 0.;
  const bool ok = pnp::solve(W, P, 0, 1, pnp::NoSync(), out);
  counts[h] = ok ? 0 : -1;
}

__global__ __launch_bounds__(256) void k_pnp_score(pnp::Cam C, const float* __restrict__ obj, const float* __restrict__ img, int n, float t,
                                                   const double* __restrict__ poses, int32_t* __restrict__ counts) {
  __shared__ int32_t s_cnt[4];
  const int h = blockIdx.x, lane = threadIdx.x & 63, wave = wave_in_block();
  if (counts[h] < 0) return;  // no pose (uniform over the workgroup)
  const double* R = poses + (size_t)h * 12;
  int cnt = 0;
  for (int i0 = 0; i0 < n; i0 += 256) {
    const int i = i0 + threadIdx.x;
    cnt += __builtin_popcountll(__ballot(i < n && pnp::project_error(C, R, R + 9, obj + 3 * i, img + 2 * i) <= t));
  }
  if (lane == 0) s_cnt[wave] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) counts[h] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}

__global__ __launch_bounds__(256) void k_pnp_finish(pnp::Cam C, const float* __restrict__ obj, const float* __restrict__ img,
                                                    const double* __restrict__ und_d, int n, int hyp, float t, double conf,
                                                    const int32_t* __restrict__ subsets, const uint32_t* __restrict__ hyp_end,
                                                    const double* __restrict__ poses, const int32_t* __restrict__ counts, PnpOut* __restrict__ out,
                                                    int32_t* __restrict__ list) {
  __shared__ double s_ws[pnp::W_SIZE];
  __shared__ double s_pose[12];
  __shared__ int32_t s_wsum[4];
  __shared__ int32_t s_winner, s_iters;
  const int tid = threadIdx.x, lane = tid & 63, wave = wave_in_block();
  const bool direct = n == pnp::kModelPoints;
  if (tid == 0) {
    if (direct) {
      s_winner = counts[0] < 0 ? -1 : 0, s_iters = 0;
    } else {
      int it = 0;
      s_winner = pnp::replay(counts, n, conf, hyp, &it);
      s_iters = it;
    }
  }
  if (tid < 12) s_pose[tid] = 0.;
  __syncthreads();
  const int winner = s_winner, iterations = s_iters;
  int total = 0;
  if (winner >= 0) {  // the winner's inliers in ascending order (the direct path: every point)
    const double* R = poses + (size_t)winner * 12;
    for (int i0 = 0; i0 < n; i0 += 256) {
      const int i = i0 + tid;
      const bool inl = i < n && (direct || pnp::project_error(C, R, R + 9, obj + 3 * i, img + 2 * i) <= t);
      const uint64_t m = __ballot(inl);
      if (lane == 0) s_wsum[wave] = __builtin_popcountll(m);
      __syncthreads();
      int off = total + __builtin_popcountll(m & ((1ull << lane) - 1));
      for (int w = 0; w < 4; ++w) {
        if (w < wave) off += s_wsum[w];
        total += s_wsum[w];
      }
      if (inl) list[off] = i;
      __syncthreads();
    }
  }
  bool ok = false;
  if (winner >= 0 && direct) {
    if (tid < 12) s_pose[tid] = poses[tid];
    ok = true;
  } else if (winner >= 0) {
    const pnp::Ws<1> W{s_ws};
    const pnp::Points P{obj, nullptr, und_d, list, total, C.fx, C.fy, C.cx, C.cy};
    ok = pnp::solve(W, P, tid, 256, SyncThreads(), s_pose);
  }
  __syncthreads();
  if (tid < 9) out->R[tid] = ok ? s_pose[tid] : 0.;
  if (tid < 3) out->t[tid] = ok ? s_pose[9 + tid] : 0.;
  if (tid == 0) {
    out->ok = ok ? 1 : 0, out->iterations = iterations, out->inliers = ok ? total : 0;
    out->rng_draws = iterations > 0 ? hyp_end[iterations - 1] : 0, out->winner = winner;
  }
}

int pnp_alloc(DevMem& m, PnpScratch& p, int max_points) {
  const size_t N = (size_t)max_points;
  RC(alloc_carved(m, [&](Carve& c) {
    c.take(p.io, N * 5).take(p.und_f, N * 2).take(p.und_d, N * 2).take(p.subsets, kFmCap * 5).take(p.hyp_end, kFmCap).take(p.poses, kFmCap * 12);
    c.take(p.counts, kFmCap).take(p.out, 1).take(p.inliers, N, alignof(int32_t));
  }));
  return m.alloc(&p.h_io, N * 20 + sizeof(PnpOut), true);
}

int pnp_enqueue(hipStream_t s, const PnpScratch& p, int n, const pnp::Cam& cam, int iterations, double thr, double conf) {
  const int hyp = n == pnp::kModelPoints ? 1 : std::min(iterations, kFmCap);
  const float* obj = p.io;
  const float* img = p.io + 3 * (size_t)n;
  const float t = (float)(thr * thr);
  hipLaunchKernelGGL(k_pnp_prepare, dim3((n + 255) / 256 + 1), dim3(256), 0, s, cam, img, n, hyp, p.und_f, p.und_d, p.subsets, p.hyp_end);
  hipLaunchKernelGGL(k_pnp_hypotheses, dim3((hyp + kPnpHypLanes - 1) / kPnpHypLanes), dim3(kPnpHypLanes), 0, s, cam, obj, p.und_f, p.subsets, hyp,
                     p.poses, p.counts);
  if (n != pnp::kModelPoints) hipLaunchKernelGGL(k_pnp_score, dim3(hyp), dim3(256), 0, s, cam, obj, img, n, t, p.poses, p.counts);
  hipLaunchKernelGGL(k_pnp_finish, dim3(1), dim3(256), 0, s, cam, obj, img, p.und_d, n, hyp, t, conf, p.subsets, p.hyp_end, p.poses, p.counts, p.out,
                     p.inliers);
  UVO_HIP_CHECK(hipGetLastError());
  return UVO_OK;
}

}  // namespace uvo
