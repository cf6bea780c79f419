// Host build of the solvePnPRansac arithmetic (u-vip-slam_amd/csrc/epnp_core.hpp): the same source the HIP kernels of pnp.hip run,
// driven by one "lane", so that every hypothesis pose and the whole run can be compared with the device bit for bit on a machine
// with a GPU, and with the numpy model (tests/pnp_model.py) where EPnP is determined on a machine without.  Test scaffolding only.
// Build with -ffp-contract=off, as the library is.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../u-vip-slam_amd/csrc/epnp_core.hpp"

using namespace uvo::pnp;

static Cam make_cam(const double* c) {  // fx fy cx cy k1 k2 p1 p2 k3 k4 k5 k6
  Cam C;
  C.fx = c[0], C.fy = c[1], C.cx = c[2], C.cy = c[3];
  for (int i = 0; i < 8; ++i) C.k[i] = c[4 + i];
  return C;
}

extern "C" {

// subsets [hyp][5], hyp_end [hyp]
void emu_pnp_subsets(int n, int hyp, int32_t* subsets, uint32_t* hyp_end) {
  Rng rng;
  for (int h = 0; h < hyp; ++h) {
    draw_subset(rng, n, subsets + 5 * h);
    hyp_end[h] = rng.draws;
  }
}

void emu_pnp_errors(const double* cam, const double* pose, const float* obj, const float* img, int n, float* err) {
  const Cam C = make_cam(cam);
  for (int i = 0; i < n; ++i) err[i] = project_error(C, pose, pose + 9, obj + 3 * i, img + 2 * i);
}

void emu_pnp_rodrigues(const double* R, double* rvec) { rodrigues(R, rvec); }

int emu_pnp_replay(const int32_t* counts, int n, double conf, int max_iters, int* iterations) { return replay(counts, n, conf, max_iters, iterations); }

// EPnP on the m listed points: as_float = the RANSAC kernel's view (undistorted points stored as float), else the refit's (double)
int emu_pnp_epnp(const double* cam, const float* obj, const float* img, int n, const int32_t* idx, int m, int as_float, double* pose) {
  const Cam C = make_cam(cam);
  std::vector<float> uf(2 * (size_t)n);
  std::vector<double> ud(2 * (size_t)n);
  for (int i = 0; i < n; ++i) {
    undistort_norm(C, (double)img[2 * i], (double)img[2 * i + 1], &ud[2 * i], &ud[2 * i + 1]);
    uf[2 * i] = (float)ud[2 * i], uf[2 * i + 1] = (float)ud[2 * i + 1];
  }
  double ws[W_SIZE];
  const Points P{obj, uf.data(), as_float ? nullptr : ud.data(), idx, m, C.fx, C.fy, C.cx, C.cy};
  for (int e = 0; e < 12; ++e) pose[e] = 0.;
  return solve(Ws<1>{ws}, P, 0, 1, NoSync(), pose) ? 1 : 0;
}

// the whole call as uvo_klt_solve_pnp_ransac runs it.  info: ok, iterations, inliers, rng_draws; the tap arrays hold `hyp` entries
// (subsets [hyp][5], poses [hyp][12], counts [hyp]) with hyp = min(iterations, 1000), or 1 for n == 5; returns hyp
int emu_pnp_run(const double* cam, const float* obj, const float* img, int n, int iterations, double thr, double conf, double* rvec, double* tvec,
                double* pose, int32_t* inliers, int32_t* info, int32_t* subsets, double* poses, int32_t* counts) {
  const Cam C = make_cam(cam);
  for (int i = 0; i < 3; ++i) rvec[i] = tvec[i] = 0.;
  for (int e = 0; e < 12; ++e) pose[e] = 0.;
  info[0] = info[1] = info[2] = info[3] = 0;
  if (n < kModelPoints) return 0;
  const bool direct = n == kModelPoints;
  const int hyp = direct ? 1 : (iterations < 1000 ? iterations : 1000);
  const float t = (float)(thr * thr);
  std::vector<float> uf(2 * (size_t)n);
  std::vector<double> ud(2 * (size_t)n);
  for (int i = 0; i < n; ++i) {
    undistort_norm(C, (double)img[2 * i], (double)img[2 * i + 1], &ud[2 * i], &ud[2 * i + 1]);
    uf[2 * i] = (float)ud[2 * i], uf[2 * i + 1] = (float)ud[2 * i + 1];
  }
  std::vector<uint32_t> hyp_end(hyp, 0);
  if (direct)
    for (int i = 0; i < 5; ++i) subsets[i] = i;
  else
    emu_pnp_subsets(n, hyp, subsets, hyp_end.data());
  double ws[W_SIZE];
  for (int h = 0; h < hyp; ++h) {
    const Points P{obj, uf.data(), nullptr, subsets + 5 * h, kModelPoints, C.fx, C.fy, C.cx, C.cy};
    double* out = poses + 12 * (size_t)h;
    for (int e = 0; e < 12; ++e) out[e] = 0.;
    const bool ok = solve(Ws<1>{ws}, P, 0, 1, NoSync(), out);
    counts[h] = ok ? 0 : -1;
    if (ok && !direct) {
      int c = 0;
      for (int i = 0; i < n; ++i) c += project_error(C, out, out + 9, obj + 3 * i, img + 2 * i) <= t;
      counts[h] = c;
    }
  }
  int winner, iters = 0;
  if (direct)
    winner = counts[0] < 0 ? -1 : 0;
  else
    winner = replay(counts, n, conf, hyp, &iters);
  info[1] = iters;
  info[3] = iters > 0 ? (int32_t)hyp_end[iters - 1] : 0;
  if (winner < 0) return hyp;
  std::vector<int32_t> list;
  const double* R = poses + 12 * (size_t)winner;
  for (int i = 0; i < n; ++i)
    if (direct || project_error(C, R, R + 9, obj + 3 * i, img + 2 * i) <= t) list.push_back(i);
  bool ok;
  if (direct) {
    std::memcpy(pose, poses, 12 * sizeof(double));
    ok = true;
  } else {
    const Points P{obj, nullptr, ud.data(), list.data(), (int)list.size(), C.fx, C.fy, C.cx, C.cy};
    ok = solve(Ws<1>{ws}, P, 0, 1, NoSync(), pose);
  }
  if (!ok) {
    for (int e = 0; e < 12; ++e) pose[e] = 0.;
    return hyp;
  }
  info[0] = 1, info[2] = (int32_t)list.size();
  std::memcpy(inliers, list.data(), list.size() * sizeof(int32_t));
  rodrigues(pose, rvec);
  for (int i = 0; i < 3; ++i) tvec[i] = pose[9 + i];
  return hyp;
}

}  // extern "C"
