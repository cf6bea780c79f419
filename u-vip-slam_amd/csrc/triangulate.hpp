// Device-side records of the triangulation kernels (triangulate.hip) and their launchers; shared with matcher_batch.cpp.
#pragma once
#include "common.hpp"

namespace uvo {

constexpr int kTriMaxLevels = 64;

// a key frame as the triangulation reads it (uvo_triangulation_camera, level tables copied in)
struct TriCam {
  float r[9], t[3], ow[3];
  float fx, fy, cx, cy;
  float sf[kTriMaxLevels];      // GetScaleFactor(level)
  float sigma2[kTriMaxLevels];  // GetSigma2(level)
};

// arguments of k_create_new_map_points
struct TriChain {
  int n_pairs, n1, check_orientation;
  float ratio_factor;
  const TriCam* cams;           // [1 + n_pairs]: key frame 1, then key frame 2 of every pair
  const int32_t* pair;          // [n_pairs][4]: q_begin, q_end, n2, base
  const int32_t* q_idx1;        // [nq] query -> feature of key frame 1
  const int32_t* cand_start;    // [nq + 1]
  const uint32_t* cand;         // packed candidates (k_group_dist_pairs)
  const uvo_keypoint* kp1;      // [n1]
  const float *tx, *ty, *tangle;  // [nt] key frame 2 key points of all pairs
  const int32_t* tlevel;        // [nt]
  uint8_t* has_mp1;             // [n1] in / out
  int32_t *owner, *owner_next;  // [max n2] (used when a pair has more than 4096 key points)
  int32_t* choice;              // [max queries of a pair]
  int32_t* match12;             // [n1]
  int32_t *out_idx1, *out_idx2, *verdict;  // [nq]
  float* x3d;                   // [nq][3]
  int32_t *n_matches, *n_accepted;         // [n_pairs]
};

void launch_triangulate(hipStream_t s, int n, const TriCam* d_cams, float ratio_factor, const uvo_keypoint* d_kp1, const uvo_keypoint* d_kp2,
                        int32_t* d_verdict, float* d_x3d);
void launch_create_new_map_points(hipStream_t s, const TriChain& A);

}  // namespace uvo
