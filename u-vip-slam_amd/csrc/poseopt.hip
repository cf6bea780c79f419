// Optimizer::PoseOptimization(Frame*) (src/Optimizer.cc:2012-2145) over a LIST of independent problems as one call.  All arithmetic and
// the whole control flow is poseopt_core.hpp (poseopt::run), shared with the host build tests/emu/poseopt_emu.cpp; this file is the
// device's Team -- which lane adds which edges and how the 256 lane sums meet -- and the host side of the C ABI.
//
// One launch: k_pose_optimize, one workgroup of 256 lanes per problem, all four rounds.  A lane owns the edges l, l + 256, ... for the
// whole call: it alone reads and writes their chi2 and state bytes (LDS up to kPoseLdsEdges edges, the set's block beyond), so the only
// exchange between lanes is the reduction: a butterfly of __shfl_xor inside each wavefront, then one LDS word per wavefront and sum,
// one barrier, and every lane adds the four words itself (a trial's sum) or 28 lanes add one sum each into 28 LDS words that all lanes
// read for the ten trials to come (a linearisation's sums: kept out of every lane's registers).  The wavefront words alternate between
// two buffers, so a reduction costs one barrier:
// a lane can reach the write of reduction i + 2 only through the barrier of reduction i + 1, which no lane passes before it has read
// the words of reduction i.  Every lane then computes the 6 x 6 solve and the Levenberg decision from the same words: all branches of
// poseopt::run are uniform, every loop has a compile-time bound (4 x 10 x 10), and there is no return before the last barrier.
#include <cstring>
#include <vector>

#include "devmem.hpp"
#include "poseopt.hpp"

namespace uvo {

struct PoseDev {
  const PoseProblemDev* prob;  // [P]
  const float* edges;          // [sum n][6]
  double* chi2;                // [P * N], used by problems above kPoseLdsEdges
  uint8_t* state;              // [P * N]
  poseopt::Trace* trace;       // [P]
  poseopt::Out* result;        // [P]
  uint8_t* mask;               // [sum n]
};

struct DevTeam {
  double* red;   // LDS [2][4][kSums]
  int32_t* redi; // LDS [2][4]
  double* store; // LDS [kSums]
  int phase;
  __device__ __forceinline__ bool lead() const { return threadIdx.x == 0; }
  // every lane's K sums through the butterfly, one word per wavefront and sum into this reduction's buffer, one barrier -> the buffer
  template <int K, class F>
  __device__ __forceinline__ const double* gather(F f) {
    double acc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = 0.;
    f((int)threadIdx.x, acc);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1)
#pragma unroll
      for (int k = 0; k < K; ++k) acc[k] = acc[k] + __shfl_xor(acc[k], m);
    double* buf = red + phase * 4 * poseopt::kSums;
    phase ^= 1;
    const int wave = wave_in_block();
    if ((threadIdx.x & 63) == 0)
#pragma unroll
      for (int k = 0; k < K; ++k) buf[wave * poseopt::kSums + k] = acc[k];
    __syncthreads();
    return buf;
  }
  static __device__ __forceinline__ double combine(const double* buf, int k) {
    return (buf[k] + buf[poseopt::kSums + k]) + (buf[2 * poseopt::kSums + k] + buf[3 * poseopt::kSums + k]);
  }
  // a trial's sum: back in a register of every lane
  template <int K, class F>
  __device__ __forceinline__ void sum(F f, double* out) {
    const double* buf = gather<K>(f);
#pragma unroll
    for (int k = 0; k < K; ++k) out[k] = combine(buf, k);
  }
  // the linearisation's sums, left in LDS for every lane to read: lanes 0..K-1 combine one each, and a second barrier publishes them.
  // The next write of `store` lies behind the first barrier of the next linearisation, which no lane passes while another still reads.
  __device__ __forceinline__ double* shared() const { return store; }
  template <int K, class F>
  __device__ __forceinline__ void sum_shared(F f, double* out) {
    const double* buf = gather<K>(f);
    const int k = (int)threadIdx.x;
    if (k < K) out[k] = combine(buf, k);
    __syncthreads();
  }
  template <class F>
  __device__ __forceinline__ int count(F f) {
    int c = f((int)threadIdx.x);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) c += __shfl_xor(c, m);
    int32_t* buf = redi + phase * 4;
    phase ^= 1;
    if ((threadIdx.x & 63) == 0) buf[wave_in_block()] = c;
    __syncthreads();
    return buf[0] + buf[1] + buf[2] + buf[3];
  }
};

// Two wavefronts per SIMD asked for: one workgroup would be allowed 512 registers a lane and the scheduler spends what it is allowed;
// at 256 (arch and accumulation registers together) it still needs no scratch (tests/test_kernel_resources_poseopt.py).
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void k_pose_optimize(PoseDev D) {
  __shared__ double s_chi2[kPoseLdsEdges];
  __shared__ double s_red[2 * 4 * poseopt::kSums];
  __shared__ double s_store[poseopt::kSums];
  __shared__ int32_t s_redi[2 * 4];
  __shared__ uint8_t s_state[kPoseLdsEdges];
  const PoseProblemDev& p = D.prob[blockIdx.x];
  const int n = p.n;
  const bool in_lds = n <= kPoseLdsEdges;  // uniform
  poseopt::Edges E;
  E.in = D.edges + (size_t)p.off * kPoseEdgeFloats;
  E.chi2 = in_lds ? s_chi2 : D.chi2 + p.off;
  E.state = in_lds ? s_state : D.state + p.off;
  E.mask = D.mask + p.off;
  E.n = n;
  const poseopt::Cam C = {(double)p.fx, (double)p.fy, (double)p.cx, (double)p.cy};
  DevTeam T = {s_red, s_redi, s_store, 0};
  poseopt::run<poseopt::kMutNone>(T, E, C, p.Tcw, D.result + blockIdx.x, D.trace + blockIdx.x);
}

}  // namespace uvo

// ---------------------------------------------------------------------------------------------------------------------------
using namespace uvo;

static_assert(sizeof(uvo_pose_trace) == sizeof(poseopt::Trace) && sizeof(uvo_pose_trace_lin) == sizeof(poseopt::TraceLin) &&
                  sizeof(uvo_pose_trace_trial) == sizeof(poseopt::TraceTrial),
              "uvo_pose_trace is poseopt::Trace");

struct uvo_pose_optimizer {
  uvo_klt* klt = nullptr;
  hipStream_t stream = nullptr;
  int device = 0, max_problems = 0, max_points = 0, last_n = 0;
  DevMem mem;  // owns D's block and the page-locked mirrors of its two exchanges
  PoseDev D;
  PoseProblemDev* h_prob = nullptr;  // the upload: problem records, then the edges
  float* h_edges = nullptr;
  poseopt::Out* h_res = nullptr;  // the download: result records, then the masks
  uint8_t* h_mask = nullptr;
};

extern "C" {

void uvo_pose_optimizer_destroy(uvo_pose_optimizer* o) {
  if (!o) return;
  hipSetDevice(o->device);
  if (o->stream) hipStreamSynchronize(o->stream);
  o->mem.release_all();
  delete o;
}

int uvo_pose_optimizer_create(uvo_klt* k, int max_problems, int max_points, uvo_pose_optimizer** out) {
  if (!k || !out) return fail(UVO_E_BADARG, "null pointer");
  *out = nullptr;
  if (max_problems < 1 || max_problems > kPoseMaxProblems || max_points < 1 || max_points > kPoseMaxPoints)
    return fail(UVO_E_BADARG, "pose optimizer: 1..64 problems of 1..16384 points");
  uvo_pose_optimizer* o = new uvo_pose_optimizer();
  o->klt = k, o->stream = klt_stream(k), o->device = klt_device(k);
  o->max_problems = max_problems, o->max_points = max_points;
  const size_t P = (size_t)max_problems, N = (size_t)max_points;
  PoseDev& D = o->D;
  float* edges = nullptr;
  PoseProblemDev* prob = nullptr;
  // each exchange is one copy: its two arrays are adjacent, on the device and in the mirror
  auto upload = [&](Carve& c, auto*& pr, auto*& ed) { c.take(pr, P).take(ed, P * N * kPoseEdgeFloats, alignof(float)); };
  auto download = [&](Carve& c, auto*& res, auto*& mk) { c.take(res, P).take(mk, P * N, alignof(uint8_t)); };
  int rc = hipSetDevice(o->device) == hipSuccess ? UVO_OK : fail(UVO_E_NOMEM, "pose optimizer allocation failed");
  if (!rc) rc = alloc_carved(o->mem, [&](Carve& c) {
    upload(c, prob, edges);
    c.take(D.chi2, P * N).take(D.state, P * N).take(D.trace, P);
    download(c, D.result, D.mask);
  });
  if (!rc) rc = alloc_carved(o->mem, [&](Carve& c) { upload(c, o->h_prob, o->h_edges); }, true);
  if (!rc) rc = alloc_carved(o->mem, [&](Carve& c) { download(c, o->h_res, o->h_mask); }, true);
  if (rc) return uvo_pose_optimizer_destroy(o), rc;
  D.prob = prob, D.edges = edges;
  *out = o;
  return UVO_OK;
}

int uvo_pose_optimize(uvo_pose_optimizer* o, const uvo_pose_problem* problems, int n_problems, uvo_pose_result* results) {
  if (!o) return fail(UVO_E_BADARG, "null handle");
  if (n_problems < 0) return fail(UVO_E_BADARG, "negative problem count");
  if (n_problems > o->max_problems) return fail(UVO_E_CAPACITY, "more problems than the pose optimizer was sized for");
  if (n_problems > 0 && (!problems || !results)) return fail(UVO_E_BADARG, "null pointer");
  size_t total = 0;
  for (int j = 0; j < n_problems; ++j) {
    const uvo_pose_problem& q = problems[j];
    if (q.n < 0) return fail(UVO_E_BADARG, "negative point count");
    if (q.n > o->max_points) return fail(UVO_E_CAPACITY, "more points than the pose optimizer was sized for");
    if (q.n > 0 && (!q.p3d || !q.p2d || !q.inv_sigma2)) return fail(UVO_E_BADARG, "null pointer");
    if (results[j].outlier && results[j].outlier_cap < q.n) return fail(UVO_E_CAPACITY, "outlier_cap is smaller than the problem's n");
    total += (size_t)q.n;
  }
  if (n_problems == 0) return UVO_OK;
  int off = 0;
  for (int j = 0; j < n_problems; ++j) {
    const uvo_pose_problem& q = problems[j];
    PoseProblemDev& r = o->h_prob[j];
    r.n = q.n, r.off = off, r.fx = q.fx, r.fy = q.fy, r.cx = q.cx, r.cy = q.cy, r.pad_[0] = r.pad_[1] = 0;
    std::memcpy(r.Tcw, q.Tcw, sizeof r.Tcw);
    float* e = o->h_edges + (size_t)off * kPoseEdgeFloats;
    for (int i = 0; i < q.n; ++i, e += kPoseEdgeFloats) {
      e[0] = q.p3d[3 * i], e[1] = q.p3d[3 * i + 1], e[2] = q.p3d[3 * i + 2];
      e[3] = q.p2d[2 * i], e[4] = q.p2d[2 * i + 1], e[5] = q.inv_sigma2[i];
    }
    off += q.n;
  }
  const size_t P = (size_t)o->max_problems;
  UVO_HIP_CHECK(hipSetDevice(o->device));
  hipStream_t st = o->stream;
  UVO_HIP_CHECK(hipMemcpyAsync(const_cast<PoseProblemDev*>(o->D.prob), o->h_prob, P * sizeof(PoseProblemDev) + total * kPoseEdgeFloats * sizeof(float),
                               hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_pose_optimize, dim3(n_problems), dim3(256), 0, st, o->D);
  UVO_HIP_CHECK(hipGetLastError());
  UVO_HIP_CHECK(hipMemcpyAsync(o->h_res, o->D.result, P * sizeof(poseopt::Out) + total, hipMemcpyDeviceToHost, st));
  UVO_HIP_CHECK(hipStreamSynchronize(st));
  o->last_n = n_problems;
  for (int j = 0; j < n_problems; ++j) {
    const poseopt::Out& r = o->h_res[j];
    std::memcpy(results[j].Tcw, r.Tcw, sizeof r.Tcw);
    results[j].n_inliers = r.n_inliers, results[j].rounds = r.rounds;
    if (results[j].outlier && problems[j].n > 0) std::memcpy(results[j].outlier, o->h_mask + o->h_prob[j].off, (size_t)problems[j].n);
  }
  return UVO_OK;
}

int uvo_pose_optimizer_trace(uvo_pose_optimizer* o, int problem, uvo_pose_trace* out) {
  if (!o || !out) return fail(UVO_E_BADARG, "null pointer");
  if (problem < 0 || problem >= o->last_n) return fail(UVO_E_BADARG, "the last call had no such problem");
  UVO_HIP_CHECK(hipSetDevice(o->device));
  UVO_HIP_CHECK(hipMemcpy(out, o->D.trace + problem, sizeof(poseopt::Trace), hipMemcpyDeviceToHost));
  // records beyond the counts are whatever an earlier call left: not part of the answer
  std::memset(out->lin + out->n_lin, 0, sizeof(uvo_pose_trace_lin) * (size_t)(poseopt::kMaxLin - out->n_lin));
  std::memset(out->trial + out->n_trials, 0, sizeof(uvo_pose_trace_trial) * (size_t)(poseopt::kMaxTrialRecs - out->n_trials));
  return UVO_OK;
}

}  // extern "C"
