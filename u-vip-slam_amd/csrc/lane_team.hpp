// The one reduction shape of the optimisers (poseopt_core.hpp's header states it: lane sums, a butterfly inside each wavefront,
// (w0 + w1) + (w2 + w3)), walked by the device's 256 lanes (LaneTeam) and by the host's one thread (HostLaneTeam).  The device and the
// host builds of poseopt, sim3opt and ba agree bit for bit because both walk this shape and no other.  KS: the stride of the LDS words,
// the most sums one reduction of that core carries.
#pragma once

namespace uvo {

constexpr int kTeamLanes = 256;

}  // namespace uvo

#if defined(__HIPCC__)
#include "common.hpp"  // wave_in_block

namespace uvo {

// The only exchange between lanes is the reduction: a butterfly of __shfl_xor inside each wavefront, then one LDS word per wavefront
// and sum, one barrier, and every lane adds the four words itself (sum: a trial's sum) or K lanes add one sum each into K LDS words
// that all lanes read for the trials to come (sum_shared: a linearisation's sums, kept out of every lane's registers).  The wavefront
// words alternate between two buffers, so a reduction costs one barrier:
// a lane can reach the write of reduction i + 2 only through the barrier of reduction i + 1, which no lane passes before it has read
// the words of reduction i.
template <int KS>
struct LaneTeam {
  double* red;   // LDS [2][4][KS]
  int32_t* redi; // LDS [2][4]
  double* store; // LDS [KS]
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
    double* buf = red + phase * 4 * KS;
    phase ^= 1;
    const int wave = wave_in_block();
    if ((threadIdx.x & 63) == 0)
#pragma unroll
      for (int k = 0; k < K; ++k) buf[wave * KS + k] = acc[k];
    __syncthreads();
    return buf;
  }
  static __device__ __forceinline__ double combine(const double* buf, int k) {
    return (buf[k] + buf[KS + k]) + (buf[2 * KS + k] + buf[3 * KS + k]);
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

}  // namespace uvo
#endif

#if !defined(__HIP_DEVICE_COMPILE__)
namespace uvo {

// one thread that plays lanes 0..255 in turn and folds as the device does
template <int KS>
struct HostLaneTeam {
  double store[KS];
  bool lead() const { return true; }
  double* shared() { return store; }
  template <int K, class F>
  void sum_shared(F f, double* out) {
    sum<K>(f, out);
  }
  template <int K, class F>
  void sum(F f, double* out) {
    static thread_local double s[kTeamLanes][K];
    for (int l = 0; l < kTeamLanes; ++l) {
      for (int k = 0; k < K; ++k) s[l][k] = 0.;
      f(l, s[l]);
    }
    for (int w = 0; w < kTeamLanes; w += 64)
      for (int m = 32; m >= 1; m >>= 1)
        for (int l = 0; l < m; ++l)
          for (int k = 0; k < K; ++k) s[w + l][k] = s[w + l][k] + s[w + l + m][k];
    for (int k = 0; k < K; ++k) out[k] = (s[0][k] + s[64][k]) + (s[128][k] + s[192][k]);
  }
  template <class F>
  int count(F f) {
    int c = 0;
    for (int l = 0; l < kTeamLanes; ++l) c += f(l);
    return c;
  }
};

}  // namespace uvo
#endif
