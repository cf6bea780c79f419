// The problem exchange of the per-problem optimisers (poseopt.hip, sim3opt.hip): what a handle owns on the device and in page-locked
// memory, and the two copies of a call.  Each exchange is ONE copy, because its two arrays are adjacent on the device and in the mirror:
// the problem records and then the packed items go up, the result records and then the masks come down.  On the stream a call is
// send, the caller's launch and hipGetLastError, receive (which ends with the call's one synchronise).
#pragma once
#include <cstring>

#include "devmem.hpp"

namespace uvo {

template <class Prob, class Res, class Trace>
struct OptExchange {
  int device = 0, max_problems = 0, max_items = 0, item_floats = 0, last_n = 0;
  hipStream_t stream = nullptr;  // of the handle it was made from; an owner whose stream can change sets it before send and destroy
  DevMem mem;  // owns the device block and the two mirrors
  Prob* prob = nullptr;      // [P]
  float* items = nullptr;    // [sum n][item_floats]
  double* chi2 = nullptr;    // [P * N][chi2_words], used by problems above the kernel's LDS capacity
  uint8_t* state = nullptr;  // [P * N]
  Trace* trace = nullptr;    // [P]
  Res* result = nullptr;     // [P]
  uint8_t* mask = nullptr;   // [sum n]
  Prob* h_prob = nullptr; float* h_items = nullptr;   // the upload's mirror: problem records, then the items
  Res* h_res = nullptr; uint8_t* h_mask = nullptr;    // the download's mirror: result records, then the masks

  // P problems of up to N items at the most; `nomem`: what uvo_last_error() says when the device cannot be set
  int create(int dev, hipStream_t st, int P_, int N_, int floats, int chi2_words, const char* nomem) {
    device = dev, stream = st, max_problems = P_, max_items = N_, item_floats = floats;
    const size_t P = (size_t)P_, N = (size_t)N_;
    auto upload = [&](Carve& c, Prob*& pr, float*& it) { c.take(pr, P).take(it, P * N * floats, alignof(float)); };
    auto download = [&](Carve& c, Res*& res, uint8_t*& mk) { c.take(res, P).take(mk, P * N, alignof(uint8_t)); };
    if (hipSetDevice(device) != hipSuccess) return fail(UVO_E_NOMEM, nomem);
    RC(alloc_carved(mem, [&](Carve& c) {
      upload(c, prob, items);
      c.take(chi2, chi2_words * P * N).take(state, P * N).take(trace, P);
      download(c, result, mask);
    }));
    RC(alloc_carved(mem, [&](Carve& c) { upload(c, h_prob, h_items); }, true));
    return alloc_carved(mem, [&](Carve& c) { download(c, h_res, h_mask); }, true);
  }
  void destroy() {
    hipSetDevice(device);
    if (stream) hipStreamSynchronize(stream);
    mem.release_all();
  }
  int send(size_t total) {  // total: the items of all problems of the call
    UVO_HIP_CHECK(hipSetDevice(device));
    UVO_HIP_CHECK(hipMemcpyAsync(prob, h_prob, (size_t)max_problems * sizeof(Prob) + total * item_floats * sizeof(float), hipMemcpyHostToDevice, stream));
    return UVO_OK;
  }
  int receive(size_t total) {
    UVO_HIP_CHECK(hipMemcpyAsync(h_res, result, (size_t)max_problems * sizeof(Res) + total, hipMemcpyDeviceToHost, stream));
    UVO_HIP_CHECK(hipStreamSynchronize(stream));
    return UVO_OK;
  }
  // CTrace: the C ABI's struct of Trace's layout (the caller asserts the sizes)
  template <class CTrace>
  int read_trace(int problem, CTrace* out) {
    if (problem < 0 || problem >= last_n) return fail(UVO_E_BADARG, "the last call had no such problem");
    UVO_HIP_CHECK(hipSetDevice(device));
    UVO_HIP_CHECK(hipMemcpy(out, trace + problem, sizeof(Trace), hipMemcpyDeviceToHost));
    // records beyond the counts are whatever an earlier call left: not part of the answer
    std::memset(out->lin + out->n_lin, 0, sizeof out->lin - sizeof out->lin[0] * (size_t)out->n_lin);
    std::memset(out->trial + out->n_trials, 0, sizeof out->trial - sizeof out->trial[0] * (size_t)out->n_trials);
    return UVO_OK;
  }
};

}  // namespace uvo
