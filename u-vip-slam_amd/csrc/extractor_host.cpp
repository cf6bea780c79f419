// The host-buffer entry points of the extractor (include/uvo/uvo.h): what replaces USLAM::ORBextractor::operator() for a caller whose
// images, keypoints and results live in host memory.  Each stages a call's inputs on the lane the batch is about to run on, hands the
// batch to run_batch_device (extractor.cpp) and collects the outputs.  Two staging forms:
//   pinned  up to kSmallBatch frames (the default): the kernels read the call's small inputs and write its results in a page-locked
//           region of the handle -- only the image is uploaded, nothing is downloaded
//   direct  larger batches, UVO_TUNE_ZERO_COPY_OUT = 0, or a page-locked block without a device address: explicit copies between the
//           caller's arrays and the handle's device staging
#include <cmath>
#include <cstring>

#include "extractor_priv.hpp"

using namespace uvo;

namespace {

// the one check of an image against what the handle was sized for
int check_image(const uvo_extractor* h, int width, int height, ptrdiff_t stride) {
  if (width < 1 || height < 1 || width > h->cfg.max_width || height > h->cfg.max_height || stride < width ||
      (int64_t)width * height > (int64_t)h->cfg.max_width * h->cfg.max_height)
    return fail(UVO_E_BADARG, "image size outside what the handle was sized for");
  return UVO_OK;
}

// `batch` frames from host memory to tight rows at d_dst, on stream s: one block copy when the source is tight, one 2-D copy per frame otherwise
int upload_frames(hipStream_t s, uint8_t* d_dst, const uint8_t* imgs, int batch, int width, int height, ptrdiff_t stride, ptrdiff_t frame_stride) {
  if (stride == width && (batch == 1 || frame_stride == (ptrdiff_t)width * height)) {
    UVO_HIP_CHECK(hipMemcpyAsync(d_dst, imgs, (size_t)batch * width * height, hipMemcpyHostToDevice, s));
    return UVO_OK;
  }
  for (int b = 0; b < batch; ++b)
    UVO_HIP_CHECK(hipMemcpy2DAsync(d_dst + (size_t)b * width * height, width, imgs + (size_t)b * frame_stride, stride, width, (size_t)height, hipMemcpyHostToDevice, s));
  return UVO_OK;
}

// How a staging form moves bytes: std::memcpy into / out of the page-locked region (hipMemcpyHostToHost), or an asynchronous copy on
// the lane's stream.
struct Mover {
  hipStream_t s;
  hipMemcpyKind kind;
  int operator()(void* dst, const void* src, size_t bytes) const {
    if (kind == hipMemcpyHostToHost) std::memcpy(dst, src, bytes);
    else UVO_HIP_CHECK(hipMemcpyAsync(dst, src, bytes, kind, s));
    return UVO_OK;
  }
};

// The caller's keypoints and their counts to where the kernels read them ([frame][in_cap], like the caller's array): only the first
// n_in[b] entries of a frame's slice are ever read on the device
int put_keypoints(const Batch& c, int in_cap, uvo_keypoint* kp_dst, int32_t* n_dst, const Mover& mv) {
  RC(mv(n_dst, c.n_in, sizeof(int32_t) * c.n));
  for (int b = 0; b < c.n; ++b)
    if (c.n_in[b] > 0) RC(mv(kp_dst + (size_t)b * in_cap, c.in_kp + (size_t)b * in_cap, sizeof(uvo_keypoint) * c.n_in[b]));
  return UVO_OK;
}

// The results to the caller's arrays, c.n_out already in place: frame b's first min(n_out[b], cap) records from slices of dcap records
// (descriptors: when the call has any).  A frame that found more than cap: UVO_E_CAPACITY, and n_out[b] keeps the full count.
int hand_out(const Batch& c, int dcap, const uvo_keypoint* kp, const uint8_t* desc, const Mover& mv) {
  int status = UVO_OK;
  for (int b = 0; b < c.n; ++b) {
    int n = c.n_out[b];
    if (n > c.cap) {
      status = fail(UVO_E_CAPACITY, "output capacity too small; n_out holds the required size");
      n = c.cap;
    }
    n = std::min(n, dcap);
    if (n <= 0) continue;
    RC(mv(c.out_kp + (size_t)b * c.cap, kp + (size_t)b * dcap, sizeof(uvo_keypoint) * n));
    if (desc) RC(mv(c.out_desc + (size_t)b * c.cap * 32, desc + (size_t)b * dcap * 32, (size_t)32 * n));
  }
  return status;
}

// What must hold before anything of a host-buffer call is enqueued.  build_grid (uvo_extract_tracked): the occupancy grid is not an
// input -- it is built on the device from the caller keypoints (src/Tracking.cc:896-912) and only returned (grid may be NULL)
int validate(const uvo_extractor* h, const Batch& c, bool build_grid) {
  if (!h || !c.out_kp || !c.out_desc || !c.n_out) return fail(UVO_E_BADARG, "null pointer");
  if (c.n < 1 || c.n > h->cfg.max_batch) return fail(UVO_E_BADARG, "batch outside 1..max_batch");
  // imgs == NULL: the frame is the result of the last uvo_clahe() call, already in HBM
  if (!c.imgs && (c.n != 1 || !h->d_clahe_out || h->clahe_w != c.width || h->clahe_h != c.height))
    return fail(UVO_E_BADARG, "img == NULL needs a preceding uvo_clahe() of the same size (single frame)");
  RC(check_image(h, c.width, c.height, c.imgs ? c.stride : c.width));
  if (c.full_detect) return UVO_OK;
  if ((!c.grid && !build_grid) || !c.nfn) return fail(UVO_E_BADARG, "top-up mode needs grid2d and num_feats_needed");
  if (!c.in_kp || !c.n_in) return UVO_OK;
  // the reference reads the centre pixel row of a caller keypoint without any bounds check; reject what would
  // leave the padded plane (patch radius 15 + descriptor reach 18 against a 16 px pad).  The blurred plane holds that pad
  // un-blurred out to 16 pixels on such calls (k_blur_pad_level0, gauss.hip).
  const int in_cap = h->cfg.max_input_keypoints;
  for (int b = 0; b < c.n; ++b) {
    if (c.n_in[b] < 0 || c.n_in[b] > in_cap) return fail(UVO_E_BADARG, "n_in outside 0..max_input_keypoints");
    for (int i = 0; i < c.n_in[b]; ++i) {
      const uvo_keypoint& k = c.in_kp[(size_t)b * in_cap + i];
      if (build_grid) {
        // the keypoints only mark grid cells, x = (int)(pt.y / d), y = (int)(pt.x / d) (src/Tracking.cc:905-907): the conversion
        // truncates towards zero and the grid has two cells of slack, so a KLT-tracked point a fraction of a cell outside the image
        // marks a cell like any other (the reference accepts it); what the reference would index OUT of its grid is refused here
        const int gx = (int)(k.y / (float)c.min_px_dist), gy = (int)(k.x / (float)c.min_px_dist);
        if (!(k.x == k.x && k.y == k.y) || fabsf(k.x) > 1e9f || fabsf(k.y) > 1e9f || gx < 0 || gx >= c.grid_rows || gy < 0 || gy >= c.grid_cols)
          return fail(UVO_E_BADARG, "tracked keypoint outside the occupancy grid");
        continue;
      }
      const int cx = (int)lrintf(k.x), cy = (int)lrintf(k.y);
      if (!(cx >= 2 && cx <= c.width - 3 && cy >= 2 && cy <= c.height - 3)) return fail(UVO_E_BADARG, "caller keypoint too close to the border");
    }
  }
  return UVO_OK;
}

// One host-buffer call between its staging and its collection
struct Staged {
  Batch dv;         // the batch as the kernels see it
  size_t gb = 0;    // bytes of the occupancy grids (top-up)
  // pinned form: the page-locked region, [n_out | nfn | n_in : 3 * n ints][grids][keypoints in][keypoints out][descriptors out]
  uint8_t *pin = nullptr, *dev = nullptr;  // as the host and as the device address it; NULL: the direct form
  size_t off_grid = 0, off_in = 0, off_kp = 0, off_desc = 0;
};

// Chooses the form: lays the call out in the handle's page-locked region (grown on demand) when it is a small batch
int choose_form(uvo_extractor* h, const Batch& c, bool have_in, Staged& st) {
  if (c.n > kSmallBatch || !h->zero_copy_out) return UVO_OK;
  const size_t n = (size_t)c.n, dcap = (size_t)h->cap_flist;
  st.off_grid = ((3 * n * sizeof(int32_t)) + 63) & ~(size_t)63;
  st.off_in = (st.off_grid + st.gb + 63) & ~(size_t)63;
  st.off_kp = (st.off_in + (have_in ? n * h->cfg.max_input_keypoints * sizeof(uvo_keypoint) : 0) + 63) & ~(size_t)63;
  st.off_desc = st.off_kp + n * dcap * sizeof(uvo_keypoint);
  const size_t want = st.off_desc + n * dcap * 32;
  if (h->mem.bytes_of(h->h_pin) < want) {
    h->h_pin_dev = nullptr;
    RC(grow(h, h->mem, &h->h_pin, want, true));
    void* dp = nullptr;
    if (hipHostGetDevicePointer(&dp, h->h_pin, 0) == hipSuccess) h->h_pin_dev = (uint8_t*)dp;
  }
  if (h->h_pin_dev) st.pin = h->h_pin, st.dev = h->h_pin_dev;
  return UVO_OK;
}

// The top-up inputs of call c to where the kernels read them (st.dv.nfn / in_kp / n_in say where); the caller's grids only `with_grid`.
// Pinned form: the kernels read the small inputs (feature budget, keypoint counts, the caller's keypoints) where the host put them --
// each host-to-device copy of a few bytes costs a DMA start-up in front of the first kernel.  The stream is in order: the keypoints
// are consumed before the outputs land in the same region.
int stage_topup(uvo_extractor* h, hipStream_t s, const Batch& c, bool have_in, bool with_grid, Staged& st) {
  const int n = c.n, in_cap = h->cfg.max_input_keypoints;
  Batch& dv = st.dv;
  dv.nfn = h->d_nfn, dv.in_kp = h->d_in_kp, dv.n_in = h->d_n_in;
  if (st.pin) {
    int32_t* const ints = (int32_t*)st.pin;
    std::memcpy(ints + n, c.nfn, sizeof(int32_t) * n);
    dv.nfn = (const int32_t*)st.dev + n;
    if (with_grid) {
      std::memcpy(st.pin + st.off_grid, c.grid, st.gb);
      UVO_HIP_CHECK(hipMemcpyAsync(h->d_grid, st.pin + st.off_grid, st.gb, hipMemcpyHostToDevice, s));
    }
    if (!have_in) return UVO_OK;
    dv.in_kp = (const uvo_keypoint*)(st.dev + st.off_in), dv.n_in = (const int32_t*)st.dev + 2 * n;
    return put_keypoints(c, in_cap, (uvo_keypoint*)(st.pin + st.off_in), ints + 2 * n, Mover{s, hipMemcpyHostToHost});
  }
  if (with_grid) UVO_HIP_CHECK(hipMemcpyAsync(h->d_grid, c.grid, st.gb, hipMemcpyHostToDevice, s));
  UVO_HIP_CHECK(hipMemcpyAsync(h->d_nfn, c.nfn, sizeof(int32_t) * n, hipMemcpyHostToDevice, s));
  return have_in ? put_keypoints(c, in_cap, h->d_in_kp, h->d_n_in, Mover{s, hipMemcpyHostToDevice}) : UVO_OK;
}

// Stages the inputs of call c on stream s and fills st.dv.  build_grid (uvo_extract_tracked): the caller's keypoints are the TRACKED
// points, which only fill the occupancy grid -- the extractor itself is called with an empty keypoint vector (`pts0_ext`,
// src/Tracking.cc:943-946) and returns the new points alone
int stage_inputs(uvo_extractor* h, hipStream_t s, const Batch& c, bool build_grid, Staged& st) {
  const int in_cap = h->cfg.max_input_keypoints;
  const bool topup = !c.full_detect;
  const bool have_in = topup && c.in_kp && c.n_in && in_cap > 0;
  st.gb = topup ? (size_t)c.n * c.grid_rows * c.grid_cols * sizeof(int32_t) : 0;
  if (topup) RC(grow(h, h->mem, &h->d_grid, st.gb / sizeof(int32_t)));
  RC(choose_form(h, c, have_in, st));
  // the frames: tight rows on the device (imgs == NULL: the last uvo_clahe() result is there already)
  if (c.imgs) RC(upload_frames(s, h->d_imgs, c.imgs, c.n, c.width, c.height, c.stride, c.frame_stride));
  Batch& dv = st.dv;
  dv = c;
  dv.imgs = c.imgs ? h->d_imgs : h->d_clahe_out;
  dv.stride = c.width, dv.frame_stride = (ptrdiff_t)c.width * c.height;
  dv.grid = nullptr, dv.nfn = nullptr;
  if (topup) {
    dv.grid = h->d_grid;
    RC(stage_topup(h, s, c, have_in, !build_grid, st));
    // build_grid: the occupancy grid is cleared and filled from the tracked keypoints in one launch (no keypoints: cleared)
    if (build_grid) launch_occupancy_grid(s, dv.in_kp, have_in ? dv.n_in : nullptr, have_in ? in_cap : 0, c.min_px_dist, c.grid_rows, c.grid_cols, h->d_grid, c.n);
  }
  if (!have_in || build_grid) dv.in_kp = nullptr, dv.n_in = nullptr;  // nothing for k_describe to pass through
  // the outputs, dcap records per frame (a frame never holds more).  Pinned form: k_describe writes the counts, keypoints and descriptors
  // straight into the region (posted writes over the link: no device-to-host copy -- three DMA start-ups of ~8 us each -- stands between
  // the last kernel and the host)
  dv.cap = h->cap_flist;
  dv.out_kp = st.dev ? (uvo_keypoint*)(st.dev + st.off_kp) : h->d_out_kp;
  dv.out_desc = st.dev ? st.dev + st.off_desc : h->d_out_desc;
  dv.n_out = st.dev ? (int32_t*)st.dev : h->d_n_out;
  return UVO_OK;
}

// Waits for the batch and hands its results (and the mutated grids) to the caller
int collect_outputs(uvo_extractor* h, hipStream_t s, const Batch& c, const Staged& st) {
  const int dcap = h->cap_flist;
  const bool grid_back = !c.full_detect && c.grid;
  const bool spin = h->spin_wait != 0 && c.n <= kSmallBatch;
  if (st.pin) {
    // the counts, the grid and every frame's whole result slice are in the region behind ONE wait
    if (grid_back) UVO_HIP_CHECK(hipMemcpyAsync(st.pin + st.off_grid, h->d_grid, st.gb, hipMemcpyDeviceToHost, s));
    UVO_HIP_CHECK(wait_stream(s, spin));
    std::memcpy(c.n_out, st.pin, sizeof(int32_t) * c.n);
    if (grid_back) std::memcpy(c.grid, st.pin + st.off_grid, st.gb);
    return hand_out(c, dcap, (const uvo_keypoint*)(st.pin + st.off_kp), st.pin + st.off_desc, Mover{s, hipMemcpyHostToHost});
  }
  // the counts first: they size the copies of the records
  UVO_HIP_CHECK(hipMemcpyAsync(c.n_out, h->d_n_out, sizeof(int32_t) * c.n, hipMemcpyDeviceToHost, s));
  UVO_HIP_CHECK(wait_stream(s, spin));
  const int status = hand_out(c, dcap, h->d_out_kp, h->d_out_desc, Mover{s, hipMemcpyDeviceToHost});
  if (status != UVO_OK && status != UVO_E_CAPACITY) return status;
  if (grid_back) UVO_HIP_CHECK(hipMemcpyAsync(c.grid, h->d_grid, st.gb, hipMemcpyDeviceToHost, s));
  UVO_HIP_CHECK(wait_stream(s, spin));
  return status;
}

int extract_host(uvo_extractor* h, const Batch& c, bool build_grid) {
  RC(validate(h, c, build_grid));
  UVO_HIP_CHECK(hipSetDevice(h->device));
  // uploads, kernels and downloads of this call share one lane: the one the batch is about to run on
  const int li = next_lane(h);
  hipStream_t s = h->lane[li].stream;
  Staged st;
  RC(stage_inputs(h, s, c, build_grid, st));
  RC(run_batch_device(h, li, st.dv));
  return collect_outputs(h, s, c, st);
}

}  // namespace

extern "C" {

int uvo_extract_batch(uvo_extractor* h, int batch, const uint8_t* imgs, int width, int height, ptrdiff_t stride, ptrdiff_t frame_stride,
                      const uvo_keypoint* in_kp, const int32_t* n_in, int32_t* grid2d, int grid_rows, int grid_cols, int min_px_dist,
                      int full_detect, const int32_t* num_feats_needed, uvo_keypoint* out_kp, uint8_t* out_desc, int cap, int32_t* n_out) {
  return extract_host(h, Batch{batch, imgs, width, height, stride, frame_stride, in_kp, n_in, grid2d, grid_rows, grid_cols, min_px_dist, full_detect,
                               num_feats_needed, out_kp, out_desc, cap, n_out}, false);
}

int uvo_extract_tracked(uvo_extractor* h, const uint8_t* img, int width, int height, ptrdiff_t stride, const uvo_keypoint* in_kp, int n_in,
                        int min_px_dist, int num_feats_needed, uvo_keypoint* out_kp, uint8_t* out_desc, int cap, int* n_out, int32_t* grid2d_out) {
  if (!h || !n_out) return fail(UVO_E_BADARG, "null pointer");
  if (n_in < 0 || n_in > h->cfg.max_input_keypoints || min_px_dist < 1) return fail(UVO_E_BADARG, "n_in outside 0..max_input_keypoints / min_px_dist < 1");
  // Eigen::MatrixXi::Zero((int)(rows / min_px_dist) + 2, (int)(cols / min_px_dist) + 2): src/Tracking.cc:896
  const int grid_rows = height / min_px_dist + 2, grid_cols = width / min_px_dist + 2;
  int32_t nin = n_in, nfn = num_feats_needed, nout = 0;
  const int rc = extract_host(h, Batch{1, img, width, height, stride, (ptrdiff_t)stride * height, in_kp, &nin, grid2d_out, grid_rows, grid_cols, min_px_dist, 0, &nfn,
                                       out_kp, out_desc, cap, &nout}, true);
  *n_out = nout;
  return rc;
}

int uvo_extract(uvo_extractor* h, const uint8_t* img, int width, int height, ptrdiff_t stride, const uvo_keypoint* in_kp, int n_in,
                int32_t* grid2d, int grid_rows, int grid_cols, int min_px_dist, int full_detect, int num_feats_needed, uvo_keypoint* out_kp,
                uint8_t* out_desc, int cap, int* n_out) {
  if (!h || !n_out) return fail(UVO_E_BADARG, "null pointer");
  if (n_in < 0 || n_in > h->cfg.max_input_keypoints) return fail(UVO_E_BADARG, "n_in outside 0..max_input_keypoints");
  int32_t nin = n_in, nfn = num_feats_needed, nout = 0;
  int rc = uvo_extract_batch(h, 1, img, width, height, stride, (ptrdiff_t)stride * height, in_kp, &nin, grid2d, grid_rows, grid_cols, min_px_dist,
                             full_detect, &nfn, out_kp, out_desc, cap, &nout);
  *n_out = nout;
  return rc;
}

int uvo_host_alloc(void** ptr, size_t bytes) {
  if (!ptr || bytes == 0) return fail(UVO_E_BADARG, "null pointer / zero size");
  if (hipHostMalloc(ptr, bytes, hipHostMallocPortable) != hipSuccess) return fail(UVO_E_NOMEM, "page-locked allocation failed");
  return UVO_OK;
}
int uvo_host_free(void* ptr) {
  if (ptr && hipHostFree(ptr) != hipSuccess) return fail(UVO_E_HIP, "hipHostFree failed");
  return UVO_OK;
}
int uvo_host_register(void* ptr, size_t bytes) {
  if (!ptr || bytes == 0) return fail(UVO_E_BADARG, "null pointer / zero size");
  hipError_t e = hipHostRegister(ptr, bytes, hipHostRegisterPortable);
  if (e != hipSuccess) {
    hip_err_set(e, "hipHostRegister");
    return UVO_E_HIP;
  }
  return UVO_OK;
}
int uvo_host_unregister(void* ptr) {
  if (ptr && hipHostUnregister(ptr) != hipSuccess) return fail(UVO_E_HIP, "hipHostUnregister failed");
  return UVO_OK;
}

// The asynchronous host form with its knobs exposed to the sharder (sharder.cpp): only the first n_download frames' results are
// copied to the caller's arrays (the rest of the batch is a halo whose owner downloads it), `after_kernels` (optional) is recorded
// between the kernels and the downloads, and the device-side descriptors / counts of the batch are handed out so that the matcher
// can read them in HBM (valid until the lane is submitted to again).
int uvo_extract_batch_submit_internal(uvo_extractor* h, int batch, int n_download, const uint8_t* imgs, int width, int height, ptrdiff_t stride,
                                      ptrdiff_t frame_stride, uvo_keypoint* out_kp, uint8_t* out_desc, int cap, int32_t* n_out, int* ticket,
                                      hipEvent_t after_kernels, const uint8_t** d_desc, const int32_t** d_n) {
  if (!h || !imgs || !out_kp || !out_desc || !n_out || !ticket) return fail(UVO_E_BADARG, "null pointer");
  *ticket = -1;
  if (batch < 1 || batch > h->cfg.max_batch || n_download < 0 || n_download > batch) return fail(UVO_E_BADARG, "batch outside 1..max_batch");
  RC(check_image(h, width, height, stride));
  const int dcap = h->cap_flist;
  if (cap < dcap) return fail(UVO_E_CAPACITY, "cap must be at least uvo_extractor_max_keypoints()");
  UVO_HIP_CHECK(hipSetDevice(h->device));
  int rc = set_geometry(h, width, height);  // before the lane is chosen: a geometry change waits for every lane
  if (rc) return rc;
  const int li = next_lane(h);
  Lane& L = h->lane[li];
  if (L.a_batch) return fail(UVO_E_BADARG, "the next lane still has a batch in flight: wait for it first");
  const size_t B = (size_t)h->cfg.max_batch;
  RC(grow(h, L.mem, &L.a_imgs, B * (size_t)h->cfg.max_width * h->cfg.max_height));
  RC(grow(h, L.mem, &L.a_kp, B * dcap));
  RC(grow(h, L.mem, &L.a_desc, B * dcap * 32));
  RC(grow(h, L.mem, &L.a_n, B));
  hipStream_t s = L.stream;
  if (!L.a_uploaded) UVO_HIP_CHECK(hipEventCreateWithFlags(&L.a_uploaded, hipEventDisableTiming));
  if (h->last_upload) UVO_HIP_CHECK(hipStreamWaitEvent(s, h->last_upload, 0));  // uploads take turns on the link (see uvo_extractor::last_upload)
  RC(upload_frames(s, L.a_imgs, imgs, batch, width, height, stride, frame_stride));
  UVO_HIP_CHECK(hipEventRecord(L.a_uploaded, s));
  h->last_upload = L.a_uploaded;
  const int prev_lane = h->cur;
  rc = run_batch_device(h, li, Batch{batch, L.a_imgs, width, height, width, (ptrdiff_t)width * height, nullptr, nullptr, nullptr, 0, 0, 0, 1, nullptr, L.a_kp, L.a_desc, dcap, L.a_n});
  if (rc) {  // no ticket is issued: leave the handle as it was (whatever was enqueued has run out, the lane order is unchanged)
    (void)hipStreamSynchronize(s);
    h->cur = prev_lane;
    return rc;
  }
  if (after_kernels) UVO_HIP_CHECK(hipEventRecord(after_kernels, s));
  // results: whole per-frame slices (a frame holds at most dcap records), frame b lands at b * cap of the caller's arrays
  if (n_download > 0) {
    UVO_HIP_CHECK(hipMemcpyAsync(n_out, L.a_n, sizeof(int32_t) * n_download, hipMemcpyDeviceToHost, s));
    UVO_HIP_CHECK(hipMemcpy2DAsync(out_kp, (size_t)cap * sizeof(uvo_keypoint), L.a_kp, (size_t)dcap * sizeof(uvo_keypoint),
                                   (size_t)dcap * sizeof(uvo_keypoint), (size_t)n_download, hipMemcpyDeviceToHost, s));
    UVO_HIP_CHECK(hipMemcpy2DAsync(out_desc, (size_t)cap * 32, L.a_desc, (size_t)dcap * 32, (size_t)dcap * 32, (size_t)n_download, hipMemcpyDeviceToHost, s));
  }
  L.a_batch = batch;
  *ticket = li;
  if (d_desc) *d_desc = L.a_desc;
  if (d_n) *d_n = L.a_n;
  return UVO_OK;
}

int uvo_extract_batch_submit(uvo_extractor* h, int batch, const uint8_t* imgs, int width, int height, ptrdiff_t stride, ptrdiff_t frame_stride,
                             uvo_keypoint* out_kp, uint8_t* out_desc, int cap, int32_t* n_out, int* ticket) {
  return uvo_extract_batch_submit_internal(h, batch, batch, imgs, width, height, stride, frame_stride, out_kp, out_desc, cap, n_out, ticket, nullptr,
                                           nullptr, nullptr);
}

// 1: the lane's batch has delivered everything (uvo_extract_batch_wait would not block), 0: still running, < 0: error
int uvo_extract_batch_done_internal(uvo_extractor* h, int ticket) {
  if (!h || ticket < 0 || ticket >= kMaxLanes || !h->lane[ticket].stream) return fail(UVO_E_BADARG, "bad ticket");
  if (hipSetDevice(h->device) != hipSuccess) return fail(UVO_E_HIP, "hipSetDevice failed");
  const hipError_t e = hipStreamQuery(h->lane[ticket].stream);
  if (e == hipSuccess) return 1;
  if (e == hipErrorNotReady) return 0;
  hip_err_set(e, "hipStreamQuery");
  return UVO_E_HIP;
}

int uvo_extract_batch_wait(uvo_extractor* h, int ticket) {
  if (!h || ticket < 0 || ticket >= kMaxLanes || !h->lane[ticket].stream) return fail(UVO_E_BADARG, "bad ticket");
  Lane& L = h->lane[ticket];
  if (!L.a_batch) return fail(UVO_E_BADARG, "no batch in flight on this lane");
  UVO_HIP_CHECK(hipSetDevice(h->device));
  const hipError_t e = hipStreamSynchronize(L.stream);
  L.a_batch = 0;  // the lane is free again whatever the wait reports: a failed batch must not block every later one
  if (e != hipSuccess) {
    hip_err_set(e, "hipStreamSynchronize");
    return UVO_E_HIP;
  }
  return UVO_OK;
}

// cv::CLAHE::apply on one host image; the result stays in HBM for uvo_extract(img = NULL) / uvo_klt_build_pyramid_from_extractor()
int uvo_clahe(uvo_extractor* h, const uint8_t* img, int width, int height, ptrdiff_t stride, double clip_limit, int tiles_x, int tiles_y,
              uint8_t* dst, ptrdiff_t dst_stride) {
  if (!h || !img) return fail(UVO_E_BADARG, "null pointer");
  RC(check_image(h, width, height, stride));
  if (dst && dst_stride < width) return fail(UVO_E_BADARG, "dst_stride smaller than the row");
  UVO_HIP_CHECK(hipSetDevice(h->device));
  RC(grow(h, h->mem, &h->d_clahe_out, (size_t)h->cfg.max_width * h->cfg.max_height));
  hipStream_t s = h->lane[next_lane(h)].stream;  // the stream uvo_clahe_batch_device() enqueues on
  RC(upload_frames(s, h->d_imgs, img, 1, width, height, stride, 0));
  int rc = uvo_clahe_batch_device(h, 1, h->d_imgs, width, height, width, (ptrdiff_t)width * height, clip_limit, tiles_x, tiles_y, h->d_clahe_out, width,
                                  (ptrdiff_t)width * height);
  if (rc) return rc;
  h->clahe_w = width, h->clahe_h = height;
  // dst == NULL: the enhanced image stays in HBM only, for uvo_extract(img = NULL) / uvo_klt_build_pyramid_from_extractor()
  if (dst) UVO_HIP_CHECK(hipMemcpy2DAsync(dst, dst_stride, h->d_clahe_out, width, width, (size_t)height, hipMemcpyDeviceToHost, s));
  UVO_HIP_CHECK(hipStreamSynchronize(s));  // the caller's image may be reused
  return UVO_OK;
}

int uvo_grider_fast(uvo_extractor* h, const uint8_t* img, int width, int height, ptrdiff_t stride, int num_features, int grid_x, int grid_y,
                    int threshold, int nonmax_suppression, uvo_keypoint* out_kp, int cap, int* n_out) {
  if (!h || !img || !out_kp || !n_out) return fail(UVO_E_BADARG, "null pointer");
  *n_out = 0;
  if (width < 7 || height < 7 || width > 4096 || height > 4096 || stride < width || grid_x < 1 || grid_y < 1 || num_features < 0 || cap < 1)
    return fail(UVO_E_BADARG, "bad image size / grid");
  if ((int64_t)width * height > (int64_t)h->cfg.max_width * h->cfg.max_height) return fail(UVO_E_BADARG, "image larger than the handle was sized for");
  const int size_x = width / grid_x, size_y = height / grid_y;
  if (size_x < 1 || size_y < 1) return fail(UVO_E_BADARG, "grid finer than the image (the reference asserts size > 0)");
  const int rois = (width / size_x) * (height / size_y);
  const int keep = num_features / (grid_x * grid_y) + 1;
  Lane& L = h->lane[0];
  if ((size_t)width * height > h->cap_cor || (size_t)rois > h->cap_cor_n)
    return fail(UVO_E_BADARG, "image / grid larger than the handle's scratch");
  const int64_t dcap = (int64_t)h->cfg.max_batch * h->cap_flist;
  if ((int64_t)rois * keep > dcap) return fail(UVO_E_CAPACITY, "num_features + cells exceeds the handle's output staging");
  UVO_HIP_CHECK(hipSetDevice(h->device));
  RC(sync_all_lanes(h));  // lane 0's corner scratch and the handle's staging are borrowed
  RC(grow(h, h->mem, &h->d_grid_score, (size_t)h->cfg.max_width * h->cfg.max_height));
  hipStream_t s = L.stream;
  RC(upload_frames(s, h->d_imgs, img, 1, width, height, stride, 0));
  UVO_HIP_CHECK(hipMemsetAsync(h->d_n_out, 0, sizeof(int32_t), s));
  launch_grider(s, h->d_imgs, width, height, width, num_features, grid_x, grid_y, threshold, nonmax_suppression ? 1 : 0, h->d_grid_score, L.d.cor,
                L.d.cor_n, h->d_out_kp, (int)std::min<int64_t>(dcap, 1 << 30), h->d_n_out);
  UVO_HIP_CHECK(hipGetLastError());
  int32_t n = 0;
  UVO_HIP_CHECK(hipMemcpyAsync(&n, h->d_n_out, 4, hipMemcpyDeviceToHost, s));
  UVO_HIP_CHECK(hipStreamSynchronize(s));
  *n_out = n;
  Batch c{};  // one frame of keypoints, no descriptors
  c.n = 1, c.out_kp = out_kp, c.cap = cap, c.n_out = &n;
  const int status = hand_out(c, (int)std::min<int64_t>(dcap, 1 << 30), h->d_out_kp, nullptr, Mover{s, hipMemcpyDeviceToHost});
  UVO_HIP_CHECK(hipStreamSynchronize(s));
  return status;
}

}  // extern "C"
