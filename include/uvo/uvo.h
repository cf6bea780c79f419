/*
 * uvo.h -- C ABI of the MI355X-native ORB feature front-end (extract + match).
 *
 * This is the drop-in boundary for the hot path of chintha/U-VIP-SLAM.  The reference has no FFI layer:
 * the path is entered through two concrete C++ classes.  Each entry point below names the reference
 * interface it replaces (file:line relative to the reference tree); include/uvo/compat/ holds C++
 * adaptors with the reference's own class/method signatures on top of this ABI, and INTEGRATION.md shows
 * the binding a maintainer would add.
 *
 * Conventions
 *   - every function returns 0 (UVO_OK) or a negative UVO_E_* code; nothing throws across the ABI.
 *   - plain pointers and sizes only; "host" pointers are ordinary CPU memory, "device" pointers are HBM
 *     addresses on the handle's GPU (hipMalloc / torch.cuda tensors).
 *   - a handle owns all device scratch (sized at create time), one HIP stream and its pinned staging;
 *     one handle = one in-flight call; use one handle per GPU / per host thread.
 *   - there is NO CPU fallback: if no gfx950 device is usable, create() fails with UVO_E_NODEVICE.
 */
#ifndef UVO_UVO_H_
#define UVO_UVO_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UVO_OK 0
#define UVO_E_BADARG (-1)      /* null pointer, non-positive size, image larger than the handle was sized for */
#define UVO_E_NODEVICE (-2)    /* no usable HIP device / kernels not loadable */
#define UVO_E_HIP (-3)         /* a HIP runtime call failed; see uvo_last_error() */
#define UVO_E_CAPACITY (-4)    /* caller's output capacity too small (n_out still reports what was needed) */
#define UVO_E_UNSUPPORTED (-5) /* geometry outside the supported envelope (see uvo_extractor_create) */
#define UVO_E_NOMEM (-6)

/* Layout-identical to cv::KeyPoint (28 bytes): pt.x, pt.y, size, angle, response, octave, class_id. */
typedef struct uvo_keypoint {
  float x, y;
  float size;
  float angle;
  float response;
  int32_t octave;
  int32_t class_id;
} uvo_keypoint;

/* ------------------------------------------------------------------------------------------------
 * Extractor -- replaces USLAM::ORBextractor (include/ORBextractor.h:47-95, src/ORBextractor.cc).
 * ---------------------------------------------------------------------------------------------- */
typedef struct uvo_extractor uvo_extractor;

typedef struct uvo_extractor_cfg {
  /* ORBextractor::ORBextractor(nfeatures, scaleFactor, nlevels, scoreType, fastTh): include/ORBextractor.h:51 */
  int32_t nfeatures;
  float scale_factor;
  int32_t nlevels;
  int32_t score_type; /* accepted and ignored, exactly like the live reference path */
  int32_t fast_th;    /* >= 0; values above 255 act as 255 (cv::FAST clamps its threshold the same way) */
  /* sizing of the device scratch owned by the handle */
  int32_t max_width, max_height; /* largest frame; every pyramid level must keep >= 56 px per side */
  int32_t max_batch;             /* frames per uvo_extract_batch* call */
  int32_t max_input_keypoints;   /* per frame: caller keypoints passed through level 0 (top-up mode) */
  int32_t device;                /* HIP device ordinal */
} uvo_extractor_cfg;

/*
 * The supported envelope.  The reference has none of these limits (it allocates as it goes); here they bound the kernels' LDS and
 * register budgets, and a configuration or image outside them is refused with UVO_E_UNSUPPORTED -- by uvo_extractor_create() for
 * max_width x max_height, and by every extract call for the size it is given -- never computed approximately:
 *   - every pyramid level must measure 56 .. 4096 px on each side (level l is round(size * invScaleFactor^l),
 *     src/ORBextractor.cc:966-969; below 56 px the 30-px FAST cell grid of :755-770 has no cell);
 *   - a FAST cell ROI (wCell + 6 x hCell + 6, :773-790) may not exceed 66 x 66 px (true whenever the detection window of the
 *     level is at least 30 px on each side);
 *   - a level's feature quota mnFeaturesPerLevel[l] (:472-485) may not exceed 2000 (with the reference's 1.2 / 8 levels that is
 *     nfeatures <= ~9200);
 *   - the number of quad-tree roots of a level, round(window width / window height) (:1010), must be 1 .. 64 (`nIni = 0`, an image
 *     more than twice as high as wide, divides by zero in the reference too);
 *   - at most 2^24 FAST cells per frame; nlevels <= 16.
 * Sizes below max_width x max_height.  A handle takes any image whose sides are both within its maximum and that is inside the
 * envelope above by itself -- not every such size is: the rules hold for EVERY level of the image's own pyramid.  The smallest square is
 * the first side whose last level, round(side * invScaleFactor^(nlevels - 1)), still measures 56 px (96 at 1.2 / 4 levels, 99 at
 * 1.33 / 3; one pixel less is UVO_E_UNSUPPORTED), and the root rule applies to each level's detection window (the level minus 26 px):
 * 150 x 256 is taken at 1.2 / 4 levels (last window 61 x 122, one root) and refused at 1.33 / 3 (59 x 119 rounds to no root) although
 * the image is not twice as high as wide.  The host-buffer forms check both sides (UVO_E_BADARG beyond either);
 * uvo_extract_batch_device checks no side, only the capacities the handle was sized with: other shapes of at most the maximum's area
 * are taken only where they fit every one of them and refused with UVO_E_BADARG where they do not (the transposed shape 256 x 320 on
 * a 320 x 256 handle: its planes, or at three levels its row tables, do not fit).  A refused call of either kind leaves the handle as
 * it was.
 * uvo_sharder additionally needs uvo_extractor_max_keypoints() <= 65535 when it matches (train indices are packed in 16 bits).
 */
int uvo_extractor_create(const uvo_extractor_cfg* cfg, uvo_extractor** out);
void uvo_extractor_destroy(uvo_extractor* h);

/* ORBextractor::GetLevels / GetScaleFactor: include/ORBextractor.h:60-64 */
/* Largest number of keypoints one frame can return with this handle (sum over levels of max(quota, 4 * nIni) + 4, plus
 * max_input_keypoints): the output capacity that can never overflow.  Negative = error code. */
int uvo_extractor_max_keypoints(const uvo_extractor* h);
int uvo_extractor_levels(const uvo_extractor* h);
float uvo_extractor_scale_factor(const uvo_extractor* h);
/* constructor tables (mvScaleFactor, mvInvScaleFactor, mnFeaturesPerLevel, umax[16]): src/ORBextractor.cc:463-511 */
int uvo_extractor_tables(const uvo_extractor* h, float* scale, float* inv_scale, int32_t* quota, int32_t* umax16);

/*
 * ORBextractor::operator()(image, mask, keypoints, descriptors, grid_2d, min_px_dist, FullDetect,
 * num_featsneeded): include/ORBextractor.h:56-58, src/ORBextractor.cc:849-961; call site src/Tracking.cc:946.
 *   img/width/height/stride : CV_8UC1 host image
 *   in_kp/n_in              : caller keypoints (reference: `keypoints` on entry); passed through level 0
 *                             with recomputed angle when full_detect == 0, dropped when full_detect != 0.
 *                             Accepted range (full_detect == 0): the centre (cvRound(x), cvRound(y)), halves to
 *                             the even neighbour, lies in [2, width - 3] x [2, height - 3] -- the orientation
 *                             patch (15 pixels) and the steered pattern (18) then stay inside the 16-pixel
 *                             REFLECT_101 border, which the descriptor samples un-blurred as the reference
 *                             does.  Any other centre: UVO_E_BADARG, nothing is written.  x and y come back
 *                             as given, unrounded.
 *   grid2d                  : Eigen::MatrixXi::data() -- column-major int32, grid_rows x grid_cols,
 *                             read and MUTATED when full_detect == 0 (may be NULL when full_detect != 0)
 *   num_feats_needed        : the reference's num_featsneeded (full_detect == 0), with its arithmetic: level l
 *                             stops after num_feats_needed * (8 - l) / 30 accepted points (int division; the
 *                             count carries over from levels that ran out of points first), the call after
 *                             num_feats_needed.  Both tests are `==`, the level's first: 30 return 36.  At and
 *                             below zero nothing is refused and no test can ever hold -- as for levels past
 *                             the eighth -- so every detected point in a free cell is returned.
 *   out_kp/out_desc/cap     : caller buffers for up to `cap` keypoints (28 B) and descriptors (32 B)
 *   n_out                   : number of keypoints produced (reference: keypoints.size() on return)
 * A cell of grid2d is free while it is <= 0 and is incremented per accepted point: a cell below zero takes
 * more than one.
 * Keypoints come out level-major in the reference's list order; nothing is truncated to nfeatures.
 */
int uvo_extract(uvo_extractor* h, const uint8_t* img, int width, int height, ptrdiff_t stride, const uvo_keypoint* in_kp, int n_in,
                int32_t* grid2d, int grid_rows, int grid_cols, int min_px_dist, int full_detect, int num_feats_needed,
                uvo_keypoint* out_kp, uint8_t* out_desc, int cap, int* n_out);

/*
 * The top-up call together with the caller's loop in front of it (src/Tracking.cc:896-946): the occupancy grid is built on the
 * device from the tracked keypoints -- grid_2d((int)(pt.y / min_px_dist), (int)(pt.x / min_px_dist))++ on a zero matrix of
 * (height / min_px_dist + 2) x (width / min_px_dist + 2) -- and the extraction runs with FullDetect = false on it, with an EMPTY
 * keypoint vector as at :946 (`pts0_ext`): in_kp are the tracked keypoints `pts0`, which only fill the grid (they must lie inside the
 * image); out_kp / out_desc hold the NEW keypoints and descriptors alone (`pts0_ext`, `New_Descriptors`), which the caller appends
 * to its own (:948-959).  grid2d_out (optional): the grid after the call, column-major, for callers that keep it.  img == NULL: the
 * result of the last uvo_clahe(), as in uvo_extract.
 */
int uvo_extract_tracked(uvo_extractor* h, const uint8_t* img, int width, int height, ptrdiff_t stride, const uvo_keypoint* in_kp, int n_in,
                        int min_px_dist, int num_feats_needed, uvo_keypoint* out_kp, uint8_t* out_desc, int cap, int* n_out, int32_t* grid2d_out);

/*
 * Batched form of the same call (B independent frames, one launch per stage).  Host buffers:
 *   imgs           : frame b at imgs + b*frame_stride, rows `stride` bytes apart
 *   in_kp / n_in   : [B][max_input_keypoints] / [B]   (NULL / NULL when there are none)
 *   grid2d         : [B][grid_rows*grid_cols] column-major each (NULL when full_detect != 0)
 *   num_feats_needed : [B] (ignored when full_detect != 0; may be NULL then)
 *   out_kp/out_desc: [B][cap] / [B][cap][32];  n_out: [B]
 */
int uvo_extract_batch(uvo_extractor* h, int batch, const uint8_t* imgs, int width, int height, ptrdiff_t stride, ptrdiff_t frame_stride,
                      const uvo_keypoint* in_kp, const int32_t* n_in, int32_t* grid2d, int grid_rows, int grid_cols, int min_px_dist,
                      int full_detect, const int32_t* num_feats_needed, uvo_keypoint* out_kp, uint8_t* out_desc, int cap,
                      int32_t* n_out);

/*
 * Asynchronous host-buffer form (FullDetect): uvo_extract_batch_submit() enqueues the upload of the frames, the extraction and
 * the download of the results on the next pipeline lane and returns at once with a ticket (the lane); uvo_extract_batch_wait()
 * blocks until that lane has finished.  With uvo_extractor_set_pipeline(h, 2) and page-locked buffers (uvo_host_alloc) the
 * PCIe transfers of one batch overlap the kernels of the other: submit(k+1), wait(k), consume k, ...
 *   imgs, out_kp, out_desc, n_out must stay valid and untouched until the matching wait returns; a lane must be waited for
 *   before it is submitted to again (with depth d: at most d batches in flight).
 *   out_kp / out_desc: [B][cap] / [B][cap][32]; records past n_out[b] are unspecified.  cap must be >= uvo_extractor_max_keypoints().
 */
int uvo_host_alloc(void** ptr, size_t bytes);
int uvo_host_free(void* ptr);
int uvo_extract_batch_submit(uvo_extractor* h, int batch, const uint8_t* imgs, int width, int height, ptrdiff_t stride, ptrdiff_t frame_stride,
                             uvo_keypoint* out_kp, uint8_t* out_desc, int cap, int32_t* n_out, int* ticket);
int uvo_extract_batch_wait(uvo_extractor* h, int ticket);
/*
 * Placement of the host side next to a GPU (N ranks on a two-socket host: every rank's frames leave over the PCIe link of ITS GPU).
 * uvo_host_bind_near_device() binds the CALLING THREAD to the CPUs local to `device` (Linux: /sys/bus/pci/devices/<bdf>/local_cpulist,
 * intersected with the CPUs the process may use) and reports the device's NUMA node (-1: unknown); memory the thread touches first
 * afterwards -- its frames, its slice of a shared gather region, before uvo_host_register() -- then lands on that node.  Returns 1 when the
 * thread was bound, 0 when there was nothing to do (no sysfs entry, no usable CPU in the list: the thread stays where it was), < 0 on error.
 * The sharder's per-shard threads bind themselves this way (environment UVO_NUMA_BIND=0 turns every binding of this library into a no-op:
 * for hosts that place their processes themselves).  uvo_host_bind_to_cpulist_file() is the same for an explicit cpulist file.
 */
int uvo_host_bind_near_device(int device, int32_t* numa_node);
int uvo_host_bind_to_cpulist_file(const char* cpulist_path);
/* Page-lock memory the caller already owns (e.g. a shared mapping that several processes gather into); uvo_host_alloc()'s sibling. */
int uvo_host_register(void* ptr, size_t bytes);
int uvo_host_unregister(void* ptr);

/* ------------------------------------------------------------------------------------------------
 * Sharder -- one job of `total` frames over N GPUs of one node, no collective.
 * The reference has one extractor call per frame on one thread (src/Tracking.cc:946); an offline
 * mapping run (BASELINE.json configs[3]) is that call over a whole sequence.  Frames are independent:
 * shard i owns one contiguous block, runs it on its own device from its own host thread in chunks
 * (two in flight: the upload of one under the kernels of the other), and every chunk's results are
 * copied straight to element frame * cap of ONE set of caller arrays -- the gather is those copies.
 * With match = 1 pair p = (frame p, frame p + 1) is matched (all-pairs knn-2, uvo_hamming_knn2) by the
 * shard that owns frame p; the last pair of a chunk needs the next frame's descriptors, so a chunk
 * extracts one halo frame beyond its own (at a shard's end: the neighbouring shard's first frame,
 * recomputed here, bit-identical to the neighbour's own copy) rather than exchanging descriptors.
 * ---------------------------------------------------------------------------------------------- */
#define UVO_SHARD_MAX 64
#define UVO_SHARD_REMOTE (-1) /* devices[i]: shard i is run by another process (same plan, same offsets) */
typedef struct uvo_sharder uvo_sharder;
typedef struct uvo_sharder_cfg {
  uvo_extractor_cfg extractor;    /* device / max_batch / max_input_keypoints are set per shard by the sharder */
  int32_t n_shards;
  int32_t devices[UVO_SHARD_MAX]; /* HIP device ordinal of shard i (ordinals may repeat), or UVO_SHARD_REMOTE */
  int32_t chunk_frames;           /* frames per chunk (per device launch sequence); device scratch is sized for chunk_frames + 1 */
  int32_t match;                  /* 1: also the knn-2 rows of consecutive frames */
} uvo_sharder_cfg;
/* The block of shard `shard` and what it matches -- pure arithmetic, no device needed. */
typedef struct uvo_shard_plan {
  int32_t first_frame, n_frames; /* frames [first_frame, first_frame + n_frames): results at element first_frame * cap of the outputs */
  int32_t first_pair, n_pairs;   /* pairs p = (p, p + 1), p in [first_pair, first_pair + n_pairs): rows at element p * cap */
  int32_t halo_frame;            /* the neighbouring shard's first frame, extracted here too for the block's last pair; -1 = none */
  int32_t n_chunks;
} uvo_shard_plan;
int uvo_shard_plan_make(int total_frames, int n_shards, int shard, int chunk_frames, uvo_shard_plan* out);
int uvo_sharder_create(const uvo_sharder_cfg* cfg, uvo_sharder** out);
void uvo_sharder_destroy(uvo_sharder* s);
int uvo_sharder_max_keypoints(const uvo_sharder* s); /* smallest `cap` uvo_sharder_run accepts */
/*
 * Run the local shards of a job.  uvo_sharder_submit() queues the job for the shard threads and returns a ticket at once,
 * uvo_sharder_wait() blocks until the job's results are in the output arrays; uvo_sharder_run() is the two together.  Jobs run in
 * submission order and the lanes are not drained between them: with a second job submitted before the first is waited for, the
 * uploads of one run under the kernels of the other (a stream of jobs moves at the steady-state rate of the pipeline lanes).
 *   imgs, n_imgs     : n_imgs host frames, frame g at imgs + (g - imgs_first_frame) * frame_stride (a process that owns only some
 *                      shards need only hold their frames and each block's halo frame: UVO_E_BADARG when a local shard's frames or
 *                      its halo frame lie outside [imgs_first_frame, imgs_first_frame + n_imgs)); page-locked memory makes the
 *                      uploads asynchronous
 *   out_kp / out_desc / n_out : [total][cap] / [total][cap][32] / [total]   (cap >= uvo_sharder_max_keypoints())
 *   idx0 / d0 / idx1 / d1     : [total - 1][cap] knn-2 rows of pair p (row q = keypoint q of frame p; as uvo_hamming_knn2), or all NULL
 * Only the elements of the local shards' frames / pairs are written.  All buffers of a job must stay valid and untouched until its
 * wait returns; jobs in flight at the same time need their own output arrays.
 */
int uvo_sharder_submit(uvo_sharder* s, const uint8_t* imgs, int n_imgs, int imgs_first_frame, int total_frames, int width, int height,
                       ptrdiff_t stride, ptrdiff_t frame_stride, uvo_keypoint* out_kp, uint8_t* out_desc, int cap, int32_t* n_out, int32_t* idx0, uint16_t* d0,
                       int32_t* idx1, uint16_t* d1, int* ticket);
int uvo_sharder_wait(uvo_sharder* s, int ticket);
int uvo_sharder_run(uvo_sharder* s, const uint8_t* imgs, int n_imgs, int imgs_first_frame, int total_frames, int width, int height,
                    ptrdiff_t stride, ptrdiff_t frame_stride, uvo_keypoint* out_kp, uint8_t* out_desc, int cap, int32_t* n_out, int32_t* idx0, uint16_t* d0,
                    int32_t* idx1, uint16_t* d1);

/*
 * HBM-resident form: every pointer is a device pointer on the handle's GPU and the call only enqueues work
 * on the handle's stream (uvo_extractor_synchronize() waits for it).  Same argument meaning as above.
 * d_n_out[b] may exceed `cap`; only the first `cap` records of a frame are written in that case.
 * A pipeline lane keeps at most two batches outstanding: the call first waits (on the host) for the lane's last but one batch, so a
 * caller that enqueues in a loop runs two to four batches ahead of the device and no further.
 * d_imgs must stay valid AND UNCHANGED until the batch has completed: with dword-aligned rows (d_imgs, stride, frame_stride multiples of
 * 4, width a multiple of 4) and no caller keypoints, level 0 of the pyramid is the caller's image itself, read in place by every stage
 * (UVO_TUNE_LEVEL0_INPLACE; cv::copyMakeBorder of src/ORBextractor.cc:996 is never materialised).  Results do not depend on it.
 */
int uvo_extract_batch_device(uvo_extractor* h, int batch, const uint8_t* d_imgs, int width, int height, ptrdiff_t stride,
                             ptrdiff_t frame_stride, const uvo_keypoint* d_in_kp, const int32_t* d_n_in, int32_t* d_grid2d, int grid_rows,
                             int grid_cols, int min_px_dist, int full_detect, const int32_t* d_num_feats_needed, uvo_keypoint* d_out_kp,
                             uint8_t* d_out_desc, int cap, int32_t* d_n_out);
int uvo_extractor_synchronize(uvo_extractor* h);
/*
 * Pipeline depth of the HBM-resident form (default 1).  With depth 2 the handle owns two scratch sets and two
 * streams and consecutive uvo_extract_batch_device() calls alternate between them, so the latency-bound stages of one
 * batch overlap with the streaming stages of the next.  The caller must then give consecutive calls different output
 * buffers.  uvo_matcher_wait_extractor() / uvo_extractor_wait_matcher() refer to the most recently used stream.
 */
int uvo_extractor_set_pipeline(uvo_extractor* h, int depth);
/*
 * Launch-shape knobs of one handle (speed only -- results never depend on them; the parity tests force each shape).
 *   UVO_TUNE_OCT_WIDE_MAX : batches with at most this many (frame, level) quad-tree problems run DistributeOctTree
 *                           (src/ORBextractor.cc:1006-1230) as 1024-thread workgroups, larger ones as 256-thread workgroups
 *                           (default 0 = always the 256-thread form, which shares its launch with the blur; a large value = always the 1024-thread form).
 */
#define UVO_TUNE_OCT_WIDE_MAX 1
/*
 *   UVO_TUNE_FAST_MODE    : how the per-cell threshold fallback of src/ORBextractor.cc:792-799 (`FAST(cell, fastTh)`, and
 *                           `FAST(cell, 7)` when that finds nothing) is computed when fastTh > 7.
 *                           UVO_FAST_MODE_TWO_PASS    every level streams once at fastTh; the cells left without a keypoint are
 *                                                     redone at the literal 7 by a sparse per-cell kernel;
 *                           UVO_FAST_MODE_SINGLE_PASS every level streams once at 7 and the per-cell vote picks the class;
 *                           UVO_FAST_MODE_ADAPTIVE    (default) per level and pipeline lane, whichever was cheaper for the previous
 *                                                     batch's share of fall-back cells (decided on the device, no host round trip).
 *                           The keypoints are the same in every mode.
 */
#define UVO_TUNE_FAST_MODE 2
#define UVO_FAST_MODE_ADAPTIVE 0
#define UVO_FAST_MODE_TWO_PASS 1
#define UVO_FAST_MODE_SINGLE_PASS 2
/*
 *   UVO_TUNE_BLUR_ROUNDING : the ONE knob that changes results -- which OpenCV build's GaussianBlur (src/ORBextractor.cc:942) is
 *                           reproduced where the two differ: an exact .5 in the column pass of the 7 x 7 blur (about one pixel in
 *                           65 536, by one grey level; descriptors follow).
 *                           UVO_BLUR_ROUNDING_SSE2   (default) x86-64 builds -- the reference is an x86-64 ROS program: the vector body of
 *                                                     SymmColumnVec_32s8u (image columns 0 .. (w & ~3) - 1) converts the exact fp32 sum with
 *                                                     cvtps2dq, half to EVEN; only the last w % 4 columns take the scalar loop, half up;
 *                           UVO_BLUR_ROUNDING_SCALAR  the generic C++ column filter: (sum + 2^15) >> 16, half up, on every column (builds
 *                                                     without SIMD).
 *                           tools/pin/ dumps the evidence that decides it for a given OpenCV binary (the gauss_<k> cases).
 */
#define UVO_TUNE_LEVEL0_INPLACE 11 /* 1 (default): level 0 is read from the caller's image in place whenever it can be (dword-aligned rows, width a
                                     multiple of 4, no caller keypoints): cv::copyMakeBorder of src/ORBextractor.cc:996 is never materialised, the
                                     blur reflects the border it needs on the fly; 0: always copy into a padded plane first */
#define UVO_TUNE_BLUR_ROUNDING 9
#define UVO_BLUR_ROUNDING_SCALAR 0
#define UVO_BLUR_ROUNDING_SSE2 1
int uvo_extractor_tune(uvo_extractor* h, int knob, int value);
/*
 * State of the adaptive FAST mode after the most recent batch (waits for it): per level the threshold the NEXT batch on that
 * pipeline lane streams at (fastTh = two-pass form, <= 7 = single pass), the fall-back cells the last batch counted (cells without a
 * keypoint at fastTh, summed over its frames) and the level's cells per frame.  Arrays of uvo_extractor_levels() entries; any may be NULL.
 */
int uvo_extractor_fast_state(uvo_extractor* h, int32_t* pass_threshold, int32_t* fallback_cells, int32_t* cells_per_frame);

/*
 * Grid-bucketed FAST -- Grider_FAST::perform_griding(img, pts, num_features, grid_x, grid_y, threshold, nonmaxSuppression)
 * (include/Grider_FAST.h:81-137; the OpenVINS helper north_star names; its only call, src/Tracking.cc:940, is commented
 * out in the reference, so this is the alternative bucketing mode).  Host buffers; keypoints come out ROI-major, inside
 * a ROI by response descending, then y, then x (the reference's std::sort leaves ties unspecified).  Uses the
 * extractor handle's device scratch; the image must fit max_width x max_height.
 * A ROI is (width / grid_x) x (height / grid_y) pixels and FAST looks at its 3-pixel-inset interior only: a ROI narrower
 * or lower than 7 pixels has no interior and yields nothing (UVO_OK with *n_out = 0 when no ROI has one), as cv::FAST does
 * on such a ROI.  At most (num_features / (grid_x * grid_y) + 1) * (width / size_x) * (height / size_y) keypoints come
 * out -- there can be more ROIs than grid cells; with a smaller cap the call returns UVO_E_CAPACITY and *n_out holds the count.
 */
int uvo_grider_fast(uvo_extractor* h, const uint8_t* img, int width, int height, ptrdiff_t stride, int num_features, int grid_x, int grid_y,
                    int threshold, int nonmax_suppression, uvo_keypoint* out_kp, int cap, int* n_out);

/*
 * cv::CLAHE::apply (8-bit), the pre-processing of Tracking::GrabImage when Enhance = 1 (src/Tracking.cc:425-431: clip limit 4,
 * 12 x 12 tiles): per-tile clipped histogram LUTs on the image extended by REFLECT_101 to a multiple of the tile grid, then the
 * bilinear blend of the four neighbouring LUTs per pixel.  In place is allowed (dst == src, same strides).
 * uvo_clahe: host buffers, one frame; the enhanced frame also stays in the handle's HBM, so that the calls that follow in
 * Tracking::GrabImage need no second upload: uvo_extract(img = NULL, same width / height) extracts from it and
 * uvo_klt_build_pyramid_from_extractor() builds the optical-flow pyramid from it; dst = NULL skips the download altogether.
 * uvo_clahe_batch_device: HBM-resident, enqueued on the stream the next
 * uvo_extract_batch_device() call of this handle will use, so that enhance -> extract needs no synchronisation in between.
 */
int uvo_clahe(uvo_extractor* h, const uint8_t* img, int width, int height, ptrdiff_t stride, double clip_limit, int tiles_x, int tiles_y,
              uint8_t* dst, ptrdiff_t dst_stride);
int uvo_clahe_batch_device(uvo_extractor* h, int batch, const uint8_t* d_imgs, int width, int height, ptrdiff_t stride, ptrdiff_t frame_stride,
                           double clip_limit, int tiles_x, int tiles_y, uint8_t* d_dst, ptrdiff_t dst_stride, ptrdiff_t dst_frame_stride);

/* Stage taps for the parity tests (valid after a completed extract call; host destination buffers). */
int uvo_extractor_level_dims(const uvo_extractor* h, int level, int* width, int* height);
/* padded plane (width+32) x (height+32), tight rows; which: 0 = pyramid level, 1 = blurred level */
int uvo_extractor_read_plane(uvo_extractor* h, int frame, int level, int which, uint8_t* dst);
/* FAST candidates of one level: (x, y, score) int32 triples relative to the (13,13) detection border,
 * unordered; returns count via n */
int uvo_extractor_read_candidates(uvo_extractor* h, int frame, int level, int32_t* dst_xys, int cap, int* n);
/* The quad-tree launch of the current lane on candidate lists of the caller's choosing, in place of what the FAST kernels leave: for
 * every problem q = frame * nlevels + level of a batch 1 .. max_batch, n_hi[q] "high" (survivors >= fastTh) and n_lo[q] "low" (x, y, score)
 * int32 triples, the problems' lists one behind the other in hi_xys / lo_xys, coordinates relative to the (13,13) detection border; and
 * per frame the cell-flag bytes, the full nRows x nCols grid of level 0, then of level 1 ... (flags_per_frame bytes).  The 256- or
 * 1024-thread form is chosen as in an extract call (UVO_TUNE_OCT_WIDE_MAX).  Out, per problem: sel_count, cand_count (the gathered
 * list: the high entries and every low entry with score >= 7 in a cell whose flag is zero), fcount (zero flags of grid positions that
 * are cells), and the first min(sel_count, sel_cap) selected (x, y, score) triples in the kernel's order at sel_xys[3 * q * sel_cap];
 * per call: the threads per workgroup launched, residue[0] / [1] = cursor words / flag bytes of the batch that the launch left
 * non-zero (it promises none).  UVO_E_BADARG, with nothing on the device touched: no geometry yet, batch out of range, a coordinate
 * outside [3, bw - 3) x [3, bh - 3) of its level's window (bw = width - 26), a score outside 0 .. 255, more than the level's candidate
 * capacity in both lists together, the same (x, y) twice in one problem, flags_per_frame not the handle's. */
int uvo_extractor_octree_tap(uvo_extractor* h, int batch, const int32_t* n_hi, const int32_t* n_lo, const int32_t* hi_xys, const int32_t* lo_xys,
                             const uint8_t* cell_flags, int flags_per_frame, int32_t* sel_count, int32_t* cand_count, int32_t* fcount, int32_t* sel_xys,
                             int sel_cap, int32_t* threads, int32_t* residue);

/*
 * Per-kernel device timing, measured with HIP events on the handle's stream around every launch made while
 * profiling is enabled (uvo_extractor_profile(h, 1); adds two event records per launch).
 * uvo_extractor_kernel_times() waits for the stream, then reports and clears what was recorded:
 * names: '\n'-separated kernel names into `names` (cap bytes); ms[i]: summed duration of that kernel's launches;
 * launches[i]: number of launches.  Behind the kernels' rows, while `cap` allows, follow spread rows for every kernel with two or more
 * launches: "name:min" / "name:p50" / "name:max" = shortest / median / longest single launch (ms), and "name:period_min" / ":period_p50" /
 * ":period_max" = start-to-start time of consecutive launches in enqueue order across the pipeline lanes (for a kernel launched once per
 * batch: the step period as the device saw it), and "name:period2_min" / ":period2_p50" / ":period2_max" = half the start-to-start time of
 * launches two apart (two pipeline lanes take the batches in turn: one lane's period per step, whatever the phase between the lanes);
 * launches[i] of a spread row = the number of samples behind it.
 */
int uvo_extractor_profile(uvo_extractor* h, int enable);
/* restricts the timing to launches of one kernel (name as reported by uvo_extractor_kernel_times; NULL or "" = all kernels) */
int uvo_extractor_profile_only(uvo_extractor* h, const char* kernel_name);
int uvo_extractor_kernel_times(uvo_extractor* h, char* names, int names_cap, float* ms, int32_t* launches, int cap, int* n);

/* ------------------------------------------------------------------------------------------------
 * Matcher -- replaces the arithmetic + search cores of USLAM::ORBmatcher (include/ORBmatcher.h:41-88,
 * src/ORBmatcher.cc) and the all-pairs knn-2 matcher of include/utils.h:81-111.
 * ---------------------------------------------------------------------------------------------- */
typedef struct uvo_matcher uvo_matcher;

typedef struct uvo_matcher_cfg {
  int32_t max_query, max_train; /* descriptors per set */
  int32_t max_batch;            /* descriptor-set pairs per batched call */
  int32_t max_map_points;       /* uvo_search_by_projection */
  int32_t device;
} uvo_matcher_cfg;

int uvo_matcher_create(const uvo_matcher_cfg* cfg, uvo_matcher** out);
void uvo_matcher_destroy(uvo_matcher* m);
int uvo_matcher_synchronize(uvo_matcher* m);

/*
 * All-pairs 256-bit Hamming knn-2: Utils::ratioMatching's knnMatch(desc1, desc2, knn=2, mask)
 * (include/utils.h:100-101); distance = ORBmatcher::DescriptorDistance (src/ORBmatcher.cc:1794-1810).
 * mask: nq x nt bytes, non-zero = pair allowed, or NULL.  Ties keep the lower train index.
 * idx = -1, d = 0xFFFF where fewer than one / two train rows are allowed.  Host buffers.
 */
int uvo_hamming_knn2(uvo_matcher* m, const uint8_t* q, int nq, const uint8_t* t, int nt, const uint8_t* mask, int32_t* idx0, uint16_t* d0,
                     int32_t* idx1, uint16_t* d1);
/*
 * Batched, HBM-resident: pair p matches d_q[p*q_stride ...] (d_nq[p] rows) against d_t[p*t_stride ...]
 * (d_nt[p] rows); strides in descriptors; outputs [P][max_query].  Enqueues on the matcher's stream.
 * q_stride <= max_query, t_stride <= 65535 (UVO_E_BADARG otherwise).  The counts are device values (an extractor's
 * d_n_out may exceed the slice it could fill): the kernel clamps d_nq[p] to q_stride and d_nt[p] to t_stride.
 */
int uvo_hamming_knn2_batch_device(uvo_matcher* m, int pairs, const uint8_t* d_q, const int32_t* d_nq, int q_stride, const uint8_t* d_t,
                                  const int32_t* d_nt, int t_stride, int32_t* d_idx0, uint16_t* d_d0, int32_t* d_idx1, uint16_t* d_d1);
/* Full nq x nt distance matrix (uint16), the core of MapPoint::ComputeDistinctiveDescriptors
 * (src/MapPoint.cc:236-247).  Host buffers. */
int uvo_hamming_matrix(uvo_matcher* m, const uint8_t* q, int nq, const uint8_t* t, int nt, uint16_t* dist);

/*
 * MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:197-270) for a batch of map points: desc holds the observed
 * descriptors of all points back to back, point p owns rows offsets[p] .. offsets[p+1]-1 (at most 65535 each).  Per point:
 * best_idx = row (relative to offsets[p]) with the least median Hamming distance to the point's rows, itself included,
 * median = sorted[int(0.5*(N-1))], first index on ties; best_median = that median; -1 / -1 for an empty point.  Host buffers.
 */
int uvo_distinctive_descriptors(uvo_matcher* m, const uint8_t* desc, const int32_t* offsets, int npoints, int32_t* best_idx,
                                int32_t* best_median);

/*
 * ORBmatcher::SearchByProjection(FrameKTL&, const vector<MapPoint*>&, th): src/ORBmatcher.cc:49-125, with the
 * frame grid of src/FrameKTL.cc:250-264,359-436 (64 x 48 cells, PosInGrid uses round()).  Host buffers.
 *   frame : kp[n] (undistorted keypoints: x, y, octave are read), desc[n][32], image bounds min/max x/y
 *   map   : per map point the values FrameKTL::isInFrustum left on it (src/FrameKTL.cc:346-352):
 *           proj_x, proj_y, level (mnTrackScaleLevel), view_cos, in_view (mbTrackInView && !isBad), desc[nmp][32]
 *   assigned[n] : in/out, index of the map point held by keypoint i or -1 (reference: F.mvpMapPoints[i] != NULL)
 *   th, nnratio : call-site values (src/Tracking.cc:2222-2228);  scale_factors[nlevels] = F.mvScaleFactors
 * The greedy, order-dependent assignment of the reference is reproduced exactly.
 * Window: radius (view_cos > 0.998 as a double ? 2.5f : 4.0f), times th when th != 1, times scale_factors[level], in float in that
 * order; levels [level - 1, level]; grid and non-finite input as stated at uvo_match_windows: a key point with a NaN or infinite
 * coordinate is never assigned, a map point whose proj_x, proj_y or radius (a NaN or infinite view_cos gives 4.0f; th and the scale
 * factor enter the radius) is not finite matches nothing.
 */
int uvo_search_by_projection(uvo_matcher* m, const uvo_keypoint* kp, int n, const uint8_t* desc, int min_x, int min_y, int max_x, int max_y,
                             int32_t* assigned, int nmp, const float* proj_x, const float* proj_y, const int32_t* level,
                             const float* view_cos, const uint8_t* in_view, const uint8_t* mp_desc, const float* scale_factors,
                             int nlevels, float th, float nnratio, int* n_matches);

/* ------------------------------------------------------------------------------------------------
 * The other search loops of ORBmatcher.  They all share one shape -- queries visited in a fixed order, a candidate
 * list per query, Hamming distance to every candidate, an acceptance rule, and (except Fuse) targets taken by an
 * earlier query skipped by later ones -- so two generic entry points carry them (candidates from grid windows, or
 * given by the caller), and the reference-named entry points below are thin marshalling layers over those.
 * The order-dependent loops are reproduced exactly (see csrc/match_engine.hip).  Host buffers throughout.
 * ---------------------------------------------------------------------------------------------- */
enum {
  UVO_RULE_BEST_RATIO_SAME_LEVEL = 0, /* SearchByProjection(F, vpMapPoints, th): src/ORBmatcher.cc:96-123 */
  UVO_RULE_BEST_ONLY = 1,             /* SearchByProjection(F, pKF, ...) :1681-1701; Fuse :1084-1119: d <= max_dist */
  UVO_RULE_BEST_RATIO_LE = 2,         /* SearchByBoW(pKF, F, ...) :194-218: d <= max_dist && d < nnratio * second */
  UVO_RULE_BEST_RATIO_LT = 3,         /* SearchByBoW(pKF1, pKF2, ...) :762-788: d < max_dist && d < nnratio * second */
  UVO_RULE_TRIANGULATION = 4,         /* SearchForTriangulation :893-935: d <= max_dist, sorted, d <= 2*best, epipolar */
  /* the members of ORBmatcher that have no caller in the reference */
  UVO_RULE_BEST_RATIO_LEQ = 5,        /* WindowSearch :409-516, SearchByProjection(F1, F2, windowSize) :519-594: d <= nnratio * second
                                         (second = INT_MAX when there is none) && d <= max_dist; both use exclusive = 1 */
  UVO_RULE_INIT_STEAL = 6             /* SearchForInitialization :598-713: candidates whose target is currently matched at <= d are
                                         skipped, d <= max_dist && d < nnratio * second, and a later query with a strictly smaller
                                         distance takes a target over (`exclusive` is ignored); match[i] >= 0 only for queries that
                                         still hold their target at the end; the rotation histogram counts every accept (:662-670) */
};
typedef struct uvo_match_rule {
  int32_t rule;              /* UVO_RULE_* */
  int32_t max_dist;          /* TH_HIGH (100), TH_LOW (50) or the caller's ORBdist */
  float nn_ratio;            /* mfNNratio */
  int32_t exclusive;         /* 1: a target accepted by an earlier query is skipped by later ones (blocked targets are skipped either way) */
  int32_t check_orientation; /* mbCheckOrientation: rotation histogram + ComputeThreeMaxima (:1748-1789) */
} uvo_match_rule;
/* ORBmatcher::CheckDistEpipolarLine (:136-153): l = x1' F12; dsqr = (l . x2)^2 / (a^2+b^2) < 3.84 * sigma2[octave2] */
typedef struct uvo_epipolar {
  float f12[9];         /* row-major 3x3 */
  const float* q_x;     /* query keypoint coordinates (kp1.pt) */
  const float* q_y;
  const float* t_x;     /* target keypoint coordinates (kp2.pt) */
  const float* t_y;
  const float* sigma2;  /* pKF2->GetSigma2(level), nlevels entries */
  int32_t nlevels;
} uvo_epipolar;

/*
 * Candidates from grid windows: FrameKTL::GetFeaturesInArea (src/FrameKTL.cc:359-424) / KeyFrame::GetFeaturesInArea
 * (src/KeyFrame.cc:952-992) over the 64 x 48 grid of the target keypoints kp[n].
 *   blocked[n]  : may be NULL; non-zero = target unavailable from the start (e.g. F.mvpMapPoints[i] != NULL)
 *   query i     : window centre (qx, qy), radius qr, level filter [qmin_level, qmax_level] with the reference's meaning
 *                 (-1,-1 = no filter; equal = that level only), qvalid (0 = query skipped), qdesc, qangle (read only
 *                 when rule->check_orientation; the target angle is kp[].angle)
 *   match[nq]   : target index or -1;  dist[nq] : its distance or -1;  *n_matches : number of matches
 * The list of a query is the reference's, element for element and in its order (ascending cell column, then cell row, then key-point
 * index), held to a brute-force model in tests/test_gpu_windows.py:
 *   grid     : cell = round() -- half away from zero -- of the float product (kp.x - min_x) * (64.0f / (max_x - min_x)), likewise y
 *              with 48; a key point whose cell lies outside 0..63 x 0..47 is in no cell and in no list (the half cell at the right and
 *              bottom edge rounds to 64 / 48; anything below -0.5, and -0.5 itself, rounds to -1 or less)
 *   window   : columns max(0, floor((qx - min_x - qr) * inv_w)) .. min(63, ceil((qx - min_x + qr) * inv_w)), rows likewise; a window
 *              wholly outside the grid is empty; inside it a key point is taken when !(|kp.x - qx| > qr) && !(|kp.y - qy| > qr): a
 *              key point exactly at distance qr is in, qr = 0 finds a key point at the centre itself, a negative qr finds nothing
 *   levels   : (-1, -1) no filter; qmin_level == qmax_level that level only; otherwise the range, so (-1, 0) is level 0 and below and
 *              qmin_level > qmax_level is empty
 *   not finite : a key point with a NaN or infinite x or y is in no cell; a query whose qx, qy or qr is NaN or infinite has an empty
 *              list.  This is the reference's behaviour as built for x86, where such a float converts to INT_MIN (the key point fails
 *              PosInGrid, the query returns at `nMaxCellX < 0`); the device's own conversion -- NaN to 0, infinities saturating --
 *              is not relied on.
 * The comparison holds for finite input whose cell expressions fit an int: |(qx - min_x +- qr) * inv_w| and the y counterpart below
 * 2^31.  Beyond that (a finite radius of about 2^31 cells and more) the reference's answer rests on x86's out-of-range conversion; that
 * case is outside this contract and untested.  Every entry point that builds the grid (this one, uvo_search_by_projection,
 * uvo_search_by_projection_kf, uvo_fuse, uvo_fuse_batch, the Sim3 searches) shares the rule.
 */
int uvo_match_windows(uvo_matcher* m, const uvo_keypoint* kp, int n, const uint8_t* desc, const uint8_t* blocked, int min_x, int min_y,
                      int max_x, int max_y, int nq, const float* qx, const float* qy, const float* qr, const int32_t* qmin_level,
                      const int32_t* qmax_level, const uint8_t* qvalid, const uint8_t* qdesc, const float* qangle, const uvo_match_rule* rule,
                      int32_t* match, int32_t* dist, int* n_matches);
/*
 * Candidates given by the caller: query i owns cand_idx[cand_start[i] .. cand_start[i+1]) (target indices, in the order
 * the reference would visit them).  tlevel / tangle / qangle / tblocked / epi may be NULL when the rule does not read them.
 */
int uvo_match_groups(uvo_matcher* m, int nq, const uint8_t* qdesc, const float* qangle, int nt, const uint8_t* tdesc, const float* tangle,
                     const int32_t* tlevel, const uint8_t* tblocked, const int32_t* cand_start, const int32_t* cand_idx,
                     const uvo_epipolar* epi, const uvo_match_rule* rule, int32_t* match, int32_t* dist, int* n_matches);

/*
 * ORBmatcher::SearchByProjection(FrameKTL& CurrentFrame, KeyFrame* pKF, sAlreadyFound, th, ORBdist): :1622-1746.
 * Per key-frame map point i the caller passes what :1647-1672 computes (uvo_project_points() does it on the device):
 * valid[i] (non-null, !isBad, not already found, projection inside the image), u, v, predicted level; kf_angle[i] =
 * pKF->GetKeyPointUn(i).angle.  Window radius th * scale_factors[level], levels [level-1, level+1], best distance
 * <= orb_dist, first-come exclusivity over the frame keypoints, rotation histogram when check_orientation.
 *   assigned[n] : in/out, index of the map point held by frame keypoint k or -1 (F.mvpMapPoints[k])
 */
int uvo_search_by_projection_kf(uvo_matcher* m, const uvo_keypoint* kp, int n, const uint8_t* desc, int min_x, int min_y, int max_x, int max_y,
                                int32_t* assigned, int nmp, const float* u, const float* v, const int32_t* level, const uint8_t* valid,
                                const uint8_t* mp_desc, const float* kf_angle, const float* scale_factors, int nlevels, float th, int orb_dist,
                                int check_orientation, int* n_matches);

/*
 * A DBoW2::FeatureVector (std::map<NodeId, vector<unsigned>>) in flat form: node ids ascending, features of node j =
 * feat[start[j] .. start[j+1]).
 */
typedef struct uvo_feature_vector {
  const uint32_t* node;
  const int32_t* start;
  const int32_t* feat;
  int32_t n_nodes;
} uvo_feature_vector;

/*
 * ORBmatcher::SearchByBoW(KeyFrame* pKF, FrameKTL& F, vpMapPointMatches) :155-284 (kf_kf = 0) and
 * SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, vpMatches12) :715-850 (kf_kf = 1).
 *   side 1 (queries): n1 keypoints, desc1, angle1, usable1[n1] = pMP1 != NULL && !isBad
 *   side 2 (targets): n2 keypoints, desc2, angle2, usable2[n2] = kf_kf ? (pMP2 != NULL && !isBad) : 1 (NULL = all usable)
 *   match12[n1] : target index or -1 (the reference stores the map point: vpMapPoints...[that index])
 */
int uvo_search_by_bow(uvo_matcher* m, int kf_kf, const uvo_feature_vector* fv1, int n1, const uint8_t* desc1, const float* angle1,
                      const uint8_t* usable1, const uvo_feature_vector* fv2, int n2, const uint8_t* desc2, const float* angle2,
                      const uint8_t* usable2, float nnratio, int check_orientation, int32_t* match12, int* n_matches);

/*
 * ORBmatcher::SearchForTriangulation(pKF1, pKF2, F12, ...) :852-1014.  kp1 / kp2 = undistorted keypoints (x, y, octave,
 * angle are read), has_mp1 / has_mp2 = "keypoint already has a map point", f12 row-major, sigma2 = pKF2 level sigmas.
 *   match12[n1] : index into kp2 or -1 (vMatchedPairs = the pairs with match12[i] >= 0, ascending i)
 */
int uvo_search_for_triangulation(uvo_matcher* m, const uvo_feature_vector* fv1, const uvo_keypoint* kp1, int n1, const uint8_t* desc1,
                                 const uint8_t* has_mp1, const uvo_feature_vector* fv2, const uvo_keypoint* kp2, int n2, const uint8_t* desc2,
                                 const uint8_t* has_mp2, const float* f12, const float* sigma2, int nlevels, int check_orientation,
                                 int32_t* match12, int* n_matches);

/*
 * Search core of ORBmatcher::Fuse(pKF, vpMapPoints, th) :1016-1134 and Fuse(pKF, Scw, ...) :1136-1265: per candidate map
 * point i (valid[i] = passed the projection tests :1037-1076, see uvo_project_points) the best key-frame keypoint in the
 * window of radius th * scale_factors[level] on levels [level-1, level] with distance <= TH_LOW; no exclusivity.
 *   best_idx[nmp] / best_dist[nmp] : keypoint index and distance, or -1.  The map mutation (:1104-1118) stays with the caller.
 */
int uvo_fuse(uvo_matcher* m, const uvo_keypoint* kp, int n, const uint8_t* desc, int min_x, int min_y, int max_x, int max_y, int nmp,
             const float* u, const float* v, const int32_t* level, const uint8_t* valid, const uint8_t* mp_desc, const float* scale_factors,
             int nlevels, float th, int32_t* best_idx, int32_t* best_dist);

/*
 * Projection prologues of the search loops: what the reference computes per map point before it queries the grid.
 *   UVO_PROJECT_FRUSTUM  : FrameKTL::isInFrustum (src/FrameKTL.cc:299-357) + MapPoint::PredictScale (src/MapPoint.cc:373-388)
 *                          -> valid (mbTrackInView), u, v (mTrackProjX/Y), level (mnTrackScaleLevel), view_cos (mTrackViewCos):
 *                          the inputs of uvo_search_by_projection
 *   UVO_PROJECT_KF_RELOC : SearchByProjection(CurrentFrame, pKF, ...) src/ORBmatcher.cc:1647-1670 -> the inputs of
 *                          uvo_search_by_projection_kf (camera centre derived as -Rcw^T tcw like :1628; `ow` is ignored)
 *   UVO_PROJECT_FUSE     : Fuse src/ORBmatcher.cc:1037-1075 -> the inputs of uvo_fuse
 * Arithmetic follows the reference expression by expression (fp32 products, the double intermediates of `1.0/z`,
 * cv::norm and cv::Mat::dot, libm logf); OpenCV's 3x3 * 3x1 product is taken as its small-matrix path (fp32 row sums, the
 * `+ t` in double) -- an unpinned assumption, stated in DESIGN.md.  log(scaleFactor) is the intended constant
 * (the reference reads it before it is initialised).
 *   usable[i]      : 0 = skip (NULL / isBad / already found / already in the key frame ...), may be NULL
 *   min_distance_inv / max_distance_inv : GetMinDistanceInvariance() / GetMaxDistanceInvariance() of every point
 *                    (max_distance_inv is not read by KF_RELOC; the PIXEL modes read neither and accept NULL); max_distance: the raw mfMaxDistance member that
 *                    MapPoint::PredictScale divides by (FRUSTUM only); normal: GetNormal(), modes FRUSTUM and FUSE
 */
enum {
  UVO_PROJECT_FRUSTUM = 0,
  UVO_PROJECT_KF_RELOC = 1,
  UVO_PROJECT_FUSE = 2,
  /* the two caller-less projection searches: u, v only; the caller supplies the level (the keypoint's octave) */
  UVO_PROJECT_PIXEL_BOUNDED = 3, /* SearchByProjection(CurrentFrame, LastFrame, th) :1530-1545: valid = inside [min_x, max_x] x [min_y, max_y] */
  UVO_PROJECT_PIXEL = 4          /* SearchByProjection(F1, F2, windowSize) :541-550: no test (not even the depth's sign) */
};
typedef struct uvo_camera_pose {
  float rcw[9]; /* row-major world -> camera rotation */
  float tcw[3];
  float ow[3];  /* camera centre in the world (mOw / GetCameraCenter()) */
  float fx, fy, cx, cy;
  float min_x, max_x, min_y, max_y; /* mnMinX, mnMaxX, mnMinY, mnMaxY */
} uvo_camera_pose;
int uvo_project_points(uvo_matcher* m, int mode, const uvo_camera_pose* cam, int npts, const float* xyz, const float* normal,
                       const float* min_distance_inv, const float* max_distance_inv, const float* max_distance, const uint8_t* usable,
                       const float* scale_factors, int nlevels, float scale_factor, float viewing_cos_limit, uint8_t* valid, float* u, float* v,
                       int32_t* level, float* view_cos);

/*
 * Batched forms of the two matcher loops of the LocalMapping thread: one device round trip for the whole loop, results identical to
 * the single calls made one after the other.
 *
 * LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:1058-1180) calls SearchForTriangulation(mpCurrentKeyFrame, pKF2, F12, ...) for
 * up to 20 neighbour key frames; between two calls it triangulates the pair's matches and the accepted ones get map points
 * (mpCurrentKeyFrame->AddMapPoint, :1177), which removes those features from the later pairs (`if(pMP1) continue;`,
 * src/ORBmatcher.cc:885-889).  uvo_search_for_triangulation_batch() computes the descriptor distances and the epipolar test of EVERY
 * pair in one launch (one upload, one host wait) for the features of key frame 1 that have no map point yet, and keeps the candidate
 * lists in the handle; uvo_search_for_triangulation_next(pair, has_mp1 as it is NOW, ...) replays the reference's acceptance loop
 * (:886-984: candidates still free, distance <= TH_LOW, sorted, walk to round(2 * best), first one on the epipolar line; rotation
 * histogram) for that pair on the host -- no device work.  Pairs may be replayed in any order and more than once; the caller passes
 * the has_mp1 the reference would see at that point (a feature may only GAIN a map point while a batch is alive: UVO_E_BADARG if one
 * lost it).  A new batch replaces the old one.
 */
typedef struct uvo_triangulation_pair {
  const uvo_feature_vector* fv2; /* pKF2->GetFeatureVector() */
  const uvo_keypoint* kp2;       /* pKF2->GetKeyPointsUn() */
  int32_t n2;
  const uint8_t* desc2;          /* [n2][32] */
  const uint8_t* has_mp2;        /* [n2] pKF2->GetMapPointMatches()[k] != NULL */
  float f12[9];                  /* row-major */
  const float* sigma2;           /* [nlevels] pKF2->GetSigma2(level) */
  int32_t nlevels;
} uvo_triangulation_pair;
int uvo_search_for_triangulation_batch(uvo_matcher* m, const uvo_feature_vector* fv1, const uvo_keypoint* kp1, int n1, const uint8_t* desc1,
                                       const uint8_t* has_mp1, int n_pairs, const uvo_triangulation_pair* pairs);
int uvo_search_for_triangulation_next(uvo_matcher* m, int pair, const uint8_t* has_mp1_now, int check_orientation, int32_t* match12,
                                      int* n_matches);
/*
 * The second half of LocalMapping::CreateNewMapPoints: the triangulation of a pair's matches (src/LocalMapping.cc:1096-1180; the same
 * linear method as Initializer::Triangulate, src/Initializer.cc:726-745) -- parallax between the rays, 4 x 4 linear triangulation by
 * SVD, depth signs, the two reprojection tests, scale consistency -- one device lane per match, in the reference's operation order
 * and types (fp32, double where the reference's expression is double).  Verdicts name the `continue` a match left the loop body at.
 */
enum {
  UVO_TRI_ACCEPTED = 0,  /* :1182 "Triangulation is succesfull" */
  UVO_TRI_PARALLAX = 1,  /* :1112 cosParallaxRays < 0 || cosParallaxRays > 0.9998 */
  UVO_TRI_W_ZERO = 2,    /* :1127 homogeneous coordinate == 0 */
  UVO_TRI_BEHIND_1 = 3,  /* :1136 z1 <= 0 */
  UVO_TRI_BEHIND_2 = 4,  /* :1140 z2 <= 0 */
  UVO_TRI_REPROJ_1 = 5,  /* :1152 reprojection error in key frame 1 > 5.991 sigma2 */
  UVO_TRI_REPROJ_2 = 6,  /* :1164 reprojection error in key frame 2 */
  UVO_TRI_ZERO_DIST = 7, /* :1174 dist1 == 0 || dist2 == 0 */
  UVO_TRI_SCALE = 8      /* :1179 distance ratio against the octave ratio */
};
typedef struct uvo_triangulation_camera {
  float rcw[9];               /* GetRotation(), row-major */
  float tcw[3];               /* GetTranslation() */
  float ow[3];                /* GetCameraCenter(): passed in, not derived, so that it is the key frame's own Ow bit for bit */
  float fx, fy, cx, cy;
  const float* scale_factors; /* [nlevels] GetScaleFactor(level) */
  const float* sigma2;        /* [nlevels] GetSigma2(level) */
  int32_t nlevels;            /* 1 .. 64; every key point's octave must lie inside */
} uvo_triangulation_camera;
/*
 * The core alone, for a caller-given list of n matched undistorted key points (kp1[j] in key frame 1 <-> kp2[j] in key frame 2; x, y,
 * octave are read).  ratio_factor = 1.5f * mpCurrentKeyFrame->GetScaleFactor() (:1055).  Host buffers.
 *   verdict[n] : UVO_TRI_*;  x3d[n][3] : the point wherever the verdict is ACCEPTED or >= BEHIND_1 (it exists from :1131 on), zeros else
 * Tolerance contract: the fp32 SVD is OpenCV 3.4's one-sided Jacobi restated, not OpenCV's binary; x3d agrees
 * with a float64 evaluation within a stated relative bound and verdicts are exact except where a test lies within a stated margin of
 * its threshold.
 */
int uvo_triangulate_matches(uvo_matcher* m, const uvo_triangulation_camera* cam1, const uvo_triangulation_camera* cam2, float ratio_factor,
                            const uvo_keypoint* kp1, const uvo_keypoint* kp2, int n, int32_t* verdict, float* x3d);
/*
 * The whole loop of src/LocalMapping.cc:1058-1199 in one call: the arguments of uvo_search_for_triangulation_batch, plus the cameras.
 * For each pair, in order, on the device: the acceptance loop of SearchForTriangulation (src/ORBmatcher.cc:886-984) with key frame 1's
 * map points as they are BY THEN, the triangulation of that pair's matches, and has_mp1 = 1 for the accepted ones -- so pair k + 1
 * sees the map points pair k created, with no host visit in between: one upload, one launch chain, one host wait.  The short-baseline
 * skip (:1066-1072) and ComputeF12 stay with the caller (skipped pairs are left out; f12 travels in uvo_triangulation_pair); the map
 * mutation (new MapPoint, AddObservation, ...) stays on the host, done after the call in the order of the output, the reference's order.
 *   cams2[n_pairs]           : camera of key frame 2 of every pair; cam1 / ratio_factor as in uvo_triangulate_matches
 * Outputs, every array [n_pairs][n1] (pair p's entries start at element p * n1; a pair has at most n1 matches):
 *   n_matches[n_pairs]       : matches of pair p = vMatchedIndices.size() at that point of the reference's loop
 *   n_accepted[n_pairs]      : how many of them were accepted
 *   idx1, idx2               : the matches, ascending idx1 -- exactly vMatchedIndices
 *   verdict, x3d ([..][3])   : per match, as uvo_triangulate_matches
 *   has_mp1_out[n1]          : has_mp1 after the loop (may be NULL)
 * A batch that uvo_search_for_triangulation_batch left in the handle is not touched (it lives on the host).
 */
typedef struct uvo_new_map_points {
  int32_t* n_matches;
  int32_t* n_accepted;
  int32_t* idx1;
  int32_t* idx2;
  int32_t* verdict;
  float* x3d;
  uint8_t* has_mp1_out;
} uvo_new_map_points;
int uvo_create_new_map_points(uvo_matcher* m, const uvo_feature_vector* fv1, const uvo_keypoint* kp1, int n1, const uint8_t* desc1,
                              const uint8_t* has_mp1, int n_pairs, const uvo_triangulation_pair* pairs, const uvo_triangulation_camera* cam1,
                              const uvo_triangulation_camera* cams2, float ratio_factor, int check_orientation, const uvo_new_map_points* out);
/*
 * LocalMapping::SearchInNeighbors (src/LocalMapping.cc:1228-1236) calls Fuse(pKFi, vpMapPointMatches) for every target key frame.  The
 * search core of Fuse has no exclusivity among the map points, so the projection tests (:1037-1075, with each target's own pose) and the
 * best key point (:1077-1101) of EVERY (target, map point) are computed in one pass: the map points are uploaded once, each target adds
 * its grid + projection + window walk to the stream, one download, one host wait.
 *   usable[nmp]            : 0 = the point is NULL (never searched); NULL = all usable.  The tests that depend on the map as the loop
 *                            mutates it -- isBad(), IsInKeyFrame(pKFi), :1031-1035 -- stay with the caller, who discards the results of
 *                            points that fail them when target i's turn comes (the search of a point depends on nothing else).
 *   best_idx / best_dist   : [n_targets][nmp] key point of target t and distance, or -1 (as uvo_fuse).
 * One thing the caller must watch: pMP->Replace(pMPinKF) (:1107) recomputes pMPinKF's descriptor; if pMPinKF is itself one of the nmp
 * points, its rows of the LATER targets were computed with the old descriptor and must be redone (uvo_project_points + uvo_fuse for
 * that point).  include/uvo/compat/ORBmatcher.h FuseTargets() does exactly that.
 */
typedef struct uvo_fuse_target {
  const uvo_keypoint* kp; /* pKF->GetKeyPointUn(k) for all k */
  int32_t n;
  const uint8_t* desc;    /* [n][32] */
  int32_t min_x, min_y, max_x, max_y; /* mnMinX .. mnMaxY */
  uvo_camera_pose cam;    /* pose, intrinsics and image bounds of the target */
  const float* scale_factors;
  int32_t nlevels;
} uvo_fuse_target;
int uvo_fuse_batch(uvo_matcher* m, int n_targets, const uvo_fuse_target* targets, int nmp, const float* xyz, const float* normal,
                   const float* min_distance_inv, const float* max_distance_inv, const uint8_t* usable, const uint8_t* mp_desc, float th,
                   int32_t* best_idx, int32_t* best_dist);


/*
 * Tracking::SearchReferencePointsInFrustum (src/Tracking.cc:2176-2230) as one call: FrameKTL::isInFrustum(pMP, viewing_cos_limit) on
 * every local map point (UVO_PROJECT_FRUSTUM above), then SearchByProjection(mCurrentFrame, mvpLocalMapPoints, th) (:49-125) on the
 * points in view -- same results as uvo_project_points followed by uvo_search_by_projection, but the inputs travel as one block,
 * the projections stay on the device and the host waits once.  Frame side: kp / desc / assigned as in uvo_search_by_projection; the
 * grid bounds are cam->min_x .. max_y.  Map side: as in uvo_project_points, plus the representative descriptors mp_desc[npts][32].
 *   usable[i]  : 0 for points the caller's loop skips (:2207-2210: seen in this frame already, or bad); NULL = all usable
 *   in_view, proj_x, proj_y, level, view_cos : optional outputs = mbTrackInView, mTrackProjX/Y, mnTrackScaleLevel, mTrackViewCos
 *   *n_to_match = number of points in view (nToMatch; the reference skips the search when it is 0 -- so does this call, in effect)
 */
int uvo_search_points_in_frustum(uvo_matcher* m, const uvo_keypoint* kp, int n, const uint8_t* desc, int32_t* assigned, const uvo_camera_pose* cam,
                                 int npts, const float* xyz, const float* normal, const float* min_distance_inv, const float* max_distance_inv,
                                 const float* max_distance, const uint8_t* usable, const uint8_t* mp_desc, const float* scale_factors, int nlevels,
                                 float scale_factor, float viewing_cos_limit, float th, float nnratio, uint8_t* in_view, float* proj_x,
                                 float* proj_y, int32_t* level, float* view_cos, int* n_to_match, int* n_matches);

/*
 * Loop-closing (Sim3) forms of the search loops.
 *
 * uvo_sim3_decompose: the head of SearchByProjection(pKF, Scw, ...) src/ORBmatcher.cc:299-303 and Fuse(pKF, Scw, ...) :1145-1149:
 *   scw = |row 0 of sR|, Rcw = sR / scw, tcw = s t / scw, Ow = -Rcw^T tcw, written to cam->rcw / tcw / ow (the other members are
 *   left alone).  scw_mat: 3 rows of row_stride floats (a 4x4 or 3x4 row-major Scw).  Host arithmetic, evaluated the way OpenCV
 *   evaluates those cv::Mat expressions (double dot product, multiplication by the float reciprocal, double-accumulating gemm).
 *   With the result, uvo_project_points(UVO_PROJECT_FUSE) is the per-point prologue of both members (:315-361 / :1161-1207 are
 *   the same tests as :1037-1075).
 * uvo_sim3_relative: SearchBySim3 :1284-1287: s_r12 = s12 R12, s_r21 = (1/s12) R12^T, t21 = -s_r21 t12 (3x3 row-major, 3-vectors).
 * uvo_project_sim3: the per-point prologue of either direction of SearchBySim3 (:1323-1359 / :1403-1441): world -> the owning
 *   key frame's camera (r_own, t_own) -> the other camera (s_r, t) -> pixel (cam_other: fx, fy, cx, cy and the image bounds are
 *   read), positive depth, KeyFrame::IsInImage, distance inside [min_distance_inv, max_distance_inv], level by lower_bound over
 *   scale_factors.  usable[i] = point exists, not already matched, not bad (may be NULL).
 * uvo_search_by_projection_sim3: :357-398 on the projected candidates: best unmatched key point within th * scale_factors[level]
 *   on levels [level-1, level], accepted at <= TH_LOW, first come first served in candidate order.
 *   matched[n]: in: >= 0 where vpMatched[idx] is set; out: newly matched key points hold the candidate's index.
 * uvo_search_by_sim3: :1361-1504: both directions (best key point of the other frame on levels [level-1, level], <= TH_HIGH,
 *   no exclusivity) and the agreement check.  *12 arrays have n1 entries (KF1's map points, projected into KF2, with their
 *   representative descriptors mp_desc1), *21 arrays n2 entries.  bounds = {mnMinX, mnMinY, mnMaxX, mnMaxY} of each key frame.
 *   match12[n1]: index into KF2 or -1.
 */
int uvo_sim3_decompose(const float* scw_mat, int row_stride, uvo_camera_pose* cam);
int uvo_sim3_relative(float s12, const float* r12, const float* t12, float* s_r12, float* s_r21, float* t21);
int uvo_project_sim3(uvo_matcher* m, const float* r_own, const float* t_own, const float* s_r, const float* t, const uvo_camera_pose* cam_other,
                     int npts, const float* xyz, const float* min_distance_inv, const float* max_distance_inv, const uint8_t* usable,
                     const float* scale_factors, int nlevels, uint8_t* valid, float* u, float* v, int32_t* level);
int uvo_search_by_projection_sim3(uvo_matcher* m, const uvo_keypoint* kp, int n, const uint8_t* desc, int min_x, int min_y, int max_x, int max_y,
                                  int32_t* matched, int nmp, const float* u, const float* v, const int32_t* level, const uint8_t* valid,
                                  const uint8_t* mp_desc, const float* scale_factors, int nlevels, int th, int* n_matches);
int uvo_search_by_sim3(uvo_matcher* m, const uvo_keypoint* kp1, int n1, const uint8_t* desc1, const int32_t* bounds1, const uvo_keypoint* kp2,
                       int n2, const uint8_t* desc2, const int32_t* bounds2, const float* u12, const float* v12, const int32_t* level12,
                       const uint8_t* valid12, const uint8_t* mp_desc1, const float* u21, const float* v21, const int32_t* level21,
                       const uint8_t* valid21, const uint8_t* mp_desc2, const float* scale_factors1, int nlevels1, const float* scale_factors2,
                       int nlevels2, float th, int32_t* match12, int* n_found);

/* ------------------------------------------------------------------------------------------------
 * Bag-of-words transform: DBoW2::TemplatedVocabulary<FORB::TDescriptor, FORB>::transform(features, BowVector&, FeatureVector&,
 * levelsup) (Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1125-1188, per-feature descent :1207-1258), as called by
 * FrameKTL::ComputeBoW (src/FrameKTL.cc:439-446) and KeyFrame::ComputeBoW (src/KeyFrame.cc:203-210) with levelsup = 4.
 * The tree descent (Hamming distance to every child, first minimum wins) runs on the device; the two std::map containers are
 * assembled on the host in the reference's insertion order.  The feature vector comes out in the flat form
 * uvo_search_by_bow / uvo_search_for_triangulation take.
 * ---------------------------------------------------------------------------------------------- */
typedef struct uvo_vocabulary uvo_vocabulary;
typedef struct uvo_vocabulary_desc {
  int32_t n_nodes;            /* m_nodes.size(); node 0 is the root */
  const int32_t* child_start; /* [n_nodes + 1]: children of node i = children[child_start[i] .. child_start[i+1]), in m_nodes[i].children order */
  const int32_t* children;    /* ids in 1..n_nodes-1, each at most once: a tree, as every DBoW2 vocabulary is.  A description that lists a
                                 node twice (its own descendant, or under two parents) is refused with UVO_E_BADARG: the root is never a
                                 child, so a descent from it cannot re-enter a node and always ends */
  const uint8_t* descriptor;  /* [n_nodes][32]: m_nodes[i].descriptor (row 0 unused) */
  const int32_t* word_id;     /* [n_nodes]: m_nodes[i].word_id (read for leaves) */
  const double* weight;       /* [n_nodes]: m_nodes[i].weight */
  int32_t L;                  /* m_L */
  int32_t weighting;          /* DBoW2::WeightingType: 0 TF_IDF, 1 TF, 2 IDF, 3 BINARY */
  int32_t normalize;          /* GeneralScoring::mustNormalize: 0 = no (DotProduct), 1 = L1, 2 = L2 */
  int32_t device;
} uvo_vocabulary_desc;
int uvo_vocabulary_create(const uvo_vocabulary_desc* desc, uvo_vocabulary** out);
void uvo_vocabulary_destroy(uvo_vocabulary* voc);
/*
 * desc[n][32] -> per feature: word_id, word_weight, node_id (node reached at level L - levelsup; 0 when that level is <= 0;
 * the leaf itself when the descent ends above that level -- the reference leaves it uninitialised there);
 * BowVector as (bow_id ascending, bow_value), *n_bow entries; FeatureVector as fv_node ascending, fv_start[*n_fv + 1],
 * fv_feat (feature indices, ascending inside a node).  Per-feature arrays may be NULL.  Host buffers.
 */
int uvo_bow_transform(uvo_vocabulary* voc, const uint8_t* desc, int n, int levelsup, int32_t* word_id, double* word_weight, int32_t* node_id,
                      uint32_t* bow_id, double* bow_value, int bow_cap, int* n_bow, uint32_t* fv_node, int32_t* fv_start, int32_t* fv_feat,
                      int fv_cap, int* n_fv);

/*
 * haloc::Hash::getHash (src/hash.cpp:57-85; KeyFrame::ComputeHaloc src/KeyFrame.cc:318-329): for every projection vector r_i and
 * descriptor column c, hash[i*32 + c] = (sum over rows m of r_i[m] * (float)desc[m][c]) / (float)n, accumulated in fp32 in row
 * order (one thread per output walks the rows, so the rounding sequence is the reference's).  proj: [num_proj][proj_stride]
 * floats (the reference builds them from time(NULL), so they are an input here), proj_stride >= n.  Host buffers.
 */
int uvo_haloc_hash(uvo_matcher* m, const float* proj, int num_proj, int proj_stride, const uint8_t* desc, int n, float* hash);

/*
 * Device-side ordering between the two handles' streams (no host synchronisation): work enqueued on the
 * matcher after uvo_matcher_wait_extractor() starts only when everything enqueued on the extractor so far
 * has finished, and vice versa.  Used when descriptors produced by uvo_extract_batch_device() feed
 * uvo_hamming_knn2_batch_device() directly in HBM.
 */
int uvo_matcher_wait_extractor(uvo_matcher* m, uvo_extractor* h);
int uvo_extractor_wait_matcher(uvo_extractor* h, uvo_matcher* m);
/*
 * The cheaper form of the same ordering: from this call on the matcher enqueues its work in the stream of the extractor's current
 * pipeline lane (the lane of the most recent batch call), directly behind that batch's kernels and in front of whatever the lane
 * runs next -- no events, no hand-off between queues (each costs tens of microseconds; a lane of the batch-256 pipeline idled
 * 0.3 ms per batch on the two hand-offs around uvo_hamming_knn2_batch_device).  One call is enough: the extractor keeps a list of the
 * matchers attached to it and moves them along whenever a batch goes to another pipeline lane, so the matcher always works behind the
 * most recent batch (calling it again after a batch is harmless).  h = NULL: back to the matcher's own stream.  While attached, calls
 * that wait for the matcher's stream (every host-buffer entry point) wait for that lane.  Either handle may be destroyed first: a
 * destroyed extractor hands its matchers back to their own streams, a destroyed matcher leaves the list.
 * ORDERING CONTRACT: an attached matcher is ordered behind the MOST RECENT batch only.  With pipeline depth >= 2, work that reads the
 * results of batch N must be enqueued before batch N + 1 is (extract N, match N, extract N + 1, match N + 1 ...); a caller that
 * enqueues two batches and then matches the first must order that match itself (uvo_matcher_wait_extractor before batch N + 1, or
 * uvo_extractor_synchronize).  The handles are not thread-safe against each other: attach / detach / destroy and the batch calls of
 * one extractor + its matchers belong to one host thread at a time (the follower list itself is locked).
 */
int uvo_matcher_attach_extractor(uvo_matcher* m, uvo_extractor* h);
/* per-kernel timing of the matcher, same contract as uvo_extractor_profile / uvo_extractor_kernel_times */
int uvo_matcher_profile(uvo_matcher* m, int enable);
int uvo_matcher_kernel_times(uvo_matcher* m, char* names, int names_cap, float* ms, int32_t* launches, int cap, int* n);

/* ------------------------------------------------------------------------------------------------
 * KLT step in front of the extractor: cv::buildOpticalFlowPyramid (src/FrameKTL.cc:76) and cv::calcOpticalFlowPyrLK with
 * OPTFLOW_USE_INITIAL_FLOW + OPTFLOW_LK_GET_MIN_EIGENVALS (src/Tracking.cc:1046-1047).  Pyramids (image levels with a
 * winSize REFLECT_101 border + Scharr derivatives) stay on the device in numbered slots, so a frame's pyramid is built once
 * and tracked against twice (as previous, then as next).  Integer stages are exact; the tracker's float sums are reduced
 * across a wavefront, i.e. associated differently from a raster-order CPU loop (positions agree to float rounding).
 * ---------------------------------------------------------------------------------------------- */
typedef struct uvo_klt uvo_klt;
typedef struct uvo_klt_cfg {
  int32_t max_width, max_height;
  int32_t max_level;              /* mPyr_Levels: levels 0..max_level (fewer when a level would not exceed the window) */
  int32_t win_width, win_height;  /* mWin_Size, e.g. 21 x 21; at most 1024 pixels */
  int32_t max_points;
  int32_t slots;                  /* pyramids kept on the device (>= 2) */
  int32_t device;
} uvo_klt_cfg;
int uvo_klt_create(const uvo_klt_cfg* cfg, uvo_klt** out);
void uvo_klt_destroy(uvo_klt* k);
int uvo_klt_build_pyramid(uvo_klt* k, int slot, const uint8_t* img, int width, int height, ptrdiff_t stride, int* levels_built);
/* HBM-resident chain: the image is the result of the extractor handle's last uvo_clahe() call (see there), no upload */
int uvo_klt_build_pyramid_from_extractor(uvo_klt* k, int slot, uvo_extractor* h, int* levels_built);
/* test tap: level without its border; img [h][w] u8, deriv [h][w][2] int16 (either may be NULL) */
int uvo_klt_read_level(uvo_klt* k, int slot, int level, uint8_t* img, int16_t* deriv, int* width, int* height);
/* prev_pts / next_pts: n x (x, y) float32; next_pts in = initial flow, out = tracked positions; status[n], err[n] (min eigenvalue).
 * max_count / epsilon: the TermCriteria (30, 0.01 at the call site); min_eig_threshold: 1e-4 (OpenCV default). */
int uvo_klt_track(uvo_klt* k, int prev_slot, int next_slot, const float* prev_pts, float* next_pts, int n, int max_level, int max_count,
                  double epsilon, double min_eig_threshold, uint8_t* status, float* err);
/*
 * Tracking::undistort_point (src/Tracking.cc:1265-1283), the step between the tracker and RANSAC (:1049-1053): for the pin-hole model
 * cv::undistortPoints(pt, pt, mK, mDistCoef, cv::Mat(), mK), for Fisheye_Cam cv::fisheye::undistortPoints(pt, pt, mK, mDistCoef,
 * cv::Mat(), mK).  dist: k1 k2 p1 p2 [k3 [k4 k5 k6]] (n_dist 0..8) resp. the four fisheye coefficients (n_dist <= 4).  Double
 * arithmetic like OpenCV's; results are float pixel coordinates.
 *   uvo_undistort_points      : n points, host in / host out (n <= 2 * max_points of the handle)
 *   uvo_klt_track_undistorted : uvo_klt_track + the undistortion of both point sets (prev_un, next_un: n x 2 floats) on the device --
 *                               the loop of :1049-1053 as part of the same call, one upload and one download
 */
typedef struct uvo_camera_model {
  float fx, fy, cx, cy; /* mK (CV_32F) */
  float dist[8];        /* mDistCoef */
  int32_t n_dist;
  int32_t fisheye;      /* Fisheye_Cam */
} uvo_camera_model;
int uvo_undistort_points(uvo_klt* k, const uvo_camera_model* cam, const float* pts, int n, float* out);
int uvo_klt_track_undistorted(uvo_klt* k, int prev_slot, int next_slot, const float* prev_pts, float* next_pts, int n, int max_level, int max_count,
                              double epsilon, double min_eig_threshold, const uvo_camera_model* cam, uint8_t* status, float* err, float* prev_un,
                              float* next_un);
/*
 * cv::findFundamentalMat(pts0_Un, pts1_Un, cv::FM_RANSAC, thr, conf, mask_rsc) (src/Tracking.cc:1062, thr 1, conf 0.999) on the device, in
 * the handle's stream, scratch sized at uvo_klt_create (n <= max_points; nothing allocated per call).  OpenCV 3.4's semantics, recalled
 * [OCV-RECALL, listed in tests/fundamental_model.py]: thr <= 0 -> 3 and conf outside (DBL_EPSILON, 1 - DBL_EPSILON) -> 0.99 (NaN in
 * either: UVO_E_BADARG); n < 7 no model; n == 7 the 7-point kernel once, mask all 1; 8..14 points LMedS; from 15 points RANSAC
 * (cv::RNG seeded with (uint64)-1, at most 1000 hypotheses).  Host buffers p0, p1: n x (x, y) float32.
 *   mask : n bytes, always written -- all 0 where OpenCV leaves the mask empty
 *   F    : 9 doubles, row-major (may be NULL): the model OpenCV returns (the first of the n == 7 kernel's), zeros where it returns none
 *   info : may be NULL
 * Tolerance contract: RNG stream, subsets, inlier counts, the chosen model, the iteration count and the mask are
 * exact, F agrees within 1e-6 (the null-space basis differs from OpenCV's SVD), with two stated exceptions.
 */
#define UVO_FM_NONE 0
#define UVO_FM_SEVEN_POINT 1
#define UVO_FM_RANSAC 2
#define UVO_FM_LMEDS 3
typedef struct uvo_fm_info {
  int32_t method;      /* UVO_FM_* */
  int32_t iterations;  /* OpenCV's iter at loop exit (0 for n <= 7) */
  int32_t inliers;     /* mask bytes set */
  uint32_t rng_draws;  /* cv::RNG::next() calls consumed */
} uvo_fm_info;
int uvo_klt_find_fundamental(uvo_klt* k, const float* p0, const float* p1, int n, double thr, double conf, uint8_t* mask, double* F,
                             uvo_fm_info* info);
/* Tracking::perform_matching from :1037 on in one call, one upload and one download: n < 10 -> mask_out all 0, F zeros, nothing else is
 * touched and the tracker does not run; otherwise uvo_klt_track_undistorted, then findFundamentalMat on all n undistorted pairs (lost
 * points included, wherever the tracker left them) and mask_out[i] = status[i] && inlier[i].  F may be NULL. */
int uvo_klt_track_filtered(uvo_klt* k, int prev_slot, int next_slot, const float* prev_pts, float* next_pts, int n, int max_level, int max_count,
                           double epsilon, double min_eig_threshold, const uvo_camera_model* cam, uint8_t* status, float* err, float* prev_un,
                           float* next_un, double thr, double conf, uint8_t* mask_out, double* F);
/* test tap: the hypotheses of the handle's last findFundamentalMat call, in draw order, up to its iterations: subsets [cap][7] point
 * indices, n_models [cap] (<= 0: the 7-point kernel gave none), scores [cap][3] (inlier counts, or LMedS medians; -1 where no model).
 * *n = hypotheses written. */
int uvo_klt_fm_hypotheses(uvo_klt* k, int32_t* subsets, int32_t* n_models, double* scores, int cap, int* n);
/*
 * cv::solvePnPRansac(mappts, pts, mK, mDistCoef, Rvec, Tvec, false, iterations, reproj_err, conf, mask_pnp, cv::SOLVEPNP_EPNP) of
 * Tracking::TrackWithPnP (src/Tracking.cc:1864: 300, 3, 0.99) on the device, in the handle's stream, scratch sized at uvo_klt_create
 * (n <= max_points, iterations 1..1000; nothing allocated per call; one upload, one download).  OpenCV 3.4's semantics, recalled
 * [OCV-RECALL, items 1-7 of tests/pnp_model.py]: 5 points per hypothesis drawn from cv::RNG seeded with (uint64)-1, only repeated
 * indices redrawn; EPnP on the float-stored undistorted points; projectPoints + float error against reproj_err^2; a hypothesis is
 * taken iff its count exceeds max(best, 4); EPnP once more on the winner's inliers in double; n == 5 solves once on all points.
 *   obj, img : n x (X, Y, Z) and n x (u, v) float32 (Point3f / Point2f layout)
 *   cam      : fisheye must be 0 (UVO_E_BADARG otherwise): solvePnPRansac applies the pin-hole model to mDistCoef whatever Fisheye_Cam
 *              says, and so does this call
 *   rvec, tvec : 3 doubles each; Tcw (may be NULL): the float 4 x 4 [R t; 0 1] that :1874-1878 builds, row-major
 *   inliers  : room for n indices; info->inliers of them are written, ascending: the RANSAC winner's, not re-evaluated after the refit
 *   info     : may be NULL.  ok = 0 (and zeros everywhere, no inliers) when n <= 4 (the else branch at :1866; the GPU is not touched),
 *              when no hypothesis reaches 5 inliers or when a pose is not finite; NaN reproj_err or conf: UVO_E_BADARG
 * Contract: the random stream, the scoring of a given pose, the replay of given counts and the inlier list are
 * exact; the returned pose agrees with a correct EPnP on the returned inliers to the refit tolerance (from 6 inliers on) PROVIDED it
 * orients the control-point axes the same way (largest component positive: a convention of this library, item 8 of the model's list,
 * UNPINNED -- OpenCV's signs come out of its 3 x 3 SVD, and one flipped axis moves a noisy pose by 1e-4 .. 1e-2).  The pose
 * of a single 5-point hypothesis is NOT part of the contract and cannot be: EPnP's system then has a two-dimensional null space whose
 * basis is rounding noise of the eigen-solver, and the pose depends on it.  Such poses are held bit for bit to a host build of the same
 * source (csrc/epnp_core.hpp) instead.
 */
typedef struct uvo_pnp_info {
  int32_t ok;          /* a pose was found */
  int32_t iterations;  /* OpenCV's iter at loop exit (0 for n == 5) */
  int32_t inliers;     /* indices written */
  uint32_t rng_draws;  /* cv::RNG::next() calls consumed */
} uvo_pnp_info;
int uvo_klt_solve_pnp_ransac(uvo_klt* k, const float* obj, const float* img, int n, const uvo_camera_model* cam, int iterations, double reproj_err,
                             double conf, double* rvec, double* tvec, float* Tcw, int32_t* inliers, uvo_pnp_info* info);
/* test tap: the hypotheses of the handle's last solve_pnp_ransac call, in draw order, up to its iterations: subsets [cap][5] point
 * indices, poses [cap][12] (R row-major, t; zeros where EPnP gave no finite pose), counts [cap] (inliers; -1 where there is no pose).
 * *n = hypotheses written. */
int uvo_klt_pnp_hypotheses(uvo_klt* k, int32_t* subsets, double* poses, int32_t* counts, int cap, int* n);

/* ------------------------------------------------------------------------------------------------
 * PnPsolver -- replaces USLAM::PnPsolver (include/PnPsolver.h, src/PnPsolver.cc) as Tracking::Relocalisation uses it
 * (src/Tracking.cc:2415-2441): one solver per candidate key frame, SetRansacParameters(0.99,10,300,4,0.5,5.991), then iterate(5,...)
 * over the candidates in turn until one returns a pose.  Here the solvers live in a set, and ONE call iterates a list of them.
 * ---------------------------------------------------------------------------------------------- */
/*
 * The reference draws its minimal sets with DUtils::Random::RandomInt, which is libc's rand(), and nothing ever seeds it: the process
 * runs on srand(1).  The library evaluates hypotheses ahead of the loop it replays and must not consume draws the reference would not,
 * so it never calls rand(): the caller owns this state and passes it to every iterate call.  Equal to glibc's srand / rand for seeds
 * in [0, 2^31) (seed 0 behaves as seed 1, as in glibc); larger seeds are outside the contract.
 */
typedef struct uvo_glibc_rand {
  int32_t r[34]; /* the last 34 words of the additive feedback sequence, as a ring */
  int32_t k;     /* ring position of the next output */
} uvo_glibc_rand;
void uvo_glibc_srand(uvo_glibc_rand* g, uint32_t seed);
int32_t uvo_glibc_rand_next(uvo_glibc_rand* g); /* rand(): 0 .. 2^31 - 1 */

typedef struct uvo_pnpsolver_set uvo_pnpsolver_set;
/* SetRansacParameters(probability, minInliers, maxIterations, minSet, epsilon, th2), src/PnPsolver.cc:122 */
typedef struct uvo_pnpsolver_params {
  double probability;
  int32_t min_inliers, max_iterations, min_set; /* min_set 4..8 */
  float epsilon, th2;
} uvo_pnpsolver_params;
/* what SetRansacParameters derives, and the solver's persistent counters */
typedef struct uvo_pnpsolver_info {
  int32_t n;            /* N: correspondences */
  int32_t min_inliers;  /* mRansacMinInliers after the adjustment */
  int32_t max_its;      /* mRansacMaxIts after the adjustment */
  int32_t iterations;   /* mnIterations */
  int32_t best_inliers; /* mnBestInliers */
} uvo_pnpsolver_info;
typedef struct uvo_pnpsolver_status {
  int32_t touched;    /* iterate() was called on this solver (everything after the returning one is untouched) */
  int32_t no_more;    /* bNoMore */
  int32_t iterations; /* mnIterations afterwards */
} uvo_pnpsolver_status;
typedef struct uvo_pnpsolver_result {
  int32_t returned;   /* position in ids[] of the solver that returned a pose, -1: none did */
  int32_t solver;     /* its id, -1 */
  int32_t n_inliers;  /* nInliers of that call */
  int32_t refined;    /* 1: Refine()'s pose and set (:227-237), 0: the best hypothesis's at exhaustion (:245-255) */
  float Tcw[16];      /* row-major 4 x 4, R and t rounded double -> float per element, last row 0 0 0 1; zeros when nothing returned */
  uint32_t draws;     /* RandomInt calls consumed by this call: min_set x iterations performed, summed over the touched solvers */
  int32_t pad_;
  uvo_pnpsolver_status* status; /* caller's [n_ids], may be NULL */
  uint8_t* inliers;   /* caller's byte mask vbInliers, as long as the returning solver's n_matches; may be NULL */
  int32_t inliers_cap;/* its length: UVO_E_CAPACITY when the returning solver's n_matches exceeds it */
  int32_t pad2_;
} uvo_pnpsolver_result;

/* A set lives on a uvo_klt handle: launches go to that handle's stream, and the set must be destroyed before it.  All scratch is
 * sized here: max_solvers 1..64 solvers of up to max_points 4..16384 correspondences, 320 hypothesis slots per solver. */
int uvo_pnpsolver_set_create(uvo_klt* k, int max_solvers, int max_points, uvo_pnpsolver_set** out);
void uvo_pnpsolver_set_destroy(uvo_pnpsolver_set* s);
int uvo_pnpsolver_set_clear(uvo_pnpsolver_set* s); /* forget every solver; ids start again at 0 */
/*
 * PnPsolver::PnPsolver(F, vpMapPointMatches) + SetRansacParameters.  The caller has walked vpMapPointMatches as :80-102 does:
 *   p3d [n][3]   GetWorldPos() of match i's map point          p2d [n][2]  F.mvKeysUn[i].pt
 *   sigma2 [n]   F.mvLevelSigma2[kp.octave]                     kp_index[n] i itself (mvKeyPointIndices), each in [0, n_matches)
 *   n_matches    vpMapPointMatches.size()                       fx fy cx cy F's float intrinsics
 * n may be anything from 0 to max_points: a solver with fewer points than its nMinInliers answers bNoMore and draws nothing.
 * UVO_E_BADARG: NaN or out-of-range parameters (probability outside (0,1), min_set outside 4..8, max_iterations < 1), the set full.
 */
int uvo_pnpsolver_add(uvo_pnpsolver_set* s, const float* p3d, const float* p2d, const float* sigma2, const int32_t* kp_index, int n, int n_matches,
                      float fx, float fy, float cx, float cy, const uvo_pnpsolver_params* params, int* id);
int uvo_pnpsolver_query(uvo_pnpsolver_set* s, int id, uvo_pnpsolver_info* info);
/*
 * iterate(n_iterations, bNoMore, vbInliers, nInliers) on ids[0], ids[1], ... in order, stopping after the first that returns a
 * non-empty Tcw (find() is n_iterations = the solver's max_its).  One upload, three launches, one download, nothing allocated.
 * The iterations a solver runs before it returns or gives up do not depend on any result -- max(max_its - mnIterations, n_iterations),
 * the loop condition being an OR (:183) -- so every subset of the call is drawn up front from *rng, every (solver, hypothesis) pair is
 * evaluated in one grid, and the loop is replayed over the counts.  On return *rng has advanced by exactly result->draws outputs:
 * what the reference's rand() would have produced by then.  Solver state (mnIterations, the best count, set and pose) persists, for
 * the touched solvers only.  ids must not repeat within one call.  Semantics pinned to src/PnPsolver.cc by tests/pnpsolver_model.py;
 * single-hypothesis poses (EPnP on 4 points) are held to the host build of the same source only.
 */
int uvo_pnpsolver_iterate(uvo_pnpsolver_set* s, const int32_t* ids, int n_ids, int n_iterations, uvo_glibc_rand* rng, uvo_pnpsolver_result* result);
/* test tap: the hypotheses solver `id` consumed in the set's last iterate call, in draw order: subsets [cap][min_set], poses [cap][12]
 * (R row-major, t; zeros where EPnP gave no finite pose), counts [cap].  *n = hypotheses written (0 for an untouched solver). */
int uvo_pnpsolver_hypotheses(uvo_pnpsolver_set* s, int id, int32_t* subsets, double* poses, int32_t* counts, int cap, int* n);

/* ------------------------------------------------------------------------------------------------
 * Pose-only optimisation -- replaces Optimizer::PoseOptimization(Frame*) (src/Optimizer.cc:2012-2145, the vision-only overload) and
 * the parts of g2o it runs, as TrackWithPnP (:1884), TrackLocalMap (:1925), TrackwithMotionModel (:867) and Relocalisation (:2468,
 * :2484, :2499) call it: one 6-DoF vertex, n fixed points, four rounds of Levenberg steps (its 10, 10, 7, 5; chi2 9.210, 7.378, 5.991,
 * 5.991) with the Huber kernel at sqrt(5.991), the correspondences classified after every round.  ONE call optimises a list of
 * independent problems: one upload, one launch (one workgroup per problem, all four rounds), one download, nothing allocated.
 * The caller gathers each problem by walking mvpMapPoints as :2050-2096 does: for every index with a map point its world position,
 * mvKeysUn[i].pt and mvInvLevelSigma2[octave].  Semantics are pinned to the reference's sources by tests/poseopt_model.py: the pose
 * state is a unit quaternion and a translation in double, built from the float Tcw and normalised after every product; it is NOT
 * reset between rounds; lambda, ni and the stall count are set anew in every round; an edge flagged in one round is judged again at
 * the pose of every later round and comes back when its chi2 has fallen to the threshold; with n < 10 only the first round runs, with
 * n >= 10 all four, however few correspondences are still active; there is no depth test.  Non-finite input is not rejected: it
 * follows the arithmetic (a NaN chi2 satisfies neither test of the classification and leaves the flag as it was).
 * Departures from the reference, all below what the float Tcw resolves on a well-posed problem:
 *   - sums over the correspondences are reduced in a fixed tree over 256 lanes, not serially in index order;
 *   - the 6 x 6 solve is an unpivoted LDL^T that fails unless every pivot is finite and > 0 (Eigen's LDLT pivots and accepts
 *     semi-definite matrices); a failed solve makes the trial's chi2 DBL_MAX, as in the reference;
 *   - sin and cos are the library's own (about 2^-51 absolute), pow(x, 3) is x * x * x; a step that rotates by more than 7 rad gives
 *     a NaN pose for that trial, which is rejected like any other NaN trial.
 * ---------------------------------------------------------------------------------------------- */
typedef struct uvo_pose_optimizer uvo_pose_optimizer;

typedef struct uvo_pose_problem {
  const float* p3d;        /* [n][3] world positions of the map points */
  const float* p2d;        /* [n][2] mvKeysUn[i].pt */
  const float* inv_sigma2; /* [n]    mvInvLevelSigma2[mvKeysUn[i].octave] */
  int32_t n;               /* 0..max_points */
  float fx, fy, cx, cy;
  float Tcw[16];           /* mTcw, row-major; only the upper 3 x 4 is read */
  int32_t pad_;
} uvo_pose_problem;

typedef struct uvo_pose_result {
  float Tcw[16];           /* the optimised pose rounded to float; with nothing to optimise the round trip of the input through a quaternion */
  int32_t n_inliers;       /* nInitialCorrespondences - nBad of the last round run: the return value */
  int32_t rounds;          /* 1 when n < 10, else 4 */
  uint8_t* outlier;        /* caller's [n]: mvbOutlier of the problem's correspondences, in its order; may be NULL */
  int32_t outlier_cap;     /* its length: UVO_E_CAPACITY when smaller than n */
  int32_t pad_;
} uvo_pose_result;

/* test tap: what the Levenberg driver saw */
typedef struct uvo_pose_trace_lin {
  int32_t round, iteration;
  double H[21];            /* upper triangle, row-major, before lambda */
  double b[6];
  double chi2;             /* activeRobustChi2 at the linearisation */
} uvo_pose_trace_lin;
typedef struct uvo_pose_trace_trial {
  int32_t lin;             /* index of its linearisation */
  int32_t ok;              /* the solve succeeded */
  int32_t accepted;
  int32_t pad_;
  double lambda;           /* as used by this trial */
  double cur, tmp;         /* currentChi and tempChi (DBL_MAX after a failed solve) */
  double scale;            /* computeScale() + 1e-3 */
} uvo_pose_trace_trial;
typedef struct uvo_pose_trace {
  int32_t n_lin, n_trials;
  double R[9], t[3];       /* the final pose in double */
  uvo_pose_trace_lin lin[32];
  uvo_pose_trace_trial trial[320];
} uvo_pose_trace;

/* max_problems 1..64, max_points 1..16384 (UVO_E_BADARG otherwise).  The set launches in the KLT handle's stream and must be
 * destroyed before it. */
int uvo_pose_optimizer_create(uvo_klt* k, int max_problems, int max_points, uvo_pose_optimizer** out);
void uvo_pose_optimizer_destroy(uvo_pose_optimizer* o);
/* results[j] answers problems[j].  UVO_E_CAPACITY: n_problems > max_problems, an n > max_points, an outlier mask shorter than n.
 * UVO_E_BADARG: null pointers, negative counts.  Nothing is written on an error.  n_problems == 0 is a no-op. */
int uvo_pose_optimize(uvo_pose_optimizer* o, const uvo_pose_problem* problems, int n_problems, uvo_pose_result* results);
/* test tap: the trace of problem `problem` of the set's last call (UVO_E_BADARG when the last call had no such problem). */
int uvo_pose_optimizer_trace(uvo_pose_optimizer* o, int problem, uvo_pose_trace* out);

/* ------------------------------------------------------------------------------------------------
 * Visual-inertial pose optimisation -- replaces the two IMU overloads of Optimizer::PoseOptimization and the parts of g2o,
 * src/IMU/g2otypes.cpp, NavState.cpp and so3.cpp they run, as TrackWithIMU (src/Tracking.cc:1099,1105), TrackLocalMapWithIMU
 * (:1996,2006) and IMU_Relocalisation (:3035) call them:
 *   UVO_NAV_KEYFRAME  (FrameKTL*, KeyFrame*, IMUPreintegrator, ...), src/Optimizer.cc:779-1103: 15 unknowns (the frame's P, V, R and
 *                     its delta biases), the last key frame fixed; edges: IMU, bias, depth (has_depth), one per correspondence.
 *   UVO_NAV_FRAME     (FrameKTL*, FrameKTL*, IMUPreintegrator, ...), :319-777: 30 unknowns, the last frame free and tied by the prior
 *                     edge (mNavStatePrior, mMargCovInv); the correspondences of both frames.
 * Four rounds of optimize(10), threshold 5.991 in each, THE ESTIMATES RESET TO THE INPUT AT THE START OF EVERY ROUND, both frames'
 * edges classified after each (const float chi2: the comparison is made in float; a NaN chi2 is an inlier), the Huber kernel taken
 * off the reprojection edges only after round index 2, and the break test on the number of ALL edges of the graph (n + n_last + 2 + the
 * prior + the depth edge < 10: one round).  n < 3 (key-frame form) or n < 4 (frame form): 0 inliers, 0 rounds, the state as it came.
 * Hessian order: frame PVR, frame bias, last PVR, last bias.  ONE call optimises a list of problems: one upload, one launch (one
 * workgroup per problem, all four rounds), one download, nothing allocated.  With compute_marg the result carries the current frame's
 * 15 x 15 block of inv(H) -- H as the LAST linearisation of the last round run left it, not a new one at the final estimate -- and
 * mMargCovInv as the overload stores it: the inverses of the 9 x 9 and the 6 x 6 diagonal blocks, the rest zero (key-frame form,
 * :1083-1085), or the inverse of the whole 15 x 15 (frame form, :752-757).
 * Semantics are pinned to the reference's sources by tests/navopt_model.py.  Departures (contract 12):
 *   - sums over the correspondences are reduced in a fixed tree over 256 lanes; the single edges are added in one stated order;
 *   - every solve and inverse (H + lambda I, CovPVPhi, the marginals, mMargCovInv) is one dense unpivoted LDL^T that fails unless
 *     every pivot is finite and > 0, where the reference has Cholmod and Eigen's inverse();
 *   - sin, cos and atan are the library's own; SO3's normalisation on every copy is done once where a quaternion is made;
 *   - the frame form's spinv.block(0,1), which computeMarginals never fills, is read as the joint 15 x 15 block it means;
 *   - the depth edge's information is the caller's scalar: the reference assigns a 2 x 2 block to a 3 x 3 matrix (:470, :913).
 * ---------------------------------------------------------------------------------------------- */
#define UVO_NAV_KEYFRAME 0
#define UVO_NAV_FRAME 1
typedef struct uvo_nav_optimizer uvo_nav_optimizer;

typedef struct uvo_nav_state {   /* NavState */
  double P[3], V[3];
  double q[4];             /* R as SO3 holds it: a unit quaternion x y z w */
  double bg[3], ba[3];     /* BiasGyr, BiasAcc */
  double dbg[3], dba[3];   /* dBias_g, dBias_a */
} uvo_nav_state;

typedef struct uvo_nav_problem {
  int32_t form;            /* UVO_NAV_KEYFRAME or UVO_NAV_FRAME */
  int32_t has_depth;       /* pFrame->mHas_depth */
  int32_t compute_marg;    /* bComputeMarg */
  int32_t n, n_last;       /* correspondences of the current and (frame form) the last frame: 0..max_points each */
  int32_t pad_;
  uvo_nav_state cur, last; /* GetNavState() of the frame and of the last frame or key frame */
  double dT, dP[3], dV[3], dR[9];                    /* getDeltaTime, getDeltaP, getDeltaV, getDeltaR (row-major) */
  double JPg[9], JPa[9], JVg[9], JVa[9], JRg[9];     /* getJPBiasg, getJPBiasa, getJVBiasg, getJVBiasa, getJRBiasg */
  double cov_pvphi[81];    /* getCovPVPhi(), inverted in the library */
  double gw[3], Rbc[9], Pbc[3];
  double fx, fy, cx, cy;
  double gyr_bias_rw2, acc_bias_rw2;                 /* IMUData::getGyrBiasRW2(), getAccBiasRW2() */
  uvo_nav_state prior;     /* frame form: the last frame's mNavStatePrior */
  double prior_info[225];  /* frame form: the last frame's mMargCovInv, row-major */
  double depth_meas;       /* mDepth - ini_depth */
  double shi;              /* (mTimeStamp - last mTimeStamp) / (mDepth_time - last mTimeStamp) */
  double depth_info;       /* the depth edge's information */
  const float* p3d;        /* [n][3], [n][2], [n]: as uvo_pose_problem */
  const float* p2d;
  const float* inv_sigma2;
  const float* p3d_last;   /* [n_last]...: the last frame's, frame form only */
  const float* p2d_last;
  const float* inv_sigma2_last;
} uvo_nav_problem;

typedef struct uvo_nav_result {
  uvo_nav_state ns;        /* ns_recov: SetNavState */
  float Tcw[16];           /* UpdatePoseFromNS */
  int32_t n_inliers;       /* nInitialCorrespondences - nBad */
  int32_t rounds;          /* 0 (too few correspondences), 1 (fewer than 10 edges) or 4 */
  int32_t marg_ok;         /* compute_marg: every factorisation behind the marginals succeeded */
  int32_t outlier_cap, outlier_last_cap;  /* UVO_E_CAPACITY when smaller than n, n_last */
  int32_t pad_;
  uint8_t* outlier;        /* caller's [n]: mvbOutlier of the current frame's correspondences; may be NULL */
  uint8_t* outlier_last;   /* caller's [n_last]: the last frame's (frame form); may be NULL */
  double marg_cov[225];    /* the current frame's (PVR, bias) block of inv(H), row-major; zero without compute_marg */
  double marg_cov_inv[225];/* mMargCovInv */
} uvo_nav_result;

/* test tap: what the Levenberg driver saw */
typedef struct uvo_nav_trace_lin {
  int32_t round, iteration;
  double H[465];           /* upper triangle of the 15 x 15 or 30 x 30 matrix, row-major, packed, before lambda; zero beyond */
  double b[30];
  double chi2;
} uvo_nav_trace_lin;
typedef struct uvo_nav_trace {
  int32_t n_lin, n_trials;
  uvo_nav_trace_lin lin[40];
  uvo_pose_trace_trial trial[400];
} uvo_nav_trace;

/* max_problems 1..64, max_points 1..16384 per frame (UVO_E_BADARG otherwise).  The set launches in the KLT handle's stream and must
 * be destroyed before it. */
int uvo_nav_optimizer_create(uvo_klt* k, int max_problems, int max_points, uvo_nav_optimizer** out);
void uvo_nav_optimizer_destroy(uvo_nav_optimizer* o);
/* results[j] answers problems[j].  UVO_E_CAPACITY: n_problems > max_problems, an n or n_last > max_points, an outlier mask shorter than
 * its count.  UVO_E_BADARG: null pointers, negative counts, a form that is neither.  Nothing is written on an error.  n_problems == 0
 * is a no-op. */
int uvo_nav_optimize(uvo_nav_optimizer* o, const uvo_nav_problem* problems, int n_problems, uvo_nav_result* results);
/* test tap: the trace of problem `problem` of the set's last call (UVO_E_BADARG when the last call had no such problem). */
int uvo_nav_optimizer_trace(uvo_nav_optimizer* o, int problem, uvo_nav_trace* out);

/* ------------------------------------------------------------------------------------------------
 * Sim3Solver -- replaces USLAM::Sim3Solver (include/Sim3Solver.h, src/Sim3Solver.cc) as LoopClosing::ComputeSim3 uses it
 * (src/LoopClosing.cc:373-479): one solver per loop candidate, SetRansacParameters(0.99,2,300), then iterate(5,...) over the candidates
 * in turn until one returns a similarity, whose R, t, s go to SearchBySim3 (uvo_sim3_relative, uvo_search_by_sim3 on the same handle).
 * Here the solvers live in a set, and ONE call iterates a list of them.  The generator is uvo_glibc_rand, as for the PnPsolver.
 * ---------------------------------------------------------------------------------------------- */
typedef struct uvo_sim3solver_set uvo_sim3solver_set;
/* SetRansacParameters(probability, minInliers, maxIterations), src/Sim3Solver.cc:114; the header's defaults are (0.99, 6, 300).
 * probability in (0, 1), min_inliers >= 0, max_iterations 1..320 (the hypothesis slots a set holds per solver): UVO_E_BADARG otherwise. */
typedef struct uvo_sim3solver_params {
  double probability;
  int32_t min_inliers, max_iterations;
} uvo_sim3solver_params;
/* what the constructor reads of one key frame: GetRotation(), GetTranslation(), GetCalibrationMatrix() */
typedef struct uvo_sim3_keyframe {
  float Rcw[9]; /* row-major */
  float tcw[3];
  float fx, fy, cx, cy;
} uvo_sim3_keyframe;
typedef struct uvo_sim3solver_info {
  int32_t n;            /* N: correspondences */
  int32_t max_its;      /* mRansacMaxIts after the adjustment */
  int32_t iterations;   /* mnIterations */
  int32_t best_inliers; /* mnBestInliers */
} uvo_sim3solver_info;
typedef struct uvo_sim3solver_status {
  int32_t touched;    /* iterate() was called on this solver (everything after the returning one is untouched) */
  int32_t no_more;    /* bNoMore */
  int32_t iterations; /* mnIterations afterwards */
} uvo_sim3solver_status;
typedef struct uvo_sim3solver_result {
  int32_t returned;   /* position in ids[] of the solver that returned a transform, -1: none did */
  int32_t solver;     /* its id, -1 */
  int32_t n_inliers;  /* nInliers of that call */
  uint32_t draws;     /* RandomInt calls consumed by this call: 3 x iterations performed, summed over the touched solvers */
  float T12[16];      /* mBestT12, row-major 4 x 4 [s R | t; 0 0 0 1]; zeros when nothing returned */
  float R12[9];       /* mBestRotation, row-major */
  float t12[3];       /* mBestTranslation */
  float scale;        /* mBestScale */
  int32_t pad_;
  uvo_sim3solver_status* status; /* caller's [n_ids], may be NULL */
  uint8_t* inliers;   /* caller's byte mask vbInliers, as long as the returning solver's n_matches, indexed through mvnIndices1; may be NULL */
  int32_t inliers_cap;/* its length: UVO_E_CAPACITY when a listed solver's n_matches exceeds it */
  int32_t pad2_;
} uvo_sim3solver_result;

/* A set lives on a uvo_matcher handle: launches go to that handle's stream and are counted by uvo_matcher_profile, and the set must be
 * destroyed before the handle.  All scratch is sized here: max_solvers 1..64 solvers of up to max_points 3..16384 correspondences,
 * 320 hypothesis slots per solver. */
int uvo_sim3solver_set_create(uvo_matcher* m, int max_solvers, int max_points, uvo_sim3solver_set** out);
void uvo_sim3solver_set_destroy(uvo_sim3solver_set* s);
int uvo_sim3solver_set_clear(uvo_sim3solver_set* s); /* forget every solver; ids start again at 0 */
/*
 * Sim3Solver::Sim3Solver(pKF1, pKF2, vpMatched12) + SetRansacParameters.  The caller has walked vpMatched12 as :62-103 does; per
 * kept correspondence:
 *   x1w, x2w [n][3]          GetWorldPos() of pMP1 and pMP2
 *   sigma2_1, sigma2_2 [n]   pKF->GetSigma2(kp.octave) of the key point in either key frame (0 .. 1e12)
 *   index1 [n]               i1, the position in vpMatched12 (mvnIndices1), each in [0, n_matches)
 *   n_matches                vpMatched12.size() (mN1)
 * The library computes mvX3Dc1/2 = Rcw X + tcw, FromCameraToImage, the truncated thresholds (size_t)(9.210 sigma2) and mRansacMaxIts
 * on the host, once.  n may be anything from 0 to max_points.  With n < 3 the reference would draw from an empty vector; here such a
 * solver never iterates (bNoMore, no draws): the one deliberate departure.
 */
int uvo_sim3solver_add(uvo_sim3solver_set* s, const float* x1w, const float* x2w, const float* sigma2_1, const float* sigma2_2, const int32_t* index1,
                       int n, int n_matches, const uvo_sim3_keyframe* kf1, const uvo_sim3_keyframe* kf2, const uvo_sim3solver_params* params, int* id);
/* SetRansacParameters again (:114-138): mRansacMaxIts is derived anew, mnIterations is zeroed, the best so far is kept */
int uvo_sim3solver_set_ransac_parameters(uvo_sim3solver_set* s, int id, const uvo_sim3solver_params* params);
int uvo_sim3solver_query(uvo_sim3solver_set* s, int id, uvo_sim3solver_info* info);
/*
 * iterate(n_iterations, bNoMore, vbInliers, nInliers) on ids[0], ids[1], ... in order, stopping after the first that returns a
 * transform.  One upload, three launches, one host wait, nothing allocated.  iterate's loop condition is an AND (:158), so a solver
 * runs min(n_iterations, mRansacMaxIts - mnIterations) iterations unless it returns (none if N < mRansacMinInliers): every subset of
 * the call is drawn up front from a copy of *rng, every (solver, hypothesis) pair is evaluated on the device, and the loop is replayed
 * over the counts.  On return *rng has advanced by exactly result->draws outputs.  mnIterations and mnBestInliers persist, for the
 * touched solvers only; a solver that returned can be entered again.  A hypothesis whose T12 or T21 is not finite counts zero
 * inliers.  ids must not repeat within one call.  Semantics pinned to src/Sim3Solver.cc by tests/sim3_model.py.
 * Departures from the reference: (1) a solver with n < 3 never iterates (see uvo_sim3solver_add); (2) mBestT12 / mBestRotation /
 * mBestTranslation / mBestScale are handed out for the returning solver of a call only: the reference also moves them with every new
 * best of a call that returns nothing, which ComputeSim3 never reads, and the library does not keep them (mnBestInliers it does keep);
 * (3) max_iterations is at most 320.
 */
int uvo_sim3solver_iterate(uvo_sim3solver_set* s, const int32_t* ids, int n_ids, int n_iterations, uvo_glibc_rand* rng, uvo_sim3solver_result* result);
/* Sim3Solver::find (:209-213): iterate(mRansacMaxIts) on one solver */
int uvo_sim3solver_find(uvo_sim3solver_set* s, int id, uvo_glibc_rand* rng, uvo_sim3solver_result* result);
/* test tap: the hypotheses solver `id` consumed in the set's last iterate call, in draw order: subsets [cap][3], T12 and T21 [cap][16]
 * (zeros where the transform is not finite), counts [cap].  *n = hypotheses written (0 for an untouched solver). */
int uvo_sim3solver_hypotheses(uvo_sim3solver_set* s, int id, int32_t* subsets, float* T12, float* T21, int32_t* counts, int cap, int* n);

/* ------------------------------------------------------------------------------------------------
 * Sim3 optimisation -- replaces Optimizer::OptimizeSim3(pKF1, pKF2, vpMatches1, g2oS12, th2) (src/Optimizer.cc:2660-2856) and the
 * parts of g2o it runs, the third step of LoopClosing::ComputeSim3 per loop candidate (src/LoopClosing.cc:463): one 7-DoF vertex,
 * n fixed point pairs, per pair the edge through the similarity (EdgeSim3ProjectXYZ) and the edge through its inverse
 * (EdgeInverseSim3ProjectXYZ), both with BaseBinaryEdge's NUMERIC Jacobian (central difference, delta 1e-9), the Huber kernel at
 * sqrt(th2); optimize(5), the inlier check, then optimize(10) when a pair was bad, else optimize(5).  The candidates are independent
 * until one succeeds, so ONE call optimises a list of them -- one upload, one launch (one workgroup per problem, both rounds), one
 * download, nothing allocated -- and the caller takes the first in candidate order with n_inliers >= 10 (:465).
 * The caller gathers each problem by walking vpMatches1 as :2713-2792 does.  Semantics are pinned to the reference's sources by
 * tests/sim3opt_model.py: the state is g2o::Sim3 in double, its quaternion built from the float R12 and NEVER normalised; the update is
 * Sim3(dx) * estimate with the four-branch exponential; lambda, ni and the stall count are set anew in each round, the estimate is
 * not; a pair is bad when the chi2 of either STORED error (that of the last evaluated trial, accepted or not) exceeds th2; a bad pair
 * of the first check is removed for good; a NaN chi2 satisfies neither comparison, so that pair stays and counts as an inlier; when
 * fewer than 10 pairs survive the first check the call returns 0 inliers and the estimate is the input's (its round trip through the
 * quaternion), as the reference returns 0 without writing g2oS12.
 * The weights are taken as given.  The reference passes GetInvSigma2(octave1) for the first edge and GetSigma2(octave2) -- the
 * variance, not its inverse -- for the second (:2781); an adaptor that wants the reference's behaviour passes exactly that.
 * Departures from the reference; parity with a built g2o is not pinned, g2o not being available to the project:
 *   - sums over the pairs are reduced in a fixed tree over 256 lanes, e12 before e21 within a pair, not serially in edge order;
 *   - the 7 x 7 solve is an unpivoted LDL^T that fails unless every pivot is finite and > 0 (Eigen's LDLT pivots and accepts
 *     semi-definite matrices); a failed solve makes the trial's chi2 DBL_MAX, as in the reference;
 *   - sin, cos and exp are the library's own (2^-51); a step with |omega| > 7 rad or |sigma| > 40 gives a NaN trial, which is rejected;
 *   - map() multiplies by one matrix s R per similarity where g2o rotates every point by the quaternion.
 * The numeric Jacobian amplifies those roundings by 5e8: agreement with the model is to a tolerance (T, M of DESIGN.md), agreement
 * between the device and the host build of the same source is bit for bit.
 * ---------------------------------------------------------------------------------------------- */
typedef struct uvo_sim3_optimizer uvo_sim3_optimizer;

typedef struct uvo_sim3_opt_problem {
  const float* x1w;        /* [n][3] GetWorldPos() of pMP1 (the map point of key i of pKF1) */
  const float* x2w;        /* [n][3] GetWorldPos() of pMP2 = vpMatches1[i] */
  const float* obs1;       /* [n][2] pKF1->GetKeyPointUn(i).pt */
  const float* obs2;       /* [n][2] pKF2->GetKeyPointUn(i2).pt */
  const float* info1;      /* [n]    information of e12: the reference passes pKF1->GetInvSigma2(octave1) */
  const float* info2;      /* [n]    information of e21: the reference passes pKF2->GetSigma2(octave2), the variance (:2781) */
  int32_t n;               /* nCorrespondences, 0..max_pairs */
  float th2;
  uvo_sim3_keyframe kf1, kf2; /* the library applies Rcw X + tcw on the host, in float as the reference's cv::Mat product */
  float R12[9], t12[3], s12;  /* the start: g2oS12 as Sim3(R, t, s) is built from the solver's floats */
  int32_t pad_;
} uvo_sim3_opt_problem;

typedef struct uvo_sim3_opt_result {
  double q[4], t[3], s;    /* the estimate: quaternion x y z w (not normalised), translation, scale */
  float R12[9], t12[3], scale; /* the same rounded to float: rotation().toRotationMatrix(), translation(), scale() */
  int32_t n_inliers;       /* the return value; 0 on the early return, the estimate is then the input's round trip */
  int32_t n_correspondences; /* n */
  int32_t n_bad;           /* nBad of the first check */
  int32_t more_iterations; /* iterations asked of the second optimize(): 5 or 10; 0 on the early return, which runs none */
  int32_t removed_cap;     /* length of removed: UVO_E_CAPACITY when smaller than n */
  uint8_t* removed;        /* caller's [n]: 1 where the reference nulls vpMatches1[idx] in either check; may be NULL */
} uvo_sim3_opt_result;

/* test tap: what the Levenberg driver saw; trials are uvo_pose_trace_trial records */
typedef struct uvo_sim3_opt_trace_lin {
  int32_t round, iteration;
  double H[28];            /* upper triangle, row-major, before lambda */
  double b[7];
  double chi2;             /* activeRobustChi2 at the linearisation */
} uvo_sim3_opt_trace_lin;
typedef struct uvo_sim3_opt_trace {
  int32_t n_lin, n_trials;
  double q[4], t[3], s;    /* the final estimate in double */
  uvo_sim3_opt_trace_lin lin[15];
  uvo_pose_trace_trial trial[150];
} uvo_sim3_opt_trace;

/* max_problems 1..64, max_pairs 1..16384 (UVO_E_BADARG otherwise).  The set lives on a uvo_matcher handle (the loop-closing thread's
 * stream, as the Sim3Solver set) and must be destroyed before it. */
int uvo_sim3_optimizer_create(uvo_matcher* m, int max_problems, int max_pairs, uvo_sim3_optimizer** out);
void uvo_sim3_optimizer_destroy(uvo_sim3_optimizer* o);
/* results[j] answers problems[j].  UVO_E_CAPACITY: n_problems > max_problems, an n > max_pairs, a removed mask shorter than n.
 * UVO_E_BADARG: null pointers, negative counts.  Nothing is written on an error.  n_problems == 0 is a no-op. */
int uvo_sim3_optimize(uvo_sim3_optimizer* o, const uvo_sim3_opt_problem* problems, int n_problems, uvo_sim3_opt_result* results);
/* test tap: the trace of problem `problem` of the set's last call (UVO_E_BADARG when the last call had no such problem). */
int uvo_sim3_optimizer_trace(uvo_sim3_optimizer* o, int problem, uvo_sim3_opt_trace* out);

/* ------------------------------------------------------------------------------------------------
 * Bundle adjustment -- replaces Optimizer::LocalBundleAdjustment(pKF, pbStopFlag, pMap, pLM) (src/Optimizer.cc:2147-2405, called at
 * src/LocalMapping.cc:807) and Optimizer::BundleAdjustment(vpKFs, vpMP, nIterations, ...) (:1896-2010, behind
 * GlobalBundleAdjustemnt and RecoveryBundleAdjustemnt) with the parts of g2o they run: VertexSE3Expmap key frames (a fixed one
 * contributes no block), marginalised VertexSBAPointXYZ points, one EdgeSE3ProjectXYZ per observation with information
 * invSigma2 * I and the Huber kernel at sqrt(5.991), BlockSolver's Schur complement rebuilt at every Levenberg trial, the Levenberg
 * driver (tau 1e-5 on the largest diagonal entry over poses AND points, rho over the whole step, ten trials).
 * UVO_BA_LOCAL: optimize(5); an edge is bad when the chi2 of its STORED error (that of the last evaluated trial, accepted or not)
 * exceeds 5.991 or its depth at the current estimates is not positive; edges of points flagged point_bad are not examined; bad edges
 * are removed for good; a point or key frame left without an edge drops out and keeps its estimate; optimize(10); the second check
 * over the surviving edges.  UVO_BA_FULL: one optimize(n_iterations), no check.  Lambda and ni are set anew in each optimize(), the
 * estimates are not.
 * The phases of a call are separate launches in the handle's stream; the Levenberg decision is made on the device and the host reads
 * one status word per trial and per optimize() (n_syncs of the result counts those reads and the download's synchronise: at most
 * 2 + 150 + 1 in local mode).  Nothing is allocated per call.  C++ adaptors: uvo/compat/Optimizer.h.
 * Departures from the reference; parity with a built g2o is not pinned, g2o not being available to the project:
 *   - pbStopFlag is not honoured inside a call: an adaptor reads it before the call and returns without optimising when it is set;
 *   - the reduced pose system is solved by a dense unpivoted LDL^T in key-frame order that fails unless every pivot is finite and > 0,
 *     not by SimplicialLDLT under an AMD ordering; a failed solve makes the trial's chi2 DBL_MAX and the step keeps its last value;
 *   - every sum has one fixed shape that depends on indices alone (csrc/ba_core.hpp), not g2o's order over its containers;
 *   - sin and cos are the library's own (2^-51); a step with |omega| > 7 rad gives a NaN trial, which is rejected.
 * Agreement with the model (tests/ba_model.py) is to a tolerance, agreement between the device and the host build of the same source
 * (tests/emu/ba_emu.cpp) is bit for bit.
 * ---------------------------------------------------------------------------------------------- */
typedef struct uvo_bundle_adjuster uvo_bundle_adjuster;

enum { UVO_BA_LOCAL = 0, UVO_BA_FULL = 1 };

typedef struct uvo_ba_problem {
  int32_t mode;            /* UVO_BA_LOCAL or UVO_BA_FULL */
  int32_t n_iterations;    /* full mode: 1..32; ignored in local mode */
  int32_t n_keyframes, n_points, n_edges, n_cameras;
  const float* kf_Tcw;     /* [n_keyframes][12] rows of [R | t]; converted as Converter::toSE3Quat does */
  const uint8_t* kf_fixed; /* [n_keyframes] 1: fixed.  The adaptor applies the mnId == 0 rule */
  const float* points;     /* [n_points][3] */
  const uint8_t* point_bad;/* [n_points] pMP->isBad() at the checks; may be NULL */
  const int32_t* point_edge_begin; /* [n_points + 1] edges are grouped by point in the order the caller lists them */
  const int32_t* edge_kf;  /* [n_edges] key-frame index */
  const float* edge_obs;   /* [n_edges][2] */
  const float* edge_inv_sigma2; /* [n_edges] */
  const int32_t* edge_camera;   /* [n_edges] row of cameras */
  const float* cameras;    /* [n_cameras][4] fx fy cx cy, 1..64 rows */
} uvo_ba_problem;

typedef struct uvo_ba_result {
  double* kf_estimate;     /* [n_keyframes][7] quaternion x y z w and t; a fixed key frame's is its input's conversion; may be NULL */
  float* kf_Tcw;           /* [n_keyframes][16] Converter::toCvMat of the estimate; may be NULL */
  double* point_estimate;  /* [n_points][3]; may be NULL */
  float* points;           /* [n_points][3]; may be NULL */
  uint8_t* removed1;       /* [n_edges] 1 where the first check erases the observation; may be NULL */
  uint8_t* removed2;       /* [n_edges] the second check; may be NULL */
  int32_t n_removed1, n_removed2;
  int32_t iterations[2];   /* linearisations run per optimize() */
  int32_t n_trials, n_syncs;
} uvo_ba_result;

/* test tap: what the Levenberg driver saw; trials are uvo_pose_trace_trial records */
typedef struct uvo_ba_trace_lin {
  int32_t round, iteration;
  int32_t n_edges, n_free, n_points, pad_; /* active edges, free key frames and points of the linearisation */
  double chi2;             /* activeRobustChi2 at the linearisation */
  double maxdiag;          /* the largest diagonal entry over poses and points */
} uvo_ba_trace_lin;
typedef struct uvo_ba_trace {
  int32_t n_lin, n_trials;
  uvo_ba_trace_lin lin[32];
  uvo_pose_trace_trial trial[320];
} uvo_ba_trace;

/* max_free 1..64, max_fixed 0..256, max_points 1..32768, max_edges 1..262144 (UVO_E_BADARG otherwise).  The adjuster lives on a
 * uvo_matcher handle (the mapping thread's stream, as uvo_create_new_map_points) and must be destroyed before it. */
int uvo_bundle_adjuster_create(uvo_matcher* m, int max_free, int max_fixed, int max_points, int max_edges, uvo_bundle_adjuster** out);
void uvo_bundle_adjuster_destroy(uvo_bundle_adjuster* a);
/* UVO_E_CAPACITY: more free or fixed key frames, points or edges than the adjuster was sized for.  UVO_E_BADARG: null pointers,
 * counts out of range, an edge naming a key frame or camera out of range, a point_edge_begin that does not ascend from 0 to n_edges,
 * two edges of one point to one free key frame.  Nothing is written on an error.  A problem with no free key frame (or no edge) is
 * answered with the inputs unchanged. */
int uvo_bundle_adjust(uvo_bundle_adjuster* a, const uvo_ba_problem* problem, uvo_ba_result* result);
/* test tap: the trace of the adjuster's last call (no record when that call optimised nothing). */
int uvo_bundle_adjuster_trace(uvo_bundle_adjuster* a, uvo_ba_trace* out);

/* ------------------------------------------------------------------------------------------------
 * Visual-inertial local bundle adjustment -- replaces Optimizer::LocalBundleAdjustmentNavState (src/Optimizer.cc:1105-1732, called at
 * src/LocalMapping.cc:811 once per key frame after the IMU is initialised) with the parts of g2o and src/IMU/g2otypes.cpp it runs.
 * Every key frame carries a uvo_nav_state; a free one has 15 unknowns (VertexNavStatePVR dP dV dPhi, then VertexNavStateBias dbg dba),
 * in the caller's order in the reduced system.  Per LINK (kf0 -> kf1, kf1's preintegration): EdgeNavStatePVR on (PVR kf0, PVR kf1,
 * Bias kf0), information CovPVPhi^-1, Huber (float)sqrt(21.666); EdgeNavStateBias on (Bias kf0, Bias kf1), information
 * InvCovBgaRW / dT, Huber (float)sqrt(16.812).  Per DEPTH entry: EdgeNavStateDepthProjected on (PVR ka, PVR kb, Bias kc) with the
 * preintegration of link `link`, Huber (float)sqrt(16.812).  Per observation: EdgeNavStatePVRPointXYZ, information invSigma2 * I,
 * Huber (float)sqrt(5.991); the points are marginalised.
 * optimize(5); first check: of every edge whose point is not flagged, chi2 > 5.991 (in double) or a non-positive depth puts it at
 * level 1 (`excluded`) and the kernel comes off whatever the verdict; edges of flagged points keep kernel and level; the inertial and
 * depth edges are never checked; optimize(10); final check over ALL edges of unflagged points, excluded ones too, on the stored chi2
 * (for an excluded edge: what round one's last evaluation left) and the depth at the final estimates (`erased`).  An edge excluded
 * for its depth alone can survive the final check: that is the reference's behaviour and why there are two masks.
 * Phases are separate launches in the matcher's stream, as for uvo_bundle_adjust; nothing is allocated per call.
 * Departures (contract 13): those of uvo_bundle_adjust and uvo_nav_optimize -- the stop flag is the adaptor's,
 * the dense unpivoted LDL^T in the stated order stands for Eigen's sparse solver and for inverse(), every sum has one shape fixed by
 * indices alone, sin cos atan are the library's own, SO3 is normalised where a quaternion is made -- and the depth entry's
 * information is the caller's scalar (block(0,0,2,2) into a Matrix3d at :1392 is not defined).
 * Agreement with the model (tests/navba_model.py) is to a tolerance; the device and the host build (tests/emu/navba_emu.cpp) agree
 * bit for bit.
 * ---------------------------------------------------------------------------------------------- */
typedef struct uvo_nav_bundle_adjuster uvo_nav_bundle_adjuster;

typedef struct uvo_nav_ba_link {
  int32_t kf0, kf1;        /* pKF1->GetPrevKeyFrame() and pKF1 */
  double dT, dP[3], dV[3], dR[9];                    /* pKF1->GetIMUPreInt(): as uvo_nav_problem */
  double JPg[9], JPa[9], JVg[9], JVa[9], JRg[9];
  double cov_pvphi[81];    /* getCovPVPhi(), inverted in the library */
} uvo_nav_ba_link;

typedef struct uvo_nav_ba_depth {
  int32_t ka, kb, kc;      /* vertices: PVR of ka, PVR of kb, Bias of kc.  Forward: (pKF1, pKF0, pKF0); backward: (pKF0, pKF_1, pKF_1) */
  int32_t link;            /* whose preintegration the edge reads.  Forward: pKF1's link; backward: pKF_1's, as :1435 has it */
  double shi, meas, info;  /* timeshi, depth - ini_depth, the information */
} uvo_nav_ba_depth;

typedef struct uvo_nav_ba_problem {
  int32_t n_keyframes, n_points, n_edges, n_cameras, n_links, n_depth;
  const uvo_nav_state* kf_state;   /* [n_keyframes] GetNavState() */
  const uint8_t* kf_fixed;         /* [n_keyframes] 1: both vertices fixed */
  const uint8_t* kf_has_bias;      /* [n_keyframes] 1: carries a bias vertex (window key frames and pKFPrevLocal) */
  const float* points;             /* the points, the edge lists and the cameras: as uvo_ba_problem */
  const uint8_t* point_bad;        /* may be NULL */
  const int32_t* point_edge_begin;
  const int32_t* edge_kf;
  const float* edge_obs;
  const float* edge_inv_sigma2;
  const int32_t* edge_camera;
  const float* cameras;            /* [n_cameras][4], 1..64 rows */
  double Rbc[9], Pbc[3], gw[3];
  double gyr_bias_rw2, acc_bias_rw2;
  const uvo_nav_ba_link* links;    /* [n_links] 0..48 */
  const uvo_nav_ba_depth* depth;   /* [n_depth] */
} uvo_nav_ba_problem;

typedef struct uvo_nav_ba_result {
  uvo_nav_state* kf_state; /* [n_keyframes] P V R of the PVR estimate, dbg dba of the bias estimate; a fixed one's is its input; may be NULL */
  float* kf_Tcw;           /* [n_keyframes][16] UpdatePoseFromNS; may be NULL */
  double* point_estimate;  /* [n_points][3]; may be NULL */
  float* points;           /* [n_points][3]; may be NULL */
  uint8_t* excluded;       /* [n_edges] 1 where the first check puts the edge at level 1; may be NULL */
  uint8_t* erased;         /* [n_edges] 1 where the final check erases the observation; may be NULL */
  int32_t n_excluded, n_erased;
  int32_t iterations[2];
  int32_t n_trials, n_syncs;
} uvo_nav_ba_result;

/* test tap: one record per linearisation (n_edges counts the inertial edges too), uvo_pose_trace_trial records per trial */
typedef struct uvo_nav_ba_trace_lin {
  int32_t round, iteration;
  int32_t n_edges, n_free, n_points, pad_;
  double chi2;
  double maxdiag;
} uvo_nav_ba_trace_lin;
typedef struct uvo_nav_ba_trace {
  int32_t n_lin, n_trials;
  uvo_nav_ba_trace_lin lin[32];
  uvo_pose_trace_trial trial[320];
} uvo_nav_ba_trace;

/* max_free 1..24 (a 360 x 360 solve), max_fixed 0..256, max_points 1..32768, max_edges 1..262144, max_depth 0..256 (UVO_E_BADARG
 * otherwise).  The adjuster lives on a uvo_matcher handle, as uvo_bundle_adjuster, and must be destroyed before it. */
int uvo_nav_bundle_adjuster_create(uvo_matcher* m, int max_free, int max_fixed, int max_points, int max_edges, int max_depth,
                                   uvo_nav_bundle_adjuster** out);
void uvo_nav_bundle_adjuster_destroy(uvo_nav_bundle_adjuster* a);
/* UVO_E_CAPACITY: more free or fixed key frames, points, edges, links or depth entries than the adjuster was sized for.
 * UVO_E_BADARG: as uvo_bundle_adjust, and: a link or depth entry naming a key frame (or a link) out of range or one key frame twice,
 * one naming the bias vertex of a key frame that carries none, a free key frame with no link ending in it or without a bias vertex.
 * Nothing is written on an error.  A problem with no free key frame is answered with the inputs unchanged. */
int uvo_nav_bundle_adjust(uvo_nav_bundle_adjuster* a, const uvo_nav_ba_problem* problem, uvo_nav_ba_result* result);
/* test tap: the trace of the adjuster's last call (no record when that call optimised nothing). */
int uvo_nav_bundle_adjuster_trace(uvo_nav_bundle_adjuster* a, uvo_nav_ba_trace* out);

/* ------------------------------------------------------------------------------------------------
 * Essential-graph optimisation -- replaces Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:2409-2658, called at
 * src/LoopClosing.cc:678) for a caller that has gathered the graph, with the parts of g2o it runs: one VertexSim3Expmap per key frame
 * (scale free: _fix_scale stays false; the loop key frame fixed), one EdgeSim3 per edge with the measurement S_j * S_i^-1, information
 * I_7, no robust kernel and BaseBinaryEdge's numeric Jacobian (delta 1e-9, central), the Levenberg driver with
 * setUserLambdaInit(1e-16), then the SE3 poses [R | t / s] and every map point as correctedSwr.map(Srw.map(X)).
 * Key frames stand in ascending mnId (the adaptor's order); the system is solved by an unpivoted block-envelope LDL^T in that order:
 * row i of 7 x 7 blocks holds the blocks first(i) .. i, first(i) the smallest free index an edge joins to i.  The handle is sized in
 * such blocks, and a graph whose envelope needs more is refused with UVO_E_CAPACITY (uvo_last_error() names both counts).
 * The phases of a call are separate launches in the handle's stream; the Levenberg decision is made on the device and the host reads
 * one status word per trial (n_syncs counts those reads and the download's synchronise).  Nothing is allocated per call.
 * Departures from the reference; parity with a built g2o is not pinned, g2o not being available to the project:
 *   - the envelope LDL^T in key-frame order fails unless every pivot is finite and > 0, where the reference runs SimplicialLDLT under
 *     an AMD ordering; a failed solve makes the trial's chi2 DBL_MAX and the step keeps its last value;
 *   - every sum has one fixed shape that depends on indices alone (csrc/essential_core.hpp), not g2o's order over its containers;
 *   - sin, cos, acos, exp and log are the library's own (2^-50 or better); a scale outside 2^-60 .. 2^60 gives a NaN trial.
 * Agreement with the model (tests/essential_model.py) is to a tolerance, agreement between the device and the host build of the same
 * source (tests/emu/essential_emu.cpp) is bit for bit.
 * ---------------------------------------------------------------------------------------------- */
typedef struct uvo_essential_graph uvo_essential_graph;
typedef struct uvo_sim3d {
  double q[4]; /* x y z w, not normalised */
  double t[3];
  double s;
} uvo_sim3d;
typedef struct uvo_essential_problem {
  int32_t n_keyframes, n_edges, n_points, fixed; /* key frames in ascending mnId; fixed: index of pLoopKF */
  const uvo_sim3d* Scw;           /* [K] vScw: CorrectedSim3 where present, else (Rcw, tcw, 1) widened from the floats */
  const uvo_sim3d* Scw_normal;    /* [K] NonCorrectedSim3 where present, else Scw: what the "normal" edges measure from */
  const int32_t *edge_i, *edge_j; /* [E] in the reference's order of insertion; vertex 0 = i, vertex 1 = j */
  const uint8_t* edge_connection; /* [E] 1: an edge of LoopConnections (measured from Scw), 0: normal (from Scw_normal) */
  const float* points;            /* [P][3] */
  const int32_t* point_ref;       /* [P] index of the key frame nIDr */
  int32_t n_iterations;           /* 1..32; the reference passes 20 */
} uvo_essential_problem;
typedef struct uvo_essential_result {
  uvo_sim3d* Scw; /* [K] the estimates; may be NULL */
  float* kf_Tcw;  /* [K][16] [R | t / s] as Converter::toCvSE3 narrows it; may be NULL */
  float* points;  /* [P][3]; may be NULL */
  int32_t iterations, n_trials, n_syncs, envelope_blocks;
} uvo_essential_result;
/* test tap: uvo_ba_trace's records; per linearisation chi2 (and the largest diagonal entry, which the user's lambda leaves unused),
 * per trial lambda, cur, tmp, scale, ok, accepted */
typedef uvo_ba_trace uvo_essential_trace;

/* max_keyframes 1..8192, max_edges 1..262144, max_envelope_blocks 1..4194304, max_points 0..1048576 (UVO_E_BADARG otherwise).  The
 * handle lives on a uvo_matcher handle (the loop-closing thread's) and must be destroyed before it. */
int uvo_essential_graph_create(uvo_matcher* m, int max_keyframes, int max_edges, int max_envelope_blocks, int max_points, uvo_essential_graph** out);
void uvo_essential_graph_destroy(uvo_essential_graph* g);
/* UVO_E_BADARG, with a message and nothing touched: null pointers, counts out of range, `fixed`, an edge's key frame or a point's
 * reference outside [0, K), an edge with i == j.  (The problem carries no mnId: that the key frames ascend is the caller's to keep.)
 * UVO_E_CAPACITY: more key frames, edges, points or envelope blocks than the handle was sized for.  With zero edges or a single
 * key frame the answer is the input's: poses recovered, points mapped, no iteration. */
int uvo_essential_graph_optimize(uvo_essential_graph* g, const uvo_essential_problem* problem, uvo_essential_result* result);
/* test tap: the trace of the handle's last call. */
int uvo_essential_graph_trace(uvo_essential_graph* g, uvo_essential_trace* out);

/*
 * Initializer -- replaces USLAM::Initializer (include/Initializer.h, src/Initializer.cc) as Tracking::Initialize (src/Tracking.cc:1340)
 * and the recovery path (:1582) use it: the constructor on the reference frame, then Initialize(current frame, matches) until it
 * returns true.  ONE call draws the sets, evaluates every hypothesis against every match, decomposes the best F and triangulates
 * every inlier under the four motions.  The generator is uvo_glibc_rand (the reference draws from the process's never-seeded rand(),
 * the stream PnPsolver and Sim3Solver consume too); a call with n2 >= 8 consumes exactly 8 * iterations outputs.
 * Only the F path is built: Initialize returns ReconstructF unconditionally (src/Initializer.cc:110; the ReconstructH branch is
 * commented out and nothing FindHomography produces leaves the function), so FindHomography, ComputeH21, CheckHomography, ReconstructH
 * and Re_CheckRT (whose only call is commented out, src/Tracking.cc:1591) do not exist here.
 * Departures from the reference: (1) n2 < 8, where the reference's draw is undefined, returns "not initialised" and consumes no
 * draws; (2) when no hypothesis scores above 0 the reference indexes an empty inlier vector: here that call returns "not initialised"
 * with best = -1; (3) iterations is at most 1024; (4) the caller's generator takes the place of rand(); (5) the parallax order
 * statistic of a set that holds a NaN is the value a total order gives.  Semantics pinned to src/Initializer.cc by
 * tests/initializer_model.py; tolerance contract: DESIGN.md section 4.
 */
typedef struct uvo_initializer uvo_initializer;
typedef struct uvo_initializer_result {
  int32_t initialized;  /* the return value of Initialize */
  int32_t best;         /* the hypothesis FindFundamental kept (strictly the first of the largest score), -1: none scored above 0 */
  int32_t n_inliers;    /* inliers of F21 (N of ReconstructF) */
  uint32_t draws;       /* generator outputs consumed */
  int32_t deciding;     /* 0..3: the first CheckRT count that equals maxGood; -1 when CheckRT never ran */
  int32_t n_good[4];    /* nGood1..4: (R1, t), (R2, t), (R1, -t), (R2, -t) */
  float parallax[4];    /* parallax1..4 in degrees */
  float score;          /* SF */
  float R21[9], t21[3]; /* row-major; zeros unless initialized */
  float F21[9];         /* zeros when best < 0 */
  int32_t pad_;
  uint8_t* inliers;      /* caller's n2 bytes, may be NULL: vbMatchesInliersF */
  float* p3d;            /* caller's n2 x 3 floats, may be NULL: vP3D, indexed by the current frame's key; zeros unless initialized */
  uint8_t* triangulated; /* caller's n2 bytes, may be NULL: vbTriangulated; zeros unless initialized */
} uvo_initializer_result;
/* max_keys: 8..16384 keys per frame.  The object launches in the uvo_klt handle's stream and must be destroyed before it. */
int uvo_initializer_create(uvo_klt* k, int max_keys, uvo_initializer** out);
void uvo_initializer_destroy(uvo_initializer* init);
/* Initializer(ReferenceFrame, sigma, iterations): keys1_xy = mvKeysUn of the reference frame (n1 x (x, y), 1 <= n1 <= max_keys), cam's
 * fx, fy, cx, cy = mK; (1.0, 200) at the call sites; 1 <= iterations <= 1024, sigma > 0.  May be called again at any time. */
int uvo_initializer_set_reference(uvo_initializer* init, const float* keys1_xy, int n1, const uvo_camera_model* cam, float sigma, int iterations);
/* Initialize(CurrentFrame, vMatches12, ...): keys2_xy = mvKeysUn of the current frame (n2 <= max_keys), matches12[i] = the reference
 * key of current key i (src/Initializer.cc:51-59: every i is a match, there is no >= 0 test; two may name the same reference key).
 * An entry outside 0..n1-1: UVO_E_BADARG.  On return *rng has advanced by exactly result->draws outputs. */
int uvo_initializer_initialize(uvo_initializer* init, const float* keys2_xy, int n2, const int32_t* matches12, uvo_glibc_rand* rng,
                               uvo_initializer_result* result);
/* test tap: every set of the last initialize call, its F21i and its score, in draw order: subsets [cap][8], F [cap][9], scores [cap].
 * *n = hypotheses written (0 after a call with n2 < 8). */
int uvo_initializer_hypotheses(uvo_initializer* init, int32_t* subsets, float* F, float* scores, int cap, int* n);

/* ------------------------------------------------------------------------------------------------------------------------------
 * Keyframe database -- replaces USLAM::KeyFrameDatabase (include/KeyFrameDatabase.h, src/KeyFrameDatabase.cc) as the first step of
 * Tracking::Relocalisation (src/Tracking.cc:2373-2379: DetectRelocalisationCandidates) and of LoopClosing::DetectLoop
 * (src/LoopClosing.cc:195-196: DetectLoopCandidates, DetectLoopCandidatesHaloc).  The keyframes' BoW vectors, haloc hashes, covisible
 * rows and the six per-keyframe query fields of the reference live on the device; ONE call answers a query: per-keyframe common-word
 * count, first common word, L1 score and hash distance in parallel, then the ordered epilogue, with no host round trip between.
 * Only the L1 score is built (DBoW2::L1Scoring, Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68): it is what ORBvoc declares; the other
 * scorings, DetectLoop's own prologue (src/LoopClosing.cc:155-188) and the cluster candidates (getCandidates_haloc,
 * getCandidates_Proximity) do not exist here.
 * A keyframe keeps the slot uvo_kfdb_add gave it until uvo_kfdb_clear.  The six fields persist between queries as the reference's do:
 * a query reads the values an earlier one left (a neighbour's score from an earlier query with the same id is added again).
 * Departures from the reference: (1) the mRelocScore / mLoopScore of a keyframe never scored since its add is 0.0f (the reference
 * reads an uninitialised float); (2) uvo_kfdb_clear drops the hash list too (the reference keeps dangling pointers in kfVec);
 * (3) the haloc matches are ordered by (distance, add order): the reference's std::sort leaves the order of equal distances open;
 * (4) a covisible neighbour that has no slot (-1) is skipped.  Semantics pinned to the sources by tests/kfdb_model.py; every float
 * is bit-exact.
 */
#define UVO_KFDB_COVISIBLES 10 /* GetBestCovisibilityKeyFrames(10) */
#define UVO_KFDB_LISTED 1      /* uvo_kfdb_query_row.flags: in lKFsSharingWords (always set) */
#define UVO_KFDB_SCORED 2      /* words > minCommonWords: the score was computed and stored */
#define UVO_KFDB_ENTERED 4     /* in lScoreAndMatch (loop: si >= minScore): acc and best are valid */
#define UVO_KFDB_RETAINED 8    /* acc > 0.75f * bestAccScore (before the first-occurrence dedup of best) */
typedef struct uvo_kfdb uvo_kfdb;
typedef struct uvo_kfdb_fields { /* the reference's per-keyframe query fields */
  int64_t loop_query;   /* mnLoopQuery, 0 at add */
  int64_t reloc_query;  /* mnRelocQuery, 0 at add */
  int32_t loop_words;   /* mnLoopWords, 0 at add */
  int32_t reloc_words;  /* mnRelocWords, 0 at add */
  float loop_score;     /* mLoopScore, 0.0f at add */
  float reloc_score;    /* mRelocScore, 0.0f at add */
} uvo_kfdb_fields;
typedef struct uvo_kfdb_query_row { /* one keyframe of lKFsSharingWords, in list order */
  int32_t slot;
  int32_t words; /* mn{Loop,Reloc}Words after the walk */
  int32_t flags; /* UVO_KFDB_* */
  int32_t best;  /* pBestKF's slot, -1 unless ENTERED */
  float score;   /* the stored m{Loop,Reloc}Score after the scoring loop (a stale value unless SCORED) */
  float acc;     /* accScore, 0 unless ENTERED */
} uvo_kfdb_query_row;
/* max_keyframes 1..65536 slots, max_words 1..4096 (longest BoW vector, of a keyframe or a query), hash_len 1..4096 floats. */
int uvo_kfdb_create(int max_keyframes, int max_words, int hash_len, int device, uvo_kfdb** out);
void uvo_kfdb_destroy(uvo_kfdb* db);
/* KeyFrameDatabase::add (:39-46): id = mnId; the BoW vector as uvo_bow_transform emits it (n_bow ids strictly ascending, else
 * UVO_E_BADARG; n_bow 0 allowed); hash = GetHalocVector(), hash_len floats, NULL for an empty one.  One row upload, no reallocation:
 * UVO_E_CAPACITY when every slot is taken or n_bow > max_words. */
int uvo_kfdb_add(uvo_kfdb* db, int64_t id, const uint32_t* bow_id, const double* bow_value, int n_bow, const float* hash, int* slot);
/* KeyFrameDatabase::erase (:48-67): out of the BoW queries only; the haloc query still sees the keyframe (kfVec is never pruned) and its
 * state stays readable as a neighbour's.  Erasing twice is a no-op; a slot that holds no keyframe: UVO_E_BADARG. */
int uvo_kfdb_erase(uvo_kfdb* db, int slot);
/* KeyFrameDatabase::clear (:69-73), and every slot freed. */
int uvo_kfdb_clear(uvo_kfdb* db);
/* GetBestCovisibilityKeyFrames(10) of the keyframe in slot, in its order: n <= 10 slots, -1 for a neighbour without one; empty at add.
 * n > 10 or a neighbour that is neither -1 nor a held slot: UVO_E_BADARG. */
int uvo_kfdb_set_covisibles(uvo_kfdb* db, int slot, const int32_t* neigh_slots, int n);
/* DetectRelocalisationCandidates(F): query_id = F->mnId, the frame's BoW vector (n_bow <= max_words, ascending).  cand_slot[0..*n_cand)
 * = vpRelocCandidates in order; *n_cand > cap: UVO_E_CAPACITY, nothing written to cand_slot (the state has been updated). */
int uvo_kfdb_detect_reloc(uvo_kfdb* db, int64_t query_id, const uint32_t* bow_id, const double* bow_value, int n_bow, int32_t* cand_slot, int cap,
                          int* n_cand);
/* DetectLoopCandidates(pKF, minScore): connected_slots = the slots of pKF->GetConnectedKeyFrames() (those that have one). */
int uvo_kfdb_detect_loop(uvo_kfdb* db, int64_t query_id, const uint32_t* bow_id, const double* bow_value, int n_bow, const int32_t* connected_slots,
                         int n_connected, float min_score, int32_t* cand_slot, int cap, int* n_cand);
/* DetectLoopCandidatesHaloc(pKF, maxScore, haloc): hash = pKF->GetHalocVector() (NULL: empty); exclude_ids = no_candidates (mnIds,
 * n_exclude <= max_keyframes).  *n_cand is 3 or 0: the reference returns its best three only when at least three matches were kept
 * (:125-132) and nothing otherwise. */
int uvo_kfdb_detect_loop_haloc(uvo_kfdb* db, int64_t query_id, const float* hash, const int64_t* exclude_ids, int n_exclude, float max_score,
                               int32_t cand_slot[3], int* n_cand);
/* test taps.  _last_query: lKFsSharingWords of the last BoW query in list order (*n rows; UVO_E_CAPACITY when cap is smaller), with
 * maxCommonWords and minCommonWords.  _last_haloc: per slot the distance m of the last haloc query and whether it was kept (a slot
 * skipped as the query itself or as excluded: m = 0, kept = 0).  _state: the fields of n slots from first_slot on. */
int uvo_kfdb_last_query(uvo_kfdb* db, uvo_kfdb_query_row* rows, int cap, int* n, int* max_common, int* min_common);
int uvo_kfdb_last_haloc(uvo_kfdb* db, float* m, uint8_t* kept, int cap, int* n);
int uvo_kfdb_state(uvo_kfdb* db, int first_slot, int n, uvo_kfdb_fields* out);
/* slots handed out since the last clear */
int uvo_kfdb_size(uvo_kfdb* db);

/* last HIP / argument error text for the calling thread's most recent failing call (never NULL) */
const char* uvo_last_error(void);
/* library + device description, e.g. "uvo 0.1 gfx950 AMD Instinct MI355X" */
int uvo_device_info(int device, char* dst, int cap);

#ifdef __cplusplus
}
#endif
#endif /* UVO_UVO_H_ */
