// Private to the library's host translation units: the handle behind uvo_extractor*, its pipeline lanes, the one owner of its
// device and page-locked memory, and the prototypes of every cross-handle hook (`*_internal`) -- the extractor's and the
// matcher's alike.  The hooks are extern "C": declared here and nowhere else, so that a changed signature fails to compile
// instead of linking and misbehaving.
//   extractor_geom.cpp  constructor tables, per-resolution geometry, resize tables, tile-group specs (no HIP runtime call)
//   extractor.cpp       the handle: create / destroy, lanes, set_geometry, the launch sequence, tune, profile, test taps
//   extractor_host.cpp  the host-buffer entry points: staging of a call's inputs and outputs around the launch sequence
#pragma once
#include <algorithm>
#include <mutex>
#include <vector>

#include "devmem.hpp"
#include "profiler.hpp"
#include "tune_internal.h"

struct uvo_matcher;

namespace uvo {

// Per-batch scratch + stream.  With pipeline depth 2 consecutive uvo_extract_batch_device calls alternate between two
// lanes, so the latency-bound stages of one batch (quad-tree, sparse NMS, small pyramid levels) overlap with the
// throughput stages of the next.
constexpr int kMaxLanes = 4;
constexpr int kTilePyramidFrames = 8;  // batches up to this size build the pyramid in one k_pyr_tiles launch
constexpr int kFewFrames = 2;  // batches up to this size are the latency path (the FAST kernels cut their segments short for them: fast_rows_per_seg)
constexpr int kSmallBatch = 16;  // host-buffer calls: above this the caller-side copies are a small part of the call

struct Lane {
  hipStream_t stream = nullptr;  // everything of a batch runs in this ONE in-order stream (no side streams: an error return leaves nothing to join)
  DevMem mem;                    // owns d.* and a_*
  LaneScratch d;
  // staging of the asynchronous host-buffer form (allocated on first use): a lane's frames and results must not be touched by the
  // other lane's batch
  uint8_t* a_imgs = nullptr;
  uvo_keypoint* a_kp = nullptr;
  uint8_t* a_desc = nullptr;
  int32_t* a_n = nullptr;
  int a_batch = 0;  // frames of the batch in flight on this lane (0 = none)
  hipEvent_t a_uploaded = nullptr;  // recorded behind the lane's frame upload (asynchronous host form)
  // Device-resident batches never make the host wait, and a caller that enqueues them in a loop runs ahead of the device until the
  // runtime's own back-pressure stops it -- in bursts: the queue drains completely before the host is let go (0.9 - 1.5 ms with nothing in
  // flight every seven batches of 256 frames, tools/step_trace_summary.py).  The lane bounds its own depth instead: a batch is enqueued
  // only when the lane's last but one has finished, so at most two batches of a lane are ever outstanding.
  hipEvent_t done[2] = {nullptr, nullptr};
  unsigned n_enqueued = 0;
  // level 0 of the lane's last batch was read in place (no padded plane was written): what uvo_extractor_read_plane needs to make one
  const uint8_t* l0_src = nullptr;
  int64_t l0_stride = 0, l0_frame_stride = 0;
  int ring_used = 0;  // border pixels the lane's last batch wrote around levels >= 1 (what uvo_extractor_read_plane has to complete)
};

// One batch as an entry point hands it on: the caller's arrays (host-buffer forms) or what the kernels read and write (run_batch_device).
struct Batch {
  int n;  // frames
  // the image view
  const uint8_t* imgs;
  int width, height;
  ptrdiff_t stride, frame_stride;
  // top-up inputs (full_detect == 0)
  const uvo_keypoint* in_kp;  // [n][max_input_keypoints]
  const int32_t* n_in;
  int32_t* grid;  // [n][grid_cols][grid_rows]
  int grid_rows, grid_cols, min_px_dist, full_detect;
  const int32_t* nfn;  // num_feats_needed
  // outputs
  uvo_keypoint* out_kp;  // [n][cap]
  uint8_t* out_desc;
  int cap;
  int32_t* n_out;
};

// A group of consecutive pyramid levels built by one k_pyr_tiles launch
struct TileGroup {
  int first = 0, last = 0, tx = 0, ty = 0, threads = 256, rows = 4;  // rows: output rows per work item (1: only with 1024 threads)
  uint32_t lds = 0;
  PyrTileLevel* d_plan = nullptr;
};

}  // namespace uvo

struct uvo_extractor {
  uvo_extractor_cfg cfg;
  std::mutex followers_mu;               // attach / detach may come from the matcher's thread
  std::vector<uvo_matcher*> followers;  // matchers attached to this handle (uvo_matcher_attach_extractor): they enqueue in the current lane's stream
  int device = 0;
  uvo::DevMem mem;  // owns every d_* / h_* below, and the tile groups' plans
  uvo::Lane lane[uvo::kMaxLanes];
  int nlanes = 1, cur = 0;  // cur = the lane of the most recent batch
  // one profiler for the handle: a handle is driven by one host thread, the lanes share the event pool, and the records are in enqueue
  // order whatever lane's stream they ran in
  uvo::Profiler prof;
  uvo::OctLaunchState oct;  // quad-tree launch shape + what has been configured on this handle's device
  uint8_t* d_grid_score = nullptr;  // score plane of the Grider_FAST mode (allocated on first use)
  // constructor tables (src/ORBextractor.cc:463-511)
  std::vector<float> scale, inv_scale;
  std::vector<int> quota;
  int umax[16];
  int gtaps[4];
  // current geometry
  uvo::Geom geom;
  bool have_geom = false;
  std::vector<uvo::CellDesc> cells;
  std::vector<int32_t> cell_flag;  // per entry of a frame's cell-flag array (the full nRows x nCols grids of all levels): cell | level << 24, -1 = no cell
  int fast_mode = UVO_FAST_MODE_ADAPTIVE;
  int blur_rounding = UVO_BLUR_ROUNDING_SSE2;  // UVO_TUNE_BLUR_ROUNDING: what an x86-64 OpenCV 3.4 build (the reference's platform) executes
  // capacities fixed at create time (from max_width x max_height)
  int64_t cap_pyr_block = 0, cap_cand_block = 0;
  int cap_cells = 0, cap_sel_block = 0, cap_flist = 0, cap_xtab = 0, cap_ytab = 0;
  size_t cap_cor = 0, cap_cor_n = 0, cap_flags = 0;
  int last_batch = 0;
  // shared read-only tables
  uvo::LevelGeom* d_lv = nullptr;
  uint16_t* d_oct_tab = nullptr;  // the quad-tree's path tables of the current geometry (octree_fill_path_tables), per level at LevelGeom::oct_tab_off
  int cap_oct_tab = 0;
  uvo::CellDesc* d_cells = nullptr;
  int32_t* d_cell_flag = nullptr;
  uvo::ResizeCol* d_ctab = nullptr;
  uint8_t* d_clahe_lut = nullptr;  // [max_batch][tiles][256], grown on demand
  uint8_t* d_clahe_out = nullptr;  // result of the host entry point (tight rows); stays valid for img == NULL calls
  int clahe_w = 0, clahe_h = 0;
  int resize_fast[uvo::kMaxLevels] = {0};  // per level: the 12-byte-window path of k_resize_level applies
  uvo::ResizeRow* d_rtab = nullptr;
  // the fused pyramid launches (pyramid.hip: k_pyr_tiles; plans: pyr_tiles.hpp).  pyr_form: UVO_TUNE_PYR_FORM.  One set of level groups per
  // geometry -- the latency shape (few frames: one launch of many small tiles), or a forced set (UVO_TUNE_PYR_TILE_GROUP); an empty set = the
  // per-level launches.  (Batches that fill the chip take the per-level launches: shallow groups of large tiles -- 4 % redundant pixels --
  // measured 0.26 - 0.31 ms against the launches' 0.16 at 256 frames, profiles/r05_pyr_tiles_ab.txt.)
  std::vector<uvo::TileGroup> tile_groups;
  uint32_t pyr_tiles_max_lds = 64 * 1024;  // LDS a tile plan may use on this device (prepare_pyr_tiles); plans that need more fall back to the per-level launches
  std::vector<uint32_t> tile_spec;  // forced groups: first << 16 | tx << 8 | ty | (1024 threads) << 24 | (1024 threads, single-row items) << 25, ascending first levels
  int pyr_form = UVO_PYR_FORM_AUTO;
  std::vector<uvo::ResizeCol> ctab_host;  // the resize tables of the current geometry (the plans are compiled from them)
  std::vector<uvo::ResizeRow> rtab_host;
  int pyr_ring = 4;          // UVO_TUNE_PYR_RING: the chain's resize launches write the ROI + this many pixels around it (0: the whole 16-pixel pad)
  int level0_inplace = 1;    // UVO_TUNE_LEVEL0_INPLACE: read level 0 from the caller's image instead of copying it into a padded plane (when it can be)
  int zero_copy_out = 1;     // UVO_TUNE_ZERO_COPY_OUT: host-buffer calls of up to kSmallBatch frames have the kernels read and write page-locked host memory (0: they take the direct copies of larger batches)
  int spin_wait = 1;         // UVO_TUNE_SPIN_WAIT: those calls, and uvo_extractor_synchronize behind a small batch, poll the stream instead of sleeping
  int few_frames_shape = 1;  // UVO_TUNE_FEW_FRAMES: FullDetect batches of up to kFewFrames frames take the short launch chain (no k_assemble: k_describe finds its slots itself)
  int fuse_blur_tree = 1;    // UVO_TUNE_FUSE_BLUR_TREE: quad-tree and blur as one launch when the batch takes the 256-thread quad-tree form
  float* d_pattern = nullptr;   // 256 point pairs (x0, y0, x1, y1) of the rBRIEF pattern as floats
  uint32_t* d_patch = nullptr;  // 256 byte masks: which of the 4 pixels of an orientation-patch dword lie inside the circle
  // staging for the host-buffer entry points
  uint8_t* d_imgs = nullptr;
  uvo_keypoint *d_out_kp = nullptr, *d_in_kp = nullptr;
  uint8_t* d_out_desc = nullptr;
  int32_t *d_n_out = nullptr, *d_n_in = nullptr, *d_nfn = nullptr, *d_grid = nullptr;  // d_grid: grown on demand
  // page-locked region of the host-buffer entry points' small batches (grown on demand): the kernels read the call's small inputs and
  // write its results here, through h_pin_dev
  uint8_t* h_pin = nullptr;
  uint8_t* h_pin_dev = nullptr;  // the same memory as the device addresses it (NULL: the block has no device address)
  // asynchronous host form: the event behind the most recent frame upload of ANY lane.  The next upload waits for it, so that uploads
  // follow one another instead of sharing the link: two lanes that upload at the same time finish together, then compute together,
  // then download together -- link idle while the GPU works and the GPU idle while the link works (measured: 2.36 instead of 1.87 ms
  // per 256-frame job, and the in-phase pattern is stable once entered).  One after the other, lane B's upload runs under lane A's
  // kernels whatever the kernels' durations are.
  hipEvent_t last_upload = nullptr;
};

namespace uvo {

// ---- extractor_geom.cpp ----
void build_ctor_tables(uvo_extractor* h);
int build_geom(const uvo_extractor* h, int width, int height, Geom& g, std::vector<CellDesc>& cells, std::vector<int32_t>* cell_flag = nullptr);
void build_resize_tables(const Geom& g, std::vector<ResizeCol>& ctab, std::vector<ResizeRow>& rtab, int* fast_ok);
void size_capacities(uvo_extractor* h, const Geom& g);
// which capacity of the handle a geometry exceeds, in the order set_geometry() holds it against them
enum { GEOM_CAP_NONE = 0, GEOM_CAP_BLOCKS, GEOM_CAP_FAST, GEOM_CAP_XTAB, GEOM_CAP_YTAB, GEOM_CAP_OCT_TAB };
int exceeded_capacity(const uvo_extractor* h, const Geom& g, size_t n_ctab, size_t n_rtab);
int oct_table_entries(const Geom& g);  // 2-byte entries of the quad-tree's path tables of geometry g
// corner-list scratch of geometry g, for the worst batch size up to max_batch (the segment height depends on the batch: fast_rows_per_seg)
// with `slack` extra work items per frame: *entries for the regions, *counts for their fill counts
void corner_scratch_size(const Geom& g, int max_batch, int slack, size_t* entries, size_t* counts);
bool tile_group_from_spec(const std::vector<uint32_t>& spec, size_t k, int nlevels, TileGroup& G);  // false: the group starts above the last level
std::vector<uint32_t> default_tile_spec(const Geom& g);
void build_patch_masks(const int* umax, std::vector<uint32_t>& patch);

// ---- extractor.cpp ----
int sync_all_lanes(uvo_extractor* h);
hipError_t wait_stream(hipStream_t s, bool spin);
int set_geometry(uvo_extractor* h, int width, int height);
// The lane the next batch runs on.  With pipeline depth > 1 consecutive batches alternate; whoever stages inputs for a batch
// (uploads, CLAHE) must enqueue them on this lane's stream, and read results back from it.
inline int next_lane(const uvo_extractor* h) { return h->nlanes > 1 ? (h->cur + 1) % h->nlanes : h->cur; }
// The launch sequence of one batch (every pointer of b a device address): everything on lane `li`'s stream, nothing synchronous.
// Makes `li` the current lane.
int run_batch_device(uvo_extractor* h, int li, const Batch& b);

// At least n elements in *p, a buffer of owner m (the handle's, or one of its lanes') that is allocated on first use or grown on
// demand; contents are undefined after growth.  EVERY lane is drained before the old buffer is freed: whatever lane the caller is
// about to use, another one's batch may still read it.
template <class T>
int grow(uvo_extractor* h, DevMem& m, T** p, size_t n, bool pinned = false) {
  if (*p && m.bytes_of(*p) >= n * sizeof(T)) return UVO_OK;
  RC(sync_all_lanes(h));
  m.release(*p);
  *p = nullptr;
  return m.alloc(p, n, pinned);
}

}  // namespace uvo

extern "C" {
// the extractor's hooks (extractor.cpp, extractor_host.cpp)
hipStream_t uvo_extractor_stream_internal(uvo_extractor* h);  // the current lane's stream
int uvo_extractor_device_internal(uvo_extractor* h);
int uvo_extractor_next_lane_internal(const uvo_extractor* h);
void uvo_extractor_add_follower_internal(uvo_extractor* h, uvo_matcher* m);
void uvo_extractor_drop_follower_internal(uvo_extractor* h, uvo_matcher* m);
const uint8_t* uvo_extractor_clahe_internal(uvo_extractor* h, int* width, int* height);  // the last uvo_clahe() result in HBM
int uvo_extract_batch_submit_internal(uvo_extractor* h, int batch, int n_download, const uint8_t* imgs, int width, int height, ptrdiff_t stride,
                                      ptrdiff_t frame_stride, uvo_keypoint* out_kp, uint8_t* out_desc, int cap, int32_t* n_out, int* ticket,
                                      hipEvent_t after_kernels, const uint8_t** d_desc, const int32_t** d_n);
int uvo_extract_batch_done_internal(uvo_extractor* h, int ticket);
// the matcher's hooks (matcher.cpp)
hipStream_t uvo_matcher_stream_internal(uvo_matcher* m);
void uvo_matcher_follow_internal(uvo_matcher* m, hipStream_t s);
void uvo_matcher_orphaned_internal(uvo_matcher* m);
}
