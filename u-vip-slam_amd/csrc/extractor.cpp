// The extractor handle: device scratch and its owner, pipeline lanes, per-resolution tables on the device, the launch sequence of a
// batch, and the C-ABI entry points of include/uvo/uvo.h that work on device memory or on the handle itself (the host-buffer forms
// that replace USLAM::ORBextractor::operator() are in extractor_host.cpp, the tables' arithmetic in extractor_geom.cpp).
// No CPU fallback: every entry point needs a usable HIP device.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <vector>

#include "extractor_priv.hpp"
#include "fast_geom.hpp"

namespace uvo {

static thread_local char g_err[512] = "";
const char* hip_err_set(hipError_t e, const char* what) {
  snprintf(g_err, sizeof(g_err), "HIP error %d (%s) in %s", (int)e, hipGetErrorString(e), what);
  return g_err;
}
int fail(int code, const char* msg) {
  snprintf(g_err, sizeof(g_err), "%s", msg);
  return code;
}

static const int8_t kPattern[1024] = {
#include "rbrief_pattern.inc"
};

// Waits for a stream.  spin: the latency path -- hipStreamSynchronize gives up its busy wait after a few microseconds and sleeps on an
// interrupt, whose wake-up costs more than a whole stage of a single frame's chain; polling the stream's state keeps the host on the
// spot for the ~100 us a frame takes (bounded: after kSpinWaitUs the blocking wait takes over).
constexpr int kSpinWaitUs = 400;
hipError_t wait_stream(hipStream_t s, bool spin) {
  if (spin) {
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
      const hipError_t e = hipStreamQuery(s);
      if (e != hipErrorNotReady) return e;
      if (std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count() > kSpinWaitUs) break;
    }
  }
  return hipStreamSynchronize(s);
}

// (Re)starts lane li's per-level FAST mode.  Adaptive and two-pass start threshold-adaptive (stream at fastTh, sparse literal-7 pass);
// single-pass streams at min(fastTh, 7) and votes.  With fastTh <= 7 the second call of src/ORBextractor.cc:797 can find nothing the
// first did not, so there is only one form.
static int set_lane_fast_mode(uvo_extractor* h, int li) {
  int32_t t[kMaxLevels];
  const int th = h->cfg.fast_th;
  for (int l = 0; l < kMaxLevels; ++l) t[l] = (th > 7 && h->fast_mode != UVO_FAST_MODE_SINGLE_PASS) ? th : (th < 7 ? th : 7);
  UVO_HIP_CHECK(hipMemcpy(h->lane[li].d.tpass, t, sizeof(t), hipMemcpyHostToDevice));
  return UVO_OK;
}

static void free_tile_groups(uvo_extractor* h, std::vector<TileGroup>& groups) {
  for (auto& G : groups) h->mem.release(G.d_plan);
  groups.clear();
}

// Compiles the plans of one set of level groups (a tile spec: {first level, tx, ty, threads} each, ascending) for geometry g, whose resize
// tables are ctab / rtab / resize_fast, into `out` (plans uploaded; h->tile_groups is not touched).  A set that cannot be built (a level
// outside the 12-byte tap window, a tile larger than the LDS) stays empty: the batch then takes the per-level launches.  An error leaves
// `out` empty and nothing allocated.
static int compile_tile_groups(uvo_extractor* h, const Geom& g, const int* resize_fast, const std::vector<ResizeCol>& ctab, const std::vector<ResizeRow>& rtab,
                               std::vector<TileGroup>& out) {
  out.clear();
  const std::vector<uint32_t> spec = h->tile_spec.empty() ? default_tile_spec(g) : h->tile_spec;
  if (spec.empty() || g.nlevels < 2) return UVO_OK;
  PyrTileDims dims[kMaxLevels];
  const ResizeCol* cp[kMaxLevels] = {nullptr};
  const ResizeRow* rp[kMaxLevels] = {nullptr};
  for (int l = 0; l < g.nlevels; ++l) {
    dims[l] = PyrTileDims{g.lv[l].w, g.lv[l].h, g.lv[l].pitch};
    if (l > 0) {
      if (!resize_fast[l]) return UVO_OK;
      cp[l] = ctab.data() + g.lv[l].xtab_off, rp[l] = rtab.data() + g.lv[l].ytab_off;
    }
  }
  for (size_t k = 0; k < spec.size(); ++k) {
    TileGroup G;
    if (!tile_group_from_spec(spec, k, g.nlevels, G)) break;
    PyrTilePlan P;
    if (G.first < 1 || G.last < G.first || (k == 0 && G.first != 1) || !pyr_tile_plan_build(dims, g.nlevels, G.first, G.last, cp, rp, 4, G.tx, G.ty, h->pyr_tiles_max_lds, P)) {
      free_tile_groups(h, out);
      return UVO_OK;
    }
    G.lds = P.lds_bytes;
    int rc = h->mem.alloc(&G.d_plan, P.lv.size());
    out.push_back(G);  // (owned from here on: the error path frees the whole set)
    if (rc == UVO_OK && hipMemcpy(G.d_plan, P.lv.data(), P.lv.size() * sizeof(PyrTileLevel), hipMemcpyHostToDevice) != hipSuccess) rc = fail(UVO_E_HIP, "plan upload failed");
    if (rc != UVO_OK) {
      free_tile_groups(h, out);
      return rc;
    }
  }
  return UVO_OK;
}

// The handle's set for its current geometry, compiled again (UVO_TUNE_PYR_TILE_GROUP changed the spec).  Called with every lane idle.
static int build_tile_groups(uvo_extractor* h) {
  std::vector<TileGroup> groups;
  const int rc = compile_tile_groups(h, h->geom, h->resize_fast, h->ctab_host, h->rtab_host, groups);
  free_tile_groups(h, h->tile_groups);  // (an error leaves the empty set: the per-level launches)
  h->tile_groups.swap(groups);
  return rc;
}

// All or nothing: everything a new resolution needs is computed into locals and held against every capacity first -- a refused call leaves
// the handle, its host tables (resize_fast among them) and its device tables exactly as they were.  Only then the lanes are drained, the
// tile plans compiled into buffers of their own and the device tables overwritten; a HIP error in that last part (the old tables may be
// half overwritten) drops the geometry, so that the next call uploads everything again whatever its size.
int set_geometry(uvo_extractor* h, int width, int height) {
  if (h->have_geom && h->geom.width == width && h->geom.height == height) return UVO_OK;
  Geom g;
  std::vector<CellDesc> cells;
  std::vector<int32_t> cell_flag;
  int rc = build_geom(h, width, height, g, cells, &cell_flag);
  if (rc) return rc;
  std::vector<ResizeCol> ctab;
  std::vector<ResizeRow> rtab;
  int resize_fast[kMaxLevels] = {0};
  build_resize_tables(g, ctab, rtab, resize_fast);
  if (exceeded_capacity(h, g, ctab.size(), rtab.size()) != GEOM_CAP_NONE) return fail(UVO_E_BADARG, "image larger than the handle was sized for");
  std::vector<uint16_t> oct_tab((size_t)oct_table_entries(g), 0);
  octree_fill_path_tables(g, oct_tab.data());
  // ---- the last check is behind us.  In-flight work may still read the old tables
  {
    int rcs = sync_all_lanes(h);
    if (rcs) return rcs;
  }
  std::vector<TileGroup> groups;  // in buffers of their own: a failure here has touched nothing the old geometry reads
  if ((rc = compile_tile_groups(h, g, resize_fast, ctab, rtab, groups)) != UVO_OK) return rc;
  hipError_t e = hipMemcpy(h->d_oct_tab, oct_tab.data(), oct_tab.size() * sizeof(uint16_t), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(h->d_lv, g.lv, sizeof(LevelGeom) * g.nlevels, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(h->d_cells, cells.data(), sizeof(CellDesc) * cells.size(), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(h->d_cell_flag, cell_flag.data(), sizeof(int32_t) * cell_flag.size(), hipMemcpyHostToDevice);
  if (e == hipSuccess && !ctab.empty()) e = hipMemcpy(h->d_ctab, ctab.data(), ctab.size() * sizeof(ResizeCol), hipMemcpyHostToDevice);
  if (e == hipSuccess && !rtab.empty()) e = hipMemcpy(h->d_rtab, rtab.data(), rtab.size() * sizeof(ResizeRow), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    free_tile_groups(h, groups);
    h->have_geom = false;  // the device tables are neither the old geometry's nor the new one's
    hip_err_set(e, "set_geometry table upload");
    return UVO_E_HIP;
  }
  free_tile_groups(h, h->tile_groups);
  h->tile_groups.swap(groups);
  h->ctab_host.swap(ctab), h->rtab_host.swap(rtab);
  std::copy(resize_fast, resize_fast + kMaxLevels, h->resize_fast);
  h->geom = g;
  h->cells.swap(cells);
  h->cell_flag.swap(cell_flag);
  h->have_geom = true;
  return UVO_OK;
}

struct ProfScope : Profiler::Scope {
  ProfScope(uvo_extractor* h, const char* name) : Profiler::Scope(&h->prof, name, h->lane[h->cur].stream) {}
};

int run_batch_device(uvo_extractor* h, int li, const Batch& b) {
  if (!h || !b.imgs || !b.out_kp || !b.out_desc || !b.n_out) return fail(UVO_E_BADARG, "null pointer");
  const int batch = b.n, width = b.width, height = b.height, cap = b.cap, full_detect = b.full_detect;
  const ptrdiff_t stride = b.stride, frame_stride = b.frame_stride;
  const uint8_t* const d_imgs = b.imgs;
  if (batch < 1 || batch > h->cfg.max_batch) return fail(UVO_E_BADARG, "batch outside 1..max_batch");
  if (width < 1 || height < 1 || stride < width || cap < 1) return fail(UVO_E_BADARG, "bad image size / stride / cap");
  if (!full_detect && (!b.grid || !b.nfn || b.min_px_dist < 1 || b.grid_rows < 1 || b.grid_cols < 1))
    return fail(UVO_E_BADARG, "top-up mode needs grid2d, num_feats_needed and min_px_dist >= 1");
  // the occupancy filter indexes grid_2d(int(y / d), int(x / d)) for every pixel position (src/ORBextractor.cc:884-891; the call
  // site allocates rows / d + 2 by cols / d + 2, src/Tracking.cc:930-934): a smaller grid would be indexed out of bounds
  if (!full_detect && (b.grid_rows <= (height - 1) / b.min_px_dist || b.grid_cols <= (width - 1) / b.min_px_dist))
    return fail(UVO_E_BADARG, "grid2d smaller than ceil(image / min_px_dist)");
  UVO_HIP_CHECK(hipSetDevice(h->device));
  int rc = set_geometry(h, width, height);
  if (rc) return rc;
  if ((rc = prepare_octree(h->geom)) != UVO_OK) return rc;  // nothing below this line fails once the first kernel is in the stream
  h->cur = li;
  Lane& L = h->lane[li];
  hipStream_t s = L.stream;
  {  // attached matchers work behind THIS batch (and only this one: the ordering contract of uvo_matcher_attach_extractor)
    std::lock_guard<std::mutex> lk(h->followers_mu);
    for (uvo_matcher* m : h->followers) uvo_matcher_follow_internal(m, s);
  }
  h->last_batch = batch;
  const Geom& g = h->geom;
  hipEvent_t& done = L.done[L.n_enqueued & 1];  // recorded behind the lane's last but one batch
  if (done) UVO_HIP_CHECK(hipEventSynchronize(done));
  else UVO_HIP_CHECK(hipEventCreateWithFlags(&done, hipEventDisableTiming));
  // Level 0 in place: every reader of level 0 (the FAST kernels, the blur, the orientation patch, the resize to level 1) takes the caller's
  // image itself -- the blur reflects its 3-pixel border on the fly -- and cv::copyMakeBorder of :996 (182 MB per 257 frames at 640 x 512)
  // is never materialised.  Needs dword-aligned rows of a width that is a multiple of 4 (a lane's four pixels are then wholly inside the
  // image or wholly border), the launch chain, and no caller keypoints (their orientation patch may reach into the border).  The image
  // must stay unchanged until the batch is complete (it always had to stay valid that long).
  const bool have_in = b.in_kp && b.n_in;
  const bool inplace = h->level0_inplace && width % 4 == 0 && stride % 4 == 0 && frame_stride % 4 == 0 &&
                       (uintptr_t)d_imgs % 4 == 0 && !have_in && width >= 64 && height >= 64 &&
                       // the kernels address in-place rows as __umul24(row, pitch) + a 32-bit lane offset: a wider stride (an ROI of a large
                       // mosaic) takes the padded copy instead
                       stride <= (1 << 20) && (int64_t)(height + 2 * kPad) * stride < (int64_t)1 << 31;
  Level0View l0{nullptr, 0, 0, 0};
  if (inplace) l0 = Level0View{d_imgs - (int64_t)kPad * stride - kPad, (int64_t)frame_stride, (int)stride, 0};
  L.l0_src = inplace ? d_imgs : nullptr, L.l0_stride = stride, L.l0_frame_stride = frame_stride;
  L.ring_used = h->pyr_ring;
  const Level0View no_l0{nullptr, 0, 0, 0};
  {
    // ComputePyramid (src/ORBextractor.cc:963-1004): a launch per group of levels (k_pyr_tiles), or one per level
    if (!inplace) {
      ProfScope p(h, "k_pad_level0");
      launch_pad_level0(s, d_imgs, width, height, stride, frame_stride, L.d.pyr, g.pyr_block, g.lv[0], batch);
    }
    const bool tiles = h->pyr_ring == 4 && !h->tile_groups.empty() && (h->pyr_form == UVO_PYR_FORM_TILES || (h->pyr_form == UVO_PYR_FORM_AUTO && batch <= kTilePyramidFrames));
    if (tiles) {
      for (const TileGroup& G : h->tile_groups) {
        ProfScope p(h, "k_pyr_tiles");
        launch_pyr_tiles(s, L.d.pyr, g.pyr_block, G.d_plan, g, h->d_ctab, h->d_rtab, l0, G.first, G.last, G.tx * G.ty, G.lds, G.threads, G.rows, batch);
      }
    } else {
      // large batches walk row bands (k_resize_level_rows: a source row is filtered once), level by level where the launch is large enough
      const bool rows = h->pyr_form == UVO_PYR_FORM_ROWS || (h->pyr_form == UVO_PYR_FORM_AUTO && batch > kTilePyramidFrames);
      for (int l = 1; l < g.nlevels; ++l) {
        const Level0View v = l == 1 ? l0 : no_l0;
        const ResizeCol* ct = h->d_ctab + g.lv[l].xtab_off;
        const ResizeRow* rt = h->d_rtab + g.lv[l].ytab_off;
        if (rows && resize_level_rows_applies(g.lv[l - 1], g.lv[l], h->resize_fast[l], batch, v, h->pyr_ring, g.pyr_block, h->pyr_form == UVO_PYR_FORM_ROWS)) {
          ProfScope p(h, "k_resize_level_rows");
          launch_resize_level_rows(s, L.d.pyr, g.pyr_block, g.lv[l - 1], g.lv[l], ct, rt, batch, v, h->pyr_ring);
        } else {
          ProfScope p(h, "k_resize_level");
          launch_resize_level(s, L.d.pyr, g.pyr_block, g.lv[l - 1], g.lv[l], ct, rt, h->resize_fast[l], batch, v, h->pyr_ring);
        }
      }
    }
  }
  const bool fused_tree = h->fuse_blur_tree && octree_gauss_applies(h->oct, g, batch);
  // A frame or two (the per-frame latency path, src/Tracking.cc:946): every stage is a chain of dependent phases on a nearly empty chip,
  // so the number of stages is what counts -- a FullDetect call has no k_assemble launch (k_describe finds its slots itself).  (One FAST
  // pass at 7 with the vote in the quad-tree instead of the sparse second launch: the pass takes 7.7 us longer, the launch it saves 8.)
  const bool few = batch <= kFewFrames && h->few_frames_shape;
  const int4 gtaps = make_int4(h->gtaps[0], h->gtaps[1], h->gtaps[2], h->gtaps[3]);
  {  // the per-cell threshold vote + candidate emit run inside k_octree
    ProfScope p(h, "k_fast_score");
    launch_fast_score(s, L.d, g, h->cfg.fast_th, batch, l0);
  }
  if (h->cfg.fast_th > 7 && h->fast_mode != UVO_FAST_MODE_SINGLE_PASS) {
    // second call of src/ORBextractor.cc:797 for the cells of threshold-adaptive levels that the pass at fastTh left empty (nearly all
    // wavefronts find nothing to do on textured frames).  With the mode pinned to one pass no level can be adaptive: not launched.
    ProfScope p(h, "k_fast_cells");
    launch_fast_cells(s, L.d, g, h->d_cells, h->d_cell_flag, batch, l0);
  }
  if (fused_tree) {
    // the quad-tree (a chain of dependent phases per (frame, level)) and the blur (a streaming kernel) read nothing of each other:
    // one grid, the quad-tree problems first, and the blur fills the issue slots they leave idle
    ProfScope p(h, "k_octree_gauss");
    launch_octree_gauss(s, h->d_lv, g, L.d, gtaps, h->blur_rounding, batch, l0, h->d_oct_tab);
  } else {
    {
      ProfScope p(h, "k_gauss7");
      launch_gauss7(s, L.d.pyr, L.d.blur, g.pyr_block, h->d_lv, g, gtaps, batch, h->blur_rounding, l0);
    }
    {
      ProfScope p(h, "k_octree");
      rc = launch_octree(s, h->oct, h->d_lv, g, L.d, batch, h->d_oct_tab);
      if (rc) return rc;
    }
  }
  if (have_in) {
    // A caller keypoint may lie 2 pixels from the border of level 0 (validate(), extractor_host.cpp) and its steered pattern reaches 18:
    // the blurred plane gets the un-blurred pad beyond the blur's ring, as the reference's in-place blur leaves it.  (Level 0 is the
    // padded plane here: a call with caller keypoints never reads the image in place.)
    ProfScope p(h, "k_blur_pad_level0");
    launch_blur_pad_level0(s, L.d.pyr, L.d.blur, g.pyr_block, g.lv[0], batch);
  }
  const bool direct = few && full_detect && !have_in;
  const FastAdapt fa{L.d.fcount, L.d.tpass, L.d.fstat, h->fast_mode == UVO_FAST_MODE_ADAPTIVE ? 1 : 0, h->cfg.fast_th};
  if (!direct) {
    ProfScope p(h, "k_assemble");
    launch_assemble(s, h->d_lv, g, fa, L.d, b.n_in, h->cfg.max_input_keypoints, b.grid, b.grid_rows, b.grid_cols, b.min_px_dist, full_detect, b.nfn, batch);
  }
  {
    ProfScope p(h, "k_describe");
    if (direct) launch_describe_direct(s, h->d_lv, g, L.d, fa, h->d_pattern, h->d_patch, b.out_kp, b.out_desc, cap, b.n_out, batch, l0);
    else launch_describe(s, h->d_lv, g, L.d, b.in_kp, h->cfg.max_input_keypoints, h->d_pattern, h->d_patch, b.out_kp, b.out_desc, cap, b.n_out, batch, l0);
  }
  UVO_HIP_CHECK(hipGetLastError());
  UVO_HIP_CHECK(hipEventRecord(done, s));
  L.n_enqueued++;
  return UVO_OK;
}

// Brings lane L up: its stream, then its scratch.  An error leaves L half built -- alloc_lane() takes it down again.
static int fill_lane(uvo_extractor* h, int li) {
  Lane& L = h->lane[li];
  LaneScratch& d = L.d;
  const size_t B = (size_t)h->cfg.max_batch;
  const hipError_t e = hipStreamCreateWithFlags(&L.stream, hipStreamNonBlocking);
  if (e != hipSuccess) {
    L.stream = nullptr;
    hip_err_set(e, "hipStreamCreate");
    return UVO_E_HIP;
  }
  RC(L.mem.alloc(&d.pyr, B * h->cap_pyr_block));
  RC(L.mem.alloc(&d.blur, B * h->cap_pyr_block + 256));  // + slack: k_describe reads whole dwords up to 3 bytes past a row end
  RC(L.mem.alloc(&d.cand_xy, B * h->cap_cand_block));
  RC(L.mem.alloc(&d.cand_sc, B * h->cap_cand_block));
  RC(L.mem.alloc(&d.cand_lo, B * h->cap_cand_block));
  RC(L.mem.alloc(&d.cursor, B * kMaxLevels * 2));
  RC(L.mem.alloc(&d.pstate, B * h->cap_cand_block));
  RC(L.mem.alloc(&d.sel_xy, B * h->cap_sel_block));
  RC(L.mem.alloc(&d.sel_sc, B * h->cap_sel_block));
  RC(L.mem.alloc(&d.cand_count, B * kMaxLevels));
  RC(L.mem.alloc(&d.sel_count, B * kMaxLevels));
  RC(L.mem.alloc(&d.n_final, B));
  RC(L.mem.alloc(&d.flist, B * h->cap_flist));
  RC(L.mem.alloc(&d.cor, h->cap_cor));
  RC(L.mem.alloc(&d.cor_n, h->cap_cor_n));
  RC(L.mem.alloc(&d.cell_hi, h->cap_flags));
  RC(L.mem.alloc(&d.tpass, (size_t)kMaxLevels));
  // the last batch's fall-back cells per level, then the length of cell_list; per (frame, level) counts of the batch in flight
  RC(L.mem.alloc(&d.fstat, (size_t)kMaxLevels + 4));
  RC(L.mem.alloc(&d.fcount, B * kMaxLevels));
  RC(L.mem.alloc(&d.cell_list, B * (size_t)h->cap_cells));
  RC(set_lane_fast_mode(h, li));
  if (hipMemset(d.fstat, 0, (kMaxLevels + 4) * sizeof(int32_t)) != hipSuccess) return fail(UVO_E_HIP, "hipMemset failed");
  // the cell flags and the fill cursors are zero between calls: k_fast_score sets / advances them, k_octree clears what it has consumed
  if (hipMemset(d.cell_hi, 0, h->cap_flags) != hipSuccess || hipMemset(d.cursor, 0, B * kMaxLevels * 2 * sizeof(int32_t)) != hipSuccess)
    return fail(UVO_E_HIP, "hipMemset failed");
  return UVO_OK;
}

// Takes a lane down (whole or half built): afterwards it owns nothing and has no stream.
static void free_lane(Lane& L) {
  if (L.stream) (void)hipStreamSynchronize(L.stream);
  L.mem.release_all();
  if (L.a_uploaded) (void)hipEventDestroy(L.a_uploaded);
  for (hipEvent_t& e : L.done)
    if (e) (void)hipEventDestroy(e);
  if (L.stream) (void)hipStreamDestroy(L.stream);
  L = Lane();
}

// All or nothing: a lane with a stream is whole, and a bring-up that failed leaves none behind, so that the next attempt starts from scratch.
static int alloc_lane(uvo_extractor* h, int li) {
  if (h->lane[li].stream) return UVO_OK;
  const int rc = fill_lane(h, li);
  if (rc != UVO_OK) free_lane(h->lane[li]);
  return rc;
}

int sync_all_lanes(uvo_extractor* h) {
  for (int i = 0; i < kMaxLanes; ++i)
    if (h->lane[i].stream) UVO_HIP_CHECK(hipStreamSynchronize(h->lane[i].stream));
  return UVO_OK;
}

}  // namespace uvo

using namespace uvo;

extern "C" {

const char* uvo_last_error(void) { return uvo::g_err; }

int uvo_device_info(int device, char* dst, int cap) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(UVO_E_NODEVICE, "no HIP device");
  if (device < 0 || device >= n) return fail(UVO_E_BADARG, "device ordinal out of range");
  hipDeviceProp_t p;
  UVO_HIP_CHECK(hipGetDeviceProperties(&p, device));
  snprintf(dst, cap, "uvo 0.1 %s %s CUs=%d", p.gcnArchName, p.name, p.multiProcessorCount);
  return UVO_OK;
}

int uvo_extractor_create(const uvo_extractor_cfg* cfg, uvo_extractor** out) {
  if (!cfg || !out) return fail(UVO_E_BADARG, "null pointer");
  *out = nullptr;
  if (cfg->nfeatures < 1 || cfg->nlevels < 1 || cfg->nlevels > kMaxLevels || !(cfg->scale_factor > 1.0f) || cfg->fast_th < 0 ||
      cfg->max_width < 1 || cfg->max_height < 1 || cfg->max_batch < 1 || cfg->max_input_keypoints < 0)
    return fail(UVO_E_BADARG, "bad extractor configuration");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(UVO_E_NODEVICE, "no HIP device available (no CPU fallback exists)");
  if (cfg->device < 0 || cfg->device >= ndev) return fail(UVO_E_BADARG, "device ordinal out of range");
  uvo_extractor* h = new uvo_extractor();
  h->cfg = *cfg;
  h->cfg.fast_th = std::min(cfg->fast_th, 255);  // cv::FAST clamps its threshold to 0 .. 255 (no byte differs from another by more)
  h->device = cfg->device;
  build_ctor_tables(h);
  Geom g;
  std::vector<CellDesc> cells;
  int rc = build_geom(h, cfg->max_width, cfg->max_height, g, cells);
  if (rc) {
    delete h;
    return rc;
  }
  size_capacities(h, g);
  const size_t B = (size_t)cfg->max_batch;
  hipError_t e = hipSetDevice(h->device);
  if (e != hipSuccess) {
    hip_err_set(e, "hipSetDevice");
    delete h;
    return UVO_E_NODEVICE;
  }
#define A(call)                    \
  if ((rc = (call)) != UVO_OK) {   \
    uvo_extractor_destroy(h);      \
    return rc;                     \
  }
  A(prepare_pyr_tiles(&h->pyr_tiles_max_lds));
  A(alloc_lane(h, 0));
  A(h->mem.alloc(&h->d_lv, (size_t)kMaxLevels));
  A(h->mem.alloc(&h->d_cells, (size_t)h->cap_cells));
  A(h->mem.alloc(&h->d_cell_flag, h->cap_flags / B + 64));
  A(h->mem.alloc(&h->d_oct_tab, (size_t)h->cap_oct_tab));
  A(h->mem.alloc(&h->d_ctab, (size_t)h->cap_xtab));
  A(h->mem.alloc(&h->d_rtab, (size_t)h->cap_ytab));
  A(h->mem.alloc(&h->d_pattern, (size_t)1024));
  A(h->mem.alloc(&h->d_patch, (size_t)256));
  // staging for host-buffer calls
  A(h->mem.alloc(&h->d_imgs, B * (size_t)cfg->max_width * cfg->max_height));
  A(h->mem.alloc(&h->d_out_kp, B * h->cap_flist));
  A(h->mem.alloc(&h->d_out_desc, B * h->cap_flist * 32));
  A(h->mem.alloc(&h->d_n_out, B));
  A(h->mem.alloc(&h->d_in_kp, B * std::max(cfg->max_input_keypoints, 1)));
  A(h->mem.alloc(&h->d_n_in, B));
  A(h->mem.alloc(&h->d_nfn, B));
#undef A
  std::vector<uint32_t> patch;
  build_patch_masks(h->umax, patch);
  std::vector<float> patf(1024);
  for (int i = 0; i < 1024; ++i) patf[i] = (float)kPattern[i];
  if (hipMemcpy(h->d_pattern, patf.data(), 4096, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(h->d_patch, patch.data(), 1024, hipMemcpyHostToDevice) != hipSuccess) {
    uvo_extractor_destroy(h);
    return fail(UVO_E_HIP, "table upload failed");
  }
  *out = h;
  return UVO_OK;
}

void uvo_extractor_destroy(uvo_extractor* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  for (int i = 0; i < kMaxLanes; ++i)
    if (h->lane[i].stream) (void)hipStreamSynchronize(h->lane[i].stream);
  {
    std::lock_guard<std::mutex> lk(h->followers_mu);
    for (uvo_matcher* m : h->followers) uvo_matcher_orphaned_internal(m);  // their work in these streams is done; they outlive the streams
    h->followers.clear();
  }
  h->prof.clear();
  for (Lane& L : h->lane) free_lane(L);
  h->mem.release_all();
  delete h;
}

int uvo_extractor_levels(const uvo_extractor* h) { return h ? h->cfg.nlevels : UVO_E_BADARG; }
float uvo_extractor_scale_factor(const uvo_extractor* h) { return h ? (float)(double)h->cfg.scale_factor : 0.f; }

int uvo_extractor_tables(const uvo_extractor* h, float* scale, float* inv_scale, int32_t* quota, int32_t* umax16) {
  if (!h) return fail(UVO_E_BADARG, "null handle");
  for (int i = 0; i < h->cfg.nlevels; ++i) {
    if (scale) scale[i] = h->scale[i];
    if (inv_scale) inv_scale[i] = h->inv_scale[i];
    if (quota) quota[i] = h->quota[i];
  }
  if (umax16)
    for (int i = 0; i < 16; ++i) umax16[i] = h->umax[i];
  return UVO_OK;
}

int uvo_extract_batch_device(uvo_extractor* h, int batch, const uint8_t* d_imgs, int width, int height, ptrdiff_t stride,
                             ptrdiff_t frame_stride, const uvo_keypoint* d_in_kp, const int32_t* d_n_in, int32_t* d_grid2d, int grid_rows,
                             int grid_cols, int min_px_dist, int full_detect, const int32_t* d_num_feats_needed, uvo_keypoint* d_out_kp,
                             uint8_t* d_out_desc, int cap, int32_t* d_n_out) {
  if (!h) return fail(UVO_E_BADARG, "null handle");
  return run_batch_device(h, next_lane(h), Batch{batch, d_imgs, width, height, stride, frame_stride, d_in_kp, d_n_in, d_grid2d, grid_rows, grid_cols, min_px_dist,
                                                 full_detect, d_num_feats_needed, d_out_kp, d_out_desc, cap, d_n_out});
}

// cv::CLAHE::apply parameters (OpenCV 3.4 clahe.cpp): tile size on the extended image, clip limit in pixels, LUT scale
static int clahe_setup(uvo_extractor* h, int batch, int width, int height, double clip_limit, int tiles_x, int tiles_y, int* tile_w, int* tile_h,
                       int* clip, float* lut_scale) {
  if (batch < 1 || batch > h->cfg.max_batch) return fail(UVO_E_BADARG, "batch outside 1..max_batch");
  if (width < 1 || height < 1 || tiles_x < 1 || tiles_y < 1 || tiles_x > width || tiles_y > height) return fail(UVO_E_BADARG, "bad image / tile grid size");
  int ew = width, eh = height;
  if (!(width % tiles_x == 0 && height % tiles_y == 0)) {  // copyMakeBorder(..., 0, tilesY - rows % tilesY, 0, tilesX - cols % tilesX, REFLECT_101)
    ew = width + (tiles_x - width % tiles_x);
    eh = height + (tiles_y - height % tiles_y);
  }
  if (ew - width >= width || eh - height >= height) return fail(UVO_E_BADARG, "tile grid too coarse for REFLECT_101 extension");
  *tile_w = ew / tiles_x, *tile_h = eh / tiles_y;
  const int tileSizeTotal = *tile_w * *tile_h;
  *lut_scale = static_cast<float>(256 - 1) / tileSizeTotal;
  *clip = 0;
  if (clip_limit > 0.0) {
    *clip = static_cast<int>(clip_limit * tileSizeTotal / 256);
    *clip = std::max(*clip, 1);
  }
  return grow(h, h->mem, &h->d_clahe_lut, (size_t)h->cfg.max_batch * tiles_x * tiles_y * 256);
}

int uvo_clahe_batch_device(uvo_extractor* h, int batch, const uint8_t* d_imgs, int width, int height, ptrdiff_t stride, ptrdiff_t frame_stride,
                           double clip_limit, int tiles_x, int tiles_y, uint8_t* d_dst, ptrdiff_t dst_stride, ptrdiff_t dst_frame_stride) {
  if (!h || !d_imgs || !d_dst) return fail(UVO_E_BADARG, "null pointer");
  if (stride < width || dst_stride < width) return fail(UVO_E_BADARG, "stride smaller than the row");
  UVO_HIP_CHECK(hipSetDevice(h->device));
  int tw, th, clip;
  float scale;
  int rc = clahe_setup(h, batch, width, height, clip_limit, tiles_x, tiles_y, &tw, &th, &clip, &scale);
  if (rc) return rc;
  Lane& L = h->lane[next_lane(h)];  // the lane of the extraction that consumes d_dst (same stream: in order behind this kernel)
  {
    Profiler::Scope ps(&h->prof, "k_clahe", L.stream);
    launch_clahe(L.stream, d_imgs, width, height, stride, frame_stride, batch, tiles_x, tiles_y, tw, th, clip, scale, h->d_clahe_lut, d_dst, dst_stride,
                 dst_frame_stride);
  }
  UVO_HIP_CHECK(hipGetLastError());
  return UVO_OK;
}

int uvo_extractor_max_keypoints(const uvo_extractor* h) {
  if (!h) return fail(UVO_E_BADARG, "null handle");
  return h->cap_flist;
}

int uvo_extractor_synchronize(uvo_extractor* h) {
  if (!h) return fail(UVO_E_BADARG, "null handle");
  UVO_HIP_CHECK(hipSetDevice(h->device));
  if (h->spin_wait && h->last_batch > 0 && h->last_batch <= 16) {  // (behind a small batch the wait is short and its wake-up latency counts)
    for (int i = 0; i < kMaxLanes; ++i)
      if (h->lane[i].stream) UVO_HIP_CHECK(wait_stream(h->lane[i].stream, true));
    return UVO_OK;
  }
  return sync_all_lanes(h);
}

int uvo_extractor_tune(uvo_extractor* h, int knob, int value) {
  if (!h) return fail(UVO_E_BADARG, "null handle");
  switch (knob) {
    case UVO_TUNE_OCT_WIDE_MAX:
      if (value < 0) return fail(UVO_E_BADARG, "knob value must be >= 0");
      h->oct.wide_max_problems = value;
      return UVO_OK;
    case UVO_TUNE_FAST_MODE: {
      if (value != UVO_FAST_MODE_ADAPTIVE && value != UVO_FAST_MODE_TWO_PASS && value != UVO_FAST_MODE_SINGLE_PASS)
        return fail(UVO_E_BADARG, "UVO_TUNE_FAST_MODE takes UVO_FAST_MODE_ADAPTIVE / _TWO_PASS / _SINGLE_PASS");
      UVO_HIP_CHECK(hipSetDevice(h->device));
      int rc = sync_all_lanes(h);
      if (rc) return rc;
      h->fast_mode = value;
      for (int i = 0; i < kMaxLanes; ++i)
        if (h->lane[i].stream && (rc = set_lane_fast_mode(h, i)) != UVO_OK) return rc;
      return UVO_OK;
    }
    case UVO_TUNE_PYR_FORM:
      if (value < UVO_PYR_FORM_AUTO || value > UVO_PYR_FORM_ROWS) return fail(UVO_E_BADARG, "UVO_TUNE_PYR_FORM takes UVO_PYR_FORM_AUTO / _LEVELS / _TILES / _ROWS");
      h->pyr_form = value;
      return UVO_OK;
    case UVO_TUNE_PYR_TILE_GROUP: {
      // value = first level << 16 | tx << 8 | ty (| 1 << 24: 1024-thread workgroups, | 1 << 25: 1024 threads and single-row work items); first level 1
      // starts a new list, 0 returns to the defaults
      const int first = (value >> 16) & 0xff, tx = (value >> 8) & 0xff, ty = value & 0xff;
      if (value != 0 && (first < 1 || first >= kMaxLevels || tx < 1 || ty < 1 || (first > 1 && (h->tile_spec.empty() || first <= (int)((h->tile_spec.back() >> 16) & 0xff)))))
        return fail(UVO_E_BADARG, "UVO_TUNE_PYR_TILE_GROUP takes first << 16 | tx << 8 | ty with ascending first levels starting at 1, or 0");
      UVO_HIP_CHECK(hipSetDevice(h->device));
      int rc = sync_all_lanes(h);
      if (rc) return rc;
      if (value == 0 || first == 1) h->tile_spec.clear();
      if (value != 0) h->tile_spec.push_back((uint32_t)value);
      return h->have_geom ? build_tile_groups(h) : UVO_OK;
    }
    case UVO_TUNE_PYR_RING:
      if (value != 0 && value != 4 && value != 8 && value != 12) return fail(UVO_E_BADARG, "UVO_TUNE_PYR_RING takes 0, 4, 8 or 12");
      h->pyr_ring = value;
      return UVO_OK;
    case UVO_TUNE_LEVEL0_INPLACE:
      h->level0_inplace = value != 0;
      return UVO_OK;
    case UVO_TUNE_ZERO_COPY_OUT:
      h->zero_copy_out = value != 0;
      return UVO_OK;
    case UVO_TUNE_SPIN_WAIT:
      h->spin_wait = value != 0;
      return UVO_OK;
    case UVO_TUNE_FEW_FRAMES:
      h->few_frames_shape = value != 0;
      return UVO_OK;
    case UVO_TUNE_FUSE_BLUR_TREE:
      h->fuse_blur_tree = value != 0;
      return UVO_OK;
    case UVO_TUNE_BLUR_ROUNDING:
      if (value != UVO_BLUR_ROUNDING_SCALAR && value != UVO_BLUR_ROUNDING_SSE2) return fail(UVO_E_BADARG, "UVO_TUNE_BLUR_ROUNDING takes UVO_BLUR_ROUNDING_SCALAR / _SSE2");
      h->blur_rounding = value;
      return UVO_OK;
    default:
      return fail(UVO_E_BADARG, "unknown knob");
  }
}

int uvo_extractor_fast_state(uvo_extractor* h, int32_t* pass_threshold, int32_t* fallback_cells, int32_t* cells_per_frame) {
  if (!h) return fail(UVO_E_BADARG, "null handle");
  if (!h->have_geom) return fail(UVO_E_BADARG, "no batch has run yet");
  UVO_HIP_CHECK(hipSetDevice(h->device));
  Lane& L = h->lane[h->cur];
  UVO_HIP_CHECK(hipStreamSynchronize(L.stream));
  int32_t t[kMaxLevels], f[kMaxLevels];
  UVO_HIP_CHECK(hipMemcpy(t, L.d.tpass, sizeof(t), hipMemcpyDeviceToHost));
  UVO_HIP_CHECK(hipMemcpy(f, L.d.fstat, sizeof(f), hipMemcpyDeviceToHost));
  for (int l = 0; l < h->geom.nlevels; ++l) {
    if (pass_threshold) pass_threshold[l] = t[l];
    if (fallback_cells) fallback_cells[l] = f[l];
    if (cells_per_frame) cells_per_frame[l] = h->geom.lv[l].n_cells;
  }
  return UVO_OK;
}

int uvo_extractor_set_pipeline(uvo_extractor* h, int depth) {
  if (!h || depth < 1 || depth > kMaxLanes) return fail(UVO_E_BADARG, "pipeline depth must be 1..4");
  UVO_HIP_CHECK(hipSetDevice(h->device));
  int rc = sync_all_lanes(h);
  if (rc) return rc;
  for (int i = 1; i < depth; ++i) {
    rc = alloc_lane(h, i);
    if (rc) return rc;
  }
  h->nlanes = depth;
  if (depth == 1) h->cur = 0;
  return UVO_OK;
}

int uvo_extractor_level_dims(const uvo_extractor* h, int level, int* width, int* height) {
  if (!h || !h->have_geom || level < 0 || level >= h->geom.nlevels) return fail(UVO_E_BADARG, "no geometry / bad level");
  *width = h->geom.lv[level].w, *height = h->geom.lv[level].h;
  return UVO_OK;
}

int uvo_extractor_read_plane(uvo_extractor* h, int frame, int level, int which, uint8_t* dst) {
  if (!h || !h->have_geom || level < 0 || level >= h->geom.nlevels || frame < 0 || frame >= h->last_batch || !dst)
    return fail(UVO_E_BADARG, "bad plane request");
  UVO_HIP_CHECK(hipSetDevice(h->device));
  UVO_HIP_CHECK(hipStreamSynchronize(h->lane[h->cur].stream));
  const LevelGeom& L = h->geom.lv[level];
  Lane& LN = h->lane[h->cur];
  if (!which && level >= 1 && LN.ring_used > 0) {
    // the batch wrote the level's ROI and the few pixels around it that a stage reads: this test tap completes the 16-pixel border (the same
    // launch over the whole padded plane; its source -- the ROI of the level below, or the caller's image -- is still there)
    const Geom& g = h->geom;
    Level0View v{nullptr, 0, 0, 0};
    if (level == 1 && LN.l0_src) v = Level0View{LN.l0_src - (int64_t)kPad * LN.l0_stride - kPad, LN.l0_frame_stride, (int)LN.l0_stride, 0};
    launch_resize_level(LN.stream, LN.d.pyr, g.pyr_block, g.lv[level - 1], g.lv[level], h->d_ctab + g.lv[level].xtab_off, h->d_rtab + g.lv[level].ytab_off,
                        h->resize_fast[level], h->last_batch, v, 0);
    UVO_HIP_CHECK(hipStreamSynchronize(LN.stream));
  }
  if (!which && level == 0 && LN.l0_src) {
    // the batch read level 0 in place: this test tap makes the padded plane it never needed (the caller's images must still be there)
    launch_pad_level0(LN.stream, LN.l0_src, h->geom.width, h->geom.height, LN.l0_stride, LN.l0_frame_stride, LN.d.pyr, h->geom.pyr_block, h->geom.lv[0], h->last_batch);
    UVO_HIP_CHECK(hipStreamSynchronize(LN.stream));
  }
  const uint8_t* src = (which ? LN.d.blur : LN.d.pyr) + (size_t)frame * h->geom.pyr_block + L.plane_off;
  if (!which) {
    UVO_HIP_CHECK(hipMemcpy2D(dst, L.pw, src, L.pitch, L.pw, L.ph, hipMemcpyDeviceToHost));
    return UVO_OK;
  }
  // the blurred plane lives in HBM as 16 x 8-pixel tiles of 128 bytes (one cache line each: k_describe's windows touch a third of the
  // lines a row-major plane would cost them); pixel (x, y) = tile (y / 8, x / 16), byte (y % 8) * 16 + x % 16
  const size_t bytes = (size_t)L.pitch * ((L.ph + 7) & ~7);
  std::vector<uint8_t> tiled(bytes);
  UVO_HIP_CHECK(hipMemcpy(tiled.data(), src, bytes, hipMemcpyDeviceToHost));
  const int tiles_x = L.pitch >> 4;
  for (int y = 0; y < L.ph; ++y)
    for (int x = 0; x < L.pw; ++x) dst[(size_t)y * L.pw + x] = tiled[((size_t)(y >> 3) * tiles_x + (x >> 4)) * 128 + (y & 7) * 16 + (x & 15)];
  return UVO_OK;
}

int uvo_extractor_read_candidates(uvo_extractor* h, int frame, int level, int32_t* dst_xys, int cap, int* n) {
  if (!h || !h->have_geom || level < 0 || level >= h->geom.nlevels || frame < 0 || frame >= h->last_batch || !n)
    return fail(UVO_E_BADARG, "bad candidate request");
  UVO_HIP_CHECK(hipSetDevice(h->device));
  UVO_HIP_CHECK(hipStreamSynchronize(h->lane[h->cur].stream));
  const LevelGeom& L = h->geom.lv[level];
  int32_t cnt = 0;
  UVO_HIP_CHECK(hipMemcpy(&cnt, h->lane[h->cur].d.cand_count + (size_t)frame * h->geom.nlevels + level, 4, hipMemcpyDeviceToHost));
  *n = cnt;
  cnt = std::min(cnt, L.cand_cap);
  const int m = std::min(cnt, cap);
  if (m > 0 && dst_xys) {
    std::vector<uint32_t> xy(m), sc(m);
    const size_t off = (size_t)frame * h->geom.cand_block + L.cand_off;
    UVO_HIP_CHECK(hipMemcpy(xy.data(), h->lane[h->cur].d.cand_xy + off, (size_t)4 * m, hipMemcpyDeviceToHost));
    UVO_HIP_CHECK(hipMemcpy(sc.data(), h->lane[h->cur].d.cand_sc + off, (size_t)4 * m, hipMemcpyDeviceToHost));
    for (int i = 0; i < m; ++i) {
      dst_xys[3 * i] = (int32_t)(xy[i] & 0xffff);
      dst_xys[3 * i + 1] = (int32_t)(xy[i] >> 16);
      dst_xys[3 * i + 2] = (int32_t)sc[i];
    }
  }
  return UVO_OK;
}

// The quad-tree launch on lists of the caller's choosing.  What a list may hold is what k_fast_score can leave behind, and octree_body is
// safe on exactly that: a coordinate inside [3, bw - 3) x [3, bh - 3) indexes the path tables (bw + bh entries), the roots (x / hX < nIni)
// and the count pyramid (a T bin below nIni * 4^G) inside their tables and gives an order key whose in-cell parts stay below 128; at most
// cand_cap entries in both lists together keep the gather's slots, P and the pstate words inside the level's part of the candidate block;
// distinct coordinates make the order key unique, which is what recognises the winner of a node; and the node tables of the LDS carve
// are sized by the quota and nIni alone (at most quota + 3 nodes, or 4 * nIni after the unconditional first pass), whatever the list.
int uvo_extractor_octree_tap(uvo_extractor* h, int batch, const int32_t* n_hi, const int32_t* n_lo, const int32_t* hi_xys, const int32_t* lo_xys,
                             const uint8_t* cell_flags, int flags_per_frame, int32_t* sel_count, int32_t* cand_count, int32_t* fcount, int32_t* sel_xys,
                             int sel_cap, int32_t* threads, int32_t* residue) {
  if (!h || !h->have_geom) return fail(UVO_E_BADARG, "no geometry yet: the tap follows a completed extract call");
  if (batch < 1 || batch > h->cfg.max_batch) return fail(UVO_E_BADARG, "batch outside 1..max_batch");
  if (!n_hi || !n_lo || !hi_xys || !lo_xys || !cell_flags || !sel_count || !cand_count || !fcount || !sel_xys || sel_cap < 0 || !threads || !residue)
    return fail(UVO_E_BADARG, "null pointer");
  const Geom& g = h->geom;
  const int nl = g.nlevels, np = batch * nl;
  if (flags_per_frame != fast_flags_per_frame(g)) return fail(UVO_E_BADARG, "cell flags: not the full nRows x nCols grid of every level");
  // ---- every check, before anything on the device is touched ----
  std::vector<uint32_t> seen;
  size_t o_hi = 0, o_lo = 0;
  for (int q = 0; q < np; ++q) {
    const LevelGeom& L = g.lv[q % nl];
    if (n_hi[q] < 0 || n_lo[q] < 0 || (int64_t)n_hi[q] + n_lo[q] > L.cand_cap) return fail(UVO_E_BADARG, "more candidates than the level's cand_cap");
    seen.clear();
    for (int part = 0; part < 2; ++part) {
      const int32_t* t = part ? lo_xys + 3 * o_lo : hi_xys + 3 * o_hi;
      for (int i = 0; i < (part ? n_lo[q] : n_hi[q]); ++i) {
        const int x = t[3 * i], y = t[3 * i + 1], s = t[3 * i + 2];
        if (x < 3 || x >= L.bw - 3 || y < 3 || y >= L.bh - 3) return fail(UVO_E_BADARG, "candidate outside [3, bw - 3) x [3, bh - 3) of its level");
        if (s < 0 || s > 255) return fail(UVO_E_BADARG, "candidate score outside 0..255");
        seen.push_back((uint32_t)x | (uint32_t)y << 16);
      }
    }
    std::sort(seen.begin(), seen.end());
    if (std::adjacent_find(seen.begin(), seen.end()) != seen.end()) return fail(UVO_E_BADARG, "the same (x, y) twice in one problem");
    o_hi += (size_t)n_hi[q], o_lo += (size_t)n_lo[q];
  }
  UVO_HIP_CHECK(hipSetDevice(h->device));
  int rc = prepare_octree(g);
  if (rc) return rc;
  Lane& LN = h->lane[h->cur];
  const LaneScratch& d = LN.d;
  UVO_HIP_CHECK(hipStreamSynchronize(LN.stream));
  // ---- the lists where k_fast_score leaves them: survivors >= fastTh in front of the candidate array, the others packed in the low list ----
  std::vector<uint32_t> a, b;
  std::vector<int32_t> cur(2 * (size_t)np);
  o_hi = o_lo = 0;
  for (int q = 0; q < np; ++q) {
    const size_t co = (size_t)(q / nl) * g.cand_block + g.lv[q % nl].cand_off;
    a.resize((size_t)n_hi[q]), b.resize((size_t)n_hi[q]);
    for (int i = 0; i < n_hi[q]; ++i) {
      const int32_t* t = hi_xys + 3 * (o_hi + i);
      a[i] = (uint32_t)t[0] | (uint32_t)t[1] << 16, b[i] = (uint32_t)t[2];
    }
    if (n_hi[q]) {
      UVO_HIP_CHECK(hipMemcpy(d.cand_xy + co, a.data(), (size_t)4 * n_hi[q], hipMemcpyHostToDevice));
      UVO_HIP_CHECK(hipMemcpy(d.cand_sc + co, b.data(), (size_t)4 * n_hi[q], hipMemcpyHostToDevice));
    }
    a.resize((size_t)n_lo[q]);
    for (int i = 0; i < n_lo[q]; ++i) {
      const int32_t* t = lo_xys + 3 * (o_lo + i);
      a[i] = (uint32_t)t[0] | (uint32_t)t[1] << 12 | (uint32_t)t[2] << 24;
    }
    if (n_lo[q]) UVO_HIP_CHECK(hipMemcpy(d.cand_lo + co, a.data(), (size_t)4 * n_lo[q], hipMemcpyHostToDevice));
    cur[2 * q] = n_hi[q], cur[2 * q + 1] = n_lo[q];
    o_hi += (size_t)n_hi[q], o_lo += (size_t)n_lo[q];
  }
  UVO_HIP_CHECK(hipMemcpy(d.cursor, cur.data(), cur.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  UVO_HIP_CHECK(hipMemcpy(d.cell_hi, cell_flags, (size_t)batch * flags_per_frame, hipMemcpyHostToDevice));
  *threads = batch * nl <= h->oct.wide_max_problems ? 1024 : 256;  // (launch_octree's choice, octree.hip)
  rc = launch_octree(LN.stream, h->oct, h->d_lv, g, d, batch, h->d_oct_tab);
  if (rc) return rc;
  UVO_HIP_CHECK(hipGetLastError());
  UVO_HIP_CHECK(hipStreamSynchronize(LN.stream));
  // ---- what the launch left ----
  UVO_HIP_CHECK(hipMemcpy(sel_count, d.sel_count, (size_t)4 * np, hipMemcpyDeviceToHost));
  UVO_HIP_CHECK(hipMemcpy(cand_count, d.cand_count, (size_t)4 * np, hipMemcpyDeviceToHost));
  UVO_HIP_CHECK(hipMemcpy(fcount, d.fcount, (size_t)4 * np, hipMemcpyDeviceToHost));
  for (int q = 0; q < np; ++q) {
    const LevelGeom& L = g.lv[q % nl];
    const int m = std::min(std::min((int)sel_count[q], L.sel_cap), sel_cap);
    if (m <= 0) continue;
    const size_t so = (size_t)(q / nl) * g.sel_block + L.sel_off;
    a.resize((size_t)m), b.resize((size_t)m);
    UVO_HIP_CHECK(hipMemcpy(a.data(), d.sel_xy + so, (size_t)4 * m, hipMemcpyDeviceToHost));
    UVO_HIP_CHECK(hipMemcpy(b.data(), d.sel_sc + so, (size_t)4 * m, hipMemcpyDeviceToHost));
    int32_t* dst = sel_xys + (size_t)3 * q * sel_cap;
    for (int i = 0; i < m; ++i) dst[3 * i] = (int32_t)(a[i] & 0xffff), dst[3 * i + 1] = (int32_t)(a[i] >> 16), dst[3 * i + 2] = (int32_t)b[i];
  }
  std::vector<uint8_t> fl((size_t)batch * flags_per_frame);
  UVO_HIP_CHECK(hipMemcpy(cur.data(), d.cursor, cur.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (!fl.empty()) UVO_HIP_CHECK(hipMemcpy(fl.data(), d.cell_hi, fl.size(), hipMemcpyDeviceToHost));
  residue[0] = (int32_t)std::count_if(cur.begin(), cur.end(), [](int32_t v) { return v != 0; });
  residue[1] = (int32_t)std::count_if(fl.begin(), fl.end(), [](uint8_t v) { return v != 0; });
  return UVO_OK;
}

int uvo_extractor_profile(uvo_extractor* h, int enable) {
  if (!h) return fail(UVO_E_BADARG, "null handle");
  UVO_HIP_CHECK(hipSetDevice(h->device));
  RC(sync_all_lanes(h));
  h->prof.on = enable != 0;
  h->prof.clear();
  return UVO_OK;
}

int uvo_extractor_profile_only(uvo_extractor* h, const char* kernel_name) {
  if (!h) return fail(UVO_E_BADARG, "null handle");
  h->prof.only = kernel_name ? kernel_name : "";
  return UVO_OK;
}

int uvo_extractor_kernel_times(uvo_extractor* h, char* names, int names_cap, float* ms, int32_t* launches, int cap, int* n) {
  if (!h || !names || !ms || !launches || !n) return fail(UVO_E_BADARG, "null pointer");
  UVO_HIP_CHECK(hipSetDevice(h->device));
  RC(sync_all_lanes(h));
  *n = h->prof.report(names, names_cap, ms, launches, cap);
  return UVO_OK;
}

hipStream_t uvo_extractor_stream_internal(uvo_extractor* h) { return h->lane[h->cur].stream; }
void uvo_extractor_add_follower_internal(uvo_extractor* h, uvo_matcher* m) {
  std::lock_guard<std::mutex> lk(h->followers_mu);
  if (std::find(h->followers.begin(), h->followers.end(), m) == h->followers.end()) h->followers.push_back(m);
}
void uvo_extractor_drop_follower_internal(uvo_extractor* h, uvo_matcher* m) {
  std::lock_guard<std::mutex> lk(h->followers_mu);
  h->followers.erase(std::remove(h->followers.begin(), h->followers.end(), m), h->followers.end());
}
int uvo_extractor_device_internal(uvo_extractor* h) { return h->device; }
int uvo_extractor_next_lane_internal(const uvo_extractor* h) { return next_lane(h); }
const uint8_t* uvo_extractor_clahe_internal(uvo_extractor* h, int* width, int* height) {
  *width = h->clahe_w, *height = h->clahe_h;
  return h->d_clahe_out;
}

}  // extern "C"
