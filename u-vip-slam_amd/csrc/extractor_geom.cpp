// Extractor tables that are pure arithmetic on the configuration and the image size: the constructor tables, the geometry of one
// resolution, the resize coefficient tables, scratch sizes and the tile-group specs of the fused pyramid.  Nothing here calls the HIP
// runtime; extractor.cpp uploads what these functions build.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "extractor_priv.hpp"
#include "fast_geom.hpp"

namespace uvo {

static inline int cv_round_host(float v) { return (int)lrintf(v); }
static inline int cv_floor_host(float v) {
  int i = (int)v;
  return i - (i > v);
}

// ORBextractor::ORBextractor: src/ORBextractor.cc:458-512
void build_ctor_tables(uvo_extractor* h) {
  const int nl = h->cfg.nlevels;
  const double scaleFactor = (double)h->cfg.scale_factor;  // member is double (include/ORBextractor.h:79)
  h->scale.assign(nl, 1.f);
  h->inv_scale.assign(nl, 1.f);
  for (int i = 1; i < nl; ++i) h->scale[i] = (float)(h->scale[i - 1] * scaleFactor);
  const float invScaleFactor = (float)(1.0f / scaleFactor);
  for (int i = 1; i < nl; ++i) h->inv_scale[i] = h->inv_scale[i - 1] * invScaleFactor;
  h->quota.assign(nl, 0);
  const float factor = (float)(1.0 / scaleFactor);
  float nDesired = h->cfg.nfeatures * (1 - factor) / (1 - (float)pow((double)factor, (double)nl));
  int sum = 0;
  for (int l = 0; l < nl - 1; ++l) {
    h->quota[l] = cv_round_host(nDesired);
    sum += h->quota[l];
    nDesired *= factor;
  }
  h->quota[nl - 1] = std::max(h->cfg.nfeatures - sum, 0);
  // umax (:494-511), HALF_PATCH_SIZE = 15
  const int HP = 15;
  int v, v0, vmax = cv_floor_host(HP * sqrtf(2.f) / 2 + 1);
  int vmin = (int)ceilf(HP * sqrtf(2.f) / 2);
  const double hp2 = HP * HP;
  for (v = 0; v <= vmax; ++v) h->umax[v] = (int)lrint(sqrt(hp2 - v * v));
  for (v = HP, v0 = 0; v >= vmin; --v) {
    while (h->umax[v0] == h->umax[v0 + 1]) ++v0;
    h->umax[v] = v0;
    ++v0;
  }
  // Gaussian taps: cv::getGaussianKernel(7, 2, CV_32F) then convertTo(CV_32S, 256)
  float cf[7];
  double s = 0;
  for (int i = 0; i < 7; ++i) {
    double x = i - 3.0;
    cf[i] = (float)std::exp(-0.5 / 4.0 * x * x);
    s += cf[i];
  }
  s = 1. / s;
  for (int i = 0; i < 4; ++i) h->gtaps[i] = cv_round_host((float)(cf[i] * s) * 256.f);
}

// Geometry of one resolution: pyramid sizes (:966-969), detection window and FAST cells (:755-790),
// quad-tree roots (:1010-1012), scratch offsets.
int build_geom(const uvo_extractor* h, int width, int height, Geom& g, std::vector<CellDesc>& cells, std::vector<int32_t>* cell_flag) {
  const int nl = h->cfg.nlevels;
  memset(&g, 0, sizeof(g));
  g.width = width, g.height = height, g.nlevels = nl;
  cells.clear();
  if (cell_flag) cell_flag->clear();
  int64_t off = 0, coff = 0;
  int soff = 0, xt = 0, yt = 0, ot = 0, flag_base = 0;
  for (int l = 0; l < nl; ++l) {
    LevelGeom& L = g.lv[l];
    L.w = cv_round_host((float)width * h->inv_scale[l]);
    L.h = cv_round_host((float)height * h->inv_scale[l]);
    if (L.w < 56 || L.h < 56 || L.w > 4096 || L.h > 4096) return fail(UVO_E_UNSUPPORTED, "pyramid level outside 56..4096 px");
    L.pw = L.w + 2 * kPad, L.ph = L.h + 2 * kPad;
    L.pitch = (L.pw + kPyrPitchAlign - 1) / kPyrPitchAlign * kPyrPitchAlign;  // whole cache lines: a line never holds bytes of two rows (pyr_schedule.hpp)
    L.plane_off = off;
    off += (int64_t)L.pitch * ((L.ph + 7) & ~7);  // whole 16 x 8 tiles: the blurred plane is stored tiled (gauss.hip), same offsets for both
    off = (off + 255) / 256 * 256;
    L.bw = L.w - 2 * kMinBorder, L.bh = L.h - 2 * kMinBorder;
    const float fw = (float)L.bw, fh = (float)L.bh;
    L.nCols = (int)(fw / 30.f), L.nRows = (int)(fh / 30.f);
    L.wCell = (int)ceilf(fw / L.nCols), L.hCell = (int)ceilf(fh / L.nRows);
    L.cell_base = (int)cells.size();
    const int maxBX = L.w - kMinBorder, maxBY = L.h - kMinBorder;
    int cap = 0;
    for (int i = 0; i < L.nRows; ++i) {
      const int iniY = kMinBorder + i * L.hCell;
      int maxY = iniY + L.hCell + 6;
      if (iniY >= maxBY - 3) continue;
      if (maxY > maxBY) maxY = maxBY;
      for (int j = 0; j < L.nCols; ++j) {
        const int iniX = kMinBorder + j * L.wCell;
        int maxX = iniX + L.wCell + 6;
        if (iniX >= maxBX - 6) continue;
        if (maxX > maxBX) maxX = maxBX;
        CellDesc c;
        c.level = (int16_t)l;
        c.x0 = (int16_t)iniX, c.y0 = (int16_t)iniY;
        c.rw = (int16_t)(maxX - iniX), c.rh = (int16_t)(maxY - iniY);
        c.ox = (int16_t)(j * L.wCell), c.oy = (int16_t)(i * L.hCell);
        c.pad = 0;
        if (c.rw > 66 || c.rh > 66) return fail(UVO_E_UNSUPPORTED, "FAST cell larger than 66 px");
        const int iw = c.rw - 6, ih = c.rh - 6;
        if (iw <= 0 || ih <= 0) continue;  // FAST on an ROI without interior finds nothing
        cap += ((iw + 1) / 2) * ((ih + 1) / 2);
        cells.push_back(c);
        if (cell_flag) {
          cell_flag->resize((size_t)flag_base + (size_t)L.nRows * L.nCols, -1);
          (*cell_flag)[flag_base + i * L.nCols + j] = (int32_t)(cells.size() - 1) | (l << 24);
        }
      }
    }
    flag_base += L.nRows * L.nCols;  // the same running base as fast_levels() (fast.hip)
    if (cell_flag) cell_flag->resize((size_t)flag_base, -1);
    if (cells.size() >= (1u << 24)) return fail(UVO_E_UNSUPPORTED, "more than 2^24 FAST cells per frame");
    L.n_cells = (int)cells.size() - L.cell_base;
    L.quota = h->quota[l];
    if (L.quota > kMaxOctN) return fail(UVO_E_UNSUPPORTED, "per-level feature quota above the quad-tree kernel's capacity");
    L.cand_cap = cap;
    L.cand_off = coff;
    coff += (cap + 63) / 64 * 64;
    L.nIni = (int)roundf((float)L.bw / (float)L.bh);
    if (L.nIni < 1 || L.nIni > 64) return fail(UVO_E_UNSUPPORTED, "image aspect ratio outside the quad-tree's range");
    // DistributeOctTree returns at most quota + 3 nodes once it is in its careful phase, but the first pass splits all nIni
    // roots unconditionally: up to 4 * nIni nodes whatever the quota (wide images with few features)
    L.sel_cap = std::max(L.quota, 4 * L.nIni) + 4;
    L.sel_off = soff;
    soff += L.sel_cap;
    L.hX = (float)L.bw / (float)L.nIni;
    L.scale = h->scale[l];
    L.patch_size = (float)(int)(31 * h->scale[l]);
    L.xtab_off = xt, L.ytab_off = yt;
    if (l > 0) xt += L.pitch, yt += (L.ph + 3) & ~3;  // row tables are padded to whole groups of 4 rows (k_resize_level reads a group at once)
    L.oct_tab_off = ot, L.pad_ = 0;
    ot += (L.bw + L.bh + 1) & ~1;  // (an even number of 2-byte entries: the kernels copy a table as dwords)
  }
  g.total_cells = (int)cells.size();
  g.pyr_block = off;
  g.cand_block = coff;
  g.sel_block = soff;
  g.flist_cap = soff + h->cfg.max_input_keypoints;
  return UVO_OK;
}

// cv::resize coefficient tables of every level >= 1 (pyr_tiles.hpp: pyr_build_level_tables), concatenated at the offsets build_geom assigned
void build_resize_tables(const Geom& g, std::vector<ResizeCol>& ctab, std::vector<ResizeRow>& rtab, int* fast_ok) {
  ctab.clear(), rtab.clear();
  for (int l = 1; l < g.nlevels; ++l) pyr_build_level_tables(g.lv[l - 1].w, g.lv[l - 1].h, g.lv[l].w, g.lv[l].h, g.lv[l].pitch, ctab, rtab, &fast_ok[l]);
}

// Rows per (strip, segment) work item.  A wavefront lives for the whole item, so long segments leave a long under-filled
// tail at the end of the launch (96 rows: +20 % kernel time over 24..32), and the NMS tile of a region has to fit its LDS.
// A single frame has only ~160 items of 24 rows for 1024 SIMDs: short segments spread it over more wavefronts and shorten the launch.  A
// wavefront streams its rows + 8 in blocks of 7: 6 rows of work are exactly two blocks (8 rows take three: 20 -> 16 us for one frame).
#ifndef UVO_FAST_ROWS_FEW
#define UVO_FAST_ROWS_FEW 6
#endif
int fast_rows_per_seg(int batch) { return batch <= 2 ? UVO_FAST_ROWS_FEW : FS_ROWS_MAX; }
int fast_items_per_frame(const Geom& g, int rows_per_seg) {
  int items = 0;
  for (int l = 0; l < g.nlevels; ++l) {
    FastLevel F;
    fast_strip_plan(g.lv[l].w - 32, g.lv[l].h - 32, rows_per_seg, F);
    items += F.items;
  }
  return items;
}
int fast_flags_per_frame(const Geom& g) {
  int n = 0;
  for (int l = 0; l < g.nlevels; ++l) n += g.lv[l].nRows * g.lv[l].nCols;
  return n;
}

void corner_scratch_size(const Geom& g, int max_batch, int slack, size_t* entries, size_t* counts) {
  *entries = *counts = 0;
  for (int b = 1; b <= max_batch; b = b < 16 ? b + 1 : max_batch) {
    const size_t it = (size_t)fast_items_per_frame(g, fast_rows_per_seg(b)) + slack;
    *entries = std::max(*entries, (size_t)b * it * (size_t)FS_REGION_ENTRIES);
    *counts = std::max(*counts, (size_t)b * it);
    if (b == max_batch) break;
  }
}

// The capacities a handle fixes at create time, from the geometry g of max_width x max_height: padded for the small non-monotonicities of
// the cell grid, and for other shapes of the same area
void size_capacities(uvo_extractor* h, const Geom& g) {
  const size_t B = (size_t)h->cfg.max_batch;
  h->cap_pyr_block = g.pyr_block;
  h->cap_cand_block = g.cand_block + g.cand_block / 16 + 4096;
  h->cap_cells = g.total_cells + g.total_cells / 8 + 64;
  h->cap_sel_block = g.sel_block;
  h->cap_flist = g.flist_cap;
  h->cap_xtab = 0, h->cap_ytab = 0;
  for (int l = 1; l < g.nlevels; ++l) h->cap_xtab += g.lv[l].pitch + 64, h->cap_ytab += g.lv[l].ph + 8;  // (row tables are padded to groups of 4 rows; smaller images of the same area have other level heights)
  h->cap_oct_tab = 2 * g.nlevels * (h->cfg.max_width + h->cfg.max_height + 2) + 64;  // (a level's window is never wider / higher than the image; x 2: other shapes of the same area)
  // corner-list regions: sized for every segment height the launcher may pick, at the maximum resolution
  size_t ce = 0, cn = 0;
  corner_scratch_size(g, h->cfg.max_batch, 8, &ce, &cn);
  h->cap_cor = ce + ce / 8, h->cap_cor_n = cn + cn / 8 + 64;
  h->cap_flags = B * ((size_t)fast_flags_per_frame(g) + fast_flags_per_frame(g) / 8 + 64);
}

int oct_table_entries(const Geom& g) {
  const LevelGeom& last = g.lv[g.nlevels - 1];
  return last.oct_tab_off + ((last.bw + last.bh + 1) & ~1);
}

// Every capacity check of a new geometry (its resize tables hold n_ctab / n_rtab entries) in one place: the first capacity it exceeds
int exceeded_capacity(const uvo_extractor* h, const Geom& g, size_t n_ctab, size_t n_rtab) {
  if (g.pyr_block > h->cap_pyr_block || g.cand_block > h->cap_cand_block || g.total_cells > h->cap_cells || g.sel_block > h->cap_sel_block ||
      g.flist_cap > h->cap_flist)
    return GEOM_CAP_BLOCKS;
  size_t cor = 0, cor_n = 0;
  corner_scratch_size(g, h->cfg.max_batch, 0, &cor, &cor_n);
  if (cor > h->cap_cor || cor_n > h->cap_cor_n || (size_t)h->cfg.max_batch * fast_flags_per_frame(g) > h->cap_flags) return GEOM_CAP_FAST;
  if ((int)n_ctab > h->cap_xtab) return GEOM_CAP_XTAB;
  if ((int)n_rtab > h->cap_ytab) return GEOM_CAP_YTAB;
  if (oct_table_entries(g) > h->cap_oct_tab) return GEOM_CAP_OCT_TAB;
  return GEOM_CAP_NONE;
}

// circular orientation patch (IC_Angle, src/ORBextractor.cc:125-152): rows v in [-15,15], |u| <= umax[|v|] (749 pixels).
// k_describe reads it as 31 rows x 8 dwords (u = -16 + 4*chunk + byte); entry row*8 + chunk masks the bytes inside the circle.
void build_patch_masks(const int* umax, std::vector<uint32_t>& patch) {
  patch.assign(256, 0u);
  for (int row = 0; row < 31; ++row) {
    const int v = row - 15, um = umax[v < 0 ? -v : v];
    for (int c = 0; c < 8; ++c)
      for (int k = 0; k < 4; ++k) {
        const int u = -16 + 4 * c + k;
        if (u >= -um && u <= um) patch[row * 8 + c] |= 0xffu << (8 * k);
      }
  }
}

// entry k of a tile spec (uvo_extractor::tile_spec) as a group of levels; the group ends where the next entry starts
bool tile_group_from_spec(const std::vector<uint32_t>& spec, size_t k, int nlevels, TileGroup& G) {
  G.first = (int)((spec[k] >> 16) & 0xff), G.tx = (int)((spec[k] >> 8) & 0xff), G.ty = (int)(spec[k] & 0xff), G.threads = (spec[k] >> 24) & 3 ? 1024 : 256, G.rows = (spec[k] >> 25) & 1 ? 1 : 4;
  G.last = k + 1 < spec.size() ? (int)((spec[k + 1] >> 16) & 0xff) - 1 : nlevels - 1;
  if (G.first >= nlevels) return false;  // (a spec written for more levels than this handle has)
  G.last = std::min(G.last, nlevels - 1);
  return true;
}

// number of tiles along an axis of `len` pixels for tiles of about `target` pixels
static inline uint32_t tiles_for(int len, int target) { return (uint32_t)std::min(255, std::max(1, (len + target / 2) / target)); }

// The default set of a geometry: the latency shape (a handful of frames cannot fill the chip: as many workgroups as CUs, ONE launch of
// 1024-thread workgroups with single-row work items -- the halo of a deep group is paid in redundant pixels, which idle CUs have to spare:
// measured against two and three launches and against 256-thread workgroups, profiles/r05_latency_ab.txt).
std::vector<uint32_t> default_tile_spec(const Geom& g) {
  if (g.nlevels < 2) return {};
  return {1u << 25 | 1u << 16 | tiles_for(g.lv[1].w, 34) << 8 | tiles_for(g.lv[1].h, 27)};  // 16 x 16 tiles at 640 x 512
}

}  // namespace uvo
