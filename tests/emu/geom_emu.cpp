// Host execution of the extractor's geometry arithmetic (u-vip-slam_amd/csrc/extractor_geom.cpp: nothing in it calls the HIP runtime) --
// test infrastructure, not product code.  It answers, without a device, what uvo_extractor_create() and set_geometry() decide about an
// image size on a handle of a given configuration: the level sizes, which capacity of the handle the size exceeds (and therefore which
// check of set_geometry() refuses it), and which levels take the 12-byte-window path of k_resize_level.
#include <cstdio>
#include <cstring>

#include "../../u-vip-slam_amd/csrc/extractor_geom.cpp"

namespace uvo {
static char g_emu_err[256] = "";
int fail(int code, const char* msg) {
  snprintf(g_emu_err, sizeof(g_emu_err), "%s", msg);
  return code;
}
}  // namespace uvo

// -> 0: the handle takes the size; 1 .. 5: the capacity it exceeds (GEOM_CAP_*: blocks, FAST scratch, column table, row table, quad-tree
// path tables); < 0: the UVO_E_* code of build_geom (-5: a level outside 56..4096 px); -100: the handle itself cannot be created.
// level_wh[2 * l], fast_ok[l]: of the probed size (fast_ok[0] = 1).
extern "C" int emu_geom_probe(int nfeatures, float scale_factor, int nlevels, int max_width, int max_height, int max_batch, int max_input_keypoints, int width,
                              int height, int* level_wh, int* fast_ok) {
  using namespace uvo;
  uvo_extractor* h = new uvo_extractor();
  h->cfg = uvo_extractor_cfg{nfeatures, scale_factor, nlevels, 0, 20, max_width, max_height, max_batch, max_input_keypoints, 0};
  build_ctor_tables(h);
  Geom g;
  std::vector<CellDesc> cells;
  int rc = build_geom(h, max_width, max_height, g, cells);
  if (rc == UVO_OK) {
    size_capacities(h, g);
    std::vector<int32_t> cell_flag;
    rc = build_geom(h, width, height, g, cells, &cell_flag);
    if (rc == UVO_OK) {
      std::vector<ResizeCol> ctab;
      std::vector<ResizeRow> rtab;
      int ok[kMaxLevels] = {0};
      build_resize_tables(g, ctab, rtab, ok);
      for (int l = 0; l < nlevels; ++l) level_wh[2 * l] = g.lv[l].w, level_wh[2 * l + 1] = g.lv[l].h, fast_ok[l] = l ? ok[l] : 1;
      rc = exceeded_capacity(h, g, ctab.size(), rtab.size());
    }
  } else {
    rc = -100;
  }
  delete h;
  return rc;
}

// The per-level geometry of a width x height image on a handle sized for exactly that image: lv[16 * l + ..] = w, h, bw, bh, nCols, nRows,
// wCell, hCell, n_cells, quota, cand_cap, nIni, sel_cap, flag base, 0, 0; is_cell[flag base + i * nCols + j] = 1 where grid position (i, j)
// of the level is a FAST cell (the cell-flag layout of fast_levels()).  -> bytes of the flag array per frame, or < 0: the code of build_geom.
extern "C" int emu_geom_levels(int nfeatures, float scale_factor, int nlevels, int width, int height, int* lv, unsigned char* is_cell, int is_cell_cap) {
  using namespace uvo;
  uvo_extractor* h = new uvo_extractor();
  h->cfg = uvo_extractor_cfg{nfeatures, scale_factor, nlevels, 0, 20, width, height, 1, 0, 0};
  build_ctor_tables(h);
  Geom g;
  std::vector<CellDesc> cells;
  std::vector<int32_t> cell_flag;
  int rc = build_geom(h, width, height, g, cells, &cell_flag);
  if (rc == UVO_OK) {
    rc = fast_flags_per_frame(g);
    int base = 0;
    for (int l = 0; l < nlevels; ++l) {
      const LevelGeom& L = g.lv[l];
      const int v[16] = {L.w, L.h, L.bw, L.bh, L.nCols, L.nRows, L.wCell, L.hCell, L.n_cells, L.quota, L.cand_cap, L.nIni, L.sel_cap, base, 0, 0};
      memcpy(lv + 16 * l, v, sizeof(v));
      base += L.nRows * L.nCols;
    }
    for (int i = 0; i < rc && i < is_cell_cap; ++i) is_cell[i] = i < (int)cell_flag.size() && cell_flag[i] >= 0 ? 1 : 0;
  }
  delete h;
  return rc;
}
