"""The FAST stage of ComputeKeyPointsOctTree (src/ORBextractor.cc:755-812) stated in numpy on top of tests/grider_model.py (`strength`,
`roi_points`: FAST-9/16 from its definition), and the strip plan of csrc/strip_plan.hpp restated in Python, for tests/test_fast_model.py
(which ties both to the C++ on the CPU) and tests/test_gpu_fast.py (which holds k_fast_score / k_fast_cells_list / k_fast_cells to it).

  grid         bw = w - 26, nCols = int(bw / 30), wCell = ceil(bw / nCols); the same in y
  cell (i, j)  ROI from (13 + j wCell, 13 + i hCell), wCell + 6 x hCell + 6, clipped to (w - 13, h - 13); skipped when it starts within
               6 columns / 3 rows of that edge
  per cell     cv::FAST(ROI, fastTh, nms); when that finds nothing, cv::FAST(ROI, 7, nms); points shifted by (j wCell, i hCell)
  candidates   sorted (x, y, score) relative to (13, 13), the coordinates uvo_extractor_read_candidates documents

The cells' 3-pixel-inset interiors tile the detection window [16, w - 16) x [16, h - 16).  k_fast_score cuts that window into regions
(`plan`): strips of 248 columns (narrow remainders: 2 or 4 sub-strips of 120 / 56 columns side by side in one wavefront) times segments
of 6 or 24 rows.  `region_corners` is how many pixels a region's wavefront puts on its corner list.

`mutant` names one deliberate mistake (MUTANTS); tests/test_fast_model.py shows which committed case tells each from the model."""
import collections

import numpy as np

import grider_model as gm

MIN_BORDER, WINDOW, FS_COLS = 13, 16, 248

MUTANTS = ("seam_blind_nms", "global_nms", "nms_ge", "corner_ge", "fallback_on_high_only", "fallback_drops_high", "window_15")

Cell = collections.namedtuple("Cell", "i j x0 y0 rw rh ox oy")              # ROI origin and size in image coordinates, shift of its points
Region = collections.namedtuple("Region", "item sub nsub x0 y0 x1 y1")      # owned rectangle [x0, x1) x [y0, y1), image coordinates


def grid(w, h):
    """(nCols, nRows, wCell, hCell)"""
    bw, bh = w - 2 * MIN_BORDER, h - 2 * MIN_BORDER
    n_cols, n_rows = int(np.float32(bw) / np.float32(30)), int(np.float32(bh) / np.float32(30))
    return n_cols, n_rows, int(np.ceil(np.float32(bw) / n_cols)), int(np.ceil(np.float32(bh) / n_rows))


def cells(w, h, mutant=None):
    """The cells the reference calls FAST on, row-major."""
    n_cols, n_rows, w_cell, h_cell = grid(w, h)
    max_bx, max_by = w - MIN_BORDER, h - MIN_BORDER
    out = []
    for i in range(n_rows):
        ini_y = MIN_BORDER + i * h_cell
        if ini_y >= max_by - 3:
            continue
        max_y = min(ini_y + h_cell + 6, max_by)
        for j in range(n_cols):
            ini_x = MIN_BORDER + j * w_cell
            if ini_x >= max_bx - 6:
                continue
            max_x = min(ini_x + w_cell + 6, max_bx)
            x0, y0 = ini_x, ini_y
            if mutant == "window_15":                      # the first column and row of cells start one pixel early
                x0, y0 = ini_x - (j == 0), ini_y - (i == 0)
            out.append(Cell(i, j, x0, y0, max_x - x0, max_y - y0, j * w_cell - (ini_x - x0), i * h_cell - (ini_y - y0)))
    return out


def cell_of(w, h, x, y):
    """(i, j) of the cell whose interior holds the candidate (x, y) (coordinates relative to (13, 13))"""
    n_cols, n_rows, w_cell, h_cell = grid(w, h)
    return min((y - 3) // h_cell, n_rows - 1), min((x - 3) // w_cell, n_cols - 1)


# ---- the strip plan ----------------------------------------------------------------------------------------------------------------------
def sub_cols(sub):
    return 256 // sub - 8


def strip_plan(window_w, window_h, rows_per_seg):
    """fast_strip_plan: (nfull, nseg, items, sub[2], x0[2])"""
    nseg = (window_h + rows_per_seg - 1) // rows_per_seg
    nfull = window_w // FS_COLS
    rem, x = window_w - nfull * FS_COLS, nfull * FS_COLS
    sub, x0 = [0, 0], [0, 0]
    if rem > sub_cols(2) + sub_cols(4):
        nfull, rem = nfull + 1, 0
    for k in range(2):
        if rem <= 0:
            break
        sub[k] = 2 if rem > sub_cols(4) else 4
        x0[k] = x
        x += sub_cols(sub[k])
        rem -= sub_cols(sub[k])
    narrow = sum(-(-nseg // s) for s in sub if s)
    if narrow >= nseg and (sub[0] or sub[1]):              # few segments: one ordinary strip instead
        nfull, sub, x0, narrow = nfull + 1, [0, 0], [0, 0], 0
    return nfull, nseg, nfull * nseg + narrow, sub, x0


def strip_items(window_w, window_h, rows_per_seg):
    """fast_strip_item of every item: (strip_x, seg, sub)"""
    nfull, nseg, items, sub, x0 = strip_plan(window_w, window_h, rows_per_seg)
    out = []
    for item in range(items):
        if item < nfull * nseg:
            out.append((item % nfull * FS_COLS, item // nfull, 1))
        else:
            it = item - nfull * nseg
            n0 = -(-nseg // sub[0]) if sub[0] else 0
            k = 0 if it < n0 else 1
            it -= n0 if k else 0
            out.append((x0[k], it * sub[k], sub[k]))
    return out


def plan(w, h, rows_per_seg):
    """Every region of a w x h level: one per (item, sub-strip); a sub-strip below the level has y0 == y1 (its lanes idle)."""
    ww, wh = w - 2 * WINDOW, h - 2 * WINDOW
    out = []
    for item, (strip_x, seg, nsub) in enumerate(strip_items(ww, wh, rows_per_seg)):
        for s in range(nsub):
            y0 = min((seg + s) * rows_per_seg, wh)
            y1 = min(y0 + rows_per_seg, wh)
            out.append(Region(item, s, nsub, WINDOW + strip_x, WINDOW + y0, WINDOW + min(strip_x + sub_cols(nsub), ww), WINDOW + y1))
    return out


def owner_map(w, h, rows_per_seg):
    """index into plan() of the region that owns each pixel, -1 outside the detection window"""
    own = np.full((h, w), -1, np.int32)
    for k, r in enumerate(plan(w, h, rows_per_seg)):
        assert (own[r.y0:r.y1, r.x0:r.x1] == -1).all()
        own[r.y0:r.y1, r.x0:r.x1] = k
    assert (own[WINDOW:h - WINDOW, WINDOW:w - WINDOW] >= 0).all()
    return own


def region_corners(S, region, t_min):
    """Pixels the region's wavefront lists: strength > max(t_min, 1) in the owned rectangle and its one-pixel ring, inside the window."""
    h, w = S.shape
    if region.y1 <= region.y0 or region.x1 <= region.x0:
        return 0
    x0, x1 = max(region.x0 - 1, WINDOW), min(region.x1 + 1, w - WINDOW)
    y0, y1 = max(region.y0 - 1, WINDOW), min(region.y1 + 1, h - WINDOW)
    return int((S[y0:y1, x0:x1] > max(t_min, 1)).sum())


# ---- the cell loop -----------------------------------------------------------------------------------------------------------------------
def _cell_points(S, c, t, mutant, owner=None, drop_above=None):
    """cv::FAST with NMS on one cell's ROI with one of this module's own mistakes: rows (x, y, score) in ROI coordinates."""
    score = np.zeros(S.shape, np.int32)
    if c.rw > 6 and c.rh > 6:
        win = (slice(c.y0 + 3, c.y0 + c.rh - 3), slice(c.x0 + 3, c.x0 + c.rw - 3))
        s = S[win]
        corner = s > t
        if drop_above is not None:
            corner &= ~(s > drop_above)                    # score >= fastTh  <=>  strength > fastTh
        score[win] = np.where(corner, s - 1, 0)
    h, w = score.shape
    p = np.pad(score, 1)
    keep = score > 0
    if mutant == "seam_blind_nms":
        po = np.pad(owner, 1, constant_values=-2)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx or dy:
                n = p[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
                if mutant == "seam_blind_nms":             # a neighbour another region owns is not seen
                    n = np.where(po[1 + dy:1 + dy + h, 1 + dx:1 + dx + w] == owner, n, 0)
                keep &= score > n
    ys, xs = np.nonzero(keep)
    return np.stack([xs - c.x0, ys - c.y0, score[ys, xs]], 1).astype(np.int64).reshape(-1, 3)


def cell_lists(img, fast_th, mutant=None, rows_per_seg=24, S=None):
    """Per cell of cells(): (cell, fell_back, rows (x, y, score) relative to (13, 13)).  fell_back: the first call found nothing."""
    assert mutant is None or mutant in MUTANTS
    img = np.asarray(img)
    h, w = img.shape
    S = gm.strength(img) if S is None else S
    own = owner_map(w, h, rows_per_seg) if mutant == "seam_blind_nms" else None
    passed = mutant if mutant in gm.MUTANTS else None      # global_nms, nms_ge, corner_ge: grider_model's own

    def fast(c, t, nms=True):
        if passed == "global_nms":                         # the one call that looks beyond the ROI
            return gm.roi_points(S, c.x0, c.y0, c.rw, c.rh, t, nms, passed)
        return gm.roi_points(S[c.y0:c.y0 + c.rh, c.x0:c.x0 + c.rw], 0, 0, c.rw, c.rh, t, nms, passed)   # cv::FAST sees the ROI alone

    out = []
    for c in cells(w, h, mutant):
        first = _cell_points(S, c, fast_th, mutant, own) if mutant == "seam_blind_nms" else fast(c, fast_th)
        pts, fell_back = first, len(first) == 0
        if fell_back:
            if mutant == "fallback_on_high_only" and len(fast(c, fast_th, False)):
                pass                                       # pixels reach fastTh, none survives: the mutant leaves the cell empty
            elif mutant == "seam_blind_nms":
                pts = _cell_points(S, c, 7, mutant, own)
            elif mutant == "fallback_drops_high":
                pts = _cell_points(S, c, 7, mutant, drop_above=fast_th)
            else:
                pts = fast(c, 7)
        out.append((c, fell_back, [(int(x) + c.ox, int(y) + c.oy, int(s)) for x, y, s in pts]))
    return out


def level_candidates(img, fast_th, mutant=None, rows_per_seg=24):
    return sorted(p for _, _, pts in cell_lists(img, fast_th, mutant, rows_per_seg) for p in pts)

