"""The occupancy filter of the top-up extraction, ORBextractor::operator() src/ORBextractor.cc:872-909, as the plain sequential loop it is.
k_assemble<TOPUP> (csrc/describe.hip) replaces the loop by a closed form per level, or walks it in HBM: both are held to this."""
import numpy as np

F = np.float32
# the staging limits of k_assemble<TOPUP>: more survivors or grid cells than these and one thread walks the lists in HBM
STAGED_POINTS, STAGED_CELLS = 2560, 6144


def c_div(a, b):
    """int / int of C: truncation towards zero."""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def cell_of(x, y, scale, min_px_dist):
    """(row, column) of a level position in the grid: the float32 products and the float division of :884-887, truncated."""
    tx, ty = F(x) * F(scale), F(y) * F(scale)
    return int(ty / F(min_px_dist)), int(tx / F(min_px_dist))


def topup(levels, scales, grid, min_px_dist, need):
    """levels[l]: the survivors of level l in list order, (n, 2) level coordinates; scales[l]: mvScaleFactor; grid: (rows, cols) int32.
    Returns (accepted, grid after, trace): accepted = [(level, index)] in output order, trace[l] = (KP_counter on entry, numofpoint,
    accepted on the level, how the level was left: 'cap', 'need', 'end' or 'skipped')."""
    grid = np.array(grid, np.int32, order="F", copy=True)
    accepted, trace = [], []
    total_counter = kp_counter = 0
    break_key = False
    for level, pts in enumerate(levels):
        if len(pts) == 0:
            trace.append((kp_counter, None, 0, "skipped"))
            continue
        numofpoint = c_div(need * (8 - level), 30)
        entry, taken, left = kp_counter, 0, "end"
        for i, (x, y) in enumerate(pts):
            r, c = cell_of(x, y, scales[level], min_px_dist)
            if grid[r, c] > 0:
                continue
            accepted.append((level, i))
            grid[r, c] += 1
            kp_counter += 1
            total_counter += 1
            taken += 1
            if kp_counter == numofpoint:
                kp_counter = 0
                left = "cap"
                break
            if total_counter == need:
                break_key = True
                left = "need"
                break
        trace.append((entry, numofpoint, taken, left))
        if break_key:
            break
    return accepted, grid, trace


def output_positions(levels, scales, accepted):
    """(x, y, octave) of the accepted points as the extractor returns them: level 0 as it is, the others times the level's scale (:948-959)."""
    out = np.zeros((len(accepted), 3), np.float32)
    for k, (level, i) in enumerate(accepted):
        x, y = F(levels[level][i][0]), F(levels[level][i][1])
        if level:
            x, y = x * F(scales[level]), y * F(scales[level])
        out[k] = (x, y, level)
    return out


def survivors_from_full_detect(kp, scales):
    """The per-level survivor lists behind a FullDetect result: level positions are whole pixels, so x / scale rounds back to them."""
    levels = []
    for level in range(len(scales)):
        k = kp[kp["octave"] == level]
        xy = np.stack([k["x"], k["y"]], 1).astype(np.float64)
        if level:
            xy = np.rint(xy / float(scales[level]))
            back = (xy.astype(F) * F(scales[level])).astype(F)
            assert (back[:, 0] == k["x"]).all() and (back[:, 1] == k["y"]).all()
        levels.append(xy.astype(np.float32))
    return levels


def takes_staged_walk(levels, grid):
    """k_assemble's choice: the closed form on staged lists, unless the lists or the grid are too large for the staging arrays or a cell
    below zero could take more than one point."""
    return sum(len(p) for p in levels) <= STAGED_POINTS and grid.size <= STAGED_CELLS and bool((np.asarray(grid) >= 0).all())
