"""Brute-force model of the grid-window search -- FrameKTL::GetFeaturesInArea with FrameKTL::PosInGrid (src/FrameKTL.cc:359-436) and
KeyFrame::GetFeaturesInArea (src/KeyFrame.cc:952-992) -- written from the reference, not from the kernels, and the scenes that
tests/test_window_model.py (CPU, against the oracle) and tests/test_gpu_windows.py (the device) share.

The model has no grid: it filters all key points by cell range, level rule and |dx| <= r && |dy| <= r, then sorts the survivors by
(ix, iy, index), which is the order the reference's nested loops over mGrid[ix][iy] visit them in.

  grid     inv_w = f32(64) / f32(max_x - min_x); cell = round-half-away-from-zero of the float32 product (kp.x - f32(min_x)) * inv_w.
           The rounding is done in float64 (|v| + 0.5 is exact there; formed in float32 it rounds a second time and disagrees with
           round()).  A key point outside 0..63 x 0..47, or with a non-finite coordinate, is in no cell.
  window   floor / ceil of the float32 expressions, the clamps and the four early returns in the reference's order.  The conversion to
           int is the x86 one the reference is built for: a value that is not finite or does not fit gives INT_MIN.  It follows that a
           query whose x, y or r is not finite returns nothing (the second test, nMaxCellX < 0, catches what the first one let pass);
           window() states that case on its own so that it does not rest on the conversion.
  levels   (-1, -1) no filter; equal values that level only; otherwise the range [min, max] -- (-1, 0) is a range, min > max is empty.
"""
import numpy as np

f32 = np.float32
COLS, ROWS = 64, 48
INT_MIN = -2 ** 31
KP = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
WIN = np.dtype([("x", "<f4"), ("y", "<f4"), ("r", "<f4"), ("level", "<i4"), ("lo", "<i4"), ("hi", "<i4")])
BIG = 4096.0                               # a radius that covers every frame used here


def inv_cell(bounds):
    """mfGridElementWidthInv, mfGridElementHeightInv (src/FrameKTL.cc:83-84)"""
    min_x, min_y, max_x, max_y = bounds
    return f32(COLS) / f32(max_x - min_x), f32(ROWS) / f32(max_y - min_y)


def round_half_away(v):
    """C's round() of float32 values, as float64 (exact: |v| + 0.5 needs at most 25 significant bits beyond v's own)"""
    v = np.asarray(v, f32).astype(np.float64)
    return np.copysign(np.floor(np.abs(v) + 0.5), v)


def grid_products(kps, bounds):
    """the float32 products PosInGrid rounds"""
    inv_w, inv_h = inv_cell(bounds)
    with np.errstate(all="ignore"):
        return (kps["x"].astype(f32) - f32(bounds[0])) * inv_w, (kps["y"].astype(f32) - f32(bounds[1])) * inv_h


def cell_of(kps, bounds):
    """-> in_grid[n], ix[n], iy[n], and the rounded products themselves (float64, NaN where not finite)"""
    u, v = grid_products(kps, bounds)
    pu, pv = round_half_away(u), round_half_away(v)
    with np.errstate(all="ignore"):
        ok = np.isfinite(pu) & np.isfinite(pv) & (pu >= 0) & (pu < COLS) & (pv >= 0) & (pv < ROWS)
    ix, iy = np.where(ok, pu, -1).astype(np.int64), np.where(ok, pv, -1).astype(np.int64)
    return ok, ix, iy, pu, pv


def _cvt(v):
    """(int)v on x86: cvttss2si gives the "integer indefinite" INT_MIN for NaN, infinities and whatever does not fit"""
    v = float(v)
    if not np.isfinite(v) or v >= 2.0 ** 31 or v <= -2.0 ** 31 - 1:
        return INT_MIN
    return int(v)


def window(bounds, x, y, r):
    """-> ((x0, x1, y0, y1), None), or (None, why) with why in "right", "left", "bottom", "top" (the early return taken) or "nonfinite"."""
    x, y, r = f32(x), f32(y), f32(r)
    if not (np.isfinite(x) and np.isfinite(y) and np.isfinite(r)):
        return None, "nonfinite"
    inv_w, inv_h = inv_cell(bounds)
    mx, my = f32(bounds[0]), f32(bounds[1])
    with np.errstate(all="ignore"):
        x0 = max(0, _cvt(np.floor((x - mx - r) * inv_w)))
        if x0 >= COLS:
            return None, "right"
        x1 = min(COLS - 1, _cvt(np.ceil((x - mx + r) * inv_w)))
        if x1 < 0:
            return None, "left"
        y0 = max(0, _cvt(np.floor((y - my - r) * inv_h)))
        if y0 >= ROWS:
            return None, "bottom"
        y1 = min(ROWS - 1, _cvt(np.ceil((y - my + r) * inv_h)))
        if y1 < 0:
            return None, "top"
    return (x0, x1, y0, y1), None


def level_mask(octave, lo, hi):
    if lo == -1 and hi == -1:
        return np.ones(len(octave), bool)
    if lo == hi:
        return octave == lo
    return ~((octave < lo) | (octave > hi))


def features_in_area(kps, bounds, x, y, r, lo=-1, hi=-1, grid=None):
    """The list GetFeaturesInArea(x, y, r, lo, hi) returns, in its order.  grid = cell_of(kps, bounds), when the caller has it."""
    w, _ = window(bounds, x, y, r)
    if w is None or len(kps) == 0:
        return np.zeros(0, np.int32)
    ok, ix, iy = (grid or cell_of(kps, bounds))[:3]
    x, y, r = f32(x), f32(y), f32(r)
    with np.errstate(all="ignore"):
        m = ok & (ix >= w[0]) & (ix <= w[1]) & (iy >= w[2]) & (iy <= w[3]) & level_mask(kps["octave"], lo, hi)
        m &= ~((np.abs(kps["x"].astype(f32) - x) > r) | (np.abs(kps["y"].astype(f32) - y) > r))
    idx = np.nonzero(m)[0]
    return idx[np.lexsort((idx, iy[idx], ix[idx]))].astype(np.int32)


def column_runs(kps, bounds, x, y, r, grid=None):
    """How many key points the cells (ix, y0..y1) hold, for every column ix of the window: the runs a walk of the grid goes through,
    whatever the level rule and the distance test then keep of them."""
    w, _ = window(bounds, x, y, r)
    if w is None:
        return []
    ok, ix, iy = (grid or cell_of(kps, bounds))[:3]
    return [int((ok & (ix == c) & (iy >= w[2]) & (iy <= w[3])).sum()) for c in range(w[0], w[1] + 1)]


# ---- the radius and level rule of each marshalling layer, in the reference's float order ------------------------------------------

def sbp_window(view_cos, th, scale_factors, level):
    """SearchByProjection(F, vpMapPoints, th) src/ORBmatcher.cc:53-73 with RadiusByViewingCos :127-133 (float against the double 0.998)"""
    r = f32(2.5) if float(f32(view_cos)) > 0.998 else f32(4.0)
    if f32(th) != f32(1.0):
        r = f32(r * f32(th))
    with np.errstate(all="ignore"):
        return f32(r * f32(scale_factors[level])), level - 1, level


def sbp_kf_window(th, scale_factors, level):
    """SearchByProjection(CurrentFrame, pKF, ...) src/ORBmatcher.cc:1672-1674"""
    with np.errstate(all="ignore"):
        return f32(f32(th) * f32(scale_factors[level])), level - 1, level + 1


def fuse_window(th, scale_factors, level):
    """Fuse src/ORBmatcher.cc:1077, levels :1094"""
    with np.errstate(all="ignore"):
        return f32(f32(th) * f32(scale_factors[level])), level - 1, level


# ---- descriptors for probing ------------------------------------------------------------------------------------------------------

def hadamard_descriptors(n):
    """Rows of the 256 x 256 Sylvester Hadamard matrix and their complements as 256-bit descriptors: up to 512, pairwise distance 128
    or 256."""
    assert n <= 512
    H = np.array([[1]], np.int8)
    for _ in range(8):
        H = np.block([[H, H], [H, -H]])
    bits = (np.concatenate([H, -H]) < 0).astype(np.uint8)
    return np.ascontiguousarray(np.packbits(bits, axis=1)[:n])


def hamming(a, b):
    return np.unpackbits(a[:, None, :] ^ b[None, :, :], axis=2).sum(2)


# ---- scenes -----------------------------------------------------------------------------------------------------------------------

LEVEL_FORMS = ((-1, -1), (2, 2), (0, 1), (-1, 0), (3, 1))       # none, one level, a range, the range that starts at -1, empty
BOUNDARY_RADII = (0.0, 1.0, 2.5, 4.0, 7.5, 12.0, 40.0)
RUN_LENGTHS = (7, 8, 9, 17)
EDGE_BOUNDS = ((0, 0, 512, 384), (-7, -5, 645, 517), (3, 2, 755, 483), (0, 0, 64, 48))


class Scene:
    """kp[n]; win[W] (centre, radius, the level a projection search would predict, the generic level rule); tags[W]: what a window is
    there for; planted: tag -> key point indices."""

    def __init__(self, name, bounds):
        self.name, self.bounds = name, tuple(bounds)
        self._kp, self._win, self.tags, self.planted = [], [], [], {}

    def add_kp(self, x, y, octave, tag=None):
        self._kp.append((f32(x), f32(y), int(octave)))
        if tag is not None:
            self.planted.setdefault(tag, []).append(len(self._kp) - 1)
        return len(self._kp) - 1

    def add_win(self, x, y, r, level, lo, hi, tag):
        self._win.append((f32(x), f32(y), f32(r), int(level), int(lo), int(hi)))
        self.tags.append(tag)

    def finish(self, rng, shuffle=True):
        n = len(self._kp)
        perm = rng.permutation(n) if shuffle else np.arange(n)      # planted groups are spread over the index range
        kp = np.zeros(n, KP)
        for new, old in enumerate(perm):
            kp["x"][new], kp["y"][new], kp["octave"][new] = self._kp[old]
        kp["size"], kp["angle"] = 31.0, rng.uniform(0, 360, n).astype(f32)
        where = np.empty(n, np.int64)
        where[perm] = np.arange(n)
        self.planted = {t: sorted(int(where[i]) for i in v) for t, v in self.planted.items()}
        self.kp, self.n = kp, n
        self.win = np.array(self._win, WIN) if self._win else np.zeros(0, WIN)
        self.grid = cell_of(kp, self.bounds)
        return self

    def which(self, tag):
        return [i for i, t in enumerate(self.tags) if t == tag or t.startswith(tag + ":")]

    def lists(self, layer="generic"):
        """the model's list of every window; layer: "generic" (the window's own level rule), "fuse" [level - 1, level],
        "kf" [level - 1, level + 1]"""
        out = []
        for w in self.win:
            lo, hi = {"generic": (w["lo"], w["hi"]), "fuse": (w["level"] - 1, w["level"]), "kf": (w["level"] - 1, w["level"] + 1)}[layer]
            out.append(features_in_area(self.kp, self.bounds, w["x"], w["y"], w["r"], int(lo), int(hi), self.grid))
        return out


def _exact_tie(bounds, axis, k):
    """a float32 coordinate whose grid product is exactly k + 0.5, or None where the cell size admits none nearby"""
    inv = inv_cell(bounds)[axis]
    o = f32(bounds[axis])
    c = f32(float(bounds[axis]) + (k + 0.5) / float(inv))
    for cand in [c] + [np.nextafter(c, f32(s * np.inf)) for s in (-1, 1)]:
        if (f32(cand) - o) * inv == f32(k + 0.5):
            return f32(cand)
    for step in range(2, 40):
        for s in (-1, 1):
            cand = c
            for _ in range(step):
                cand = np.nextafter(cand, f32(s * np.inf))
            if (cand - o) * inv == f32(k + 0.5):
                return cand
    return None


def edge_scene(bounds, seed=7):
    """One frame with everything an extractor's key points never do: cells 64, 48 and -1, exact x.5 ties, members exactly at
    |dx| == r with their nextafter neighbours, windows that leave the grid on every side, column runs of 7, 8, 9 and 17 items, a cell
    whose index order is not its position order, clusters for the order tests, every form of the level rule."""
    rng = np.random.default_rng(seed)
    min_x, min_y, max_x, max_y = bounds
    W, H = max_x - min_x, max_y - min_y
    cw, ch = W / 64.0, H / 48.0
    s = Scene("edges_%d_%d_%d_%d" % tuple(bounds), bounds)
    q = lambda v: np.round(v * 4) / 4                                   # quarter pixels: sums with the radii below are exact
    at = lambda u, v: (min_x + u * cw, min_y + v * ch)                  # from grid units
    clean = []                                                          # windows no random key point may share a cell with

    # members exactly on the border of their window, one float outside it, on all four sides
    for k, r in enumerate(BOUNDARY_RADII):
        level = k % 5
        x, y = q(min_x + W * (0.14 + 0.03 * k)), q(min_y + H * (0.03 + 0.02 * k))
        lo, hi = ((-1, -1), (level, level), (level - 1, level + 1))[k % 3]
        s.add_win(x, y, r, level, lo, hi, "boundary:%g" % r)
        for dx, dy in ((1, 0), (-1, 0), (0, 1), (0, -1)):
            ex, ey = f32(x + dx * r), f32(y + dy * r)
            s.add_kp(ex, ey, level, "on:%g" % r)
            s.add_kp(np.nextafter(ex, f32(dx * np.inf)) if dx else ex, np.nextafter(ey, f32(dy * np.inf)) if dy else ey, level, "off:%g" % r)

    # column runs of exactly 7, 8, 9 and 17 items: the cells (c, 8..10) hold them, the columns around stay empty
    r_run = f32(1.4 * max(cw, ch))
    for j, length in enumerate(RUN_LENGTHS):
        c = 45 + 4 * j
        x, y = at(c, 9)
        s.add_win(x, y, r_run, 1, -1, -1, "run:%d" % length)
        clean.append((x, y, r_run))
        for _ in range(length):
            px, py = at(c + rng.uniform(-0.35, 0.35), rng.integers(8, 11) + rng.uniform(-0.35, 0.35))
            s.add_kp(px, py, rng.integers(0, 3), "run:%d" % length)

    # clusters for the order tests: 12 key points of level 0 around a cell corner, so that they fall in four cells at least
    for j, r in enumerate((2.5, 4.0, 7.5)):
        x, y = at((6.5, 20.5, 38.5)[j], 30.5)
        s.add_win(x, y, r, 0, *((-1, -1), (0, 0), (-1, 0))[j], "order:%g" % r)
        clean.append((x, y, r))
        for dx, dy in ((-1, -1), (1, -1), (-1, 1), (1, 1)):            # one per quadrant for certain, the rest anywhere
            s.add_kp(x + dx * 0.6 * r, y + dy * 0.6 * r, 0, "order:%g" % r)
        for _ in range(8):
            s.add_kp(x + rng.uniform(-0.95, 0.95) * r, y + rng.uniform(-0.95, 0.95) * r, 0, "order:%g" % r)

    # one cell, index order against position order: the shuffle decides the indices, the test checks that the orders differ
    for j in range(6):
        px, py = at(20 + 0.06 * j - 0.2, 22 + 0.05 * (j * 5 % 6) - 0.15)
        s.add_kp(px, py, j % 3, "one_cell")
    s.add_win(*at(20, 22), f32(1.2 * max(cw, ch)), 1, -1, -1, "one_cell")

    # cells outside the grid and exact ties
    s.add_kp(*at(63.7, 20.2), 1, "cell64")
    s.add_kp(*at(31.3, 47.7), 1, "cell48")
    s.add_kp(*at(-0.7, 11.1), 1, "cell-1")
    s.add_kp(*at(12.2, -0.7), 1, "cell-1")
    s.add_kp(*at(63.45, 47.45), 1, "last_cell")
    s.add_kp(*at(-0.45, -0.45), 1, "first_cell")
    for axis in (0, 1):
        for k in (-1, 0, 17, (63, 47)[axis]):
            t = _exact_tie(bounds, axis, k)
            if t is not None:
                other = at(25.2, 25.2)[1 - axis]
                s.add_kp(*((t, other) if axis == 0 else (other, t)), 1, "tie")

    # windows that leave the grid: wholly (one per early return) and partly (the corners, a radius of 40)
    s.add_win(max_x + 2 * cw + 41, min_y + H / 2, 40, 1, -1, -1, "early:right")
    s.add_win(min_x - 2 * cw - 41, min_y + H / 2, 40, 1, -1, -1, "early:left")
    s.add_win(min_x + W / 2, max_y + 2 * ch + 41, 40, 1, -1, -1, "early:bottom")
    s.add_win(min_x + W / 2, min_y - 2 * ch - 41, 40, 1, -1, -1, "early:top")
    for j, (u, v) in enumerate(((0, 0), (64, 0), (0, 48), (64, 48))):
        s.add_win(*at(u, v), 40, 1, *LEVEL_FORMS[j], "corner")
    s.add_win(min_x + W / 2, min_y + H / 2, BIG, 2, -1, -1, "whole")
    s.add_win(min_x + W / 2, min_y + H / 2, BIG, 1, 0, 1, "whole")

    # the random rest: key points anywhere in the frame (not in the cells of a clean window), windows around some of them
    windows_of_clean = [window(bounds, *c)[0] for c in clean]
    placed = 0
    while placed < 150:
        u, v = rng.uniform(0.6, 62.4), rng.uniform(0.6, 46.4)
        px, py = at(u, v)
        if placed % 3 == 0:
            px, py = q(px), q(py)
        _, ix, iy, _, _ = cell_of(np.array([(px, py, 0, 0, 0, 0, 0)], KP), bounds)
        if any(w[0] <= ix[0] <= w[1] and w[2] <= iy[0] <= w[3] for w in windows_of_clean):
            continue
        s.add_kp(px, py, rng.integers(0, 5), "random")
        placed += 1
    randoms = s.planted["random"]
    radii = (0.0, 1.0, 7.5, 40.0, 2.5, 12.0)
    for j in range(30):
        px, py, _ = s._kp[randoms[j * 5]]
        r = radii[j % len(radii)]
        off = 0.0 if r == 0.0 else float(q(rng.uniform(-0.6, 0.6) * r))
        s.add_win(px + f32(off), py - f32(off), r, j % 5, *LEVEL_FORMS[j % 5], "random")
    return s.finish(rng)


def nonfinite_scene(seed=11):
    """Key points with a NaN or infinite coordinate among ordinary ones in the first cells (where a conversion that gives 0 for NaN
    would put them), queries that reach those cells, and queries whose centre or radius is not finite."""
    rng = np.random.default_rng(seed)
    bounds = (0, 0, 512, 384)
    s = Scene("nonfinite", bounds)
    nan, inf = f32(np.nan), f32(np.inf)
    for _ in range(40):
        s.add_kp(rng.uniform(0, 30), rng.uniform(0, 30), 0, "finite")
    for _ in range(40):
        s.add_kp(rng.uniform(30, 500), rng.uniform(30, 370), 0, "finite")
    for y in (2.0, 100.0, 300.0):
        s.add_kp(nan, y, 0, "nan")
        s.add_kp(inf, y, 0, "inf")
        s.add_kp(-inf, y, 0, "inf")
    for x in (3.0, 200.0, 400.0):
        s.add_kp(x, nan, 0, "nan")
        s.add_kp(x, inf, 0, "inf")
    s.add_kp(nan, nan, 0, "nan")
    for x, y, r in ((4, 4, 12), (2, 100, 12), (200, 3, 7.5), (0, 0, 40), (256, 192, BIG), (10, 300, 40)):
        s.add_win(x, y, r, 0, -1, -1, "finite")
        for _ in range(3):
            s.add_kp(min(x, 500) + rng.uniform(0, 0.5) * min(r, 40), min(y, 370) + rng.uniform(0, 0.5) * min(r, 40), 0, "finite")
    for x, y, r in ((nan, 4, 12), (4, nan, 12), (4, 4, nan), (nan, nan, nan), (inf, 4, 12), (-inf, 4, 12), (4, inf, 12), (4, -inf, 12), (4, 4, inf),
                    (256, 192, inf), (nan, 192, BIG)):
        s.add_win(x, y, r, 0, -1, -1, "nonfinite")
    return s.finish(rng)


def one_cell_scene(n=40, seed=13):
    """every key point in cell (31, 23): one run holds the whole frame"""
    rng = np.random.default_rng(seed)
    bounds = (3, 2, 755, 483)
    cw, ch = 752 / 64.0, 481 / 48.0
    s = Scene("one_cell", bounds)
    for _ in range(n):
        s.add_kp(3 + (31 + rng.uniform(-0.4, 0.4)) * cw, 2 + (23 + rng.uniform(-0.4, 0.4)) * ch, rng.integers(0, 3), "all")
    x, y = 3 + 31 * cw, 2 + 23 * ch
    for j, r in enumerate((0.0, 1.0, 4.0, 7.5, 40.0, BIG)):
        s.add_win(x, y, r, j % 3, *LEVEL_FORMS[j % 5], "centre")
    s.add_win(x + 5 * cw, y, 7.5, 1, -1, -1, "beside")
    s.add_win(x, y, -1.0, 1, -1, -1, "negative")                        # every |dx| exceeds a negative radius: nothing
    return s.finish(rng)


def big_scene(n, seed=17):
    """n key points spread over the frame (4096 and 4097: the two regimes of the grid build), a few windows"""
    rng = np.random.default_rng(seed + n)
    bounds = (0, 0, 752, 480)
    s = Scene("big_%d" % n, bounds)
    for _ in range(n):
        s.add_kp(rng.uniform(-4, 756), rng.uniform(-4, 484), rng.integers(0, 4), "random")
    for j in range(12):
        s.add_win(rng.uniform(20, 730), rng.uniform(20, 460), (7.5, 40.0, 12.0)[j % 3], j % 4, *LEVEL_FORMS[j % 4], "random")
    s.add_win(376, 240, BIG, 1, -1, -1, "whole")
    s.add_win(0, 0, 40, 1, -1, -1, "corner")
    s.add_win(752, 480, 40, 1, -1, -1, "corner")
    return s.finish(rng, shuffle=False)


def big_targets(s, count=64):
    """the key points of a big scene that are probed: up to four from every window's list, the rest evenly spread"""
    t = []
    for li in s.lists():
        if len(li) < s.n // 2:
            t += [int(j) for j in li[:4]]
    t = sorted(set(t))[:count // 2]
    rest = [j for j in range(0, s.n, s.n // count) if j not in t]
    return np.array(sorted(t + rest[:count - len(t)]))


def random_descriptors(n, seed=19):
    return np.random.default_rng(seed).integers(0, 256, (n, 32), dtype=np.uint8)
