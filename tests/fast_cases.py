"""The inputs of tests/test_gpu_fast.py, shared with tests/test_fast_model.py, which shows on the CPU that each of them reaches the place
in csrc/fast.hip it is named for.  Nothing here needs a GPU or the oracle; the model is tests/fast_model.py.

A case is a set of distinct frames of one size, the order in which a batch holds them (`order`: indices into the frames, at least 3 so
that the batch takes the 24-row regions), a fastTh and a number of pyramid levels.  All heights are 130: the detection window is
98 = 4 x 24 + 2 = 16 x 6 + 2 rows, so the last segment has two rows in both region heights.

Families (what each aims at: the module docstring of tests/test_gpu_fast.py):
  a  every pixel as an isolated corner     single-pixel dots on a pitch-7 lattice over flat 128, one frame per lattice offset
  b  pairs across every seam               two-pixel blobs on pitch 8 in four orientations, one frame per offset; equal pairs alone in a cell
  c  list limits                           one region with exactly 319 / 320 / 321 / 641 listed corners; uniform noise everywhere
  d  busy fall-back cells                  noise under a fastTh that leaves every cell empty: cells above and below CCAP
  e  a wavefront that takes a second cell  200 frames of 45 cells that all fall back, dense and sparse in rotation
  f  arc atlas                             every arc start x length 8 / 9 x polarity x centre value at thresholds 6 .. 128
  g  three levels                          the frames of (a) through a 3-level pyramid"""
import collections
import functools

import numpy as np

import fast_model as fm
import grider_model as gm

H = 130
SHAPES = [(122, H), (200, H), (300, H), (380, H), (430, H), (480, H), (84, H)]
GROUND = 128
DOT_CLASSES = (5, 8, 19, 20, 21, 60, 127)       # contrast of a dot, constant over 64 x 64 blocks
ORIENTATIONS = ((1, 0), (0, 1), (1, 1), (-1, 1))
PAIR_KINDS = ((190, 190), (200, 190), (190, 200))
FAST_TH = 20
COUNT_TARGETS = (319, 320, 321, 641)            # around FL_CAP = 320 and twice that
ATLAS_THRESHOLDS = (6, 7, 8, 20, 21, 128)
ATLAS_CENTRES = (0, 1, 2, 3, 126, 127, 128, 129, 252, 253, 254, 255)
ATLAS_W, ATLAS_H = 300, 200
NFEATURES = 500

Case = collections.namedtuple("Case", "name family w h fast_th nlevels frames order")


def noise(seed, w, h):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def blocky_noise(seed, w, h):
    n = noise(seed, (w + 1) // 2, (h + 1) // 2)
    return np.ascontiguousarray(np.repeat(np.repeat(n, 2, 0), 2, 1)[:h, :w])


# ---- (a) dots ----------------------------------------------------------------------------------------------------------------------------
def dot_sites(w, h, ox, oy, pitch=7):
    """(xs, ys) of the lattice points = (ox, oy) mod pitch whose ring lies inside the image -- also outside the detection window, where
    a corner must NOT be found"""
    xs, ys = np.arange(3, w - 3), np.arange(3, h - 3)
    gx, gy = np.meshgrid(xs[xs % pitch == ox], ys[ys % pitch == oy])
    return gx.ravel(), gy.ravel()


def dot_contrast(xs, ys):
    """(contrast, sign) by position: the class is constant over 64 x 64 blocks, the polarity alternates from dot to dot"""
    cls = np.array(DOT_CLASSES)[(xs // 64 + 4 * (ys // 64)) % len(DOT_CLASSES)]
    sign = np.where((xs // 7 + ys // 7) % 2 == 0, 1, -1)
    return cls, sign


def dots(w, h, ox, oy):
    img = np.full((h, w), GROUND, np.uint8)
    xs, ys = dot_sites(w, h, ox, oy)
    c, s = dot_contrast(xs, ys)
    img[ys, xs] = GROUND + c * s
    return img


def dot_frames(w, h):
    return np.stack([dots(w, h, ox, oy) for oy in range(7) for ox in range(7)])


# ---- (b) pairs ---------------------------------------------------------------------------------------------------------------------------
def pair_sites(w, h, orient, ox, oy):
    """first pixels (xs, ys) of the blobs = (ox, oy) mod 8 whose two pixels and their rings lie inside the image"""
    xs, ys = np.arange(4, w - 4), np.arange(3, h - 4)       # (orient only moves the second pixel: by at most one, inside that margin)
    gx, gy = np.meshgrid(xs[xs % 8 == ox], ys[ys % 8 == oy])
    return gx.ravel(), gy.ravel()


def pairs(w, h, orient, ox, oy):
    dx, dy = orient
    img = np.full((h, w), GROUND, np.uint8)
    xs, ys = pair_sites(w, h, orient, ox, oy)
    kind = np.array(PAIR_KINDS)[(xs // 8 + 2 * (ys // 8)) % 3]
    img[ys, xs] = kind[:, 0]
    img[ys + dy, xs + dx] = kind[:, 1]
    return img


def pair_frames(w, h, orient):
    return np.stack([pairs(w, h, orient, ox, oy) for oy in range(8) for ox in range(8)])


def lone_pairs(w, h, orient):
    """One equal pair in the middle of every cell, dots of contrast 8 (score 7: only the literal-7 call finds them) on a pitch-7 lattice
    everywhere else, none closer than 6 pixels to a pair.  Both pixels of a pair reach fastTh and suppress each other: the first call
    finds nothing, the second finds the dots.  A third pixel at 140 continues each pair: a corner of score 11 right next to a pixel of
    score 61 -- in the second call the pair's pixels still suppress it, although they themselves annihilate again."""
    dx, dy = orient
    img = np.full((h, w), GROUND, np.uint8)
    xs, ys = dot_sites(w, h, 1, 2)
    near = np.zeros(len(xs), bool)
    centres = []
    for c in fm.cells(w, h):
        if c.rw > 16 and c.rh > 16:
            cx, cy = c.x0 + c.rw // 2, c.y0 + c.rh // 2
            centres.append((cx, cy))
            near |= (np.abs(xs - cx) <= 6) & (np.abs(ys - cy) <= 6)
    img[ys[~near], xs[~near]] = GROUND + 8
    for cx, cy in centres:
        img[cy, cx] = img[cy + dy, cx + dx] = 190
        img[cy + 2 * dy, cx + 2 * dx] = 140
    return img


# ---- (c) list limits ---------------------------------------------------------------------------------------------------------------------
def count_region(w, h, rows_per_seg):
    """index in plan() of the region the count frames fill: the full strip's second segment"""
    regs = fm.plan(w, h, rows_per_seg)
    return next(k for k, r in enumerate(regs) if r.nsub == 1 and r.x0 == fm.WINDOW and r.y0 == fm.WINDOW + rows_per_seg)


def count_frame(w, h, rows_per_seg, target, seed=31):
    """Flat ground with uniform noise in the left part of one region (a 6-row region: and in the row above and the row below it, which it
    lists as its halo: 250 x 8 pixels hold 641 corners, six rows do not), trimmed until the model counts exactly `target` listed corners at
    threshold 7.  None when the region cannot hold that many."""
    r = fm.plan(w, h, rows_per_seg)[count_region(w, h, rows_per_seg)]
    grow = 0 if rows_per_seg >= 24 else 1
    ya, yb = r.y0 - grow, r.y1 + grow
    full = noise(seed, w, h)
    c0, c1 = max(ya - 8, 0), min(yb + 8, h)                                     # the rows a change can reach
    in_crop = r._replace(y0=r.y0 - c0 + fm.WINDOW, y1=r.y1 - c0 + fm.WINDOW)

    def count(img):
        crop = np.full((c1 - c0 + 2 * fm.WINDOW, w), GROUND, np.uint8)          # flat rows around it: the crop's own window must not cut the region
        crop[fm.WINDOW:fm.WINDOW + c1 - c0] = img[c0:c1]
        return fm.region_corners(gm.strength(crop), in_crop, 7)

    def with_columns(n):
        img = np.full((h, w), GROUND, np.uint8)
        img[ya:yb, r.x0:r.x0 + n] = full[ya:yb, r.x0:r.x0 + n]
        return img

    widest = r.x1 - r.x0
    if count(with_columns(widest)) < target:
        return None
    lo, hi = 1, widest
    while lo < hi:                                                                # the count grows with the columns, near enough
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if count(with_columns(mid)) >= target else (mid + 1, hi)
    while count(with_columns(lo)) < target:
        lo += 1
    img = with_columns(lo)
    n = count(img)
    for x in range(r.x0 + lo - 1, r.x0, -1):                                      # flatten pixels from the right while the count stays >= target
        for y in range(yb - 1, ya - 1, -1):
            if n == target:
                return img
            keep = img[y, x]
            img[y, x] = GROUND
            m = count(img)
            if m >= target:
                n = m
            else:
                img[y, x] = keep
    return img if n == target else None


@functools.lru_cache(maxsize=None)
def count_frames(w=300, h=H):
    """[(rows_per_seg, target, frame)] for every target a region of that height can hold"""
    out = []
    for rps in (24, 6):
        for target in COUNT_TARGETS:
            img = count_frame(w, h, rps, target)
            if img is not None:
                out.append((rps, target, img))
    return out


# ---- (d), (e) busy fall-back cells ---------------------------------------------------------------------------------------------------------
def mixed(w, h, seed):
    """uniform noise in the left half, the dots of (a) in the right half"""
    img = dots(w, h, 2, 5)
    img[:, :w // 2] = noise(seed, w, h)[:, :w // 2]
    return img


def busy_frames(w, h):
    return np.stack([noise(41, w, h), blocky_noise(42, w, h), mixed(w, h, 43)])


def rotation_frames(w, h):
    """dense, sparse, flat, mixed"""
    return np.stack([noise(51, w, h), dots(w, h, 3, 3), np.full((h, w), GROUND, np.uint8), mixed(w, h, 53)])


@functools.lru_cache(maxsize=None)
def busy_threshold():
    """The fastTh of (d) and (e): the first from 200 up at which the model finds every cell of every frame of both families empty."""
    frames = [f for w, h in ((300, H), (84, H)) for f in busy_frames(w, h)] + list(rotation_frames(480, H))
    S = [(gm.strength(f), f.shape) for f in frames]
    for th in range(200, 255):
        if all((s[fm.WINDOW:sh[0] - fm.WINDOW, fm.WINDOW:sh[1] - fm.WINDOW] <= th).all() for s, sh in S):
            return th
    raise AssertionError("no threshold leaves every cell empty")


# ---- (f) arc atlas -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def atlas(t):
    """-> (frame, [(cx, cy, v, polarity, length, start)] of the patterns placed, combinations skipped, combinations in all).
    8 x 8 tiles from (16, 16); a tile is flat at its centre value v, the ring of its centre (tile offset 3, 3) holds `length` contiguous
    pixels from ring position `start` at v +- (t + 1) and the others at v +- t."""
    ring = gm.ring()
    combos = [(v, pol, length, start) for v in ATLAS_CENTRES for pol in (1, -1) for length in (9, 8) for start in range(16)]
    kept = [c for c in combos if 0 <= c[0] + c[1] * (t + 1) <= 255]
    sites = [(fm.WINDOW + 8 * i + 3, fm.WINDOW + 8 * j + 3) for j in range((ATLAS_H - 2 * fm.WINDOW) // 8) for i in range((ATLAS_W - 2 * fm.WINDOW) // 8)]
    assert len(kept) <= len(sites)
    img = np.full((ATLAS_H, ATLAS_W), GROUND, np.uint8)
    placed = []
    for (cx, cy), (v, pol, length, start) in zip(sites, kept):
        img[cy - 3:cy + 5, cx - 3:cx + 5] = v
        for k, (dx, dy) in enumerate(ring):
            img[cy + dy, cx + dx] = v + pol * (t + 1 if (k - start) % 16 < length else t)
        placed.append((cx, cy, v, pol, length, start))
    return img, placed, len(combos) - len(kept), len(combos)


# ---- the frames of test_gpu_parity.py::test_fast_modes_give_the_reference_candidates, which the model is held to the oracle on as well ----
def fast_mode_images(synth):
    """Frames that put the per-cell fallback of src/ORBextractor.cc:792-799 in every state: no cell falls back (textured), all do (flat,
    low contrast), some do (textured left half / low-contrast right half; a dim frame), cells whose only corners >= fastTh are
    equal-score neighbours that suppress each other (so `FAST(cell, 20)` is empty although pixels score >= 20, and in the second
    call those pixels still suppress their weaker neighbours), and dense noise."""
    rng = np.random.default_rng(11)
    H, W = 512, 640
    tex = synth.make_frame(4242, W, H)
    low = (rng.integers(0, 12, (H, W)) + 100).astype(np.uint8)
    half = tex.copy()
    half[:, W // 2:] = low[:, W // 2:]
    dim = (tex.astype(np.float32) * 0.22 + 90).astype(np.uint8)   # contrast cut to a fifth: most corners score below 20
    # pairs of identical bright 2x1 blobs on a flat background: both pixels of a pair get the same score and annihilate
    ties = np.full((H, W), 100, np.uint8)
    ties += rng.integers(0, 9, (H, W)).astype(np.uint8)           # weak corners (score >= 7) around them
    for y in range(40, H - 40, 37):
        for x in range(40, W - 40, 41):
            ties[y, x] = ties[y, x + 1] = 190
    noise = rng.integers(0, 256, (H, W), dtype=np.uint8)
    flat = np.full((H, W), 77, np.uint8)
    return (("textured", tex), ("lowcontrast", low), ("half", half), ("dim", dim), ("ties", ties), ("noise", noise), ("flat", flat))


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------
def _batch_order(n):
    return tuple(range(n)) if n >= 3 else tuple(k % n for k in range(3))


@functools.lru_cache(maxsize=None)
def cases():
    c = []
    for w, h in SHAPES:
        c.append(Case("a dots %d x %d" % (w, h), "a", w, h, FAST_TH, 1, dot_frames(w, h), tuple(range(49))))
    for w, h in ((300, H), (430, H)):
        for o in ORIENTATIONS:
            c.append(Case("b pairs %d x %d (%d, %d)" % ((w, h) + o), "b", w, h, FAST_TH, 1, pair_frames(w, h, o), tuple(range(64))))
    c.append(Case("b lone equal pairs 300 x 130", "b", 300, H, FAST_TH, 1, np.stack([lone_pairs(300, H, o) for o in ORIENTATIONS[:3]]), (0, 1, 2)))
    counted = np.stack([f for _, _, f in count_frames()] + [noise(32, 300, H)])
    c.append(Case("c list limits 300 x 130", "c", 300, H, 7, 1, counted, _batch_order(len(counted))))
    for w, h in ((300, H), (84, H)):
        c.append(Case("d busy cells %d x %d" % (w, h), "d", w, h, busy_threshold(), 1, busy_frames(w, h), (0, 1, 2)))
    c.append(Case("e second cell 480 x 130", "e", 480, H, busy_threshold(), 1, rotation_frames(480, H), tuple(k % 4 for k in range(200))))
    for t in ATLAS_THRESHOLDS:
        c.append(Case("f atlas t=%d" % t, "f", ATLAS_W, ATLAS_H, t, 1, atlas(t)[0][None], (0, 0, 0)))
    c.append(Case("g dots 380 x 130, 3 levels", "g", 380, H, FAST_TH, 3, dot_frames(380, H), tuple(range(49))))
    assert len({k.name for k in c}) == len(c)
    return c


NAMES = ("a dots 122 x 130", "a dots 200 x 130", "a dots 300 x 130", "a dots 380 x 130", "a dots 430 x 130", "a dots 480 x 130", "a dots 84 x 130",
         "b pairs 300 x 130 (1, 0)", "b pairs 300 x 130 (0, 1)", "b pairs 300 x 130 (1, 1)", "b pairs 300 x 130 (-1, 1)",
         "b pairs 430 x 130 (1, 0)", "b pairs 430 x 130 (0, 1)", "b pairs 430 x 130 (1, 1)", "b pairs 430 x 130 (-1, 1)",
         "b lone equal pairs 300 x 130", "c list limits 300 x 130", "d busy cells 300 x 130", "d busy cells 84 x 130", "e second cell 480 x 130",
         "f atlas t=6", "f atlas t=7", "f atlas t=8", "f atlas t=20", "f atlas t=21", "f atlas t=128", "g dots 380 x 130, 3 levels")
SINGLE_LEVEL = tuple(n for n in NAMES if not n.startswith("g "))


def by_name(name):
    return next(k for k in cases() if k.name == name)


@functools.lru_cache(maxsize=None)
def expected(name):
    """Per distinct frame of a single-level case: (the model's sorted candidates, its count of fall-back cells), computed once."""
    k = by_name(name)
    assert k.nlevels == 1
    out = []
    for f in k.frames:
        lists = fm.cell_lists(f, k.fast_th)
        out.append((sorted(p for _, _, pts in lists for p in pts), sum(fb for c, fb, _ in lists if c.rw > 6 and c.rh > 6)))
    return out


def owner(level_w, level_h, x, y, rows_per_seg):
    """Who owns the candidate (x, y) of a level of that size: a line for a failure message."""
    regs = fm.plan(level_w, level_h, rows_per_seg)
    ix, iy = x + fm.MIN_BORDER, y + fm.MIN_BORDER
    reg = next((r for r in regs if r.x0 <= ix < r.x1 and r.y0 <= iy < r.y1), None)
    return "pixel (%d, %d): cell (row %d, column %d), %d-row region %s" % ((ix, iy) + fm.cell_of(level_w, level_h, x, y) + (rows_per_seg, reg))


def first_difference(got, want):
    """the first candidate (in sorted order) that one list has and the other has not: (x, y, score), 'missing' | 'invented' | None"""
    g, w = set(got), set(want)
    odd = sorted(g ^ w)
    if not odd:
        return None, ("the same candidates, %d against %d entries: a duplicate" % (len(got), len(want))) if len(got) != len(want) else None
    return odd[0], "invented (not in the model)" if odd[0] in g else "missing (in the model only)"


def handle_verdict(k):
    """tests/emu/geom_emu.cpp: what a handle of max_width x max_height = the case's size and max_batch = its batch decides about that size
    (0: accepted), and the level sizes."""
    import ctypes
    import host_build
    lib = ctypes.CDLL(host_build.build("geom_emu"))
    lib.emu_geom_probe.argtypes = [ctypes.c_int, ctypes.c_float] + [ctypes.c_int] * 7 + [ctypes.c_void_p] * 2
    wh, ok = np.zeros(2 * k.nlevels, np.int32), np.zeros(k.nlevels, np.int32)
    rc = lib.emu_geom_probe(NFEATURES, 1.2, k.nlevels, k.w, k.h, len(k.order), 0, k.w, k.h, wh.ctypes.data, ok.ctypes.data)
    return rc, [tuple(x) for x in wh.reshape(-1, 2).tolist()]
