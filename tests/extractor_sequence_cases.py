"""Scenarios that hold ONE extractor handle to the CPU oracle across changing calls (test_gpu_extractor_sequence.py), and what makes
them able to catch a carry-over (test_extractor_sequence_cases.py, CPU only).

A scenario is a handle configuration (`Cfg`) and an ordered list of steps.  A step names an entry point and its arguments; its expected
result is what the oracle returns for THAT step's arguments alone -- a fresh oracle extractor per step, never another GPU handle:
keypoints as raw 28-byte records, descriptors, the mutated grid where there is one, and per level the FAST candidates and the planes.

The handle of every scenario is 320 x 256 (`MAX_W`, `MAX_H`); the walks use three pyramids:
  1.2  / 4 levels   the project's usual small configuration
  1.33 / 3 levels   the largest scale factor at which every size up to 320 px keeps the 12-byte-window path of k_resize_level on
                    every level (searched exhaustively with tests/emu/geom_emu.cpp: no width from 90 to 320 px loses it)
  1.35 / 3 levels   sizes on both sides of that limit: `resize_fast` -- and with it whether the tile plans exist at all -- differs
                    between consecutive steps of the walk
"""
import collections
import ctypes

import numpy as np

import host_build
import oracle_lib

KP = oracle_lib.KP
MAX_W, MAX_H = 320, 256
FAST_TH = 20

Cfg = collections.namedtuple("Cfg", "nfeatures scale nlevels fast_th max_batch max_input_keypoints")
Cfg.__new__.__defaults__ = (500, 1.2, 4, FAST_TH, 1, 0)

Step = collections.namedtuple("Step", "op name img kin min_px need want_grid extra claims_fallback")
Step.__new__.__defaults__ = (None,) * 3 + (20, 0, False, None, False)

Result = collections.namedtuple("Result", "kp desc grid levels cands planes")
# kp: the records' bytes; desc: (n, 32) uint8; grid: int32 F-order or None; levels: keypoints per level; cands: per level the sorted
# (x, y, response) of the FAST candidates; planes: (last level's plane, its blurred plane or None when the level kept no keypoint)


# ---- frames ----------------------------------------------------------------------------------------------------------
def frame(synth, seed, w, h):
    return synth.make_frame(seed, w, h, n_shapes=max(20, w * h // 600))


def faded(synth, seed, w, h):
    """tools/soak_parity.py kind 5: contrast fading from left to right -- cells that fall back to the literal threshold 7 and cells that do not"""
    img = frame(synth, seed, w, h).astype(np.float32)
    fade = np.linspace(1.0, 0.05, w, dtype=np.float32)[None, :]
    return (img * fade + 110 * (1 - fade)).astype(np.uint8)


def low_contrast(seed, w, h):
    """tools/soak_parity.py kind 4: noise of amplitude 30 around 100 -- hardly a corner at fastTh 20, most cells fall back"""
    return (np.random.default_rng(seed).integers(0, 30, (h, w)) + 100).astype(np.uint8)


def tracked_points(seed, n, w, h):
    rng = np.random.default_rng(seed)
    kin = np.zeros(n, KP)
    kin["x"] = rng.uniform(20, w - 21, n).astype(np.float32)
    kin["y"] = rng.uniform(20, h - 21, n).astype(np.float32)
    kin["size"], kin["angle"], kin["response"], kin["class_id"] = 31, -1, rng.uniform(0, 99, n), np.arange(n)
    return kin


def occupancy_grid(kin, min_px, w, h):
    """Eigen::MatrixXi::Zero(rows / d + 2, cols / d + 2), then grid((int)(y / d), (int)(x / d))++ (src/Tracking.cc:896-907)"""
    grid = np.zeros((h // min_px + 2, w // min_px + 2), np.int32, order="F")
    for k in kin:
        grid[int(np.float32(k["y"]) / np.float32(min_px)), int(np.float32(k["x"]) / np.float32(min_px))] += 1
    return grid


# ---- the size rule ---------------------------------------------------------------------------------------------------
def level_side(side, inv_scale, level):
    """cvRound(size * invScale^l) as src/ORBextractor.cc:966-969 computes it: a float product, rounded half to even"""
    return int(np.rint(np.float32(side) * np.float32(inv_scale[level])))


def smallest_side(inv_scale):
    """smallest square side whose last level still measures 56 px (the lower end of the envelope), from a handle's (or the oracle's)
    own mvInvScaleFactor"""
    last = len(inv_scale) - 1
    side = 56
    while level_side(side, inv_scale, last) < 56:
        side += 1
    return side


_geom = None


def geom_probe(cfg, w, h):
    """tests/emu/geom_emu.cpp: what a 320 x 256 handle of configuration cfg decides about a w x h image, without a device.
    -> (verdict, [(level w, level h)], [fast_ok per level]); verdict 0 = accepted, 1..5 = the capacity exceeded (blocks, FAST scratch,
    column table, row table, quad-tree path tables), -5 = UVO_E_UNSUPPORTED."""
    global _geom
    if _geom is None:
        _geom = ctypes.CDLL(host_build.build("geom_emu"))
        _geom.emu_geom_probe.argtypes = [ctypes.c_int, ctypes.c_float] + [ctypes.c_int] * 7 + [ctypes.c_void_p] * 2
    wh, ok = np.zeros(2 * cfg.nlevels, np.int32), np.zeros(cfg.nlevels, np.int32)
    rc = _geom.emu_geom_probe(cfg.nfeatures, cfg.scale, cfg.nlevels, MAX_W, MAX_H, cfg.max_batch, cfg.max_input_keypoints, w, h, wh.ctypes.data, ok.ctypes.data)
    return rc, [tuple(x) for x in wh.reshape(-1, 2).tolist()], ok.tolist()


def default_tile_plan_on_host(oracle, cfg, img, max_lds=160 * 1024):
    """The tile plan a handle compiles for this image's size by default (default_tile_spec(), csrc/extractor_geom.cpp: one group of
    tiles_for(level-1 width, 34) x tiles_for(level-1 height, 27) tiles), executed on the host by tests/emu/pyr_tiles_emu.cpp, which holds
    every load and store of the plan to the planes and the LDS allocation.  -> (the emulation's verdict: 0 = every property holds,
    2 = a level outside the 12-byte window (no plan: per-level launches), 3 = no plan within the LDS; planes equal the oracle's)"""
    emu = ctypes.CDLL(host_build.build("pyr_tiles_emu"))
    vp, ci = ctypes.c_void_p, ctypes.c_int
    emu.emu_pyr_tiles_run.argtypes = [vp, ci, ci, vp, vp, ci, ci, vp, vp, vp, ctypes.c_uint32, vp, vp, vp, vp]
    oe = oracle.extractor(cfg.nfeatures, cfg.scale, cfg.nlevels, cfg.fast_th)
    oe(img)
    nl = cfg.nlevels
    dims = [oe.level_dims(l) for l in range(nl)]
    lw, lh = np.array([d[0] for d in dims], np.int32), np.array([d[1] for d in dims], np.int32)
    tiles_for = lambda n, target: min(255, max(1, (n + target // 2) // target))
    gf, gx, gy = np.array([1], np.int32), np.array([tiles_for(int(lw[1]), 34)], np.int32), np.array([tiles_for(int(lh[1]), 27)], np.int32)
    pitch = (lw + 32 + 63) // 64 * 64
    planes = np.full(int((pitch.astype(np.int64) * (lh + 32)).sum()), 0xEE, np.uint8)
    off, pitch_out, stats = np.zeros(nl, np.int64), np.zeros(nl, np.int32), np.zeros(3, np.int64)
    img = np.ascontiguousarray(img)
    rc = emu.emu_pyr_tiles_run(img.ctypes.data, img.strides[0], nl, lw.ctypes.data, lh.ctypes.data, 4, 1, gf.ctypes.data, gx.ctypes.data, gy.ctypes.data, max_lds,
                               planes.ctypes.data, off.ctypes.data, pitch_out.ctypes.data, stats.ctypes.data)
    same = rc == 0
    for l in range(1, nl if rc == 0 else 0):
        got = planes[off[l]:off[l] + int(pitch_out[l]) * (int(lh[l]) + 32)].reshape(int(lh[l]) + 32, int(pitch_out[l]))[12:int(lh[l]) + 20, 12:int(lw[l]) + 20]
        same = same and np.array_equal(got, oe.level_plane(l)[12:-12, 12:-12])     # the ROI and the 4-px ring the launch stores
    return rc, same


GEOM_OK, GEOM_CAP_BLOCKS, GEOM_CAP_FAST, GEOM_CAP_XTAB, GEOM_CAP_YTAB, GEOM_CAP_OCT_TAB, GEOM_UNSUPPORTED = 0, 1, 2, 3, 4, 5, -5


# ---- the oracle side of a step ---------------------------------------------------------------------------------------
def _pack(oe, kp, desc, grid, nlevels):
    cands = []
    for l in range(nlevels):
        c = oe.level_candidates(l)
        cands.append(sorted(zip(c["x"].astype(int).tolist(), c["y"].astype(int).tolist(), c["response"].astype(int).tolist())))
    last = nlevels - 1
    blurred = oe.level_plane(last, blurred=True) if (kp["octave"] == last).any() else None   # the oracle blurs only levels that kept keypoints
    return Result(kp.tobytes(), desc, grid, [int((kp["octave"] == l).sum()) for l in range(nlevels)], cands, (oe.level_plane(last), blurred))


def expected(oracle, cfg, step):
    """The oracle's answer to one step (for a batch: a list, one Result per frame)."""
    def fresh():
        return oracle.extractor(cfg.nfeatures, cfg.scale, cfg.nlevels, cfg.fast_th)
    if step.op == "batch":
        out = []
        for img in step.img:
            oe = fresh()
            out.append(_pack(oe, *oe(img), None, cfg.nlevels))
        return out
    if step.op == "grider":
        num, gx, gy, th = step.extra
        return Result(oracle.grider_fast(step.img, num, gx, gy, th).tobytes(), None, None, None, None, None)
    oe = fresh()
    img = oracle.clahe(step.img, 4.0, (12, 12)) if step.op == "clahe_full" else step.img
    h, w = img.shape
    if step.op in ("full", "clahe_full"):
        return _pack(oe, *oe(img), None, cfg.nlevels)
    if step.op == "topup":       # caller keypoints pass through level 0, the grid they filled filters the rest
        grid = occupancy_grid(step.kin, step.min_px, w, h) if step.kin is not None else np.zeros((h // step.min_px + 2, w // step.min_px + 2), np.int32, order="F")
        kp, de = oe(img, None if step.kin is None else step.kin.copy(), grid, step.min_px, False, step.need)
        return _pack(oe, kp, de, grid, cfg.nlevels)
    if step.op == "tracked":     # the tracked points only fill the grid (src/Tracking.cc:943-946: the extractor gets an empty vector)
        grid = occupancy_grid(step.kin, step.min_px, w, h)
        kp, de = oe(img, None, grid, step.min_px, False, step.need)
        return _pack(oe, kp, de, grid, cfg.nlevels)
    raise ValueError(step.op)


def is_extraction(step):
    return step.op != "grider"


# ---- scenarios -------------------------------------------------------------------------------------------------------
WALK_PYRAMIDS = [(1.2, 4), (1.33, 3), (1.35, 3)]
# (w, h) per step: full, half (at 1.35 a size near it whose `resize_fast` differs from both neighbours), a width that is no multiple of 4 (the padded-copy source after an in-place one), the smallest accepted
# square, a wide strip (several quad-tree roots per level), a tall image (one root), full again (size_walk() appends the strip
# and the full size once more: between them only the height changes).  The tall image differs per pyramid: the
# detection window of EVERY level must be at least half as wide as high (nIni >= 1), which 150 x 256 meets at 1.2 / 4 only.
WALK_SIZES = {
    (1.2, 4): [(320, 256), (160, 128), (253, 190), (96, 96), (320, 100), (150, 256), (320, 256)],
    (1.33, 3): [(320, 256), (160, 128), (253, 190), (99, 99), (320, 100), (160, 256), (320, 256)],
    (1.35, 3): [(320, 256), (144, 116), (253, 190), (102, 102), (320, 104), (152, 256), (320, 256)],
}
SMALLEST_SQUARE = {(1.2, 4): 96, (1.33, 3): 99, (1.35, 3): 102}


def walk_cfg(scale, nlevels):
    return Cfg(500, scale, nlevels, FAST_TH, 1, 0)


def size_walk(synth, scale, nlevels):
    steps = []
    sizes = WALK_SIZES[(scale, nlevels)]
    for i, (w, h) in enumerate(sizes[:-1]):
        steps.append(Step("full", "%dx%d" % (w, h), frame(synth, 9100 + i, w, h)))
    steps.append(Step("full", "%dx%d again" % sizes[-1], steps[0].img))
    # and two changes of the height alone: the strip's image again, then the full size with another image
    steps.append(Step("full", "%dx%d again" % sizes[4], steps[4].img))
    steps.append(Step("full", "%dx%d, third image" % sizes[-1], frame(synth, 9190, *sizes[-1])))
    return walk_cfg(scale, nlevels), steps


MODE_CFG = Cfg(500, 1.2, 4, FAST_TH, 1, 64)


def mode_walk(synth, w=MAX_W, h=MAX_H, seed=9200):
    """FullDetect, the top-up forms, CLAHE, Grider_FAST and FullDetect again, on one size."""
    a, b, c = frame(synth, seed, w, h), frame(synth, seed + 1, w, h), faded(synth, seed + 2, w, h)
    kin = tracked_points(seed + 3, 40, w, h)
    return MODE_CFG, [
        Step("full", "1 FullDetect", a),
        Step("topup", "2 top-up with caller keypoints, d 20", b, kin, 20, 150),
        Step("topup", "3 top-up without keypoints, d 5", c, None, 5, 200, claims_fallback=True),
        Step("tracked", "4a extract_tracked with the grid", a, kin, 20, 120, True),
        Step("tracked", "4b extract_tracked without the grid", b, kin[:17], 10, 90, False),
        Step("clahe_full", "5 clahe then ex(None)", c),
        Step("grider", "6 grider_fast", a, extra=(60, 5, 4, 20)),
        Step("full", "7 FullDetect again", a),
        Step("topup", "8 top-up with a negative budget", b, kin, 20, -5),
    ]


def mode_walk_small(synth):
    """The same walk on a second size of the same handle (a width that is no multiple of 4: every call takes the padded copy)."""
    return mode_walk(synth, 253, 190, 9300)


ADAPT_CFG = Cfg(500, 1.2, 4, FAST_TH, 1, 0)


def adaptive_walk(synth):
    """A low-contrast frame between normal ones: with UVO_TUNE_FAST_MODE adaptive the per-level pass threshold flips to 7 and back."""
    n1, n2 = frame(synth, 9400, MAX_W, MAX_H), frame(synth, 9401, MAX_W, MAX_H)
    return ADAPT_CFG, [
        Step("full", "normal", n1),
        Step("full", "faded", faded(synth, 9402, MAX_W, MAX_H), claims_fallback=True),
        Step("full", "low contrast", low_contrast(9403, MAX_W, MAX_H)),
        Step("full", "normal again", n2),
    ]


BATCH_SIZES = [1, 2, 3, 8, 9, 16, 17, 20, 1]     # both sides of kFewFrames (2), kTilePyramidFrames (8) and kSmallBatch (16)
BATCH_CFG = Cfg(300, 1.2, 4, FAST_TH, 20, 0)
BATCH_W, BATCH_H = 160, 128


def batch_walk(synth):
    """Every frame of every batch is another image (seeds never repeat), all at the half size of the handle."""
    steps, seed = [], 9500
    for n in BATCH_SIZES:
        steps.append(Step("batch", "batch of %d" % n, np.stack([frame(synth, seed + i, BATCH_W, BATCH_H) for i in range(n)])))
        seed += n
    return BATCH_CFG, steps


def pipeline_batches(synth):
    """A (full size), B (half size), C (full size) for the two-lane submit / wait walk, then one frame for the synchronous call."""
    a = np.stack([frame(synth, 9600 + i, MAX_W, MAX_H) for i in range(3)])
    b = np.stack([frame(synth, 9610 + i, BATCH_W, BATCH_H) for i in range(5)])
    c = np.stack([frame(synth, 9620 + i, MAX_W, MAX_H) for i in range(2)])
    return BATCH_CFG, [Step("batch", "A 3 x full", a), Step("batch", "B 5 x half", b), Step("batch", "C 2 x full", c),
                       Step("batch", "synchronous", frame(synth, 9630, MAX_W, MAX_H)[None])]


# two handles on one device: A's level-0 quota puts the quad-tree's dynamic LDS above 64 KiB, B's stays far below
BIG_CFG = Cfg(1600, 1.2, 2, FAST_TH, 1, 0)
SMALL_CFG = Cfg(300, 1.2, 4, FAST_TH, 1, 0)


def octree_lds(quota, level_sizes):
    """octree_lds() of csrc/octree.hip, restated: bytes of dynamic LDS the quad-tree kernel asks for with these per-level quotas and sizes"""
    M, pyr_words = 0, 0
    for q, (w, h) in zip(quota, level_sizes):
        n_ini = int(np.rint(np.float32(w - 26) / np.float32(h - 26)))          # roundf(bw / bh): no tie occurs at the sizes used here
        M = max(M, (max(int(q), 4 * n_ini) + 8 + 3) & ~3)
        depth = 5 if n_ini <= 4 else (4 if n_ini <= 16 else (3 if n_ini <= 64 else 0))
        pyr_words = max(pyr_words, sum(n_ini * 4 ** g for g in range(depth + 1)))
    Mp2 = 1
    while Mp2 < M:
        Mp2 <<= 1
    box_region = (max(16 * M, 4 * (pyr_words + 16)) + 15) & ~15
    return 32 * M + box_region + 28 * M + 4 * Mp2 + 4 * 48


def two_handle_frames(synth):
    return [frame(synth, 9700 + i, MAX_W, MAX_H) for i in range(4)]


def all_scenarios(synth):
    """name -> (cfg, steps), everything the GPU tests run"""
    out = collections.OrderedDict()
    for scale, nlevels in WALK_PYRAMIDS:
        out["size walk %.2f / %d" % (scale, nlevels)] = size_walk(synth, scale, nlevels)
    out["mode walk 320 x 256"] = mode_walk(synth)
    out["mode walk 253 x 190"] = mode_walk_small(synth)
    out["adaptive walk"] = adaptive_walk(synth)
    out["batch walk"] = batch_walk(synth)
    out["pipeline walk"] = pipeline_batches(synth)
    fr = two_handle_frames(synth)
    out["two handles, large quota"] = (BIG_CFG, [Step("full", "A %d" % i, f) for i, f in enumerate(fr)])
    out["two handles, small quota"] = (SMALL_CFG, [Step("full", "B %d" % i, f) for i, f in enumerate(fr)])
    return out


# ---- the literal-7 fall-back, per cell ---------------------------------------------------------------------------------
def fallback_cells(oracle, cfg, img):
    """Per level (cells that hold a candidate scoring >= fastTh, cells whose candidates all score 7 .. fastTh - 1), from the candidates of
    oracle extractors built with fastTh and with 7, binned into the level's FAST cell grid (30-px cells over the detection window,
    src/ORBextractor.cc:755-770; a cell's FAST call finds corners from 3 px inside its ROI, so cell j owns x - 3 in [j, j + 1) * wCell).  The oracle exposes no per-cell flag: a cell of the second kind can only have been filled by the
    literal-7 pass."""
    o_th, o_7 = oracle.extractor(cfg.nfeatures, cfg.scale, cfg.nlevels, cfg.fast_th), oracle.extractor(cfg.nfeatures, cfg.scale, cfg.nlevels, 7)
    o_th(img), o_7(img)
    out = []
    for l in range(cfg.nlevels):
        w, h = o_th.level_dims(l)
        bw, bh = w - 26, h - 26
        n_cols, n_rows = int(np.float32(bw) / np.float32(30)), int(np.float32(bh) / np.float32(30))
        w_cell, h_cell = -(-bw // n_cols), -(-bh // n_rows)
        hi, lo7 = set(), set()
        for c in o_th.level_candidates(l):
            cell = (min((int(c["y"]) - 3) // h_cell, n_rows - 1), min((int(c["x"]) - 3) // w_cell, n_cols - 1))
            if c["response"] >= cfg.fast_th:
                hi.add(cell)
        for c in o_7.level_candidates(l):
            cell = (min((int(c["y"]) - 3) // h_cell, n_rows - 1), min((int(c["x"]) - 3) // w_cell, n_cols - 1))
            if 7 <= c["response"] < cfg.fast_th:
                lo7.add(cell)
        out.append((hi, lo7 - hi, n_rows * n_cols))
    return out
