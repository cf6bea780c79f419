"""Candidate lists for the quad-tree kernel (csrc/octree.hip: k_octree<256>, k_octree<1024>), injected through
uvo_extractor_octree_tap instead of grown from images, and the references they are held to.  tests/test_octree_cases.py proves on the
CPU which path of octree_body every problem takes for each workgroup size; tests/test_gpu_octree.py runs the same batches on the device.

A Batch is what one tap call gets: problems[frame][level] = Problem(high list, low list, cell flags of the level).  Device lists come in
two VARIANTS of every batch -- two orders of the arrays, and in the second a random half of a problem's free high entries handed over to
the low list -- which must both give the answer of the reference.

The references:
  selection   the literal std::list restatement of DistributeOctTree, oracle.extractor(...).octree(points, W, H, N), points in the
              reference's candidate order (reference_order: cell-major, raster inside a cell)
  gather      gather(): a few lines of numpy from the comment in octree_body -- the high list plus every low entry with score >= 7 whose
              cell's flag is zero; fcount = the zero flags at grid positions that are cells

What each case would catch is said where it is built."""
import collections
import ctypes
import functools

import numpy as np

import host_build

SCALE = 1.2
NLEVELS = 4
# name -> (width, height, nfeatures): every handle has 4 levels at 1.2 and max_batch 3
HANDLES = {
    "main": (320, 256, 500),      # level 0: window 294 x 230, quota 161 -- the window and quota the path-taking sets were probed at
    "three": (320, 256, 10),      # level 0: quota 3
    "big": (320, 256, 2500),      # level 0: quota 805: node tables past 64 KiB of LDS
    "wide": (400, 100, 200),      # level 0: window 374 x 74, nIni = 5, a count pyramid of depth 4
    "small": (160, 120, 500),     # grids of 4 x 3 down to 2 x 1 cells; level 3 has nIni = 2
}
# A grid position that is no cell needs (nCols - 1) * wCell >= bw - 6 with wCell = ceil(bw / nCols) >= 30, i.e. nCols >= 25: a window of
# 750 pixels or more.  None of these sizes has one (test_octree_cases.py asserts it), so fcount's correction term nRows * nCols - n_cells
# is zero in every case here.

Level = collections.namedtuple("Level", "w h bw bh nCols nRows wCell hCell n_cells quota cand_cap nIni sel_cap flag_base is_cell")
Problem = collections.namedtuple("Problem", "hi lo flags movable")   # hi, lo: (n, 3) int arrays of (x, y, score); flags: (nRows, nCols) uint8
Batch = collections.namedtuple("Batch", "name handle problems aim catches")  # aim: {(frame, level): {256: path, 1024: path}}

PYRAMID, RUN8, RUN0, EMPTY = "run_pyramid", "run<8>", "run<0>", "empty"


# ---- geometry ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def levels(handle):
    """tests/emu/geom_emu.cpp: the levels of the handle's image size as build_geom() lays them out"""
    w, h, nfeatures = HANDLES[handle]
    lib = ctypes.CDLL(host_build.build("geom_emu"))
    lib.emu_geom_levels.argtypes = [ctypes.c_int, ctypes.c_float] + [ctypes.c_int] * 3 + [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    lv, is_cell = np.zeros(16 * NLEVELS, np.int32), np.zeros(1 << 16, np.uint8)
    n = lib.emu_geom_levels(nfeatures, SCALE, NLEVELS, w, h, lv.ctypes.data, is_cell.ctypes.data, len(is_cell))
    assert 0 < n <= len(is_cell), n
    out = []
    for l in range(NLEVELS):
        v = [int(x) for x in lv[16 * l:16 * l + 14]]
        out.append(Level(*v, is_cell[v[13]:v[13] + v[4] * v[5]].reshape(v[5], v[4]).copy()))
    return tuple(out)


def flags_per_frame(handle):
    return sum(L.nRows * L.nCols for L in levels(handle))


def carve(handle):
    """-> (M, pyr_words) of octree_lds() in csrc/octree.hip: the node capacity and the count-pyramid words every level of the handle is
    carved with (the largest of its levels, M rounded as oct_capacity() rounds)"""
    lv = levels(handle)
    depth = lambda n: 5 if n <= 4 else 4 if n <= 16 else 3 if n <= 64 else 0
    return (max(((max(L.quota, 4 * L.nIni) + 8 + 3) & ~3) for L in lv),
            max(sum(L.nIni * 4 ** g for g in range(depth(L.nIni) + 1)) for L in lv))


def lds_bytes(handle):
    """oct_lds_bytes() of csrc/octree.hip for the handle: M = the largest node table of its levels, rounded as oct_capacity() rounds"""
    M, pyr_words = carve(handle)
    Mp2 = 1 << (M - 1).bit_length()
    box = (max(16 * M, 4 * (pyr_words + 16)) + 15) & ~15
    return 32 * M + box + 28 * M + 4 * Mp2 + 4 * (32 + 16)


def cell_of(L, x, y):
    return np.minimum((np.asarray(y) - 3) // L.hCell, L.nRows - 1), np.minimum((np.asarray(x) - 3) // L.wCell, L.nCols - 1)


def reference_order(pts, nCols, nRows, wCell, hCell):
    """the rows of pts (x, y, ...) in the reference's candidate order: cell-major, raster inside a cell"""
    pts = np.asarray(pts)
    j = np.minimum((pts[:, 0] - 3) // wCell, nCols - 1)
    i = np.minimum((pts[:, 1] - 3) // hCell, nRows - 1)
    return pts[np.lexsort((pts[:, 0], pts[:, 1], j, i))]


def gather(L, p):
    """-> (candidates (n, 3), fcount) of one problem, from the comment in octree_body"""
    ci, cj = cell_of(L, p.lo[:, 0], p.lo[:, 1])
    keep = (p.lo[:, 2] >= 7) & (p.flags[ci, cj] == 0)
    return np.concatenate([p.hi, p.lo[keep]]), int(((p.flags == 0) & (L.is_cell != 0)).sum())


# ---- builders ---------------------------------------------------------------------------------------------------------------------------
def _arr(rows):
    return np.asarray(rows, np.int64).reshape(-1, 3)


def _scored(xy, rng, score=None):
    xy = np.asarray(xy, np.int64).reshape(-1, 2)
    sc = np.full(len(xy), score) if score is not None else rng.integers(7, 200, len(xy))
    return np.concatenate([xy, sc[:, None]], 1)


def _block(x0, y0, bw, bh):
    ys, xs = np.mgrid[y0:y0 + bh, x0:x0 + bw]
    return np.stack([xs.ravel(), ys.ravel()], 1)


def _uniform(L, n, rng):
    p = rng.permutation((L.bw - 6) * (L.bh - 6))[:n]
    return np.stack([3 + p % (L.bw - 6), 3 + p // (L.bw - 6)], 1)


def _free(L, pts=None):
    """a problem whose entries all start in the high list, flags zero: free to move to the low list"""
    return Problem(_arr([] if pts is None else pts), _arr([]), np.zeros((L.nRows, L.nCols), np.uint8), True)


def _single(name, handle, pts, aim256, aim1024, catches, level=0):
    lv = levels(handle)
    return Batch(name, handle, [[_free(L, pts if l == level else None) for l, L in enumerate(lv)]], {(0, level): {256: aim256, 1024: aim1024}}, catches)


def _boundary_problem(L, rng, parity):
    """low entries on both sides of every cell boundary in x and in y (x - 3 = k * wCell - 1 and k * wCell), scores 6 / 7 / 255 in turn,
    flags in a chessboard; the high list is a few random points elsewhere"""
    xs = sorted({3 + k * L.wCell + d for k in range(L.nCols + 1) for d in (-1, 0) if 3 <= 3 + k * L.wCell + d < L.bw - 3})
    ys = sorted({3 + k * L.hCell + d for k in range(L.nRows + 1) for d in (-1, 0) if 3 <= 3 + k * L.hCell + d < L.bh - 3})
    lo = np.array([(x, y) for y in ys for x in xs], np.int64)
    lo = np.concatenate([lo, np.array([6, 7, 255])[np.arange(len(lo)) % 3][:, None]], 1)
    taken = {(int(x), int(y)) for x, y, _ in lo}
    hi = np.array([q for q in _uniform(L, 40, rng).tolist() if tuple(q) not in taken], np.int64).reshape(-1, 2)
    ii, jj = np.mgrid[0:L.nRows, 0:L.nCols]
    return Problem(_scored(hi, rng), lo[rng.permutation(len(lo))], (((ii + jj) & 1) == parity).astype(np.uint8), False)


def _lo_only(L, n, rng, flag_cells=()):
    """n low entries, scores 7 .. 255, no high list; the listed cells' flags set"""
    fl = np.zeros((L.nRows, L.nCols), np.uint8)
    for i, j in flag_cells:
        fl[i, j] = 1
    return Problem(_arr([]), _scored(_uniform(L, n, rng), rng), fl, False)


@functools.lru_cache(maxsize=None)
def batches():
    rng = np.random.default_rng(20240607)
    m0, w0, b0, t0 = levels("main")[0], levels("wide")[0], levels("big")[0], levels("three")[0]
    N = m0.quota
    row = np.stack([np.arange(3, m0.bw - 3), np.full(m0.bw - 6, 57)], 1)
    ties3 = np.concatenate([_uniform(m0, 3000, rng), rng.integers(1, 4, 3000)[:, None]], 1)
    out = [
        # ---- the paths: sets that leave the closed form, by list length ----
        _single("row", "main", _scored(row, rng), RUN8, RUN8,
                "adjacent pixels in one row: no FAST frame has them (NMS).  x splits only, the tree is as deep as the row is long: run<8> with "
                "the register state, the careful rounds and their rank sort on the device, frozen single points in many generations"),
        _single("diagonal", "main", _scored(np.stack([np.arange(3, m0.bh - 3)] * 2, 1), rng), RUN8, RUN8,
                "one child per split in x AND y: a wrong child digit or box corner in run<8> moves every later generation"),
        _single("band of 8 rows", "main", _scored(_block(3, 100, m0.bw - 6, 8), rng), RUN0, RUN8,
                "2304 candidates: past 8 x 256, so k_octree<256> keeps the state words in pstate (HBM) while k_octree<1024> still has registers; "
                "a wrong P <= 8 * NT test, or a pstate offset that ignores cand_off, shows here"),
        _single("band of 29 rows", "main", _scored(_block(3, 100, m0.bw - 6, 29), rng), RUN0, RUN0,
                "8352 candidates: past 8 x 1024 too, run<0> in both forms; kRt = ceil(P / NT) trips of the point loop"),
        _single("random, P = quota", "main", _scored(_uniform(m0, N, rng), rng), RUN8, RUN8,
                "as many points as nodes wanted: every close pair needs a deep split, the tree ends below the pyramid with P just reaching N"),
        _single("random, P = quota + 9", "main", _scored(_uniform(m0, N + 9, rng), rng), RUN8, RUN8,
                "nine to spare: the careful round is truncated (ST_UNPROC parents keep their slot behind the new generation)"),
        # ---- the control group: the closed form ----
        _single("random 200", "main", _scored(_uniform(m0, 200, rng), rng), PYRAMID, PYRAMID, "closed form, short list: path arithmetic per candidate (no tables: P <= 2 (W + H))"),
        _single("random 400", "main", _scored(_uniform(m0, 400, rng), rng), PYRAMID, PYRAMID, "closed form, still without the path tables"),
        _single("random 9000", "main", _scored(_uniform(m0, 9000, rng), rng), PYRAMID, PYRAMID,
                "closed form WITH the ready-made path tables (P > 2 (W + H)): tab_src, its offset per level and the dword copy into LDS"),
        _single("block 20 x 20", "main", _scored(_block(100, 90, 20, 20), rng), PYRAMID, PYRAMID,
                "400 adjacent pixels inside one depth-5 bin: the node count stops growing, the loop ends with ONE point -- a form that goes on "
                "splitting, or falls back, gives more"),
        _single("two adjacent", "main", _scored([[100, 100], [101, 100]], rng), PYRAMID, PYRAMID, "one node of two points: the better one out"),
        _single("one pixel", "main", _scored([[17, 200]], rng), PYRAMID, PYRAMID, "P = 1: the clamped look-ahead loads of the candidate passes read entry P - 1 = 0"),
        _single("empty", "main", _arr([]), EMPTY, EMPTY, "P = 0: sel_count 0 and an early return before any LDS table exists"),
        # ---- ties ----
        _single("row, every score 50", "main", _scored(row, rng, 50), RUN8, RUN8,
                "every node's best is a tie: the first in the REFERENCE's candidate order wins, and the device array is in another order -- an "
                "order key built from the wrong cell size, or a winner taken by array position, picks another pixel"),
        _single("random 3000, scores 1 .. 3", "main", ties3, PYRAMID, PYRAMID,
                "ties inside the closed form's nodes: there the winner's coordinates are decoded back out of the order key (the 24-bit reciprocal "
                "division by the cell size on the way in)"),
        # ---- a quota below the first pass ----
        _single("quota 3", "three", _scored(_uniform(t0, 500, rng), rng), PYRAMID, PYRAMID,
                "the first pass splits the root whatever the quota: 4 points for a quota of 3; a kernel that tests the quota first gives 1"),
        # ---- node tables past 64 KiB ----
        _single("big: row", "big", _scored(np.stack([np.arange(3, b0.bw - 3), np.full(b0.bw - 6, 57)], 1), rng), RUN8, RUN8,
                "P < N: every node ends as a single point, 288 out -- on a handle whose LDS request needs the raised limit (a launch that fails, or a "
                "carve sized for another M, shows here)"),
        _single("big: random 6000", "big", _scored(_uniform(b0, 6000, rng), rng), PYRAMID, PYRAMID,
                "805 nodes: the rank sort over more keys than threads in the 256-thread form, Mp2 = 1024"),
        # ---- nIni = 5: a pyramid of depth 4 ----
        _single("wide: clusters", "wide", _scored(np.concatenate([_block(10 + 30 * k, 8 + 6 * (k % 9), 3, 3) for k in range(12)]), rng), RUN8, RUN8,
                "five roots, pyramid depth 4: twelve 3 x 3 clusters need splits below it; hX = 74.8 is no integer (the root of x, the root boxes)"),
        _single("wide: random 3000", "wide", _scored(_uniform(w0, 3000, rng), rng), PYRAMID, PYRAMID, "five roots in the closed form, path tables of 374 + 74 entries"),
        _single("wide: row", "wide", _scored(np.stack([np.arange(3, w0.bw - 3), np.full(w0.bw - 6, 30)], 1), rng), PYRAMID, PYRAMID,
                "the row that leaves the closed form at 294 x 230 stays inside it here: 80 x-bins of depth 4 against a quota of 64"),
    ]
    out += [_mixed(rng), _gather_boundaries(rng)] + _gather_trips(rng) + [_gather_small(rng)]
    return tuple(out)


def _mixed(rng):
    """three frames x four levels, every problem its own list: deep, shallow and empty side by side, the upper levels with their own smaller
    windows and quotas while the LDS carve is sized by level 0 (pr.M = Mmax)"""
    lv = levels("main")
    rowl = lambda L, y: np.stack([np.arange(3, L.bw - 3), np.full(L.bw - 6, y)], 1)
    f0 = [_free(lv[0], _scored(rowl(lv[0], 120), rng)), _free(lv[1], _scored(_uniform(lv[1], 3000, rng), rng)), _free(lv[2]),
          _free(lv[3], _scored(np.stack([np.arange(3, lv[3].bh - 3)] * 2, 1), rng))]
    f1 = [_free(lv[0]), _free(lv[1], _scored(rowl(lv[1], 40), rng, 50)), _free(lv[2], _scored(_block(3, 30, lv[2].bw - 6, 12), rng)),
          _free(lv[3], _scored(_uniform(lv[3], 2500, rng), rng))]
    f2 = [_free(lv[0], _scored(_uniform(lv[0], 5000, rng), rng)), _free(lv[1], _scored([[5, 5]], rng)),
          _free(lv[2], _scored(_uniform(lv[2], lv[2].quota + 5, rng), rng)), _free(lv[3], _scored(_block(20, 20, 9, 9), rng))]
    aim = {(0, 0): {256: RUN8, 1024: RUN8}, (0, 1): {256: PYRAMID, 1024: PYRAMID}, (0, 2): {256: EMPTY, 1024: EMPTY}, (0, 3): {256: RUN8, 1024: RUN8},
           (1, 0): {256: EMPTY, 1024: EMPTY}, (1, 1): {256: RUN8, 1024: RUN8}, (1, 2): {256: RUN0, 1024: RUN8}, (1, 3): {256: PYRAMID, 1024: PYRAMID},
           (2, 0): {256: PYRAMID, 1024: PYRAMID}, (2, 1): {256: PYRAMID, 1024: PYRAMID}, (2, 2): {256: RUN8, 1024: RUN8}, (2, 3): {256: PYRAMID, 1024: PYRAMID}}
    return Batch("mixed batch", "main", [f0, f1, f2], aim,
                 "the grid's (frame, level) -> problem mapping, cand_off / sel_off / oct_tab_off of the upper levels, a level's own W, H, quota and cells "
                 "under the handle's Mmax; an empty problem between two deep ones must not leave state behind (one LDS allocation per workgroup)")


def _gather_boundaries(rng):
    lv = levels("main")
    none = {256: None, 1024: None}
    return Batch("gather: cell boundaries", "main", [[_boundary_problem(L, rng, 0) for L in lv], [_boundary_problem(L, rng, 1) for L in lv]],
                 {(f, l): none for f in range(2) for l in range(4)},
                 "the cell of a low entry by the 24-bit reciprocal (inv_wcell, inv_hcell) on both sides of every boundary, the clamp of the last "
                 "column and row, flag_base of the upper levels and flags_per_frame of the second frame (the chessboard inverted there), the "
                 "literal 7 from both sides (6 is dropped, 7 and 255 are kept), fcount per (frame, level)")


def _gather_trips(rng):
    L = levels("main")
    e = lambda l: _free(L[l])
    one = lambda n, **kw: [_lo_only(L[0], n, rng, **kw), e(1), e(2), e(3)]
    none = {256: None, 1024: None}
    return [Batch("gather: n_lo = %s" % name, "main", [one(n, flag_cells=fc)], {(0, 0): none}, why)
            for name, n, fc, why in (("1", 1, (), "one low entry and no high list: a single lane of the first trip of the load loop"),
                                     ("8 x 256", 2048, ((0, 0), (3, 4)), "exactly one trip of the eight-deep load loop of k_octree<256>; two cells flagged"),
                                     ("8 x 256 + 1", 2049, ((0, 0), (3, 4)), "one entry into the second trip: seven of eight loads of one lane are past the list"),
                                     ("8 x 1024", 8192, ((6, 8),), "exactly one trip of k_octree<1024>"),
                                     ("8 x 1024 + 1", 8193, ((6, 8),), "one entry into its second trip"))]


def _gather_small(rng):
    lv = levels("small")
    none = {256: None, 1024: None}
    hi_only = lambda L: Problem(_scored(_uniform(L, 30, rng), rng), _arr([]), np.ones((L.nRows, L.nCols), np.uint8), False)
    return Batch("gather: 160 x 120", "small", [[_boundary_problem(L, rng, 1) for L in lv], [hi_only(L) for L in lv]],
                 {(f, l): none for f in range(2) for l in range(4)},
                 "grids of 4 x 3 down to 2 x 1 cells (fewer flags than lanes of one wavefront); a frame with every flag set and no low list: "
                 "fcount 0 and the high list alone")


def by_name(name):
    return {b.name: b for b in batches()}[name]


# The batches' names, written out: the test modules parametrise over them when they are COLLECTED, and building the batches loads
# libgeom_emu.so -- a HIP-compiled library, which brings the system's HIP runtime into the process.  In a GPU run that must not happen
# before the `uvo` fixture has let torch initialise its own copy (tests/conftest.py): afterwards no device is found by anybody.
NAMES = ("row", "diagonal", "band of 8 rows", "band of 29 rows", "random, P = quota", "random, P = quota + 9", "random 200", "random 400",
         "random 9000", "block 20 x 20", "two adjacent", "one pixel", "empty", "row, every score 50", "random 3000, scores 1 .. 3", "quota 3",
         "big: row", "big: random 6000", "wide: clusters", "wide: random 3000", "wide: row", "mixed batch", "gather: cell boundaries",
         "gather: n_lo = 1", "gather: n_lo = 8 x 256", "gather: n_lo = 8 x 256 + 1", "gather: n_lo = 8 x 1024", "gather: n_lo = 8 x 1024 + 1",
         "gather: 160 x 120")


def names():
    return list(NAMES)


# ---- device lists -----------------------------------------------------------------------------------------------------------------------
VARIANTS = (0, 1)


def device_lists(batch, variant):
    """-> (problems[frame][level] = (hi, lo), flags (frames, flags_per_frame) uint8) as the tap takes them.  Variant 0: both lists of every
    problem in one random order; variant 1: in another, and a random half of a free problem's entries with score >= 7 moved to the low list
    (its flags are zero: they come back behind the high ones, in whatever order the wavefronts arrive)."""
    rng = np.random.default_rng(77 + variant)
    lv = levels(batch.handle)
    problems, flags = [], np.zeros((len(batch.problems), flags_per_frame(batch.handle)), np.uint8)
    for f, frame in enumerate(batch.problems):
        row = []
        for L, p in zip(lv, frame):
            hi, lo = p.hi[rng.permutation(len(p.hi))], p.lo[rng.permutation(len(p.lo))]
            if variant == 1 and p.movable:
                move = (hi[:, 2] >= 7) & (rng.random(len(hi)) < 0.5)
                hi, lo = hi[~move], np.concatenate([lo, hi[move]])
            row.append((hi, lo))
            flags[f, L.flag_base:L.flag_base + L.nRows * L.nCols] = p.flags.ravel()
        problems.append(row)
    return problems, flags


# ---- references -------------------------------------------------------------------------------------------------------------------------
_expected = {}


def expected(oracle, batch):
    """-> {(frame, level): (selected [(x, y, score)] in list order, cand_count, fcount, candidates in reference order)}, computed once"""
    if batch.name not in _expected:
        w, h, nfeatures = HANDLES[batch.handle]
        e = oracle.extractor(nfeatures, SCALE, NLEVELS, 20)
        lv = levels(batch.handle)
        out = {}
        for f, frame in enumerate(batch.problems):
            for l, (L, p) in enumerate(zip(lv, frame)):
                cand, fcount = gather(L, p)
                cand = reference_order(cand, L.nCols, L.nRows, L.wCell, L.hCell)
                sel = e.octree(cand, L.bw, L.bh, int(e.quota[l])).tolist() if len(cand) else []
                out[(f, l)] = ([tuple(s) for s in sel], len(cand), fcount, cand)
        _expected[batch.name] = out
    return _expected[batch.name]


# ---- the host emulation of the kernel body: which path a list takes -----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _emu(nt):
    E = ctypes.CDLL(host_build.build("octree_emu" if nt == 256 else "octree_emu_1024"))
    E.emu_octree_algo.argtypes = [ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int] * 8 + [ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int] * 3
    E.emu_octree_device_shape.argtypes = E.emu_octree_algo.argtypes + [ctypes.c_int] * 2
    return E


def emulate(nt, L, cand, N, k_regs, algo, handle=None):
    """tests/emu/octree_emu.cpp with phases of nt threads on the candidates cand (n, 3) in the given array order -> (return value, selected).
    handle: in the device's shape -- one block carved as octree_body carves its LDS, with the HANDLE's node capacity and pyramid words
    (more than the level's own on upper levels), and the path tables ready-made in memory"""
    P = len(cand)
    xy = (cand[:, 0].astype(np.uint32) | (cand[:, 1].astype(np.uint32) << 16)).astype(np.uint32)
    sc = cand[:, 2].astype(np.uint32)
    sxy, ssc = np.zeros(N + 16 + P, np.uint32), np.zeros(N + 16 + P, np.uint32)
    args = (xy.ctypes.data, sc.ctypes.data, P, N, L.bw, L.bh, L.nCols, L.nRows, L.wCell, L.hCell, sxy.ctypes.data, ssc.ctypes.data, len(sxy), k_regs, algo)
    m = _emu(nt).emu_octree_algo(*args) if handle is None else _emu(nt).emu_octree_device_shape(*args, *carve(handle))
    return m, [(int(v & 0xffff), int(v >> 16), int(s)) for v, s in zip(sxy[:max(m, 0)], ssc[:max(m, 0)])]


def path(nt, L, cand, N):
    """the branch octree_body<nt> takes on these candidates: emu_octree_algo(algo = 1) returns -2 exactly when the closed form gives up"""
    if len(cand) == 0:
        return EMPTY
    if emulate(nt, L, cand, N, 0, 1)[0] != -2:
        return PYRAMID
    return RUN8 if len(cand) <= 8 * nt else RUN0
