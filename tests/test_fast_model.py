"""The numpy model of the FAST stage (tests/fast_model.py) held to the C++ oracle and to the strip plan of csrc/strip_plan.hpp, and the
committed cases (tests/fast_cases.py) held to what each is named for.  No GPU: this shows that tests/test_gpu_fast.py looks where
csrc/fast.hip can go wrong, and that a model with one deliberate mistake would not pass it."""
import ctypes

import numpy as np
import pytest

import fast_cases as fc
import fast_model as fm
import grider_model as gm
import host_build

FL_CAP = 320                      # csrc/fast.hip: corner records a wavefront keeps in LDS
CCAP = {48: 256, 66: 512}         # FcGeom<MAXROI>::CCAP


def _oracle_candidates(oe, level):
    c = oe.level_candidates(level)
    return sorted(zip(c["x"].astype(int).tolist(), c["y"].astype(int).tolist(), c["response"].astype(int).tolist()))


def _max_roi(w, h):
    _, _, w_cell, h_cell = fm.grid(w, h)
    return max(w_cell, h_cell) + 6


def _interior_corners(S, c, t=7):
    return int((S[c.y0 + 3:c.y0 + c.rh - 3, c.x0 + 3:c.x0 + c.rw - 3] > t).sum())


# ---- the model against the oracle --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["textured", "half", "dim", "ties", "noise", "flat"])
def test_level_candidates_equal_the_oracle_on_the_fast_mode_images(oracle, synth, kind):
    img = dict(fc.fast_mode_images(synth))[kind]
    oe = oracle.extractor(1000, 1.2, 1, 20)
    oe(img)
    assert fm.level_candidates(img, 20) == _oracle_candidates(oe, 0), kind


@pytest.mark.parametrize("name", ["a dots 122 x 130", "a dots 84 x 130", "b pairs 430 x 130 (-1, 1)", "b lone equal pairs 300 x 130", "c list limits 300 x 130",
                                  "d busy cells 300 x 130", "d busy cells 84 x 130", "e second cell 480 x 130", "f atlas t=6", "f atlas t=128"])
def test_level_candidates_equal_the_oracle_on_the_cases(oracle, name):
    k = fc.by_name(name)
    oe = oracle.extractor(fc.NFEATURES, 1.2, 1, k.fast_th)
    for i in sorted({0, len(k.frames) // 2, len(k.frames) - 1}):
        oe(k.frames[i])
        assert fc.expected(name)[i][0] == _oracle_candidates(oe, 0), (name, i)


def test_level_candidates_equal_the_oracle_on_three_levels(oracle):
    k = fc.by_name("g dots 380 x 130, 3 levels")
    oe = oracle.extractor(fc.NFEATURES, 1.2, k.nlevels, k.fast_th)
    oe(k.frames[17])
    for l in range(k.nlevels):
        plane = oe.level_plane(l)[16:-16, 16:-16]
        assert plane.shape[::-1] == oe.level_dims(l)
        want = _oracle_candidates(oe, l)
        assert fm.level_candidates(plane, k.fast_th) == want and len(want) > 50, l


# ---- the plan against the C++ --------------------------------------------------------------------------------------------------------------
def _level_sizes():
    sizes = {(k.w, k.h) for k in fc.cases()}
    for k in fc.cases():
        if k.nlevels > 1:
            sizes |= set(fc.handle_verdict(k)[1])
    return sorted(sizes)


def test_plan_equals_the_cpp_plan():
    lib = ctypes.CDLL(host_build.build("strip_plan_emu"))
    lib.emu_strip_plan_items.argtypes = [ctypes.c_int] * 3 + [ctypes.c_void_p] * 2 + [ctypes.c_int]
    sizes = _level_sizes()
    assert (264, 90) in sizes and len(sizes) == 10                      # the third level of (g)
    for w, h in sizes:
        for rps in (6, 24):
            head, items = np.zeros(7, np.int32), np.zeros((256, 3), np.int32)
            n = lib.emu_strip_plan_items(w - 32, h - 32, rps, head.ctypes.data, items.ctypes.data, 256)
            nfull, nseg, n_items, sub, x0 = fm.strip_plan(w - 32, h - 32, rps)
            assert head.tolist() == [nfull, nseg, n_items] + sub + x0 and n == n_items <= 256, (w, h, rps)
            assert [tuple(r) for r in items[:n].tolist()] == fm.strip_items(w - 32, h - 32, rps), (w, h, rps)
            own = fm.owner_map(w, h, rps)                                # asserts: every window pixel has exactly one owner
            assert (own >= 0).sum() == (w - 32) * (h - 32)


def test_every_plan_class_occurs():
    """The table of shapes: (nfull, sub) of the 6-row and of the 24-row plan, and what makes each shape special."""
    want = {122: ((0, [2, 0]), (0, [2, 0])), 200: ((0, [2, 4]), (1, [0, 0])), 300: ((1, [4, 0]), (1, [4, 0])), 380: ((1, [2, 0]), (1, [2, 0])),
            430: ((1, [2, 4]), (2, [0, 0])), 480: ((2, [0, 0]), (2, [0, 0])), 84: ((0, [4, 0]), (0, [4, 0]))}
    for w, h in fc.SHAPES:
        got = tuple((p[0], p[3]) for p in (fm.strip_plan(w - 32, h - 32, rps) for rps in (6, 24)))
        assert got == want[w], (w, got)
        assert (h - 32) % 24 == 2 and (h - 32) % 6 == 2                  # a last segment of two rows in both forms
    assert {w for w, _ in fc.SHAPES if w % 4} == {122, 430}             # level 0 of these is copied, the others' can be read in place
    below = lambda w, rps: [(r.item, r.sub) for r in fm.plan(w, fc.H, rps) if r.y1 == r.y0]
    assert below(122, 24) == [(2, 1)]                                   # 5 segments two by two
    assert below(300, 24) == [(6, 1), (6, 2), (6, 3)]                   # the second narrow item: three of four sub-strips below the level
    narrow = [r for r in fm.plan(300, fc.H, 24) if r.nsub == 4]
    assert {r.x1 - r.x0 for r in narrow} == {20}                        # a 4-way strip 20 columns wide
    last = [r for r in fm.plan(430, fc.H, 24) if r.x0 == 16 + 248]
    assert {r.x1 - r.x0 for r in last} == {430 - 32 - 248} and 430 - 32 - 248 < 248 - 8   # the second full strip runs past the window: the Xc clamp
    assert {r.x1 - r.x0 for r in fm.plan(480, fc.H, 24) if r.x0 == 16 + 248} == {200}
    assert fm.grid(84, fc.H)[:3] == (1, 3, 58) and 48 < _max_roi(84, fc.H) <= 66 and all(_max_roi(w, h) <= 48 for w, h in fc.SHAPES[:6])
    assert len(fm.cells(122, fc.H)) == 9 and len(fm.cells(480, fc.H)) == 45


def test_every_case_fits_the_handle_the_gpu_tests_create():
    for k in fc.cases():
        rc, sizes = fc.handle_verdict(k)
        assert rc == 0 and sizes[0] == (k.w, k.h), (k.name, rc)
        assert k.frames.shape[1:] == (k.h, k.w) and k.frames.dtype == np.uint8 and len(k.order) >= 3 and set(k.order) == set(range(len(k.frames))), k.name
    assert [k.name for k in fc.cases()] == list(fc.NAMES)
    assert len(fc.by_name("e second cell 480 x 130").order) == 200


# ---- (a) -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", fc.SHAPES)
def test_dots_are_isolated_and_every_pixel_is_one_once(w, h):
    """Each dot is a corner of strength = its contrast and no other pixel has any strength; over the 49 frames every pixel whose ring lies
    in the image -- every window pixel, and the 13 columns and rows around the window, where nothing may be found -- is a dot once."""
    seen = np.zeros((h, w), np.int32)
    classes = set()
    for oy in range(7):
        for ox in range(7):
            img = fc.dots(w, h, ox, oy)
            xs, ys = fc.dot_sites(w, h, ox, oy)
            c, s = fc.dot_contrast(xs, ys)
            S = gm.strength(img)
            assert (S[ys, xs] == c).all() and (img[ys, xs].astype(int) == fc.GROUND + c * s).all()
            S[ys, xs] = 0
            assert not S.any()
            seen[ys, xs] += 1
            inside = (xs >= 16) & (xs < w - 16) & (ys >= 16) & (ys < h - 16)
            classes |= set(zip(c[inside].tolist(), s[inside].tolist()))
    assert (seen[3:h - 3, 3:w - 3] == 1).all() and seen.sum() == (w - 6) * (h - 6)
    got = {c for c, _ in classes}                                         # the window of the narrow shapes holds 2 x 2 or 3 x 2 blocks only
    assert (got == set(fc.DOT_CLASSES) if w >= 300 else got >= {5, 8, 21, 60}) and {s for _, s in classes} == {1, -1}
    assert fc.GROUND + 127 == 255 and fc.GROUND - 127 == 1


@pytest.mark.parametrize("w,h", fc.SHAPES)
def test_dots_leave_whole_cells_to_the_fallback_and_whole_cells_not(w, h):
    name = "a dots %d x %d" % (w, h)
    k = fc.by_name(name)
    for (cands, n_fb), f in zip(fc.expected(name), k.frames):
        lists = fm.cell_lists(f, k.fast_th)
        assert 0 < n_fb < len(lists) or w == 84, (name, n_fb)
        for c, fb, pts in lists:
            assert all((s < k.fast_th) == fb for _, _, s in pts)          # a cell's points are all of one class
    assert any(0 < n for _, n in fc.expected(name))


# ---- (b) -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("orient", fc.ORIENTATIONS)
def test_pair_strengths(orient):
    dx, dy = orient
    for w in (300, 430):
        for ox, oy in ((0, 0), (3, 5), (7, 7)):
            img = fc.pairs(w, fc.H, orient, ox, oy)
            S = gm.strength(img)
            xs, ys = fc.pair_sites(w, fc.H, orient, ox, oy)
            a, b = img[ys, xs].astype(int), img[ys + dy, xs + dx].astype(int)
            assert {(int(p), int(q)) for p, q in zip(a, b)} == set(fc.PAIR_KINDS)
            assert (S[ys, xs] == a - fc.GROUND).all() and (S[ys + dy, xs + dx] == b - fc.GROUND).all()       # 62 and 62, 72 and 62, 62 and 72
            S[ys, xs] = S[ys + dy, xs + dx] = 0
            assert not S.any()                                                                              # no corner off the blobs


def _seam_pairs(w, rps, orient):
    """(unequal pairs whose pixels two regions own while one cell holds both, equal pairs that a cell boundary separates), over all offsets"""
    dx, dy = orient
    own = fm.owner_map(w, fc.H, rps)
    n_cols, n_rows, w_cell, h_cell = fm.grid(w, fc.H)
    cell = lambda x, y: (np.minimum((y - 16) // h_cell, n_rows - 1), np.minimum((x - 16) // w_cell, n_cols - 1))
    across, split = 0, 0
    for oy in range(8):
        for ox in range(8):
            img = fc.pairs(w, fc.H, orient, ox, oy)
            xs, ys = fc.pair_sites(w, fc.H, orient, ox, oy)
            x2, y2 = xs + dx, ys + dy
            inside = (own[ys, xs] >= 0) & (own[y2, x2] >= 0)
            c1, c2 = cell(xs, ys), cell(x2, y2)
            same_cell = (c1[0] == c2[0]) & (c1[1] == c2[1])
            unequal = img[ys, xs] != img[y2, x2]
            across += int((inside & same_cell & unequal & (own[ys, xs] != own[y2, x2])).sum())
            split += int((inside & ~same_cell & ~unequal).sum())
    return across, split


@pytest.mark.parametrize("w", [300, 430])
@pytest.mark.parametrize("rps", [6, 24])
def test_pairs_lie_across_every_kind_of_seam(w, rps):
    """Per orientation there are unequal pairs across a segment seam inside one cell (the loser must see the winner through the halo) and
    equal pairs that a cell boundary separates (both survive).  At 300 px the strip seam (column 264) is a cell boundary as well, at 430 px
    it is not: there the pairs with a horizontal component also cross a strip seam inside a cell."""
    for o in fc.ORIENTATIONS:
        across, split = _seam_pairs(w, rps, o)
        # (a horizontal pair can only cross a vertical seam, and the only one of 300 x 130 is a cell boundary)
        assert (across == 0 if (w, o) == (300, (1, 0)) else across >= 8) and split >= 8, (w, rps, o, across, split)
    assert (264 - 16) % fm.grid(300, fc.H)[2] == 0 and (264 - 16) % fm.grid(430, fc.H)[2] != 0
    own = fm.owner_map(430, fc.H, rps)
    img = fc.pairs(430, fc.H, (1, 0), 263 % 8, 0)
    ys = np.nonzero(img[:, 263] != fc.GROUND)[0]
    ys = ys[(ys >= 16) & (ys < fc.H - 16)]
    assert len(ys) >= 8 and (own[ys, 263] != own[ys, 264]).all() and (img[ys, 264] != fc.GROUND).all() and (img[ys, 263] != img[ys, 264]).any()


def test_lone_equal_pairs_make_their_cells_fall_back():
    name = "b lone equal pairs 300 x 130"
    k = fc.by_name(name)
    for f, (cands, n_fb), (dx, dy) in zip(k.frames, fc.expected(name), fc.ORIENTATIONS):
        S = gm.strength(f)
        lists = fm.cell_lists(f, k.fast_th, S=S)
        assert n_fb == len(lists) == 27
        for c, fb, pts in lists:
            cx, cy = c.x0 + c.rw // 2, c.y0 + c.rh // 2
            assert S[cy, cx] == S[cy + dy, cx + dx] == 62 and S[cy + 2 * dy, cx + 2 * dx] == 12
            assert _interior_corners(S, c, k.fast_th) == 2 and fb and len(pts) >= 6
            gone = {(cx - 13, cy - 13), (cx + dx - 13, cy + dy - 13), (cx + 2 * dx - 13, cy + 2 * dy - 13)}
            assert not gone & {(x, y) for x, y, _ in pts} and {s for _, _, s in pts} == {7}


# ---- (c) -----------------------------------------------------------------------------------------------------------------------------------
def test_list_limit_frames_hold_exactly_the_counts():
    frames = fc.count_frames()
    assert [(r, t) for r, t, _ in frames] == [(r, t) for r in (24, 6) for t in fc.COUNT_TARGETS] and fc.COUNT_TARGETS == (FL_CAP - 1, FL_CAP, FL_CAP + 1, 2 * FL_CAP + 1)
    k = fc.by_name("c list limits 300 x 130")
    assert k.fast_th == 7 and len(k.frames) == len(frames) + 1          # both forced modes stream at 7: the count is the list's
    for (rps, target, img), f in zip(frames, k.frames):
        assert (img == f).all()
        S = gm.strength(img)
        regs = fm.plan(300, fc.H, rps)
        counts = [fm.region_corners(S, r, 7) for r in regs]
        at = fc.count_region(300, fc.H, rps)
        assert counts[at] == target and regs[at].x1 - regs[at].x0 == 248 and regs[at].y1 - regs[at].y0 == rps
        assert max(c for i, c in enumerate(counts) if i != at) < FL_CAP, (rps, target, counts)
    S = gm.strength(k.frames[-1])                                          # plain noise: a full 6-row region flushes once or twice, a 24-row one six times
    for rps, least in ((6, 600), (24, 6 * FL_CAP)):
        full = [fm.region_corners(S, r, 7) for r in fm.plan(300, fc.H, rps) if r.nsub == 1 and r.y1 - r.y0 == rps]
        assert min(full) > least, (rps, min(full))


# ---- (d), (e) --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["d busy cells 300 x 130", "d busy cells 84 x 130", "e second cell 480 x 130"])
def test_every_cell_is_empty_at_the_busy_threshold(name):
    k = fc.by_name(name)
    assert k.fast_th == fc.busy_threshold() >= 200
    for f, (cands, n_fb) in zip(k.frames, fc.expected(name)):
        S = gm.strength(f)
        lists = fm.cell_lists(f, k.fast_th, S=S)
        assert n_fb == len(lists) and all(fb for _, fb, _ in lists)
        assert all(_interior_corners(S, c, k.fast_th) == 0 for c, _, _ in lists) and all(s < k.fast_th for _, _, s in cands)


def test_fallback_cells_above_and_below_ccap():
    for name, maxroi in (("d busy cells 300 x 130", 48), ("d busy cells 84 x 130", 66)):
        k = fc.by_name(name)
        assert (48 if _max_roi(k.w, k.h) <= 48 else 66) == maxroi
        n = [_interior_corners(gm.strength(f), c) for f in k.frames for c in fm.cells(k.w, k.h)]
        cap = CCAP[maxroi]
        assert sum(x > cap for x in n) >= 3 and sum(0 < x <= cap for x in n) >= 3, (name, sorted(n))
    # the mixed frame of 300 x 130 holds sparse cells (the dots), dense ones (the noise) and the cells in between in one frame
    k = fc.by_name("d busy cells 300 x 130")
    n = [_interior_corners(gm.strength(k.frames[2]), c) for c in fm.cells(k.w, k.h)]
    assert min(n) < 30 and max(n) > CCAP[48]


def test_the_rotation_gives_a_wavefront_a_dense_and_a_sparse_cell():
    """200 x 45 = 9000 listed cells for 7168 wavefronts: 1832 wavefronts redo a second cell (items v and v + 7168 of the list).
    k_fast_cells_list fills the list by per-workgroup reservations, in arrival order, so which cells meet in a wavefront is not controlled;
    what the case controls is that a quarter of the listed cells each are dense, sparse, flat and mixed, so that most pairs differ."""
    k = fc.by_name("e second cell 480 x 130")
    n_cells = len(fm.cells(k.w, k.h))
    waves = 256 * 7 * 4
    assert _max_roi(k.w, k.h) <= 48 and n_cells == 45 and len(k.order) * n_cells == 9000 > waves
    dense = [max(_interior_corners(gm.strength(f), c) for c in fm.cells(k.w, k.h)) for f in k.frames]
    assert dense[0] > CCAP[48] and 0 < dense[1] < 30 and dense[2] == 0 and dense[3] > CCAP[48]
    assert [len(c) for c, _ in fc.expected(k.name)][2] == 0
    assert [k.order.count(i) for i in range(4)] == [50] * 4 and len(k.order) * n_cells - waves == 1832


# ---- (f) -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", fc.ATLAS_THRESHOLDS)
def test_atlas_coverage(t):
    """Every pattern's centre has the strength it was built for: t + 1 with an arc of 9 (a corner at fastTh = t, by one), t with an arc of 8
    (none, by one).  A combination is skipped when v +- (t + 1) leaves the byte range: a third of them up to t = 21.  At t = 128 only
    v <= 126 can have a brighter and v >= 129 a darker arc, 5 of the 12 centre values each: 7 / 12 are skipped there, which no choice
    among these centre values can bring below one half."""
    img, placed, skipped, total = fc.atlas(t)
    S = gm.strength(img)
    for cx, cy, v, pol, length, start in placed:
        assert img[cy, cx] == v and S[cy, cx] == (t + 1 if length == 9 else t), (t, cx, cy)
    assert len(placed) + skipped == total == 16 * 2 * 2 * len(fc.ATLAS_CENTRES)
    if t <= 21:
        assert skipped * 2 < total and skipped * 3 == total
    else:
        assert skipped * 12 == total * 7
    for pol in (1, -1):
        for length in (8, 9):
            assert {p[5] for p in placed if p[3] == pol and p[4] == length} == set(range(16))
            assert len({p[2] & 1 for p in placed if p[3] == pol and p[4] == length}) == 2          # both parities of v
    cands = {(x, y): s for x, y, s in fc.expected("f atlas t=%d" % t)[0][0]}
    nine = [cands.get((cx - 13, cy - 13)) for cx, cy, v, pol, length, start in placed if length == 9]
    assert sum(s == t for s in nine) > len(nine) // 2                        # most survive as candidates of score t (the rest lose to a neighbour)


# ---- the cases tell the model from its mutants -----------------------------------------------------------------------------------------------
KILLED_BY = {
    "seam_blind_nms": "b pairs 430 x 130 (1, 0)",
    "global_nms": "b pairs 300 x 130 (0, 1)",
    "nms_ge": "b pairs 300 x 130 (1, 1)",
    "corner_ge": "f atlas t=20",
    "fallback_on_high_only": "b lone equal pairs 300 x 130",
    "fallback_drops_high": "b lone equal pairs 300 x 130",
    "window_15": "a dots 122 x 130",
}


@pytest.mark.parametrize("mutant", fm.MUTANTS)
def test_a_committed_case_kills_the_mutant(mutant):
    assert set(KILLED_BY) == set(fm.MUTANTS)
    k = fc.by_name(KILLED_BY[mutant])
    differs = lambda i, rps: fm.level_candidates(k.frames[i], k.fast_th, mutant, rps) != fc.expected(k.name)[i][0]
    if mutant in ("fallback_on_high_only", "fallback_drops_high"):
        assert all(differs(i, 24) for i in range(len(k.frames))), (mutant, k.name)       # every orientation of the lone pairs
    else:
        for rps in ((6, 24) if mutant == "seam_blind_nms" else (24,)):
            assert any(differs(i, rps) for i in range(len(k.frames))), (mutant, k.name, rps)


def test_each_orientation_of_pairs_kills_the_seam_blind_mutant():
    """but the horizontal pairs of 300 x 130, which have no seam to cross inside a cell"""
    for w in (300, 430):
        for o in fc.ORIENTATIONS:
            k = fc.by_name("b pairs %d x %d (%d, %d)" % ((w, fc.H) + o))
            for rps in (6, 24):
                assert (w, o) == (300, (1, 0)) or any(fm.level_candidates(k.frames[i], k.fast_th, "seam_blind_nms", rps) != fc.expected(k.name)[i][0] for i in range(0, 64, 9)), (k.name, rps)
