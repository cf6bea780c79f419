"""k_fast_score, k_fast_cells_list and k_fast_cells (csrc/fast.hip) held to the numpy model of tests/fast_model.py at the cases of
tests/fast_cases.py -- tests/test_fast_model.py ties the model to the oracle and to csrc/strip_plan.hpp on the CPU and shows what each
case reaches.  Every frame of every case is compared, candidate by candidate, in both forced FAST modes and both region heights:
as one batch (batch >= 3: 24-row regions, k_fast_cells_list + the listed k_fast_cells) and frame by frame (6-row regions, the direct
k_fast_cells).  A failure names the first differing candidate, the region and the cell that own it.

What a failing family points at:
  a  dots       one queued pixel alone: the queue's rule that an incomplete batch is scored only after two checkpoints, every row residue
                of the 14-row LDS ring and both parities of the 7-row block, every halo row and column, the last rows of a segment, lanes
                on both sides of every strip, sub-strip and segment seam, the window's edge (dots at columns / rows 13 .. 15 are not
                corners), a whole cell of weak dots that falls back next to one that does not.  By shape: 122 a lone 2-way strip with a
                sub-strip below the level, level 0 copied; 200 the 2-way + 4-way strips, and the "few segments" single strip; 300 a 4-way
                strip 20 columns wide, three of four sub-strips below the level; 380 full + 2-way; 430 full + 2-way + 4-way, and a second
                full strip that runs past the window (the Xc clamp); 480 two full strips; 84 the k_fast_cells<66> geometry
  b  pairs      the halo ring: the loser of an unequal pair across a strip or segment seam must see the winner's score; equal pairs
                annihilate inside a cell and both survive across a cell boundary (the in-cell masks mL / mR / mU / mD); lone equal pairs:
                the fall-back is decided by survivors, not by pixels >= fastTh, and in the second call those pixels still suppress
  c  limits     the FL_CAP = 320 corner list: 319 / 320 / 321 / 641 listed corners in one region (no flush, none, one, two), plain
                noise (every region flushes; the NMS tail runs on the list in memory)
  d  busy       k_fast_cells on cells with more corners than CCAP (256 / 512): positions no longer remembered, the whole score tile
                scanned and cleared; and cells below CCAP beside them
  e  rotation   9000 listed cells for the 7168 wavefronts of the fixed k_fast_cells grid: 1832 wavefronts redo a second cell.  The list is
                filled in arrival order, so which two cells meet is not controlled; with four kinds of frame in rotation most pairs are of
                different kinds.  A score tile that was not wiped changes a sparse cell that follows a dense one: a weak dot goes missing
                next to a stale score, or a stale score survives as a candidate (a flat cell finds no corner and never looks at its tile)
  f  atlas      the 7-bit screen (Screen4) and the exact arc test at every arc start, both polarities, arcs of 8 and 9, every parity of
                the centre and the threshold, centres at both ends of the byte range
  g  levels     item -> level mapping, per-level cand_off and cursors"""
import numpy as np
import pytest

import fast_cases as fc
import fast_model as fm

pytestmark = pytest.mark.gpu

CAP = 1 << 14          # candidates read back per (frame, level): the busiest frame has 4832


def _mode(uvo, mode):
    return {"two_pass": uvo.UVO_FAST_MODE_TWO_PASS, "single_pass": uvo.UVO_FAST_MODE_SINGLE_PASS, "adaptive": uvo.UVO_FAST_MODE_ADAPTIVE}[mode]


def _handle(uvo, k, mode, inplace=None):
    ex = uvo.ORBextractor(fc.NFEATURES, 1.2, k.nlevels, 0, k.fast_th, max_width=k.w, max_height=k.h, max_batch=len(k.order))
    ex.tune(uvo.UVO_TUNE_FAST_MODE, _mode(uvo, mode))
    if inplace is not None:
        ex.tune(uvo.UVO_TUNE_LEVEL0_INPLACE, inplace)
    return ex


def _compare(ex, k, level, frame, want, batch, what):
    got = sorted(map(tuple, ex.read_candidates(level, frame=frame, cap=CAP).tolist()))
    if got != want:
        lw, lh = ex.level_dims(level)
        d, kind = fc.first_difference(got, want)
        where = fc.owner(lw, lh, d[0], d[1], 6 if batch <= 2 else 24) if d else ""
        pytest.fail("%s, %s, level %d: %d candidates, the model has %d; first difference %s %s; %s" % (k.name, what, level, len(got), len(want), d, kind, where))


def _run_single_level(ex, k, want, pairs_of_two):
    """one batch in the case's order, every distinct frame singly, and (a, b) one batch of exactly two frames"""
    ex.extract_batch(k.frames[list(k.order)])
    for f, i in enumerate(k.order):
        _compare(ex, k, 0, f, want[i][0], len(k.order), "frame %d of the batch of %d (image %d)" % (f, len(k.order), i))
    for i, img in enumerate(k.frames):
        ex(img)
        _compare(ex, k, 0, 0, want[i][0], 1, "image %d alone" % i)
    if pairs_of_two:
        two = [len(k.frames) - 1, len(k.frames) // 2]
        ex.extract_batch(k.frames[two])
        for f, i in enumerate(two):
            _compare(ex, k, 0, f, want[i][0], 2, "frame %d of a batch of two (image %d)" % (f, i))


@pytest.mark.parametrize("mode", ["two_pass", "single_pass"])
@pytest.mark.parametrize("name", fc.SINGLE_LEVEL)
def test_case_equals_the_model(uvo, name, mode):
    k, want = fc.by_name(name), fc.expected(name)
    ex = _handle(uvo, k, mode)
    try:
        _run_single_level(ex, k, want, k.family in "ab")
        t = ex.fast_state()[0]
        assert t[0] == (k.fast_th if mode == "two_pass" else min(k.fast_th, 7)), (name, mode, t)       # the form that was asked for ran
    finally:
        ex.close()


@pytest.mark.parametrize("mode", ["two_pass", "single_pass"])
@pytest.mark.parametrize("name", ["a dots 300 x 130", "a dots 480 x 130"])
def test_dots_with_level0_copied_instead_of_read_in_place(uvo, name, mode):
    k, want = fc.by_name(name), fc.expected(name)
    assert k.w % 4 == 0                          # by default these frames are read in place (test_case_equals_the_model)
    ex = _handle(uvo, k, mode, inplace=0)
    try:
        _run_single_level(ex, k, want, True)
    finally:
        ex.close()


@pytest.mark.parametrize("name", [n for n in fc.SINGLE_LEVEL if n.startswith("a ")])
def test_dots_adaptive_twice_on_one_handle(uvo, name):
    """The adaptive form decides a level's pass from the previous batch's share of fall-back cells (> 22 %: one pass at 7, < 14 %: two):
    the second batch runs in whatever form the first one chose.  fast_state() counts the cells whose first call finds nothing."""
    k, want = fc.by_name(name), fc.expected(name)
    n_cells = sum(1 for c in fm.cells(k.w, k.h) if c.rw > 6 and c.rh > 6)
    n_fb = sum(want[i][1] for i in k.order)
    ex = _handle(uvo, k, "adaptive")
    try:
        for rep in range(2):
            ex.extract_batch(k.frames[list(k.order)])
            for f, i in enumerate(k.order):
                _compare(ex, k, 0, f, want[i][0], len(k.order), "adaptive round %d, frame %d of the batch" % (rep, f))
            t, fb, cells = ex.fast_state()
            assert (int(fb[0]), int(cells[0])) == (n_fb, n_cells), (name, rep, fb, cells, n_fb, n_cells)
            if n_fb * 100 > n_cells * len(k.order) * 22:
                assert t[0] == 7, (name, rep, t)
            elif n_fb * 100 < n_cells * len(k.order) * 14:
                assert t[0] == k.fast_th, (name, rep, t)
            else:
                assert t[0] in (7, k.fast_th), (name, rep, t)
        img = k.frames[len(k.frames) // 3]          # and one frame alone behind them
        ex(img)
        _compare(ex, k, 0, 0, want[len(k.frames) // 3][0], 1, "adaptive, one image alone")
        assert int(ex.fast_state()[1][0]) == want[len(k.frames) // 3][1]
    finally:
        ex.close()


@pytest.mark.parametrize("mode", ["two_pass", "single_pass"])
def test_dots_through_three_levels(uvo, mode):
    """The model takes each level's plane from the handle (the pyramid is held to the oracle elsewhere)."""
    k = fc.by_name("g dots 380 x 130, 3 levels")
    ex = _handle(uvo, k, mode)
    wants = {}

    def compare_all(batch, frames, what):
        for f in frames:
            for l in range(k.nlevels):
                plane = np.ascontiguousarray(ex.read_plane(l, frame=f)[16:-16, 16:-16])
                key = (l, plane.tobytes())
                if key not in wants:
                    wants[key] = fm.level_candidates(plane, k.fast_th)
                assert len(wants[key]) > (300 if l == 0 else 20)          # a level-0 frame holds about 480 dots, the blurred-down levels fewer
                _compare(ex, k, l, f, wants[key], batch, "%s %d" % (what, f))

    try:
        ex.extract_batch(k.frames)
        assert [ex.level_dims(l) for l in range(3)] == [(380, 130), (317, 108), (264, 90)]
        compare_all(len(k.frames), range(len(k.frames)), "frame of the batch")
        for i in range(len(k.frames)):
            ex(k.frames[i])
            compare_all(1, [0], "image %d alone, frame" % i)
        ex.extract_batch(k.frames[[5, 40]])
        compare_all(2, [0, 1], "frame of a batch of two")
    finally:
        ex.close()
