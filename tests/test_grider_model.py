"""The numpy model of Grider_FAST (tests/grider_model.py) held to hand-computed pixels and to the C++ oracle, and the committed cases
(tests/grider_cases.py) held to the edges they are named for.  No GPU: this ties together the two references of the grid-bucketed FAST
and shows that tests/test_gpu_grider.py looks where csrc/grider.hip can go wrong."""
import numpy as np
import pytest

import grider_cases as gc
import grider_model as gm

ALL = [k.name for k in gc.cases()]


def _call(fn, k, **kw):
    return fn(k.image, k.num_features, k.grid_x, k.grid_y, k.threshold, k.nms, **kw)


def _roi_lists(k, nms=None):
    """Per ROI: (x0, y0, rows (x, y, response) in ROI coordinates)."""
    h, w = k.image.shape
    size_x, size_y, ct_cols, ct_rows = gm.geometry(w, h, k.grid_x, k.grid_y)
    S = gm.strength(k.image)
    return [(r % ct_cols * size_x, r // ct_cols * size_y,
             gm.roi_points(S, r % ct_cols * size_x, r // ct_cols * size_y, size_x, size_y, k.threshold, k.nms if nms is None else nms))
            for r in range(ct_cols * ct_rows)]


# ---- the model by hand -----------------------------------------------------------------------------------------------------------------
def test_ring_and_record_layout():
    import oracle_lib
    assert set(gm.ring()) == {(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0),
                              (-3, 1), (-2, 2), (-1, 3)}
    r = gm.ring()
    assert all(max(abs(r[i][0] - r[i - 1][0]), abs(r[i][1] - r[i - 1][1])) == 1 for i in range(16))   # neighbours on the circle
    assert gm.KEYPOINT_DTYPE == oracle_lib.KP and gm.KEYPOINT_DTYPE.itemsize == 28


def test_strength_by_hand():
    """The right half of the circle, top to bottom, is 9 contiguous pixels: (x, y) in a 7 x 7 image centred on (3, 3)."""
    half = [(3, 0), (4, 0), (5, 1), (6, 2), (6, 3), (6, 4), (5, 5), (4, 6), (3, 6)]
    img = np.full((7, 7), 50, np.uint8)
    for x, y in half:
        img[y, x] = 80
    assert gm.strength(img)[3, 3] == 30                              # nine brighter by 30
    assert gm.fast(img, 29)["response"].tolist() == [29.0] and len(gm.fast(img, 30)) == 0
    img[6, 3] = 50
    assert gm.strength(img)[3, 3] == 0                               # eight are not enough
    img[6, 3] = 70
    assert gm.strength(img)[3, 3] == 20                              # the arc's weakest pixel
    for x, y in half:
        img[y, x] = 10
    assert gm.strength(img)[3, 3] == 40                              # nine darker by 40
    img[3, 3] = 255
    img[half[0][1], half[0][0]] = 0
    assert gm.strength(img)[3, 3] == 245                             # the whole ring is darker: the half at 10 and 0 is the best arc
    assert gm.strength(gc.dots(16, 16))[8, 8] == 255 and gm.strength(gc.dots(16, 16))[8, 9] == 0


def test_nms_and_selection_by_hand():
    """Two dots side by side would need three pixels between them to be corners both; instead: a plane of strengths fed to the selection."""
    S = np.zeros((20, 20), np.int32)
    S[5, 5], S[5, 6], S[9, 9], S[9, 11], S[3, 3], S[2, 9] = 40, 41, 30, 30, 25, 99
    pts = gm.roi_points(S, 0, 0, 20, 20, 20, True).tolist()
    assert pts == [[3, 3, 24], [6, 5, 40], [9, 9, 29], [11, 9, 29]]       # (5, 5) is below its neighbour; row 2 is outside the interior
    assert gm.roi_points(S, 0, 0, 20, 20, 20, False).tolist() == [[3, 3, 24], [5, 5, 39], [6, 5, 40], [9, 9, 29], [11, 9, 29]]
    S[9, 10] = 30
    assert gm.roi_points(S, 0, 0, 20, 20, 20, True).tolist() == [[3, 3, 24], [6, 5, 40]]      # equal neighbours: neither is strictly above
    assert gm.roi_points(S, 0, 0, 20, 20, 24, True).tolist()[0] == [3, 3, 24] and gm.roi_points(S, 0, 0, 20, 20, 25, True).tolist()[0] != [3, 3, 24]
    assert gm.roi_points(S, 2, 2, 6, 6, 20, True).shape == (0, 3)           # a 6 x 6 ROI has no interior
    assert gm.roi_points(S, 0, 0, 7, 7, 20, True).tolist() == [[3, 3, 24]]  # a 7 x 7 ROI has one pixel of it
    assert gm.keep_per_roi(20, 2, 2) == 6 and gm.keep_per_roi(0, 3, 2) == 1 and gm.keep_per_roi(250, 10, 10) == 3
    assert gm.geometry(89, 88, 10, 10) == (8, 8, 11, 11) and gm.geometry(100, 90, 3, 4) == (33, 22, 3, 4)


# ---- the model against the oracle --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(gc.fills()) + ALL)
def test_oracle_equals_model(oracle, name):
    k = gc.fills()[name] if name in gc.fills() else gc.by_name(name)
    want = gc.expected(name)
    got = _call(oracle.grider_fast, k)
    assert len(got) == len(want) and got.tobytes() == want.tobytes(), name


def test_oracle_fast_equals_model_fast(oracle):
    """cv::FAST on one ROI -- the whole image -- with and without NMS, at every threshold a case uses on that image."""
    seen = set()
    for k in list(gc.fills().values()) + gc.cases():
        for nms in (True, False):
            key = (k.image.tobytes(), k.image.shape, k.threshold, nms)
            if key in seen or k.image.shape[0] < 7:
                continue
            seen.add(key)
            want = gm.fast(k.image, k.threshold, nms)
            assert oracle.fast(k.image, k.threshold, nms).tobytes() == want.tobytes(), (k.name, nms)
            assert oracle.fast(k.image, k.threshold, nms, bruteforce=True).tobytes() == want.tobytes(), (k.name, nms)
    assert len(seen) >= 30


# ---- every case holds its edge -----------------------------------------------------------------------------------------------------------
def test_every_image_fits_the_handle_by_area():
    for k in list(gc.fills().values()) + gc.cases():
        h, w = k.image.shape
        assert w * h <= gc.HANDLE_W * gc.HANDLE_H and w >= 7 and h >= 7, k.name


def test_the_gpu_tests_handle_accepts_every_case():
    """uvo_grider_fast refuses (UVO_E_BADARG) an image with more pixels than the corner scratch has entries or more ROIs than it has counts,
    and (UVO_E_CAPACITY) ROIs x quota above the output staging: none of that happens to a case on the test's handle, the staging ends
    where the capacity test says, and the same handle with max_batch = 1 would refuse the cases with 256 and 441 ROIs."""
    pixels, rois, staging = gc.handle_capacities()
    most = 0
    for k in list(gc.fills().values()) + gc.cases():
        h, w = k.image.shape
        _, _, ct_cols, ct_rows = gm.geometry(w, h, k.grid_x, k.grid_y)
        assert w * h <= pixels and ct_cols * ct_rows <= rois, k.name
        assert ct_cols * ct_rows * gm.keep_per_roi(k.num_features, k.grid_x, k.grid_y) <= staging, k.name
        most = max(most, ct_cols * ct_rows)
    assert most == 441 and staging == gc.HANDLE_CFG[3] * (gc.HANDLE_CFG[0] + 4)
    assert gc.handle_capacities(max_batch=1)[1] == 127


def test_partial_blocks_and_leftovers():
    k = gc.by_name("partial blocks")
    h, w = k.image.shape
    assert w % 64 and h % 4 and w > 64 and gm.geometry(w, h, k.grid_x, k.grid_y) == (33, 30, 2, 2)      # column 66 and row 60 belong to no ROI
    assert len(gc.expected(k.name)) == 44
    k = gc.by_name("corners in a partial block")
    assert k.image.shape == (62, 75) and (gc.expected(k.name)["x"] >= 64).sum() >= 3


def test_leftover_strips_are_not_part_of_the_last_rois():
    """Column 99 and rows 88 .. 89 belong to no ROI.  The strips are thinner than FAST's 3-pixel border, so no corner of the whole-image FAST
    can lie IN them; what they change is where the last ROIs end: a kernel that stretched the last ROI to the image's edge would move its
    interior out to column 96 and rows 85 .. 86, where the whole-image FAST has corners; the ROIs as they are reach 95 and 84."""
    k = gc.by_name("leftover strips")
    h, w = k.image.shape
    assert gm.geometry(w, h, k.grid_x, k.grid_y) == (33, 22, 3, 4) and (w - 3 * 33, h - 4 * 22) == (1, 2)
    whole = gm.fast(k.image, k.threshold, k.nms)
    got = gc.expected(k.name)
    assert (whole["x"] == 96).any() and (whole["y"] >= 85).any()
    assert got["x"].max() <= 95 and got["y"].max() <= 84
    uncut = [(x0 + p[:, 0].max(), y0 + p[:, 1].max()) for x0, y0, p in _roi_lists(k)]
    assert max(x for x, _ in uncut) == 95 and max(y for _, y in uncut) == 84             # the last interior column and row are in use


def test_more_rois_than_grid_cells():
    k = gc.by_name("more ROIs than grid cells")
    h, w = k.image.shape
    size_x, size_y, ct_cols, ct_rows = gm.geometry(w, h, k.grid_x, k.grid_y)
    assert w % k.grid_x >= w // k.grid_x and h % k.grid_y >= h // k.grid_y
    assert (size_x, size_y) == (8, 8) and ct_cols == 11 > k.grid_x and ct_rows == 11 > k.grid_y
    got = gc.expected(k.name)
    assert (got["x"] >= 80).any() and (got["y"] >= 80).any()                        # points from the ROIs beyond the grid
    assert any(len(p) > gm.keep_per_roi(k.num_features, k.grid_x, k.grid_y) for _, _, p in _roi_lists(k))   # and the quota cuts


def test_more_points_than_the_old_binding_buffer():
    k = gc.by_name("more points than num_features + cells + 64")
    got = gc.expected(k.name)
    assert len(got) == 11 * 71 > k.num_features + k.grid_x * k.grid_y + 64


def test_smallest_interior():
    k = gc.by_name("smallest interior")
    h, w = k.image.shape
    assert gm.geometry(w, h, k.grid_x, k.grid_y) == (7, 7, 10, 9)
    got = gc.expected(k.name)
    assert 0 < len(got) < 90 and ((got["x"] % 7 == 3) & (got["y"] % 7 == 3)).all()


def test_per_roi_nms_differs_from_global_nms():
    """A kept corner has a stronger corner of the whole-image FAST next to it, just outside its ROI's interior."""
    k = gc.by_name("smallest interior")
    h, w = k.image.shape
    S = gm.strength(k.image)
    G = np.zeros((h, w), np.int32)
    G[3:h - 3, 3:w - 3] = np.where(S[3:h - 3, 3:w - 3] > k.threshold, S[3:h - 3, 3:w - 3] - 1, 0)
    found = 0
    for p in gc.expected(k.name):
        x, y = int(p["x"]), int(p["y"])
        around = G[y - 1:y + 2, x - 1:x + 2]
        found += bool(around.max() > p["response"])          # every neighbour of a 7 x 7 ROI's one interior pixel is outside that interior
    assert found >= 1


@pytest.mark.parametrize("w,h,gx,gy", gc.NO_INTERIOR)
def test_no_interior_cases_and_what_the_unguarded_loop_read(w, h, gx, gy):
    """The full-size fill leaves strength 255 at every (4 i, 4 j) of its interior.  With ROIs of 6 x 6 and 4 x 40 the product of the interior's
    sides is <= 0 and the unguarded loop never ran.  With 4 x 4 and 3 x 3 it read behind the image's w * h bytes, where the fill's row 12
    holds dots.  With 2 x 2 and 1 x 1 what it read behind the plane are the fill's rows 3 and 0 -- no dots there -- (and, for 1 x 1, bytes in
    FRONT of the plane), so those two also run behind a 64-wide fill, whose rows 16 and 4 lie there."""
    sx, sy = w // gx, h // gy
    name = "no interior %d x %d" % (sx, sy)
    k = gc.by_name(name)
    assert k.fill == "full" and k.image.shape == (h, w) and len(gc.expected(name)) == 0
    reads, _ = gc.unguarded_reads(w, h, gx, gy)
    if sx > 5 or sy > 5:
        assert (sx - 6) * (sy - 6) <= 0 and len(reads) == 0
        return
    assert (sx - 6) < 0 and (sy - 6) < 0 and len(reads) == (sx - 6) * (sy - 6) * (w // sx) * (h // sy)
    stale = gc.plane_after(gc.fills()["full"])
    behind = reads[reads >= w * h]                              # not overwritten by the case's own k_grid_score
    assert len(behind) > 0 and behind.max() < len(stale)
    assert (reads.min() < 0) == ((sx, sy) == (1, 1))
    hit = stale[behind]
    if sx >= 3:
        assert (hit == 255).any()
        if (sx, sy) == (4, 4):
            assert behind.tolist() == [w * h]                   # one element past the plane
        else:
            rows, cols = np.unique(behind // gc.HANDLE_W), behind % gc.HANDLE_W
            assert rows.tolist() == [12] and (cols.min(), cols.max()) == (129, 194)    # (129 .. 131: row 62's columns 63 .. 65)
    else:
        assert not hit.any()
        small = gc.by_name(name + " behind the small fill")
        assert small.fill == "small" and small.image.shape == (h, w) and len(gc.expected(small.name)) == 0
        assert (gc.plane_after(gc.fills()["small"])[behind] == 255).any()


def test_a_stale_score_would_have_become_a_keypoint_below_the_image():
    """The 3 x 3 case without the guard, worked through: the stale 255 at plane row 63 of the 63-wide image is a key point with y = 63."""
    w, h, gx, gy = gc.NO_INTERIOR[3]
    reads, ys = gc.unguarded_reads(w, h, gx, gy)
    stale = gc.plane_after(gc.fills()["full"])
    assert {int(y) for i, y in zip(reads, ys) if i >= w * h and stale[i]} == {h}


def test_clamps():
    img = gc.by_name("clamps t=0").image
    assert img.min() == 100 and img.max() == 103
    below, zero, zero_all, one = (gc.expected("clamps t=" + s) for s in ("-5", "0", "0 nms off", "1"))
    assert below.tobytes() == zero.tobytes() and len(zero) > 0                      # -5 is clamped to 0
    assert (zero_all["response"] == 0).any() and (zero["response"] > 0).all()       # score-0 corners exist and never survive NMS
    assert len(gm.fast(img, 0, False)) > len(gm.fast(img, 1, False)) > 0            # the threshold 1 drops them as corners
    assert (one["response"] >= 1).all()
    assert len(zero_all) == gc.by_name("clamps t=0 nms off").num_features + 1       # the quota cuts inside the responses 0 and 1
    assert gm.grider_fast(img, 300, 1, 1, -5, True, mutant="threshold_unclamped")["response"].min() < 0


def test_saturated_scores():
    k = gc.by_name("saturated t=254")
    assert gc.plane_after(k).max() == 255                                             # the plane's byte is full
    got = gc.expected(k.name)
    assert len(got) == 104 and (got["response"] == 254).all()
    assert len(gc.expected("saturated t=255")) == 0 and len(gc.expected("saturated t=300")) == 0
    assert len(gm.grider_fast(k.image, 100, 2, 2, 300, True, mutant="threshold_unclamped")) == 0


@pytest.mark.parametrize("name", ["ties at the cut", "ties at the cut nms off"])
def test_the_cut_runs_through_equal_responses(name):
    k = gc.by_name(name)
    keep = gm.keep_per_roi(k.num_features, k.grid_x, k.grid_y)
    assert keep == 6
    for x0, y0, pts in _roi_lists(k):
        assert len(pts) == 11 * 9 > keep and set(pts[:, 2].tolist()) == {254}
    got, other = gc.expected(name), _call(gm.grider_fast, k, mutant="ties_x_then_y")
    assert len(got) == len(other) == 24
    assert got[:6]["y"].tolist() == [4] * 6 and got[:6]["x"].tolist() == [4, 8, 12, 16, 20, 24]
    assert other[:6]["x"].tolist() == [4] * 6 and other[:6]["y"].tolist() == [4, 8, 12, 16, 20, 24]


def test_num_features_zero_and_wider():
    k = gc.by_name("num_features = 0")
    assert gm.keep_per_roi(0, k.grid_x, k.grid_y) == 1 and len(gc.expected(k.name)) == 6
    for (x0, y0, pts), p in zip(_roi_lists(k), gc.expected(k.name)):
        assert p["response"] == pts[:, 2].max()
    k = gc.by_name("wider than max_width")
    h, w = k.image.shape
    assert w > gc.HANDLE_W and w * h <= gc.HANDLE_W * gc.HANDLE_H and (gc.expected(k.name)["x"] >= gc.HANDLE_W).any()


# ---- the cases tell the model from its mutants -------------------------------------------------------------------------------------------
KILLED_BY = {
    "global_nms": "smallest interior",
    "nms_ge": "clamps t=0",
    "corner_ge": "saturated t=255",
    "ties_x_then_y": "ties at the cut",
    "keep_without_plus_one": "num_features = 0",
    "rois_from_grid": "more ROIs than grid cells",
    "inset_2": "no interior 6 x 6",
    "threshold_unclamped": "clamps t=-5",
    "response_is_strength": "saturated t=254",
}


@pytest.mark.parametrize("mutant", gm.MUTANTS)
def test_a_committed_case_kills_the_mutant(mutant):
    assert set(KILLED_BY) == set(gm.MUTANTS)
    k = gc.by_name(KILLED_BY[mutant])
    assert _call(gm.grider_fast, k, mutant=mutant).tobytes() != gc.expected(k.name).tobytes(), (mutant, k.name)
