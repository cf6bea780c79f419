"""The inputs of tests/test_gpu_topup.py, shared with tests/test_topup_model.py, which shows on the oracle alone that they reach the
places of k_assemble<TOPUP> they aim at.  A scene is an extractor configuration and an image; its cases are built from the scene's per-level
survivor lists (the oracle's on the CPU, a FullDetect call's on the GPU), because some grids are made to fit them."""
import functools

import numpy as np

import topup_model as tm

W, H = 320, 240
NEEDS = (0, 1, 2, 3, 4, 29, 30, 31, 36, 37, 38, 1000, 100000, -1, -30)      # at and below zero: see uvo.h
# the carry cases: level 0 stays below its cap (it takes 99 and 76 points on these grids; the caps are 109, 95, 81 ... and 77, 67, 57 ...),
# so KP_counter is carried on and enters level 2 beyond that level's cap
CARRY_NEED = {"noise": 409, "synth": 289}
# scene -> (nfeatures, scaleFactor, nlevels, fastTh), image
CFGS = {"noise": (500, 1.2, 8, 20), "synth": (500, 1.2, 8, 20), "noise10": (500, 1.1, 10, 20), "synth10": (500, 1.1, 10, 20), "rich": (3000, 1.2, 8, 20)}


@functools.lru_cache(maxsize=None)
def images(synth):
    noise = np.random.default_rng(7).integers(0, 256, (H, W), dtype=np.uint8)
    frame = synth.make_frame(900, W, H, n_shapes=120)
    return {"noise": noise, "synth": frame, "noise10": noise, "synth10": frame, "rich": synth.make_frame(901, W, H, n_shapes=400),
            "const": np.full((H, W), 90, np.uint8)}


def empty_grid(d):
    return np.zeros((H // d + 2, W // d + 2), np.int32, order="F")


def cells(levels, scales, d):
    """Per level the (row, column) of every survivor."""
    return [[tm.cell_of(x, y, scales[l], d) for x, y in pts] for l, pts in enumerate(levels)]


def carry_grid(levels, scales, d, k):
    """Every cell that a survivor of level 1 falls into is taken, except the first k of those that level 0 leaves alone."""
    g = empty_grid(d)
    lv = cells(levels, scales, d)
    seen = []
    for rc in lv[1]:
        if rc not in seen:
            seen.append(rc)
    free = [rc for rc in seen if rc not in lv[0]][:k]
    for r, c in seen:
        if (r, c) not in free:
            g[r, c] = 1
    return g


def contents_grid(levels, scales, d):
    """The four cells most survivors fall into hold -5, -1, 2 and 7: the first two are free -- and stay free until they count up to 1 --,
    the others are taken.  Returns (grid, the four cells)."""
    count = {}
    for lv in cells(levels, scales, d):
        for rc in lv:
            count[rc] = count.get(rc, 0) + 1
    top = sorted(count, key=lambda rc: (-count[rc], rc))[:4]
    g = empty_grid(d)
    for rc, v in zip(top, (-5, -1, 2, 7)):
        g[rc] = v
    return g, top


def scene_cases(scene, levels, scales):
    """[(label, grid, min_px_dist, need)] of a scene."""
    out = []
    if scene in ("noise", "synth"):
        out += [("sweep need=%d" % n, empty_grid(5), 5, n) for n in NEEDS]
        out += [("carry k=%d" % k, carry_grid(levels, scales, 5, k), 5, CARRY_NEED[scene]) for k in range(4)]
        out += [("walk d=%d need=%d" % (d, n), empty_grid(d), d, n) for d in (1, 3, 5, 20, 64) for n in (30, 31, 1000)]
        out += [("contents need=%d" % n, contents_grid(levels, scales, 20)[0], 20, n) for n in (31, 1000)]
        out += [("occupied", np.full_like(empty_grid(20), 3), 20, 100)]
    elif scene in ("noise10", "synth10"):
        out += [("ten levels need=%d" % n, empty_grid(5), 5, n) for n in (30, 300, 100000)]
    else:
        out += [("rich d=%d need=%d" % (d, n), empty_grid(d), d, n) for d in (5, 20) for n in (30, 31, 1000, 3000)]
    return out


def batch_of_three(images_, levels_synth, scales):
    """Three frames with their own need, grid and caller keypoints; the third is a constant image: no survivors at all."""
    from describe_cases import keypoints
    d = 5
    g1 = empty_grid(d)
    for r, c in cells(levels_synth, scales, d)[0][::2]:
        g1[r, c] += 1
    return d, [(images_["noise"], keypoints([(2, 2), (W - 3, H - 3)]), empty_grid(d), 30),
               (images_["synth"], keypoints(np.zeros((0, 2))), g1, 1000),
               (images_["const"], keypoints([(50.5, 60.25), (2, H - 3), (W // 2, H // 2)]), empty_grid(d), 50)]
