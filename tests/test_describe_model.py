"""tests/describe_model.py held to the oracle on the very inputs of tests/test_gpu_describe.py (tests/describe_cases.py), and the coverage
conditions of those inputs shown from the oracle alone: no GPU."""
from fractions import Fraction

import numpy as np
import pytest

import describe_cases as dc
import describe_model as dm


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def oracle_run(oracle, img, kin, grid=None, need=0, min_px=dc.MIN_PX):
    """The top-up call of the cases on the oracle: (extractor with its planes, keypoints, descriptors, grid after the call)."""
    h, w = img.shape
    oe = oracle.extractor(*dc.cfg(w, h))
    g = dc.ones_grid(w, h) if grid is None else grid.copy(order="F")
    kp, de = oe(img, kin.copy(), g, min_px, False, need)
    return oe, kp, de, g


def check_model_on_oracle(oracle, name, img, kin):
    """Both model functions reproduce the oracle's call, from the oracle's own planes; returns (keypoints, descriptors)."""
    oe, kp, de, g = oracle_run(oracle, img, kin)
    assert len(kp) == len(kin) and (g == 1).all(), name              # every detected point is rejected, the grid stays
    assert all(kp[f].tobytes() == kin[f].tobytes() for f in ("x", "y", "size", "response", "octave", "class_id")), name   # the caller's floats, unrounded
    plane, blurred = oe.level_plane(0, False), oe.level_plane(0, True)
    pad = np.ones(plane.shape, bool)
    pad[16:-16, 16:-16] = False
    assert (plane[pad] == blurred[pad]).all(), name                  # the reference blurs the ROI: the whole pad stays un-blurred
    angles, desc = dm.describe(plane, blurred, kin["x"], kin["y"], oe.pattern())
    bad = np.nonzero(bits(angles) != bits(kp["angle"]))[0]
    assert len(bad) == 0, "%s: angle of keypoint %d (%g, %g): model %r, oracle %r" % (name, bad[0], kin["x"][bad[0]], kin["y"][bad[0]], angles[bad[0]], kp["angle"][bad[0]])
    bad = np.nonzero((desc != de).any(1))[0]
    assert len(bad) == 0, "%s: descriptor of keypoint %d (%g, %g)" % (name, bad[0], kin["x"][bad[0]], kin["y"][bad[0]])
    return oe, kp, de


def test_tables_and_scalars(oracle):
    oe = oracle.extractor(*dc.CFG)
    assert dm.UMAX.tolist() == oe.umax.tolist()
    # fastAtan2 over every integer direction of the patch, the axes, the diagonals, the origin, and moments as large as they get
    vals = list(range(-16, 17)) + [255 * 15 * 300, -255 * 15 * 300, 1000, -1000, 16777216, 16777217]
    for y in vals:
        got = dm.fast_atan2(np.full(len(vals), y, np.float32), np.array(vals, np.float32))
        want = np.array([oracle.fast_atan2(y, x) for x in vals], np.float32)
        assert (bits(got) == bits(want)).all(), y
    # the sine / cosine of every angle fastAtan2 can hand over is libm's (sampled densely: 0 .. 360 degrees in 2^-7 steps and their float neighbours)
    deg = np.arange(0, 360 * 128 + 1, dtype=np.float32) / np.float32(128)
    for d in np.concatenate([deg[::7], np.nextafter(deg[::13], np.float32(400)), dm.fast_atan2(np.arange(-16, 17, dtype=np.float32)[:, None], np.arange(-16, 17, dtype=np.float32)[None, :]).ravel()]):
        a = np.float32(d) * np.float32(np.pi / 180.0)
        s, c = dm.sincosf(a)
        so, co = oracle.sincosf(a)
        assert bits(s) == bits(np.float32(so)) and bits(c) == bits(np.float32(co)), d


@pytest.mark.parametrize("shape", dc.SHAPES)
def test_border_bands(oracle, shape):
    w, h = shape
    img, other, kin = dc.border_case(w, h)
    oe, kp, de = check_model_on_oracle(oracle, "border", img, kin)
    # coverage: the centres are the issue's; their samples reach deeper into the pad than the blur's 4-pixel ring on every side, and the
    # oracle's entry points agree at the issue's four spot positions
    cx, cy = kin["x"].astype(int), kin["y"].astype(int)
    assert {(2, 2), (w - 3, h - 3), (2, h - 3), (w - 3, 2)} <= set(zip(cx.tolist(), cy.tolist()))
    for x in list(range(2, 20)) + list(range(w - 20, w - 2)):
        assert ((cx == x) & (cy == h // 2)).any()
    for y in list(range(2, 20)) + list(range(h - 20, h - 2)):
        assert ((cy == y) & (cx == w // 2)).any()
    lo_r = lo_c = 99
    hi_r = hi_c = 0
    for k in kp:
        dr, dcol = dm.sample_offsets(oe.pattern(), k["angle"])
        lo_r, hi_r = min(lo_r, int(k["y"]) + 16 + dr.min()), max(hi_r, int(k["y"]) + 16 + dr.max())
        lo_c, hi_c = min(lo_c, int(k["x"]) + 16 + dcol.min()), max(hi_c, int(k["x"]) + 16 + dcol.max())
    print("padded rows %d..%d of %d, columns %d..%d of %d sampled" % (lo_r, hi_r, h + 32, lo_c, hi_c, w + 32))
    assert lo_r < 6 and lo_c < 6 and hi_r > h + 25 and hi_c > w + 25 and lo_r >= 0 and lo_c >= 0 and hi_r < h + 32 and hi_c < w + 32
    plane, blurred = oe.level_plane(0, False), oe.level_plane(0, True)
    for x, y in ((2, 2), (w - 3, h - 3), (8, 40), (13, 40)):
        i = int(np.nonzero((cx == x) & (cy == y))[0][0])
        assert bits(oe.ic_angle(plane, x, y)) == bits(kp["angle"][i]) == bits(dm.ic_angle(plane, x, y))
        assert (oe.descriptor(blurred, x, y, kp["angle"][i]) == de[i]).all()
    # the second image of the GPU test differs from the first in the pad: stale bytes would show
    assert (oracle.border101(img) != oracle.border101(other)).mean() > 0.9


def test_plain_cases(oracle):
    octants, on_axis, directions = set(), set(), set()
    ones, zeros = np.zeros(256, bool), np.zeros(256, bool)
    for name, img, kin in dc.plain_cases():
        oe, kp, de = check_model_on_oracle(oracle, name, img, kin)
        h, w = img.shape
        what = name.split("/")[1]
        if what == "tile_phases":
            t = np.array([dc.window_tiles(int(x), int(y)) for x, y in zip(kin["x"], kin["y"])])
            assert len(set(map(tuple, t[:, :2]))) == 128 and t[:, 2].max() == 4 and t[:, 3].max() == 6 and t[:, 2].min() == 3 and t[:, 3].min() == 5
            assert (kin["x"] == 2).any() and (kin["x"] == w - 3).any() and (kin["y"] == 2).any() and (kin["y"] == h - 3).any()
        if what == "rounding":
            for n, v in ((w, dc.rounding_values(w)), (h, dc.rounding_values(h))):
                r = dm.cv_round(v).tolist()
                assert r[:6] == [40, 40, 41, 42, 41, 42] and r[6:10] == [2, 2, 2, 3] and r[10:] == [n - 3, n - 3, n - 4], r
                assert dm.cv_round(dc.rejected_values(n)).tolist() == [1, n - 2]
        if what.startswith("pixel"):
            # the keypoint at (cx - u, cy - v) sees the pixel at (u, v): inside the disc fastAtan2(v, u), outside it fastAtan2(0, 0)
            u, v = w // 2 - kin["x"].astype(int), h // 2 - kin["y"].astype(int)
            inside = (np.abs(v) <= 15) & (np.abs(u) <= dm.UMAX[np.minimum(np.abs(v), 15)])
            want = np.where(inside, dm.fast_atan2(v.astype(np.float32), u.astype(np.float32)), dm.fast_atan2(np.float32(0), np.float32(0)))
            assert (bits(kp["angle"]) == bits(want)).all(), name
            assert (~inside).sum() >= 33 * 4 - 4 and inside.sum() > 700
            directions |= {(Fraction(int(b), int(a)) if a else None, int(np.sign(a)), int(np.sign(b))) for a, b in zip(u[inside], v[inside]) if a or b}
            assert all(bits(kp["angle"][(u == a) & (v == b)])[0] == bits(np.float32(d)) for a, b, d in ((3, 0, 0), (0, 3, 90), (-3, 0, 180), (0, -3, 270)))
        if what in ("pair_plus", "pair_minus"):
            i = int(np.nonzero((kin["x"] == w // 2) & (kin["y"] == h // 2))[0][0])
            m01, m10 = dm.moments(oe.level_plane(0, False), w // 2, h // 2)
            assert (m01, m10) == ((1000, 1000) if what == "pair_plus" else (-1000, 1000))
        if what == "symmetric":
            assert dm.moments(oe.level_plane(0, False), w // 2, h // 2) == (0, 0) and kp["angle"][4] == 0
        if what.startswith("const"):
            # every t0 < t1 is false wherever the samples stay on one side of the ROI's edge.  (The taps sum to 257 per pass: a
            # constant 128 blurs to 129 inside the ROI and stays 128 in the pad, so the four corner keypoints of that image compare
            # unequal bytes; 0 stays 0 and 255 saturates.  The un-blurred plane is constant: no moments, angle 0 everywhere.)
            corner = (kin["x"] < 16) | (kin["x"] > w - 17)
            assert corner.sum() == 4 and not de[~corner].any() and (kp["angle"] == 0).all(), name
            assert de[corner].any() == (what == "const128"), name
        if what.startswith("gradient"):
            b = np.unpackbits(de, axis=1, bitorder="little").astype(bool)
            ones |= b.any(0)
            zeros |= (~b).any(0)
        if not what.startswith(("const", "gradient")):
            a = kp["angle"]
            octants |= set((a[(a % 45) != 0] // 45).astype(int).tolist())
            on_axis |= set(a[(a % 90) == 0].astype(int).tolist())
    print("octants %s, axis angles %s, %d directions, descriptor bits set %d / clear %d" % (sorted(octants), sorted(on_axis), len(directions), ones.sum(), zeros.sum()))
    assert octants == set(range(8)) and {0, 90, 180, 270} <= on_axis
    assert len(directions) > 400          # the disc's 700-odd offsets are 464 distinct rational directions
    assert ones.all() and zeros.all()


def test_group_shapes(oracle, synth):
    """Case 6 from the oracle: with an empty grid and 1000 wanted, the frames' totals leave 1, 2 and 3 slots in their last group of four and
    slots of the caller, of level 0, 1 and 2 share groups."""
    frames, kps = dc.group_frames(synth)
    w, h = dc.GROUP_SHAPE
    residues = set()
    for call in dc.GROUP_CALLS:
        for f, n_in in enumerate(call):
            grid = np.zeros((h // dc.GROUP_MIN_PX + 2, w // dc.GROUP_MIN_PX + 2), np.int32, order="F")
            oe, kp, de, g = oracle_run(oracle, frames[f], kps[f][:n_in], grid, dc.GROUP_NEED, dc.GROUP_MIN_PX)
            octave = kp["octave"][n_in:]
            assert (np.diff(octave) >= 0).all() and set(octave.tolist()) == {0, 1, 2}, (call, f)
            bounds = [n_in] + [n_in + int((octave <= l).sum()) for l in range(2)]
            assert any(b % 4 for b in bounds), (call, f, bounds)      # a group of four holds slots of two kinds
            residues.add(len(kp) % 4)
            if n_in:
                check_model_on_oracle(oracle, "group %s frame %d" % (call, f), frames[f], kps[f][:n_in])
    print("totals modulo 4:", sorted(residues))
    assert {1, 2, 3} <= residues
