"""GPU parity of the blur's walk (csrc/gauss_body.hpp: gauss7_body, run by k_gauss7 and by the blur workgroups of k_octree_gauss) at the
edges of its strip plan: the region the blur writes -- padded rows and columns [12, n + 20) -- of every level of every frame, byte for
byte against the oracle's blurred plane, under both rounding contracts, with level 0 read in place and from the padded copy, with the
blur fused into the quad-tree launch and on its own.  Every run asserts through kernel_times() which kernels it took.

A wavefront walks one strip of a level's region (w + 8) x (h + 8) down a segment of rows (16 per segment below 16 frames, 64 from 16 on);
fast_strip_plan (csrc/strip_plan.hpp, compiled on the host: tests/emu/blur_plan_emu.cpp) cuts the region into `nfull` full strips of 248
columns and up to two narrow ones that hold sub = 2 / 4 segments side by side.  The sizes are the smallest the extractor accepts (a level
is at least 56 x 56, level 0 in place at least 64 x 64 with a width that is a multiple of 4) that give the plans below; test_plans holds
them to this list without a GPU.

  image, levels, frames     level: size      w%4  region    nfull nseg sub     what
  200 x  64, 1,  3          0: 200 x  64      0   208 x 72    1     5  -       a full strip only
  304 x 104, 2,  3          0: 304 x 104      0   312 x 112   1     7  2       a full strip + a two-segment strip; 7 segments: the last item's
                                                                               second sub-strip lies below the level
                            1: 253 x  87      1   261 x 95    1     6  4       a full strip + a four-segment strip whose second item holds 2 of 4
                                                                               sub-strips; 95 rows: no multiple of 8 or 16 (incomplete last group)
  148 x 121, 2,  3          0: 148 x 121      0   156 x 129   0     9  2, 4    narrow strips only, both kinds, odd segment counts
                            1: 123 x 101      3   131 x 109   0     7  2, 4    three scalar-tail columns, in a narrow strip
  156 x 121, 2,  3          1: 130 x 101      2   138 x 109   0     7  2, 4    two scalar-tail columns
   64 x  64, 1, 16          0:  64 x  64      0    72 x 72    0     2  2       64-row segments: ONE wavefront, the upper reflected border in its
                                                                               first sub-strip and the lower one in its second
   67 x  56, 1, 16          0:  67 x  56      3    75 x 64    1     1  -       one 64-row segment holds both borders (padded copy only: 67 is odd)
  640 x 512, 8, 16          the benchmark's geometry at the benchmark's 64-row segments: two full strips + both narrow kinds on level 0, tail
                            columns 1, 2 and 3 further up; frames 0, 7 and 15 are compared

Frames are uniform noise (every level keeps keypoints, so the oracle blurs every level), the last one of a batch in 200 .. 255 (sums that
saturate).  A wrong frame stride shows in frames 1 and 2.
"""
import ctypes

import numpy as np
import pytest

import host_build

# (width, height, levels, frames, frames compared) -> per level (nfull, nseg, sub[0], sub[1]) at the batch's rows per segment
CASES = {
    (200, 64, 1, 3): [(1, 5, 0, 0)],
    (304, 104, 2, 3): [(1, 7, 2, 0), (1, 6, 4, 0)],
    (148, 121, 2, 3): [(0, 9, 2, 4), (0, 7, 2, 4)],
    (156, 121, 2, 3): [(0, 9, 2, 4), (0, 7, 2, 4)],
    (64, 64, 1, 16): [(0, 2, 2, 0)],
    (67, 56, 1, 16): [(1, 1, 0, 0)],
    (640, 512, 8, 16): [(2, 9, 2, 4), (2, 7, 4, 0), (2, 6, 0, 0), (2, 5, 0, 0), (1, 4, 2, 0), (1, 4, 4, 0), (1, 3, 0, 0), (1, 3, 0, 0)],
}
LEVEL_SIZES = {
    (200, 64, 1, 3): [(200, 64)], (304, 104, 2, 3): [(304, 104), (253, 87)], (148, 121, 2, 3): [(148, 121), (123, 101)],
    (156, 121, 2, 3): [(156, 121), (130, 101)], (64, 64, 1, 16): [(64, 64)], (67, 56, 1, 16): [(67, 56)],
    (640, 512, 8, 16): [(640, 512), (533, 427), (444, 356), (370, 296), (309, 247), (257, 206), (214, 171), (179, 143)],
}


def _rows_per_seg(frames):
    return 64 if frames >= 16 else 16       # gauss7_rows_per_seg (csrc/gauss.hip)


def _plan_lib():
    E = ctypes.CDLL(host_build.build("blur_plan_emu"))
    E.emu_strip_plan.argtypes = [ctypes.c_int] * 3 + [ctypes.c_void_p]
    return E


def test_plans():
    """the sizes give the plans the cases are named for (no GPU: fast_strip_plan compiled on the host)"""
    E = _plan_lib()
    for case, want in CASES.items():
        rps = _rows_per_seg(case[3])
        for (w, h), plan in zip(LEVEL_SIZES[case], want):
            out = (ctypes.c_int * 7)()
            E.emu_strip_plan(w + 8, h + 8, rps, out)
            assert (out[0], out[1], out[3], out[4]) == plan, (case, (w, h), list(out))
    # what the cases stand for
    assert (95 % 8, 95 % 16) == (7, 15) and 7 % 2 == 1 and 6 % 4 == 2
    assert sorted({w % 4 for sizes in LEVEL_SIZES.values() for (w, h) in sizes}) == [0, 1, 2, 3]


def _frames(w, h, n, seed):
    rng = np.random.default_rng(seed)
    imgs = rng.integers(0, 256, (n, h, w)).astype(np.uint8)
    imgs[n - 1] = rng.integers(200, 256, (h, w)).astype(np.uint8)
    return imgs


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES), ids=lambda c: "%dx%d_l%d_b%d" % c)
def test_blur_walk(uvo, oracle, case):
    w, h, nlev, B = case
    compared = (0, 1, 2) if B == 3 else (0, 7, 15)
    imgs = _frames(w, h, B, 9100 + w + h)
    ex = uvo.ORBextractor(500, 1.2, nlev, 0, 20, max_width=w, max_height=h, max_batch=B)
    oe = oracle.extractor(500, 1.2, nlev, 20)
    ex.tune(uvo.UVO_TUNE_OCT_WIDE_MAX, 0)          # the fused launch at any batch the interleave admits
    can_inplace = w % 4 == 0 and w >= 64 and h >= 64
    fused_seen = False
    for mode, tune in ((0, uvo.UVO_BLUR_ROUNDING_SCALAR), (1, uvo.UVO_BLUR_ROUNDING_SSE2)):
        oe.set_blur_rounding(mode)
        want = {}
        for f in compared:
            kp_o, _ = oe(imgs[f])
            assert all((kp_o["octave"] == l).any() for l in range(nlev)), "the oracle blurs only levels that keep keypoints"
            want[f] = [oe.level_plane(l, True)[12:-12, 12:-12].copy() for l in range(nlev)]
        ex.tune(uvo.UVO_TUNE_BLUR_ROUNDING, tune)
        for inplace in (1, 0):
            for fuse in (1, 0):
                ex.tune(uvo.UVO_TUNE_LEVEL0_INPLACE, inplace)
                ex.tune(uvo.UVO_TUNE_FUSE_BLUR_TREE, fuse)
                ex.profile(True)
                ex.extract_batch(imgs)
                kt = ex.kernel_times()
                assert [ex.level_dims(l) for l in range(nlev)] == LEVEL_SIZES[case]
                ex.profile(False)
                what = "%s contract %d inplace %d fuse %d" % (case, mode, inplace, fuse)
                assert ("k_pad_level0" not in kt) == bool(inplace and can_inplace), (what, sorted(kt))
                assert ("k_gauss7" in kt) != ("k_octree_gauss" in kt), (what, sorted(kt))
                if not fuse:
                    assert "k_gauss7" in kt, (what, sorted(kt))
                fused_seen |= "k_octree_gauss" in kt
                for f in compared:
                    for l in range(nlev):
                        np.testing.assert_array_equal(ex.read_plane(l, True, f)[12:-12, 12:-12], want[f][l], err_msg="%s frame %d level %d" % (what, f, l))
    # the interleave needs two blur workgroups per quad-tree problem: the one-wavefront cases cannot fuse, every other case has to
    assert fused_seen == (case not in ((64, 64, 1, 16), (67, 56, 1, 16))), case
    ex.close()
