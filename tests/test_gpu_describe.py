"""k_describe held to tests/describe_model.py at its edges: caller keypoints of the top-up call at every border distance, every tile phase of
the blurred window, the centre's rounding boundaries, every direction of the orientation, descriptor ties, and the shapes of a wavefront's
group of four.  Every case is a top-up call with a grid of all ones and num_featsneeded = 0: the caller keypoints are all that comes back.
The model is evaluated on the GPU's OWN level-0 planes, read back after the call, which pins a mismatch to k_describe alone; the result is
also compared with the oracle's call on the same image.  tests/test_describe_model.py shows without a GPU that the inputs
(tests/describe_cases.py) reach what they aim at.  Everything is compared exactly."""
import numpy as np
import pytest

import describe_cases as dc
import describe_model as dm
from test_gpu_parity import _assert_same_features

pytestmark = pytest.mark.gpu
SENTINEL = 0x5A


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def handles(uvo):
    """One extractor per shape, shared by the cases (a handle keeps its planes between calls: that is part of what is tested)."""
    h = {}
    for w, hh in dc.SHAPES:
        nf, sf, nl, th = dc.cfg(w, hh)
        h[(w, hh)] = uvo.ORBextractor(nf, sf, nl, 0, th, max_width=w, max_height=hh, max_batch=5, max_input_keypoints=dc.IN_CAP)
    yield h
    for ex in h.values():
        ex.close()


@pytest.fixture(scope="module")
def pattern(oracle):
    return oracle.extractor(*dc.CFG).pattern()


def raw_batch(uvo, ex, imgs, kins, grids, min_px, need, full_detect=False):
    """uvo_extract_batch on sentinel-filled outputs: (rc, n_out, out_kp, out_desc, grids after).  kins: per-frame keypoint arrays or None."""
    imgs = np.ascontiguousarray(np.stack(imgs))
    b, h, w = imgs.shape
    in_cap = ex.cfg.max_input_keypoints
    kin = n_in = None
    if kins is not None:
        kin = np.zeros((b, in_cap), uvo.KEYPOINT_DTYPE)
        n_in = np.array([len(k) for k in kins], np.int32)
        for f, k in enumerate(kins):
            kin[f, :len(k)] = k
    out_kp = np.frombuffer(bytes([SENTINEL]) * (b * ex.cap * uvo.KEYPOINT_DTYPE.itemsize), uvo.KEYPOINT_DTYPE).reshape(b, ex.cap).copy()
    out_desc = np.full((b, ex.cap, 32), SENTINEL, np.uint8)
    n_out = np.full(b, -7, np.int32)
    g = None if grids is None else np.ascontiguousarray(np.stack([np.asfortranarray(x).T for x in grids]))   # per frame (rows, cols) column-major
    needs = None if need is None else np.array(need, np.int32)
    ptr = lambda a: None if a is None else a.ctypes.data
    rc = uvo.lib.uvo_extract_batch(ex._h, b, imgs.ctypes.data, w, h, w, w * h, ptr(kin), ptr(n_in), ptr(g), 0 if g is None else g.shape[2],
                                   0 if g is None else g.shape[1], int(min_px), 1 if full_detect else 0, ptr(needs), out_kp.ctypes.data,
                                   out_desc.ctypes.data, ex.cap, n_out.ctypes.data)
    return rc, n_out, out_kp, out_desc, None if g is None else [np.asfortranarray(x.T) for x in g]


def check_frame_against_model(ex, pattern, kin, kp, de, name, frame=0):
    """k_describe alone: angles and descriptors of the caller keypoints from the planes the kernel itself read."""
    plane, blurred = ex.read_plane(0, False, frame), ex.read_plane(0, True, frame)
    angles, desc = dm.describe(plane, blurred, kin["x"], kin["y"], pattern)
    bad = np.nonzero(bits(angles) != bits(kp["angle"]))[0]
    assert len(bad) == 0, "%s: %d angles differ from the model on the GPU's plane, first at (%g, %g): gpu %r, model %r" % (
        name, len(bad), kin["x"][bad[0]], kin["y"][bad[0]], kp["angle"][bad[0]], angles[bad[0]])
    bad = np.nonzero((desc != de).any(1))[0]
    assert len(bad) == 0, "%s: %d descriptors differ from the model on the GPU's planes, at %s" % (
        name, len(bad), [(float(kin["x"][i]), float(kin["y"][i])) for i in bad[:12]])
    return plane, blurred


def check_case(uvo, oracle, ex, pattern, name, img, kin):
    h, w = img.shape
    grid = dc.ones_grid(w, h)
    kp, de = ex(img, kin.copy(), grid, dc.MIN_PX, False, 0)
    assert len(kp) == len(kin), "%s: n_out %d, n_in %d" % (name, len(kp), len(kin))
    assert (grid == 1).all(), name
    oe = oracle.extractor(*dc.cfg(w, h))
    kp_o, de_o = oe(img, kin.copy(), dc.ones_grid(w, h), dc.MIN_PX, False, 0)
    planes = check_frame_against_model(ex, pattern, kin, kp, de, name)
    _assert_same_features(kp, de, kp_o, de_o, name)
    assert kp["x"].tobytes() == kin["x"].tobytes() and kp["y"].tobytes() == kin["y"].tobytes(), name   # the caller's floats, unrounded
    return oe, planes


def blurred_plane_differences(ex_blurred, oe):
    want = oe.level_plane(0, True)
    ys, xs = np.nonzero(ex_blurred != want)
    return len(ys), [(int(x) - 16, int(y) - 16) for x, y in zip(xs[:8], ys[:8])]


@pytest.mark.parametrize("shape", dc.SHAPES)
def test_border_bands(uvo, oracle, handles, pattern, shape):
    """Case 1.  Caller keypoints from 2 pixels inside the border: the steered pattern reaches 18 pixels, 16 of them into the pad, which the
    reference's in-place blur leaves un-blurred.  Twice on one handle: behind a call on another image, and behind a FullDetect call on the
    same one, so that bytes of the blurred plane that this call does not write are another image's or an earlier call's."""
    w, h = shape
    ex = handles[shape]
    img, other, kin = dc.border_case(w, h)
    ex(other, kin.copy(), dc.ones_grid(w, h), dc.MIN_PX, False, 0)
    for lap in ("behind another image", "behind FullDetect"):
        oe, (plane, blurred) = check_case(uvo, oracle, ex, pattern, "border bands %dx%d %s" % (w, h, lap), img, kin)
        # every byte an accepted caller keypoint can sample: the whole level-0 plane with its 16-pixel pad
        n, first = blurred_plane_differences(blurred, oe)
        assert n == 0, "%s: %d bytes of the blurred level-0 plane differ from the reference's, first (image coordinates) %s" % (lap, n, first)
        assert (plane == oe.level_plane(0, False)).all()
        ex(img)


def test_plain_cases(uvo, oracle, handles, pattern):
    """Cases 2, 4, 5 and the accepted positions of case 3."""
    for name, img, kin in dc.plain_cases():
        h, w = img.shape
        check_case(uvo, oracle, handles[(w, h)], pattern, name, img, kin)


@pytest.mark.parametrize("shape", dc.SHAPES)
def test_first_rejected_centres(uvo, handles, shape):
    """Case 3: the first coordinate that rounds out of [2, n - 3] on each side is refused, and nothing is written."""
    w, h = shape
    ex = handles[shape]
    img = dc.noise(3, w, h)
    for axis, n in (("x", w), ("y", h)):
        for bad in dc.rejected_values(n):
            kin = dc.keypoints([(30, 30), (31, 30), (30, 31)])
            kin[axis][1] = bad
            grid = dc.ones_grid(w, h)
            rc, n_out, out_kp, out_desc, g = raw_batch(uvo, ex, [img], [kin], [grid], dc.MIN_PX, [0])
            assert rc == uvo.UVO_E_BADARG, (axis, bad, rc)
            assert n_out[0] == -7 and (out_desc == SENTINEL).all() and out_kp.tobytes() == bytes([SENTINEL]) * out_kp.nbytes and (g[0] == 1).all()


def test_group_shapes(uvo, oracle, synth, handles, pattern):
    """Case 6: batches of 1, 2 and 5 frames with 0 .. 7 caller keypoints per frame -- caller slots only, then caller, level-0, level-1 and
    level-2 slots in one list whose length leaves 1, 2 and 3 live slots in the last group (test_describe_model.py shows it)."""
    w, h = dc.GROUP_SHAPE
    ex = handles[dc.GROUP_SHAPE]
    frames, kps = dc.group_frames(synth)
    oe = oracle.extractor(*dc.cfg(w, h))

    def run(call):
        b = len(call)
        kins = [kps[f][:n] for f, n in enumerate(call)]
        # caller slots only
        rc, n_out, out_kp, out_desc, g = raw_batch(uvo, ex, frames[:b], kins, [dc.ones_grid(w, h)] * b, dc.MIN_PX, [0] * b)
        assert rc == uvo.UVO_OK and n_out.tolist() == list(call), (call, rc, n_out)
        for f, n in enumerate(call):
            assert (g[f] == 1).all()
            kp_o, de_o = oe(frames[f], kins[f].copy(), dc.ones_grid(w, h), dc.MIN_PX, False, 0)
            _assert_same_features(out_kp[f, :n], out_desc[f, :n], kp_o, de_o, "caller slots %s frame %d" % (call, f))
            if n:
                check_frame_against_model(ex, pattern, kins[f], out_kp[f, :n], out_desc[f, :n], "caller slots %s frame %d" % (call, f), f)
            assert (out_desc[f, n:] == SENTINEL).all()                 # dead slots of the last group are not stored
        # slots of every kind in one list
        empty = np.zeros((h // dc.GROUP_MIN_PX + 2, w // dc.GROUP_MIN_PX + 2), np.int32, order="F")
        rc, n_out, out_kp, out_desc, g = raw_batch(uvo, ex, frames[:b], kins, [empty] * b, dc.GROUP_MIN_PX, [dc.GROUP_NEED] * b)
        assert rc == uvo.UVO_OK, (call, rc)
        for f, n in enumerate(call):
            g_o = empty.copy(order="F")
            kp_o, de_o = oe(frames[f], kins[f].copy(), g_o, dc.GROUP_MIN_PX, False, dc.GROUP_NEED)
            _assert_same_features(out_kp[f, :n_out[f]], out_desc[f, :n_out[f]], kp_o, de_o, "mixed slots %s frame %d" % (call, f))
            np.testing.assert_array_equal(g[f], g_o)
            assert (out_desc[f, n_out[f]:] == SENTINEL).all()
        # FullDetect ignores the caller keypoints
        rc, n_full, kp_full, de_full, _ = raw_batch(uvo, ex, frames[:b], kins, None, 0, None, full_detect=True)
        rc2, n_plain, kp_plain, de_plain, _ = raw_batch(uvo, ex, frames[:b], None, None, 0, None, full_detect=True)
        assert rc == rc2 == uvo.UVO_OK and n_full.tolist() == n_plain.tolist() and (n_full > 20).all()
        assert kp_full.tobytes() == kp_plain.tobytes() and (de_full == de_plain).all(), call

    for call in dc.GROUP_CALLS:
        run(call)
    ex.tune(uvo.UVO_TUNE_ZERO_COPY_OUT, 0)
    try:
        run(dc.GROUP_CALLS[-1])
        run((7,))
    finally:
        ex.tune(uvo.UVO_TUNE_ZERO_COPY_OUT, 1)


def test_pad_copy_runs_only_with_caller_keypoints(uvo, handles):
    """The launch that completes level 0's pad in the blurred plane belongs to calls that carry caller keypoints; every other call launches
    exactly the kernels it launched before that kernel existed."""
    w, h = dc.SHAPES[0]
    ex = handles[dc.SHAPES[0]]
    img, _, kin = dc.border_case(w, h)

    def launched(call):
        ex.profile(True)
        try:
            call()
            return {k: n for k, (ms, n) in ex.kernel_times().items()}
        finally:
            ex.profile(False)

    full = launched(lambda: ex(img))
    tracked = launched(lambda: ex.extract_tracked(img, kin[:40], dc.MIN_PX, 50))
    topup_plain = launched(lambda: ex(img, None, dc.ones_grid(w, h), dc.MIN_PX, False, 50))
    topup_kin = launched(lambda: ex(img, kin.copy(), dc.ones_grid(w, h), dc.MIN_PX, False, 50))
    print("FullDetect:", full, "\nextract_tracked:", tracked, "\ntop-up:", topup_plain, "\ntop-up with keypoints:", topup_kin)
    for name, got in (("FullDetect", full), ("extract_tracked", tracked), ("top-up without keypoints", topup_plain)):
        assert "k_blur_pad_level0" not in got and "k_describe" in got, (name, got)
    assert "k_assemble" not in full and tracked.get("k_assemble") == 1 and tracked.get("k_occupancy_grid", 1) == 1
    assert topup_kin.get("k_blur_pad_level0") == 1 and topup_kin.get("k_pad_level0") == 1
    rest = dict(topup_kin)
    del rest["k_blur_pad_level0"]
    rest.pop("k_pad_level0")
    plain = dict(topup_plain)
    plain.pop("k_pad_level0", None)
    assert rest == plain, (rest, plain)
