"""GPU parity of k_resize_level_rows (csrc/pyramid.hip; schedule: csrc/resize_rows.hpp) -- the per-level resize of a batch as a walk down
row bands -- against the oracle's ComputePyramid (src/ORBextractor.cc:963-1004), forced through UVO_PYR_FORM_ROWS.

Planes are compared with UVO_TUNE_PYR_RING = 0: the launch then writes the whole padded plane and read_plane re-launches nothing (with a
ring it completes a level's border by running k_resize_level over the whole plane, which would overwrite what the batch wrote).  At ring 4,
8 and 12 keypoints and descriptors are compared byte for byte: they were computed from the batch's own planes.  Every run asserts through
kernel_times() which kernel its levels took.

Shapes, each for a way the walk can go wrong: rows shorter than a wavefront (a wavefront straddles frames, several frames in one
wavefront), last bands shorter than UVO_RESIZE_BAND (16) and level heights of exactly n x 16 and n x 16 + 1 rows, level 1 from the padded
copy with partial last dwords, level 1 in place with the last frame ending at the end of its allocation (the frame-end guard), scale
factors 1.1 and 1.33 (other step patterns of the source rows), 1.5 and 2.0 (byte-gather levels keep k_resize_level), two pipeline lanes."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RINGS = (4, 8, 12)


def _profiled(ex, nlev, rows_levels, run):
    """runs `run` under the profiler and asserts that rows_levels of the nlev - 1 resize launches were k_resize_level_rows"""
    ex.profile(True)
    out = run()
    kt = ex.kernel_times()
    spread = ex.last_spread
    ex.profile(False)
    got_rows, got_old = kt.get("k_resize_level_rows", (0.0, 0))[1], kt.get("k_resize_level", (0.0, 0))[1]
    assert (got_rows, got_old) == (rows_levels, nlev - 1 - rows_levels), kt
    assert "k_pyr_tiles" not in kt
    if rows_levels >= 2:
        assert 0 < spread["k_resize_level_rows"]["min"] <= spread["k_resize_level_rows"]["max"]
    return out


class _Oracle:
    """the oracle's keypoints, descriptors and planes of a frame, computed once per (extractor, frame)"""

    def __init__(self, oe, nlev):
        self.oe, self.nlev, self.cache = oe, nlev, {}

    def __call__(self, key, img):
        if key not in self.cache:
            kp, de = self.oe(img)
            self.cache[key] = (kp, de, [self.oe.level_plane(l).copy() for l in range(self.nlev)])
        return self.cache[key]


def _check_batch(uvo, ex, orc, imgs, nlev, rows_levels, frames, what, key0=0):
    """ring 0: planes, keypoints and descriptors of `frames`; rings 4, 8, 12: keypoints and descriptors"""
    for ring in (0,) + RINGS:
        ex.tune(uvo.UVO_TUNE_PYR_RING, ring)
        out = _profiled(ex, nlev, rows_levels, lambda: ex.extract_batch(imgs))
        for f in frames:
            kp_o, de_o, planes = orc(key0 + f, imgs[f])
            kp, de = out[f]
            assert kp.tobytes() == kp_o.tobytes() and (de == de_o).all(), "%s ring %d frame %d" % (what, ring, f)
            if ring == 0:
                for l in range(nlev):
                    np.testing.assert_array_equal(ex.read_plane(l, frame=f), planes[l], err_msg="%s frame %d level %d" % (what, f, l))


@pytest.fixture(scope="module")
def straddle(uvo, oracle, synth):
    w, h, nlev = 320, 256, 6
    imgs = synth.make_batch(40, w, h, seed0=7300)
    ex = uvo.ORBextractor(400, 1.2, nlev, 0, 20, max_width=w, max_height=h, max_batch=40)
    ex.tune(uvo.UVO_TUNE_PYR_FORM, uvo.UVO_PYR_FORM_ROWS)
    yield ex, _Oracle(oracle.extractor(400, 1.2, nlev, 20), nlev), imgs, nlev
    ex.close()


@pytest.mark.parametrize("n", [9, 33, 40])
def test_wavefronts_that_straddle_frames(uvo, straddle, n):
    """320 x 256, six levels: from level 2 on a row is shorter than a wavefront's 64 dwords, so a wavefront holds the end of one frame's row and
    the start of the next frame's -- first, middle and last frame of batches whose entry counts are no multiple of 64."""
    ex, orc, imgs, nlev = straddle
    _check_batch(uvo, ex, orc, imgs[:n], nlev, nlev - 1, sorted({0, n // 2, n - 1}), "batch %d" % n)


@pytest.mark.parametrize("shape,nlev", [((97, 131), 3), ((637, 509), 7), ((333, 301), 5), ((320, 230), 3), ((320, 232), 3)])
def test_small_unaligned_and_band_multiple_shapes(uvo, oracle, synth, shape, nlev):
    """97 x 131: several frames in one wavefront, last bands shorter than 16 rows.  637 x 509, 333 x 301: level 1 from the padded copy of level 0,
    partial last dwords.  320 x 230 / 232: level 1 is 224 = 14 x 16 and 225 = 14 x 16 + 1 padded rows."""
    w, h = shape
    imgs = synth.make_batch(9, w, h, seed0=7400 + w)
    ex = uvo.ORBextractor(500, 1.2, nlev, 0, 20, max_width=w, max_height=h, max_batch=9)
    ex.tune(uvo.UVO_TUNE_PYR_FORM, uvo.UVO_PYR_FORM_ROWS)
    _check_batch(uvo, ex, _Oracle(oracle.extractor(500, 1.2, nlev, 20), nlev), imgs, nlev, nlev - 1, (0, 4, 8), "%dx%d" % shape)
    ex.close()


@pytest.mark.parametrize("shape,scale,nlev,rows_levels", [((200, 180), 1.1, 6, 5), ((333, 222), 1.33, 5, 4), ((400, 300), 1.5, 4, 0), ((512, 384), 2.0, 3, 0)])
def test_scale_factors(uvo, oracle, synth, shape, scale, nlev, rows_levels):
    """1.1: the source rows step by one, rarely by two (most reuse); 1.33: by one or two, two a third of the time (least reuse the 12-byte window
    admits).  1.5 and 2.0 gather bytes: every level reports k_resize_level, whatever the form asked for."""
    w, h = shape
    imgs = synth.make_batch(9, w, h, seed0=7500 + w)
    ex = uvo.ORBextractor(500, scale, nlev, 0, 20, max_width=w, max_height=h, max_batch=9)
    ex.tune(uvo.UVO_TUNE_PYR_FORM, uvo.UVO_PYR_FORM_ROWS)
    _check_batch(uvo, ex, _Oracle(oracle.extractor(500, scale, nlev, 20), nlev), imgs, nlev, rows_levels, (0, 8), "%dx%d scale %.2f" % (w, h, scale))
    ex.close()


@pytest.mark.parametrize("W,H,B,stride_extra,off", [(320, 240, 9, 0, 0), (320, 240, 9, 64, 4 * 37), (316, 200, 9, 4, 8), (320, 240, 9, 3, 0), (320, 240, 9, 64, 1),
                                                    (640, 512, 3, 0, 0)])
def test_level1_in_place_up_to_the_end_of_the_allocation(uvo, oracle, synth, W, H, B, stride_extra, off):
    """The in-place cases of test_level0_is_read_in_place_from_the_callers_rows (dword-aligned rows: level 1 reads the caller's image; a stride or
    a base that is not: the padded copy) with the images inside a noise buffer that ends with the last frame's last pixel: the 12-byte windows
    of that row's last lanes must stay inside the frame."""
    torch = pytest.importorskip("torch")
    nlev = 6 if W >= 600 else 4
    stride = W + stride_extra
    fstride = stride * H + 4 * 11 * (stride % 4 == 0) + (0 if stride % 4 == 0 else 7)
    rng = np.random.default_rng(W * 7 + H + off)
    host = rng.integers(0, 256, off + (B - 1) * fstride + stride * (H - 1) + W, dtype=np.uint8)
    frames = [synth.make_frame(7600 + W + b, W, H) for b in range(B)]
    for b in range(B):
        for y in range(H):
            o = off + b * fstride + y * stride
            host[o:o + W] = frames[b][y]
    buf = torch.from_numpy(host).cuda()
    orc = _Oracle(oracle.extractor(500, 1.2, nlev, 20), nlev)
    ex = uvo.ORBextractor(500, 1.2, nlev, 0, 20, max_width=W, max_height=H, max_batch=B)
    ex.tune(uvo.UVO_TUNE_PYR_FORM, uvo.UVO_PYR_FORM_ROWS)
    cap = ex.cap
    for ring in (0,) + RINGS:
        ex.tune(uvo.UVO_TUNE_PYR_RING, ring)
        kp = torch.zeros((B, cap, 7), dtype=torch.float32, device="cuda")
        de = torch.zeros((B, cap, 32), dtype=torch.uint8, device="cuda")
        n = torch.zeros(B, dtype=torch.int32, device="cuda")

        def run():
            ex.extract_batch_device(buf.data_ptr() + off, B, W, H, kp.data_ptr(), de.data_ptr(), n.data_ptr(), cap, stride=stride, frame_stride=fstride)
            ex.synchronize()
        _profiled(ex, nlev, nlev - 1, run)
        cnt = n.cpu().numpy()
        for b in sorted({0, B // 2, B - 1}):
            kp_o, de_o, planes = orc(b, frames[b])
            k, d = kp[b, :cnt[b]].cpu().numpy(), de[b, :cnt[b]].cpu().numpy()
            assert len(k) == len(kp_o) and (d == de_o).all(), "ring %d frame %d" % (ring, b)
            assert np.array_equal(k[:, 0], kp_o["x"]) and np.array_equal(k[:, 1], kp_o["y"]) and np.array_equal(k[:, 3], kp_o["angle"])
            if ring == 0:
                for l in range(1, nlev):
                    np.testing.assert_array_equal(ex.read_plane(l, frame=b), planes[l], err_msg="frame %d level %d" % (b, l))
    assert (buf.cpu().numpy() == host).all()                 # the caller's buffer is read only
    ex.close()


def test_two_pipeline_lanes_three_batches(uvo, oracle, synth):
    """set_pipeline(2): each lane has its own planes; three consecutive batches of different frames."""
    w, h, nlev, B = 320, 256, 6, 9
    imgs = synth.make_batch(3 * B, w, h, seed0=7700)
    orc = _Oracle(oracle.extractor(400, 1.2, nlev, 20), nlev)
    ex = uvo.ORBextractor(400, 1.2, nlev, 0, 20, max_width=w, max_height=h, max_batch=B)
    ex.set_pipeline(2)
    ex.tune(uvo.UVO_TUNE_PYR_FORM, uvo.UVO_PYR_FORM_ROWS)
    for ring in (0, 4):
        ex.tune(uvo.UVO_TUNE_PYR_RING, ring)
        for k in range(3):
            batch = imgs[k * B:(k + 1) * B]
            out = _profiled(ex, nlev, nlev - 1, lambda: ex.extract_batch(batch))
            for f in (0, B - 1):
                kp_o, de_o, planes = orc(k * B + f, batch[f])
                assert out[f][0].tobytes() == kp_o.tobytes() and (out[f][1] == de_o).all(), "ring %d batch %d frame %d" % (ring, k, f)
                if ring == 0:
                    for l in range(nlev):
                        np.testing.assert_array_equal(ex.read_plane(l, frame=f), planes[l], err_msg="batch %d frame %d level %d" % (k, f, l))
    ex.close()


def test_auto_takes_the_rows_form_only_above_eight_frames(uvo, synth):
    """UVO_PYR_FORM_AUTO: batches up to 8 frames keep k_pyr_tiles, larger ones take the per-level launches, k_resize_level_rows on the levels
    whose launch is large enough for it; UVO_PYR_FORM_LEVELS keeps k_resize_level on every level."""
    w, h, nlev = 320, 256, 6
    imgs = synth.make_batch(40, w, h, seed0=7800)
    ex = uvo.ORBextractor(400, 1.2, nlev, 0, 20, max_width=w, max_height=h, max_batch=40)
    for n in (1, 8):
        ex.profile(True)
        ex.extract_batch(imgs[:n])
        kt = ex.kernel_times()
        ex.profile(False)
        assert "k_pyr_tiles" in kt and "k_resize_level" not in kt and "k_resize_level_rows" not in kt, kt
    ex.profile(True)
    ex.extract_batch(imgs)
    kt = ex.kernel_times()
    ex.profile(False)
    assert "k_pyr_tiles" not in kt and kt.get("k_resize_level_rows", (0, 0))[1] + kt.get("k_resize_level", (0, 0))[1] == nlev - 1, kt
    ex.tune(uvo.UVO_TUNE_PYR_FORM, uvo.UVO_PYR_FORM_LEVELS)
    _profiled(ex, nlev, 0, lambda: ex.extract_batch(imgs))
    with pytest.raises(uvo.UvoError):
        ex.tune(uvo.UVO_TUNE_PYR_FORM, uvo.UVO_PYR_FORM_ROWS + 1)
    ex.close()


def test_auto_takes_the_rows_form_on_large_launches(uvo, oracle, synth):
    """UVO_PYR_FORM_AUTO at 256 frames of 320 x 256: level 1 is a launch of a few thousand wavefronts and walks row bands, the smaller levels
    keep k_resize_level -- one pyramid from two kernels, byte for byte the oracle's."""
    w, h, nlev, B = 320, 256, 6, 256
    imgs = np.concatenate([synth.make_batch(32, w, h, seed0=7900)] * 8)
    orc = _Oracle(oracle.extractor(400, 1.2, nlev, 20), nlev)
    ex = uvo.ORBextractor(400, 1.2, nlev, 0, 20, max_width=w, max_height=h, max_batch=B)
    for ring in (0, 4):
        ex.tune(uvo.UVO_TUNE_PYR_RING, ring)
        ex.profile(True)
        out = ex.extract_batch(imgs)
        kt = ex.kernel_times()
        ex.profile(False)
        n_rows, n_old = kt.get("k_resize_level_rows", (0, 0))[1], kt.get("k_resize_level", (0, 0))[1]
        assert n_rows >= 1 and n_old >= 1 and n_rows + n_old == nlev - 1 and "k_pyr_tiles" not in kt, kt
        for f in (0, 100, B - 1):
            kp_o, de_o, planes = orc(f % 32, imgs[f])
            assert out[f][0].tobytes() == kp_o.tobytes() and (out[f][1] == de_o).all(), "ring %d frame %d" % (ring, f)
            if ring == 0:
                for l in range(nlev):
                    np.testing.assert_array_equal(ex.read_plane(l, frame=f), planes[l], err_msg="frame %d level %d" % (f, l))
    ex.close()
