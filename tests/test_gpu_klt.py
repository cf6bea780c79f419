"""The KLT tracker (csrc/klt.hip) against the CPU oracle at the reference's window sizes and depths, at both instances of k_klt_track
(<7>: windows of up to 448 pixels, <16>: 449 to 1024), with non-square windows, odd image sizes, every termination criterion, points on
the image-bounds edges, non-finite coordinates and pyramid slots built below the handle's size.

The bar is the one of test_gpu_parity.py::test_klt_pyramid_and_tracking: pyramid levels and derivatives byte-equal; positions, status
and err equal as raw bits to the oracle run in the kernel's summation order (sum_mode 1).  A NaN position is compared as "NaN on both
sides": IEEE 754 does not fix the payload an operation returns.  Where the points are random, the raster order (sum_mode 0) of
OpenCV's generic loop is held to the same tolerances as there.  One check needs no oracle: a frame shifted by a known sub-pixel
offset, built at float64, whose offset the tracker must recover."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NAN, INF = np.float32(np.nan), np.float32(np.inf)


def _bits(a):
    a = np.ascontiguousarray(a, np.float32)
    u = a.view(np.uint32).copy()
    u[np.isnan(a)] = 0x7FC00000
    return u


def _levels_equal(k, slot, p, what=""):
    for lvl in range(p.levels):
        gi, gd = k.read_level(slot, lvl)
        oi, od = p.level(lvl)
        np.testing.assert_array_equal(gi, oi, err_msg="%s image level %d" % (what, lvl))
        np.testing.assert_array_equal(gd, od, err_msg="%s derivative level %d" % (what, lvl))


def _track_equal(k, oracle, slots, pyrs, pts, init, win, ml, what="", max_level=None, max_count=30, epsilon=0.01, min_eig=1e-4):
    """GPU track against oracle.klt_track_ex(sum_mode=1), bit for bit; returns the GPU result.  max_level: the argument of the call
    (None = the handle's ml)."""
    g = k.track(slots[0], slots[1], pts, init, max_count=max_count, epsilon=epsilon, min_eig_threshold=min_eig, max_level=max_level)
    o = oracle.klt_track_ex(pyrs[0], pyrs[1], pts, init, win, ml if max_level is None else max_level, max_count, epsilon, min_eig, sum_mode=1)
    np.testing.assert_array_equal(g[1], o[1], err_msg="%s: status" % what)
    np.testing.assert_array_equal(_bits(g[0]), _bits(o[0]), err_msg="%s: positions" % what)
    np.testing.assert_array_equal(_bits(g[2]), _bits(o[2]), err_msg="%s: err" % what)
    return g


def _raster_close(g, oracle, pyrs, pts, init, win, ml):
    """The tolerances of test_gpu_parity.py::test_klt_pyramid_and_tracking against the raster summation order.  The 0.01 px bound
    holds for points whose iterations converged: a point that is still moving after all 30 iterations (its position changes when a
    31st is allowed) ends wherever the last step left it, and rounding differences in the sums move that end freely."""
    g_next, g_st, _ = g
    r_next, r_st, _, r_mg = oracle.klt_track_ex(pyrs[0], pyrs[1], pts, init, win, ml, sum_mode=0)
    assert ((g_st == r_st) | (r_mg < 1e-3)).all()
    moving = (oracle.klt_track_ex(pyrs[0], pyrs[1], pts, init, win, ml, 31, sum_mode=0)[0] != r_next).any(axis=1)
    both = (g_st > 0) & (r_st > 0)
    d = np.abs(g_next - r_next).max(axis=1)
    assert np.median(d[both]) < 1e-3 and (d[both & (r_mg > 0.1) & ~moving] < 0.01).all()
    assert (both & ~moving).sum() > 0.4 * both.sum()            # a 3 x 3 window leaves about half its points still moving


def _random_points(rng, w, h, n):
    pts = np.stack([rng.uniform(-5, w + 5, n), rng.uniform(-5, h + 5, n)], 1).astype(np.float32)   # some outside / at the border
    init = (pts + rng.normal(0, 1.0, (n, 2))).astype(np.float32)                                   # OPTFLOW_USE_INITIAL_FLOW
    return pts, init


def _setup(uvo, oracle, synth, w, h, win, ml, seed, slots=2, max_points=4096):
    a = synth.make_frame(seed, w, h)
    b = synth.warp_frame(a, seed + 1)
    k = uvo.KLT(w, h, win, ml, max_points=max_points, slots=slots)
    na, nb = k.build_pyramid(0, a), k.build_pyramid(1, b)
    pa, pb = oracle.klt_pyramid(a, win, ml), oracle.klt_pyramid(b, win, ml)
    assert na == nb == pa.levels == pb.levels
    _levels_equal(k, 0, pa, "frame a")
    _levels_equal(k, 1, pb, "frame b")
    return k, (pa, pb)


# Data/euroc.yaml + EuroC/V2_2.yaml (9 / 3), the Aqualoc setting (21 / 5), EuroC/V1_3.yaml + V2_3.yaml (25 / 7); Tracking.cc:75-77.
# At 752 x 480 the pyramid stops when a level gets too small for the window: 25 / 7 builds 5 levels, 21 / 5 too.
@pytest.mark.parametrize("win,ml,levels", [((9, 9), 3, 4), ((21, 21), 5, 5), ((25, 25), 7, 5)])
def test_reference_settings(uvo, oracle, synth, win, ml, levels):
    w, h = 752, 480
    rng = np.random.default_rng(90 + win[0])
    k, pyrs = _setup(uvo, oracle, synth, w, h, win, ml, 7100 + win[0])
    assert pyrs[0].levels == levels
    pts, init = _random_points(rng, w, h, 2000)
    g = _track_equal(k, oracle, (0, 1), pyrs, pts, init, win, ml, "win %s" % (win,))
    assert (g[1] > 0).sum() > 0.6 * len(pts)
    _raster_close(g, oracle, pyrs, pts, init, win, ml)
    # the pyramids in swapped roles, default initial flow
    _track_equal(k, oracle, (1, 0), pyrs[::-1], pts, None, win, ml, "swapped roles")
    k.close()


# both sides of the k_klt_track<7> / <16> dispatch (448 / 450 pixels), the 1024-pixel limit, the smallest window, non-square windows
# both ways round (win_w != win_h separates halfx / halfy, bx / by, the wx / wy split and the minEig divisor); an odd image size
@pytest.mark.parametrize("win", [(3, 3), (16, 28), (15, 30), (32, 32), (9, 25), (31, 15)])
def test_window_dispatch_and_shapes(uvo, oracle, synth, win):
    w, h, ml = 427, 251, 4
    rng = np.random.default_rng(win[0] * 100 + win[1])
    k, pyrs = _setup(uvo, oracle, synth, w, h, win, ml, 7300 + win[0] + win[1])
    pts, init = _random_points(rng, w, h, 1000)
    g = _track_equal(k, oracle, (0, 1), pyrs, pts, init, win, ml, "win %s" % (win,))
    assert (g[1] > 0).sum() > 0.5 * len(pts)
    _raster_close(g, oracle, pyrs, pts, init, win, ml)
    _track_equal(k, oracle, (1, 0), pyrs[::-1], pts, None, win, ml, "win %s, swapped roles" % (win,))
    k.close()


def test_max_level_argument(uvo, oracle, synth):
    """The call's max_level: 0 (level 0 only), below the pyramid's depth, above it (clamped to the levels built); the same argument
    reaches uvo_klt_track_undistorted."""
    w, h, win, ml = 752, 480, (21, 21), 5
    rng = np.random.default_rng(93)
    k, pyrs = _setup(uvo, oracle, synth, w, h, win, ml, 7500)
    pts, init = _random_points(rng, w, h, 1500)
    init = (pts + rng.normal(0, 4.0, pts.shape)).astype(np.float32)       # far enough that the depth changes the outcome
    res = {}
    for arg in (0, 2, 7):
        res[arg] = _track_equal(k, oracle, (0, 1), pyrs, pts, init, win, ml, "max_level %d" % arg, max_level=arg)
    full = k.track(0, 1, pts, init)
    np.testing.assert_array_equal(_bits(res[7][0]), _bits(full[0]))      # 7 clamps to the 5 levels built, as does the handle's 5
    assert (res[0][1] != full[1]).any() and (res[2][1] != full[1]).any()
    cam = uvo.CameraModel.make(458.654, 457.296, 367.215, 248.375, [-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05])
    un = k.track_undistorted(0, 1, pts, cam, init, max_level=2)
    np.testing.assert_array_equal(_bits(un[0]), _bits(res[2][0]))
    np.testing.assert_array_equal(un[1], res[2][1])
    k.close()


def test_image_with_level_zero_only(uvo, oracle, synth):
    """48 x 40 with a 25 x 25 window: the next level (24 x 20) would not exceed the window, so only level 0 is built."""
    w, h, win, ml = 48, 40, (25, 25), 7
    rng = np.random.default_rng(94)
    k, pyrs = _setup(uvo, oracle, synth, w, h, win, ml, 7600)
    assert pyrs[0].levels == 1
    pts, init = _random_points(rng, w, h, 300)
    g = _track_equal(k, oracle, (0, 1), pyrs, pts, init, win, ml)
    assert (g[1] > 0).sum() > 0.5 * len(pts)
    _track_equal(k, oracle, (0, 1), pyrs, _edge_points(w, h, win, 0), None, win, ml, "edge previous points")
    k.close()


def test_termination_criteria(uvo, oracle, synth):
    """max_count 0 / 1 / 150 (clamped to 100), epsilon 0 / 20 (clamped to 10), min_eig_threshold 0 and one that every point fails;
    on both kernel instances."""
    w, h = 640, 480
    for win, ml in (((15, 15), 3), ((25, 25), 7)):
        rng = np.random.default_rng(95 + win[0])
        k, pyrs = _setup(uvo, oracle, synth, w, h, win, ml, 7700 + win[0])
        pts, init = _random_points(rng, w, h, 600)
        run = lambda what, **kw: _track_equal(k, oracle, (0, 1), pyrs, pts, init, win, ml, "win %s %s" % (win, what), **kw)
        default = run("default")
        none = run("max_count 0", max_count=0)
        assert (none[1] > 0).sum() >= (default[1] > 0).sum()                # without iterations nothing leaves the image
        one = run("max_count 1", max_count=1)
        assert (_bits(one[0]) != _bits(default[0])).any()
        many = run("max_count 150", max_count=150)
        hundred = k.track(0, 1, pts, init, max_count=100)
        np.testing.assert_array_equal(_bits(many[0]), _bits(hundred[0]))
        exact = run("epsilon 0", epsilon=0.0)
        assert (_bits(exact[0]) != _bits(default[0])).any()
        coarse = run("epsilon 20", epsilon=20.0)
        ten = k.track(0, 1, pts, init, epsilon=10.0)
        np.testing.assert_array_equal(_bits(coarse[0]), _bits(ten[0]))
        run("min_eig 0", min_eig=0.0)
        fail = run("min_eig 1e6", min_eig=1e6)
        assert (fail[1] == 0).all() and (fail[2] > 0).any()
        k.close()


def _edge_points(w, h, win, top):
    """Points whose floor(x - halfx) (or y) lands exactly on -win, -win - 1, L.w - 1 and L.w of level `top` and of level 0,
    at a few fractions; the other coordinate in the middle of the image."""
    halfx, halfy = (win[0] - 1) * 0.5, (win[1] - 1) * 0.5
    out = []
    for lvl in sorted({0, top}):
        lw, lh = w, h
        for _ in range(lvl):
            lw, lh = (lw + 1) // 2, (lh + 1) // 2
        s = float(1 << lvl)
        for f in (0.0, 0.5, 0.96875):
            for c in (-win[0], -win[0] - 1, lw - 1, lw):
                out.append(((c + f + halfx) * s, h * 0.5))
            for c in (-win[1], -win[1] - 1, lh - 1, lh):
                out.append((w * 0.5, (c + f + halfy) * s))
            out.append(((-win[0] + f + halfx) * s, (lh - 1 + f + halfy) * s))
            out.append(((lw - 1 + f + halfx) * s, (-win[1] + f + halfy) * s))
    return np.array(out, np.float32)


@pytest.mark.parametrize("win,ml", [((21, 21), 5), ((25, 25), 7), ((9, 25), 3)])
def test_points_counts_edges_and_non_finite(uvo, oracle, synth, win, ml):
    w, h = 501, 333
    rng = np.random.default_rng(96 + win[1])
    k, pyrs = _setup(uvo, oracle, synth, w, h, win, ml, 7900 + win[0], max_points=2048)
    top = pyrs[0].levels - 1
    # point counts that are not a multiple of the four waves of a block, and the handle's maximum
    pts, init = _random_points(rng, w, h, 2048)
    for n in (1, 5, 2048):
        _track_equal(k, oracle, (0, 1), pyrs, pts[:n], init[:n], win, ml, "%d points" % n)
    # the image-bounds tests at their edges.  A previous point there has a window without x (or y) derivatives -- the derivative
    # planes are zero outside the image, the Scharr x-derivative is zero on the first and last column -- so it fails the eigenvalue
    # test whichever way the bounds test went: these runs are compared bit for bit only
    edge = _edge_points(w, h, win, top)
    _track_equal(k, oracle, (0, 1), pyrs, edge, None, win, ml, "edge previous points")
    _track_equal(k, oracle, (0, 1), pyrs, edge, edge + np.float32([0.25, -0.25]), win, ml, "edge both")
    inner = np.tile(np.float32([[w * 0.5, h * 0.5]]), (len(edge), 1))
    _track_equal(k, oracle, (0, 1), pyrs, inner, edge, win, ml, "edge initial flow")
    # the first iteration's bounds test, template in the middle of level 0, one iteration (none re-tests after the step): floor on
    # -win and L.w - 1 passes, on -win - 1 and L.w fails
    lvl0 = _edge_points(w, h, win, 0)
    g = _track_equal(k, oracle, (0, 1), pyrs, inner[:len(lvl0)], lvl0, win, ml, "edge initial flow, level 0", max_level=0, max_count=1)
    np.testing.assert_array_equal(g[1], np.tile([1, 0, 1, 0, 1, 0, 1, 0, 1, 1], 3))
    assert (g[2] > 1e-4).all()
    # initial flows that leave the image, near and far
    mid = pts[(pts[:, 0] > 30) & (pts[:, 0] < w - 30) & (pts[:, 1] > 30) & (pts[:, 1] < h - 30)][:64]
    away = np.concatenate([mid + np.float32([w, 0]), mid - np.float32([0, h]), mid + np.float32([40, 40]), mid * np.float32(-1),
                           mid + np.float32([1e6, 0]), mid + np.float32([0, -1e9])])
    g = _track_equal(k, oracle, (0, 1), pyrs, np.tile(mid, (6, 1)), away, win, ml, "initial flow outside")
    assert (g[1][len(mid) * 4:] == 0).all() and (g[2][len(mid) * 4:] > 0).all()    # outside at every level: rejected on level 0
    # NaN, +-inf and out-of-range values in the previous points and in the initial flow: rejected, like cvFloor's INT_MIN on x86
    bad = np.float32([NAN, INF, -INF, 3e38, -3e38, 2.0 ** 31, -(2.0 ** 31)])
    c = np.float32([w * 0.5, h * 0.5])
    prev = [[v, c[1]] for v in bad] + [[c[0], v] for v in bad] + [[NAN, NAN]]
    prev = np.array(prev, np.float32)
    g = _track_equal(k, oracle, (0, 1), pyrs, prev, np.tile(c, (len(prev), 1)), win, ml, "non-finite previous points")
    assert (g[1] == 0).all() and (g[2] == 0).all()
    g = _track_equal(k, oracle, (0, 1), pyrs, np.tile(c, (len(prev), 1)), prev, win, ml, "non-finite initial flow")
    assert (g[1] == 0).all() and (g[2] > 0).all()
    for arg in (0, 1):
        _track_equal(k, oracle, (0, 1), pyrs, np.tile(c, (len(prev), 1)), prev, win, ml, "non-finite flow, max_level %d" % arg, max_level=arg)
    k.close()


def test_pyramid_below_the_handle_size_and_reused_slots(uvo, oracle, synth):
    """Slots built at a size below the handle's maximum (level offsets of the smaller geometry inside the larger slot), tracked in
    both roles; then slots of the full size beside them."""
    W, H, win, ml = 752, 480, (25, 25), 7
    rng = np.random.default_rng(97)
    k = uvo.KLT(W, H, win, ml, max_points=2048, slots=3)
    small = [synth.make_frame(8100, 501, 301)]
    small.append(synth.warp_frame(small[0], 8101))
    assert k.build_pyramid(2, small[0]) == k.build_pyramid(0, small[1])
    ps = [oracle.klt_pyramid(im, win, ml) for im in small]
    _levels_equal(k, 2, ps[0], "small a")
    _levels_equal(k, 0, ps[1], "small b")
    pts, init = _random_points(rng, 501, 301, 1500)
    _track_equal(k, oracle, (2, 0), ps, pts, init, win, ml, "small 2 -> 0")
    _track_equal(k, oracle, (0, 2), ps[::-1], pts, init, win, ml, "small 0 -> 2")
    big = [synth.make_frame(8200, W, H)]
    big.append(synth.warp_frame(big[0], 8201))
    k.build_pyramid(1, big[0])
    with pytest.raises(uvo.UvoError):                         # the two pyramids have different sizes
        k.track(2, 1, pts)
    k.build_pyramid(0, big[1])
    pb = [oracle.klt_pyramid(im, win, ml) for im in big]
    _levels_equal(k, 1, pb[0], "big a")
    _levels_equal(k, 0, pb[1], "big b")
    pts, init = _random_points(rng, W, H, 1500)
    _track_equal(k, oracle, (1, 0), pb, pts, init, win, ml, "big 1 -> 0")
    _track_equal(k, oracle, (0, 1), pb[::-1], pts, None, win, ml, "big 0 -> 1")
    k.close()


def test_euroc_front_end_chain(uvo, oracle, synth):
    """The EuRoC V1_3 / V2_3 front end: CLAHE (4.0, 12 x 12) on the device, the 25 / 7 pyramid built from the extractor's HBM result,
    the tracker -- against oracle.clahe, the oracle pyramid and the oracle tracker."""
    W, H, win, ml = 752, 480, (25, 25), 7
    rng = np.random.default_rng(98)
    raw = [(synth.make_frame(8300, W, H).astype(np.float32) * 0.45 + 25).astype(np.uint8)]
    raw.append((synth.warp_frame(synth.make_frame(8300, W, H), 8301).astype(np.float32) * 0.45 + 25).astype(np.uint8))
    ex = uvo.ORBextractor(1000, 1.2, 8, 0, 20, max_width=W, max_height=H)
    k = uvo.KLT(W, H, win, ml, max_points=2048, slots=2)
    pyrs = []
    for slot, im in enumerate(raw):
        enh = oracle.clahe(im, 4.0, (12, 12))
        np.testing.assert_array_equal(ex.clahe(im, 4.0, (12, 12)), enh)
        assert k.build_pyramid_from(slot, ex) == 5
        pyrs.append(oracle.klt_pyramid(enh, win, ml))
        _levels_equal(k, slot, pyrs[-1], "slot %d" % slot)
    pts, init = _random_points(rng, W, H, 2000)
    g = _track_equal(k, oracle, (0, 1), pyrs, pts, init, win, ml, "clahe chain")
    assert (g[1] > 0).sum() > 0.6 * len(pts)
    _raster_close(g, oracle, pyrs, pts, init, win, ml)
    ex.close()
    k.close()


def _sine_texture(w, h, shift, seed=5, n=48):
    """Sum of plane waves with wavelengths 10..400 px, evaluated at float64 at (x - shift[0], y - shift[1]), rounded to 8 bits:
    content at every pyramid level and nothing near the Nyquist limit of level 0."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    x, y = x - shift[0], y - shift[1]
    f = np.zeros((h, w))
    for _ in range(n):
        lam, th, ph = np.exp(rng.uniform(np.log(10), np.log(400))), rng.uniform(0, np.pi), rng.uniform(0, 2 * np.pi)
        f += np.sin(2 * np.pi / lam * (np.cos(th) * x + np.sin(th) * y) + ph)
    return f


def test_known_subpixel_shift_is_recovered(uvo):
    """No oracle: a frame and its copy shifted by a known offset.  Measured with the CPU statement in both summation orders on these
    images: the mean displacement is within 0.007 px of the offset at every window; windows 21 and 25 put every point within 0.035
    px; a 9 x 9 window of 8-bit pixels leaves 95 % of the points within 0.05 px and single ones up to 0.18 px."""
    w, h = 752, 480
    ys, xs = np.mgrid[40:h - 40:17, 40:w - 40:17]
    pts = np.stack([xs.ravel(), ys.ravel()], 1).astype(np.float32) + np.float32(0.3)
    base = _sine_texture(w, h, (0.0, 0.0))
    scale = 100.0 / np.abs(base).max()
    quant = lambda f: np.clip(np.rint(128 + f * scale), 0, 255).astype(np.uint8)
    a = quant(base)
    for d in ((1.3125, -0.6875), (-5.55, 3.3)):
        b = quant(_sine_texture(w, h, d))
        for win, ml in (((9, 9), 3), ((21, 21), 5), ((25, 25), 7)):
            k = uvo.KLT(w, h, win, ml, max_points=len(pts), slots=2)
            k.build_pyramid(0, a), k.build_pyramid(1, b)
            nxt, st, _ = k.track(0, 1, pts)
            k.close()
            assert (st > 0).all(), (d, win)
            dev = (nxt - pts).astype(np.float64) - np.array(d)
            err = np.abs(dev).max(axis=1)
            assert np.abs(dev.mean(axis=0)).max() < 0.01, (d, win, dev.mean(axis=0))
            if win[0] == 9:
                assert np.percentile(err, 90) < 0.05 and err.max() < 0.25, (d, win, np.percentile(err, 90), err.max())
            else:
                assert err.max() < 0.05, (d, win, err.max())
