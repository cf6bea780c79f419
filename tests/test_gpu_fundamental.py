"""uvo_klt_find_fundamental / uvo_klt_track_filtered (csrc/fundamental.hip) against tests/fundamental_model.py, the restatement of
cv::findFundamentalMat(FM_RANSAC) at src/Tracking.cc:1062, under the tolerance contract of DESIGN.md section 4: the mask bytes, the
info (method, iterations, inliers, RNG draws) and -- through the hypothesis tap -- every subset and every hypothesis's multiset of
model scores are compared exactly, F within 1e-6 (relative, Frobenius, after normalising sign and scale).  The committed seeds keep
the model's sensitivity flags clear (no error within 1e-6 of its threshold, no tie at a new maximum), which the test asserts, so
the exact comparison holds without exceptions."""
import ctypes

import numpy as np
import pytest

import fundamental_model as fm

pytestmark = pytest.mark.gpu

MAXP = 2048
GRID_N = (7, 8, 10, 14, 15, 16, 64, 400, 1000, MAXP)
RATIOS = (0.95, 0.7, 0.5, 0.35)
NOISES = (0.1, 0.5)
# (n, inlier ratio, noise) -> the first seed from 1000 * n_index + 100 * ratio_index + 10 * noise_index whose model run raises no
# sensitivity flag (noise 0.1 in a 640 x 512 camera, 0.5 in a 752 x 480 one)
SEEDS = {(15, 0.95, 0.5): 4011, (15, 0.7, 0.5): 4114, (15, 0.5, 0.5): 4211, (15, 0.35, 0.1): 4302, (15, 0.35, 0.5): 4311, (16, 0.7, 0.5): 5111,
         (16, 0.5, 0.5): 5211, (16, 0.35, 0.5): 5311, (64, 0.5, 0.5): 6212, (64, 0.35, 0.5): 6312, (1000, 0.7, 0.1): 8101}


def parity_points(n, ratio, noise, seed):
    size = (640, 512) if noise < 0.3 else (752, 480)
    p0, p1, _, _ = fm.scene(seed, n, ratio, noise, size)
    return p0, p1


def _rel(a, b):
    return float(np.linalg.norm(fm.normalized_F(a) - fm.normalized_F(b)))


def check(k, p0, p1, thr=1.0, conf=0.999, what="", decisions=True):
    """One GPU call against the model, everything the contract fixes; returns the model's result.  decisions=False (and LMedS
    below 14 points, where the winner is rounding noise): the draws, subsets and model counts exactly, and the mask must be the
    inliers of the F the GPU returned."""
    p0 = np.ascontiguousarray(p0, np.float32).reshape(-1, 2)
    p1 = np.ascontiguousarray(p1, np.float32).reshape(-1, 2)
    ref = fm.find_fundamental(p0, p1, thr, conf)
    residual = ("median_is_fit_residual", -1) in ref.flags     # LMedS below 14 points: the winner is rounding noise
    assert not [f for f in ref.flags if f[0] != "median_is_fit_residual"], (what, ref.flags[:4])
    mask, F, info = k.find_fundamental(p0, p1, thr, conf)
    sub, nm, sc = k.fm_hypotheses()
    assert len(sub) == ref.iterations == len(ref.hypotheses), what
    if residual or not decisions:   # the draws, the subsets, the models' count; the mask = the GPU winner's inliers
        assert info.method == ref.method and (info.iterations, info.rng_draws) == (ref.iterations, ref.rng_draws) or not decisions, what
        for h, (idx, models, _) in enumerate(ref.hypotheses[:info.iterations]):
            assert list(sub[h]) == idx and max(int(nm[h]), 0) == len(models), (what, h)
        F = F.reshape(9)
        t = np.float32(0.001 * 0.001) if residual else np.float32(thr * thr)
        win = fm.errors(p0, p1, F) <= t if F.any() else np.zeros(len(p0), bool)
        assert info.inliers == int(mask.sum()) and (not F.any() or (mask.astype(bool) == win).all()), what
        assert info.inliers >= 7 or not F.any(), what
        return ref
    assert info.astuple() == ref.info, (what, info.astuple(), ref.info)
    np.testing.assert_array_equal(mask, ref.mask, err_msg=what)
    for h, (idx, models, scores) in enumerate(ref.hypotheses):
        assert list(sub[h]) == idx, (what, h)
        assert max(int(nm[h]), 0) == len(models), (what, h)
        got = sorted(sc[h][:len(models)])
        if ref.method == fm.METHOD_RANSAC:
            assert got == sorted(scores), (what, h, got, scores)
        else:
            np.testing.assert_allclose(got, sorted(scores), rtol=fm.LMEDS_RTOL, err_msg="%s hypothesis %d" % (what, h))
    F = F.reshape(9)
    if ref.method == fm.METHOD_7POINT:
        models = fm.run_7point(p0, p1, list(range(7)))      # root order depends on the basis: F is one of them
        assert (not models and not F.any()) or min(_rel(F, M) for M in models) < 1e-6, what
    elif ref.F.any():
        assert _rel(F, ref.F) < 1e-6, (what, _rel(F, ref.F))
    else:
        assert not F.any(), what
    return ref


@pytest.fixture(scope="module")
def klt(uvo):
    k = uvo.KLT(752, 512, (21, 21), 5, max_points=MAXP, slots=2)
    yield k
    k.close()


@pytest.mark.parametrize("n", GRID_N)
def test_parity_grid(klt, n):
    methods = set()
    for ri, ratio in enumerate(RATIOS):
        for ni, noise in enumerate(NOISES):
            seed = SEEDS.get((n, ratio, noise), 1000 * GRID_N.index(n) + 100 * ri + 10 * ni)
            p0, p1 = parity_points(n, ratio, noise, seed)
            ref = check(klt, p0, p1, what="n %d ratio %.2f noise %.1f seed %d" % (n, ratio, noise, seed))
            methods.add(ref.method)
            if n >= 400 and ratio == 0.35:
                assert ref.iterations == 1000                   # the cap
            if n >= 400 and ratio == 0.95 and noise < 0.3:
                assert ref.iterations < 20
    assert methods == {fm.METHOD_7POINT if n == 7 else fm.METHOD_LMEDS if n < 15 else fm.METHOD_RANSAC}


def test_edge_cases(uvo, klt):
    p0, p1 = parity_points(64, 0.7, 0.1, 65)
    for n in range(7):                                          # no model: the mask all 0, nothing drawn
        mask, F, info = klt.find_fundamental(p0[:n], p1[:n])
        assert info.astuple() == (fm.METHOD_NONE, 0, 0, 0) and not mask.any() and not F.any() and mask.shape == (n,)
        assert len(klt.fm_hypotheses()[0]) == 0
    same = np.tile(np.float32([[100.5, 200.25]]), (40, 1))      # identical points: every subset collinear, no model
    ref = check(klt, same, same + np.float32([3, -1]), what="identical points")
    assert ref.info[:3] == (fm.METHOD_RANSAC, 0, 0) and ref.rng_draws > 70000
    ref = check(klt, same[:12], same[:12], what="identical points, LMedS")
    assert ref.info[:3] == (fm.METHOD_LMEDS, 0, 0)
    x = np.arange(50, dtype=np.float32) * 7 + 5                 # all on one line (exactly, in float32)
    line = np.stack([x, 2 * x + 3], 1)
    ref = check(klt, line, line + np.float32([4, 1]), what="one line")
    assert ref.iterations == 0 and not ref.mask.any()
    q0 = p0.copy()
    q0[17, 0] = np.nan                                          # one NaN point: its error is NaN, never an inlier
    ref = check(klt, q0, p1, what="one NaN point")
    assert ref.mask[17] == 0 and ref.inliers > 30
    # near 1e6 the raw 7 x 9 system spans 24 orders of magnitude: F carries more than the contract's 1e-6 and counts move with it
    far = check(klt, p0 + np.float32(1e6), p1 + np.float32(1e6), what="coordinates near 1e6", decisions=False)
    assert far.method == fm.METHOD_RANSAC
    for thr in (0.0, -1.0):                                     # thr <= 0 -> 3
        ref = check(klt, p0, p1, thr=thr, what="thr %g" % thr)
        assert ref.info == fm.find_fundamental(p0, p1, 3.0).info
    for conf in (0.0, 1.0, 1.5):                                # conf out of range -> 0.99
        check(klt, p0, p1, conf=conf, what="conf %g" % conf)
    big = np.zeros((MAXP + 1, 2), np.float32)
    with pytest.raises(uvo.UvoError) as ei:
        klt.find_fundamental(big, big)
    assert ei.value.code == uvo.UVO_E_BADARG
    for thr, conf in ((np.nan, 0.999), (1.0, np.nan)):
        with pytest.raises(uvo.UvoError) as ei:
            klt.find_fundamental(p0, p1, thr, conf)
        assert ei.value.code == uvo.UVO_E_BADARG
    lib, m = uvo.lib, np.zeros(64, np.uint8)
    a, b = p0.ctypes.data, p1.ctypes.data
    assert lib.uvo_klt_find_fundamental(klt._h, None, b, 64, 1.0, 0.999, m.ctypes.data, None, None) == uvo.UVO_E_BADARG
    assert lib.uvo_klt_find_fundamental(klt._h, a, None, 64, 1.0, 0.999, m.ctypes.data, None, None) == uvo.UVO_E_BADARG
    assert lib.uvo_klt_find_fundamental(klt._h, a, b, 64, 1.0, 0.999, None, None, None) == uvo.UVO_E_BADARG
    assert lib.uvo_klt_find_fundamental(klt._h, a, b, -1, 1.0, 0.999, m.ctypes.data, None, None) == uvo.UVO_E_BADARG
    n = ctypes.c_int()
    assert lib.uvo_klt_fm_hypotheses(klt._h, None, None, None, 4, ctypes.byref(n)) == uvo.UVO_E_BADARG
    assert lib.uvo_klt_fm_hypotheses(klt._h, None, None, None, 4, None) == uvo.UVO_E_BADARG


def _bilinear(img, sx, sy):
    h, w = img.shape
    sx, sy = np.clip(sx, 0, w - 1.001), np.clip(sy, 0, h - 1.001)
    x0, y0 = np.floor(sx).astype(np.int64), np.floor(sy).astype(np.int64)
    fx, fy = sx - x0, sy - y0
    f = img.astype(np.float64)
    v = (f[y0, x0] * (1 - fx) * (1 - fy) + f[y0, x0 + 1] * fx * (1 - fy) + f[y0 + 1, x0] * (1 - fx) * fy + f[y0 + 1, x0 + 1] * fx * fy)
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def _frame_pair(synth, w, h, seed):
    """A textured frame and the next one of a camera translating along (1, 0.3) over a scene of smoothly varying depth (the flow
    is disparity x (1, 0.3): the epipolar lines are parallel to it), with one independently moving rectangle -- the injected outlier
    flows (-4, +5)."""
    a = synth.make_frame(seed, w, h)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    d = 2.0 + 1.5 * np.sin(xx / 37.0) * np.cos(yy / 53.0)
    sx, sy = xx - d, yy - 0.3 * d
    obj = (yy >= 180) & (yy < 300) & (xx >= 260) & (xx < 420)
    sx[obj], sy[obj] = xx[obj] + 4.0, yy[obj] - 5.0
    return a, _bilinear(a, sx, sy), obj


def _track_points(w, h, n, rng):
    pts = np.stack([rng.uniform(30, w - 30, n), rng.uniform(30, h - 30, n)], 1).astype(np.float32)
    return pts, (pts + rng.normal(0, 0.7, pts.shape)).astype(np.float32)


def test_fused_call(uvo, oracle, synth):
    w, h = 640, 512
    a, b, obj = _frame_pair(synth, w, h, 9100)
    k = uvo.KLT(w, h, (21, 21), 5, max_points=MAXP, slots=2)
    k.build_pyramid(0, a), k.build_pyramid(1, b)
    cam = uvo.CameraModel.make(460.0, 458.0, 322.0, 250.0, [-0.02, 0.005, 0.0002, -0.0001])
    rng = np.random.default_rng(91)
    seen_lmeds = seen_outliers = False
    for n, want_F in ((600, True), (50, False), (14, True), (9, True), (MAXP, True), (300, False)):
        pts, init = _track_points(w, h, n, rng)
        plain = k.track(0, 1, pts, init)                        # interleaved plain tracker calls on the same handle
        u = k.track_undistorted(0, 1, pts, cam, init)
        f = k.track_filtered(0, 1, pts, cam, init, want_F=want_F)
        if n < 10:                                              # perform_matching :1037-1041: no tracking, mask all 0
            assert not f[5].any() and f[6] is not None and not f[6].any()
            np.testing.assert_array_equal(f[0], init)
            assert not f[1].any() and not f[2].any() and not f[3].any() and not f[4].any()
            continue
        np.testing.assert_array_equal(plain[0].view(np.uint32), u[0].view(np.uint32))
        for i in range(5):                                      # tracker + undistortion byte-equal to the unfused call
            np.testing.assert_array_equal(np.asarray(f[i]).view(np.uint8), np.asarray(u[i]).view(np.uint8), err_msg="n %d output %d" % (n, i))
        ref = fm.find_fundamental(u[3], u[4], 1.0, 0.999)       # on all n undistorted pairs, lost points included
        assert not ref.flags, (n, ref.flags[:4])
        np.testing.assert_array_equal(f[5], u[1] & ref.mask, err_msg="n %d mask_out" % n)
        if want_F:
            assert _rel(f[6], ref.F) < 1e-6 if ref.F.any() else not f[6].any()
        else:
            assert f[6] is None
        sub, nm, sc = k.fm_hypotheses()
        assert len(sub) == ref.iterations and all(list(sub[i]) == ref.hypotheses[i][0] for i in range(len(sub)))
        seen_lmeds |= ref.method == fm.METHOD_LMEDS
        inside = obj[np.clip(pts[:, 1].astype(int), 0, h - 1), np.clip(pts[:, 0].astype(int), 0, w - 1)]
        if ref.method == fm.METHOD_RANSAC and n >= 300:         # the moving rectangle's points are the outliers
            tracked = u[1] > 0
            assert ref.mask[tracked & inside].mean() < 0.1 and ref.mask[tracked & ~inside].mean() > 0.8, n
            seen_outliers = True
    assert seen_lmeds and seen_outliers
    k.close()
