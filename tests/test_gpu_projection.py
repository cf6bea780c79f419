"""k_project (five modes) and k_project_sim3 (csrc/match_engine.hip) against the numpy model of tests/projection_model.py, on scenes that
sit on the decision boundaries: the exact scene (a point ON every boundary and the nearest inputs either side of it whose fp32 result
differs), the depth boundary (Z = +0, -0, +-2^-149), the degenerate scene (non-finite intermediates from finite inputs, NaN and
infinite coordinates), the generic scenes and the launch shapes.  tests/test_projection_model.py holds the model to the oracle, to a
hand-derived table and to a real-valued evaluator on the CPU.  The entry points are called directly; every comparison is exact (NaN
compares as NaN: the device produces the positive quiet NaN, x86 the negative one).  Outputs have PAD more rows than the call may write,
prefilled with values no result can equal; the pad must keep them.

Which test covers which boundary of which mode (F = FRUSTUM, K = KF_RELOC, U = FUSE, B = PIXEL_BOUNDED, P = PIXEL, S = sim3, both
directions):
  depth `Z < 0`, zeros pass (F, U, S; absent in K, B, P)        test_depth_boundary_and_degenerate_scene, test_exact_scene (row `behind`)
  image bounds, closed (F, K, B) / half-open (U, S) / none (P)  test_exact_scene (rows u_max, u_min, v_max, v_min and their neighbours)
  NaN centre passes closed bounds, fails IsInImage              test_depth_boundary_and_degenerate_scene
  distance, closed [min_inv, max_inv] (F, U, S; absent in K)    test_exact_scene (rows dist_min, dist_max and neighbours)
  sim3 distance is the camera point's norm                      test_exact_scene[sim3_*], test_generic_scene[sim3_*]
  cosine `(float)(dot / dist) < limit` (F)                      test_exact_scene[frustum] (row cos_frustum and neighbours)
  cosine `dot < 0.5 dist` in double (U)                         test_exact_scene[fuse] (row cos_fuse and neighbours)
  lower bound over the table, clamp (K, U, S)                   test_exact_scene (rows ratio_*, ratio_below, ratio_above; repeated and one-entry tables)
  PredictScale: ceil, clamps at 0 and nlevels - 1 (F)           test_exact_scene[frustum] (rows ps_-1 .. ps_9, scale factor 2 and float32(1.2))
  PredictScale: +inf / NaN quotient -> INT_MIN -> level 0 (F)   test_depth_boundary_and_degenerate_scene[frustum]
  camera centre derived, cam->ow not read (K)                   test_exact_scene[kf_reloc] (again with cam->ow NaN), test_generic_scene[kf_reloc] (cam->ow NaN)
  invalid rows write zeros; usable = 0                          every test, with and without a mask; view_cos NULL in test_exact_scene
  grid tail, n = 0, 1, 255, 256, 257, 65537                     test_launch_shapes
  argument checks of uvo_project_points                         test_argument_checks
  k_project inside uvo_search_points_in_frustum                 test_search_points_in_frustum_outputs
  k_project inside uvo_fuse_batch (two targets, two poses)      test_fuse_batch_projects_as_the_model
"""
import ctypes

import numpy as np
import pytest

import projection_model as pm
import window_model as wm
from projection_model import f32, FRUSTUM, KF_RELOC, FUSE, PIXEL_BOUNDED, PIXEL, SIM3

pytestmark = pytest.mark.gpu

PAD = 7
V_FILL, F_FILL, L_FILL = 0xA5, f32(-7.25e11), -12345
mode_param = pytest.mark.parametrize("mode", pm.ALL_MODES, ids=pm.MODE_IDS)


def _p(a):
    return None if a is None else a.ctypes.data


def bits(a):
    a = np.asarray(a)
    return np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32)) if a.dtype == np.float32 else a


@pytest.fixture(scope="module")
def matcher(uvo):
    m = uvo.ORBmatcher(0.8, False, max_query=8192, max_map_points=8192)
    yield m
    m.close()


def _cam(uvo, cam):
    return uvo.CameraPose.from_buffer_copy(cam.array().tobytes())


def _run(uvo, m, mode, s, sf, sfac, usable=None, cos_limit=0.5, with_cos=True, all_arrays=False):
    """The entry point of this mode on a scene -> valid, u, v, level, view_cos (zeros for sim3 and where view_cos is NULL).  Arrays the
    mode does not read are passed as NULL unless all_arrays."""
    n, mm = len(s["xyz"]), min(mode, SIM3)
    sf = np.ascontiguousarray(sf, f32)
    valid, u, v = np.full(n + PAD, V_FILL, np.uint8), np.full(n + PAD, F_FILL, f32), np.full(n + PAD, F_FILL, f32)
    level, vc = np.full(n + PAD, L_FILL, np.int32), np.full(n + PAD, F_FILL, f32)
    cam = _cam(uvo, s["cam"])
    if mm == SIM3:
        ch = [np.ascontiguousarray(c, f32) for c in s["chain"]]
        rc = uvo.lib.uvo_project_sim3(m._h, _p(ch[0]), _p(ch[1]), _p(ch[2]), _p(ch[3]), ctypes.addressof(cam), n, _p(s["xyz"]), _p(s["min_inv"]), _p(s["max_inv"]),
                                      _p(usable), _p(sf), len(sf), _p(valid), _p(u), _p(v), _p(level))
        with_cos = False
    else:
        pixel = mm in (PIXEL_BOUNDED, PIXEL)
        nrm = s["normal"] if all_arrays or mm in (FRUSTUM, FUSE) else None
        mn = s["min_inv"] if all_arrays or not pixel else None
        mx = s["max_inv"] if all_arrays or mm in (FRUSTUM, FUSE) else None
        raw = s["max_raw"] if all_arrays or mm == FRUSTUM else None
        rc = uvo.lib.uvo_project_points(m._h, mm, ctypes.addressof(cam), n, _p(s["xyz"]), _p(nrm), _p(mn), _p(mx), _p(raw), _p(usable), _p(sf), len(sf),
                                        float(sfac), float(cos_limit), _p(valid), _p(u), _p(v), _p(level), _p(vc) if with_cos else None)
    assert rc == 0, uvo.last_error()
    assert (valid[n:] == V_FILL).all() and (bits(u[n:]) == bits(F_FILL)).all() and (bits(v[n:]) == bits(F_FILL)).all() and (level[n:] == L_FILL).all()
    if with_cos:
        assert (bits(vc[n:]) == bits(F_FILL)).all()
    else:
        assert (bits(vc) == bits(F_FILL)).all()                      # never touched
        vc = np.zeros(n + PAD, f32)
    return valid[:n], u[:n], v[:n], level[:n], vc[:n]


def _check(uvo, m, mode, s, sf, sfac, name, **kw):
    for usable in (None, pm.usable_mask(len(s["xyz"]))):
        got = _run(uvo, m, mode, s, sf, sfac, usable=usable, **kw)
        ref = pm.run_model(s, min(mode, SIM3), sf, sfac, usable=usable)
        if not kw.get("with_cos", True):
            ref = ref[:4] + (np.zeros_like(ref[4]),)
        for g, r, what in zip(got, ref, ("valid", "u", "v", "level", "view_cos")):
            assert g.dtype == r.dtype
            np.testing.assert_array_equal(bits(g), bits(r), err_msg="%s, %s, %s%s" % (pm.MODE_IDS[mode], name, what, "" if usable is None else ", masked"))
    return ref


@mode_param
@pytest.mark.parametrize("sfac", [2.0, f32(1.2)], ids=["sf2", "sf1.2f"])
def test_exact_scene(uvo, matcher, mode, sfac):
    s = pm.exact_scene(mode, sfac)
    _check(uvo, matcher, mode, s, pm.T8, sfac, "exact")
    _check(uvo, matcher, mode, s, pm.T8_REPEATED, sfac, "exact, repeated entries")
    _check(uvo, matcher, mode, s, pm.T1, sfac, "exact, one level")
    _check(uvo, matcher, mode, s, pm.T8, sfac, "exact, view_cos NULL", with_cos=False)
    _check(uvo, matcher, mode, s, pm.T8, sfac, "exact, every array given", all_arrays=True)
    if min(mode, SIM3) == KF_RELOC:
        _check(uvo, matcher, mode, dict(s, cam=s["cam"].with_ow(np.full(3, np.nan))), pm.T8, sfac, "exact, cam->ow NaN")


@mode_param
def test_depth_boundary_and_degenerate_scene(uvo, matcher, mode):
    _check(uvo, matcher, mode, pm.depth_scene(mode), pm.T8, 2.0, "depth")
    _check(uvo, matcher, mode, pm.degenerate_scene(mode), pm.T8, 2.0, "degenerate")
    _check(uvo, matcher, mode, pm.degenerate_scene(mode), pm.SF12, f32(1.2), "degenerate, 1.2f")


@mode_param
def test_generic_scene(uvo, matcher, mode):
    for p in range(pm.GENERIC_POSES):
        ref = _check(uvo, matcher, mode, pm.generic_scene(mode, p), pm.SF12, f32(1.2), "generic %d" % p)
    assert ref[0].sum() > 200


@mode_param
def test_launch_shapes(uvo, matcher, mode):
    s = pm.exact_scene(mode, 2.0)
    for n in pm.LAUNCH_SHAPES:
        _check(uvo, matcher, mode, pm.tiled(s, n), pm.T8, 2.0, "n = %d" % n)


def test_argument_checks(uvo, matcher):
    s = pm.exact_scene(FRUSTUM, 2.0)
    n = len(s["xyz"])
    out = [np.zeros(n, np.uint8), np.zeros(n, f32), np.zeros(n, f32), np.zeros(n, np.int32), np.zeros(n, f32)]
    cam = _cam(uvo, s["cam"])

    def call(mode, nrm=s["normal"], mn=s["min_inv"], mx=s["max_inv"], raw=s["max_raw"], sfac=2.0):
        return uvo.lib.uvo_project_points(matcher._h, mode, ctypes.addressof(cam), n, _p(s["xyz"]), _p(nrm), _p(mn), _p(mx), _p(raw), None, _p(pm.T8), 8, float(sfac),
                                          0.5, *[_p(o) for o in out])

    assert call(FRUSTUM) == 0 and call(FUSE) == 0
    assert call(FRUSTUM, sfac=1.0) != 0 and call(FRUSTUM, sfac=0.5) != 0 and call(FRUSTUM, sfac=np.nan) != 0
    assert call(KF_RELOC, sfac=1.0) == 0 and call(FUSE, sfac=1.0) == 0                 # only PredictScale reads it
    assert call(FRUSTUM, raw=None) != 0 and call(FUSE, raw=None) == 0
    assert call(FRUSTUM, nrm=None) != 0 and call(FUSE, nrm=None) != 0
    assert call(FRUSTUM, mx=None) != 0 and call(FUSE, mx=None) != 0 and call(FRUSTUM, mn=None) != 0 and call(KF_RELOC, mn=None) != 0
    assert call(KF_RELOC, nrm=None, mx=None, raw=None) == 0
    for mode in (PIXEL_BOUNDED, PIXEL):
        assert call(mode, nrm=None, mn=None, mx=None, raw=None) == 0
    assert call(-1) != 0 and call(5) != 0


def test_search_points_in_frustum_outputs(uvo, matcher):
    """The optional outputs of uvo_search_points_in_frustum are k_project's FRUSTUM results"""
    for sfac in (2.0, f32(1.2)):
        s = pm.exact_scene(FRUSTUM, sfac)
        n, nk = len(s["xyz"]), 5
        rng = np.random.default_rng(3)
        kp = np.zeros(nk, uvo.KEYPOINT_DTYPE)
        kp["x"], kp["y"], kp["octave"] = rng.uniform(10, 600, nk), rng.uniform(10, 400, nk), rng.integers(0, 8, nk)
        desc, mpd = rng.integers(0, 256, (nk, 32), dtype=np.uint8), rng.integers(0, 256, (n, 32), dtype=np.uint8)
        for usable in (None, pm.usable_mask(n)):
            assigned = np.full(nk, -1, np.int32)
            valid, u, v = np.full(n + PAD, V_FILL, np.uint8), np.full(n + PAD, F_FILL, f32), np.full(n + PAD, F_FILL, f32)
            level, vc = np.full(n + PAD, L_FILL, np.int32), np.full(n + PAD, F_FILL, f32)
            ntm, nm = ctypes.c_int(-5), ctypes.c_int(-5)
            cam = _cam(uvo, s["cam"])
            rc = uvo.lib.uvo_search_points_in_frustum(matcher._h, _p(kp), nk, _p(desc), _p(assigned), ctypes.addressof(cam), n, _p(s["xyz"]), _p(s["normal"]),
                                                      _p(s["min_inv"]), _p(s["max_inv"]), _p(s["max_raw"]), _p(usable), _p(mpd), _p(pm.T8), 8, float(sfac), 0.5, 1.0, 0.8,
                                                      _p(valid), _p(u), _p(v), _p(level), _p(vc), ctypes.byref(ntm), ctypes.byref(nm))
            assert rc == 0, uvo.last_error()
            ref = pm.run_model(s, FRUSTUM, pm.T8, sfac, usable=usable)
            for g, r, what in zip((valid, u, v, level, vc), ref, ("in_view", "proj_x", "proj_y", "level", "view_cos")):
                np.testing.assert_array_equal(bits(g[:n]), bits(r), err_msg=what)
            assert (valid[n:] == V_FILL).all() and (bits(u[n:]) == bits(F_FILL)).all() and (level[n:] == L_FILL).all() and (bits(vc[n:]) == bits(F_FILL)).all()
            assert ntm.value == int(ref[0].sum()) and nm.value >= 0


def test_fuse_batch_projects_as_the_model(uvo, matcher):
    """uvo_fuse_batch returns best_idx only.  Every map point has a key point at its projection, with its own descriptor (rows of the
    Hadamard matrix: 128 bits apart, TH_LOW is 50) on its predicted level, inside its window, so best_idx = its own index exactly where the model says valid.
    Two targets with different poses in one call."""
    s = pm.exact_scene(FUSE, 2.0)
    n = len(s["xyz"])
    mpd = wm.hadamard_descriptors(n)
    cam_a = s["cam"]
    tb = cam_a.tcw + f32([0, 0, 1])                                   # one unit further along the optical axis
    cam_b = pm.Cam(cam_a.rcw, tb, -(cam_a.rcw.reshape(3, 3).astype(np.float64).T @ tb.astype(np.float64)))
    T = (uvo.FuseTargetC * 2)()
    keep, refs = [], []
    for t, cam in enumerate((cam_a, cam_b)):
        valid, u, v, level, _, inter = pm.run_model(dict(s, cam=cam), FUSE, pm.T8, 2.0, full=True)
        refs.append(valid)
        kp = np.zeros(n, uvo.KEYPOINT_DTYPE)
        fin = np.isfinite(inter["u"]) & np.isfinite(inter["v"])
        # a key point at x >= 635 or y >= 475 rounds into column 64 / row 48 and is in no cell (FrameKTL::PosInGrid): the key points of
        # the rows at the far image edges sit just inside that, still within their windows (radius 3 x sf[level] >= 12 there)
        kp["x"], kp["y"], kp["octave"] = np.where(fin, np.minimum(inter["u"], f32(634)), 1), np.where(fin, np.minimum(inter["v"], f32(474)), 1), level
        assert wm.cell_of(kp, (0, 0, 640, 480))[0][valid != 0].all()
        assert (np.maximum(np.abs(kp["x"] - u), np.abs(kp["y"] - v))[valid != 0] <= 3 * pm.T8[level[valid != 0]] - 1).all()
        sf = pm.T8.copy()
        keep += [kp, sf]
        T[t].kp, T[t].n, T[t].desc = _p(kp), n, _p(mpd)
        T[t].min_x, T[t].min_y, T[t].max_x, T[t].max_y = 0, 0, 640, 480
        T[t].cam = _cam(uvo, cam)
        T[t].scale_factors, T[t].nlevels = _p(sf), 8
    assert (refs[0] != refs[1]).any() and refs[0].sum() > 10 and refs[1].sum() > 10
    for usable in (None, pm.usable_mask(n)):
        bi, bd = np.full(2 * n + PAD, L_FILL, np.int32), np.full(2 * n + PAD, L_FILL, np.int32)
        rc = uvo.lib.uvo_fuse_batch(matcher._h, 2, T, n, _p(s["xyz"]), _p(s["normal"]), _p(s["min_inv"]), _p(s["max_inv"]), _p(usable), _p(mpd), 3.0, _p(bi), _p(bd))
        assert rc == 0, uvo.last_error()
        assert (bi[2 * n:] == L_FILL).all() and (bd[2 * n:] == L_FILL).all()
        for t in range(2):
            ok = (refs[t] != 0) & (True if usable is None else usable != 0)
            np.testing.assert_array_equal(bi[t * n:(t + 1) * n], np.where(ok, np.arange(n), -1), err_msg="target %d" % t)
            np.testing.assert_array_equal(bd[t * n:(t + 1) * n], np.where(ok, 0, -1), err_msg="target %d" % t)
