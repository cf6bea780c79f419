"""The test model of the triangulation (tests/triangulation_model.py) against itself and against closed-form cases, and the argument
checks of the new entry points.  No GPU needed."""
import ctypes

import numpy as np
import pytest

import triangulation_model as tm


def test_noise_free_matches_give_back_the_true_point():
    s = tm.match_list_scene(seed=7, n=200, noise=0.0, parallax_deg=6.0, wrong_share=0.0)
    # the key points themselves are float32 (~3e-5 px of rounding at 700 px, times depth / baseline): 1e-4 of the point's norm
    for prec, tol in (("f64", 1e-4), ("f32", 2e-4)):
        v, x, _ = tm.triangulate(s["cam1"], s["cam2"], s["ratio_factor"], s["kp1"], s["kp2"], prec, s["depth"])
        assert (v == tm.ACCEPTED).all()
        for cam, kp in ((s["cam1"], s["kp1"]), (s["cam2"], s["kp2"])):
            pu, pv, pz = cam.project(x)
            assert (pz > 0).all()
            assert np.abs(pu - kp["x"]).max() < 0.02 and np.abs(pv - kp["y"]).max() < 0.02
        assert tm.rel_dev(x, s["Xw"]).max() < tol
    # and the point itself: a hand-built one
    name, exp, c1, c2, a, b = tm.hand_cases()[0]
    v, x, _ = tm.triangulate(c1, c2, tm.ratio_factor(c1), a, b, "f64", 6.0)
    assert v[0] == tm.ACCEPTED
    np.testing.assert_allclose(x[0], [0.3, -0.2, 6.0], rtol=0, atol=2e-6)


@pytest.mark.parametrize("case", tm.hand_cases(), ids=[c[0] for c in tm.hand_cases()])
def test_each_verdict_code_by_hand(case):
    name, expected, c1, c2, a, b = case
    r = tm.both(c1, c2, tm.ratio_factor(c1), a, b, 6.0)
    assert r["v32"][0] == expected and r["v64"][0] == expected
    assert not r["sensitive"][0], "a hand-built case must sit clear of every threshold"


def test_hand_cases_cover_every_reachable_code():
    # W_ZERO and ZERO_DIST need an exactly zero homogeneous coordinate / a point exactly at a camera centre: not reachable by data
    assert {c[1] for c in tm.hand_cases()} == {tm.ACCEPTED, tm.PARALLAX, tm.BEHIND_1, tm.BEHIND_2, tm.REPROJ_1, tm.REPROJ_2, tm.SCALE}


def _all_match_lists(oracle):
    """every match list of the committed scenes: (label, both()-result)"""
    for name, kw in tm.SCENES.items():
        sc = tm.make_scene(**kw)
        for ori in (False, True):
            res, _ = tm.chain(oracle, sc, ori)
            yield "%s/ori=%d" % (name, ori), res
    for seed, n, noise, par in tm.GRID_SCENES:
        s = tm.match_list_scene(seed, n, noise, par)
        yield "grid/%d" % seed, [tm.both(s["cam1"], s["cam2"], s["ratio_factor"], s["kp1"], s["kp2"], s["depth"])]


def test_float32_and_float64_models_agree_on_the_committed_scenes(oracle):
    total = 0
    for label, res in _all_match_lists(oracle):
        n = sum(len(r["v32"]) for r in res)
        ns = sum(int(r["sensitive"].sum()) for r in res)
        total += n
        for p, r in enumerate(res):
            clear = ~r["sensitive"]
            np.testing.assert_array_equal(r["v32"][clear], r["v64"][clear], err_msg="%s pair %d" % (label, p))
        # the cap of the tolerance contract holds for the model alone
        assert ns <= tm.SENSITIVE_CAP * n, "%s: %d of %d matches are sensitive" % (label, ns, n)
    assert total > 5000


def test_one_twenty_pair_chain_has_no_sensitive_match(oracle):
    sc = tm.make_scene(**tm.SCENES[tm.SCENE_WITHOUT_SENSITIVE])
    assert len(sc["pairs"]) == 20
    for ori in (False, True):
        res, _ = tm.chain(oracle, sc, ori)
        assert sum(int(r["sensitive"].sum()) for r in res) == 0
        assert sum(len(r["idx1"]) for r in res) > 300


def test_float32_model_deviation_is_the_recorded_one(oracle):
    """X3D_F32_MODEL_DEVIATION is a measurement of the float32 model on the committed scenes, and the kernel's bound is 4 x that.  LAPACK
    builds differ in summation order, so the measurement has to come out within a factor of two of the recorded value, either way."""
    worst = 0.0
    for label, res in _all_match_lists(oracle):
        for r in res:
            has_point = (r["v64"] == tm.ACCEPTED) | (r["v64"] >= tm.BEHIND_1)
            if has_point.any():
                worst = max(worst, float(tm.rel_dev(r["x32"], r["x64"])[has_point].max()))
    print("largest relative deviation of the float32 model from the float64 model: %.3e (recorded %.3e, kernel bound %.3e)"
          % (worst, tm.X3D_F32_MODEL_DEVIATION, tm.X3D_BOUND))
    assert 0.5 * tm.X3D_F32_MODEL_DEVIATION <= worst <= 2.0 * tm.X3D_F32_MODEL_DEVIATION


def test_chain_hands_map_points_over(oracle):
    """The scenes really exercise the hand-over: features accepted in pair j would match again in a later pair if has_mp1 stood still."""
    sc = tm.make_scene(**tm.SCENES["twenty_pairs"])
    res, has1 = tm.chain(oracle, sc, False)
    accepted, again = set(), 0
    for r, P in zip(res, sc["pairs"]):
        m0, _ = oracle.search_for_triangulation(sc["groups1"], sc["kp1"], sc["desc1"], sc["has_mp1"], P["groups"], P["kp"], P["desc"], P["has_mp"],
                                                P["F12"], P["sigma2"], False)
        again += len(accepted & set(np.nonzero(m0 >= 0)[0].tolist()))
        assert not (accepted & set(r["idx1"].tolist())), "a feature that holds a map point was matched again"
        accepted |= set(r["idx1"][r["verdict"] == tm.ACCEPTED].tolist())
    assert again > 100
    assert has1.sum() == sc["has_mp1"].sum() + len(accepted)


def test_new_entry_points_reject_a_null_handle(uvo):
    lib = uvo.lib
    R = np.eye(3)
    c = uvo.TriangulationCamera(R, [0, 0, 0], [0, 0, 0], 458, 457, 367, 248, [1.0, 1.2], [1.0, 1.44])
    kp = np.zeros(1, uvo.KEYPOINT_DTYPE)
    verdict, x3d = np.zeros(1, np.int32), np.zeros(3, np.float32)
    assert lib.uvo_triangulate_matches(None, ctypes.byref(c.c), ctypes.byref(c.c), 1.8, kp.ctypes.data, kp.ctypes.data, 1, verdict.ctypes.data,
                                       x3d.ctypes.data) == uvo.UVO_E_BADARG
    fv = uvo.FeatureVector({})
    nm = np.zeros(1, np.int32)
    out = uvo.NewMapPointsC(nm.ctypes.data, nm.ctypes.data, None, None, None, None, None)
    has = np.zeros(1, np.uint8)
    desc = np.zeros(32, np.uint8)
    assert lib.uvo_create_new_map_points(None, ctypes.byref(fv.c), kp.ctypes.data, 1, desc.ctypes.data, has.ctypes.data, 0, None, ctypes.byref(c.c), None,
                                         1.8, 0, ctypes.byref(out)) == uvo.UVO_E_BADARG
    assert b"null handle" in lib.uvo_last_error()
