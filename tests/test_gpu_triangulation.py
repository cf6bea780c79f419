"""uvo_triangulate_matches and uvo_create_new_map_points on the device against the test model (tests/triangulation_model.py), under the
tolerance contract of DESIGN.md section 4 (third contract):
  x3D       relative error against the float64 model <= X3D_BOUND = 4 x the float32 model's own measured deviation;
  verdicts  exact wherever the match is not sensitive (no evaluated test within the contract's margin of its threshold);
  the chain the model follows the device on sensitive matches only and must agree on everything else -- every pair's match list, every
            other verdict, every count; sensitive matches are at most 1 % of a scene's matches, and one 20-pair scene has none at all.
"""
import numpy as np
import pytest

import triangulation_model as tm

pytestmark = pytest.mark.gpu


def _cam(uvo, c):
    return uvo.TriangulationCamera(c.rcw, c.tcw, c.ow, c.fx, c.fy, c.cx, c.cy, c.sf, c.sigma2)


def _check_list(label, dev_v, dev_x, r):
    """one match list: device verdicts / points against both()'s result; returns the largest x3D deviation seen"""
    n, ns = len(r["v32"]), int(r["sensitive"].sum())
    clear = ~r["sensitive"]
    np.testing.assert_array_equal(dev_v[clear], r["v32"][clear], err_msg="%s: verdicts of the matches that are not sensitive" % label)
    assert ((dev_v >= 0) & (dev_v <= 8)).all()
    has_point = clear & ((r["v64"] == tm.ACCEPTED) | (r["v64"] >= tm.BEHIND_1))
    no_point = clear & ~has_point
    assert not dev_x[no_point].any(), "%s: x3D is zero where the loop body left before :1131" % label
    dev = tm.rel_dev(dev_x, r["x64"])[has_point]
    worst = float(dev.max()) if len(dev) else 0.0
    print("%s: %d matches, %d sensitive, x3D deviation from the float64 model: max %.3e (bound %.3e)" % (label, n, ns, worst, tm.X3D_BOUND))
    assert worst <= tm.X3D_BOUND, "%s: x3D deviates by %.3e from the float64 model (bound %.3e)" % (label, worst, tm.X3D_BOUND)
    return worst


@pytest.mark.parametrize("seed,n,noise,par", tm.GRID_SCENES)
def test_triangulate_matches_against_the_model(uvo, seed, n, noise, par):
    s = tm.match_list_scene(seed, n, noise, par)
    m = uvo.ORBmatcher(0.6, False)
    v, x = m.TriangulateMatches(_cam(uvo, s["cam1"]), _cam(uvo, s["cam2"]), s["ratio_factor"], s["kp1"], s["kp2"])
    m.close()
    assert v.shape == (n,) and x.shape == (n, 3)
    r = tm.both(s["cam1"], s["cam2"], s["ratio_factor"], s["kp1"], s["kp2"], s["depth"])
    assert int(r["sensitive"].sum()) <= tm.SENSITIVE_CAP * n
    _check_list("seed %d" % seed, v, x, r)


def test_every_rejection_reason_on_the_device(uvo):
    m = uvo.ORBmatcher(0.6, False)
    seen = set()
    for name, expected, c1, c2, a, b in tm.hand_cases():
        v, x = m.TriangulateMatches(_cam(uvo, c1), _cam(uvo, c2), tm.ratio_factor(c1), a, b)
        assert v[0] == expected, name
        r = tm.both(c1, c2, tm.ratio_factor(c1), a, b, 6.0)
        _check_list(name, v, x, r)
        seen.add(int(v[0]))
    assert seen == {tm.ACCEPTED, tm.PARALLAX, tm.BEHIND_1, tm.BEHIND_2, tm.REPROJ_1, tm.REPROJ_2, tm.SCALE}
    # and in bulk: the 1000-match scenes between them hold every reason a random wrong match can reach
    bulk = set()
    for seed, n, noise, par in tm.GRID_SCENES:
        if n == 1000:
            s = tm.match_list_scene(seed, n, noise, par)
            v, _ = m.TriangulateMatches(_cam(uvo, s["cam1"]), _cam(uvo, s["cam2"]), s["ratio_factor"], s["kp1"], s["kp2"])
            bulk |= set(v.tolist())
    m.close()
    assert bulk >= {tm.ACCEPTED, tm.PARALLAX, tm.BEHIND_1, tm.REPROJ_1, tm.REPROJ_2, tm.SCALE}


def test_triangulate_matches_argument_checks(uvo):
    name, expected, c1, c2, a, b = tm.hand_cases()[0]
    m = uvo.ORBmatcher(0.6, False)
    bad = a.copy()
    bad["octave"] = 8                                        # outside the camera's 8 levels
    with pytest.raises(uvo.UvoError) as ei:
        m.TriangulateMatches(_cam(uvo, c1), _cam(uvo, c2), 1.8, bad, b)
    assert ei.value.code == uvo.UVO_E_BADARG
    m.close()


def _pairs(uvo, sc):
    return [(uvo.FeatureVector(P["groups"]), P["kp"], P["desc"], P["has_mp"], P["F12"], P["sigma2"]) for P in sc["pairs"]]


@pytest.mark.parametrize("ori", [False, True])
@pytest.mark.parametrize("name", list(tm.SCENES))
def test_create_new_map_points_against_the_chained_model(uvo, oracle, name, ori):
    sc = tm.make_scene(**tm.SCENES[name])
    fv1, pairs = uvo.FeatureVector(sc["groups1"]), _pairs(uvo, sc)
    m = uvo.ORBmatcher(0.6, ori)
    dev, has_after = m.CreateNewMapPoints(fv1, sc["kp1"], sc["desc1"], sc["has_mp1"], pairs, _cam(uvo, sc["cam1"]), [_cam(uvo, c) for c in sc["cams2"]],
                                          sc["ratio_factor"])
    assert len(dev) == len(sc["pairs"])
    # the model, following the device on sensitive matches only; it compares every pair's match list on its way
    res, has_model = tm.chain(oracle, sc, ori, device=dev)
    n = sum(len(r["idx1"]) for r in res)
    ns = sum(int(r["sensitive"].sum()) for r in res)
    print("%s ori=%d: %d matches in %d pairs, %d sensitive" % (name, ori, n, len(res), ns))
    assert n > 150
    assert ns <= tm.SENSITIVE_CAP * n, "%d of %d matches are sensitive" % (ns, n)
    if name == tm.SCENE_WITHOUT_SENSITIVE:
        assert ns == 0 and len(res) == 20                    # this chain is compared with no exception whatever
    for p, (d, r) in enumerate(zip(dev, res)):
        _check_list("%s pair %d" % (name, p), d["verdict"], d["x3d"], r)
        assert d["n_accepted"] == int((d["verdict"] == tm.ACCEPTED).sum()) == int((r["verdict"] == tm.ACCEPTED).sum())
        assert (np.diff(d["idx1"]) > 0).all()                # ascending idx1
    np.testing.assert_array_equal(has_after, has_model)
    if "empty_pair" in tm.SCENES[name]:
        assert len(dev[tm.SCENES[name]["empty_pair"]]["idx1"]) == 0
    # the same lists from the existing, oracle-held path: uvo_search_for_triangulation_batch + _next fed the same has_mp1 sequence
    mb = uvo.ORBmatcher(0.6, ori)
    mb.SearchForTriangulationBatch(fv1, sc["kp1"], sc["desc1"], sc["has_mp1"], pairs)
    has1 = sc["has_mp1"].copy()
    accepted, again = set(), 0
    for k, d in enumerate(dev):
        match, nm = mb.SearchForTriangulationNext(k, has1)
        idx1 = np.nonzero(match >= 0)[0]
        np.testing.assert_array_equal(d["idx1"], idx1, err_msg="pair %d against _next" % k)
        np.testing.assert_array_equal(d["idx2"], match[idx1], err_msg="pair %d against _next" % k)
        assert nm == len(idx1)
        still, _ = mb.SearchForTriangulationNext(k, sc["has_mp1"])     # what the pair would match had has_mp1 stood still
        again += len(accepted & set(np.nonzero(still >= 0)[0].tolist()))
        assert not (accepted & set(idx1.tolist()))
        won = d["idx1"][d["verdict"] == tm.ACCEPTED]
        accepted |= set(won.tolist())
        has1[won] = 1
    if len(dev) > 1:
        assert again > 0, "no feature accepted in one pair would have matched again later: the hand-over is not exercised"
    m.close()
    mb.close()


def test_create_new_map_points_edges(uvo):
    sc = tm.make_scene(seed=301, n_pairs=2, n_points=120, clutter=20)
    fv1, pairs = uvo.FeatureVector(sc["groups1"]), _pairs(uvo, sc)
    cam1, cams2 = _cam(uvo, sc["cam1"]), [_cam(uvo, c) for c in sc["cams2"]]
    m = uvo.ORBmatcher(0.6, True)
    # no pairs at all
    dev, has_after = m.CreateNewMapPoints(fv1, sc["kp1"], sc["desc1"], sc["has_mp1"], [], cam1, [], sc["ratio_factor"])
    assert dev == [] and (has_after == sc["has_mp1"]).all()
    # every feature of key frame 1 holds a map point already: nothing to match
    dev, has_after = m.CreateNewMapPoints(fv1, sc["kp1"], sc["desc1"], np.ones(len(sc["kp1"]), np.uint8), pairs, cam1, cams2, sc["ratio_factor"])
    assert [len(d["idx1"]) for d in dev] == [0, 0] and has_after.all()
    # the same call twice gives the same answer (nothing of the first call lingers in the handle)
    a, ha = m.CreateNewMapPoints(fv1, sc["kp1"], sc["desc1"], sc["has_mp1"], pairs, cam1, cams2, sc["ratio_factor"])
    b, hb = m.CreateNewMapPoints(fv1, sc["kp1"], sc["desc1"], sc["has_mp1"], pairs, cam1, cams2, sc["ratio_factor"])
    for x, y in zip(a, b):
        for key in ("idx1", "idx2", "verdict", "x3d"):
            np.testing.assert_array_equal(x[key], y[key])
    assert (ha == hb).all() and sum(len(x["idx1"]) for x in a) > 20
    m.close()


def test_create_new_map_points_is_one_launch_chain(uvo):
    """One upload, the distance launch, ONE launch that walks the pairs, one host wait: no per-pair launch, no host visit in between."""
    sc = tm.make_scene(**tm.SCENES["twenty_pairs"])
    m = uvo.ORBmatcher(0.6, True)
    m.profile(True)
    m.CreateNewMapPoints(uvo.FeatureVector(sc["groups1"]), sc["kp1"], sc["desc1"], sc["has_mp1"], _pairs(uvo, sc), _cam(uvo, sc["cam1"]),
                         [_cam(uvo, c) for c in sc["cams2"]], sc["ratio_factor"])
    times = m.kernel_times()
    m.close()
    print(times)
    assert {k: v[1] for k, v in times.items()} == {"k_group_dist_pairs": 1, "k_create_new_map_points": 1}
