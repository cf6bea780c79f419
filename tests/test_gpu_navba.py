"""The visual-inertial bundle adjustment on the device (csrc/navba.hip) against the host build of the same source
(tests/emu/navba_emu.cpp), bit for bit -- the states and points in double and in float, both masks, the counts and every record of the
trace tap, non-finite values by class -- and against the numpy model through the same layer checks as the host build
(tests/navba_checks.py: the exact replay of the driver's rules, the first linearisation, the trajectory, masks and final estimates)."""
import ctypes

import numpy as np
import pytest

import navba_checks as pc
import navba_model as vm
import navopt_model as nm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def emu(uvo):
    return pc.Emu(uvo)


@pytest.fixture(scope="module")
def matcher(uvo):
    return uvo.ORBmatcher(0.8)


@pytest.fixture(scope="module")
def adj(uvo, matcher):
    a = uvo.NavBundleAdjuster(matcher, 24, 16, 600, 3000, 8)
    yield a
    a.close()


def device_run(adj, sc):
    res = adj.adjust(sc)
    return pc.of_result(res, adj.trace())


def assert_equal_runs(dev, host, what):
    bad = pc.same_run(dev, host)
    assert not bad, (what, bad)


@pytest.mark.parametrize("name", list(vm.SCENES))
def test_scenes_bit_for_bit_and_against_the_model(adj, emu, name):
    """1 free + previous and 2 free + previous + 1 covisible with 8 points; a window key frame fixed by its id; a forward and a backward
    depth entry; a single edge, a point seen only from fixed key frames, a point and a key frame that lose all mono edges, negative depth,
    a flagged point; excluded and not erased; rejected trials; the largest diagonal entry a point's; edge lists of 1, 255, 256, 257, 513 and
    Schur lists of 1, 64, 65, 255, 256, 257; 255 / 256 / 257 points; the realistic window."""
    sc, _ = pc.model(name)
    dev = device_run(adj, sc)
    assert_equal_runs(dev, emu.adjust(sc), name)
    pc.check_all(name, dev)


@pytest.mark.parametrize("name", ["failed_solve", "threshold"])
def test_scenes_held_to_the_host_build_and_the_replay(adj, emu, name):
    """Every solve failing (an infinite covariance); a stored chi2 between 5.991 and 5.991f."""
    sc = getattr(vm, name)()
    dev = device_run(adj, sc)
    assert_equal_runs(dev, emu.adjust(sc), name)
    assert not pc.replay(dev)
    if name == "threshold":
        e = int(sc["begin"][8])
        assert dev.excluded[e] == 1 and dev.erased[e] == 1
    else:
        assert not dev.trace.trial["ok"].any()


def test_largest_reduced_system(adj, emu):
    """F = 24: 276 off-diagonal 15-block pairs, a 360 x 360 solve."""
    sc = vm.widest()
    dev = device_run(adj, sc)
    assert_equal_runs(dev, emu.adjust(sc), "F = 24")
    assert not pc.replay(dev) and dev.trace.lin["n_free"][0] == 24 and dev.trace.trial["ok"].all()
    assert dev.trace.lin["chi2"][dev.iterations[0] - 1] < dev.trace.lin["chi2"][0]


def test_small_call_after_a_large_one_and_the_same_call_twice(adj, emu):
    big, small = pc.model("realistic")[0], pc.model("free1_p8")[0]
    a = device_run(adj, big)
    b = device_run(adj, big)
    assert_equal_runs(a, b, "the same call twice")
    assert_equal_runs(device_run(adj, small), emu.adjust(small), "a small call after a large one")


def test_no_free_key_frame_answers_with_the_inputs(adj):
    sc = dict(pc.model("free2_cov1_p8")[0])
    adj.adjust(sc)
    sc["fixed"] = np.ones(len(sc["fixed"]), np.uint8)
    res = adj.adjust(sc)
    a = vm.arrays(sc)
    est, X = vm.start(a)
    assert np.array_equal(res.kf_state, np.stack([nm.state_vec(s) for s in est])) and np.array_equal(res.point_estimate, X) and np.array_equal(res.points, a["pts"])
    want = np.stack([nm.pose_from_ns(s, dict(Rbc=a["Rbc"], Pbc=a["Pbc"])) for s in est])
    assert np.abs(res.kf_Tcw - want).max() <= 2.0 ** -22 * 4 and res.n_trials == 0 and not res.excluded.any() and not res.erased.any()
    tr = adj.trace()                                             # the trace is this call's: no record, not the call's before
    assert len(tr.lin) == 0 and len(tr.trial) == 0


def test_errors_write_nothing(uvo, matcher, adj):
    E = uvo.UvoError
    for args in ((0, 1, 10, 10, 1), (25, 1, 10, 10, 1), (1, -1, 10, 10, 1), (1, 257, 10, 10, 1), (1, 1, 0, 10, 1), (1, 1, 32769, 10, 1), (1, 1, 10, 0, 1),
                 (1, 1, 10, 262145, 1), (1, 1, 10, 10, -1), (1, 1, 10, 10, 257)):
        with pytest.raises(E) as ei:
            uvo.NavBundleAdjuster(matcher, *args)
        assert ei.value.code == uvo.UVO_E_BADARG, args
    with pytest.raises(E) as ei:
        uvo.NavBundleAdjuster(None, 1, 1, 10, 10, 1)
    assert ei.value.code == uvo.UVO_E_BADARG
    small = uvo.NavBundleAdjuster(matcher, 2, 2, 8, 32, 0)
    try:
        small.adjust(pc.model("free2_cov1_p8")[0])                 # exactly its capacity
        for grow in ("fixed_by_id", "specials", "points_255", "depth_forward"):   # a third fixed key frame; a third free one; more points and edges; a depth entry
            with pytest.raises(E) as ei:
                small.adjust(pc.model(grow)[0])
            assert ei.value.code == uvo.UVO_E_CAPACITY, grow
    finally:
        small.close()
    sc = pc.model("depth_backward")[0]

    def refused(bad, what):
        c, r, arrays, keep = uvo.navba_marshal(bad)
        r.n_trials = -7
        arrays[0][:] = 7.0
        assert adj._api.uvo_nav_bundle_adjust(adj._h, ctypes.byref(c), ctypes.byref(r)) == uvo.UVO_E_BADARG, what
        assert r.n_trials == -7 and (arrays[0] == 7.0).all() and not arrays[4].any() and not arrays[5].any(), what     # nothing is written on an error

    for key, value in (("edge_kf", 5), ("edge_kf", -1), ("edge_camera", 2), ("edge_camera", -1)):
        bad = dict(sc)
        bad[key] = sc[key].copy()
        bad[key][5] = value
        refused(bad, (key, value))
    for field, value in (("kf0", 5), ("kf1", -1), ("kf0", 4)):       # out of range; key frame 4 is the covisible one: it carries no bias vertex
        bad = dict(sc)
        bad["links"] = sc["links"].copy()
        bad["links"][field][1] = value
        refused(bad, ("link", field, value))
    for field, value in (("ka", 5), ("kb", -1), ("kc", 4), ("link", 3), ("link", -1)):
        bad = dict(sc)
        bad["depth"] = sc["depth"].copy()
        bad["depth"][field][0] = value
        refused(bad, ("depth", field, value))
    bad = dict(sc)
    bad["links"] = sc["links"][:2].copy()                            # free key frame 2 has no link ending in it
    refused(bad, "a free key frame without a link")
    bad = dict(sc)
    bad["begin"] = sc["begin"].copy()
    bad["begin"][3] = bad["begin"][2] - 1
    refused(bad, "begin")
    lib = adj._api
    assert lib.uvo_nav_bundle_adjust(None, None, None) == uvo.UVO_E_BADARG and lib.uvo_nav_bundle_adjust(adj._h, None, None) == uvo.UVO_E_BADARG
    assert lib.uvo_nav_bundle_adjuster_trace(adj._h, None) == uvo.UVO_E_BADARG
    # and the adjuster still works
    got = adj.adjust(sc)
    assert got.iterations[0] == 5 and got.n_trials >= 5
