"""The bundle adjustment on the device (csrc/ba.hip) against the host build of the same source (tests/emu/ba_emu.cpp), bit for bit --
the estimates in double and in float, both masks, the counts and every record of the trace tap, non-finite values by class -- and
against the numpy model through the same layer checks as the host build (tests/ba_checks.py: the exact replay of the driver's rules,
the first linearisation, the trajectory, masks and final estimates of every clear scene)."""
import ctypes

import numpy as np
import pytest

import ba_checks as pc
import ba_model as bm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def emu(uvo):
    return pc.Emu(uvo)


@pytest.fixture(scope="module")
def matcher(uvo):
    return uvo.ORBmatcher(0.8)


@pytest.fixture(scope="module")
def adj(uvo, matcher):
    a = uvo.BundleAdjuster(matcher, 64, 16, 8200, 25000)
    yield a
    a.close()


def device_run(adj, sc):
    res = adj.adjust(sc, sc.get("mode", bm.LOCAL), sc.get("n_iterations", 0))
    return pc.of_result(res, adj.trace())


def assert_equal_runs(dev, host, what):
    bad = pc.same_run(dev, host)
    assert not bad, (what, bad)


@pytest.mark.parametrize("name", list(bm.SCENES))
def test_scenes_bit_for_bit_and_against_the_model(adj, emu, name):
    """2 + 1 and 3 + 0 key frames with 8 points; a single edge, a point seen only from fixed key frames, a point and a key frame that
    drop out, negative depth, a flagged point; a rejected trial, failed solves; edge lists of 1, 255, 256, 257, 513 and Schur lists of
    1, 64, 65, 255, 256, 257; 255 / 256 / 257 points; the realistic scene; full mode with 20 iterations."""
    sc, _ = pc.model(name)
    dev = device_run(adj, sc)
    assert_equal_runs(dev, emu.adjust(sc), name)
    pc.check_all(name, dev)


def test_largest_reduced_system(adj, emu):
    """F = 64 with 4 points per key-frame pair: 2016 Schur blocks off the diagonal, a 384 x 384 solve."""
    sc = bm.widest()
    dev = device_run(adj, sc)
    assert_equal_runs(dev, emu.adjust(sc), "F = 64")
    assert not pc.replay(dev) and dev.trace.lin["n_free"][0] == 64 and dev.trace.lin["n_points"][0] == 8064
    assert dev.trace.lin["chi2"][dev.iterations[0] - 1] < dev.trace.lin["chi2"][0]


def test_small_call_after_a_large_one_and_the_same_call_twice(adj, emu):
    big, small = pc.model("realistic")[0], pc.model("kf2_fixed1_p8")[0]
    a = device_run(adj, big)
    b = device_run(adj, big)
    assert_equal_runs(a, b, "the same call twice")
    assert_equal_runs(device_run(adj, small), emu.adjust(small), "a small call after a large one")


def test_no_free_key_frame_answers_with_the_inputs(adj):
    sc = dict(pc.model("kf2_fixed1_p8")[0])
    adj.adjust(sc)
    sc["fixed"] = np.ones(3, np.uint8)
    res = adj.adjust(sc)
    a = bm.arrays(sc)
    est, X = bm.start(a)
    assert np.array_equal(res.kf_estimate, est) and np.array_equal(res.point_estimate, X) and np.array_equal(res.points, a["pts"])
    assert np.array_equal(res.kf_Tcw[:, :3, :].reshape(-1, 12), a["T"]) and res.n_trials == 0 and not res.removed1.any()
    tr = adj.trace()                                             # the trace is this call's: no record, not the call's before
    assert len(tr.lin) == 0 and len(tr.trial) == 0


def test_errors_write_nothing(uvo, matcher, adj):
    E = uvo.UvoError
    for args in ((0, 1, 10, 10), (65, 1, 10, 10), (1, -1, 10, 10), (1, 257, 10, 10), (1, 1, 0, 10), (1, 1, 32769, 10), (1, 1, 10, 0), (1, 1, 10, 262145)):
        with pytest.raises(E) as ei:
            uvo.BundleAdjuster(matcher, *args)
        assert ei.value.code == uvo.UVO_E_BADARG, args
    with pytest.raises(E) as ei:
        uvo.BundleAdjuster(None, 1, 1, 10, 10)
    assert ei.value.code == uvo.UVO_E_BADARG
    small = uvo.BundleAdjuster(matcher, 2, 1, 8, 24)
    try:
        sc = pc.model("kf2_fixed1_p8")[0]
        small.adjust(sc)                                           # exactly its capacity
        for grow in ("lonely_keyframe", "specials", "points_255"):  # a third free key frame; a second fixed one; more points and edges
            with pytest.raises(E) as ei:
                small.adjust(pc.model(grow)[0])
            assert ei.value.code == uvo.UVO_E_CAPACITY, grow
    finally:
        small.close()
    sc = pc.model("kf2_fixed1_p8")[0]
    for key, value in (("edge_kf", 3), ("edge_kf", -1), ("edge_camera", 2), ("edge_camera", -1)):
        bad = dict(sc)
        bad[key] = sc[key].copy()
        bad[key][5] = value
        c, r, arrays, keep = uvo.ba_marshal(bad)
        r.n_trials = -7
        arrays[0][:] = 7.0
        assert adj._api.uvo_bundle_adjust(adj._h, ctypes.byref(c), ctypes.byref(r)) == uvo.UVO_E_BADARG, (key, value)
        assert r.n_trials == -7 and (arrays[0] == 7.0).all() and not arrays[4].any()     # nothing is written on an error
    bad = dict(sc)
    bad["begin"] = sc["begin"].copy()
    bad["begin"][3] = bad["begin"][2] - 1
    with pytest.raises(E) as ei:
        adj.adjust(bad)
    assert ei.value.code == uvo.UVO_E_BADARG
    twice = dict(sc)
    twice["edge_kf"] = sc["edge_kf"].copy()
    twice["edge_kf"][1] = twice["edge_kf"][0]                      # two edges of one point to one free key frame
    with pytest.raises(E) as ei:
        adj.adjust(twice)
    assert ei.value.code == uvo.UVO_E_BADARG
    for mode, its in ((2, 5), (uvo.UVO_BA_FULL, 0), (uvo.UVO_BA_FULL, 33)):
        with pytest.raises(E) as ei:
            adj.adjust(sc, mode, its)
        assert ei.value.code == uvo.UVO_E_BADARG
    lib = adj._api
    assert lib.uvo_bundle_adjust(None, None, None) == uvo.UVO_E_BADARG and lib.uvo_bundle_adjust(adj._h, None, None) == uvo.UVO_E_BADARG
    assert lib.uvo_bundle_adjuster_trace(adj._h, None) == uvo.UVO_E_BADARG
    # and the adjuster still works
    got = adj.adjust(sc)
    assert got.iterations[0] == 5 and got.n_trials >= 5
