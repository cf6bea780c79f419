"""Optimizer::OptimizeSim3 on the device (csrc/sim3opt.hip) against the host build of the same source (tests/emu/sim3opt_emu.cpp),
bit for bit -- the estimate in double and in float, the counts, more_iterations, the mask and every record of the trace tap, non-finite
values by class -- and against the numpy model through the same layer checks as the host build (tests/sim3opt_checks.py: layer 2 on
the trace's first linearisation, the exact replay of the driver's rules and the trajectory prefix of layer 3, layer 4 on the call)."""
import ctypes

import numpy as np
import pytest

import sim3opt_checks as pc
import sim3opt_model as sm

pytestmark = pytest.mark.gpu

LDS_PAIRS = 1024      # kSim3OptLdsPairs


@pytest.fixture(scope="module")
def emu(uvo):
    return pc.Emu(uvo)


@pytest.fixture(scope="module")
def matcher(uvo):
    return uvo.ORBmatcher(0.8)


@pytest.fixture(scope="module")
def opt(uvo, matcher):
    o = uvo.Sim3Optimizer(matcher, 8, 1100)
    yield o
    o.close()


def assert_equal_runs(dev, host, what):
    bad = pc.same_run(dev, host)
    assert not bad, (what, bad)


def device_runs(opt, scenes):
    res = opt.optimize(scenes)
    return [pc.of_result(r, opt.trace(j)) for j, r in enumerate(res)]


def sized(n, seed=0):
    return sm.scene(seed=900 + n + seed, n=n, shifted2=n // 5)


@pytest.mark.parametrize("n", [0, 1, 9, 10, 11, 63, 64, 65, 255, 256, 257, 513, LDS_PAIRS + 1])
def test_sizes_bit_for_bit(opt, emu, n):
    """Above LDS_PAIRS the two chi2 and the state byte of a pair live in the set's block, not in LDS."""
    sc = sized(n)
    dev, = device_runs(opt, [sc])
    assert_equal_runs(dev, emu.optimize(sc), n)
    assert dev.n_correspondences == n and (dev.more_iterations in (5, 10)) == (n - dev.n_bad >= 10)


def test_nothing_to_optimise_returns_the_round_trip(opt):
    sc = sized(0)
    dev, = device_runs(opt, [sc])
    assert dev.n_inliers == 0 and dev.more_iterations == 0 and len(dev.trace.lin) == 0 and len(dev.removed) == 0
    assert np.array_equal(np.concatenate([dev.q, dev.t, [dev.s]]), sm.sim_from_floats(sc["R12"], sc["t12"], sc["s12"]).vec())


def test_max_pairs_of_a_small_set(uvo, matcher, emu):
    small = uvo.Sim3Optimizer(matcher, 1, 37)
    try:
        sc = sized(37)
        dev, = device_runs(small, [sc])
        assert_equal_runs(dev, emu.optimize(sc), "max_pairs 37")
    finally:
        small.close()


@pytest.mark.parametrize("sizes", [(40, 17), (300, 12, 0, 65, 9, 256, 1, 130)])
def test_several_problems_in_one_call(opt, emu, sizes):
    scenes = [sized(n, seed=7 * j) for j, n in enumerate(sizes)]
    for j, dev in enumerate(device_runs(opt, scenes)):
        assert_equal_runs(dev, emu.optimize(scenes[j]), (sizes, j))


@pytest.mark.parametrize("name", ["left_10", "left_9", "all_bad_12", "none_0", "sigma_below", "sigma_above", "zero_z_30", "octave3_60",
                                  "octave3_shift_60", "shift_100", "gross_257", "plain_64"])
def test_special_scenes_bit_for_bit_and_against_the_model(opt, emu, name):
    sc, res = pc.model(name)
    dev, = device_runs(opt, [sc])
    assert_equal_runs(dev, emu.optimize(sc), name)
    pc.check_all(name, dev)


def test_every_scene_against_the_model(opt):
    """The layer checks on the device, eight scenes to a call."""
    names = list(sm.SCENES)
    for i in range(0, len(names), 8):
        part = names[i:i + 8]
        for name, dev in zip(part, device_runs(opt, [pc.model(n)[0] for n in part])):
            pc.check_all(name, dev)


def test_same_call_twice_and_a_small_call_after_a_large_one(opt, emu):
    big = [sized(513), sized(300, 3), sized(257, 5)]
    a = device_runs(opt, big)
    b = device_runs(opt, big)
    for x, y in zip(a, b):
        assert_equal_runs(x, y, "the same call twice")
    small = [sized(11, 2)]
    dev, = device_runs(opt, small)
    assert_equal_runs(dev, emu.optimize(small[0]), "a small call after a large one")
    with pytest.raises(Exception):
        opt.trace(1)          # the last call had one problem


def test_errors(uvo, matcher, opt):
    E = uvo.UvoError
    for args in ((0, 10), (65, 10), (1, 0), (1, 16385)):
        with pytest.raises(E) as ei:
            uvo.Sim3Optimizer(matcher, *args)
        assert ei.value.code == uvo.UVO_E_BADARG, args
    with pytest.raises(E) as ei:
        uvo.Sim3Optimizer(None, 1, 10)
    assert ei.value.code == uvo.UVO_E_BADARG
    with pytest.raises(E) as ei:
        opt.optimize([sized(5)] * 9)
    assert ei.value.code == uvo.UVO_E_CAPACITY
    with pytest.raises(E) as ei:
        opt.optimize([sized(1101)])
    assert ei.value.code == uvo.UVO_E_CAPACITY
    with pytest.raises(E) as ei:
        opt.optimize([sized(20)], removed_cap=19)
    assert ei.value.code == uvo.UVO_E_CAPACITY
    lib = opt._api
    assert lib.uvo_sim3_optimize(None, None, 0, None) == uvo.UVO_E_BADARG
    assert lib.uvo_sim3_optimize(opt._h, None, 1, None) == uvo.UVO_E_BADARG
    assert lib.uvo_sim3_optimize(opt._h, None, -1, None) == uvo.UVO_E_BADARG
    assert lib.uvo_sim3_optimize(opt._h, None, 0, None) == uvo.UVO_OK
    p, r = uvo.Sim3OptProblemC(), uvo.Sim3OptResultC()
    r.n_inliers = -7
    p.n = -1
    assert lib.uvo_sim3_optimize(opt._h, ctypes.byref(p), 1, ctypes.byref(r)) == uvo.UVO_E_BADARG
    p.n = 3                   # pairs announced, none given
    assert lib.uvo_sim3_optimize(opt._h, ctypes.byref(p), 1, ctypes.byref(r)) == uvo.UVO_E_BADARG
    assert r.n_inliers == -7  # nothing is written on an error
    assert lib.uvo_sim3_optimizer_trace(opt._h, 0, None) == uvo.UVO_E_BADARG
    with pytest.raises(E) as ei:
        opt.trace(-1)
    assert ei.value.code == uvo.UVO_E_BADARG
    # and the set still works
    got, = opt.optimize([sized(12)])
    assert got.n_correspondences == 12 and got.more_iterations in (0, 5, 10)
