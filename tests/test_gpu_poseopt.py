"""Optimizer::PoseOptimization on the device (csrc/poseopt.hip) against the host build of the same source (tests/emu/poseopt_emu.cpp),
BIT FOR BIT: Tcw, the masks, the counts, rounds and every record of the trace tap (non-finite values by class: host and device NaNs
differ in sign) -- and against the numpy model through the same layer checks as the host build (tests/poseopt_checks.py: layer 2 on
the first linearisation, layers 4 and 5).  The shapes are the smallest at which the call can still go wrong: around the break test
at 10, around one wavefront (64), one pass of the workgroup (256) and two (513), the set's max_points, several problems of unequal
size with an empty one in the middle, the special scenes, a repeated call, a large call followed by a small one, every error."""
import ctypes

import numpy as np
import pytest

import poseopt_checks as pc
import poseopt_model as pm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def emu(uvo):
    return pc.Emu(uvo)


@pytest.fixture(scope="module")
def klt(uvo):
    k = uvo.KLT(64, 64, max_points=16)
    yield k
    k.close()


@pytest.fixture(scope="module")
def opt(uvo, klt):
    o = uvo.PoseOptimizer(klt, 8, 2600)
    yield o
    o.close()


def same_bits(a, b):
    """Equal bit for bit where finite, equal by class where not."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.names:
        return all(same_bits(a[n], b[n]) for n in a.dtype.names if n != "pad_")
    if a.dtype.kind != "f":
        return a.tobytes() == b.tobytes()
    fin = np.isfinite(a)
    return a.shape == b.shape and pc.same_class(a, b) and a[fin].tobytes() == b[fin].tobytes()


def assert_equal_runs(dev, host, what):
    assert (dev.n_inliers, dev.rounds) == (host.n_inliers, host.rounds), what
    assert dev.outlier.tobytes() == host.outlier.tobytes(), what
    assert same_bits(dev.Tcw, host.Tcw), (what, dev.Tcw, host.Tcw)
    assert same_bits(dev.trace.R, host.trace.R) and same_bits(dev.trace.t, host.trace.t), what
    assert len(dev.trace.lin) == len(host.trace.lin) and len(dev.trace.trial) == len(host.trace.trial), what
    assert same_bits(dev.trace.lin, host.trace.lin), (what, "linearisations")
    assert same_bits(dev.trace.trial, host.trace.trial), (what, "trials")


def device_runs(opt, scenes):
    res = opt.optimize(scenes)
    return [pc.Run(r.Tcw, r.n_inliers, r.rounds, r.outlier, opt.trace(j)) for j, r in enumerate(res)]


def sized(n, seed=0):
    return pm.scene(seed=900 + n + seed, n=n, shifted=n // 4, off=(0.1, 0.2))


@pytest.mark.parametrize("n", [0, 1, 2, 3, 5, 9, 10, 11, 63, 64, 65, 255, 256, 257, 513])
def test_sizes_bit_for_bit(opt, emu, n):
    sc = sized(n)
    dev, = device_runs(opt, [sc])
    assert_equal_runs(dev, emu.optimize(sc), n)
    assert dev.rounds == (1 if n < 10 else 4)


def test_nothing_to_optimise_returns_the_round_trip(opt, emu):
    sc = sized(0)
    dev, = device_runs(opt, [sc])
    assert dev.n_inliers == 0 and len(dev.trace.lin) == 0 and dev.Tcw.tobytes() == pm.matrix_of(*pm.pose_of(sc[4]))[0].tobytes()


def test_max_points_of_a_small_set_and_edge_state_beyond_lds(uvo, klt, emu, opt):
    small = uvo.PoseOptimizer(klt, 1, 37)
    try:
        sc = sized(37)
        dev, = device_runs(small, [sc])
        assert_equal_runs(dev, emu.optimize(sc), "max_points 37")
    finally:
        small.close()
    sc = sized(2600)          # above 2048 edges the chi2 and state bytes live in the set's block, not in LDS
    dev, = device_runs(opt, [sc])
    assert_equal_runs(dev, emu.optimize(sc), 2600)


@pytest.mark.parametrize("sizes", [(40, 17), (300, 12, 0, 65, 9, 256, 1, 130)])
def test_several_problems_in_one_call(opt, emu, sizes):
    scenes = [sized(n, seed=7 * j) for j, n in enumerate(sizes)]
    for j, dev in enumerate(device_runs(opt, scenes)):
        assert_equal_runs(dev, emu.optimize(scenes[j]), (sizes, j))


@pytest.mark.parametrize("name", ["shift_100_2", "shift_150_5", "plain_1000", "thin_12", "few_9", "none_left_12", "plane_exact_50", "plain_64", "gross_257"])
def test_special_scenes_bit_for_bit_and_against_the_model(opt, emu, name):
    sc, res = pc.model(name)
    dev, = device_runs(opt, [sc])
    assert_equal_runs(dev, emu.optimize(sc), name)
    k = pc.check_all(name, dev, pc.first_sums(dev) if name != "plane_exact_50" else None)
    print(name, "compared prefix", k, "of", len(res.trials))
    if name in pm.REENTRY or name == "plain_1000":
        assert pm.reentries(res) >= 1


def test_every_scene_against_the_model(opt):
    """The layer checks on the device, eight scenes to a call."""
    names = list(pm.SCENES)
    for i in range(0, len(names), 8):
        part = names[i:i + 8]
        for name, dev in zip(part, device_runs(opt, [pc.model(n)[0] for n in part])):
            pc.check_all(name, dev, pc.first_sums(dev) if name != "plane_exact_50" else None)


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


def test_errors(uvo, klt, opt):
    E = uvo.UvoError
    for args in ((0, 10), (65, 10), (1, 0), (1, 16385)):
        with pytest.raises(E) as ei:
            uvo.PoseOptimizer(klt, *args)
        assert ei.value.code == uvo.UVO_E_BADARG, args
    with pytest.raises(E) as ei:
        uvo.PoseOptimizer(None, 1, 10)
    assert ei.value.code == uvo.UVO_E_BADARG
    with pytest.raises(E) as ei:
        opt.optimize([sized(5)] * 9)
    assert ei.value.code == uvo.UVO_E_CAPACITY
    with pytest.raises(E) as ei:
        opt.optimize([sized(2601)])
    assert ei.value.code == uvo.UVO_E_CAPACITY
    with pytest.raises(E) as ei:
        opt.optimize([sized(20)], outlier_cap=19)
    assert ei.value.code == uvo.UVO_E_CAPACITY
    lib = opt._api
    assert lib.uvo_pose_optimize(None, None, 0, None) == uvo.UVO_E_BADARG
    assert lib.uvo_pose_optimize(opt._h, None, 1, None) == uvo.UVO_E_BADARG
    assert lib.uvo_pose_optimize(opt._h, None, -1, None) == uvo.UVO_E_BADARG
    assert lib.uvo_pose_optimize(opt._h, None, 0, None) == uvo.UVO_OK
    p, r = uvo.PoseProblemC(), uvo.PoseResultC()
    p.n = -1
    assert lib.uvo_pose_optimize(opt._h, ctypes.byref(p), 1, ctypes.byref(r)) == uvo.UVO_E_BADARG
    p.n = 3                   # points announced, none given
    assert lib.uvo_pose_optimize(opt._h, ctypes.byref(p), 1, ctypes.byref(r)) == uvo.UVO_E_BADARG
    assert lib.uvo_pose_optimizer_trace(opt._h, 0, None) == uvo.UVO_E_BADARG
    with pytest.raises(E) as ei:
        opt.trace(-1)
    assert ei.value.code == uvo.UVO_E_BADARG
    # and the set still works
    assert opt.optimize([sized(12)])[0].rounds == 4
