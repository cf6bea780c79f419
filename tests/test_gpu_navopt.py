"""The two IMU overloads of Optimizer::PoseOptimization on the device (csrc/navopt.hip) against the host build of the same source
(tests/emu/navopt_emu.cpp), BIT FOR BIT: the recovered NavState, Tcw, the masks of both frames, the counts, rounds, the marginals and
every record of the trace tap (non-finite values by class: host and device NaNs differ in sign) -- and against the numpy model
through the same layer checks as the host build (tests/navopt_checks.py: layer 2 on the trace, layers 4, 5 and 6).  The shapes are
the smallest at which the call can still go wrong: around the early returns (n < 3, n < 4), around the break test at 10 edges of the
whole graph, around one wavefront (64), one pass of the workgroup (256) and two (513), above the kernel's LDS edge capacity (2048), the
set's max_points, several problems of mixed form and unequal size with an empty one among them, the special scenes, a repeated call,
a large call followed by a small one, every error."""
import ctypes

import numpy as np
import pytest

import navopt_checks as nc
import navopt_model as nm

pytestmark = pytest.mark.gpu
KF, FR = nm.KEYFRAME, nm.FRAME


@pytest.fixture(scope="module")
def emu(uvo):
    return nc.Emu(uvo)


@pytest.fixture(scope="module")
def klt(uvo):
    k = uvo.KLT(64, 64, max_points=16)
    yield k
    k.close()


@pytest.fixture(scope="module")
def opt(uvo, klt):
    o = uvo.NavOptimizer(klt, 8, 2200)
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
    return a.shape == b.shape and nc.same_class(a, b) and a[fin].tobytes() == b[fin].tobytes()


def assert_equal_runs(dev, host, what):
    assert (dev.n_inliers, dev.rounds, dev.marg_ok) == (host.n_inliers, host.rounds, host.marg_ok), what
    assert len(dev.outlier) == len(host.outlier) and all(a.tobytes() == b.tobytes() for a, b in zip(dev.outlier, host.outlier)), what
    assert same_bits(nm.state_vec(dev.ns), nm.state_vec(host.ns)), (what, nm.state_vec(dev.ns) - nm.state_vec(host.ns))
    assert same_bits(dev.Tcw, host.Tcw), (what, dev.Tcw, host.Tcw)
    assert same_bits(dev.marg_cov, host.marg_cov) and same_bits(dev.marg_cov_inv, host.marg_cov_inv), (what, "marginals")
    assert len(dev.trace.lin) == len(host.trace.lin) and len(dev.trace.trial) == len(host.trace.trial), what
    assert same_bits(dev.trace.lin, host.trace.lin), (what, "linearisations")
    assert same_bits(dev.trace.trial, host.trace.trial), (what, "trials")


def device_runs(opt, scenes):
    res = opt.optimize(scenes)
    return [nc.Run(r.ns, r.Tcw, r.n_inliers, r.rounds, [r.outlier] + ([r.outlier_last] if sc["form"] == FR else []), r.marg_cov, r.marg_cov_inv, r.marg_ok,
                   opt.trace(j)) for j, (sc, r) in enumerate(zip(scenes, res))]


def sized(form, n, n_last=None, seed=0, **kw):
    kw.setdefault("marg", True)
    return nm.scene(seed=900 + 3 * n + form + seed, form=form, n=n, n_last=n_last, shifted=n // 4, **kw)


@pytest.mark.parametrize("form", [KF, FR])
@pytest.mark.parametrize("n", [0, 2, 3, 4])
def test_around_the_early_return(opt, emu, form, n):
    sc = sized(form, n, n_last=12)
    dev, = device_runs(opt, [sc])
    assert_equal_runs(dev, emu.optimize(sc), (form, n))
    ran = n >= (4 if form == FR else 3)
    assert dev.rounds == (4 if ran and form == FR else 1 if ran else 0) and (ran or (dev.n_inliers == 0 and not dev.outlier[0].any() and len(dev.trace.lin) == 0))
    if not ran:      # nothing changed: the state as it came, its quaternion normalised
        assert np.abs(nm.state_vec(dev.ns) - nm.state_vec(sc["cur"])).max() <= 4 * nc.U


# the break test counts ALL edges of the graph: n + n_last + IMU + bias (+ prior) (+ depth)
@pytest.mark.parametrize("form,n,depth,edges", [(KF, 7, False, 9), (KF, 8, False, 10), (KF, 6, True, 9), (KF, 7, True, 10), (FR, 6, False, 9), (FR, 7, False, 10),
                                                (FR, 5, True, 9), (FR, 6, True, 10)])
def test_break_test_boundary(opt, emu, form, n, depth, edges):
    sc = sized(form, n, n_last=0, has_depth=depth)
    assert nm.n_edges(sc) == edges
    dev, = device_runs(opt, [sc])
    assert_equal_runs(dev, emu.optimize(sc), (form, n, depth))
    assert dev.rounds == (1 if edges < 10 else 4)


@pytest.mark.parametrize("form", [KF, FR])
@pytest.mark.parametrize("n", [63, 64, 65, 255, 256, 257, 513])
def test_sizes_bit_for_bit(opt, emu, form, n):
    sc = sized(form, n, n_last=max(n - 7, 0), has_depth=n % 2 == 1)
    dev, = device_runs(opt, [sc])
    assert_equal_runs(dev, emu.optimize(sc), (form, n))
    assert dev.rounds == 4 and dev.marg_ok == 1


def test_max_points_of_a_small_set_and_edge_state_beyond_lds(uvo, klt, emu, opt):
    small = uvo.NavOptimizer(klt, 1, 37)
    try:
        for form in (KF, FR):
            sc = sized(form, 37, n_last=37)
            dev, = device_runs(small, [sc])
            assert_equal_runs(dev, emu.optimize(sc), ("max_points 37", form))
    finally:
        small.close()
    # above 2048 edges of both frames together the chi2 and state bytes live in the set's block, not in LDS
    for sc in (sized(KF, 2100), sized(FR, 1100, n_last=1000)):
        dev, = device_runs(opt, [sc])
        assert_equal_runs(dev, emu.optimize(sc), "beyond the LDS capacity")


def test_eight_problems_of_mixed_form_in_one_call(opt, emu):
    shapes = [(KF, 300, 0), (FR, 40, 17), (KF, 0, 0), (FR, 65, 130), (KF, 9, 0), (FR, 256, 1), (KF, 1, 0), (FR, 130, 0)]
    scenes = [sized(f, n, n_last=nl, seed=7 * j, has_depth=j % 3 == 0, marg=j % 2 == 0) for j, (f, n, nl) in enumerate(shapes)]
    for j, dev in enumerate(device_runs(opt, scenes)):
        assert_equal_runs(dev, emu.optimize(scenes[j]), (shapes[j], j))


SPECIAL = ["kf_shift_100", "fr_shift_150", "kf_none_left_12", "fr_none_left_12", "kf_degenerate_50", "fr_degenerate_50", "kf_bias_step_100", "fr_bias_step_100",
           "kf_depth_marg_120", "fr_depth_marg_120", "kf_few_5", "fr_too_few"]


def test_special_scenes_bit_for_bit_and_against_the_model(opt, emu):
    for i in range(0, len(SPECIAL), 8):
        part = SPECIAL[i:i + 8]
        for name, dev in zip(part, device_runs(opt, [nc.model(n)[0] for n in part])):
            assert_equal_runs(dev, emu.optimize(nc.model(name)[0]), name)
            k = nc.check_all(name, dev)
            print(name, "compared prefix", k, "of", len(nc.model(name)[1].trials))


def test_every_scene_against_the_model(opt):
    """The layer checks on the device, eight scenes to a call."""
    names = list(nm.SCENES)
    for i in range(0, len(names), 8):
        part = names[i:i + 8]
        for name, dev in zip(part, device_runs(opt, [nc.model(n)[0] for n in part])):
            nc.check_all(name, dev)


def test_same_call_twice_and_a_small_call_after_a_large_one(opt, emu):
    big = [sized(FR, 513, n_last=300), sized(KF, 300, seed=3), sized(FR, 257, n_last=64, seed=5)]
    a = device_runs(opt, big)
    b = device_runs(opt, big)
    for x, y in zip(a, b):
        assert_equal_runs(x, y, "the same call twice")
    small = [sized(KF, 11, seed=2)]
    dev, = device_runs(opt, small)
    assert_equal_runs(dev, emu.optimize(small[0]), "a small call after a large one")
    with pytest.raises(Exception):
        opt.trace(1)          # the last call had one problem


def test_errors(uvo, klt, opt):
    E = uvo.UvoError
    for args in ((0, 10), (65, 10), (1, 0), (1, 16385)):
        with pytest.raises(E) as ei:
            uvo.NavOptimizer(klt, *args)
        assert ei.value.code == uvo.UVO_E_BADARG, args
    with pytest.raises(E) as ei:
        uvo.NavOptimizer(None, 1, 10)
    assert ei.value.code == uvo.UVO_E_BADARG
    with pytest.raises(E) as ei:
        opt.optimize([sized(KF, 5)] * 9)
    assert ei.value.code == uvo.UVO_E_CAPACITY
    for sc in (sized(KF, 2201), sized(FR, 10, n_last=2201)):
        with pytest.raises(E) as ei:
            opt.optimize([sc])
        assert ei.value.code == uvo.UVO_E_CAPACITY
    with pytest.raises(E) as ei:
        opt.optimize([sized(FR, 20, n_last=20)], outlier_cap=19)
    assert ei.value.code == uvo.UVO_E_CAPACITY
    bad = sized(KF, 5)
    bad["form"] = 2
    with pytest.raises(E) as ei:
        opt.optimize([bad])
    assert ei.value.code == uvo.UVO_E_BADARG
    lib = opt._api
    assert lib.uvo_nav_optimize(None, None, 0, None) == uvo.UVO_E_BADARG
    assert lib.uvo_nav_optimize(opt._h, None, 1, None) == uvo.UVO_E_BADARG
    assert lib.uvo_nav_optimize(opt._h, None, -1, None) == uvo.UVO_E_BADARG
    assert lib.uvo_nav_optimize(opt._h, None, 0, None) == uvo.UVO_OK
    p, r = uvo.NavProblemC(), uvo.NavResultC()
    p.n = -1
    assert lib.uvo_nav_optimize(opt._h, ctypes.byref(p), 1, ctypes.byref(r)) == uvo.UVO_E_BADARG
    p.n = 3                   # points announced, none given
    assert lib.uvo_nav_optimize(opt._h, ctypes.byref(p), 1, ctypes.byref(r)) == uvo.UVO_E_BADARG
    p.n, p.form, p.n_last = 0, uvo.NAV_FRAME, 3
    assert lib.uvo_nav_optimize(opt._h, ctypes.byref(p), 1, ctypes.byref(r)) == uvo.UVO_E_BADARG
    assert lib.uvo_nav_optimizer_trace(opt._h, 0, None) == uvo.UVO_E_BADARG
    with pytest.raises(E) as ei:
        opt.trace(-1)
    assert ei.value.code == uvo.UVO_E_BADARG
    # and the set still works
    assert opt.optimize([sized(KF, 12)])[0].rounds == 4
