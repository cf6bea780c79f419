"""USLAM::Sim3Solver for loop closing on the device (csrc/sim3solver.hip) against the host build of the same source
(tests/emu/sim3solver_emu.cpp, which walks iterate() solver by solver as the reference writes it), BIT FOR BIT: subsets, every
hypothesis T12 / T21 and count through the test tap, masks, T12, R, t, s, nInliers, bNoMore, mnIterations and the generator state handed
back -- and against the numpy model layer by layer (tests/sim3_checks.py, layers 1-5).  The shapes are the smallest at which the call
can still go wrong: the short iteration tables and repeating triples of N = 3..15, the edges of a wavefront in the scoring, one to
max_solvers solvers in a call, a return at the first and at the last planned hypothesis of a solver in the middle of the list, re-entry,
exhaustion, both capacity edges."""
import numpy as np
import pytest

import sim3_checks as sc
import sim3_model as sm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def emu():
    return sc.Emu()


@pytest.fixture(scope="module")
def matcher(uvo):
    m = uvo.ORBmatcher(0.8)
    yield m
    m.close()


def both(uvo, emu, matcher, cands, calls, params=None, max_solvers=None, max_points=None, what=""):
    """The session on the device and on the host build, held to each other bit for bit and to the model; -> the device's session."""
    S = max_solvers or len(cands)
    N = max_points or max(max(len(c[0]) for c in cands), 3)
    dev, host = uvo.Sim3SolverSet(matcher, S, N), emu.make_set(uvo, S, N)
    try:
        a = sc.run_session(uvo, dev, cands, calls, params)
        b = sc.run_session(uvo, host, cands, calls, params)
    finally:
        dev.close()
        host.close()
    sc.assert_sessions_equal(a, b, what)
    sc.check_session_against_model(uvo, emu, a, cands, params, what=what)
    return a


def advanced(uvo, draws, seed=1):
    g = uvo.GlibcRand(seed)
    for _ in range(draws):
        g.next()
    return g.state()


RATIO = (0.3, 0.5, 0.7, 0.95)


@pytest.mark.parametrize("n", (3, 4, 5, 8, 15, 63, 64, 65, 300))
def test_sizes_two_solvers_two_calls(uvo, emu, matcher, n):
    cands = [sm.candidate(2000 + n, n, 0.3, 0.5, n_matches=n + 9), sm.candidate(2100 + n, n, 0.9, 0.5)]
    s = both(uvo, emu, matcher, cands, [([0, 1], 5), ([1, 0], 5), ([0], 1)], what="N=%d" % n)
    assert s[0].infos[0][1] == sm.derive_params(n, **sm.CALL_SITE)


@pytest.mark.parametrize("k", (1, 8))
def test_solvers_in_one_call(uvo, emu, matcher, k):
    cands = [sm.candidate(2300 + j, (15, 8, 64, 5, 33, 4, 3, 20)[j], RATIO[j % 4] if k > 1 else 0.2) for j in range(k)]
    s = both(uvo, emu, matcher, cands, [(list(range(k)), 5), (list(range(k))[::-1], 5)], what="%d solvers" % k)
    assert s[0].result.status[0][0] == 1


def test_header_default_parameters_min_inliers_equal_and_above_n(uvo, emu, matcher):
    prm = uvo.Sim3SolverParams(**sm.HEADER_DEFAULT)
    cands = [sm.candidate(77, 6, 1.0, 0.0), sm.candidate(78, 5, 1.0, 0.0), sm.candidate(79, 15, 1.0, 0.0), sm.candidate(80, 64, 0.8)]
    s = both(uvo, emu, matcher, cands, [([0, 1, 2, 3], 5), ([2, 3], 5), ([2], 5), ([0, 1, 2, 3], 40)], prm, what="header default")
    r = s[0].result
    assert s[0].infos[0][:2] == (6, 1) and r.status[0].tolist() == [1, 1, 1]      # minInliers == N: one iteration
    assert r.status[1].tolist() == [1, 1, 0]                                      # N < minInliers: bNoMore, nothing drawn
    assert r.returned == 2 and r.status[3].tolist() == [0, 0, 0]                   # the fourth is untouched
    assert s[1].result.solver == 2 and s[2].result.solver == 2                    # re-entry: the same solver returns again


def test_nobody_returns_and_the_stream_continues(uvo, emu, matcher):
    prm = uvo.Sim3SolverParams(0.99, 14, 300)
    cands = [sm.candidate(21, 15, 0.2), sm.candidate(22, 20, 0.2), sm.candidate(23, 64, 0.2)]
    s = both(uvo, emu, matcher, cands, [([0, 1, 2], 5), ([0, 1, 2], 5)], prm)
    r = s[0].result
    assert s[0].infos[0][1] == sm.derive_params(15, 0.99, 14, 300) == 3                             # N = 15, minInliers 14: three iterations in all
    assert r.returned == -1 and r.status.tolist() == [[1, 1, 3], [1, 0, 5], [1, 0, 5]]
    assert r.draws == 3 * (3 + 5 + 5) and s[0].rng_state == advanced(uvo, 39)
    assert s[1].result.status.tolist() == [[1, 1, 3], [1, 0, 10], [1, 0, 10]] and s[1].rng_state == advanced(uvo, 39 + 30)


@pytest.mark.parametrize("at", (1, 5), ids=("at_its_first_hypothesis", "at_its_last_planned_hypothesis"))
def test_second_of_three_returns(uvo, emu, matcher, at):
    # the first solver has too few good points to return with minInliers = 5 and draws 3 * 5; the stream position of the second is
    # therefore 15, and its scene is searched for on the host build with the generator advanced that far
    prm = uvo.Sim3SolverParams(0.99, 5, 300)
    first = sm.candidate(11, 6, 0.0)
    second = None
    for seed in range(5000, 5600):
        c = sm.candidate(seed, 8, 0.8, 0.5)
        hs = emu.make_set(uvo, 2, 8)
        sc.add_candidate(hs, first, prm), sc.add_candidate(hs, c, prm)
        r = hs.iterate([0, 1], 5, uvo.GlibcRand(1))
        perf = len(hs.hypotheses(1)[3])
        hs.close()
        if r.returned == 1 and perf == at:
            second = c
            break
    assert second is not None
    cands = [first, second, sm.candidate(13, 64, 0.7)]
    s = both(uvo, emu, matcher, cands, [([0, 1, 2], 5), ([2], 5), ([1, 0], 5)], prm, what="second returns")
    r = s[0].result
    assert (r.returned, r.solver) == (1, 1)
    assert r.status.tolist() == [[1, 0, 5], [1, 0, at], [0, 0, 0]]                                 # the third is untouched
    assert r.draws == 3 * (5 + at) and s[0].rng_state == advanced(uvo, 3 * (5 + at))               # the state is cut at the second
    assert len(s[0].taps[2][3]) == 0 and s[0].infos[2][2:] == (0, 0)
    assert s[1].result.status[0][0] == 1 and s[1].infos[0][2] > 0
    assert s[2].result.status[0][0] == 1


def test_find_and_set_ransac_parameters(uvo, emu, matcher):
    cands = [sm.candidate(90, 8, 0.4, 0.5), sm.candidate(91, 40, 0.75)]
    prm = uvo.Sim3SolverParams(0.99, 7, 300)
    calls = [([0], 5), ("set", 0, uvo.Sim3SolverParams(0.99, 7, 3)), ([0], 5), ([0], 5), ([1], sc.FIND), ("set", 1, uvo.Sim3SolverParams()), ([1], sc.FIND)]
    s = both(uvo, emu, matcher, cands, calls, prm)
    assert s[1].infos[0][:3] == (8, 3, 0) and s[2].result.status.tolist() == [[1, 1, 3]] and s[3].result.draws == 0
    assert s[4].result.returned == 0 and s[6].result.returned == 0


def test_max_solvers_and_max_points_once(uvo, emu, matcher):
    cands = [sm.candidate(3000 + j, 3 + j % 6, 0.2) for j in range(63)] + [sm.candidate(3100, 16384, 0.9, 0.5, n_matches=16400)]
    ids = list(range(64))
    a = both(uvo, emu, matcher, cands, [(ids, 5)], uvo.Sim3SolverParams(0.99, 8, 300), max_solvers=64, max_points=16384, what="capacity")
    r = a[0].result
    assert r.solver == 63 and r.n_inliers > 5000 and len(r.inliers) == 16400 and r.status[:, 0].all()


def test_a_set_filled_to_capacity_equals_one_with_room_to_spare(uvo, emu, matcher):
    """Both solvers of a (2, 65) set hold 65 points -- the last element of every array of the set's block is written and read, the inlier
    set spans two 64-bit words -- and the session equals, bit for bit, the one on an (8, 256) set, where every array lies elsewhere."""
    cands = [sm.candidate(2065, 65, 0.3, 0.5, n_matches=74), sm.candidate(2166, 65, 0.9, 0.5)]
    calls = [([0, 1], 5), ([1, 0], 5), ([0], 1)]
    tight = both(uvo, emu, matcher, cands, calls, what="(2, 65)")
    roomy = both(uvo, emu, matcher, cands, calls, max_solvers=8, max_points=256, what="(8, 256)")
    sc.assert_sessions_equal(tight, roomy, "(2, 65) against (8, 256)")
    r = tight[0].result
    assert (r.returned, r.solver) == (1, 1) and r.inliers[cands[1][4][64]] == 1                    # bit 0 of the second word


def test_degenerate_inputs_leave_no_nan(uvo, emu, matcher):
    x1w, x2w, sg1, sg2, index1, nm, kf1, kf2, _ = sm.candidate(5, 40, 0.9)
    same = (np.tile(x1w[:1], (40, 1)), np.tile(x2w[:1], (40, 1)), sg1, sg2, index1, nm, kf1, kf2)
    line1 = x1w[0] + np.outer(np.linspace(0, 1, 40), x1w[1] - x1w[0])
    line2 = x2w[0] + np.outer(np.linspace(0, 1, 40), x2w[1] - x2w[0])
    collinear = (line1.astype(np.float32), line2.astype(np.float32), sg1, sg2, index1, nm, kf1, kf2)
    dup = (np.repeat(x1w[:2], 20, 0), np.repeat(x2w[:2], 20, 0), sg1, sg2, index1, nm, kf1, kf2)
    depth0 = [a.copy() if isinstance(a, np.ndarray) else a for a in (x1w, x2w, sg1, sg2, index1, nm, kf1, kf2)]
    depth0[0][3] = (-kf1[1].astype(np.float64) @ kf1[0].astype(np.float64)).astype(np.float32)
    tiny = [tuple(a[:k] if isinstance(a, np.ndarray) else a for a in (x1w, x2w, sg1, sg2, index1)) + (nm, kf1, kf2) for k in (0, 1, 2)]
    cands = [same, collinear, dup, tuple(depth0)] + tiny + [sm.candidate(6, 3, 1.0)[:8]]
    ids = [4, 5, 6, 0, 1, 2, 7, 3]
    s = both(uvo, emu, matcher, cands, [(ids, 5), (ids, 5), ([3], sc.FIND)], max_points=64, what="degenerate")
    for c in s:
        assert all(np.isfinite(getattr(c.result, k)).all() for k in ("T12", "R", "t", "s"))
        for sub, t12, t21, cnt in c.taps:
            assert np.isfinite(t12).all() and np.isfinite(t21).all() and (cnt >= 0).all()
    assert s[0].result.status[:3].tolist() == [[1, 1, 0]] * 3


def test_bad_arguments_and_capacity(uvo, matcher):
    sset = uvo.Sim3SolverSet(matcher, 2, 70)
    try:
        c = sm.candidate(1, 71, 0.5)
        with pytest.raises(uvo.UvoError) as ei:
            sc.add_candidate(sset, c, uvo.Sim3SolverParams())                                       # more points than max_points
        assert ei.value.code == uvo.UVO_E_BADARG
        c = sm.candidate(1, 20, 0.9, n_matches=50)
        for bad in (dict(probability=float("nan")), dict(probability=1.0), dict(min_inliers=-1), dict(max_iterations=0), dict(max_iterations=321)):
            with pytest.raises(uvo.UvoError) as ei:
                sc.add_candidate(sset, c, uvo.Sim3SolverParams(**bad))
            assert ei.value.code == uvo.UVO_E_BADARG, bad
        a, b = sc.add_candidate(sset, c, uvo.Sim3SolverParams()), sc.add_candidate(sset, c, uvo.Sim3SolverParams())
        with pytest.raises(uvo.UvoError) as ei:
            sc.add_candidate(sset, c, uvo.Sim3SolverParams())                                       # the set is full
        assert ei.value.code == uvo.UVO_E_BADARG
        with pytest.raises(uvo.UvoError) as ei:
            sset.set_ransac_parameters(a, uvo.Sim3SolverParams(max_iterations=321))         # more than the slots a set holds per solver
        assert ei.value.code == uvo.UVO_E_BADARG
        sset.set_ransac_parameters(a, uvo.Sim3SolverParams(max_iterations=320))
        assert sset.query(a).max_its == sm.derive_params(20, 0.99, 2, 320) == 320
        g = uvo.GlibcRand(1)
        for ids, n_it in (([a, a], 5), ([a, 5], 5), ([a], 0)):                                      # one solver twice, no such solver, no iterations
            with pytest.raises(uvo.UvoError) as ei:
                sset.iterate(ids, n_it, g)
            assert ei.value.code == uvo.UVO_E_BADARG
        with pytest.raises(uvo.UvoError) as ei:
            sset.iterate([a], 5, g, inliers_cap=49)                                                 # the mask is shorter than n_matches
        assert ei.value.code == uvo.UVO_E_CAPACITY
        assert g.state() == advanced(uvo, 0) and sset.query(a).iterations == 0                      # nothing of it ran
        assert sset.iterate([a, b], 5, g, inliers_cap=50).returned in (-1, 0, 1)
    finally:
        sset.close()
    for S, N in ((0, 10), (65, 10), (1, 2), (1, 16385)):
        with pytest.raises(uvo.UvoError) as ei:
            uvo.Sim3SolverSet(matcher, S, N)
        assert ei.value.code == uvo.UVO_E_BADARG


def test_one_iterate_call_is_at_most_three_launches(uvo, matcher):
    cands = [sm.candidate(40 + j, 64, 0.3) for j in range(4)]
    sset = uvo.Sim3SolverSet(matcher, 4, 64)
    try:
        for c in cands:
            sc.add_candidate(sset, c, uvo.Sim3SolverParams(0.99, 60, 300))
        matcher.profile(True)
        sset.iterate([0, 1, 2, 3], 5, uvo.GlibcRand(1))
        times = matcher.kernel_times()
        matcher.profile(False)
    finally:
        sset.close()
    assert set(times) == {"k_sim3_hypotheses", "k_sim3_score", "k_sim3_finish"}, times
    assert sum(v[1] for v in times.values()) == 3, times
