"""USLAM::PnPsolver for relocalisation on the device (csrc/pnpsolver.hip) against the host build of the same source
(tests/emu/pnpsolver_emu.cpp, which walks iterate() solver by solver as the reference writes it), BIT FOR BIT: subsets, every
hypothesis pose and count through the test tap, masks, Tcw, nInliers, bNoMore, mnIterations and the generator state handed back --
and against the numpy model layer by layer (tests/pnpsolver_checks.py).  The shapes are the smallest at which the call can still go
wrong: the thresholds of iterate()'s loop, a return at the first and at the last hypothesis of a solver in the middle of the list,
re-entry, exhaustion, a mask longer than four ballot words, both capacity edges."""
import numpy as np
import pytest

import pnp_model as pm
import pnpsolver_checks as pc
import pnpsolver_model as psm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def emu():
    return pc.Emu()


@pytest.fixture(scope="module")
def klt(uvo):
    k = uvo.KLT(64, 64, max_points=16)
    yield k
    k.close()


def both(uvo, emu, klt, cands, calls, params=None, max_solvers=None, max_points=None, what=""):
    """The session on the device and on the host build, held to each other bit for bit and to the model; -> the device's session."""
    S = max_solvers or len(cands)
    N = max_points or max(max(len(c[0]) for c in cands), 4)
    dev, host = uvo.PnPsolverSet(klt, S, N), emu.make_set(uvo, S, N)
    try:
        a = pc.run_session(uvo, dev, cands, calls, params)
        b = pc.run_session(uvo, host, cands, calls, params)
    finally:
        dev.close()
        host.close()
    pc.assert_sessions_equal(a, b, what)
    worst = pc.check_session_against_model(uvo, emu, a, cands, params, what=what)
    assert worst is None or worst <= pm.REFIT_TOL, (what, worst)
    return a


def advanced(uvo, draws, seed=1):
    g = uvo.GlibcRand(seed)
    for _ in range(draws):
        g.next()
    return g.state()


def test_nine_points_no_more_and_nothing_drawn(uvo, emu, klt):
    s = both(uvo, emu, klt, [psm.candidate(1, 9, 1.0)], [([0], 5)])
    r = s[0].result
    assert (r.returned, r.draws, r.status.tolist()) == (-1, 0, [[1, 1, 0]]) and s[0].rng_state == advanced(uvo, 0)


def test_ten_points_five_iterations_although_max_its_is_one(uvo, emu, klt):
    s = both(uvo, emu, klt, [psm.candidate(2, 10, 0.5)], [([0], 5), ([0], 5)])
    assert s[0].infos[0][:3] == (10, 10, 1)
    assert s[0].result.status.tolist() == [[1, 1, 5]] and s[0].result.draws == 20
    assert s[1].result.status.tolist() == [[1, 1, 10]] and s[1].rng_state == advanced(uvo, 40)      # exhausted, called again: five more


def test_three_solvers_none_returning(uvo, emu, klt):
    cands = [psm.candidate(21, 15, 0.2), psm.candidate(22, 20, 0.2), psm.candidate(23, 64, 0.2)]
    s = both(uvo, emu, klt, cands, [([0, 1, 2], 5), ([0, 1, 2], 5)])
    r = s[0].result
    assert r.returned == -1 and r.status.tolist() == [[1, 1, 14], [1, 1, 35], [1, 1, 35]]
    assert r.draws == 4 * (14 + 35 + 35) and s[0].rng_state == advanced(uvo, 4 * (14 + 35 + 35))
    assert s[1].result.status.tolist() == [[1, 1, 19], [1, 1, 40], [1, 1, 40]] and s[1].rng_state == advanced(uvo, 4 * (14 + 35 + 35 + 15))


@pytest.mark.parametrize("seed,at", [(5000, 1), (5274, 35)], ids=("at_its_first_hypothesis", "at_its_last_hypothesis"))
def test_second_of_three_returns(uvo, emu, klt, seed, at):
    cands = [psm.candidate(11, 15, 0.2), psm.candidate(seed, 20, 0.6, 0.5), psm.candidate(13, 64, 0.7)]
    s = both(uvo, emu, klt, cands, [([0, 1, 2], 5), ([2], 5), ([1, 0], 5)], what="second returns")
    r = s[0].result
    assert (r.returned, r.solver, r.refined) == (1, 1, 1)
    assert r.status.tolist() == [[1, 1, 14], [1, 0, at], [0, 0, 0]]                 # the third is untouched
    assert r.draws == 4 * (14 + at) and s[0].rng_state == advanced(uvo, 4 * (14 + at))             # the state is cut at the second
    assert len(s[0].taps[2][2]) == 0 and s[0].infos[2][3:] == (0, 0)
    # a following call starting at the third continues the stream (held to the host build and the model by both())
    assert s[1].result.status[0][0] == 1 and s[1].infos[0][3] > 0
    # re-entry on the solver that returned: again, at its first hypothesis with count >= nMinInliers; where the remaining iterations
    # bring none, the call ends in exhaustion and hands back the unrefined best
    r2, cnt = s[2].result, s[2].taps[0][2]
    hits = np.flatnonzero(cnt >= 10)
    assert r2.returned == 0 and r2.solver == 1 and s[2].result.status[1].tolist() == [0, 0, 14]
    if len(hits):
        assert r2.refined == 1 and len(cnt) == 1 + int(hits[0])
        if s[2].infos[0][4] == s[0].infos[1][4]:                                                   # the best set unchanged: the same refit
            assert r2.Tcw.tobytes() == r.Tcw.tobytes() and r2.n_inliers == r.n_inliers
    else:
        assert r2.refined == 0 and s[2].result.status[0].tolist() == [1, 1, 35] and r2.n_inliers == s[2].infos[0][4]
    assert len(hits) > 0 or at == 1                                                                # the second variant does re-enter


def test_min_set_five_and_a_mask_longer_than_four_words(uvo, emu, klt):
    prm = uvo.PnPsolverParams(0.99, 10, 300, 5, 0.5, 7.815)
    cands = [psm.candidate(31, 300, 0.7, 0.5, n_matches=517)]
    s = both(uvo, emu, klt, cands, [([0], 5), ([0], 5)], prm)
    r = s[0].result
    assert r.returned == 0 and r.refined == 1 and r.n_inliers > 150 and len(r.inliers) == 517
    assert r.draws == 5 * len(s[0].taps[0][2]) and s[0].taps[0][0].shape[1] == 5
    assert pm.pose_deviation(r.Tcw[:3, :3], r.Tcw[:3, 3], cands[0][6], cands[0][7]) < 1e-2


def test_capacity_edges(uvo, emu, klt):
    # max_solvers solvers at once, one of them with N = max_points (no multiple of 64)
    cands = [psm.candidate(70 + j, n, ratio) for j, (n, ratio) in enumerate([(70, 0.3), (15, 0.2), (9, 1.0), (33, 0.2), (64, 0.2), (20, 0.2), (10, 0.3), (70, 0.8)])]
    s = both(uvo, emu, klt, cands, [(list(range(8)), 5), (list(range(8))[::-1], 5)], max_solvers=8, max_points=70)
    assert s[0].result.solver == 7 and s[0].result.status[:, 0].all()
    pset = uvo.PnPsolverSet(klt, 2, 70)
    try:
        p3d, p2d, sigma2, kp, nm, K, _, _ = psm.candidate(1, 71, 0.5)
        with pytest.raises(uvo.UvoError) as ei:
            pset.add(p3d, p2d, sigma2, kp, nm, K)                                                   # more points than max_points
        assert ei.value.code == uvo.UVO_E_BADARG
        p3d, p2d, sigma2, kp, nm, K, _, _ = psm.candidate(1, 20, 0.5)
        for bad in (dict(min_set=3), dict(min_set=9), dict(probability=float("nan")), dict(epsilon=float("nan")), dict(th2=float("nan"))):
            with pytest.raises(uvo.UvoError) as ei:
                pset.add(p3d, p2d, sigma2, kp, nm, K, uvo.PnPsolverParams(**bad))
            assert ei.value.code == uvo.UVO_E_BADARG, bad
        a, b = pset.add(p3d, p2d, sigma2, kp, nm, K), pset.add(p3d, p2d, sigma2, kp, nm, K)
        with pytest.raises(uvo.UvoError) as ei:
            pset.add(p3d, p2d, sigma2, kp, nm, K)                                                   # the set is full
        assert ei.value.code == uvo.UVO_E_BADARG
        g = uvo.GlibcRand(1)
        with pytest.raises(uvo.UvoError):
            pset.iterate([a, a], 5, g)                                                              # one solver twice in a call
        with pytest.raises(uvo.UvoError):
            pset.iterate([a, 5], 5, g)
        assert g.state() == advanced(uvo, 0)
        assert pset.iterate([a, b], 5, g).returned in (-1, 0, 1)
    finally:
        pset.close()


@pytest.mark.parametrize("S,N", [(0, 10), (65, 10), (1, 3), (1, 16385)])
def test_a_set_outside_1_to_64_solvers_of_4_to_16384_points_is_refused(uvo, klt, S, N):
    with pytest.raises(uvo.UvoError) as ei:
        uvo.PnPsolverSet(klt, S, N)
    assert ei.value.code == uvo.UVO_E_BADARG and "1..64 solvers of 4..16384 points" in str(ei.value)


def one_call(uvo, pset, ids, n_iterations, g):
    """One iterate call with everything a session records of it."""
    res = pset.iterate(ids, n_iterations, g)
    infos = [pset.query(i) for i in ids]
    return pc.Call(list(ids), n_iterations, res, g.state(), [pset.hypotheses(i) for i in ids],
                   [(f.n, f.min_inliers, f.max_its, f.iterations, f.best_inliers) for f in infos])


def test_refused_iterate_calls_leave_the_generator_the_solvers_and_the_next_call_alone(uvo, klt):
    """No iterations, a mask shorter than n_matches, more hypotheses than the set has slots (max(mRansacMaxIts, 321) > 320 per solver: at
    the only solver of a (1, 70) set, and at the second of a (2, 70) set, when the first's records are written already): each is
    refused with its code and text, the caller's generator and mnIterations stay, and the call that follows equals, field for field,
    tap for tap and in generator state, the same call on a set that saw none of them."""
    p3d, p2d, sigma2, kp, nm, K, _, _ = psm.candidate(1, 20, 0.5)
    pset, fresh, single = uvo.PnPsolverSet(klt, 2, 70), uvo.PnPsolverSet(klt, 2, 70), uvo.PnPsolverSet(klt, 1, 70)
    try:
        for p in (pset, fresh):
            a, b = p.add(p3d, p2d, sigma2, kp, nm, K), p.add(p3d, p2d, sigma2, kp, nm, K)
        assert single.add(p3d, p2d, sigma2, kp, nm, K) == a
        g = uvo.GlibcRand(1)
        slots = "more hypothesis slots than the set has (320 per solver)"
        for p, ids, n_it, kw, code, text in ((pset, [a], 0, {}, uvo.UVO_E_BADARG, "n_iterations must be at least 1"),
                                             (pset, [a], 5, dict(inliers_cap=nm - 1), uvo.UVO_E_CAPACITY, "inliers_cap is smaller"),
                                             (single, [a], 321, {}, uvo.UVO_E_BADARG, slots),
                                             (pset, [a, b], 321, {}, uvo.UVO_E_BADARG, slots)):
            with pytest.raises(uvo.UvoError) as ei:
                p.iterate(ids, n_it, g, **kw)
            assert ei.value.code == code and text in str(ei.value), (ids, n_it, kw, str(ei.value))
            assert g.state() == advanced(uvo, 0) and p.query(a).iterations == 0, (ids, n_it, kw)
            assert all(len(p.hypotheses(i)[2]) == 0 for i in ids), (ids, n_it, kw)
        x, y = one_call(uvo, pset, [a, b], 5, g), one_call(uvo, fresh, [a, b], 5, uvo.GlibcRand(1))
        pc.assert_sessions_equal([x], [y], "after the refused calls")
        assert x.result.status[0].tolist()[:1] == [1] and x.infos[0][3] > 0 and x.rng_state == advanced(uvo, x.result.draws)
    finally:
        for p in (pset, fresh, single):
            p.close()


def test_a_set_filled_to_capacity_equals_one_with_room_to_spare(uvo, emu, klt):
    """Both solvers of a (2, 65) set hold 65 points -- the last element of every array of the set's block is written and read, the inlier
    set spans two 64-bit words -- and the session equals, bit for bit, the one on an (8, 256) set, where every array lies elsewhere."""
    cands = [psm.candidate(301, 65, 0.2), psm.candidate(302, 65, 0.8, 0.5, n_matches=65)]
    calls = [([0, 1], 5), ([1, 0], 5)]
    tight = both(uvo, emu, klt, cands, calls, what="(2, 65)")
    roomy = both(uvo, emu, klt, cands, calls, max_solvers=8, max_points=256, what="(8, 256)")
    pc.assert_sessions_equal(tight, roomy, "(2, 65) against (8, 256)")
    r = tight[0].result
    assert (r.returned, r.solver) == (1, 1) and r.status[0].tolist() == [1, 1, 35] and len(r.inliers) == 65
    assert r.inliers[cands[1][3][64]] == 1                                                          # bit 0 of the second word


def test_find_is_iterate_of_max_its(uvo, emu, klt):
    cands = [psm.candidate(90, 40, 0.75)]
    dev, host = uvo.PnPsolverSet(klt, 1, 40), emu.make_set(uvo, 1, 40)
    try:
        out = []
        for pset in (dev, host):
            sid = pset.add(*cands[0][:6])
            g = uvo.GlibcRand(1)
            r = pset.find(sid, g)
            out.append((r.returned, r.n_inliers, r.refined, r.Tcw.tobytes(), r.inliers.tobytes(), g.state(), pset.query(sid).iterations))
        assert out[0] == out[1] and out[0][0] == 0 and out[0][6] <= 35
    finally:
        dev.close()
        host.close()
