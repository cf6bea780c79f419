"""USLAM::PnPsolver for relocalisation without a GPU: the host build of csrc/pnpsolver_core.hpp (tests/emu/pnpsolver_emu.cpp, the source
the kernels of csrc/pnpsolver.hip run) against the numpy model written from the reference's source (tests/pnpsolver_model.py), layer
by layer as DESIGN.md section 4 states the contract: exact for the generator, the subsets, the derived parameters, CheckInliers of a given
pose (up to the model's threshold margin) and the replay; the refined pose against an independent EPnP within pnp_model.REFIT_TOL."""
import ctypes
import ctypes.util

import numpy as np
import pytest

import pnp_model as pm
import pnpsolver_checks as pc
import pnpsolver_model as psm

SEEDS = (0, 1, 2, 12345, 2 ** 31 - 1)


@pytest.fixture(scope="module")
def emu():
    return pc.Emu()


def test_new_symbols_are_declared_and_exported(uvo):
    names = ("uvo_glibc_srand", "uvo_glibc_rand_next", "uvo_pnpsolver_set_create", "uvo_pnpsolver_set_destroy", "uvo_pnpsolver_set_clear",
             "uvo_pnpsolver_add", "uvo_pnpsolver_query", "uvo_pnpsolver_iterate", "uvo_pnpsolver_hypotheses")
    lib = ctypes.CDLL(uvo.LIB_PATH)
    for n in names:
        assert n in uvo.ABI_SYMBOLS and hasattr(lib, n), n
    assert ctypes.sizeof(uvo.GlibcRand) == 35 * 4 and ctypes.sizeof(uvo.PnPsolverParams) == 32 and ctypes.sizeof(uvo.PnPsolverResultC) == 112


def _libc_rand(seed, count):
    name = ctypes.util.find_library("c")
    libc = ctypes.CDLL(name) if name else None
    if libc is None or not hasattr(libc, "gnu_get_libc_version"):
        pytest.skip("this machine's libc is not glibc: there is no srand / rand to compare the restated generator with")
    libc.srand.argtypes, libc.rand.restype = [ctypes.c_uint], ctypes.c_int
    libc.srand(seed)
    return np.array([libc.rand() for _ in range(count)], np.int64)


@pytest.mark.parametrize("seed", SEEDS)
def test_generator_equals_this_machines_rand(uvo, emu, seed):
    want = _libc_rand(seed, 2000)
    g = psm.GlibcRand(seed)
    np.testing.assert_array_equal([g.next() for _ in range(2000)], want, err_msg="the model")
    np.testing.assert_array_equal(emu.rand(seed, 2000), want, err_msg="the host build")
    lg = uvo.GlibcRand(seed)        # the library's own entry points (host code: no device needed)
    np.testing.assert_array_equal([lg.next() for _ in range(2000)], want, err_msg="uvo_glibc_rand_next")


def test_seed_zero_is_seed_one(emu):
    np.testing.assert_array_equal(emu.rand(0, 100), emu.rand(1, 100))


@pytest.mark.parametrize("n", (4, 5, 8, 15, 40, 200))
def test_subsets_equal_the_model_repeated_points_included(emu, n):
    got = emu.subsets(1, n, 4, 3000)
    g, gi = psm.GlibcRand(1), psm.GlibcRand(1)
    want = np.array([psm.draw_subset(g, n, 4) for _ in range(3000)], np.int32)
    intended = np.array([psm.draw_subset_intended(gi, n, 4) for _ in range(3000)], np.int32)
    np.testing.assert_array_equal(got, want)
    assert got.min() >= 0 and got.max() < n
    repeats = np.array([len(set(r)) < 4 for r in got])
    print("N = %d: %d of 3000 sets repeat a point" % (n, int(repeats.sum())))
    if n == 8:
        assert repeats.sum() > 0
    # the draw as written differs from the draw as meant exactly where it repeats a point
    np.testing.assert_array_equal((got != intended).any(1), repeats)
    assert all(len(set(r)) == 4 for r in intended)


@pytest.mark.parametrize("min_set", (5, 8))
def test_subsets_for_larger_minimal_sets(emu, min_set):
    for n in (8, 9, 33):
        g = psm.GlibcRand(1)
        want = np.array([psm.draw_subset(g, n, min_set) for _ in range(500)], np.int32)
        np.testing.assert_array_equal(emu.subsets(1, n, min_set, 500), want)


def test_derived_parameters(uvo, emu):
    for n, want in psm.CALL_SITE_TABLE.items():
        assert psm.derive_params(n, **psm.CALL_SITE) == want, n
        assert emu.derive(n, uvo.PnPsolverParams()) == want, n
    sets = (psm.CALL_SITE, dict(probability=0.99, min_inliers=6, max_iterations=300, min_set=5, epsilon=0.3, th2=7.815),
            dict(probability=0.999, min_inliers=20, max_iterations=50, min_set=8, epsilon=0.1, th2=5.991))
    for prm in sets:
        for n in range(4, 1201):
            assert emu.derive(n, uvo.PnPsolverParams(**prm)) == psm.derive_params(n, **prm), (prm, n)


def _replay_both(emu, it0, best0, counts, script, carried, n_it, max_its, min_inl):
    pad = [0] * (max_its + n_it + 8)
    m = psm.replay(it0, best0, list(counts) + pad, list(script) + pad, carried, n_it, max_its, min_inl)
    e = emu.replay(it0, best0, list(counts) + pad, list(script) + pad, carried, n_it, max_its, min_inl)
    for key in ("performed", "returned", "no_more", "inliers", "iterations", "best"):
        assert m[key] == e[key], (key, m, e)
    assert emu.L.emu_pnps_iterations_ahead(it0, max_its, n_it) == psm.iterations_ahead(it0, max_its, n_it) >= m["performed"]
    return m


def test_replay_named_cases(emu):
    R = lambda *a: _replay_both(emu, *a)
    # N = 10: mRansacMaxIts is 1, yet iterate(5) runs five iterations -- the loop condition is an OR
    m = R(0, 0, [0] * 5, [0] * 5, 0, 5, 1, 10)
    assert (m["performed"], m["no_more"], m["returned"], m["iterations"]) == (5, 1, psm.NONE, 5)
    # a second and a third call on the exhausted solver: five more each
    m = R(5, 0, [0] * 5, [0] * 5, 0, 5, 1, 10)
    assert (m["performed"], m["iterations"], m["no_more"]) == (5, 10, 1)
    m = R(10, 0, [0] * 5, [0] * 5, 0, 5, 1, 10)
    assert (m["performed"], m["iterations"]) == (5, 15)
    # the first call runs max(mRansacMaxIts, 5)
    assert R(0, 0, [0] * 35, [0] * 35, 0, 5, 35, 10)["performed"] == 35
    assert R(33, 0, [0] * 35, [0] * 35, 0, 5, 35, 10)["performed"] == 5
    # early return at the third hypothesis, then re-entry: the first hypothesis with count >= nMinInliers returns again on the carried set
    m = R(0, 0, [3, 9, 14, 30], [0, 0, 13, 0], 0, 5, 35, 10)
    assert (m["performed"], m["returned"], m["inliers"], m["best"], m["no_more"]) == (3, psm.REFINED, 13, 14, 0)
    m = R(3, 14, [2, 9, 11, 30], [0, 0, 0, 0], 13, 5, 35, 10)
    assert (m["performed"], m["returned"], m["inliers"], m["best"]) == (3, psm.REFINED, 13, 14)
    # equal counts: no new best, Refine still consulted (on the old set, whose outcome it repeats)
    m = R(0, 0, [12, 12, 12, 0, 0], [10, 99, 99, 0, 0], 0, 5, 1, 10)
    assert (m["returned"], m["best_from"], m["refines"], m["performed"]) == (psm.BEST_AT_EXHAUSTION, 0, 3, 5)
    # refined count == nMinInliers fails: strict
    assert R(0, 0, [12] + [0] * 4, [10] + [0] * 4, 0, 5, 5, 10)["returned"] == psm.BEST_AT_EXHAUSTION
    assert R(0, 0, [12] + [0] * 4, [11] + [0] * 4, 0, 5, 5, 10)["returned"] == psm.REFINED
    # count == nMinInliers qualifies (>=)
    assert R(0, 0, [10] + [0] * 4, [11] + [0] * 4, 0, 5, 5, 10)["returned"] == psm.REFINED
    assert R(0, 0, [9] + [0] * 4, [11] + [0] * 4, 0, 5, 5, 10)["returned"] == psm.NONE
    # exhaustion with a best: the unrefined best comes back; without: nothing
    m = R(0, 0, [0, 11, 0, 15, 0], [0, 4, 0, 10, 0], 0, 5, 5, 10)
    assert (m["returned"], m["inliers"], m["no_more"]) == (psm.BEST_AT_EXHAUSTION, 15, 1)
    m = R(0, 0, [0, 9, 0, 5, 0], [0] * 5, 0, 5, 5, 10)
    assert (m["returned"], m["inliers"], m["no_more"]) == (psm.NONE, 0, 1)


def test_replay_equals_the_model_on_random_sequences(emu):
    rng = np.random.default_rng(5)
    seen = set()
    for _ in range(400):
        min_inl = int(rng.integers(4, 30))
        max_its = int(rng.integers(1, 40))
        n_it = int(rng.integers(1, 12))
        it0 = int(rng.integers(0, max_its + 10))
        best0 = int(rng.choice([0, 0, min_inl, min_inl + 3]))
        K = psm.iterations_ahead(it0, max_its, n_it)
        counts = rng.integers(0, min_inl + 8, K) * (rng.random(K) < 0.4)
        script = rng.integers(min_inl - 2, min_inl + 3, K)
        carried = int(rng.integers(min_inl - 2, min_inl + 2)) if best0 else 0
        m = _replay_both(emu, it0, best0, counts, script, carried, n_it, max_its, min_inl)
        seen.add((m["returned"], m["performed"] == K))
    assert {(psm.NONE, True), (psm.REFINED, False), (psm.BEST_AT_EXHAUSTION, True)} <= seen


def test_check_inliers_within_the_threshold_margin(emu):
    total_near = 0
    for seed in range(6):
        p3d, p2d, sigma2, kp, nm, K, R, t = psm.candidate(400 + seed, 300, 0.6, 2.0)
        me = psm.max_error(sigma2, 5.991)
        rng = np.random.default_rng(seed)
        for _ in range(4):
            pose = np.concatenate([R.reshape(9), t + rng.normal(size=3) * 0.01])
            _, inl, near = psm.check_inliers(pose, p3d, p2d, K, me)
            got = emu.check_inliers(pose, p3d, p2d, me, K)
            assert ((got == inl) | near).all(), (seed, np.flatnonzero((got != inl) & ~near))
            assert 20 < got.sum() < 300
            total_near += int(near.sum())
    # a NaN pose counts nothing, and so does a pose that puts points on the camera plane
    bad = np.full(12, np.nan)
    assert not emu.check_inliers(bad, p3d, p2d, me, K).any() and not psm.check_inliers(bad, p3d, p2d, K, me)[1].any()
    assert not emu.check_inliers(np.zeros(12), p3d, p2d, me, K).any()


RUN_N = (10, 15, 20, 64, 300)
RUN_RATIO = (0.3, 0.5, 0.7, 0.95)


def _candidates(base, n, k=8):
    return [psm.candidate(base + 13 * j, n, RUN_RATIO[j % 4], 0.5, n_matches=n + (j % 3) * 7) for j in range(k)]


@pytest.mark.parametrize("n", RUN_N)
def test_whole_runs_hold_every_layer(uvo, emu, n):
    cands = _candidates(1000 + n, n)
    ids = list(range(8))
    calls = [(ids, 5), (ids, 5), (ids[::-1], 5), ([3, 1], 7), (ids, 5)]
    pset = emu.make_set(uvo, 8, max(n, 16))
    session = pc.run_session(uvo, pset, cands, calls)
    pset.close()
    worst = pc.check_session_against_model(uvo, emu, session, cands, what="N=%d" % n)
    returned = [c.result.returned >= 0 for c in session]
    print("N = %d: returned per call %s, worst refit deviation %s" % (n, returned, worst))
    if n >= 20:
        assert any(c.result.refined for c in session) and worst is not None
    if worst is not None:
        assert worst <= pm.REFIT_TOL, worst


def test_mixed_sizes_and_a_second_parameter_set(uvo, emu):
    cands = [psm.candidate(77, 9, 0.9), psm.candidate(78, 300, 0.6, 0.5, n_matches=450), psm.candidate(79, 33, 0.2), psm.candidate(80, 64, 0.8)]
    prm = uvo.PnPsolverParams(0.99, 10, 300, 5, 0.3, 7.815)
    pset = emu.make_set(uvo, 4, 300)
    session = pc.run_session(uvo, pset, cands, [([0, 2, 1, 3], 5), ([2, 3], 5), ([0, 1, 2, 3], 40)], prm)
    pset.close()
    worst = pc.check_session_against_model(uvo, emu, session, cands, prm, what="mixed")
    assert worst is not None and worst <= pm.REFIT_TOL, worst
    assert session[0].result.solver == 1


def test_degenerate_inputs_leave_no_nan(uvo, emu):
    p3d, p2d, sigma2, kp, nm, K, _, _ = psm.candidate(5, 40, 0.9)
    same = (np.tile(p3d[:1], (40, 1)), np.tile(p2d[:1], (40, 1)), sigma2, kp, nm, K, None, None)
    flat = p3d.copy()
    flat[:, 2] = 3.0
    plane = (flat, p2d, sigma2, kp, nm, K, None, None)
    dup = (np.repeat(p3d[:5], 8, 0), np.repeat(p2d[:5], 8, 0), sigma2, kp, nm, K, None, None)     # every minimal set repeats a point
    small = psm.candidate(6, 10, 1.0)                                                              # N = 10: sets of 4 out of 10 repeat often
    cands = [same, plane, dup, small]
    pset = emu.make_set(uvo, 4, 64)
    session = pc.run_session(uvo, pset, cands, [([0, 1, 2, 3], 5), ([0, 1, 2, 3], 5)])
    pset.close()
    for c in session:
        assert np.isfinite(c.result.Tcw).all()
        for sub, poses, cnt in c.taps:
            assert np.isfinite(poses).all() and (cnt >= 0).all()
    pc.check_session_against_model(uvo, emu, session, cands, what="degenerate")
