"""USLAM::Sim3Solver for loop closing without a GPU: the host build of csrc/sim3_core.hpp (tests/emu/sim3solver_emu.cpp, the source the
kernels of csrc/sim3solver.hip run) against the numpy model written from the reference's source (tests/sim3_model.py), layer by layer
as DESIGN.md section 4 states the contract: exact for the generator, the subsets, the derived parameters, the thresholds and the replay;
every hypothesis transform within 2 float ulp of the model's and within the Horn tolerance of an independent double-precision Horn;
CheckInliers up to the model's threshold margin.  Four seeded mutations of the host build have to fail these same checks."""
import ctypes
import math

import numpy as np
import pytest

import sim3_checks as sc
import sim3_model as sm


@pytest.fixture(scope="module")
def emu():
    return sc.Emu()


def test_new_symbols_are_declared_and_exported(uvo):
    names = ("uvo_sim3solver_set_create", "uvo_sim3solver_set_destroy", "uvo_sim3solver_set_clear", "uvo_sim3solver_add",
             "uvo_sim3solver_set_ransac_parameters", "uvo_sim3solver_query", "uvo_sim3solver_iterate", "uvo_sim3solver_find", "uvo_sim3solver_hypotheses")
    lib = ctypes.CDLL(uvo.LIB_PATH)
    for n in names:
        assert n in uvo.ABI_SYMBOLS and hasattr(lib, n), n
    assert ctypes.sizeof(uvo.Sim3SolverParams) == 16 and ctypes.sizeof(uvo.Sim3KeyFrame) == 64 and ctypes.sizeof(uvo.Sim3SolverInfo) == 16
    assert ctypes.sizeof(uvo.Sim3SolverResultC) == 160


# ---- layers 1 and 2 ------------------------------------------------------------------------------------------------------------------
def test_subsets_equal_the_model_repeated_points_included(emu):
    sc.check_subsets(emu)


def test_derived_parameters_and_thresholds(uvo, emu):
    sc.check_tables(uvo, emu)


def test_constructor_work_equals_the_model(uvo, emu):
    for seed, n in ((1, 3), (2, 64), (3, 300)):
        c = sm.candidate(seed, n, 0.7)
        for kf, xw in ((c[6], c[0]), (c[7], c[1])):
            xc, uv = emu.prepare(uvo, kf, xw)
            mxc, muv = sm.prepare(kf, xw)
            assert xc.tobytes() == mxc.tobytes() and uv.tobytes() == muv.tobytes(), (seed, n)


# ---- layer 3 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,n", [s for s in sm.HORN_SCENES if s[0] in (1, 3)])
def test_hypotheses_against_both_forms_of_the_model(emu, seed, n):
    x1c, x2c, triples = sm.horn_triples(seed, n, 150)
    worst, checked, not_finite = 0.0, 0, 0
    for t in triples:
        P1, P2 = x1c[t].T, x2c[t].T
        m = sm.compute_t(P1, P2)
        ok, e = emu.compute_t(x1c, x2c, t)
        assert ok == m["finite"], t
        if not ok:
            assert not any(e[k].any() for k in ("T12", "T21", "R", "t")) and e["s"] == 0
            not_finite += 1
            continue
        for name in ("T12", "T21"):
            d = np.abs(e[name].astype(np.float64) - m[name].astype(np.float64))
            assert (d <= sc._row_bound(m[name])).all(), (name, t, e[name], m[name])
        assert e["T12"][:3, 3].tobytes() == e["t"].tobytes()
        if sm.well_conditioned(P1, P2, t):
            s64, R64, t64 = sm.horn64(P1, P2)
            dev = sm.sim3_deviation(e["s"], e["R"], e["t"], s64, R64, t64)
            assert dev <= sm.HORN_TOL, (t, dev)
            worst, checked = max(worst, dev), checked + 1
    print("seed %d N = %d: %d triples held to horn64, worst %.3e (tolerance %.3e), %d not finite" % (seed, n, checked, worst, sm.HORN_TOL, not_finite))
    assert checked >= 100


# ---- layer 4 -------------------------------------------------------------------------------------------------------------------------
def test_check_inliers_within_the_threshold_margin(uvo, emu):
    for seed in range(4):
        c = sm.candidate(400 + seed, 300, 0.6, 2.0)
        (x1c, p1), (x2c, p2) = sm.prepare(c[6], c[0]), sm.prepare(c[7], c[1])
        e1, e2 = sm.thresholds(c[2]), sm.thresholds(c[3])
        g = sm.GlibcRand(seed + 1)
        hit = 0
        for _ in range(12):
            t = sm.draw_subset(g, 300, 3)
            m = sm.compute_t(x1c[t].T, x2c[t].T)
            if not m["finite"]:
                continue
            _, _, inl, near = sm.check_inliers(m["T12"], m["T21"], x1c, x2c, p1, p2, c[6][2], c[7][2], e1, e2)
            got = emu.check_inliers(m["T12"], m["T21"], x1c, x2c, p1, p2, e1, e2, c[6][2], c[7][2])
            assert ((got == inl) | near).all(), (seed, np.flatnonzero((got != inl) & ~near))
            hit += int(got.sum() > 30)
        assert hit >= 1
    bad = np.full((4, 4), np.nan, np.float32)
    assert not emu.check_inliers(bad, bad, x1c, x2c, p1, p2, e1, e2, c[6][2], c[7][2]).any()
    assert not sm.check_inliers(bad, bad, x1c, x2c, p1, p2, c[6][2], c[7][2], e1, e2)[2].any()


# ---- layer 5 -------------------------------------------------------------------------------------------------------------------------
def _replay_both(emu, it0, best0, counts, n_it, max_its, min_inl):
    pad = [0] * (n_it + 8)
    m = sm.replay(it0, best0, list(counts) + pad, n_it, max_its, min_inl)
    e = emu.replay(it0, best0, list(counts) + pad, n_it, max_its, min_inl)
    for key in ("performed", "returned", "no_more", "inliers", "iterations", "best", "best_from"):
        assert m[key] == e[key], (key, m, e)
    assert emu.L.emu_sim3_iterations_ahead(it0, max_its, n_it) == sm.iterations_ahead(it0, max_its, n_it) >= m["performed"]
    return m


def test_replay_named_cases(emu):
    R = lambda *a: _replay_both(emu, *a)
    assert R(0, 0, [0] * 5, 5, 14, 2)["performed"] == 5                       # AND: five, not fourteen
    m = R(10, 0, [0] * 5, 5, 14, 2)
    assert (m["performed"], m["no_more"]) == (4, 1)
    assert R(14, 0, [], 5, 14, 2)["performed"] == 0
    assert R(0, 0, [0, 2, 2, 1, 0], 5, 14, 2)["best_from"] == 2               # a later tie wins
    assert R(0, 0, [2] * 5, 5, 14, 2)["returned"] == -1                       # the return is strict
    m = R(13, 0, [5], 5, 14, 2)
    assert (m["returned"], m["no_more"]) == (0, 0)                            # a return at the last iteration leaves bNoMore false
    assert R(1, 8, [8], 5, 293, 2)["returned"] == 0                           # re-entry: a tie with the best returns again


def test_replay_equals_the_model_on_random_sequences(emu):
    rng = np.random.default_rng(5)
    seen = set()
    for _ in range(400):
        min_inl = int(rng.integers(0, 12))
        max_its = int(rng.integers(1, 40))
        n_it = int(rng.integers(1, 12))
        it0 = int(rng.integers(0, max_its + 3))
        best0 = int(rng.choice([0, 0, min_inl, min_inl + 3]))
        counts = rng.integers(0, min_inl + 6, n_it) * (rng.random(n_it) < 0.5)
        m = _replay_both(emu, it0, best0, counts, n_it, max_its, min_inl)
        seen.add((m["returned"] >= 0, m["no_more"]))
    assert {(True, 0), (False, 0), (False, 1)} <= seen


RUN_N = (3, 4, 5, 8, 15, 64, 300)
RUN_RATIO = (0.3, 0.5, 0.7, 0.95)


def _candidates(base, n, k=8):
    return [sm.candidate(base + 13 * j, n, RUN_RATIO[j % 4], 0.5, n_matches=n + (j % 3) * 7) for j in range(k)]


@pytest.mark.parametrize("n", RUN_N)
def test_whole_runs_hold_every_layer(uvo, emu, n):
    cands = _candidates(1000 + n, n)
    ids = list(range(8))
    calls = [(ids, 5), (ids, 5), (ids[::-1], 5), ([3, 1], 7), ("set", 3, uvo.Sim3SolverParams(0.99, 6, 300)), (ids, 5), ([5], sc.FIND), (ids, 1)]
    sset = emu.make_set(uvo, 8, max(n, 16))
    session = sc.run_session(uvo, sset, cands, calls)
    sset.close()
    stats = sc.check_session_against_model(uvo, emu, session, cands, what="N=%d" % n)
    returned = [c.result.returned >= 0 for c in session if c.result is not None]
    print("N = %d: returned per call %s, %s" % (n, returned, stats))
    assert stats["hypotheses"] > 20
    if n >= 8:
        assert any(returned) and stats["horn_checked"] > 0


def test_header_default_parameters_and_reentry(uvo, emu):
    prm = uvo.Sim3SolverParams(**sm.HEADER_DEFAULT)
    cands = [sm.candidate(77, 6, 1.0, 0.0), sm.candidate(78, 5, 1.0, 0.0), sm.candidate(79, 15, 1.0, 0.0), sm.candidate(80, 64, 0.8)]
    sset = emu.make_set(uvo, 4, 64)
    session = sc.run_session(uvo, sset, cands, [([0, 1, 2, 3], 5), ([2, 3], 5), ([2], 5), ([0, 1, 2, 3], 40)], prm)
    sset.close()
    sc.check_session_against_model(uvo, emu, session, cands, prm, what="header default")
    r = session[0].result
    assert session[0].infos[0][:2] == (6, 1) and r.status[0].tolist() == [1, 1, 1]         # minInliers == N: one iteration, and 6 > 6 never returns
    assert r.status[1].tolist() == [1, 1, 0]                                               # N < minInliers: bNoMore, nothing drawn
    assert r.returned == 2 and r.status[3].tolist() == [0, 0, 0]
    # ComputeSim3 enters a solver again after OptimizeSim3 rejected its transform: the same solver returns again
    assert session[1].result.solver == 2 and session[2].result.solver == 2
    assert session[2].infos[0][2] > session[1].infos[0][2] > session[0].infos[2][2]


def test_set_ransac_parameters_zeroes_the_iterations_and_keeps_the_best(uvo, emu):
    cands = [sm.candidate(90, 8, 0.4, 0.5)]
    sset = emu.make_set(uvo, 1, 8)
    prm = uvo.Sim3SolverParams(0.99, 7, 300)
    calls = [([0], 5), ("set", 0, uvo.Sim3SolverParams(0.99, 7, 3)), ([0], 5), ([0], 5)]
    session = sc.run_session(uvo, sset, cands, calls, prm)
    sset.close()
    sc.check_session_against_model(uvo, emu, session, cands, prm, what="set again")
    best = session[0].infos[0][3]
    assert session[1].infos[0] == (8, 3, 0, best) and session[0].infos[0][2] == 5
    assert session[2].result.status.tolist() == [[1, 1, 3]] and session[3].result.status.tolist() == [[1, 1, 3]] and session[3].result.draws == 0


def test_max_iterations_is_bounded_by_the_slots_of_a_set(uvo, emu):
    c = sm.candidate(95, 20, 0.0)
    sset = emu.make_set(uvo, 1, 20)
    try:
        with pytest.raises(uvo.UvoError) as ei:
            sc.add_candidate(sset, c, uvo.Sim3SolverParams(0.99, 2, 321))
        assert ei.value.code == uvo.UVO_E_BADARG
        sid = sc.add_candidate(sset, c, uvo.Sim3SolverParams(0.99, 19, 320))
        with pytest.raises(uvo.UvoError):
            sset.set_ransac_parameters(sid, uvo.Sim3SolverParams(0.99, 2, 321))
        sset.set_ransac_parameters(sid, uvo.Sim3SolverParams(0.99, 2, 320))
        assert sset.query(sid).max_its == 320
    finally:
        sset.close()


# ---- layer 6 -------------------------------------------------------------------------------------------------------------------------
def test_sincos_and_atan2_against_libm(emu):
    rng = np.random.default_rng(11)
    edges = np.array([np.float32(k * math.pi / 4) for k in range(9)], np.float64)
    edges = np.concatenate([edges, np.nextafter(edges.astype(np.float32), np.float32(0)).astype(np.float64), [0.0, 2 * math.pi]])
    th = np.concatenate([rng.uniform(0, 2 * math.pi, 10 ** 6), edges[(edges >= 0) & (edges <= 2 * math.pi)]])
    s, c = emu.sincos(th)
    ws = np.array([math.sin(v) for v in th])
    wc = np.array([math.cos(v) for v in th])
    es, ec = np.abs(s - ws).max(), np.abs(c - wc).max()
    y = np.abs(rng.normal(size=10 ** 6)) * 10.0 ** rng.uniform(-6, 3, 10 ** 6)
    x = rng.normal(size=10 ** 6) * 10.0 ** rng.uniform(-6, 3, 10 ** 6)
    y = np.concatenate([y, [0.0, 1.0, 1.0, 0.0, 1.0, 3.0]])
    x = np.concatenate([x, [1.0, 0.0, 1.0, -1.0, -1.0, -3.0]])
    a = emu.atan2_pos(y, x)
    wa = np.array([math.atan2(p, q) for p, q in zip(y, x)])
    ea = np.abs(a - wa).max()
    print("largest absolute error against libm: sin %.3g, cos %.3g, atan2 %.3g (2^-50 = %.3g)" % (es, ec, ea, 2.0 ** -50))
    assert es <= 2.0 ** -50 and ec <= 2.0 ** -50 and ea <= 2.0 ** -50
    assert (a >= 0).all() and (a <= math.pi).all()
    assert np.isnan(emu.sincos(np.array([np.nan, np.inf]))[0]).all() and np.isnan(emu.atan2_pos(np.array([np.nan]), np.array([1.0]))).all()


def test_rotations_of_random_quaternions_equal_libms(emu):
    rng = np.random.default_rng(12)
    q = rng.normal(size=(10 ** 5, 4))
    q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    got = emu.rotation(q).reshape(-1, 3, 3)
    want = sm.rotations_from_quaternions(q)
    differ = got != want
    print("%d of %d float entries differ from the rotation built with libm" % (int(differ.sum()), differ.size))
    assert differ.sum() <= 10
    assert (np.abs(got[differ].astype(np.float64) - want[differ]) <= np.spacing(np.abs(want[differ]))).all()


# ---- layer 7 -------------------------------------------------------------------------------------------------------------------------
def test_degenerate_inputs_leave_no_nan(uvo, emu):
    x1w, x2w, sg1, sg2, index1, nm, kf1, kf2, _ = sm.candidate(5, 40, 0.9)
    same = (np.tile(x1w[:1], (40, 1)), np.tile(x2w[:1], (40, 1)), sg1, sg2, index1, nm, kf1, kf2)
    line1 = x1w[0] + np.outer(np.linspace(0, 1, 40), x1w[1] - x1w[0])
    line2 = x2w[0] + np.outer(np.linspace(0, 1, 40), x2w[1] - x2w[0])
    collinear = (line1.astype(np.float32), line2.astype(np.float32), sg1, sg2, index1, nm, kf1, kf2)
    dup = (np.repeat(x1w[:2], 20, 0), np.repeat(x2w[:2], 20, 0), sg1, sg2, index1, nm, kf1, kf2)      # every triple repeats a point
    depth0 = [a.copy() if isinstance(a, np.ndarray) else a for a in (x1w, x2w, sg1, sg2, index1, nm, kf1, kf2)]
    depth0[0][3] = (-kf1[1].astype(np.float64) @ kf1[0].astype(np.float64)).astype(np.float32)          # the first camera's centre: depth 0 there
    tiny = [tuple(a[:k] if isinstance(a, np.ndarray) else a for a in (x1w, x2w, sg1, sg2, index1)) + (nm, kf1, kf2) for k in (0, 1, 2)]
    cands = [same, collinear, dup, tuple(depth0)] + tiny + [sm.candidate(6, 3, 1.0)[:8]]
    sset = emu.make_set(uvo, 8, 64)
    ids = [4, 5, 6, 0, 1, 2, 7, 3]
    session = sc.run_session(uvo, sset, cands, [(ids, 5), (ids, 5), ([3], sc.FIND)])
    sset.close()
    for c in session:
        assert all(np.isfinite(getattr(c.result, k)).all() for k in ("T12", "R", "t", "s"))
        for sub, t12, t21, cnt in c.taps:
            assert np.isfinite(t12).all() and np.isfinite(t21).all() and (cnt >= 0).all()
    assert session[0].result.status[:3].tolist() == [[1, 1, 0]] * 3                                    # n = 0, 1, 2: never iterate
    sc.check_session_against_model(uvo, emu, session, cands, what="degenerate")


# ---- the checks can fail: four seeded mutations of the host build ----------------------------------------------------------------------
def _session(uvo, emu, cands, calls, params=None):
    sset = emu.make_set(uvo, len(cands), 64)
    try:
        return sc.run_session(uvo, sset, cands, calls, params)
    finally:
        sset.close()


REENTRY = ([sm.candidate(31, 8, 1.0, 0.0)], [([0], 5), ([0], 5), ([0], 5)])
SHORT = ([sm.candidate(32, 4, 0.5), sm.candidate(33, 15, 0.3)], [([0, 1], 5), ([1, 0], 5)])


def test_the_unmutated_build_passes_the_mutation_scenes(uvo, emu):
    for cands, calls in (REENTRY, SHORT):
        sc.check_session_against_model(uvo, emu, _session(uvo, emu, cands, calls), cands)
    assert all(c.result.returned == 0 for c in _session(uvo, emu, *REENTRY))        # a tie with the best returns again, call after call


def test_mutation_or_fails_the_replay(uvo):
    mut = sc.Emu("SIM3_MUT_OR")
    sc.check_tables(uvo, mut)
    sc.check_subsets(mut, ns=(4, 15), count=300)
    cands, calls = SHORT
    with pytest.raises(AssertionError, match="performed|solver"):
        sc.check_session_against_model(uvo, sc.Emu(), _session(uvo, mut, cands, calls), cands)


def test_mutation_gt_fails_the_replay_at_reentry(uvo):
    mut = sc.Emu("SIM3_MUT_GT")
    sc.check_tables(uvo, mut)
    sc.check_subsets(mut, ns=(4, 15), count=300)
    cands, calls = REENTRY
    session = _session(uvo, mut, cands, calls)
    assert session[0].result.returned == 0 and session[1].result.returned == -1
    with pytest.raises(AssertionError):
        sc.check_session_against_model(uvo, sc.Emu(), session, cands)
    sc.check_session_against_model(uvo, sc.Emu(), session[:1], cands)              # the first call alone is beyond reproach


def test_mutation_threshold_fails_the_tables(uvo):
    mut = sc.Emu("SIM3_MUT_THRESHOLD")
    sc.check_subsets(mut, ns=(4, 15), count=300)
    with pytest.raises(AssertionError):
        sc.check_tables(uvo, mut)


def test_mutation_draw_fails_the_subsets(uvo):
    mut = sc.Emu("SIM3_MUT_DRAW")
    sc.check_tables(uvo, mut)
    with pytest.raises(AssertionError):
        sc.check_subsets(mut)
    cands, calls = SHORT
    with pytest.raises(AssertionError, match="subsets"):
        sc.check_session_against_model(uvo, sc.Emu(), _session(uvo, mut, cands, calls), cands)
