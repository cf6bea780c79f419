"""The order-dependent matcher loops on the device -- every copy of the parallel fixed point that stands in for the reference's sequential
loop -- against the sequential model of tests/resolve_model.py, the oracle and the closed forms, on scenes built to drive the iteration
deep: dominoes that need one sweep per query (up to 4097), piles TH_LOW + 1 deep, contention scenes with planted queues (at least 12).
tests/test_resolve_model.py proves those depths on the CPU and holds the model to the oracle.

Which test covers which copy:
  k_group_dist + k_match_resolve (csrc/match_engine.hip)     test_contention_*, test_domino_through_match_groups, test_pile_through_match_groups,
                                                             test_row_window_search, test_pile_search_by_bow, test_pile_search_for_triangulation
  k_match_resolve_steal (csrc/match_engine.hip)              test_steal_domino_through_match_groups, test_contention_* (init_steal),
                                                             test_row_search_for_initialization
  k_sbp_resolve (csrc/search.hip)                            test_row_search_by_projection
  k_create_new_map_points (csrc/triangulate.hip)             test_pile_create_new_map_points
  the host replay (csrc/matcher_batch.cpp)                   test_pile_search_for_triangulation (Batch + Next)

Every comparison is exact on match, dist and n_matches.  Outputs have nq + PAD rows prefilled with values no result can equal; the pad
must keep them."""
import ctypes

import numpy as np
import pytest

import resolve_model as rm
import triangulation_model as tm

pytestmark = pytest.mark.gpu

M_FILL, D_FILL, N_FILL, PAD = 0x5EADBEEF, 0x0BADF00D, -12345, 7
INT_MAX = 0x7fffffff


def _p(a):
    return None if a is None else a.ctypes.data


def _match_groups(uvo, m, s, rule, max_dist, exclusive, blocked=None, epi=None, ratio=rm.NN_RATIO, expect_rc=0, nt=None):
    """uvo_match_groups through the C entry point on scene s -> match[nq], dist[nq], n_matches.  tlevel goes in only where the rule
    reads it (the same-level rule, the epipolar predicate): everywhere else the NULL form is what runs."""
    start, idx = s.csr()
    nq, nt = s.nq, s.nt if nt is None else nt
    match, dist = np.full(nq + PAD, M_FILL, np.int32), np.full(nq + PAD, D_FILL, np.int32)
    nm = ctypes.c_int(N_FILL)
    r = uvo.MatchRule(rule, max_dist, ratio, exclusive, 0)
    keep, E = [], None
    if epi is not None:
        E = uvo.Epipolar()
        E.f12[:] = [float(x) for x in epi["f12"]]
        keep = [np.ascontiguousarray(epi[k], np.float32) for k in ("q_x", "q_y", "t_x", "t_y", "sigma2")]
        E.q_x, E.q_y, E.t_x, E.t_y, E.sigma2 = [a.ctypes.data for a in keep]
        E.nlevels = len(keep[4])
    tlevel = s.tlevel if (rule == rm.RULE_BEST_RATIO_SAME_LEVEL or epi is not None) else None
    bl = None if blocked is None else np.ascontiguousarray(blocked, np.uint8)
    rc = uvo.lib.uvo_match_groups(m._h, nq, _p(s.qdesc), None, nt, _p(s.tdesc), None, _p(tlevel), _p(bl), _p(start), _p(idx) if len(idx) else None,
                                  None if E is None else ctypes.byref(E), ctypes.byref(r), _p(match), _p(dist), ctypes.byref(nm))
    assert rc == expect_rc, "uvo_match_groups(%s, rule %d) returned %d: %s" % (s.name, rule, rc, uvo.last_error())
    assert (match[nq:] == M_FILL).all() and (dist[nq:] == D_FILL).all(), "%s: written past nq = %d" % (s.name, nq)
    return match[:nq], dist[:nq], nm.value


def _same(got, want, what):
    for g, w, name in zip(got, want, ("match", "dist", "n_matches")):
        np.testing.assert_array_equal(np.asarray(g, np.int64), np.asarray(w, np.int64), err_msg="%s: %s" % (what, name))


def _check(uvo, m, s, rule, max_dist, exclusive, blocked=None, epi=None, pred=None, ratio=rm.NN_RATIO):
    want = rm.resolve(rule, max_dist, ratio, exclusive, s.cand_lists, s.D, s.tlevel, pred, blocked)
    got = _match_groups(uvo, m, s, rule, max_dist, exclusive, blocked, epi, ratio)
    _same(got, want, "%s rule=%s max_dist=%d exclusive=%d blocked=%s epi=%s" % (s.name, rm.RULE_NAMES[rule], max_dist, exclusive,
                                                                                 blocked is not None, epi is not None))
    return want


# ---- a. uvo_match_groups against the model ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("nq", rm.GROUP_NQ)
@pytest.mark.parametrize("nt", rm.GROUP_NT)
def test_contention_grid(uvo, nq, nt):
    """Every rule at every launch shape: one query per thread, 1024 and 1025, two and three per thread; ownership tables in LDS (nt <= 4096)
    and in global memory; target indices up to the 16-bit limit."""
    s = rm.contention(nq, nt, rm.CONTENTION_SEED)
    epi, pred = rm.epipolar_third(s)
    m = uvo.ORBmatcher(rm.NN_RATIO, False)
    matched = 0
    for rule in rm.RULES:
        matched += _check(uvo, m, s, rule, 100, 1, s.blocked)[2]
    _check(uvo, m, s, rm.RULE_TRIANGULATION, 100, 1, s.blocked, epi, pred)
    m.close()
    if rm.deep_enough(nq, nt):
        assert matched > nq


@pytest.mark.parametrize("rule", rm.RULES, ids=rm.RULE_NAMES)
def test_contention_variants(uvo, rule):
    """exclusive 1 and 0, blocked given and NULL, max_dist 0, 50, 100 and 256; the triangulation rule with epi = NULL and with an
    epipolar predicate that fails for the targets with t % 3 == 2.  Without exclusivity every query gets the choice it makes alone
    (blocked targets still out of reach); the steal rule reads neither `exclusive` nor `tblocked`."""
    m = uvo.ORBmatcher(rm.NN_RATIO, False)
    for nq, nt, seed in rm.VARIANT_SCENES:
        s = rm.contention(nq, nt, seed)
        epis = [(None, None)] + ([rm.epipolar_third(s)] if rule == rm.RULE_TRIANGULATION else [])
        for epi, pred in epis:
            for exclusive in (1, 0):
                for blocked in (s.blocked, None):
                    for max_dist in rm.MAX_DISTS:
                        _check(uvo, m, s, rule, max_dist, exclusive, blocked, epi, pred)
    m.close()


@pytest.mark.parametrize("n", rm.DOMINO_N)
@pytest.mark.parametrize("rule", [r for r in rm.RULES if r != rm.RULE_INIT_STEAL], ids=rm.RULE_NAMES[:6])
def test_domino_through_match_groups(uvo, rule, n):
    """N sweeps, one query settling per sweep, the last thread's query alone moving in the last one.  At 4097 the tables are global and
    thread 0 owns five queries."""
    s = rm.domino(n)
    m = uvo.ORBmatcher(rm.NN_RATIO, False)
    got = _match_groups(uvo, m, s, rule, 50, 1)
    _same(got, s.expected + (n,), "%s rule=%s" % (s.name, rm.RULE_NAMES[rule]))
    _same(got, rm.resolve(rule, 50, rm.NN_RATIO, 1, s.cand_lists, s.D, s.tlevel), "%s rule=%s against the model" % (s.name, rm.RULE_NAMES[rule]))
    # without exclusivity: the choice each query makes alone, its left target at 5
    alone = _match_groups(uvo, m, s, rule, 50, 0)
    _same(alone, (np.r_[0, np.arange(n - 1)], np.r_[20, np.full(n - 1, 5)], n), "%s rule=%s exclusive=0" % (s.name, rm.RULE_NAMES[rule]))
    m.close()


@pytest.mark.parametrize("n", rm.DOMINO_N)
def test_steal_domino_through_match_groups(uvo, n):
    s = rm.steal_domino(n)
    m = uvo.ORBmatcher(rm.NN_RATIO, False)
    got = _match_groups(uvo, m, s, rm.RULE_INIT_STEAL, 50, 1)
    _same(got, s.expected + (n,), s.name)
    _same(got, rm.resolve(rm.RULE_INIT_STEAL, 50, rm.NN_RATIO, 1, s.cand_lists, s.D), s.name + " against the model")
    m.close()


@pytest.mark.parametrize("max_dist", [50, 100])
def test_pile_through_match_groups(uvo, max_dist):
    s = rm.pile(max_dist + 20, max_dist + 10, max_dist)
    m = uvo.ORBmatcher(rm.NN_RATIO, False)
    for rule in (rm.RULE_BEST_RATIO_SAME_LEVEL, rm.RULE_BEST_ONLY, rm.RULE_TRIANGULATION):
        got = _match_groups(uvo, m, s, rule, max_dist, 1)
        _same(got, s.expected + (max_dist + 1,), "%s rule=%s" % (s.name, rm.RULE_NAMES[rule]))
    for rule in rm.RULES:
        _check(uvo, m, s, rule, max_dist, 1)
    m.close()


def test_more_than_65535_targets_are_rejected(uvo):
    """Target indices are packed in 16 bits: nt = 65536 is UVO_E_BADARG, and match / dist are not touched (n_matches is zeroed on entry,
    as by every entry point of the matcher)."""
    s = rm.contention(64, 65535, 5)
    m = uvo.ORBmatcher(rm.NN_RATIO, False)
    s.tdesc = np.concatenate([s.tdesc, s.tdesc[:1]])
    start, idx = s.csr()
    match, dist = np.full(64 + PAD, M_FILL, np.int32), np.full(64 + PAD, D_FILL, np.int32)
    nm = ctypes.c_int(N_FILL)
    r = uvo.MatchRule(rm.RULE_BEST_ONLY, 100, rm.NN_RATIO, 1, 0)
    rc = uvo.lib.uvo_match_groups(m._h, 64, _p(s.qdesc), None, 65536, _p(s.tdesc), None, None, None, _p(start), _p(idx), None, ctypes.byref(r),
                                  _p(match), _p(dist), ctypes.byref(nm))
    assert rc == uvo.UVO_E_BADARG
    assert (match == M_FILL).all() and (dist == D_FILL).all() and nm.value == 0
    # and the handle is as good as before
    s.tdesc = s.tdesc[:65535]
    _check(uvo, m, s, rm.RULE_BEST_ONLY, 100, 1, s.blocked)
    m.close()


# ---- b. the copies behind geometry: the domino laid out along x -------------------------------------------------------------------

def _match_windows(uvo, m, row, rule, max_dist, ratio, blocked=None):
    """uvo_match_windows with the row's key points as targets and one window of radius 4 on level 0 per query."""
    n = len(row["kp"])
    kp, tdesc, qdesc = np.ascontiguousarray(row["kp"], uvo.KEYPOINT_DTYPE), row["tdesc"], row["qdesc"]
    qr, lv, valid = np.full(n, rm.ROW_RADIUS, np.float32), np.zeros(n, np.int32), np.ones(n, np.uint8)
    match, dist = np.full(n + PAD, M_FILL, np.int32), np.full(n + PAD, D_FILL, np.int32)
    nm = ctypes.c_int(N_FILL)
    r = uvo.MatchRule(rule, max_dist, ratio, 1, 0)
    b = row["bounds"]
    rc = uvo.lib.uvo_match_windows(m._h, _p(kp), n, _p(tdesc), _p(blocked), b[0], b[1], b[2], b[3], n, _p(row["qx"]), _p(row["qy"]), _p(qr), _p(lv),
                                   _p(lv), _p(valid), _p(qdesc), None, ctypes.byref(r), _p(match), _p(dist), ctypes.byref(nm))
    assert rc == 0, uvo.last_error()
    assert (match[n:] == M_FILL).all() and (dist[n:] == D_FILL).all()
    return match[:n], dist[:n], nm.value


def _row_kp(row):
    """the row's key points for WindowSearch / SearchForInitialization's side 1: at the window centres, level 0"""
    kp1 = row["kp"].copy()
    kp1["x"], kp1["y"] = row["qx"], row["qy"]
    return kp1


@pytest.mark.parametrize("n", rm.ROW_N)
def test_row_search_by_projection(uvo, oracle, n):
    """k_sbp_resolve: n map points projected midway between neighbouring key points, radius 4 (view_cos 0.9, th 1, scale 1).  Map point j
    ends on key point j after n sweeps; with key points pre-assigned in the middle the chain restarts behind them (the oracle decides)."""
    row = rm.domino_row(n)
    kp = np.ascontiguousarray(row["kp"], uvo.KEYPOINT_DTYPE)
    level, view_cos, in_view = np.zeros(n, np.int32), np.full(n, 0.9, np.float32), np.ones(n, np.uint8)
    sf = np.ones(1, np.float32)
    b = row["bounds"]
    m = uvo.ORBmatcher(0.8, False, max_query=n + 8, max_map_points=n + 8)
    pre = np.full(n, -1, np.int32)
    pre[[n // 3, n // 2, n // 2 + 1, n - 2]] = 70000 + np.arange(4)
    for name, start in (("free", np.full(n, -1, np.int32)), ("pre-assigned", pre)):
        want = start.copy()
        n_o = oracle.search_by_projection(row["kp"], row["tdesc"], b, want, row["qx"], row["qy"], level, view_cos, in_view, row["qdesc"], sf, 1.0, 0.8)
        got = np.concatenate([start, np.full(PAD, M_FILL, np.int32)])
        nm = ctypes.c_int(N_FILL)
        rc = uvo.lib.uvo_search_by_projection(m._h, _p(kp), n, _p(row["tdesc"]), b[0], b[1], b[2], b[3], _p(got), n, _p(row["qx"]), _p(row["qy"]),
                                              _p(level), _p(view_cos), _p(in_view), _p(row["qdesc"]), _p(sf), 1, 1.0, 0.8, ctypes.byref(nm))
        assert rc == 0, uvo.last_error()
        assert (got[n:] == M_FILL).all()
        np.testing.assert_array_equal(got[:n], want, err_msg="row of %d, %s" % (n, name))
        assert nm.value == n_o
        if name == "free":
            np.testing.assert_array_equal(want, np.arange(n))            # the closed form
            assert n_o == n
        else:
            assert n - 8 <= n_o < n and (want[start >= 0] == start[start >= 0]).all()
    m.close()


@pytest.mark.parametrize("n", rm.ROW_N)
def test_row_window_search(uvo, oracle, n):
    """WindowSearch's rule (best <= ratio * second, exclusive) through uvo_match_windows: k_win_cand + k_match_resolve."""
    row = rm.domino_row(n)
    m = uvo.ORBmatcher(rm.NN_RATIO, False)
    got = _match_windows(uvo, m, row, rm.RULE_BEST_RATIO_LEQ, 100, rm.NN_RATIO)
    _same(got, row["scene"].expected + (n,), "row of %d" % n)
    m21, n_o = oracle.window_search(_row_kp(row), row["qdesc"], np.ones(n, np.uint8), row["kp"], row["tdesc"], row["bounds"], int(rm.ROW_RADIUS), -1,
                                    INT_MAX, rm.NN_RATIO, False)
    assert n_o == n
    np.testing.assert_array_equal(m21, np.arange(n))
    # the named wrapper, as a caller reaches it
    m21_w, n_w = m.WindowSearch(_row_kp(row), row["qdesc"], np.ones(n, np.uint8), row["kp"], row["tdesc"], row["bounds"], int(rm.ROW_RADIUS))
    np.testing.assert_array_equal(m21_w, m21)
    assert n_w == n
    m.close()


@pytest.mark.parametrize("n", rm.ROW_N)
def test_row_search_for_initialization(uvo, oracle, n):
    """SearchForInitialization's rule on the steal-domino through uvo_match_windows: k_win_cand + k_match_resolve_steal."""
    row = rm.domino_row(n, steal=True)
    m = uvo.ORBmatcher(rm.NN_RATIO, False)
    got = _match_windows(uvo, m, row, rm.RULE_INIT_STEAL, 50, rm.NN_RATIO)
    _same(got, row["scene"].expected + (n,), "row of %d" % n)
    prev = np.ascontiguousarray(np.stack([row["qx"], row["qy"]], 1), np.float32)
    m12, n_o = oracle.search_for_initialization(_row_kp(row), row["qdesc"], row["kp"], row["tdesc"], row["bounds"], prev.copy(), int(rm.ROW_RADIUS),
                                                rm.NN_RATIO, False)
    assert n_o == n
    np.testing.assert_array_equal(m12, np.arange(n))
    m12_w, n_w = m.SearchForInitialization(_row_kp(row), row["qdesc"], row["kp"], row["tdesc"], row["bounds"], prev.copy(), int(rm.ROW_RADIUS))
    np.testing.assert_array_equal(m12_w, m12)
    assert n_w == n
    m.close()


# ---- c. the pile through the vocabulary-guided entry points -----------------------------------------------------------------------

@pytest.fixture(scope="module")
def pile_scene():
    return tm.pile_scene()


def _model_lists(sc, P, has1, rule, ratio, blocked=None, with_pred=False):
    """the model's match12[n1] for one pair of the pile scene"""
    q_of, lists = rm.bow_lists(sc["groups1"], P["groups"], has1)
    D = rm.Hamming(sc["desc1"][q_of], P["desc"])
    pred = None
    if with_pred:
        pred = rm.epipolar_pred(P["F12"], sc["kp1"]["x"][q_of], sc["kp1"]["y"][q_of], P["kp"]["x"], P["kp"]["y"], P["sigma2"], P["kp"]["octave"])
    match, _, n = rm.resolve(rule, 50, ratio, 1, lists, D, pred=pred, blocked=blocked)
    out = np.full(len(sc["kp1"]), -1, np.int32)
    out[q_of] = match
    return out, n


@pytest.mark.parametrize("kf_kf", [False, True])
def test_pile_search_by_bow(uvo, oracle, pile_scene, kf_kf):
    """Both forms of SearchByBoW on the pile (nnratio 1: d < 1 * (d + 1) always holds, so the best free target is taken): 1150 queries,
    the second node's in the second query of their threads, TH_LOW + 1 sweeps."""
    sc, P = pile_scene, pile_scene["pairs"][0]
    n1, n2 = len(sc["kp1"]), len(P["kp"])
    usable1 = np.ones(n1, np.uint8)
    usable1[[0, 5, 1031]] = 0                                            # some features of side 1 are not queries at all
    usable2 = None
    if kf_kf:
        usable2 = np.ones(n2, np.uint8)
        usable2[[3, 64]] = 0
    want, n = _model_lists(sc, P, 1 - usable1, rm.RULE_BEST_RATIO_LT if kf_kf else rm.RULE_BEST_RATIO_LE, 1.0,
                           None if usable2 is None else 1 - usable2)
    assert n == 2 * ((49 if kf_kf else 51))                              # KF-KF: d < TH_LOW and two targets are not usable
    m12_o, n_o = oracle.search_by_bow(kf_kf, sc["groups1"], sc["desc1"], sc["kp1"]["angle"], usable1, P["groups"], P["desc"], P["kp"]["angle"], usable2,
                                      1.0, False)
    np.testing.assert_array_equal(m12_o, want)
    m = uvo.ORBmatcher(1.0, False)
    m12, nm = m.SearchByBoW(uvo.FeatureVector(sc["groups1"]), sc["desc1"], sc["kp1"]["angle"], usable1, uvo.FeatureVector(P["groups"]), P["desc"],
                            P["kp"]["angle"], usable2, kf_kf=kf_kf)
    m.close()
    np.testing.assert_array_equal(m12, want)
    assert nm == n == n_o


def test_pile_search_for_triangulation(uvo, oracle, pile_scene):
    """SearchForTriangulation on the device, and its batch form whose acceptance loop is replayed on the host (csrc/matcher_batch.cpp):
    both pairs, the second one also with the map points the first one would have made."""
    sc = pile_scene
    fv1 = uvo.FeatureVector(sc["groups1"])
    pairs = [(uvo.FeatureVector(P["groups"]), P["kp"], P["desc"], P["has_mp"], P["F12"], P["sigma2"]) for P in sc["pairs"]]
    m = uvo.ORBmatcher(0.6, False)
    m.SearchForTriangulationBatch(fv1, sc["kp1"], sc["desc1"], sc["has_mp1"], pairs)
    after_first = sc["has_mp1"].copy()
    for k, P in enumerate(sc["pairs"]):
        for has1 in (sc["has_mp1"], after_first):
            want, n = _model_lists(sc, P, has1, rm.RULE_TRIANGULATION, 0.0, P["has_mp"], with_pred=True)
            assert n == 102
            m12_o, n_o = oracle.search_for_triangulation(sc["groups1"], sc["kp1"], sc["desc1"], has1, P["groups"], P["kp"], P["desc"], P["has_mp"],
                                                         P["F12"], P["sigma2"], False)
            np.testing.assert_array_equal(m12_o, want)
            m12, nm = m.SearchForTriangulation(fv1, sc["kp1"], sc["desc1"], has1, pairs[k][0], P["kp"], P["desc"], P["has_mp"], P["F12"], P["sigma2"])
            np.testing.assert_array_equal(m12, want, err_msg="pair %d on the device" % k)
            m12_b, nm_b = m.SearchForTriangulationNext(k, has1)
            np.testing.assert_array_equal(m12_b, want, err_msg="pair %d replayed on the host" % k)
            assert nm == nm_b == n == n_o
            if k == 0 and has1 is sc["has_mp1"]:
                after_first[np.nonzero(want >= 0)[0]] = 1
                assert after_first.sum() == 102
    m.close()


@pytest.mark.parametrize("extra2", [0, 4040])
def test_pile_create_new_map_points(uvo, oracle, pile_scene, extra2):
    """The in-kernel copy (512 threads, its own tri_choice): 1150 queries, so a thread owns up to three; the second pair's queue forms
    from the features the first pair left without a map point.  With 4040 more key points in front of key frame 2's (zero descriptors,
    distance 0 from every query, in a node of their own) the ownership tables are the global ones and the pile's targets sit above
    index 4040.  Match lists against the model, verdicts against tests/triangulation_model.py as in test_gpu_triangulation.py."""
    from test_gpu_triangulation import _cam, _check_list, _pairs
    sc = pile_scene if extra2 == 0 else tm.pile_scene(extra2=extra2)
    m = uvo.ORBmatcher(0.6, False)
    dev, has_after = m.CreateNewMapPoints(uvo.FeatureVector(sc["groups1"]), sc["kp1"], sc["desc1"], sc["has_mp1"], _pairs(uvo, sc), _cam(uvo, sc["cam1"]),
                                          [_cam(uvo, c) for c in sc["cams2"]], sc["ratio_factor"])
    m.close()
    res, has_model = tm.chain(oracle, sc, False, device=dev)             # compares every pair's match list with the oracle's on its way
    has1 = sc["has_mp1"].copy()
    for p, (d, r, P) in enumerate(zip(dev, res, sc["pairs"])):
        want, n = _model_lists(sc, P, has1, rm.RULE_TRIANGULATION, 0.0, P["has_mp"], with_pred=True)
        idx1 = np.nonzero(want >= 0)[0]
        np.testing.assert_array_equal(d["idx1"], idx1, err_msg="pair %d: idx1 against the model" % p)
        np.testing.assert_array_equal(d["idx2"], want[idx1], err_msg="pair %d: idx2 against the model" % p)
        assert n == 102 == len(d["idx1"])
        _check_list("pile pair %d" % p, d["verdict"], d["x3d"], r)
        assert d["n_accepted"] == int((d["verdict"] == tm.ACCEPTED).sum()) == int((r["verdict"] == tm.ACCEPTED).sum())
        has1[d["idx1"][r["verdict"] == tm.ACCEPTED]] = 1
    assert sum(int(r["sensitive"].sum()) for r in res) == 0
    assert dev[0]["n_accepted"] > 90                                     # the first pair's matches are true correspondences
    np.testing.assert_array_equal(has_after, has_model)
    np.testing.assert_array_equal(has_after, has1)
