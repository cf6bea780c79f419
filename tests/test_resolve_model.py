"""The sequential model of tests/resolve_model.py against the oracle's named functions (two independent sequential statements of
src/ORBmatcher.cc: they must agree exactly), against the closed forms of its constructed scenes, and the proof that every scene the GPU
file (tests/test_gpu_resolve.py) runs is as deep as it is meant to be."""
import numpy as np
import pytest

import oracle_lib
import resolve_model as rm
import triangulation_model as tm

SF = np.array([1.2 ** i for i in range(8)], np.float32)
BOUNDS = (0, 0, 752, 480)


def _descs(rng, protos, n):
    """Prototypes with 0, 3 or 12 random bits toggled: a query has several candidates inside every threshold, ties among them."""
    out = protos[rng.integers(0, len(protos), n)].copy()
    for r in range(n):
        b = np.unpackbits(out[r])
        b[rng.choice(256, int(rng.choice([0, 3, 12])), replace=False)] ^= 1
        out[r] = np.packbits(b)
    return out


def _frame(rng, protos, n, around=None, octaves=4):
    kp = np.zeros(n, oracle_lib.KP)
    if around is None:
        kp["x"], kp["y"] = rng.uniform(60, 330, n), rng.uniform(60, 240, n)
    else:
        kp["x"], kp["y"] = around["x"] + rng.uniform(-6, 6, n), around["y"] + rng.uniform(-6, 6, n)
    kp["octave"], kp["angle"] = rng.integers(0, octaves, n), rng.uniform(0, 360, n)
    return kp, _descs(rng, protos, n)


def _protos(rng):
    base = rng.integers(0, 256, 32, dtype=np.uint8)
    out = []
    for k in range(4):
        b = np.unpackbits(base)
        b[40 * k:40 * k + 20] ^= 1
        out.append(np.packbits(b))
    return np.stack(out)


@pytest.mark.parametrize("seed,th,ratio", [(1, 1.0, 0.8), (2, 3.0, 0.9), (3, 1.0, 0.6)])
def test_model_against_oracle_search_by_projection(oracle, seed, th, ratio):
    rng = np.random.default_rng(seed)
    protos = _protos(rng)
    kp, desc = _frame(rng, protos, 300)
    nmp = 400
    src = rng.integers(0, len(kp), nmp)
    px = (kp["x"][src] + rng.uniform(-3, 3, nmp)).astype(np.float32)
    py = (kp["y"][src] + rng.uniform(-3, 3, nmp)).astype(np.float32)
    level = np.clip(kp["octave"][src] + rng.integers(0, 2, nmp), 0, 7).astype(np.int32)
    view_cos = rng.choice(np.array([0.9, 0.999], np.float32), nmp)
    in_view = (rng.random(nmp) < 0.9).astype(np.uint8)
    mp_desc = _descs(rng, protos, nmp)
    assigned = np.where(rng.random(len(kp)) < 0.1, 7000, -1).astype(np.int32)
    lists = []
    for i in range(nmp):
        r = np.float32(2.5) if float(view_cos[i]) > 0.998 else np.float32(4.0)         # RadiusByViewingCos :127-133
        if th != 1.0:
            r = np.float32(r * np.float32(th))
        r = np.float32(r * SF[level[i]])
        lists.append(oracle.features_in_area(kp, BOUNDS, px[i], py[i], r, level[i] - 1, level[i]) if in_view[i] else [])
    match, _, n = rm.resolve(rm.RULE_BEST_RATIO_SAME_LEVEL, 100, ratio, 1, lists, rm.Hamming(mp_desc, desc), tlevel=kp["octave"],
                             blocked=assigned >= 0)
    want = assigned.copy()
    want[match[match >= 0]] = np.nonzero(match >= 0)[0]
    got = assigned.copy()
    n_o = oracle.search_by_projection(kp, desc, BOUNDS, got, px, py, level, view_cos, in_view, mp_desc, SF, th, ratio)
    assert n > 100 and n == n_o
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("seed,levels", [(4, (-1, 0x7fffffff)), (5, (1, 2))])
def test_model_against_oracle_window_search(oracle, seed, levels):
    rng = np.random.default_rng(seed)
    protos = _protos(rng)
    kp1, d1 = _frame(rng, protos, 300)
    kp2, d2 = _frame(rng, protos, 300, around=kp1)
    kp2["octave"] = np.where(rng.random(300) < 0.8, kp1["octave"], kp2["octave"])
    has1 = (rng.random(300) < 0.8).astype(np.uint8)
    lists = []
    for i in range(300):
        lv = int(kp1["octave"][i])
        skip = not has1[i] or (levels[0] > 0 and lv < levels[0]) or (levels[1] < 0x7fffffff and lv > levels[1])      # :427-441
        lists.append([] if skip else oracle.features_in_area(kp2, BOUNDS, kp1["x"][i], kp1["y"][i], 15, lv, lv))
    match, _, n = rm.resolve(rm.RULE_BEST_RATIO_LEQ, 100, 0.9, 1, lists, rm.Hamming(d1, d2))
    want = np.full(300, -1, np.int32)
    want[match[match >= 0]] = np.nonzero(match >= 0)[0]
    m21, n_o = oracle.window_search(kp1, d1, has1, kp2, d2, BOUNDS, 15, levels[0], levels[1], 0.9, False)
    assert n > 50 and n == n_o
    np.testing.assert_array_equal(m21, want)


@pytest.mark.parametrize("seed", [6, 7])
def test_model_against_oracle_search_for_initialization(oracle, seed):
    rng = np.random.default_rng(seed)
    protos = _protos(rng)
    kp1, d1 = _frame(rng, protos, 400, octaves=2)
    kp2, d2 = _frame(rng, protos, 400, around=kp1, octaves=2)
    prev = np.ascontiguousarray(np.stack([kp1["x"], kp1["y"]], 1) + rng.uniform(-4, 4, (400, 2)), np.float32)
    lists = [oracle.features_in_area(kp2, BOUNDS, prev[i, 0], prev[i, 1], 20, 0, 0) if kp1["octave"][i] == 0 else [] for i in range(400)]
    match, dist, n = rm.resolve(rm.RULE_INIT_STEAL, 50, 0.9, 1, lists, rm.Hamming(d1, d2))
    m12, n_o = oracle.search_for_initialization(kp1, d1, kp2, d2, BOUNDS, prev.copy(), 20, 0.9, False)
    assert n > 50 and n == n_o
    np.testing.assert_array_equal(m12, match)
    # the scene does steal: more queries accept a target than hold one at the end
    accepts, _, _ = rm.resolve(rm.RULE_BEST_RATIO_LE, 50, 0.9, 0, lists, rm.Hamming(d1, d2))
    assert (accepts >= 0).sum() > n


def _bow_scene(rng, n1=300, n2=300, nodes=12):
    protos = _protos(rng)
    kp1, d1 = _frame(rng, protos, n1)
    kp2, d2 = _frame(rng, protos, n2)
    # integer rows: with the sideways F12 the squared distance to the epipolar line is (y2 - y1)^2 exactly, never at a threshold
    kp1["y"], kp2["y"] = rng.integers(0, 4, n1), rng.integers(0, 4, n2)
    g1, g2 = tm.bow_groups(rng.integers(0, nodes, n1)), tm.bow_groups(rng.integers(0, nodes + 2, n2))
    return kp1, d1, g1, kp2, d2, g2


@pytest.mark.parametrize("kf_kf", [False, True])
@pytest.mark.parametrize("seed", [8, 9])
def test_model_against_oracle_search_by_bow(oracle, seed, kf_kf):
    rng = np.random.default_rng(seed)
    kp1, d1, g1, kp2, d2, g2 = _bow_scene(rng)
    usable1 = (rng.random(len(kp1)) < 0.8).astype(np.uint8)
    usable2 = (rng.random(len(kp2)) < 0.8).astype(np.uint8) if kf_kf else None
    q_of, lists = rm.bow_lists(g1, g2, 1 - usable1)
    match, _, n = rm.resolve(rm.RULE_BEST_RATIO_LT if kf_kf else rm.RULE_BEST_RATIO_LE, 50, 0.9, 1, lists, rm.Hamming(d1[q_of], d2),
                             blocked=None if usable2 is None else 1 - usable2)
    want = np.full(len(kp1), -1, np.int32)
    want[q_of] = match
    m12, n_o = oracle.search_by_bow(kf_kf, g1, d1, kp1["angle"], usable1, g2, d2, kp2["angle"], usable2, 0.9, False)
    assert n > 20 and n == n_o
    np.testing.assert_array_equal(m12, want)


@pytest.mark.parametrize("seed", [10, 11])
def test_model_against_oracle_search_for_triangulation(oracle, seed):
    rng = np.random.default_rng(seed)
    kp1, d1, g1, kp2, d2, g2 = _bow_scene(rng)
    has1, has2 = (rng.random(len(kp1)) < 0.2).astype(np.uint8), (rng.random(len(kp2)) < 0.2).astype(np.uint8)
    sigma2 = (SF * SF).astype(np.float32)
    q_of, lists = rm.bow_lists(g1, g2, has1)
    pred = rm.epipolar_pred(rm.SIDEWAYS_F12, kp1["x"][q_of], kp1["y"][q_of], kp2["x"], kp2["y"], sigma2, kp2["octave"])
    fails = sum(not pred(i, t) for i in range(len(lists)) for t in lists[i])
    assert 0.1 < fails / sum(len(c) for c in lists) < 0.6                  # the predicate decides: (y2 - y1)^2 = 4 or 9 on low octaves
    match, _, n = rm.resolve(rm.RULE_TRIANGULATION, 50, 0.0, 1, lists, rm.Hamming(d1[q_of], d2), pred=pred, blocked=has2)
    want = np.full(len(kp1), -1, np.int32)
    want[q_of] = match
    m12, n_o = oracle.search_for_triangulation(g1, kp1, d1, has1, g2, kp2, d2, has2, rm.SIDEWAYS_F12, sigma2, False)
    assert n > 50 and n == n_o
    np.testing.assert_array_equal(m12, want)


# ---- closed forms -----------------------------------------------------------------------------------------------------------------

BEST_RULES = (rm.RULE_BEST_RATIO_SAME_LEVEL, rm.RULE_BEST_ONLY, rm.RULE_BEST_RATIO_LE, rm.RULE_BEST_RATIO_LT, rm.RULE_BEST_RATIO_LEQ)


def _sweeps(s, rule, max_dist, ratio=rm.NN_RATIO, exclusive=1, blocked=None):
    return rm.jacobi_sweeps(rule, max_dist, ratio, exclusive, s.cand_lists, s.D, s.nt, s.tlevel, None, blocked)


@pytest.mark.parametrize("n", rm.DOMINO_N)
def test_domino_closed_form_and_depth(n):
    s = rm.domino(n)
    assert all(s.D(j, j) == 20 for j in range(n)) and all(s.D(j, j - 1) == 5 for j in range(1, n))
    for rule in BEST_RULES + (rm.RULE_TRIANGULATION,):
        match, dist, k = rm.resolve(rule, 50, rm.NN_RATIO, 1, s.cand_lists, s.D, s.tlevel)
        np.testing.assert_array_equal(match, s.expected[0])
        np.testing.assert_array_equal(dist, s.expected[1])
        assert k == n
        alone, d_alone, _ = rm.resolve(rule, 50, rm.NN_RATIO, 0, s.cand_lists, s.D, s.tlevel)      # every query wants its left target
        assert alone.tolist() == [0] + list(range(n - 1)) and d_alone.tolist() == [20] + [5] * (n - 1)
        if n == 64 or rule == rm.RULE_BEST_ONLY:          # the depth does not depend on the rule: all of them at 64, one at every N
            assert _sweeps(s, rule, 50) == n
            assert _sweeps(s, rule, 50, exclusive=0) == 1


@pytest.mark.parametrize("n", rm.DOMINO_N)
def test_steal_domino_closed_form_and_depth(n):
    s = rm.steal_domino(n)
    assert all(s.D(j, j) == 20 for j in range(n)) and all(s.D(j, j - 1) == 20 for j in range(1, n))
    match, dist, k = rm.resolve(rm.RULE_INIT_STEAL, 50, rm.NN_RATIO, 1, s.cand_lists, s.D)
    np.testing.assert_array_equal(match, s.expected[0])
    np.testing.assert_array_equal(dist, s.expected[1])
    assert k == n and _sweeps(s, rm.RULE_INIT_STEAL, 50) == n


@pytest.mark.parametrize("max_dist", [50, 100])
def test_pile_closed_form_and_depth(max_dist):
    s = rm.pile(max_dist + 20, max_dist + 10, max_dist)
    for rule in (rm.RULE_BEST_RATIO_SAME_LEVEL, rm.RULE_BEST_ONLY, rm.RULE_TRIANGULATION):     # levels alternate: no ratio test
        match, dist, _ = rm.resolve(rule, max_dist, rm.NN_RATIO, 1, s.cand_lists, s.D, s.tlevel)
        np.testing.assert_array_equal(match, s.expected[0])
        np.testing.assert_array_equal(dist, s.expected[1])
        assert _sweeps(s, rule, max_dist) >= max_dist + 1


def test_pile_scene_of_the_named_entry_points_is_deep():
    """The scene SearchByBoW, SearchForTriangulation, its batch and CreateNewMapPoints get on the GPU: the model's answer is the closed
    form, per vocabulary node, and the iteration needs TH_LOW + 1 sweeps (SearchByBoW(KF, KF): `<`, one fewer target, the same count
    with the sweep in which the rest let go)."""
    sc = tm.pile_scene()
    P = sc["pairs"][0]
    q_of, lists = rm.bow_lists(sc["groups1"], P["groups"], sc["has_mp1"])
    assert len(lists) == len(sc["kp1"]) > 1024 and len(lists[0]) == 60
    D = rm.Hamming(sc["desc1"][q_of], P["desc"])
    pred = rm.epipolar_pred(P["F12"], sc["kp1"]["x"][q_of], sc["kp1"]["y"][q_of], P["kp"]["x"], P["kp"]["y"], P["sigma2"], P["kp"]["octave"])
    assert all(pred(i, t) for i in (0, 1, 500, 1029, 1030, 1149) for t in lists[i])
    want = np.full(len(q_of), -1)
    want[:51], want[1030:1030 + 51] = np.arange(51), 60 + np.arange(51)
    match, _, n = rm.resolve(rm.RULE_TRIANGULATION, 50, 0.0, 1, lists, D, pred=pred, blocked=P["has_mp"])
    np.testing.assert_array_equal(match, want)
    assert rm.jacobi_sweeps(rm.RULE_TRIANGULATION, 50, 0.0, 1, lists, D, 120) >= 51
    for rule, last in ((rm.RULE_BEST_RATIO_LE, 51), (rm.RULE_BEST_RATIO_LT, 50)):           # nnratio 1: d < 1 * (d + 1) always holds
        want = np.full(len(q_of), -1)
        want[:last], want[1030:1030 + last] = np.arange(last), 60 + np.arange(last)
        match, _, n = rm.resolve(rule, 50, 1.0, 1, lists, D)
        np.testing.assert_array_equal(match, want)
        assert rm.jacobi_sweeps(rule, 50, 1.0, 1, lists, D, 120) >= 51


# ---- every contention scene of the GPU file is deep -------------------------------------------------------------------------------

def _contention_depths(s):
    return {(rule, md): _sweeps(s, rule, md, blocked=s.blocked) for rule in rm.RULES for md in rm.MAX_DISTS if md >= 50}


@pytest.mark.parametrize("nq", rm.GROUP_NQ)
@pytest.mark.parametrize("nt", rm.GROUP_NT)
def test_contention_grid_scenes_are_deep(nq, nt):
    s = rm.contention(nq, nt, rm.CONTENTION_SEED)
    assert s.nq == nq and s.nt == nt
    if nq >= 3:
        assert len(s.cand_lists[0]) == 0 and len(s.cand_lists[-1]) == 0            # empty lists in front and behind
    if nt > 1 and nq >= 64:
        used = np.concatenate(s.cand_lists)
        assert used.min() == 0 or used.max() == nt - 1 or nt > 4096                # the hot targets span the index range
        assert used.max() > nt // 2
    if not rm.deep_enough(nq, nt):
        return
    empty = sum(len(c) == 0 for c in s.cand_lists)
    assert 0.05 * nq < empty < 0.2 * nq and s.blocked.sum() > 0
    assert any(0 < i < nq - 1 and len(s.cand_lists[i - 1]) and len(s.cand_lists[i + 1]) for i in range(nq) if not len(s.cand_lists[i]))
    depths = _contention_depths(s)
    assert min(depths.values()) >= rm.CONTENTION_DEPTH, depths
    # the distances are few-valued: ties for best, best == second, d == max_dist all occur
    ds = np.array([s.D(i, int(t)) for i in range(nq) for t in s.cand_lists[i]])
    assert {0, 50, 100, 256} <= set(ds.tolist()) and len(set(ds.tolist())) < 80
    ties = sum(1 for i in range(nq) if len(s.cand_lists[i]) > 1 and
               sorted(s.D(i, int(t)) for t in set(s.cand_lists[i].tolist()))[:2].count(min(s.D(i, int(t)) for t in s.cand_lists[i])) == 2)
    assert ties > nq // 50


@pytest.mark.parametrize("nq,nt,seed", rm.VARIANT_SCENES)
def test_contention_variant_scenes_are_deep(nq, nt, seed):
    s = rm.contention(nq, nt, seed)
    depths = _contention_depths(s)
    assert min(depths.values()) >= rm.CONTENTION_DEPTH, depths
    # without exclusivity nothing depends on anything: one sweep (the steal rule has no such switch)
    assert all(_sweeps(s, rule, 100, exclusive=0, blocked=s.blocked) == 1 for rule in rm.RULES if rule != rm.RULE_INIT_STEAL)
    # the epipolar predicate of the GPU runs fails for the targets with t % 3 == 2, a third of the pairs, and for no other
    epi, pred = rm.epipolar_third(s)
    pairs = [(i, int(t)) for i in range(nq) for t in s.cand_lists[i]]
    assert all(pred(i, t) == (t % 3 != 2) for i, t in pairs)
    assert 0.25 < sum(t % 3 == 2 for _, t in pairs) / len(pairs) < 0.42


@pytest.mark.parametrize("n", rm.ROW_N)
@pytest.mark.parametrize("steal", [False, True])
def test_domino_row_windows_hold_exactly_their_two_key_points(oracle, n, steal):
    row = rm.domino_row(n, steal)
    for j in range(n):
        for levels in ((-1, 0), (0, 0)):                 # SearchByProjection's [level - 1, level] and the two window searches' level 0
            got = oracle.features_in_area(row["kp"], row["bounds"], row["qx"][j], row["qy"][j], rm.ROW_RADIUS, *levels).tolist()
            assert got == ([0] if j == 0 else [j - 1, j]), (j, got)
