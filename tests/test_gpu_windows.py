"""The first and the last stage of the ORBmatcher search loops on the device -- candidate lists from the 64 x 48 key-point grid, and the
rotation-consistency filter -- against the brute-force models of tests/window_model.py and tests/rotation_model.py, on scenes built
for the places extractor-made key points never reach: cells 64, 48 and -1, exact x.5 ties, members exactly at |dx| == r and one float
beyond, windows that leave the grid, radius 0, column runs of 7 / 8 / 9 / 17 items, 4096 and 4097 key points, NaN and infinite input.
tests/test_window_model.py holds the models to the oracle on the CPU and proves that the scenes contain those edges.

Membership is found by probing: the targets carry descriptors that are far apart (rows of the Sylvester Hadamard matrix: 128 or 256
bits), a probe has a window's centre, radius and levels and the descriptor of ONE target, so it matches that target exactly when the
target is in the window's list, and nothing otherwise.  Order is found with all descriptors equal: the first candidate in visiting order
wins, and blocking the winner and calling again peels the list.

Which test covers which kernel:
  k_grid_build (csrc/search.hip), LDS regime               every test below with n <= 4096
  k_grid_build, global-memory regime                       test_4096_and_4097_key_points[4097]
  k_win_cand (csrc/match_engine.hip)                       test_match_windows_membership, test_fuse_membership, test_search_by_projection_kf_membership,
                                                           test_order_*[windows / kf / fuse], test_nonfinite_*, test_4096_and_4097_key_points
  k_sbp_cand (csrc/search.hip)                             test_search_by_projection_membership, test_order_by_peeling[sbp], test_nonfinite_input[sbp]
  k_fuse_walk (csrc/match_engine.hip; uvo_fuse_batch)      test_fuse_batch_membership, test_order_first_of_equals[fuse_batch], test_nonfinite_input[fuse_batch],
                                                           test_4096_and_4097_key_points
  k_rot_filter (csrc/match_engine.hip)                     test_rotation_filter
uvo_fuse_batch projects its map points itself, and KeyFrame::IsInImage drops a centre that is NaN, infinite or outside the frame before
the search: of k_fuse_walk's tests for non-finite input only the one on the radius (th NaN or infinite) can be reached and is; its tests
on the centre cannot be reached through any entry point.

Every comparison is exact.  Outputs have PAD more rows than the call may write, prefilled with values no result can equal; the pad must
keep them."""
import ctypes

import numpy as np
import pytest

import rotation_model as rot
import window_model as wm

pytestmark = pytest.mark.gpu

f32 = np.float32
M_FILL, D_FILL, N_FILL, PAD = 0x5EADBEEF, 0x0BADF00D, -12345, 7
RULE_BEST_ONLY = 1


def _p(a):
    return None if a is None else a.ctypes.data


@pytest.fixture(scope="module")
def scenes():
    s = {b: wm.edge_scene(b) for b in wm.EDGE_BOUNDS}
    s["nonfinite"], s["one_cell"] = wm.nonfinite_scene(), wm.one_cell_scene()
    return s


@pytest.fixture(scope="module")
def matcher(uvo):
    m = uvo.ORBmatcher(0.8, False, max_query=8192, max_map_points=8192)
    yield m
    m.close()


SCENE_KEYS = list(wm.EDGE_BOUNDS) + ["nonfinite", "one_cell"]
SCENE_IDS = ["%d_%d_%d_%d" % b for b in wm.EDGE_BOUNDS] + ["nonfinite", "one_cell"]


# ---- the entry points, each on (key points, descriptors) x (a list of queries) -> the raw outputs ------------------------------------

def _match_windows(uvo, m, kp, desc, bounds, q, qdesc, blocked=None, max_dist=0, valid=None):
    """q: WIN rows (the window's own level rule is used).  -> match[nq], dist[nq], n_matches"""
    nq, n = len(q), len(kp)
    kp = np.ascontiguousarray(kp, uvo.KEYPOINT_DTYPE)
    qx, qy, qr = [np.ascontiguousarray(q[k], f32) for k in ("x", "y", "r")]
    lo, hi = np.ascontiguousarray(q["lo"], np.int32), np.ascontiguousarray(q["hi"], np.int32)
    valid = np.ones(nq, np.uint8) if valid is None else np.ascontiguousarray(valid, np.uint8)
    match, dist = np.full(nq + PAD, M_FILL, np.int32), np.full(nq + PAD, D_FILL, np.int32)
    nm = ctypes.c_int(N_FILL)
    rule = uvo.MatchRule(RULE_BEST_ONLY, max_dist, 0.0, 0, 0)
    bl = None if blocked is None else np.ascontiguousarray(blocked, np.uint8)
    rc = uvo.lib.uvo_match_windows(m._h, _p(kp), n, _p(desc), _p(bl), *[int(b) for b in bounds], nq, _p(qx), _p(qy), _p(qr), _p(lo), _p(hi), _p(valid),
                                   _p(qdesc), None, ctypes.byref(rule), _p(match), _p(dist), ctypes.byref(nm))
    assert rc == 0, uvo.last_error()
    assert (match[nq:] == M_FILL).all() and (dist[nq:] == D_FILL).all(), "written past nq = %d" % nq
    return match[:nq], dist[:nq], nm.value


def _fuse(uvo, m, kp, desc, bounds, q, qdesc, th, sf):
    """uvo_fuse: q's centre and level; radius th * sf[level] -> best_idx[nq], best_dist[nq]"""
    nq, n = len(q), len(kp)
    kp = np.ascontiguousarray(kp, uvo.KEYPOINT_DTYPE)
    u, v, level = np.ascontiguousarray(q["x"], f32), np.ascontiguousarray(q["y"], f32), np.ascontiguousarray(q["level"], np.int32)
    valid, sf = np.ones(nq, np.uint8), np.ascontiguousarray(sf, f32)
    bi, bd = np.full(nq + PAD, M_FILL, np.int32), np.full(nq + PAD, D_FILL, np.int32)
    rc = uvo.lib.uvo_fuse(m._h, _p(kp), n, _p(desc), *[int(b) for b in bounds], nq, _p(u), _p(v), _p(level), _p(valid), _p(qdesc), _p(sf), len(sf),
                          float(th), _p(bi), _p(bd))
    assert rc == 0, uvo.last_error()
    assert (bi[nq:] == M_FILL).all() and (bd[nq:] == D_FILL).all()
    return bi[:nq], bd[:nq]


def _fuse_batch(uvo, m, kp, desc, bounds, q, qdesc, th, nlevels):
    """uvo_fuse_batch with one target whose camera is the identity with fx = fy = 1, cx = cy = 0: the map point (x, y, 1) projects to
    (x, y) exactly (1 * x + 0 * y + 0 * 1, the divide by z = 1, 1 * x + 0), KeyFrame::IsInImage drops centres outside the frame, and
    with a table of `nlevels` ones and a minimum distance of 0 every point is predicted on level nlevels - 1: radius th, levels
    [nlevels - 2, nlevels - 1].  -> best_idx[nq], best_dist[nq]"""
    nq, n = len(q), len(kp)
    kp = np.ascontiguousarray(kp, uvo.KEYPOINT_DTYPE)
    sf = np.ones(nlevels, f32)
    T = (uvo.FuseTargetC * 1)()
    T[0].kp, T[0].n, T[0].desc = _p(kp), n, _p(desc)
    T[0].min_x, T[0].min_y, T[0].max_x, T[0].max_y = [int(b) for b in bounds]
    T[0].cam = uvo.CameraPose.make(np.eye(3), np.zeros(3), np.zeros(3), 1.0, 1.0, 0.0, 0.0, bounds)
    T[0].scale_factors, T[0].nlevels = _p(sf), nlevels
    xyz = np.ascontiguousarray(np.stack([q["x"], q["y"], np.ones(nq, f32)], 1), f32)
    with np.errstate(all="ignore"):                                     # a NaN or infinite centre gives a NaN normal: the point is dropped
        normal = (xyz / np.linalg.norm(xyz.astype(np.float64), axis=1)[:, None]).astype(f32)
    mn, mx = np.zeros(nq, f32), np.full(nq, 1e30, f32)
    bi, bd = np.full(nq + PAD, M_FILL, np.int32), np.full(nq + PAD, D_FILL, np.int32)
    rc = uvo.lib.uvo_fuse_batch(m._h, 1, T, nq, _p(xyz), _p(normal), _p(mn), _p(mx), None, _p(qdesc), float(th), _p(bi), _p(bd))
    assert rc == 0, uvo.last_error()
    assert (bi[nq:] == M_FILL).all() and (bd[nq:] == D_FILL).all()
    return bi[:nq], bd[:nq]


def _in_image(bounds, w):
    return bool(w["x"] >= f32(bounds[0]) and w["x"] < f32(bounds[2]) and w["y"] >= f32(bounds[1]) and w["y"] < f32(bounds[3]))


def _sbp(uvo, m, kp, desc, bounds, w, qdesc, view_cos, th, sf, assigned):
    """uvo_search_by_projection: every row of qdesc a map point projected at w's centre on w's level -> assigned[n] after, n_matches"""
    nmp, n = len(qdesc), len(kp)
    kp = np.ascontiguousarray(kp, uvo.KEYPOINT_DTYPE)
    px, py, level = np.full(nmp, w["x"], f32), np.full(nmp, w["y"], f32), np.full(nmp, w["level"], np.int32)
    vc, in_view, sf = np.full(nmp, view_cos, f32), np.ones(nmp, np.uint8), np.ascontiguousarray(sf, f32)
    got = np.concatenate([np.asarray(assigned, np.int32), np.full(PAD, M_FILL, np.int32)])
    nm = ctypes.c_int(N_FILL)
    rc = uvo.lib.uvo_search_by_projection(m._h, _p(kp), n, _p(desc), *[int(b) for b in bounds], _p(got), nmp, _p(px), _p(py), _p(level), _p(vc), _p(in_view),
                                          _p(qdesc), _p(sf), len(sf), float(th), 0.8, ctypes.byref(nm))
    assert rc == 0, uvo.last_error()
    assert (got[n:] == M_FILL).all()
    return got[:n], nm.value


def _sbp_kf(uvo, m, kp, desc, bounds, w, qdesc, th, sf, assigned):
    """uvo_search_by_projection_kf, as _sbp (orb_dist 0, no orientation check)"""
    nmp, n = len(qdesc), len(kp)
    kp = np.ascontiguousarray(kp, uvo.KEYPOINT_DTYPE)
    u, v, level = np.full(nmp, w["x"], f32), np.full(nmp, w["y"], f32), np.full(nmp, w["level"], np.int32)
    valid, sf = np.ones(nmp, np.uint8), np.ascontiguousarray(sf, f32)
    got = np.concatenate([np.asarray(assigned, np.int32), np.full(PAD, M_FILL, np.int32)])
    nm = ctypes.c_int(N_FILL)
    rc = uvo.lib.uvo_search_by_projection_kf(m._h, _p(kp), n, _p(desc), *[int(b) for b in bounds], _p(got), nmp, _p(u), _p(v), _p(level), _p(valid), _p(qdesc),
                                             None, _p(sf), len(sf), float(th), 0, 0, ctypes.byref(nm))
    assert rc == 0, uvo.last_error()
    assert (got[n:] == M_FILL).all()
    return got[:n], nm.value


# ---- how a window's radius is handed to each marshalling layer -----------------------------------------------------------------------

NLEVELS = 6                                                             # the scenes' levels are 0..4; level + 1 must have a table entry
ABOVE, BELOW = f32(0.998), np.nextafter(f32(0.998), f32(0))            # as doubles: above 0.998 (radius 2.5) and below it (radius 4)
SBP_EXACT = {2.5: (ABOVE, 1.0), 4.0: (BELOW, 1.0), 7.5: (ABOVE, 3.0), 12.0: (BELOW, 3.0)}   # radii met with a scale factor of 1


def _table(level, value):
    sf = np.ones(NLEVELS, f32)
    sf[level] = value
    return sf


def _sbp_params(k, w):
    """(view_cos, th, scale factors) for window k: the four radii SearchByProjection makes at scale 1 are made that way, every other
    one as 4 * (r / 4), or by the variant k picks; the radius that comes out is the model's to say"""
    r = float(w["r"])
    if r in SBP_EXACT:
        return SBP_EXACT[r] + (_table(w["level"], 1.0),)
    vc, th = ((BELOW, 1.0), (ABOVE, 1.0), (BELOW, 3.0), (ABOVE, 3.0), (BELOW, 1.0))[k % 5 if r not in (0.0, 1.0, 40.0) else 0]
    base = (2.5 if vc == ABOVE else 4.0) * th
    with np.errstate(all="ignore"):
        return vc, th, _table(w["level"], f32(w["r"]) / f32(base))


def _th_params(k, w):
    """(th, scale factors) with th * sf[level] == r exactly: th = 1 or, for every other window, th = 0.5 against a doubled entry"""
    with np.errstate(all="ignore"):
        return (1.0, _table(w["level"], w["r"])) if k % 2 == 0 else (0.5, _table(w["level"], f32(2) * w["r"]))


def _expect(lists_per_query, targets):
    """probe (query q, target j) -> j when j is in q's list, else -1; as match, dist, n_matches"""
    sets = [set(int(t) for t in li) for li in lists_per_query]
    match = np.array([[j if j in li else -1 for j in targets] for li in sets], np.int64).reshape(-1)
    return match, np.where(match >= 0, 0, -1), int((match >= 0).sum())


def _probes(win, desc, targets):
    """every window against every target's descriptor: WIN rows [W * T], qdesc [W * T][32]"""
    return np.repeat(win, len(targets)), np.ascontiguousarray(np.tile(desc[targets], (len(win), 1)))


def _same(got, want, what):
    for g, w, name in zip(got, want, ("match", "dist", "n_matches")):
        np.testing.assert_array_equal(np.asarray(g, np.int64), np.asarray(w, np.int64), err_msg="%s: %s" % (what, name))


# ---- a. membership -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", SCENE_KEYS, ids=SCENE_IDS)
def test_match_windows_membership(uvo, matcher, scenes, key):
    """k_grid_build + k_win_cand: W x n probes in one call, every 97th one switched off by qvalid"""
    s = scenes[key]
    desc, targets = wm.hadamard_descriptors(s.n), np.arange(s.n)
    q, qdesc = _probes(s.win, desc, targets)
    nq = len(q) - (1 if len(q) % 256 == 0 else 0)                       # never a whole number of blocks
    q, qdesc = q[:nq], qdesc[:nq]
    valid = (np.arange(nq) % 97 != 0).astype(np.uint8)
    m0 = np.where(valid > 0, _expect(s.lists(), targets)[0][:nq], -1)
    want = (m0, np.where(m0 >= 0, 0, -1), int((m0 >= 0).sum()))
    assert nq % 256 != 0 and want[2] > len(s.win)
    _same(_match_windows(uvo, matcher, s.kp, desc, s.bounds, q, qdesc, valid=valid), want, s.name)


def _groups(s):
    """windows that share radius and level -> one call of an entry point whose radius is th * scale_factors[level]"""
    g = {}
    for k, w in enumerate(s.win):
        g.setdefault((w["r"].tobytes(), int(w["level"])), []).append(k)
    return list(g.values())


@pytest.mark.parametrize("key", SCENE_KEYS, ids=SCENE_IDS)
def test_fuse_membership(uvo, matcher, scenes, key):
    """uvo_fuse as it is (th * scale_factors[level], levels [level - 1, level], TH_LOW): one call per (radius, level)"""
    s = scenes[key]
    desc, targets = wm.hadamard_descriptors(s.n), np.arange(s.n)
    found = 0
    for gi, ks in enumerate(_groups(s)):
        w0 = s.win[ks[0]]
        th, sf = _th_params(gi, w0)
        r, lo, hi = wm.fuse_window(th, sf, int(w0["level"]))
        assert r == w0["r"] or not np.isfinite(w0["r"])
        lists = [wm.features_in_area(s.kp, s.bounds, w["x"], w["y"], r, lo, hi, s.grid) for w in s.win[ks]]
        q, qdesc = _probes(s.win[ks], desc, targets)
        want = _expect(lists, targets)
        _same(_fuse(uvo, matcher, s.kp, desc, s.bounds, q, qdesc, th, sf), want[:2], "%s windows %s" % (s.name, ks))
        found += want[2]
    assert found > len(s.win) // 2


@pytest.mark.parametrize("key", SCENE_KEYS, ids=SCENE_IDS)
def test_fuse_batch_membership(uvo, matcher, scenes, key):
    """k_fuse_walk, which only uvo_fuse_batch launches: one call per (radius, level); centres outside the frame find nothing there"""
    s = scenes[key]
    desc, targets = wm.hadamard_descriptors(s.n), np.arange(s.n)
    found = 0
    for ks in _groups(s):
        w0 = s.win[ks[0]]
        level = int(w0["level"])
        r, lo, hi = wm.fuse_window(w0["r"], np.ones(level + 1, f32), level)
        lists = [wm.features_in_area(s.kp, s.bounds, w["x"], w["y"], r, lo, hi, s.grid) if _in_image(s.bounds, w) else [] for w in s.win[ks]]
        q, qdesc = _probes(s.win[ks], desc, targets)
        want = _expect(lists, targets)
        _same(_fuse_batch(uvo, matcher, s.kp, desc, s.bounds, q, qdesc, w0["r"], level + 1), want[:2], "%s windows %s" % (s.name, ks))
        found += want[2]
    assert found > len(s.win) // 2


@pytest.mark.parametrize("key", SCENE_KEYS, ids=SCENE_IDS)
def test_search_by_projection_membership(uvo, matcher, scenes, key):
    """k_sbp_cand behind uvo_search_by_projection: one call per window, n map points that each want a different key point; view_cos at
    float32(0.998) and one float below, th 1 and 3"""
    s = scenes[key]
    desc = wm.hadamard_descriptors(s.n)
    found, variants = 0, set()
    for k, w in enumerate(s.win):
        vc, th, sf = _sbp_params(k, w)
        r, lo, hi = wm.sbp_window(vc, th, sf, int(w["level"]))
        if float(w["r"]) in SBP_EXACT or float(w["r"]) in (0.0, 1.0, 40.0):
            assert r == w["r"]
        want = wm.features_in_area(s.kp, s.bounds, w["x"], w["y"], r, lo, hi, s.grid)
        exp = np.full(s.n, -1, np.int32)
        exp[want] = want
        got, nm = _sbp(uvo, matcher, s.kp, desc, s.bounds, w, desc, vc, th, sf, np.full(s.n, -1, np.int32))
        np.testing.assert_array_equal(got, exp, err_msg="%s window %d %s view_cos %r th %g" % (s.name, k, w, vc, th))
        assert nm == len(want)
        found += len(want)
        variants.add((vc == ABOVE, th))
    assert found > len(s.win) // 2 and (len(variants) == 4 or key not in wm.EDGE_BOUNDS)


@pytest.mark.parametrize("key", SCENE_KEYS, ids=SCENE_IDS)
def test_search_by_projection_kf_membership(uvo, matcher, scenes, key):
    """uvo_search_by_projection_kf (th * scale_factors[level], levels [level - 1, level + 1]): one call per window"""
    s = scenes[key]
    desc = wm.hadamard_descriptors(s.n)
    found = 0
    for k, w in enumerate(s.win):
        th, sf = _th_params(k, w)
        r, lo, hi = wm.sbp_kf_window(th, sf, int(w["level"]))
        assert r == w["r"] or not np.isfinite(w["r"])
        want = wm.features_in_area(s.kp, s.bounds, w["x"], w["y"], r, lo, hi, s.grid)
        exp = np.full(s.n, -1, np.int32)
        exp[want] = want
        got, nm = _sbp_kf(uvo, matcher, s.kp, desc, s.bounds, w, desc, th, sf, np.full(s.n, -1, np.int32))
        np.testing.assert_array_equal(got, exp, err_msg="%s window %d %s th %g" % (s.name, k, w, th))
        assert nm == len(want)
        found += len(want)
    assert found > len(s.win) // 2


# ---- b. order ----------------------------------------------------------------------------------------------------------------------

def _order_windows(s):
    ks = s.which("order") + s.which("one_cell") + s.which("run")
    assert len(ks) >= 8
    return ks


@pytest.mark.parametrize("bounds", wm.EDGE_BOUNDS, ids=SCENE_IDS[:4])
@pytest.mark.parametrize("entry", ["windows", "sbp", "kf"])
def test_order_by_peeling(uvo, matcher, scenes, bounds, entry):
    """All descriptors equal: the first candidate in (ix, iy, index) order wins.  Blocking the winner (`blocked` for uvo_match_windows,
    `assigned` for the two projection searches) and calling again peels the whole list, which must come off in the model's order."""
    s = scenes[bounds]
    desc = np.zeros((s.n, 32), np.uint8)
    ks = _order_windows(s)
    if entry == "windows":
        lists = [list(s.lists()[k]) for k in ks]
        blocked, peeled = np.zeros(s.n, np.uint8), [[] for _ in ks]
        for _ in range(max(map(len, lists)) + 1):
            match, dist, nm = _match_windows(uvo, matcher, s.kp, desc, s.bounds, s.win[ks], np.zeros((len(ks), 32), np.uint8), blocked)
            assert nm == int((match >= 0).sum()) and ((dist == 0) == (match >= 0)).all()
            for i, t in enumerate(match):
                if t >= 0:
                    peeled[i].append(int(t))
            blocked[match[match >= 0]] = 1
        assert nm == 0
        # a winner blocked for one window is blocked for all: a list comes off in its own order, less what others took before
        for i, k in enumerate(ks):
            assert peeled[i] == [t for t in lists[i] if t in peeled[i]], "%s window %d" % (s.name, k)
        assert sorted(sum(peeled, [])) == sorted(set(sum(lists, [])))
        for i, k in enumerate(s.which("order")):
            assert peeled[ks.index(k)] == lists[ks.index(k)]            # the clusters share no key point: their lists come off whole
        return
    for k in ks:
        w = s.win[k]
        if entry == "sbp":
            vc, th, sf = _sbp_params(k, w)
            r, lo, hi = wm.sbp_window(vc, th, sf, int(w["level"]))
            call = lambda a: _sbp(uvo, matcher, s.kp, desc, s.bounds, w, np.zeros((1, 32), np.uint8), vc, th, sf, a)
        else:
            th, sf = _th_params(k, w)
            r, lo, hi = wm.sbp_kf_window(th, sf, int(w["level"]))
            call = lambda a: _sbp_kf(uvo, matcher, s.kp, desc, s.bounds, w, np.zeros((1, 32), np.uint8), th, sf, a)
        want = list(wm.features_in_area(s.kp, s.bounds, w["x"], w["y"], r, lo, hi, s.grid))
        assert len(want) >= 3
        assigned, peeled = np.full(s.n, -1, np.int32), []
        for _ in range(len(want) + 1):
            after, nm = call(assigned)
            new = np.nonzero(after != assigned)[0]
            assert nm == len(new) <= 1 and (after[new] == 0).all()
            peeled += [int(t) for t in new]
            assigned = np.where(after >= 0, 70000, -1).astype(np.int32)     # held by some other map point from now on
        assert nm == 0 and peeled == want, "%s window %d through %s" % (s.name, k, entry)


@pytest.mark.parametrize("key", SCENE_KEYS, ids=SCENE_IDS)
@pytest.mark.parametrize("entry", ["fuse", "fuse_batch"])
def test_order_first_of_equals(uvo, matcher, scenes, key, entry):
    """Fuse has no blocking: with all descriptors equal every window must return the first key point of its list"""
    s = scenes[key]
    desc = np.zeros((s.n, 32), np.uint8)
    firsts = 0
    for gi, ks in enumerate(_groups(s)):
        w0, q = s.win[ks[0]], s.win[ks]
        level = int(w0["level"])
        qdesc = np.zeros((len(ks), 32), np.uint8)
        if entry == "fuse":
            th, sf = _th_params(gi, w0)
            r, lo, hi = wm.fuse_window(th, sf, level)
            got = _fuse(uvo, matcher, s.kp, desc, s.bounds, q, qdesc, th, sf)
            lists = [wm.features_in_area(s.kp, s.bounds, w["x"], w["y"], r, lo, hi, s.grid) for w in q]
        else:
            r, lo, hi = wm.fuse_window(w0["r"], np.ones(level + 1, f32), level)
            got = _fuse_batch(uvo, matcher, s.kp, desc, s.bounds, q, qdesc, w0["r"], level + 1)
            lists = [wm.features_in_area(s.kp, s.bounds, w["x"], w["y"], r, lo, hi, s.grid) if _in_image(s.bounds, w) else [] for w in q]
        first = np.array([li[0] if len(li) else -1 for li in lists])
        _same(got, (first, np.where(first >= 0, 0, -1)), "%s windows %s through %s" % (s.name, ks, entry))
        firsts += sum(len(li) > 1 and li[0] != min(li) for li in lists)
    if key in wm.EDGE_BOUNDS:
        assert firsts >= 5                                              # lists whose first key point is not their lowest index


# ---- c. sizes ----------------------------------------------------------------------------------------------------------------------

def test_no_key_points_and_no_queries(uvo, matcher, scenes):
    s = scenes[wm.EDGE_BOUNDS[0]]
    desc = wm.hadamard_descriptors(s.n)
    none, q = s.kp[:0], s.win[:9]
    qdesc = np.ascontiguousarray(desc[:9])
    _same(_match_windows(uvo, matcher, none, desc[:0], s.bounds, q, qdesc), (np.full(9, -1), np.full(9, -1), 0), "n = 0")
    _same(_fuse(uvo, matcher, none, desc[:0], s.bounds, q, qdesc, 1.0, np.ones(NLEVELS, f32)), (np.full(9, -1), np.full(9, -1)), "fuse, n = 0")
    _same(_fuse_batch(uvo, matcher, none, desc[:0], s.bounds, q, qdesc, 1.0, 1), (np.full(9, -1), np.full(9, -1)), "fuse_batch, n = 0")
    assert _sbp(uvo, matcher, none, desc[:0], s.bounds, q[0], qdesc, 0.5, 1.0, np.ones(NLEVELS, f32), np.zeros(0, np.int32))[1] == 0
    assert _sbp_kf(uvo, matcher, none, desc[:0], s.bounds, q[0], qdesc, 1.0, np.ones(NLEVELS, f32), np.zeros(0, np.int32))[1] == 0
    # no queries: nothing is written, n_matches is 0
    assert _match_windows(uvo, matcher, s.kp, desc, s.bounds, s.win[:0], desc[:0])[2] == 0
    _fuse(uvo, matcher, s.kp, desc, s.bounds, s.win[:0], desc[:0], 1.0, np.ones(NLEVELS, f32))
    _fuse_batch(uvo, matcher, s.kp, desc, s.bounds, s.win[:0], desc[:0], 1.0, 1)
    before = np.full(s.n, -1, np.int32)
    for got, nm in (_sbp(uvo, matcher, s.kp, desc, s.bounds, s.win[0], desc[:0], 0.5, 1.0, np.ones(NLEVELS, f32), before),
                    _sbp_kf(uvo, matcher, s.kp, desc, s.bounds, s.win[0], desc[:0], 1.0, np.ones(NLEVELS, f32), before)):
        assert nm == 0 and (got == -1).all()


@pytest.mark.parametrize("n", [4096, 4097])
def test_4096_and_4097_key_points(uvo, matcher, n):
    """The grid build keeps up to 4096 key points in LDS and works in global memory beyond: both sides of the switch, through
    uvo_match_windows, uvo_fuse and uvo_fuse_batch.  Random descriptors; 64 targets are probed, each more than 50 bits (TH_LOW) from
    every other row (tests/test_window_model.py), and with all descriptors equal the first of every list is checked."""
    s = wm.big_scene(n)
    desc = wm.random_descriptors(n)
    targets = wm.big_targets(s)
    q, qdesc = _probes(s.win, desc, targets)
    want = _expect(s.lists(), targets)
    assert want[2] >= 80
    _same(_match_windows(uvo, matcher, s.kp, desc, s.bounds, q, qdesc), want, "%s through uvo_match_windows" % s.name)
    zeros, qz = np.zeros((n, 32), np.uint8), np.zeros((len(s.win), 32), np.uint8)
    first = np.array([li[0] if len(li) else -1 for li in s.lists()])
    assert (first >= 0).sum() >= 10
    _same(_match_windows(uvo, matcher, s.kp, zeros, s.bounds, s.win, qz), (first, np.where(first >= 0, 0, -1), int((first >= 0).sum())), s.name + " firsts")
    for ks in _groups(s):
        w0 = s.win[ks[0]]
        level = int(w0["level"])
        sub, subdesc = _probes(s.win[ks], desc, targets)
        r, lo, hi = wm.fuse_window(1.0, _table(level, w0["r"]), level)
        lists = [wm.features_in_area(s.kp, s.bounds, w["x"], w["y"], r, lo, hi, s.grid) for w in s.win[ks]]
        _same(_fuse(uvo, matcher, s.kp, desc, s.bounds, sub, subdesc, 1.0, _table(level, w0["r"])), _expect(lists, targets)[:2], "%s through uvo_fuse" % s.name)
        inside = [li if _in_image(s.bounds, w) else [] for li, w in zip(lists, s.win[ks])]
        _same(_fuse_batch(uvo, matcher, s.kp, desc, s.bounds, sub, subdesc, w0["r"], level + 1), _expect(inside, targets)[:2], "%s through uvo_fuse_batch" % s.name)
        first = np.array([li[0] if len(li) else -1 for li in inside])
        _same(_fuse_batch(uvo, matcher, s.kp, zeros, s.bounds, s.win[ks], qz[:len(ks)], w0["r"], level + 1), (first, np.where(first >= 0, 0, -1)),
              "%s firsts through uvo_fuse_batch" % s.name)


# ---- d. non-finite input -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("entry", ["windows", "fuse", "fuse_batch", "sbp", "kf"])
def test_nonfinite_input(uvo, matcher, scenes, entry):
    """A key point with a NaN or infinite coordinate is in no cell, so no window finds it; a query whose centre or radius is NaN or
    infinite finds nothing.  (The membership tests above run this scene too; this one says what must hold without the model: the
    answer is written out.)"""
    s = scenes["nonfinite"]
    desc = wm.hadamard_descriptors(s.n)
    bad = set(s.planted["nan"] + s.planted["inf"])
    finite_w, bad_w = s.which("finite"), s.which("nonfinite")
    found = {k: set() for k in range(len(s.win))}
    if entry == "windows":
        q, qdesc = _probes(s.win, desc, np.arange(s.n))
        match, _, _ = _match_windows(uvo, matcher, s.kp, desc, s.bounds, q, qdesc)
        for k, row in enumerate(match.reshape(len(s.win), s.n)):
            found[k] = set(int(t) for t in row[row >= 0])
    else:
        for k, w in enumerate(s.win):
            one, level = s.win[[k]], int(w["level"])
            q, qdesc = _probes(one, desc, np.arange(s.n))
            if entry == "fuse":
                got = _fuse(uvo, matcher, s.kp, desc, s.bounds, q, qdesc, *_th_params(k, w))[0]
            elif entry == "fuse_batch":
                if not (np.isfinite(w["x"]) and np.isfinite(w["y"])):
                    continue                                            # fails KeyFrame::IsInImage before the search: nothing to show here
                got = _fuse_batch(uvo, matcher, s.kp, desc, s.bounds, q, qdesc, w["r"], level + 1)[0]
            elif entry == "sbp":
                got = _sbp(uvo, matcher, s.kp, desc, s.bounds, w, desc, *_sbp_params(k, w), np.full(s.n, -1, np.int32))[0]
            else:
                got = _sbp_kf(uvo, matcher, s.kp, desc, s.bounds, w, desc, *_th_params(k, w), np.full(s.n, -1, np.int32))[0]
            assert ((got == -1) | (got == np.arange(s.n))).all()
            found[k] = set(int(t) for t in np.nonzero(got >= 0)[0])
    for k in finite_w:
        assert found[k] and not (found[k] & bad), "window %s finds the key points %s that are in no cell" % (s.win[k], sorted(found[k] & bad))
    for k in bad_w:
        assert not found[k], "query %s finds %s" % (s.win[k], sorted(found[k]))


# ---- e. the rotation filter ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(rot.cases()))
def test_rotation_filter(uvo, matcher, name):
    """k_rot_filter alone: uvo_match_groups with check_orientation, every query with one candidate at distance 0 (query i -> target i),
    so that the outcome is the filter's.  Every third query of the larger cases has no candidate at all."""
    rots = rot.cases()[name]
    qa, ta = rot.from_rots(rots)
    nq = len(rots)
    has = np.ones(nq, bool) if nq < 40 else (np.arange(nq) % 3 != 2) | (np.arange(nq) >= nq - 2)
    start = np.concatenate([[0], np.cumsum(has)]).astype(np.int32)
    idx = np.ascontiguousarray(np.nonzero(has)[0], np.int32)
    desc = np.ascontiguousarray(wm.random_descriptors(nq))
    before = np.where(has, np.arange(nq), -1)
    want = rot.rot_filter(before, np.where(has, 0, -1), qa, ta)[:3]
    match, dist = np.full(nq + PAD, M_FILL, np.int32), np.full(nq + PAD, D_FILL, np.int32)
    nm = ctypes.c_int(N_FILL)
    rule = uvo.MatchRule(RULE_BEST_ONLY, 0, 0.0, 0, 1)
    rc = uvo.lib.uvo_match_groups(matcher._h, nq, _p(desc), _p(qa), nq, _p(desc), _p(ta), None, None, _p(start), _p(idx), None, ctypes.byref(rule),
                                  _p(match), _p(dist), ctypes.byref(nm))
    assert rc == 0, uvo.last_error()
    assert (match[nq:] == M_FILL).all() and (dist[nq:] == D_FILL).all()
    _same((match[:nq], dist[:nq], nm.value), want, name)
    # and without the filter every candidate is the match: what the comparison above shows is the filter's doing
    rule = uvo.MatchRule(RULE_BEST_ONLY, 0, 0.0, 0, 0)
    rc = uvo.lib.uvo_match_groups(matcher._h, nq, _p(desc), None, nq, _p(desc), None, None, None, _p(start), _p(idx), None, ctypes.byref(rule),
                                  _p(match), _p(dist), ctypes.byref(nm))
    assert rc == 0, uvo.last_error()
    _same((match[:nq], dist[:nq], nm.value), (before, np.where(has, 0, -1), int(has.sum())), name + " unfiltered")


def test_rotation_filter_without_matches(uvo, matcher):
    """no query has a candidate: nothing to bin, nothing kept, n_matches 0"""
    nq = 37
    desc = np.ascontiguousarray(wm.random_descriptors(nq))
    ang = np.linspace(0, 359, nq).astype(f32)
    start = np.zeros(nq + 1, np.int32)
    match, dist = np.full(nq + PAD, M_FILL, np.int32), np.full(nq + PAD, D_FILL, np.int32)
    nm = ctypes.c_int(N_FILL)
    rule = uvo.MatchRule(RULE_BEST_ONLY, 0, 0.0, 0, 1)
    rc = uvo.lib.uvo_match_groups(matcher._h, nq, _p(desc), _p(ang), nq, _p(desc), _p(ang), None, None, _p(start), None, None, ctypes.byref(rule),
                                  _p(match), _p(dist), ctypes.byref(nm))
    assert rc == 0, uvo.last_error()
    assert (match[nq:] == M_FILL).all() and (match[:nq] == -1).all() and (dist[:nq] == -1).all() and nm.value == 0
