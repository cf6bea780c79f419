"""tests/window_model.py and tests/rotation_model.py against the oracle (the lists must agree exactly, order included), and the proof
that every scene tests/test_gpu_windows.py runs holds the edges it is named for -- so that no GPU test passes on a vacuous scene."""
import numpy as np
import pytest

import rotation_model as rot
import window_model as wm

f32 = np.float32


@pytest.fixture(scope="module")
def scenes():
    s = {b: wm.edge_scene(b) for b in wm.EDGE_BOUNDS}
    s["nonfinite"], s["one_cell"] = wm.nonfinite_scene(), wm.one_cell_scene()
    return s


def _all_scenes(scenes):
    return list(scenes.values()) + [wm.big_scene(4096), wm.big_scene(4097)]


def test_model_against_oracle_on_every_scene(oracle, scenes):
    """every window of every scene, under its own level rule and under the rules of the projection searches"""
    for s in _all_scenes(scenes):
        for layer in ("generic", "fuse", "kf"):
            lists = s.lists(layer)
            for w, want in zip(s.win, lists):
                lo, hi = {"generic": (w["lo"], w["hi"]), "fuse": (w["level"] - 1, w["level"]), "kf": (w["level"] - 1, w["level"] + 1)}[layer]
                got = oracle.features_in_area(s.kp, s.bounds, w["x"], w["y"], w["r"], int(lo), int(hi))
                np.testing.assert_array_equal(got, want, err_msg="%s %s window %s" % (s.name, layer, w))


def test_model_against_oracle_on_random_windows(oracle):
    """the rounding of the cell and of the window borders, where draws are dense: centres and radii anywhere, also outside the frame"""
    rng = np.random.default_rng(3)
    for bounds in wm.EDGE_BOUNDS:
        s = wm.edge_scene(bounds)
        W, H = bounds[2] - bounds[0], bounds[3] - bounds[1]
        for k in range(600):
            x, y = rng.uniform(bounds[0] - 0.2 * W, bounds[2] + 0.2 * W), rng.uniform(bounds[1] - 0.2 * H, bounds[3] + 0.2 * H)
            r = (0.0, 1.0, rng.uniform(0, 60), rng.uniform(0, 400))[k % 4]
            lo, hi = wm.LEVEL_FORMS[k % 5]
            got = oracle.features_in_area(s.kp, bounds, f32(x), f32(y), f32(r), lo, hi)
            np.testing.assert_array_equal(got, wm.features_in_area(s.kp, bounds, x, y, r, lo, hi, s.grid))


@pytest.mark.parametrize("bounds", wm.EDGE_BOUNDS)
def test_cell_rounding_against_oracle(oracle, bounds):
    """PosInGrid alone: a key point is in the list of the window that covers everything exactly when the model gives it a cell;
    coordinates on and next to every x.5 product"""
    inv_w, inv_h = wm.inv_cell(bounds)
    xs = []
    for k in range(-2, 66):
        c = f32(bounds[0] + (k + 0.5) / float(inv_w))
        xs += [c, np.nextafter(c, f32(np.inf)), np.nextafter(c, f32(-np.inf))]
    ys = []
    for k in range(-2, 50):
        c = f32(bounds[1] + (k + 0.5) / float(inv_h))
        ys += [c, np.nextafter(c, f32(np.inf)), np.nextafter(c, f32(-np.inf))]
    kp = np.zeros(len(xs) + len(ys), wm.KP)
    kp["x"] = xs + [f32(bounds[0] + 20.3 / float(inv_w))] * len(ys)
    kp["y"] = [f32(bounds[1] + 20.3 / float(inv_h))] * len(xs) + ys
    ok, ix, iy, _, _ = wm.cell_of(kp, bounds)
    got = oracle.features_in_area(kp, bounds, (bounds[0] + bounds[2]) / 2, (bounds[1] + bounds[3]) / 2, 1e6, -1, -1)
    want = np.nonzero(ok)[0]
    np.testing.assert_array_equal(got, want[np.lexsort((want, iy[want], ix[want]))])
    assert 0 < ok.sum() < len(kp)


@pytest.mark.parametrize("bounds", wm.EDGE_BOUNDS)
def test_edge_scene_holds_its_edges(scenes, bounds):
    s = scenes[bounds]
    ok, ix, iy, pu, pv = s.grid
    u, v = wm.grid_products(s.kp, bounds)
    assert 300 <= s.n <= 400 and 55 <= len(s.win) <= 70
    # cells 64, 48 and -1, and the last / first cell next to them
    assert (pu[s.planted["cell64"]] == 64).all() and (pv[s.planted["cell48"]] == 48).all()
    c = s.planted["cell-1"]
    assert pu[c[0]] == -1 or pv[c[0]] == -1
    assert ((pu[c] == -1) | (pv[c] == -1)).all() and (pu[c] == -1).any() and (pv[c] == -1).any()
    for t in ("cell64", "cell48", "cell-1"):
        assert not ok[s.planted[t]].any()
    assert (ix[s.planted["last_cell"]] == 63).all() and (iy[s.planted["last_cell"]] == 47).all()
    assert (ix[s.planted["first_cell"]] == 0).all() and (iy[s.planted["first_cell"]] == 0).all() and (u[s.planted["first_cell"]] < 0).all()
    # exact ties: a product of exactly k + 0.5 (every bounds admits some; the cell sizes that are powers of two admit all, -0.5 included)
    ties = s.planted["tie"]
    frac = [(float(u[i]) % 1.0 == 0.5) or (float(v[i]) % 1.0 == 0.5) for i in ties]
    assert len(ties) >= 1 and all(frac)
    if bounds in ((0, 0, 512, 384), (0, 0, 64, 48)):
        assert len(ties) == 8
        assert any(u[i] == -0.5 and pu[i] == -1 for i in ties) and any(v[i] == -0.5 and pv[i] == -1 for i in ties)
        assert any(u[i] == 63.5 and pu[i] == 64 for i in ties) and any(u[i] == 17.5 and ix[i] == 18 for i in ties)
    # boundary windows: a member at |dx| == r or |dy| == r exactly that the model accepts, its nextafter neighbour that it rejects
    # for no other reason than the distance
    lists = s.lists()
    for wi in s.which("boundary"):
        w = s.win[wi]
        r = float(w["r"])
        on, off = s.planted["on:%g" % r], s.planted["off:%g" % r]
        cells, _ = wm.window(bounds, w["x"], w["y"], w["r"])
        pairs = 0
        for a in on:
            d = max(abs(s.kp["x"][a] - w["x"]), abs(s.kp["y"][a] - w["y"]))
            assert d == w["r"]
            if a not in lists[wi]:
                assert not ok[a]                                        # only a member outside the grid is missing
                continue
            for b in off:
                db = max(abs(s.kp["x"][b] - w["x"]), abs(s.kp["y"][b] - w["y"]))
                near = abs(s.kp["x"][b] - s.kp["x"][a]) <= abs(s.kp["x"][a]) * 2e-7 + 1e-44 and \
                    abs(s.kp["y"][b] - s.kp["y"][a]) <= abs(s.kp["y"][a]) * 2e-7 + 1e-44
                if near and db > w["r"] and ok[b] and cells[0] <= ix[b] <= cells[1] and cells[2] <= iy[b] <= cells[3] and \
                        wm.level_mask(s.kp["octave"][[b]], int(w["lo"]), int(w["hi"]))[0]:
                    assert b not in lists[wi]
                    pairs += 1
        assert pairs >= 1, "boundary window r = %g has no accepted member with a rejected neighbour" % r
    # the four early returns, and windows partly outside
    for side in ("right", "left", "bottom", "top"):
        (wi,) = s.which("early:" + side)
        w = s.win[wi]
        assert wm.window(bounds, w["x"], w["y"], w["r"]) == (None, side)
    for wi in s.which("corner"):
        w = s.win[wi]
        cells, _ = wm.window(bounds, w["x"], w["y"], w["r"])
        assert cells is not None and (cells[0] == 0 or cells[1] == 63) and (cells[2] == 0 or cells[3] == 47)
    # column runs of exactly 7, 8, 9 and 17 items, every item of them in the list
    for length in wm.RUN_LENGTHS:
        (wi,) = s.which("run:%d" % length)
        w = s.win[wi]
        runs = wm.column_runs(s.kp, bounds, w["x"], w["y"], w["r"], s.grid)
        assert sorted(runs)[-1] == length and sum(runs) == length, (length, runs)
        assert sorted(lists[wi]) == s.planted["run:%d" % length]
        assert len(set(iy[lists[wi]])) >= 2
    # one cell whose key points' index order differs from their position order
    c = s.planted["one_cell"]
    assert len(set(zip(ix[c], iy[c]))) == 1 and len(c) == 6
    assert list(np.argsort(s.kp["x"][c], kind="stable")) != list(range(6)) and list(np.argsort(s.kp["y"][c], kind="stable")) != list(range(6))
    (wi,) = s.which("one_cell")
    assert [i for i in lists[wi] if i in c] == c
    # the clusters of the order tests: at most 24 candidates over two columns and two rows at least, index order not visiting order,
    # and no key point in two of them
    seen = set()
    for wi in s.which("order"):
        for layer in ("generic", "fuse", "kf"):
            li = s.lists(layer)[wi]
            assert 12 <= len(li) <= 24 and len(set(ix[li])) >= 2 and len(set(iy[li])) >= 2
            assert list(li) != sorted(li)
        assert not (seen & set(s.lists("kf")[wi]))
        seen |= set(s.lists("kf")[wi])
    # every form of the level rule among the windows, and radius 0 that finds its key point
    assert {(int(w["lo"]), int(w["hi"])) for w in s.win} >= set(wm.LEVEL_FORMS)
    assert any(len(lists[wi]) > 0 and s.win[wi]["r"] == 0 for wi in range(len(s.win)))
    assert {0.0, 1.0, 7.5, 40.0, wm.BIG} <= {float(r) for r in s.win["r"]}


def test_at_least_a_quarter_of_the_windows_find_something(scenes):
    for s in _all_scenes(scenes):
        for layer in ("generic", "fuse", "kf"):
            n = sum(len(li) > 0 for li in s.lists(layer))
            assert 4 * n >= len(s.win), (s.name, layer, n, len(s.win))


def test_nonfinite_scene(oracle, scenes):
    """a key point with a NaN or infinite coordinate is in no cell and in no list; a query with a NaN or infinite centre or radius
    returns nothing -- the model's statement, which is the oracle's"""
    s = scenes["nonfinite"]
    ok = s.grid[0]
    bad = s.planted["nan"] + s.planted["inf"]
    assert len(s.planted["nan"]) == 7 and not ok[bad].any() and ok[s.planted["finite"]].all()
    lists = s.lists()
    for wi in s.which("finite"):
        assert len(lists[wi]) > 0 and not set(lists[wi]) & set(bad)
    assert len(s.which("nonfinite")) == 11
    for wi in s.which("nonfinite"):
        w = s.win[wi]
        assert len(lists[wi]) == 0 and wm.window(s.bounds, w["x"], w["y"], w["r"]) == (None, "nonfinite")
        assert len(oracle.features_in_area(s.kp, s.bounds, w["x"], w["y"], w["r"], -1, -1)) == 0
    # the scene would show a conversion that turns NaN into 0: the first cells are populated and reached
    assert (s.grid[1][s.planted["finite"]] == 0).any() and (s.grid[2][s.planted["finite"]] == 0).any()


def test_one_cell_and_big_scenes(scenes):
    s = scenes["one_cell"]
    assert len(set(zip(s.grid[1], s.grid[2]))) == 1 and s.grid[0].all()
    assert max(len(li) for li in s.lists()) == s.n
    for n in (4096, 4097):
        b = wm.big_scene(n)
        assert b.n == n and 0 < (~b.grid[0]).sum() < n // 10
        desc = wm.random_descriptors(n)
        sample = wm.big_targets(b)
        assert len(sample) == 64 == len(set(sample)) and sum(len(set(li) & set(sample)) for li in b.lists()) >= 80
        D = wm.hamming(desc[sample], desc)
        D[np.arange(64), sample] = 999
        assert D.min() > 50                                             # a probe for one of the sampled rows matches no other row


def test_hadamard_descriptors_are_far_apart():
    d = wm.hadamard_descriptors(512)
    D = wm.hamming(d, d)
    assert set(np.unique(D)) == {0, 128, 256} and (np.diag(D) == 0).all() and (D == 0).sum() == 512


def test_radius_helpers():
    """the comparison with 0.998 is made in double: float32(0.998) is above it; `th != 1` decides whether th multiplies"""
    sf = np.array([1.0, 1.2, 1.44], f32)
    above, below = f32(0.998), np.nextafter(f32(0.998), f32(0))
    assert float(above) > 0.998 > float(below)
    assert wm.sbp_window(above, 1.0, sf, 0) == (f32(2.5), -1, 0) and wm.sbp_window(below, 1.0, sf, 0) == (f32(4.0), -1, 0)
    assert wm.sbp_window(above, 3.0, sf, 1) == (f32(f32(7.5) * f32(1.2)), 0, 1) and wm.sbp_window(below, 3.0, sf, 2) == (f32(f32(12) * f32(1.44)), 1, 2)
    assert wm.sbp_kf_window(3.0, sf, 1) == (f32(f32(3) * f32(1.2)), 0, 2) and wm.fuse_window(3.0, sf, 1) == (f32(f32(3) * f32(1.2)), 0, 1)


# ---- the rotation filter ----------------------------------------------------------------------------------------------------------

def test_three_maxima_against_oracle(oracle):
    rng = np.random.default_rng(5)
    for k in range(3000):
        top = (1, 2, 3, 10, 30, 100)[k % 6]
        h = rng.integers(0, top + 1, 30)
        if k % 4 == 0:
            h[rng.integers(0, 30, 20)] = 0
        if k % 7 == 0:
            h[rng.integers(0, 30)] = 10 * top
        assert rot.compute_three_maxima(h) == oracle.compute_three_maxima(h), h
    for name, rots in rot.cases().items():
        qa, ta = rot.from_rots(rots)
        n = len(rots)
        _, _, _, hist, keep = rot.rot_filter(np.arange(n), np.zeros(n), qa, ta)
        assert keep == oracle.compute_three_maxima(hist), name


def test_rotation_cases_hold_what_they_are_named_for():
    c = rot.cases()
    res = {}
    for name, rots in c.items():
        qa, ta = rot.from_rots(rots)
        n = len(rots)
        res[name] = rot.rot_filter(np.arange(n), np.zeros(n), qa, ta)
    b = lambda r: rot.bin_of(*[a[0] for a in rot.from_rots([r])])
    # x.5 products round away from zero: 15 -> bin 1, 45 -> 2, 345 -> 12; the wrap; 360 from the smallest negative difference
    assert [b(15.0), b(45.0), b(345.0), b(0.0), b(-15.0), b(-345.0)] == [1, 2, 12, 0, 12, 1]
    products = [float(f32(r) * rot.FACTOR) for r in c["ties_15_45_345"]]
    assert {0.5, 1.5, 11.5} <= set(products) and float(f32(15.0) * rot.FACTOR) == 0.5
    assert b(np.nextafter(f32(45.0), f32(0))) == 2 and b(np.nextafter(f32(15.0), f32(0))) == 1       # their float32 products are 1.5 and 0.5
    tiny = c["zero_and_smallest_negative"][3]
    assert tiny < 0 and rot.rot_of(*[a[0] for a in rot.from_rots([tiny])]) == f32(360.0) and b(tiny) == 12
    assert np.isnan(c["nan_difference"][:3]).all() and b(float("nan")) == -2
    assert (res["nan_difference"][0][:3] == -1).all() and res["nan_difference"][2] == 7
    hist = lambda name: sorted((v for v in res[name][3] if v), reverse=True)
    assert hist("three_equal_bins") == [6, 6, 6] and res["three_equal_bins"][4] == [4, 7, 11] and res["three_equal_bins"][2] == 18
    assert hist("four_equal_bins") == [5, 5, 5, 5] and res["four_equal_bins"][4] == [2, 5, 9] and res["four_equal_bins"][2] == 15
    assert hist("tie_for_third") == [9, 7, 4, 4] and res["tie_for_third"][4] == [3, 8, 10]
    assert hist("tie_for_first") == [8, 8, 3] and res["tie_for_first"][4] == [6, 9, 12]
    assert hist("ten_percent_kept") == [20, 2, 2, 1] and res["ten_percent_kept"][4] == [5, 8, 12] and res["ten_percent_kept"][2] == 24
    assert res["ten_percent_third_dropped"][4] == [5, 12, -1] and res["ten_percent_second_dropped"][4] == [5, -1, -1]
    assert res["thirty_and_three"][4] == [0, 6, 12] and res["thirty_and_three"][2] == 36
    assert res["one_bin"][4] == [10, -1, -1] and res["one_bin"][2] == 9 and res["nq_1"][2] == 1
    assert len(c["nq_1024"]) == 1024 and len(c["nq_1025"]) == 1025 and res["nq_1025"][2] == 900
