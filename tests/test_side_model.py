"""The numpy models of tests/side_model.py against the C++ oracle, on the case lists tests/test_gpu_side.py runs against the kernels:
bit equality (NaN compared as "NaN on both sides"), and every constructed case is what its name says.  No GPU."""
import numpy as np
import pytest

import side_cases as sc
import side_model as sm
from side_model import same_bow, same_floats


# ---- CLAHE ---------------------------------------------------------------------------------------------------------------
def test_clahe_model_against_the_oracle(oracle):
    n = 0
    for name, img, clip, tiles in sc.clahe_cases():
        np.testing.assert_array_equal(sm.clahe(img, clip, tiles), oracle.clahe(img, clip, tiles), err_msg=name)
        n += 1
    assert n == len(sc.CLAHE_GEOMETRIES) * len(sc.CLAHE_CLIPS) * len(sc.CLAHE_IMAGES)


def test_clahe_geometries_are_what_they_claim():
    padded = {(w, h, t): (w % t[0] != 0, h % t[1] != 0) for w, h, t in sc.CLAHE_GEOMETRIES}
    assert padded[(96, 64, (8, 8))] == (False, False) and padded[(97, 61, (4, 4))] == (True, True)
    assert padded[(96, 61, (4, 4))] == (False, True) and padded[(97, 64, (4, 4))] == (True, False)
    # 12-pixel tiles: int(4.0 * 12 / 256) = 0, clamped to 1
    assert sm.clahe_clipped_count(sc.clahe_image("uniform", 24, 16), 4.0, (8, 4))[1] == 1
    # the single tile at clip 4: 192 pixels per bin, and an ordinary image already has a batch to spread
    clipped, limit = sm.clahe_clipped_count(sc.clahe_image("bimodal", 128, 96), 4.0, (1, 1))
    assert limit == 192 and clipped[0, 0] // 256 > 0


def test_residual_classes_occur_and_match_the_oracle(oracle):
    steps = set()
    for name, img, clip, limit, want in sc.residual_cases():
        h, w = img.shape
        clipped, lim = sm.clahe_clipped_count(img, clip, (1, 1))
        assert lim == limit and clipped[0, 0] == want, name
        hist = np.bincount(img.ravel(), minlength=256)
        assert (np.delete(hist, 7) < limit).all(), name
        r = want % 256
        steps.add(max(256 // r, 1))
        np.testing.assert_array_equal(sm.clahe(img, clip, (1, 1)), oracle.clahe(img, clip, (1, 1)), err_msg=name)
    assert steps == {256, 128, 85, 3, 2, 1}
    assert any(c // 256 > 0 for _, _, _, _, c in sc.residual_cases())


# ---- undistortion --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("camera", sorted(sc.CAMERAS))
def test_undistort_model_against_the_oracle(oracle, camera):
    fx, fy, cx, cy, dist, fisheye = sc.CAMERAS[camera]
    pts = sc.undistort_points()
    for n in sc.UNDISTORT_COUNTS:
        ref = oracle.undistort_points(pts[:n], np.float32(fx), np.float32(fy), np.float32(cx), np.float32(cy), dist, fisheye)
        got = sm.undistort(pts[:n], fx, fy, cx, cy, dist, fisheye)
        assert same_floats(got, ref, np.uint32), (camera, n, np.argwhere(got.view(np.uint32) != ref.view(np.uint32))[:5])


def test_undistort_cases_are_what_they_claim():
    pts = sc.undistort_points()
    assert len(pts) == 2 * sc.KLT_MAX_POINTS and np.isnan(pts).any() and np.isposinf(pts).any() and np.isneginf(pts).any()
    for name in ("harbor_fisheye", "fisheye_none", "fisheye1", "fisheye_unsettled"):
        fx, fy, cx, cy, _, _ = sc.CAMERAS[name]
        assert sm.fisheye_clamped(pts, fx, fy, cx, cy).mean() > 0.5, name
    # the small-theta branch, off the principal point; and points between the kernel's 1e-8 and a slip to 1e-6
    fx, fy, cx, cy, dist, _ = sc.CAMERAS["fisheye_origin"]
    theta_d = np.hypot((pts[:, 0].astype(np.float64) - cx) / fx, (pts[:, 1].astype(np.float64) - cy) / fy)
    assert ((theta_d > 0) & (theta_d <= 1e-8)).sum() >= 2 and ((theta_d > 1e-8) & (theta_d < 1e-6)).sum() >= 4
    # the unsettled model takes all ten Newton steps somewhere: a ninth-step result differs from the tenth
    fx, fy, cx, cy, dist, _ = sc.CAMERAS["fisheye_unsettled"]
    a = sm.undistort(pts, fx, fy, cx, cy, dist, True)
    theta = np.fmin(np.hypot((pts[:, 0].astype(np.float64) - cx) / fx, (pts[:, 1].astype(np.float64) - cy) / fy), np.pi / 2)
    k = np.zeros(4)
    k[:len(dist)] = np.asarray(dist, np.float32)
    t, steps, live = theta.copy(), np.zeros(len(theta), int), np.isfinite(theta) & (theta > 1e-8)
    with np.errstate(all="ignore"):
        for _ in range(10):
            t2 = t * t
            fix = (t * (1 + k[0] * t2 + k[1] * t2 ** 2 + k[2] * t2 ** 3 + k[3] * t2 ** 4) - theta) / (1 + 3 * k[0] * t2 + 5 * k[1] * t2 ** 2 + 7 * k[2] * t2 ** 3 + 9 * k[3] * t2 ** 4)
            t = np.where(live, t - fix, t)
            steps += live
            live = live & ~(np.abs(fix) < 1e-8)
    assert (steps == 10).sum() > 10 and live.sum() > 10 and np.isfinite(a[live]).all()


# ---- BoW transform -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("branching", sc.BRANCHINGS, ids=str)
def test_bow_model_against_the_oracle(oracle, branching):
    voc = sc.build_vocabulary(branching, len(branching))
    L = voc["L"]
    cases = 0
    for n in sc.BOW_COUNTS:
        feats = sc.bow_features(voc, n, n)
        for levelsup in sc.bow_levelsups(L):
            descent = sm.bow_descend(voc, feats, levelsup)
            for weighting in sc.WEIGHTINGS:
                for normalize in sc.NORMALIZES:
                    v = sc.with_scoring(voc, weighting, normalize)
                    assert same_bow(sm.bow_transform(v, feats, levelsup, descent), oracle.bow_transform(v, feats, levelsup)), (n, levelsup, weighting, normalize)
                    cases += 1
    assert cases == len(sc.BOW_COUNTS) * 5 * 12


def test_bow_vocabularies_are_what_they_claim():
    voc = sc.build_vocabulary([10, 10, 10], 3)
    feats = sc.bow_features(voc, 130, 130)
    leaf, _ = sm.bow_descend(voc, feats, 0)
    depth = voc["level"][leaf][:128].reshape(-1, 4)
    assert (depth.min(1) != depth.max(1)).any(), "no group of four consecutive features ends at different depths"
    for b in ([17, 2], [33, 5], [100], [3, 1, 40]):
        v = sc.build_vocabulary(b, len(b))
        assert np.diff(v["child_start"]).max() > 16                     # a second trip of the lanes' loop
    v = sc.build_vocabulary([16, 3], 2)
    dup = sum(1 for i in range(len(v["child_start"]) - 1) for c in [v["descriptor"][v["children"][v["child_start"][i]:v["child_start"][i + 1]]]]
              if len(c) > 1 and len({x.tobytes() for x in c}) < len(c))
    assert dup > 0
    assert (voc["weight"][voc["word_id"] >= 0] == 0).any() and (voc["weight"][leaf] == 0).any()      # stop words exist and are reached
    assert len(sc.build_vocabulary([], 0)["child_start"]) == 2


@pytest.mark.parametrize("name", sorted(sc.tie_trees()))
def test_tie_trees_in_model_and_oracle(oracle, name):
    voc, feats, want = sc.tie_trees()[name]
    kids = voc["descriptor"][1:]
    d = sm._POP[feats[:, None, :] ^ kids[None, :, :]].sum(-1)
    assert ((d == d.min(1, keepdims=True)).sum(1) >= 2).all()            # the tie is real for every feature
    g, o = sm.bow_transform(voc, feats, 0), oracle.bow_transform(voc, feats, 0)
    assert (g[0] == want).all() and same_bow(g, o)


def test_stop_word_vocabulary_gives_empty_containers(oracle):
    voc = sc.stop_word_vocabulary()
    feats = sc.bow_features(voc, 40, 1)
    for weighting in sc.WEIGHTINGS:
        for normalize in sc.NORMALIZES:
            v = sc.with_scoring(voc, weighting, normalize)
            g = sm.bow_transform(v, feats, 1)
            assert len(g[3][0]) == 0 and g[4] == {} and same_bow(g, oracle.bow_transform(v, feats, 1))


def test_bad_vocabularies_list_a_node_twice():
    for name, (cs, ch, mended_cs, mended_ch) in sc.bad_vocabularies().items():
        n = len(cs) - 1
        for a, b in ((cs, ch), (mended_cs, mended_ch)):
            assert len(a) == n + 1 and a[0] == 0 and a[-1] == len(b) and all(0 < c < n for c in b) and all(np.diff(a) >= 0), name
        assert len(set(ch)) < len(ch) and len(set(mended_ch)) == len(mended_ch), name


@pytest.mark.parametrize("name", sorted(sc.bad_vocabularies()))
def test_vocabulary_create_refuses_a_repeated_node_before_it_asks_for_a_device(uvo, name):
    """The check is host code ahead of the device query, so it is held here too: UVO_E_BADARG for the bad description, and for the
    same nodes as a tree whatever a box without a GPU answers (UVO_E_NODEVICE) or success."""
    import ctypes
    cs, ch, mended_cs, mended_ch = (np.asarray(a, np.int32) for a in sc.bad_vocabularies()[name])
    n = len(cs) - 1
    desc, word, weight = np.zeros((n, 32), np.uint8), np.arange(n, dtype=np.int32), np.ones(n)
    h = ctypes.c_void_p()
    d = uvo.VocabularyDesc(n, cs.ctypes.data, ch.ctypes.data, desc.ctypes.data, word.ctypes.data, weight.ctypes.data, 2, 0, 1, 0)
    assert uvo.lib.uvo_vocabulary_create(ctypes.byref(d), ctypes.byref(h)) == uvo.UVO_E_BADARG and not h.value
    d = uvo.VocabularyDesc(n, mended_cs.ctypes.data, mended_ch.ctypes.data, desc.ctypes.data, word.ctypes.data, weight.ctypes.data, 2, 0, 1, 0)
    rc = uvo.lib.uvo_vocabulary_create(ctypes.byref(d), ctypes.byref(h))
    assert rc in (uvo.UVO_OK, uvo.UVO_E_NODEVICE)
    if rc == uvo.UVO_OK:
        uvo.lib.uvo_vocabulary_destroy(h)


# ---- haloc ---------------------------------------------------------------------------------------------------------------
def test_haloc_model_against_the_oracle(oracle):
    seen = {}
    for name, proj, desc in sc.haloc_cases():
        got, ref = sm.haloc_hash(proj, desc), oracle.haloc_hash(proj, desc)
        assert same_floats(got, ref, np.uint32), name
        seen[name] = got
    assert len(seen) == len(sc.HALOC_COUNTS) * len(sc.HALOC_PROJS) + 3
    tiny = np.finfo(np.float32).tiny
    sub = seen["subnormal"]
    assert ((sub != 0) & (np.abs(sub) < tiny)).any(), "no subnormal output"
    assert np.isnan(seen["inf"]).any() and np.isinf(seen["inf"]).any()       # inf * 0 in the all-zero column, inf elsewhere
    assert not any(np.isnan(v).any() for k, v in seen.items() if k != "inf"), "a NaN from the padding columns"
    # the cancellation case loses what a float64 sum keeps: its result is set by the order of the additions
    _, proj, desc = [c for c in sc.haloc_cases() if c[0] == "cancel"][0]
    exact = (proj[:, :300].astype(np.float64) @ desc.astype(np.float64) / 300).reshape(-1)
    with np.errstate(all="ignore"):
        assert (np.abs(seen["cancel"] - exact) > 1e-7 * np.abs(exact)).any()
