"""CLAHE, undistortion, the BoW transform and the haloc hash on the device against the numpy models of tests/side_model.py, at the
edges tests/test_gpu_parity.py never reaches: loose strides with sentinels, tiles of a few pixels, the residual classes of the clip
redistribution, the fisheye clamp and its unsettled Newton steps, all eight pin-hole coefficients, non-finite points, vocabularies with
more than 16 children per node and ties between the lanes, every weighting x normalisation, exact capacities, padded projections,
subnormal and cancelling sums.  The cases are tests/side_cases.py; tests/test_side_model.py holds the models to the oracle on them.

Every comparison is on raw bits (a NaN equals any NaN): the CLAHE and BoW kernels are integer plus a few float32 operations in a fixed
order, the library is built without FMA contraction, with correctly rounded fp32 division and with denormals kept, and k_undistort is
IEEE double arithmetic except for tan().  For the fisheye model alone a device result that is a float32 neighbour of the model's is
let through, for at most 0.1 % of a camera's points, and counted: a few double ulps in tan() cannot move the rounded float further."""
import ctypes

import numpy as np
import pytest

import side_cases as sc
import side_model as sm
from side_model import same_bow, same_floats

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ex(uvo):
    e = uvo.ORBextractor(100, 1.2, 2, 0, 20, max_width=sc.CLAHE_MAX_W, max_height=sc.CLAHE_MAX_H, max_batch=sc.CLAHE_MAX_BATCH)
    yield e
    e.close()


@pytest.fixture(scope="module")
def klt(uvo):
    k = uvo.KLT(128, 96, (21, 21), 2, max_points=sc.KLT_MAX_POINTS, slots=2)
    yield k
    k.close()


@pytest.fixture(scope="module")
def matcher(uvo):
    m = uvo.ORBmatcher(0.8)
    yield m
    m.close()


# ---- CLAHE ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geometry", sc.CLAHE_GEOMETRIES, ids=lambda g: "%dx%d_%dx%d" % (g[0], g[1], g[2][0], g[2][1]))
def test_clahe_geometry(ex, geometry):
    """Every clip limit x image kind on one geometry."""
    w, h, tiles = geometry
    gi = sc.CLAHE_GEOMETRIES.index(geometry)
    for clip in sc.CLAHE_CLIPS:
        for ki, kind in enumerate(sc.CLAHE_IMAGES):
            img = sc.clahe_image(kind, w, h, 10 * gi + ki)
            np.testing.assert_array_equal(ex.clahe(img, clip, tiles), sm.clahe(img, clip, tiles), err_msg="clip %g, %s" % (clip, kind))


def test_clahe_residual_classes(ex):
    """Clipped counts of exactly r and 256 + r pixels on one tile: the steps 256, 128, 85, 3, 2, 1 of the strided residual, with and
    without a batch; on a 256-pixel tile every single count of the redistribution moves the LUT."""
    n = 0
    for name, img, clip, _, _ in sc.residual_cases():
        np.testing.assert_array_equal(ex.clahe(img, clip, (1, 1)), sm.clahe(img, clip, (1, 1)), err_msg=name)
        n += 1
    assert n >= 2 * len(sc.RESIDUALS)


@pytest.mark.parametrize("geometry", [(97, 61, (4, 4)), (44, 30, (7, 4)), (128, 96, (1, 1))], ids=str)
def test_clahe_host_call_with_loose_strides(uvo, ex, geometry):
    """uvo_clahe with stride = w + 5 and dst_stride = w + 9: the input padding is never read into the result, the output padding comes
    back untouched."""
    w, h, tiles = geometry
    img = sc.clahe_image("skewed", w, h, 5)
    src = np.full((h, w + 5), 0xEE, np.uint8)
    src[:, :w] = img
    dst = np.full((h, w + 9), 0xA5, np.uint8)
    rc = uvo.lib.uvo_clahe(ex._h, src.ctypes.data, w, h, w + 5, 4.0, tiles[0], tiles[1], dst.ctypes.data, w + 9)
    assert rc == uvo.UVO_OK
    np.testing.assert_array_equal(dst[:, :w], sm.clahe(img, 4.0, tiles))
    assert (dst[:, w:] == 0xA5).all() and (src[:, w:] == 0xEE).all() and (src[:, :w] == img).all()


@pytest.mark.parametrize("geometry", [(97, 61, (4, 4)), (48, 40, (16, 2))], ids=str)
def test_clahe_batch_device_not_in_place_with_loose_strides(uvo, ex, geometry):
    """uvo_clahe_batch_device on three different frames, source and destination apart, all four strides loose: each frame equals its own
    model result (its own LUTs), and no byte between rows or frames is written."""
    import torch
    w, h, tiles = geometry
    B = 3
    stride, dst_stride = w + 5, w + 9
    frame_stride, dst_frame_stride = h * stride + 13, h * dst_stride + 21
    frames = [sc.clahe_image(kind, w, h, 40 + i) for i, kind in enumerate(("uniform", "skewed", "bimodal"))]
    src = np.full(B * frame_stride, 0xEE, np.uint8)
    for b in range(B):
        src[b * frame_stride:b * frame_stride + h * stride].reshape(h, stride)[:, :w] = frames[b]
    d_src = torch.from_numpy(src).cuda()
    d_dst = torch.full((B * dst_frame_stride,), 0xA5, dtype=torch.uint8, device="cuda")
    rc = uvo.lib.uvo_clahe_batch_device(ex._h, B, d_src.data_ptr(), w, h, stride, frame_stride, 4.0, tiles[0], tiles[1], d_dst.data_ptr(), dst_stride,
                                        dst_frame_stride)
    assert rc == uvo.UVO_OK
    ex.synchronize()
    dst = d_dst.cpu().numpy()
    written = np.zeros(len(dst), bool)
    for b in range(B):
        rows = dst[b * dst_frame_stride:b * dst_frame_stride + h * dst_stride].reshape(h, dst_stride)
        np.testing.assert_array_equal(rows[:, :w], sm.clahe(frames[b], 4.0, tiles), err_msg="frame %d" % b)
        written[b * dst_frame_stride:b * dst_frame_stride + h * dst_stride].reshape(h, dst_stride)[:, :w] = True
    assert (dst[~written] == 0xA5).all()
    np.testing.assert_array_equal(d_src.cpu().numpy(), src)


def test_clahe_refusals(uvo, ex):
    """Bad tile grids, batch sizes and strides are refused with UVO_E_BADARG, and nothing is written."""
    import torch
    lib = uvo.lib
    img = sc.clahe_image("uniform", 16, 16, 1)
    dst = np.full((16, 16), 0xA5, np.uint8)

    def host(w, h, stride, tiles, dst_stride=16):
        return lib.uvo_clahe(ex._h, img.ctypes.data, w, h, stride, 4.0, tiles[0], tiles[1], dst.ctypes.data, dst_stride)
    assert host(8, 8, 16, (9, 1)) == uvo.UVO_E_BADARG            # tiles_x > width
    assert host(8, 8, 16, (1, 9)) == uvo.UVO_E_BADARG
    assert host(5, 7, 16, (5, 4)) == uvo.UVO_E_BADARG            # 7 rows extended by 4 + the quirk's 5 columns: too coarse for REFLECT_101
    assert host(16, 16, 15, (4, 4)) == uvo.UVO_E_BADARG          # stride < width
    assert host(16, 16, 16, (4, 4), 15) == uvo.UVO_E_BADARG      # dst_stride < width
    assert host(16, 16, 16, (0, 4)) == uvo.UVO_E_BADARG
    assert (dst == 0xA5).all()
    d_src = torch.from_numpy(np.stack([img] * 4)).cuda()
    d_dst = torch.full((4, 16, 16), 0xA5, dtype=torch.uint8, device="cuda")

    def dev(batch, stride=16, dst_stride=16, tiles=(4, 4)):
        return lib.uvo_clahe_batch_device(ex._h, batch, d_src.data_ptr(), 16, 16, stride, 256, 4.0, tiles[0], tiles[1], d_dst.data_ptr(), dst_stride, 256)
    assert dev(0) == uvo.UVO_E_BADARG and dev(sc.CLAHE_MAX_BATCH + 1) == uvo.UVO_E_BADARG
    assert dev(1, stride=15) == uvo.UVO_E_BADARG and dev(1, dst_stride=15) == uvo.UVO_E_BADARG
    assert dev(1, tiles=(17, 4)) == uvo.UVO_E_BADARG
    ex.synchronize()
    assert bool((d_dst == 0xA5).all())
    assert dev(sc.CLAHE_MAX_BATCH) == uvo.UVO_OK                 # and the handle still works
    ex.synchronize()
    np.testing.assert_array_equal(d_dst[2].cpu().numpy(), sm.clahe(img, 4.0, (4, 4)))
    assert bool((d_dst[3] == 0xA5).all())


# ---- undistortion --------------------------------------------------------------------------------------------------------
def _ordered(a):
    """float32 -> integers in the order of the floats, so that neighbours differ by one."""
    i = np.asarray(a, np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7fffffff), i)


def _hold_to_model(got, ref, fisheye, what):
    """Bit equality; for the fisheye model, returns the number of coordinates that are float32 neighbours instead."""
    if same_floats(got, ref, np.uint32):
        return 0
    assert fisheye, "%s: pin-hole results differ from the model at %s" % (what, np.argwhere(got.view(np.uint32) != ref.view(np.uint32))[:5].tolist())
    na, nb = np.isnan(got), np.isnan(ref)
    assert (na == nb).all(), what
    off = np.abs(_ordered(got) - _ordered(ref))[~na]
    assert off.max() <= 1, "%s: %d coordinates further than one float32 ulp from the model" % (what, int((off > 1).sum()))
    return int((off == 1).sum())


@pytest.mark.parametrize("camera", sorted(sc.CAMERAS))
def test_undistort_camera(uvo, klt, camera):
    """1, 255, 256, 257 and 2 * max_points points: clamped fisheye points, unsettled Newton steps, the small-theta branch, NaN and
    infinities, all eight pin-hole coefficients."""
    fx, fy, cx, cy, dist, fisheye = sc.CAMERAS[camera]
    cam = uvo.CameraModel.make(fx, fy, cx, cy, dist, fisheye)
    pts = sc.undistort_points()
    neighbours = total = 0
    for n in sc.UNDISTORT_COUNTS:
        got = klt.undistort(cam, pts[:n])
        neighbours += _hold_to_model(got, sm.undistort(pts[:n], fx, fy, cx, cy, dist, fisheye), fisheye, "%s, %d points" % (camera, n))
        total += 2 * n
    print("undistort %s: %d of %d coordinates needed the one-ulp allowance" % (camera, neighbours, total))
    assert neighbours <= 0.001 * total


def test_undistort_point_count_edges(uvo, klt):
    fx, fy, cx, cy, dist, fisheye = sc.HARBOR
    cam = uvo.CameraModel.make(fx, fy, cx, cy, dist, fisheye)
    pts = np.concatenate([sc.undistort_points(), [[1.0, 2.0]]]).astype(np.float32)
    assert len(pts) == 2 * sc.KLT_MAX_POINTS + 1
    out = np.full((len(pts), 2), 7.25, np.float32)
    assert uvo.lib.uvo_undistort_points(klt._h, ctypes.byref(cam), pts.ctypes.data, len(pts), out.ctypes.data) == uvo.UVO_E_BADARG
    assert uvo.lib.uvo_undistort_points(klt._h, ctypes.byref(cam), pts.ctypes.data, -1, out.ctypes.data) == uvo.UVO_E_BADARG
    assert uvo.lib.uvo_undistort_points(klt._h, ctypes.byref(cam), pts.ctypes.data, 0, out.ctypes.data) == uvo.UVO_OK
    assert (out == 7.25).all()
    assert uvo.lib.uvo_undistort_points(klt._h, ctypes.byref(cam), pts.ctypes.data, 3, out.ctypes.data) == uvo.UVO_OK
    assert (out[3:] == 7.25).all() and not (out[:3] == 7.25).any()


def test_track_undistorted_against_the_model(uvo, klt, synth):
    """The fused call's two undistorted outputs at the harbor fisheye model: prev_un from the given points, next_un from the tracked ones."""
    fx, fy, cx, cy, dist, fisheye = sc.HARBOR
    cam = uvo.CameraModel.make(fx, fy, cx, cy, dist, fisheye)
    a = synth.make_frame(7100, 128, 96)
    b = synth.warp_frame(a, 7101)
    klt.build_pyramid(0, a), klt.build_pyramid(1, b)
    rng = np.random.default_rng(3100)
    p0 = np.stack([rng.uniform(4, 124, 150), rng.uniform(4, 92, 150)], 1).astype(np.float32)
    nxt, st, er, pu, nu = klt.track_undistorted(0, 1, p0, cam)
    n2, s2, _ = klt.track(0, 1, p0)
    assert nxt.tobytes() == n2.tobytes() and st.tobytes() == s2.tobytes()
    k = _hold_to_model(pu, sm.undistort(p0, fx, fy, cx, cy, dist, True), True, "prev_un")
    k += _hold_to_model(nu, sm.undistort(nxt, fx, fy, cx, cy, dist, True), True, "next_un")
    print("track_undistorted: %d of %d coordinates needed the one-ulp allowance" % (k, 4 * len(p0)))
    assert k <= 0.001 * 4 * len(p0)


# ---- BoW transform -------------------------------------------------------------------------------------------------------
def _vocabulary(uvo, voc):
    return uvo.ORBVocabulary(voc["child_start"], voc["children"], voc["descriptor"], voc["word_id"], voc["weight"], voc["L"], voc["weighting"],
                             voc["normalize"])


def _as_oracle_form(g):
    fv = g[4]
    groups = {int(fv.node[j]): [int(x) for x in fv.feat[fv.start[j]:fv.start[j + 1]]] for j in range(len(fv.node))}
    return g[0], g[1], g[2], g[3], groups


@pytest.mark.parametrize("branching", sc.BRANCHINGS, ids=str)
def test_bow_vocabulary(uvo, branching):
    """Word ids, weights, node ids, BowVector and FeatureVector for every weighting x normalisation, n at the edges of 4 features per
    wavefront and 16 per workgroup, levelsup below 0, at L and above it."""
    voc = sc.build_vocabulary(branching, len(branching))
    handles = {(w, nm): _vocabulary(uvo, sc.with_scoring(voc, w, nm)) for w in sc.WEIGHTINGS for nm in sc.NORMALIZES}
    for n in sc.BOW_COUNTS:
        feats = sc.bow_features(voc, n, n)
        for levelsup in sc.bow_levelsups(voc["L"]):
            descent = sm.bow_descend(voc, feats, levelsup)
            for (w, nm), V in handles.items():
                want = sm.bow_transform(sc.with_scoring(voc, w, nm), feats, levelsup, descent)
                assert same_bow(_as_oracle_form(V.transform(feats, levelsup)), want), (n, levelsup, w, nm)
    for V in handles.values():
        V.close()


@pytest.mark.parametrize("name", sorted(sc.tie_trees()))
def test_bow_ties_between_lanes_and_trips(uvo, name):
    voc, feats, want = sc.tie_trees()[name]
    V = _vocabulary(uvo, voc)
    g = _as_oracle_form(V.transform(feats, 0))
    V.close()
    assert (g[0] == want).all(), g[0]
    assert same_bow(g, sm.bow_transform(voc, feats, 0))


def test_bow_stop_words_only(uvo):
    voc = sc.stop_word_vocabulary()
    feats = sc.bow_features(voc, 40, 1)
    for w in sc.WEIGHTINGS:
        for nm in sc.NORMALIZES:
            v = sc.with_scoring(voc, w, nm)
            V = _vocabulary(uvo, v)
            g = _as_oracle_form(V.transform(feats, 1))
            V.close()
            assert len(g[3][0]) == 0 and g[4] == {} and same_bow(g, sm.bow_transform(v, feats, 1))


def test_bow_capacity_exact_and_one_less(uvo):
    """bow_cap / fv_cap of exactly the sizes needed succeed; one less in either returns UVO_E_CAPACITY."""
    voc = sc.build_vocabulary([10, 10, 10], 3)
    feats = sc.bow_features(voc, 130, 130)
    want = sm.bow_transform(voc, feats, 1)
    nb, nf = len(want[3][0]), len(want[4])
    assert 1 < nf < nb < 130
    V = _vocabulary(uvo, voc)

    def call(bow_cap, fv_cap):
        n = len(feats)
        wid, nid, ww = np.full(n, -7, np.int32), np.full(n, -7, np.int32), np.zeros(n)
        bid, bval = np.full(nb + 1, 0xA5A5A5A5, np.uint32), np.full(nb + 1, -1.5)
        fnode, fstart, ffeat = np.full(nf + 1, 0xA5A5A5A5, np.uint32), np.full(nf + 2, -7, np.int32), np.full(n + 1, -7, np.int32)
        n_bow, n_fv = ctypes.c_int(-1), ctypes.c_int(-1)
        rc = uvo.lib.uvo_bow_transform(V._h, feats.ctypes.data, n, 1, wid.ctypes.data, ww.ctypes.data, nid.ctypes.data, bid.ctypes.data, bval.ctypes.data,
                                       bow_cap, ctypes.byref(n_bow), fnode.ctypes.data, fstart.ctypes.data, ffeat.ctypes.data, fv_cap, ctypes.byref(n_fv))
        return rc, (wid, ww, nid, bid, bval, fnode, fstart, ffeat, n_bow.value, n_fv.value)
    rc, (wid, ww, nid, bid, bval, fnode, fstart, ffeat, n_bow, n_fv) = call(nb, nf)
    assert rc == uvo.UVO_OK and (n_bow, n_fv) == (nb, nf)
    groups = {int(fnode[j]): [int(x) for x in ffeat[fstart[j]:fstart[j + 1]]] for j in range(n_fv)}
    assert same_bow((wid, ww, nid, (bid[:nb].copy(), bval[:nb].copy()), groups), want)
    assert bid[nb] == 0xA5A5A5A5 and bval[nb] == -1.5 and fnode[nf] == 0xA5A5A5A5 and fstart[nf + 1] == -7 and ffeat[fstart[nf]:].tolist() == [-7] * (len(ffeat) - fstart[nf])
    for caps in ((nb - 1, nf), (nb, nf - 1)):
        rc, out = call(*caps)
        assert rc == uvo.UVO_E_CAPACITY, caps
        assert (out[3] == 0xA5A5A5A5).all() and (out[5] == 0xA5A5A5A5).all() and out[8:] == (0, 0)      # the containers are not half written
    V.close()


def test_bow_handle_grows_then_takes_a_small_call(uvo):
    """130, then 5000, then 3, then 130 features through one handle: the staging grows (its four buffers are released and allocated anew),
    then holds stale rows past the third and the fourth."""
    voc = sc.build_vocabulary([10, 10, 10], 3)
    V = _vocabulary(uvo, voc)
    for n in (130, 5000, 3, 130):
        feats = sc.bow_features(voc, n, 9000 + n)
        assert same_bow(_as_oracle_form(V.transform(feats, 1)), sm.bow_transform(voc, feats, 1)), n
    V.close()


@pytest.mark.parametrize("name", sorted(sc.bad_vocabularies()))
def test_vocabulary_that_lists_a_node_twice_is_refused(uvo, name):
    """uvo_vocabulary_create only: a descent through such a description might never end, so transform is never called on it."""
    cs, ch, mended_cs, mended_ch = (np.asarray(a, np.int32) for a in sc.bad_vocabularies()[name])
    n = len(cs) - 1
    desc, word, weight = np.zeros((n, 32), np.uint8), np.arange(n, dtype=np.int32), np.ones(n)
    h = ctypes.c_void_p()
    d = uvo.VocabularyDesc(n, cs.ctypes.data, ch.ctypes.data, desc.ctypes.data, word.ctypes.data, weight.ctypes.data, 2, 0, 1, 0)
    rc = uvo.lib.uvo_vocabulary_create(ctypes.byref(d), ctypes.byref(h))
    if rc == uvo.UVO_OK:
        uvo.lib.uvo_vocabulary_destroy(h)
    assert rc == uvo.UVO_E_BADARG and not h.value
    # the same nodes without the repeated entry are a tree, and are accepted
    d = uvo.VocabularyDesc(n, mended_cs.ctypes.data, mended_ch.ctypes.data, desc.ctypes.data, word.ctypes.data, weight.ctypes.data, 2, 0, 1, 0)
    assert uvo.lib.uvo_vocabulary_create(ctypes.byref(d), ctypes.byref(h)) == uvo.UVO_OK
    uvo.lib.uvo_vocabulary_destroy(h)


# ---- haloc ---------------------------------------------------------------------------------------------------------------
def test_haloc_hash_cases(uvo, matcher):
    """n of 0, 1, 2, 63..65, 500 x 1, 2, 3, 5 projections with proj_stride = n + 7 and NaN in the unused columns (a NaN in an output
    shows a read past n); descriptor columns of all 0 and all 255; subnormal products, cancelling +-1e30 terms, one +inf entry."""
    for name, proj, desc in sc.haloc_cases():
        assert proj.shape[1] == len(desc) + sc.HALOC_PAD and np.isnan(proj[:, len(desc):]).all()
        got, want = matcher.haloc_hash(proj, desc), sm.haloc_hash(proj, desc)
        assert same_floats(got, want, np.uint32), (name, np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:5].tolist())
        if name != "inf":
            assert not np.isnan(got).any(), name


def test_haloc_refusals(uvo, matcher):
    proj, desc = sc.haloc_projections(2, 10), sc.haloc_descriptors(10)
    out = np.full(64, 7.25, np.float32)
    lib = uvo.lib
    assert lib.uvo_haloc_hash(matcher._h, proj.ctypes.data, 2, 9, desc.ctypes.data, 10, out.ctypes.data) == uvo.UVO_E_BADARG      # proj_stride < n
    assert lib.uvo_haloc_hash(matcher._h, proj.ctypes.data, 0, 17, desc.ctypes.data, 10, out.ctypes.data) == uvo.UVO_E_BADARG
    assert lib.uvo_haloc_hash(matcher._h, proj.ctypes.data, 2, 17, desc.ctypes.data, -1, out.ctypes.data) == uvo.UVO_E_BADARG
    assert (out == 7.25).all()
