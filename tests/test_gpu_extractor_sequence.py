"""One long-lived extractor handle against the CPU oracle across changing calls (extractor_sequence_cases.py): sizes, modes, batch
sizes, refused calls and a second handle on the same device.  Every step is compared with what the oracle returns for that step's
arguments alone, byte for byte -- a handle that carries anything from one call into the next fails at the step that meets it."""
import ctypes

import numpy as np
import pytest

import extractor_sequence_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scenarios(synth):
    return sc.all_scenarios(synth)


@pytest.fixture(scope="module")
def want(oracle, scenarios):
    """the oracle's answer to every step of every scenario, computed once and never changed"""
    return {name: [sc.expected(oracle, cfg, st) for st in steps] for name, (cfg, steps) in scenarios.items()}


def _handle(uvo, cfg, **kw):
    return uvo.ORBextractor(cfg.nfeatures, cfg.scale, cfg.nlevels, 0, cfg.fast_th, max_width=sc.MAX_W, max_height=sc.MAX_H, max_batch=cfg.max_batch,
                            max_input_keypoints=cfg.max_input_keypoints, **kw)


def _same(kp, desc, w, what):
    assert len(kp) == len(w.kp) // 28, "%s: %d keypoints, the oracle has %d" % (what, len(kp), len(w.kp) // 28)
    assert kp.tobytes() == w.kp, "%s: keypoint records differ" % what
    if w.desc is not None:
        np.testing.assert_array_equal(desc, w.desc, err_msg="%s: descriptors" % what)


def _same_stages(ex, cfg, w, what, frame=0, planes=True):
    """the FAST candidates of every level and the last level's planes, as the batch left them on the device"""
    for l in range(cfg.nlevels):
        got = sorted(map(tuple, ex.read_candidates(l, frame=frame, cap=1 << 15).tolist()))
        assert got == w.cands[l], "%s: FAST candidates of level %d (%d, the oracle has %d)" % (what, l, len(got), len(w.cands[l]))
    if planes:
        last = cfg.nlevels - 1
        np.testing.assert_array_equal(ex.read_plane(last, frame=frame), w.planes[0], err_msg="%s: plane of level %d" % (what, last))
        if w.planes[1] is not None:   # the descriptor reaches 2 px into the border
            np.testing.assert_array_equal(ex.read_plane(last, blurred=True, frame=frame)[14:-14, 14:-14], w.planes[1][14:-14, 14:-14], err_msg="%s: blurred plane" % what)


def _run(uvo, oracle, ex, cfg, step, w, what):
    """one step on the handle, held to the oracle's result w"""
    what = "%s, step '%s'" % (what, step.name)
    if step.op == "grider":
        kp = ex.grider_fast(step.img, *step.extra)
        assert kp.tobytes() == w.kp, what
        return
    if step.op == "batch":
        res = ex.extract_batch(step.img)
        assert len(res) == len(w)
        for f, (kp, desc) in enumerate(res):
            _same(kp, desc, w[f], "%s frame %d" % (what, f))
        for f in range(len(res)):
            _same_stages(ex, cfg, w[f], "%s frame %d" % (what, f), frame=f, planes=f in (0, len(res) - 1))
        return
    grid = None
    if step.op == "full":
        kp, desc = ex(step.img)
    elif step.op == "clahe_full":
        np.testing.assert_array_equal(ex.clahe(step.img), oracle.clahe(step.img, 4.0, (12, 12)), err_msg=what + ": clahe")
        kp, desc = ex(None)
    elif step.op == "topup":
        h, wd = step.img.shape
        grid = sc.occupancy_grid(step.kin, step.min_px, wd, h) if step.kin is not None else np.zeros((h // step.min_px + 2, wd // step.min_px + 2), np.int32, order="F")
        kp, desc = ex(step.img, None if step.kin is None else step.kin.copy(), grid, step.min_px, False, step.need)
    elif step.op == "tracked":
        out = ex.extract_tracked(step.img, step.kin, step.min_px, step.need, want_grid=step.want_grid)
        kp, desc = out[:2]
        grid = out[2] if step.want_grid else None
    else:
        raise ValueError(step.op)
    _same(kp, desc, w, what)
    if grid is not None:
        np.testing.assert_array_equal(grid, w.grid, err_msg=what + ": grid")
    _same_stages(ex, cfg, w, what)


# ---- a. size walk ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["tiles", "levels"])
@pytest.mark.parametrize("scale,nlevels", sc.WALK_PYRAMIDS)
def test_size_walk(uvo, oracle, scenarios, want, scale, nlevels, form):
    """Full size, half size, a width that is no multiple of 4 (the padded copy of level 0 after an in-place call), the smallest accepted
    square, a wide strip, a tall image, the full size again with the first image, then the strip and the full size once more (only the
    height changes): set_geometry() on a used handle, with the fused
    pyramid launch and with the per-level launches.  At 1.35 / 3 `resize_fast` changes from step to step (the tile plans come and go);
    at 1.33 / 3 it cannot (test_extractor_sequence_cases.py).  The handle's own tables give the smallest square."""
    name = "size walk %.2f / %d" % (scale, nlevels)
    cfg, steps = scenarios[name]
    ex = _handle(uvo, cfg)
    assert ex.mvInvScaleFactor.tobytes() == oracle.extractor(cfg.nfeatures, scale, nlevels, cfg.fast_th).inv_scale.tobytes()
    assert sc.smallest_side(ex.mvInvScaleFactor) == sc.SMALLEST_SQUARE[(scale, nlevels)]
    ex.tune(uvo.UVO_TUNE_PYR_FORM, uvo.UVO_PYR_FORM_TILES if form == "tiles" else uvo.UVO_PYR_FORM_LEVELS)
    for st, w in zip(steps, want[name]):
        _run(uvo, oracle, ex, cfg, st, w, "%s (%s)" % (name, form))
        h, wd = st.img.shape
        assert ex.level_dims(0) == (wd, h)
    ex.close()


# ---- b. mode walk ----------------------------------------------------------------------------------------------------
def test_mode_walk_on_one_size_then_on_another(uvo, oracle, scenarios, want):
    """FullDetect, top-up with caller keypoints (d 20), top-up without (d 5: the grid and the page-locked region behind it grow),
    extract_tracked with and without the grid, clahe() + ex(None), grider_fast (which borrows lane 0's corner scratch and the image
    staging), FullDetect again -- the first step's bytes -- and a top-up with a negative budget; then all of it again at 253 x 190 on the
    same handle, and once more at the first size."""
    ex = _handle(uvo, sc.MODE_CFG)
    for name in ("mode walk 320 x 256", "mode walk 253 x 190", "mode walk 320 x 256"):
        cfg, steps = scenarios[name]
        assert want[name][7].kp == want[name][0].kp
        for st, w in zip(steps, want[name]):
            _run(uvo, oracle, ex, cfg, st, w, name)
    ex.close()


def test_adaptive_fast_mode_flips_and_flips_back(uvo, oracle, scenarios, want):
    """A faded and a low-contrast frame between two normal ones with UVO_TUNE_FAST_MODE adaptive: every level's pass threshold goes to 7
    behind the low-contrast frame and back to fastTh behind the normal one, the keypoints never depend on it, and the state afterwards is
    that of a second handle that made the last two calls only."""
    cfg, steps = scenarios["adaptive walk"]
    ex = _handle(uvo, cfg)
    ex.tune(uvo.UVO_TUNE_FAST_MODE, uvo.UVO_FAST_MODE_ADAPTIVE)
    thresholds = {}
    for st, w in zip(steps, want["adaptive walk"]):
        _run(uvo, oracle, ex, cfg, st, w, "adaptive walk")
        thresholds[st.name] = ex.fast_state()[0].tolist()
    assert thresholds["normal"] == [cfg.fast_th] * cfg.nlevels
    assert thresholds["low contrast"] == [7] * cfg.nlevels
    assert thresholds["normal again"] == [cfg.fast_th] * cfg.nlevels
    other = _handle(uvo, cfg)
    other.tune(uvo.UVO_TUNE_FAST_MODE, uvo.UVO_FAST_MODE_ADAPTIVE)
    for st, w in list(zip(steps, want["adaptive walk"]))[-2:]:
        _run(uvo, oracle, other, cfg, st, w, "adaptive walk, second handle")
    for a, b in zip(ex.fast_state(), other.fast_state()):
        assert a.tolist() == b.tolist()
    other.close()
    ex.close()


# ---- c. batch walk ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wide_max", [0, 1 << 20])
def test_batch_walk_then_two_lanes(uvo, oracle, scenarios, want, wide_max):
    """Batches of 1, 2, 3, 8, 9, 16, 17, 20, 1 frames -- both sides of kFewFrames, kTilePyramidFrames and kSmallBatch -- every frame another
    image and every frame checked, with the quad-tree in its 256-thread form (fused with the blur) and in its 1024-thread form.  Then
    two lanes: A (full size) and B (half size) submitted before either is waited for, C (full size) behind them, and a synchronous call."""
    cfg, steps = scenarios["batch walk"]
    ex = _handle(uvo, cfg)
    ex.tune(uvo.UVO_TUNE_OCT_WIDE_MAX, wide_max)
    for st, w in zip(steps, want["batch walk"]):
        _run(uvo, oracle, ex, cfg, st, w, "batch walk (wide_max %d)" % wide_max)
    ex.set_pipeline(2)
    _, (A, B, C, S) = scenarios["pipeline walk"]
    wA, wB, wC, wS = want["pipeline walk"]

    def buffers(n):
        return uvo.pinned_empty((n, ex.cap), uvo.KEYPOINT_DTYPE), uvo.pinned_empty((n, ex.cap, 32), np.uint8), uvo.pinned_empty((n,), np.int32)

    def held(bufs, w, what):
        kp, desc, n = bufs
        for f in range(len(w)):
            _same(kp[f, :n[f]], desc[f, :n[f]], w[f], "%s frame %d" % (what, f))
    bA, bB, bC = buffers(len(A.img)), buffers(len(B.img)), buffers(len(C.img))
    tA = ex.submit(A.img, *bA)
    tB = ex.submit(B.img, *bB)
    ex.wait(tA)
    ex.wait(tB)
    held(bA, wA, "A")
    held(bB, wB, "B")
    tC = ex.submit(C.img, *bC)
    ex.wait(tC)
    held(bC, wC, "C")
    _run(uvo, oracle, ex, cfg, sc.Step("full", "synchronous call behind the lanes", S.img[0]), wS[0], "pipeline walk")
    ex.close()


# ---- d. refused calls ------------------------------------------------------------------------------------------------
REFUSE_CFG = sc.Cfg(500, 1.35, 3, sc.FAST_TH, 2, 8)
LATE_SHAPES = [(256, 320, sc.GEOM_CAP_YTAB), (163, 267, sc.GEOM_CAP_YTAB), (640, 110, sc.GEOM_CAP_XTAB), (484, 102, sc.GEOM_CAP_XTAB)]


def test_refused_calls_leave_the_handle_as_it_was(uvo, oracle, synth):
    """A good FullDetect call, then each refused call followed by the same good call, which must return the recorded bytes (the
    oracle's) with fast_state() unchanged.  Every refusal but one comes from host-side validation in front of any launch
    (extractor_host.cpp: validate(), check_image(), uvo_extract(), uvo_grider_fast(); extractor.cpp: the argument checks of
    run_batch_device() and set_geometry(), both in front of the batch's first kernel); the exception is the output capacity one below
    n_out, a complete and valid extraction that is refused only when its results are handed out (UVO_E_CAPACITY, n_out = the full count).
    The clahe() in front of the refused ex(None) is a valid call of its own.

    The late refusals of set_geometry(): through extract_batch_device, which does not check the sides, a 1.35 / 3 handle of 320 x 256
    refuses the transposed shape 256 x 320 and 163 x 267 at the ROW-table capacity and the strips 640 x 110 and 484 x 102 at the
    COLUMN-table capacity, behind the block and FAST-scratch checks (test_extractor_sequence_cases.py works that out on the host).
    163 x 267 and 484 x 102 take the 12-byte-window resize on level 1, the handle's own size does not: a set_geometry() that kept the
    refused size's `resize_fast` would resize level 1 of the next good call through a window its taps do not fit.  No shape of at most the
    handle's area reaches the quad-tree path-table capacity at this configuration (every one of them was probed): that check has no
    reachable refusal here."""
    import torch
    cfg = REFUSE_CFG
    good, other = sc.frame(synth, 9800, sc.MAX_W, sc.MAX_H), sc.frame(synth, 9801, 160, 128)
    w_good = sc.expected(oracle, cfg, sc.Step("full", "good", good))
    assert len(w_good.kp) // 28 >= 30
    ex = _handle(uvo, cfg)
    good_step = sc.Step("full", "good call", good)
    _run(uvo, oracle, ex, cfg, good_step, w_good, "refusals: first")
    state = [a.tolist() for a in ex.fast_state()]
    n_good = len(w_good.kp) // 28
    kin = sc.tracked_points(9802, 8, sc.MAX_W, sc.MAX_H)
    grid20 = lambda: np.zeros((sc.MAX_H // 20 + 2, sc.MAX_W // 20 + 2), np.int32, order="F")
    near = kin.copy()
    near["x"][3] = 1.0
    side = sc.smallest_side(ex.mvInvScaleFactor) - 1

    def capacity_one_short():
        kp, desc, n = np.zeros(n_good - 1, uvo.KEYPOINT_DTYPE), np.zeros((n_good - 1, 32), np.uint8), ctypes.c_int(0)
        rc = uvo.lib.uvo_extract(ex._h, good.ctypes.data, sc.MAX_W, sc.MAX_H, sc.MAX_W, None, 0, None, 0, 0, 20, 1, 0, kp.ctypes.data, desc.ctypes.data, n_good - 1, ctypes.byref(n))
        assert n.value == n_good and kp.tobytes() == w_good.kp[:28 * (n_good - 1)] and np.array_equal(desc, w_good.desc[:-1])
        raise uvo.UvoError(rc, "uvo_extract")

    def none_after_clahe_of_another_size():
        ex.clahe(other, download=False)
        ex._clahe_shape = (sc.MAX_H, sc.MAX_W)
        ex(None)

    d_img = torch.zeros(sc.MAX_W * sc.MAX_H, dtype=torch.uint8, device="cuda")
    d_kp, d_desc, d_n = (torch.zeros(n, dtype=torch.uint8, device="cuda") for n in (ex.cap * 28, ex.cap * 32, 16))
    refused = [
        ("one pixel wider than max_width", uvo.UVO_E_BADARG, lambda: ex(np.zeros((sc.MAX_H, sc.MAX_W + 1), np.uint8))),
        ("one pixel higher than max_height", uvo.UVO_E_BADARG, lambda: ex(np.zeros((sc.MAX_H + 1, sc.MAX_W), np.uint8))),
        ("a level below 56 px", uvo.UVO_E_UNSUPPORTED, lambda: ex(sc.frame(synth, 9803, side, side))),
        ("a caller keypoint at x = 1", uvo.UVO_E_BADARG, lambda: ex(good, near, grid20(), 20, False, 100)),
        ("a grid one row too small", uvo.UVO_E_BADARG, lambda: ex(good, kin.copy(), np.zeros(((sc.MAX_H - 1) // 20, sc.MAX_W // 20 + 2), np.int32, order="F"), 20, False, 100)),
        ("n_in > max_input_keypoints", uvo.UVO_E_BADARG, lambda: ex(good, sc.tracked_points(9804, 9, sc.MAX_W, sc.MAX_H), grid20(), 20, False, 100)),
        ("ex(None) after a clahe() of another size", uvo.UVO_E_BADARG, none_after_clahe_of_another_size),
        ("a grider_fast grid finer than the image", uvo.UVO_E_BADARG, lambda: ex.grider_fast(other, 50, 161, 4, 20)),
        ("a batch of max_batch + 1", uvo.UVO_E_BADARG, lambda: ex.extract_batch(np.stack([good] * 3))),
        ("an output capacity one below n_out", uvo.UVO_E_CAPACITY, capacity_one_short),
    ]
    for w, h, verdict in LATE_SHAPES:
        assert w * h <= sc.MAX_W * sc.MAX_H and sc.geom_probe(cfg, w, h)[0] == verdict
        refused.append(("%d x %d through extract_batch_device" % (w, h), uvo.UVO_E_BADARG,
                        lambda w=w, h=h: ex.extract_batch_device(d_img.data_ptr(), 1, w, h, d_kp.data_ptr(), d_desc.data_ptr(), d_n.data_ptr())))
    assert sc.geom_probe(cfg, side, side)[0] == sc.GEOM_UNSUPPORTED
    for what, code, call in refused:
        with pytest.raises(uvo.UvoError) as ei:
            call()
        assert ei.value.code == code, (what, ei.value.code, str(ei.value))
        _run(uvo, oracle, ex, cfg, good_step, w_good, "refusals: after " + what)
        assert [a.tolist() for a in ex.fast_state()] == state, what
        assert ex.level_dims(0) == (sc.MAX_W, sc.MAX_H)
    torch.cuda.synchronize()
    ex.close()


# ---- e. two handles on one device ------------------------------------------------------------------------------------
@pytest.mark.parametrize("wide_max", [0, 1 << 20])
@pytest.mark.parametrize("big_first", [False, True])
def test_two_handles_with_quad_tree_lds_above_and_below_64_kib(uvo, oracle, scenarios, want, big_first, wide_max):
    """Handle A (1600 features on 2 levels) needs more than 64 KiB of dynamic LDS for the quad-tree, handle B (300 on 4) far less; the
    kernel's limit is a per-device setting that prepare_octree() only ever raises.  B, A, B, A; destroy A; B; a new A; A; B -- an
    ordinary sequence of valid calls, every one equal to the oracle -- with either handle created first."""
    cfg_a, steps_a = scenarios["two handles, large quota"]
    cfg_b, steps_b = scenarios["two handles, small quota"]
    w_a, w_b = want["two handles, large quota"], want["two handles, small quota"]

    def make(cfg):
        ex = _handle(uvo, cfg)
        ex.tune(uvo.UVO_TUNE_OCT_WIDE_MAX, wide_max)
        return ex
    if big_first:
        a, b = make(cfg_a), make(cfg_b)
    else:
        b, a = make(cfg_b), make(cfg_a)
    calls = {"a": 0, "b": 0}

    def call(which):
        ex, cfg, steps, w = (a, cfg_a, steps_a, w_a) if which == "a" else (b, cfg_b, steps_b, w_b)
        i = calls[which] % len(steps)
        calls[which] += 1
        _run(uvo, oracle, ex, cfg, steps[i], w[i], "two handles (%s first, wide_max %d), call %d of %s" % ("A" if big_first else "B", wide_max, calls[which], which.upper()))
    call("b"), call("a")
    lds_a = sc.octree_lds(a.mnFeaturesPerLevel, [a.level_dims(l) for l in range(cfg_a.nlevels)])
    lds_b = sc.octree_lds(b.mnFeaturesPerLevel, [b.level_dims(l) for l in range(cfg_b.nlevels)])
    assert lds_a > 64 * 1024 > 16 * 1024 > lds_b, (lds_a, lds_b)
    call("b"), call("a")
    a.close()
    call("b")
    a = make(cfg_a)
    call("a"), call("b")
    a.close()
    b.close()
