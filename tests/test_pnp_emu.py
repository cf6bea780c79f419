"""The host build of the solvePnPRansac arithmetic (csrc/epnp_core.hpp through tests/emu/pnp_emu.cpp) against the numpy model
(tests/pnp_model.py) wherever the call is determined by its data: the random stream, the scoring of a given pose, the replay of given
counts, Rodrigues, EPnP from 6 points on (the refit tolerance of the model), and layers 1 - 3 of the contract on whole runs at the
build's own hypothesis poses.  The GPU suite then holds the device to this build bit for bit (tests/test_gpu_pnp.py)."""
import numpy as np
import pytest

import pnp_checks as pc
import pnp_model as pm


@pytest.fixture(scope="module")
def emu():
    return pc.Emu()


def test_subsets_and_draw_counts_equal_the_model(emu):
    for n in (6, 7, 8, 20, 64, 400, 1000, 4096):
        sub, end = emu.subsets(n, 300)
        msub, mend = pm.subsets(n, 300)
        np.testing.assert_array_equal(sub, msub)
        np.testing.assert_array_equal(end, mend)
    assert pm.subsets(6, 300)[1][-1] > 1500      # repeated indices are redrawn: more than 5 draws per subset at 6 points


def test_errors_equal_the_model_within_the_threshold_margin(emu):
    for sc in ((1, 400, 0.7, 1.0, pm.EUROC), (2, 400, 0.7, 1.0, pm.PLAIN), (3, 64, 0.5, 0.3, pm.EUROC)):
        cam, obj, img, R, t, _ = pm.scene(*sc)
        pose = np.concatenate([R.reshape(9), t])
        e, m = emu.errors(cam, pose, obj, img), pm.errors(cam, R, t, obj, img)
        rel = np.abs(e.astype(np.float64) - m) / np.maximum(m, 1e-30)
        print("errors: worst relative difference %.2e" % rel.max())
        assert rel.max() <= pm.SENS_RTOL
        _, lo, hi, _, _ = pm.count(cam, R, t, obj, img)
        assert lo <= int((e <= np.float32(9.0)).sum()) <= hi


def test_replay_equals_the_model(emu):
    rng = np.random.default_rng(5)
    for trial in range(200):
        n = int(rng.choice([6, 20, 64, 400, 1000]))
        counts = rng.integers(0, n + 1, 300) if trial % 2 else (rng.integers(0, 8, 300) * (rng.uniform(size=300) < 0.2))
        counts = np.minimum(counts, n).astype(np.int32)
        assert emu.replay(counts, n, 0.99, 300) == pm.replay(counts, n, 0.99, 300), (trial, n)


def test_rodrigues_equals_the_model(emu):
    rng = np.random.default_rng(6)
    for theta in (0.0, 1e-9, 1e-6, 1e-3, 0.3, 1.5, 3.0, np.pi - 1e-3, np.pi - 1e-7, np.pi):
        for _ in range(5):
            ax = rng.normal(size=3)
            r = ax / np.linalg.norm(ax) * theta
            R = pm.rodrigues_to_matrix(r)
            a, b = emu.rodrigues(R), pm.rodrigues(R)
            # within 1e-5 of pi both take the diagonal form sqrt((R_ii + 1) / 2), conditioned like sqrt(eps) = 1.5e-8
            assert np.abs(a - b).max() <= (1e-6 if theta > np.pi - 1e-4 else 1e-9), (theta, a, b)


def test_epnp_from_six_points_on_agrees_with_the_model_within_the_refit_tolerance(emu):
    worst = 0.0
    for sc in pm.refit_scenes():
        cam, obj, img, R, t, _ = pm.scene(*sc)
        idx = np.arange(len(obj), dtype=np.int32)
        ok, pose = emu.epnp(cam, obj, img, idx, False)
        ref = pm.refit(cam, obj, img, idx)
        assert ok and ref is not None, sc[:4]
        d = pm.pose_deviation(pose[:9].reshape(3, 3), pose[9:], ref[0], ref[1])
        worst = max(worst, d)
        assert d <= pm.REFIT_TOL, (sc[:4], d)
    print("host build vs model over %d refits of 6 .. 2048 points: worst %.2e (tolerance %.2e)" % (len(pm.refit_scenes()), worst, pm.REFIT_TOL))


def test_five_point_hypotheses_meet_their_reprojections(emu):
    for seed in range(20):
        cam, obj, img, R, t, _ = pm.scene(seed, 5, 1.0, 0.0, pm.PLAIN if seed % 2 else pm.EUROC, spread=0.25)
        ok, pose = emu.epnp(cam, obj, img, np.arange(5, dtype=np.int32), True)
        assert ok
        assert emu.errors(cam, pose, obj, img).max() < 1e-2, seed    # px^2: five points leave EPnP's system a null space, not the projections


@pytest.mark.parametrize("sc", [(11, 6, 0.95, 0.3, pm.EUROC), (12, 8, 0.7, 1.0, pm.PLAIN), (13, 20, 0.5, 0.3, pm.EUROC), (14, 64, 0.7, 1.0, pm.EUROC),
                                (15, 400, 0.95, 0.3, pm.PLAIN), (16, 400, 0.3, 1.0, pm.EUROC), (17, 1000, 0.5, 0.3, pm.PLAIN)],
                         ids=lambda s: "n%d_r%.2f_s%.1f" % (s[1], s[2], s[3]))
def test_whole_runs_layers_1_to_3_and_5(emu, sc):
    cam, obj, img, R, t, _ = pm.scene(*sc)
    run = emu.run(cam, obj, img)
    pc.check_layers_1_to_3(run, cam, obj, img, what=str(sc[:4]))
    d = pc.check_layer_5(run, cam, obj, img)
    if d is not None:
        assert d <= pm.REFIT_TOL, (sc[:4], d)
    if run.ok:
        np.testing.assert_array_equal(run.rvec, emu.rodrigues(run.R))


@pytest.mark.parametrize("sc", list(pm.TIE_SCENES) + [(41, 400, 0.7, 1.0, pm.STRONG), (42, 64, 0.7, 0.3, pm.STRONG)], ids=lambda s: "seed%d" % s[0])
def test_ties_at_the_maximum_and_strong_distortion(emu, sc):
    cam, obj, img, R, t, _ = pm.scene(*sc, spread=0.6 if sc[4] is pm.STRONG else 1.0)
    run = emu.run(cam, obj, img)
    pc.check_layers_1_to_3(run, cam, obj, img, what=str(sc[:4]))
    d = pc.check_layer_5(run, cam, obj, img)
    assert run.ok and d is not None and d <= pm.REFIT_TOL, (sc[:4], d)
    if sc in pm.TIE_SCENES:      # the scene is what its name says
        w, it = pm.replay(np.append(np.maximum(run.counts, 0), np.zeros(300, np.int64)), len(obj), 0.99, 300)
        assert any(run.counts[h] == run.counts[w] and ((emu.errors(cam, run.poses[h], obj, img) <= 9) != (emu.errors(cam, run.poses[w], obj, img) <= 9)).any()
                   for h in range(w + 1, it))


def test_degenerate_inputs_leave_no_nan(emu):
    cam = pm.Camera(pm.EUROC)
    rng = np.random.default_rng(9)
    n = 40
    same = np.tile(np.array([[0.3, -0.2, 5.0]], np.float32), (n, 1))
    img = np.stack([rng.uniform(0, 752, n), rng.uniform(0, 480, n)], 1).astype(np.float32)
    plane = np.stack([rng.uniform(-2, 2, n), rng.uniform(-2, 2, n), np.full(n, 6.0)], 1).astype(np.float32)
    pimg = pm.project_points(cam, np.eye(3), np.zeros(3), plane).astype(np.float32)
    for obj, im in ((same, img), (plane, pimg), (same[:5], img[:5])):
        run = emu.run(cam, obj, im)
        for a in (run.rvec, run.tvec, run.R, run.t, run.poses):
            assert np.isfinite(a).all()
        if not run.ok:
            assert not run.rvec.any() and not run.tvec.any() and len(run.inliers) == 0
        pc.check_layers_1_to_3(run, cam, obj, im)


def test_short_inputs(emu):
    cam, obj, img, _, _, _ = pm.scene(3, 8, 1.0, 0.3)
    for n in range(5):
        run = emu.run(cam, obj[:n], img[:n])
        pc.check_layers_1_to_3(run, cam, obj[:n], img[:n])
    run = emu.run(cam, obj[:5], img[:5])
    pc.check_layers_1_to_3(run, cam, obj[:5], img[:5])
    assert run.ok and run.iterations == 0 and list(run.inliers) == [0, 1, 2, 3, 4]
