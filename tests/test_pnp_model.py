"""tests/pnp_model.py, the numpy restatement of cv::solvePnPRansac(SOLVEPNP_EPNP), held to known answers on the CPU -- and the
measurements the GPU contract rests on, reproduced from the committed model so that they are checked, not
believed: how much a 5-point hypothesis depends on the null-space basis, how little a refit from 6 points on does, and how much
either depends on the sign of the control-point axes."""
import math

import numpy as np
import pytest

import fundamental_model as fm
import pnp_model as pm


def test_rng_stream_is_cv_rng_and_subsets_redraw_only_repeats():
    for n in (6, 9, 400):
        r = fm.Rng()
        sub, ends = pm.subsets(n, 50)
        for h in range(50):
            idx = []
            while len(idx) < 5:
                v = r.next() % n
                if v not in idx:
                    idx.append(v)
            assert list(sub[h]) == idx and int(ends[h]) == r.draws
        s, e = pm.subset(n, 17)
        assert list(s) == list(sub[17]) and e == int(ends[17])
    assert fm.state_after(int(pm.subsets(400, 10)[1][-1])) == _state_after_subsets(400, 10)


def _state_after_subsets(n, count):
    r = fm.Rng()
    for _ in range(int(pm.subsets(n, count)[1][-1])):
        r.next()
    return r.state


def test_replay_on_hand_made_counts():
    # nothing above 4: no winner, every iteration runs
    assert pm.replay([4] * 300, 100, 0.99, 300) == (-1, 300)
    # a perfect hypothesis at 0 ends the loop at once: niters becomes 0 (denominator below DBL_MIN)
    assert pm.replay([100] + [0] * 299, 100, 0.99, 300) == (0, 1)
    # half the points at iteration 3: niters = round(log(0.01) / log(1 - 0.5^5)) = 145; a later equal count is not taken (strict >)
    counts = [0, 0, 0, 50] + [50] * 296
    assert fm.update_num_iters(0.99, 0.5, 5, 300) == 145
    assert pm.replay(counts, 100, 0.99, 300) == (3, 145)
    # a better one inside the window shortens it again; one outside it is never seen
    counts = [0, 0, 0, 50] + [0] * 100 + [90] + [0] * 195
    it = fm.update_num_iters(0.99, 0.1, 5, 145)
    assert pm.replay(counts, 100, 0.99, 300) == (104, max(it, 105))
    counts = [0, 0, 0, 50] + [0] * 150 + [90] + [0] * 145
    assert pm.replay(counts, 100, 0.99, 300) == (3, 145)
    # 5 inliers is the least that is taken
    assert pm.replay([5] + [0] * 299, 1000, 0.99, 300)[0] == 0


def test_project_points_against_a_closed_form():
    cam = pm.Camera(pm.EUROC)
    rng = np.random.default_rng(0)
    R = pm.rodrigues_to_matrix([0.1, -0.2, 0.05])
    t = np.array([0.2, -0.1, 0.3])
    P = rng.uniform([-3, -2, 2], [3, 2, 15], (50, 3))
    got = pm.project_points(cam, R, t, P)
    k1, k2, p1, p2 = cam.k[:4]
    for i in range(50):
        X = R @ P[i] + t
        x, y = X[0] / X[2], X[1] / X[2]
        r2 = x * x + y * y
        radial = 1 + k1 * r2 + k2 * r2 * r2
        xd = x * radial + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
        yd = y * radial + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
        assert abs(got[i, 0] - (cam.fx * xd + cam.cx)) < 1e-9 and abs(got[i, 1] - (cam.fy * yd + cam.cy)) < 1e-9


def test_undistort_inverts_the_lens_model_where_five_iterations_converge():
    cam = pm.Camera(pm.EUROC)
    x = np.linspace(-0.2, 0.2, 9)
    u, v = pm.distort(cam, x, x[::-1] * 0.5)
    und = pm.undistort(cam, np.stack([u, v], 1))
    assert np.abs(und[:, 0] - x).max() < 1e-8 and np.abs(und[:, 1] - x[::-1] * 0.5).max() < 1e-8


def test_rodrigues_round_trips():
    rng = np.random.default_rng(1)
    for theta in (0.0, 1e-12, 1e-7, 1e-3, 0.5, 2.0, 3.1, math.pi - 1e-4):
        for _ in range(4):
            ax = rng.normal(size=3)
            r = ax / np.linalg.norm(ax) * theta
            back = pm.rodrigues(pm.rodrigues_to_matrix(r))
            if theta < 2e-5:      # sin(theta) / ... below 1e-5: cv::Rodrigues returns the zero vector
                assert not back.any(), (theta, back)
            else:
                assert np.abs(back - r).max() < 1e-9, (theta, r, back)
    for theta in (math.pi - 1e-7, math.pi):      # the diagonal form: the vector up to its sign, conditioned like sqrt(eps)
        ax = rng.normal(size=3)
        r = ax / np.linalg.norm(ax) * theta
        back = pm.rodrigues(pm.rodrigues_to_matrix(r))
        assert min(np.abs(back - r).max(), np.abs(back + r).max()) < 1e-6
    # a matrix that is only nearly a rotation is projected first (U Vt of its SVD)
    R = pm.rodrigues_to_matrix([0.3, 0.2, -0.4])
    assert np.abs(pm.rodrigues(R * 1.001 + 1e-5) - [0.3, 0.2, -0.4]).max() < 1e-4


@pytest.mark.parametrize("camera", [pm.PLAIN, pm.EUROC], ids=["plain", "euroc"])
@pytest.mark.parametrize("n", [6, 50, 1000])
def test_pose_recovery_on_noise_free_scenes(n, camera):
    """To the rounding of the float32 inputs (a few 1e-6: 5e-6) with points stored as float, and to 1e-10 when the scene is kept in double.
    cv::undistortPoints runs five fixed-point iterations whatever their residual, which at the EuRoC corners (k1 = -0.28, r^2 = 0.9) is
    1e-2 in normalised units -- a property of the call, not rounding.  The scene absorbs that, not the bound: with distortion the
    projections stay in the central part of the image, where the residual is far below the bound -- the central quarter for the float
    scenes (residual 3e-9 against float rounding; measured worst 1.2e-6, distortion-free 5.7e-7) and the central tenth for the double
    scenes (measured worst 3.7e-13 there, 1.3e-11 at 0.15, 2.6e-9 at 0.25; distortion-free, whole image: 5.9e-14)."""
    for seed in range(5):
        cam, obj, img, R, t, _ = pm.scene(seed, n, 1.0, 0.0, camera, spread=1.0 if camera is pm.PLAIN else 0.25)
        r = pm.refit(cam, obj, img, np.arange(n))
        d = pm.pose_deviation(r[0], r[1], R, t)
        assert d < 5e-6, (seed, d)
        cam, obj, img, R, t, _ = pm.scene(seed, n, 1.0, 0.0, camera, dtype=np.float64, spread=1.0 if camera is pm.PLAIN else 0.1)
        r = pm.refit(cam, obj, img, np.arange(n))
        d = pm.pose_deviation(r[0], r[1], R, t)
        assert d < 1e-10, (seed, d)


def test_five_points_meet_their_reprojections():
    for seed in range(10):
        cam, obj, img, R, t, _ = pm.scene(seed, 5, 1.0, 0.0, pm.PLAIN)
        for basis in pm.BASES:
            r = pm.solve_pnp(cam, obj, img, range(5), True, basis, np.random.default_rng(seed))
            assert r is not None and pm.errors(cam, r[0], r[1], obj, img).max() < 1e-2, (seed, basis)


def test_five_point_hypotheses_depend_on_the_null_space_basis_and_refits_do_not():
    """The table of DESIGN.md section 4 (its four scenes, 100 hypotheses each), within loose brackets: at 5 points more than 20 % of the
    hypotheses move by more than 1e-6 when only the basis of the null space changes, and the inlier count at 3 px changes in some but in
    fewer than a third of the variant runs; the refit over the inliers moves by less than the refit tolerance."""
    for (n, ratio, noise) in ((400, 0.95, 0.3), (400, 0.7, 1.0), (400, 0.5, 1.0), (64, 0.7, 0.3)):
        cam, obj, img, R, t, inl = pm.scene(7, n, ratio, noise, pm.PLAIN)
        sub, _ = pm.subsets(n, 100)
        moved, changed = 0, 0
        rng = np.random.default_rng(1)
        for s in sub:
            base = pm.solve_pnp(cam, obj, img, s, True, "svd")
            worst, cb = 0.0, pm.count(cam, base[0], base[1], obj, img)[0]
            for basis in pm.BASES[1:]:
                o = pm.solve_pnp(cam, obj, img, s, True, basis, rng)
                if o is None:
                    worst = 1.0
                    continue
                worst = max(worst, pm.pose_deviation(o[0], o[1], base[0], base[1]))
                changed += pm.count(cam, o[0], o[1], obj, img)[0] != cb
            moved += worst > 1e-6
        print("n %d ratio %.2f noise %.1f: %d of 100 hypotheses move by more than 1e-6, inlier count changes in %d of 300 variant runs" % (n, ratio, noise, moved, changed))
        assert moved > 0.2 * 100
        assert 1 <= changed < 100
        idx = np.flatnonzero(inl)
        fits = [pm.refit(cam, obj, img, idx, b) for b in pm.BASES[:3]]
        assert max(pm.pose_deviation(a[0], a[1], b[0], b[1]) for a in fits for b in fits) <= pm.REFIT_TOL


def test_refit_spread_between_the_variants_stays_below_the_measured_value():
    """REFIT_SPREAD_MEASURED is what the tolerance of the GPU contract is 4 times of: a scene change that moves the measurement past it
    has to move the constant, in the open."""
    worst, where = 0.0, None
    for sc in pm.refit_scenes():
        cam, obj, img, _, _, _ = pm.scene(*sc)
        fits = [pm.refit(cam, obj, img, np.arange(len(obj)), b) for b in pm.BASES[:3]]
        d = max(pm.pose_deviation(a[0], a[1], b[0], b[1]) for a in fits for b in fits)
        if d > worst:
            worst, where = d, sc[:4]
    print("largest deviation between the variants over %d refits: %.2e at %s (constant %.2e, tolerance %.2e)" %
          (len(pm.refit_scenes()), worst, where, pm.REFIT_SPREAD_MEASURED, pm.REFIT_TOL))
    assert worst <= pm.REFIT_SPREAD_MEASURED
    assert worst >= pm.REFIT_SPREAD_MEASURED / 10      # and the constant is a measurement, not a generous guess


def test_the_sign_of_a_control_axis_moves_the_pose_with_noisy_data():
    """Item 8 of the model's list.  Flipping one principal axis changes nothing on exact data and the pose by about the size of the
    noise-induced error on noisy data; permuting the axes changes nothing."""
    for (n, noise, lo) in ((50, 0.0, None), (50, 1.0, 1e-4), (400, 0.3, 1e-4)):
        cam, obj, img, R, t, _ = pm.scene(5, n, 1.0, noise, pm.PLAIN)
        und = pm.undistort(cam, img)
        uv = und * [cam.fx, cam.fy] + [cam.cx, cam.cy]
        a = pm.epnp(obj.astype(np.float64), uv, cam.K)
        b = pm.epnp(obj.astype(np.float64), uv, cam.K, axis_signs=(1, 1, -1))
        d = pm.pose_deviation(a[0], a[1], b[0], b[1])
        print("n %d noise %.1f: one axis flipped moves the pose by %.2e (error against the truth %.2e)" % (n, noise, d, pm.pose_deviation(a[0], a[1], R, t)))
        if lo is None:
            assert d < 1e-5
        else:
            assert d > lo


def test_whole_runs_recover_the_pose_and_stop_early_on_clean_scenes():
    for camera in (pm.EUROC, pm.PLAIN):
        cam, obj, img, R, t, inl = pm.scene(3, 400, 0.95, 0.3, camera)
        r = pm.run(cam, obj, img)
        assert r.ok and r.iterations < 20 and len(r.inliers) >= 0.9 * inl.sum()
        assert pm.pose_deviation(r.R, r.t, R, t) < 0.05
        assert r.rng_draws == int(pm.subsets(400, r.iterations)[1][-1])
    cam, obj, img, R, t, inl = pm.scene(3, 400, 0.3, 1.0)
    assert pm.run(cam, obj, img).iterations == 300
    assert not pm.run(cam, obj[:4], img[:4]).ok
    r = pm.run(cam, obj[inl][:5], img[inl][:5])
    assert r.ok and list(r.inliers) == [0, 1, 2, 3, 4] and r.iterations == 0


def test_mutations_of_the_run_are_visible():
    """The switches the GPU suite's mutation check leans on do change the model's own results."""
    cam, obj, img, R, t, inl = pm.scene(21, 400, 0.5, 1.0)
    base = pm.run(cam, obj, img)
    assert pm.run(cam, obj, img, update_points=4).iterations < base.iterations
    for sc in pm.TIE_SCENES:      # a later hypothesis ties the winner's count with other inliers: >= takes it, > does not
        cam2, obj2, img2, _, _, _ = pm.scene(*sc)
        a, b = pm.run(cam2, obj2, img2), pm.run(cam2, obj2, img2, accept_ge=True)
        assert b.winner > a.winner and len(a.inliers) == len(b.inliers) and (a.inliers != b.inliers).any()
    allp = pm.run(cam, obj, img, refit_all=True)
    assert pm.pose_deviation(allp.R, allp.t, base.R, base.t) > 1e-3


def test_bands_of_the_four_variants_on_part_of_the_grid():
    """Layer 6 of the GPU contract compares against these bands (computed there for every scene of the grid); printed here so that
    their width can be read without a GPU."""
    widest_cnt, widest_err = 0, 0.0
    for sc in [s for s in pm.grid_scenes() if s[1] in (20, 64, 400) and s[3] == 1.0]:
        cam, obj, img, R, t, _ = pm.scene(*sc)
        vs = [pm.run(cam, obj, img, basis=b, rot_seed=sc[0]) for b in pm.BASES]
        cnt = [len(v.inliers) for v in vs]
        err = [pm.pose_deviation(v.R, v.t, R, t) for v in vs]
        widest_cnt, widest_err = max(widest_cnt, max(cnt) - min(cnt)), max(widest_err, max(err) - min(err))
        print(sc[:4], "inliers", cnt, "pose error", ["%.2e" % e for e in err], "iterations", [v.iterations for v in vs])
    print("widest band: %d inliers, %.2e pose error" % (widest_cnt, widest_err))
