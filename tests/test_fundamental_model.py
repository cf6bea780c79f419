"""Known answers for tests/fundamental_model.py, the restatement of cv::findFundamentalMat(FM_RANSAC) that the GPU parity test
(test_gpu_fundamental.py) holds csrc/fundamental.hip to.  None of these rests on the recalled OpenCV details: they are geometry
(a known K, R, t), the algebra of the RNG, the arithmetic of RANSACUpdateNumIters and of a cubic's roots, and ground-truth masks."""
import ctypes

import numpy as np

import fundamental_model as fm


def _rel(a, b):
    a, b = fm.normalized_F(a), fm.normalized_F(b)
    return float(np.linalg.norm(a - b))


def test_seven_point_model_of_noise_free_points_is_the_true_F():
    for seed in range(5):
        p0, p1, _, F = fm.scene(100 + seed, 7, 1.0, 0.0, dtype=np.float64)
        models = fm.run_7point(p0, p1, list(range(7)))
        assert 1 <= len(models) <= 3
        assert min(_rel(M, F) for M in models) < 1e-9, seed


def test_ransac_mask_is_the_ground_truth():
    p0, p1, inl, F = fm.scene(7, 200, 0.7, 0.0)
    res = fm.find_fundamental(p0, p1, 1.0, 0.999)
    assert res.method == fm.METHOD_RANSAC
    np.testing.assert_array_equal(res.mask.astype(bool), inl)
    assert res.inliers == 140 and res.iterations == fm.update_num_iters(0.999, 60 / 200, 7, 1000) == 80
    assert _rel(res.F, F) < 1e-3


def test_lmeds_mask_is_the_ground_truth():
    """14 points, 2 of them outliers.  (At 12 points the median is the 7th smallest error, which the exact 7-point fit makes ~0 for
    every subset, outliers or not: LMedS cannot tell the models apart there.  From 14 points the median reaches past the subset.)"""
    p0, p1, inl, F = fm.scene(11, 14, 12 / 14, 0.0)
    res = fm.find_fundamental(p0, p1, 1.0, 0.999)
    assert res.method == fm.METHOD_LMEDS and res.iterations == 450 and len(res.hypotheses) == 450
    np.testing.assert_array_equal(res.mask.astype(bool), inl)
    assert res.inliers == 12 and _rel(res.F, F) < 1e-3


def test_jump_ahead_equals_the_recurrence():
    r = fm.Rng()
    states = [r.state]
    for _ in range(200000):
        r.next()
        states.append(r.state)
    assert states[0] > fm.MWC_M and states[1] > fm.MWC_M and max(states[2:]) < fm.MWC_M
    for k in (0, 1, 2, 3, 7, 2048, 2049, 65537, 123456, 200000):
        assert fm.state_after(k) == states[k], k
    # the device's windows: lane t starts 2t draws after the window's state, one modular product by A^(2t) mod M
    for ws in (0, 1, 2047, 4096, 150001):
        base = states[ws + 1] % fm.MWC_M
        for t in (1, 2, 511, 1023):
            assert pow(fm.MWC_A, 2 * t, fm.MWC_M) * base % fm.MWC_M == states[ws + 2 * t + 1]


def test_iteration_counts():
    table = {0.9: 11, 0.8: 29, 0.7: 80, 0.6: 243, 0.5: 881, 0.4: 1000, 0.3: 1000}
    for ratio, iters in table.items():
        assert fm.update_num_iters(0.999, 1 - ratio, 7, 1000) == iters, ratio
    assert max(fm.update_num_iters(0.999, 0.45, 7, 1000), 3) == 450
    assert fm.update_num_iters(0.999, 0.0, 7, 1000) == 0             # all inliers: 1 - (1 - 0)^7 = 0
    assert fm.update_num_iters(0.999, 0.5, 7, 100) == 100            # capped at the previous count


def test_solve_cubic_branches():
    n, r = fm.solve_cubic([1, -6, 11, -6])                          # (x-1)(x-2)(x-3): three real roots
    assert n == 3 and np.allclose(sorted(r), [1, 2, 3], atol=1e-12)
    n, r = fm.solve_cubic([1, -2, 1, -2])                           # (x-2)(x^2+1): one real root
    assert n == 1 and abs(r[0] - 2) < 1e-12
    n, r = fm.solve_cubic([1, 0, -3, 2])                            # (x-1)^2 (x+2): Q^3 == R^2 exactly
    assert n == 2 and r[0] == -2 and r[1] == 1
    n, r = fm.solve_cubic([2, -6, 6, -2])                           # 2 (x-1)^3: d == 0, the two roots coincide
    assert n == 1 and r[0] == 1
    n, r = fm.solve_cubic([0, 1, -3, 2])                            # quadratic
    assert n == 2 and sorted(r[:2]) == [1, 2]
    n, r = fm.solve_cubic([0, 1, 0, 1])                             # quadratic without real roots
    assert n == 0
    n, r = fm.solve_cubic([0, 0, 2, -4])                            # linear
    assert n == 1 and r[0] == 2
    assert fm.solve_cubic([0, 0, 0, 5])[0] == 0 and fm.solve_cubic([0, 0, 0, 0])[0] == -1


def test_collinear_subsets_are_rejected():
    x = np.arange(7, dtype=np.float32) * 3 + 10
    line = np.stack([x, 2 * x + 3], 1)                               # exactly on y = 2x + 3 in float32
    xs, ys = [float(v) for v in line[:, 0]], [float(v) for v in line[:, 1]]
    assert fm._collinear(xs, ys, list(range(7)))
    ys2 = list(ys)
    ys2[6] += 5.0                                                    # the last point off the line: only it is tested
    assert not fm._collinear(xs, ys2, list(range(7)))
    ys3 = list(ys)
    ys3[0] += 5.0                                                    # an earlier point off the line: pairs (1, 2) still hold
    assert fm._collinear(xs, ys3, list(range(7)))


def test_all_collinear_input_gives_no_model():
    x = np.arange(40, dtype=np.float32) * 7 + 5
    p0 = np.stack([x, 2 * x + 3], 1)
    p1 = p0 + np.float32([4, 1])
    res = fm.find_fundamental(p0, p1)
    assert res.info[:3] == (fm.METHOD_RANSAC, 0, 0) and not res.hypotheses
    assert not res.mask.any() and not res.F.any()
    r = fm.Rng()
    drawer = fm.SubsetDrawer(p0, p1, rng=r)
    assert drawer.draw(10000) is None and res.rng_draws == r.draws > 70000


def test_small_point_counts():
    p0, p1, _, _ = fm.scene(5, 7, 1.0, 0.3)
    for n in range(7):
        res = fm.find_fundamental(p0[:n], p1[:n])
        assert res.info == (fm.METHOD_NONE, 0, 0, 0) and res.mask.shape == (n,) and not res.mask.any()
    res = fm.find_fundamental(p0, p1)
    assert res.method == fm.METHOD_7POINT and (res.mask == 1).all() and res.inliers == 7 and res.rng_draws == 0
    assert res.F.any()
    res = fm.find_fundamental(np.zeros((7, 2)), np.zeros((7, 2)))  # a degenerate 7-point system: the mask is still all 1
    assert (res.mask == 1).all()


def test_parameter_fixups():
    p0, p1, _, _ = fm.scene(9, 60, 0.6, 0.5)
    three = fm.find_fundamental(p0, p1, 3.0, 0.999)
    for thr in (0.0, -2.0):
        assert fm.find_fundamental(p0, p1, thr, 0.999).info == three.info
    nine = fm.find_fundamental(p0, p1, 1.0, 0.99)
    for conf in (0.0, 1.0, 1.5, -1.0):
        assert fm.find_fundamental(p0, p1, 1.0, conf).info == nine.info


def test_new_entry_points_reject_a_null_handle(uvo):
    lib = uvo.lib
    mask, F, pts = np.zeros(32, np.uint8), np.zeros(9), np.zeros((32, 2), np.float32)
    info = uvo.FmInfo()
    assert lib.uvo_klt_find_fundamental(None, pts.ctypes.data, pts.ctypes.data, 32, 1.0, 0.999, mask.ctypes.data, F.ctypes.data,
                                        ctypes.byref(info)) == uvo.UVO_E_BADARG
    cam = uvo.CameraModel.make(400, 400, 320, 256, [])
    st, er = np.zeros(32, np.uint8), np.zeros(32, np.float32)
    assert lib.uvo_klt_track_filtered(None, 0, 1, pts.ctypes.data, pts.ctypes.data, 32, 3, 30, 0.01, 1e-4, ctypes.byref(cam), st.ctypes.data,
                                      er.ctypes.data, pts.ctypes.data, pts.ctypes.data, 1.0, 0.999, mask.ctypes.data, None) == uvo.UVO_E_BADARG
    sub, nm, sc, n = np.zeros((4, 7), np.int32), np.zeros(4, np.int32), np.zeros((4, 3)), ctypes.c_int()
    assert lib.uvo_klt_fm_hypotheses(None, sub.ctypes.data, nm.ctypes.data, sc.ctypes.data, 4, ctypes.byref(n)) == uvo.UVO_E_BADARG

