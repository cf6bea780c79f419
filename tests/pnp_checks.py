"""What tests/test_pnp_emu.py (the host build of csrc/epnp_core.hpp) and tests/test_gpu_pnp.py (the device) have in common: the host
build's loader and the layers of the solvePnPRansac contract that hold for any implementation of the call,
stated once.  Test infrastructure only."""
import ctypes

import numpy as np

import host_build
import pnp_model as pm

CAP = 1000


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


class Emu:
    """tests/emu/pnp_emu.cpp, built on first use with the library's contract: no FMA contraction."""

    def __init__(self):
        L = self.L = ctypes.CDLL(host_build.build("pnp_emu"))
        vp, ci, cd = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
        L.emu_pnp_subsets.argtypes = [ci, ci, vp, vp]
        L.emu_pnp_subsets.restype = None
        L.emu_pnp_errors.argtypes = [vp, vp, vp, vp, ci, vp]
        L.emu_pnp_errors.restype = None
        L.emu_pnp_rodrigues.argtypes = [vp, vp]
        L.emu_pnp_rodrigues.restype = None
        L.emu_pnp_replay.argtypes = [vp, ci, cd, ci, vp]
        L.emu_pnp_epnp.argtypes = [vp, vp, vp, ci, vp, ci, ci, vp]
        L.emu_pnp_run.argtypes = [vp, vp, vp, ci, ci, cd, cd, vp, vp, vp, vp, vp, vp, vp, vp]

    def subsets(self, n, hyp):
        sub, end = np.zeros((hyp, 5), np.int32), np.zeros(hyp, np.uint32)
        self.L.emu_pnp_subsets(n, hyp, _p(sub), _p(end))
        return sub, end

    def errors(self, cam, pose, obj, img):
        c, pose = cam.as_doubles(), np.ascontiguousarray(pose, np.float64).reshape(12)
        obj, img = np.ascontiguousarray(obj, np.float32), np.ascontiguousarray(img, np.float32)
        err = np.zeros(len(obj), np.float32)
        self.L.emu_pnp_errors(_p(c), _p(pose), _p(obj), _p(img), len(obj), _p(err))
        return err

    def rodrigues(self, R):
        R, r = np.ascontiguousarray(R, np.float64).reshape(9), np.zeros(3)
        self.L.emu_pnp_rodrigues(_p(R), _p(r))
        return r

    def replay(self, counts, n, conf, max_iters):
        counts, it = np.ascontiguousarray(counts, np.int32), ctypes.c_int()
        w = self.L.emu_pnp_replay(_p(counts), n, conf, max_iters, ctypes.byref(it))
        return w, it.value

    def epnp(self, cam, obj, img, idx, as_float):
        """-> (ok, pose float64[12])"""
        c = cam.as_doubles()
        obj, img = np.ascontiguousarray(obj, np.float32), np.ascontiguousarray(img, np.float32)
        idx, pose = np.ascontiguousarray(idx, np.int32), np.zeros(12)
        ok = self.L.emu_pnp_epnp(_p(c), _p(obj), _p(img), len(obj), _p(idx), len(idx), 1 if as_float else 0, _p(pose))
        return bool(ok), pose

    def run(self, cam, obj, img, iterations=300, thr=3.0, conf=0.99):
        """The whole call -> Run."""
        c = cam.as_doubles()
        obj, img = np.ascontiguousarray(obj, np.float32).reshape(-1, 3), np.ascontiguousarray(img, np.float32).reshape(-1, 2)
        n = len(obj)
        rvec, tvec, pose, inl, info = np.zeros(3), np.zeros(3), np.zeros(12), np.zeros(max(n, 1), np.int32), np.zeros(4, np.int32)
        sub, poses, cnt = np.zeros((CAP, 5), np.int32), np.zeros((CAP, 12)), np.zeros(CAP, np.int32)
        self.L.emu_pnp_run(_p(c), _p(obj), _p(img), n, iterations, thr, conf, _p(rvec), _p(tvec), _p(pose), _p(inl), _p(info), _p(sub), _p(poses),
                           _p(cnt))
        it = int(info[1])
        return Run(int(info[0]), it, inl[:info[2]].copy(), int(np.uint32(info[3])), rvec, tvec, pose[:9].reshape(3, 3).copy(), pose[9:].copy(),
                   sub[:it].copy(), poses[:it].copy(), cnt[:it].copy())


class Run:
    """One call's outputs and its hypothesis tap (the first `iterations` hypotheses), whoever computed them."""

    def __init__(self, ok, iterations, inliers, rng_draws, rvec, tvec, R, t, subsets, poses, counts):
        self.ok, self.iterations, self.inliers, self.rng_draws = ok, iterations, inliers, rng_draws
        self.rvec, self.tvec, self.R, self.t = rvec, tvec, R, t
        self.subsets, self.poses, self.counts = subsets, poses, counts


def gpu_run(k, uvo, cam, obj, img, iterations=300, thr=3.0, conf=0.99):
    """uvo_klt_solve_pnp_ransac + its tap as a Run.  The call returns R as rvec (double) and as Tcw (float); Run.R is rvec brought back
    to a matrix by the model's Rodrigues (a rounding or two away from the device's R -- far inside the refit tolerance)."""
    cm = uvo.CameraModel.make(cam.fx, cam.fy, cam.cx, cam.cy, cam.k[:cam.n_dist])
    rvec, tvec, Tcw, inl, info = k.solve_pnp_ransac(obj, img, cm, iterations, thr, conf)
    sub, poses, cnt = k.pnp_hypotheses()
    r = Run(info.ok, info.iterations, inl, info.rng_draws, rvec, tvec, pm.rodrigues_to_matrix(rvec), tvec.copy(), sub, poses, cnt)
    r.Tcw = Tcw
    r.info_inliers = info.inliers
    return r


def check_layers_1_to_3(run, cam, obj, img, iterations=300, thr=3.0, conf=0.99, what=""):
    """Layers 1 - 3 of the contract for one run: the random stream exactly, the scoring exactly at the run's own poses, the replay
    exactly at the run's own counts, the inlier list = the winner's inliers in order.  No exception, no case left out."""
    obj, img = np.ascontiguousarray(obj, np.float32).reshape(-1, 3), np.ascontiguousarray(img, np.float32).reshape(-1, 2)
    n = len(obj)
    if n < pm.MODEL_POINTS:
        assert (run.ok, run.iterations, len(run.inliers), run.rng_draws, len(run.subsets)) == (0, 0, 0, 0, 0), what
        return
    if n == pm.MODEL_POINTS:   # the direct path: nothing drawn, every point an inlier
        assert (run.iterations, run.rng_draws, len(run.subsets)) == (0, 0, 0), what
        assert not run.ok or list(run.inliers) == list(range(5)), what
        return
    # 1. the random stream
    assert len(run.subsets) == run.iterations == len(run.counts) == len(run.poses), what
    sub, ends = pm.subsets(n, run.iterations)
    np.testing.assert_array_equal(run.subsets, sub, err_msg=what)
    assert run.rng_draws == int(ends[-1]), (what, run.rng_draws, int(ends[-1]))
    # 2. the scoring, at the run's own poses
    tt = float(np.float32(thr * thr))
    for h in range(run.iterations):
        c = int(run.counts[h])
        if c < 0:   # no finite pose: it must not have been invented either
            assert not run.poses[h].any(), (what, h)
            continue
        assert np.isfinite(run.poses[h]).all(), (what, h)
        _, lo, hi, _, _ = pm.count(cam, run.poses[h][:9], run.poses[h][9:], obj, img, thr)
        assert lo <= c <= hi, (what, h, c, lo, hi)
    # 3. the replay, at the run's own counts
    winner, it = pm.replay(np.append(np.maximum(run.counts, 0), np.zeros(iterations, np.int64)), n, conf, min(iterations, CAP))
    assert it == run.iterations, (what, it, run.iterations)
    if winner < 0:
        assert run.ok == 0 and len(run.inliers) == 0, what
        return
    _, _, _, err, inl = pm.count(cam, run.poses[winner][:9], run.poses[winner][9:], obj, img, thr)
    near = np.abs(err.astype(np.float64) - tt) <= pm.SENS_RTOL * tt
    if run.ok:
        got = np.zeros(n, bool)
        got[run.inliers] = True
        assert (np.diff(run.inliers) > 0).all(), what
        assert ((got == inl) | near).all(), (what, np.flatnonzero((got != inl) & ~near)[:8])
        assert len(run.inliers) == int(run.counts[winner]), (what, len(run.inliers), int(run.counts[winner]))


def check_layer_5(run, cam, obj, img, what=""):
    """The returned pose against the independent model's refit on the run's own inlier list (from 6 points on)."""
    if not run.ok or len(run.inliers) < 6:
        return None
    ref = pm.refit(cam, obj, img, run.inliers)
    assert ref is not None, what
    d = pm.pose_deviation(run.R, run.t, ref[0], ref[1])
    return d
