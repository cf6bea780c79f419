"""What tests/test_pnpsolver_emu.py (the host build of csrc/pnpsolver_core.hpp) and tests/test_gpu_pnpsolver.py (the device) have in
common: the host build's loader, a driver that runs one scripted session on any implementation of the solver set, and the layers of the
PnPsolver contract that hold for any implementation, stated once.  Test infrastructure only."""
import ctypes

import numpy as np

import host_build
import pnp_model as pm
import pnpsolver_model as psm


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


class Emu:
    """tests/emu/pnpsolver_emu.cpp, built on first use with the library's contract: no FMA contraction."""
    _lib = None

    def __init__(self):
        if Emu._lib is None:
            L = ctypes.CDLL(host_build.build("pnpsolver_emu"))
            vp, ci, cd, cf, u32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_float, ctypes.c_uint32
            L.emu_glibc_rand.argtypes = [u32, ci, vp]
            L.emu_glibc_rand.restype = None
            L.emu_pnps_subsets.argtypes = [u32, ci, ci, ci, vp]
            L.emu_pnps_subsets.restype = None
            L.emu_pnps_derive.argtypes = [ci, vp, vp]
            L.emu_pnps_derive.restype = None
            L.emu_pnps_check_inliers.argtypes = [vp, vp, vp, vp, ci, cd, cd, cd, cd, vp]
            L.emu_pnps_check_inliers.restype = None
            L.emu_pnps_iterations_ahead.argtypes = [ci, ci, ci]
            L.emu_pnps_replay.argtypes = [vp, vp, vp, ci, ci, ci, ci, vp]
            L.emu_pnps_replay.restype = None
            L.emu_pnps_epnp.argtypes = [vp, vp, vp, ci, cd, cd, cd, cd, vp]
            L.emu_pnpsolver_set_create.argtypes = [vp, ci, ci, vp]
            L.emu_pnpsolver_set_destroy.argtypes = [vp]
            L.emu_pnpsolver_set_destroy.restype = None
            L.emu_pnpsolver_set_clear.argtypes = [vp]
            L.emu_pnpsolver_add.argtypes = [vp, vp, vp, vp, vp, ci, ci, cf, cf, cf, cf, vp, vp]
            L.emu_pnpsolver_query.argtypes = [vp, ci, vp]
            L.emu_pnpsolver_iterate.argtypes = [vp, vp, ci, ci, vp, vp]
            L.emu_pnpsolver_hypotheses.argtypes = [vp, ci, vp, vp, vp, ci, vp]
            Emu._lib = L
        self.L = Emu._lib

    def rand(self, seed, count):
        out = np.zeros(count, np.int32)
        self.L.emu_glibc_rand(seed, count, _p(out))
        return out

    def subsets(self, seed, n, min_set, count):
        out = np.zeros((count, min_set), np.int32)
        self.L.emu_pnps_subsets(seed, n, min_set, count, _p(out))
        return out

    def derive(self, n, params):
        out = np.zeros(3, np.int32)
        self.L.emu_pnps_derive(n, ctypes.byref(params), _p(out))
        return int(out[1]), int(out[2])

    def check_inliers(self, pose, p3d, p2d, max_err, K):
        pose = np.ascontiguousarray(pose, np.float64).reshape(12)
        p3d, p2d, me = (np.ascontiguousarray(a, np.float32) for a in (p3d, p2d, max_err))
        inl = np.zeros(len(p3d), np.uint8)
        f = lambda v: float(np.float32(v))
        self.L.emu_pnps_check_inliers(_p(pose), _p(p3d), _p(p2d), _p(me), len(p3d), f(K[0]), f(K[1]), f(K[2]), f(K[3]), _p(inl))
        return inl.astype(bool)

    def replay(self, iterations, best, counts, script, carried, n_iterations, max_its, min_inliers):
        state, out = np.array([iterations, best], np.int32), np.zeros(6, np.int32)
        counts, script = np.ascontiguousarray(counts, np.int32), np.ascontiguousarray(script, np.int32)
        self.L.emu_pnps_replay(_p(state), _p(counts), _p(script), carried, n_iterations, max_its, min_inliers, _p(out))
        return dict(performed=int(out[0]), returned=int(out[1]), no_more=int(out[2]), inliers=int(out[3]), iterations=int(state[0]), best=int(state[1]),
                    takes=int(out[4]), refines=int(out[5]))

    def epnp(self, p3d, p2d, idx, K):
        p3d, p2d, idx = np.ascontiguousarray(p3d, np.float32), np.ascontiguousarray(p2d, np.float32), np.ascontiguousarray(idx, np.int32)
        pose = np.zeros(12)
        f = lambda v: float(np.float32(v))
        ok = self.L.emu_pnps_epnp(_p(p3d), _p(p2d), _p(idx), len(idx), f(K[0]), f(K[1]), f(K[2]), f(K[3]), _p(pose))
        return bool(ok), pose

    def make_set(self, uvo, max_solvers, max_points):
        """The host build behind the product's own Python class."""
        cls = type("EmuPnPsolverSet", (uvo.PnPsolverSet,), {"_prefix": "emu_pnpsolver_"})
        return cls(None, max_solvers, max_points, _api=self.L)


# ---- one scripted session on any implementation ----------------------------------------------------------------------------------
class Call:
    """What one iterate call gave: the result, the generator state afterwards, each listed solver's tap and counters."""

    def __init__(self, ids, n_iterations, result, rng_state, taps, infos):
        self.ids, self.n_iterations, self.result, self.rng_state, self.taps, self.infos = ids, n_iterations, result, rng_state, taps, infos


def run_session(uvo, pset, candidates, calls, params=None, seed=1):
    """Add `candidates` (psm.candidate tuples) to the empty set, then make the listed calls [(ids, n_iterations), ...] on one generator
    seeded with `seed`.  -> [Call]."""
    prm = params if params is not None else uvo.PnPsolverParams()
    pset.clear()
    for (p3d, p2d, sigma2, kp, nm, K, _, _) in candidates:
        pset.add(p3d, p2d, sigma2, kp, nm, K, prm)
    rng = uvo.GlibcRand(seed)
    out = []
    for ids, n_it in calls:
        res = pset.iterate(ids, n_it, rng)
        taps = [pset.hypotheses(i, prm.min_set) for i in ids]
        infos = [pset.query(i) for i in ids]
        out.append(Call(list(ids), n_it, res, rng.state(), taps, [(f.n, f.min_inliers, f.max_its, f.iterations, f.best_inliers) for f in infos]))
    return out


def assert_sessions_equal(a, b, what=""):
    """Two implementations' sessions, bit for bit: subsets, every hypothesis pose and count, masks, Tcw, nInliers, bNoMore, mnIterations,
    the generator state handed back."""
    assert len(a) == len(b), what
    for k, (x, y) in enumerate(zip(a, b)):
        w = "%s call %d" % (what, k)
        rx, ry = x.result, y.result
        assert (rx.returned, rx.solver, rx.n_inliers, rx.refined, rx.draws) == (ry.returned, ry.solver, ry.n_inliers, ry.refined, ry.draws), \
            (w, (rx.returned, rx.solver, rx.n_inliers, rx.refined, rx.draws), (ry.returned, ry.solver, ry.n_inliers, ry.refined, ry.draws))
        assert rx.Tcw.tobytes() == ry.Tcw.tobytes(), (w, rx.Tcw, ry.Tcw)
        np.testing.assert_array_equal(rx.status, ry.status, err_msg=w)
        np.testing.assert_array_equal(rx.inliers, ry.inliers, err_msg=w)
        assert x.rng_state == y.rng_state, w
        assert x.infos == y.infos, (w, x.infos, y.infos)
        for j, (tx, ty) in enumerate(zip(x.taps, y.taps)):
            np.testing.assert_array_equal(tx[0], ty[0], err_msg="%s solver %d subsets" % (w, x.ids[j]))
            np.testing.assert_array_equal(tx[2], ty[2], err_msg="%s solver %d counts" % (w, x.ids[j]))
            assert tx[1].tobytes() == ty[1].tobytes(), ("%s solver %d poses" % (w, x.ids[j]), np.abs(tx[1] - ty[1]).max())


def _tcw(pose):
    T = np.zeros((4, 4), np.float32)
    T[:3, :3], T[:3, 3], T[3, 3] = np.asarray(pose[:9]).reshape(3, 3), pose[9:], 1
    return T


def check_session_against_model(uvo, emu, session, candidates, params=None, seed=1, what=""):
    """The layers that hold for any implementation, at the session's own hypothesis poses: the random stream and its continuity from
    solver to solver and call to call; the derived parameters; CheckInliers of every hypothesis pose within the model's margin; the
    replay at the run's own counts, where Refine()'s outcome is taken from the run (the one consultation the run reports as returning
    returned, every earlier one did not); the returned pose and set as the host build's EPnP + CheckInliers on the best set, scattered
    through kp_index; that EPnP against the independent model's.  Returns the largest refit deviation seen (None: no refined pose
    from a best set of 6 points or more)."""
    prm = params if params is not None else uvo.PnPsolverParams()
    g = psm.GlibcRand(seed)
    ref = uvo.GlibcRand(seed)
    state = {}   # solver id -> [mnIterations, best, best set, best pose]
    worst = None
    for k, call in enumerate(session):
        res = call.result
        w = "%s call %d" % (what, k)
        assert np.isfinite(res.Tcw).all(), w
        draws = 0
        stopped = False
        for j, sid in enumerate(call.ids):
            p3d, p2d, sigma2, kp, nm, K, _, _ = candidates[sid]
            n = len(p3d)
            it0, best0, best_set, best_pose = state.setdefault(sid, [0, 0, None, None])
            sub, poses, cnt = call.taps[j]
            touched, no_more, its_after = (int(v) for v in res.status[j])
            if stopped:
                assert (touched, no_more, its_after, len(cnt)) == (0, 0, it0, 0), (w, sid)
                continue
            assert touched == 1, (w, sid)
            min_inl, max_its = psm.derive_params(n, prm.probability, prm.min_inliers, prm.max_iterations, prm.min_set, prm.epsilon) if n else (1, 1)
            if n < min_inl:
                assert (no_more, its_after, len(cnt)) == (1, it0, 0), (w, sid)
                assert res.returned != j, (w, sid)
                continue
            assert call.infos[j][:3] == (n, min_inl, max_its), (w, sid, call.infos[j])
            # the stream: this solver's subsets continue where the last one stopped
            performed = len(cnt)
            want = [psm.draw_subset(g, n, prm.min_set) for _ in range(performed)]
            np.testing.assert_array_equal(sub, np.array(want, np.int32).reshape(performed, prm.min_set), err_msg="%s solver %d" % (w, sid))
            draws += performed * prm.min_set
            assert np.isfinite(poses).all() and its_after == it0 + performed == call.infos[j][3], (w, sid)
            # CheckInliers at the run's own poses
            me = psm.max_error(sigma2, prm.th2)
            for h in range(performed):
                if not poses[h].any():
                    assert cnt[h] == 0, (w, sid, h)
                    continue
                _, inl, near = psm.check_inliers(poses[h], p3d, p2d, K, me)
                lo, hi = int((inl & ~near).sum()), int((inl | near).sum())
                assert lo <= cnt[h] <= hi, (w, sid, h, int(cnt[h]), lo, hi)
                mine = emu.check_inliers(poses[h], p3d, p2d, me, K)
                assert int(mine.sum()) == cnt[h] and ((mine == inl) | near).all(), (w, sid, h)
            # the replay at the run's own counts
            returned_here = res.returned == j
            pad = [0] * 400
            script, carried = np.zeros(performed + 400, np.int64), 0
            if returned_here and res.refined:
                # Refine() depends on the best set only, so the consultation that returned is the first on that set: find the set in force
                # after `performed` iterations with every Refine failing, and let that one succeed
                probe = psm.replay(it0, best0, list(cnt) + pad, script, 0, performed, it0 + performed, min_inl)
                if probe["best_from"] >= 0:
                    script[probe["best_from"]] = res.n_inliers
                else:
                    carried = res.n_inliers
            m = psm.replay(it0, best0, list(cnt) + pad, script, carried, call.n_iterations, max_its, min_inl)
            assert m["performed"] == performed, (w, sid, m, performed)
            assert (m["returned"] != psm.NONE) == returned_here, (w, sid, m)
            assert (m["no_more"], m["iterations"], m["best"]) == (no_more, its_after, call.infos[j][4]), (w, sid, m, call.infos[j])
            if m["best_from"] >= 0:
                best_pose = poses[m["best_from"]]
                best_set = emu.check_inliers(best_pose, p3d, p2d, me, K)
                assert int(best_set.sum()) == m["best"], (w, sid)
            state[sid] = [m["iterations"], m["best"], best_set, best_pose]
            if not returned_here:
                continue
            stopped = True
            assert (res.solver, res.n_inliers, res.refined) == (sid, m["inliers"], 1 if m["returned"] == psm.REFINED else 0), (w, sid, m)
            assert len(res.inliers) == nm and int(res.inliers.sum()) == res.n_inliers, (w, sid)
            assert not np.delete(res.inliers, kp).any(), (w, sid)          # nothing outside mvKeyPointIndices
            got = res.inliers[kp].astype(bool)
            if res.refined:
                assert res.n_inliers > min_inl, (w, sid)
                idx = np.flatnonzero(best_set)
                ok, pose = emu.epnp(p3d, p2d, idx, K)
                assert ok and res.Tcw.tobytes() == _tcw(pose).tobytes(), (w, sid)
                np.testing.assert_array_equal(got, emu.check_inliers(pose, p3d, p2d, me, K), err_msg=w)
                _, inl, near = psm.check_inliers(pose, p3d, p2d, K, me)
                assert ((got == inl) | near).all(), (w, sid)
                if len(idx) >= 6:
                    r = psm.refit(p3d, p2d, K, idx)
                    assert r is not None, (w, sid)
                    d = pm.pose_deviation(pose[:9].reshape(3, 3), pose[9:], r[0], r[1])
                    worst = d if worst is None else max(worst, d)
            else:
                assert no_more == 1 and res.Tcw.tobytes() == _tcw(best_pose).tobytes(), (w, sid)
                np.testing.assert_array_equal(got, best_set, err_msg=w)
        assert res.draws == draws, (w, res.draws, draws)
        if not stopped:
            assert (res.returned, res.solver, res.n_inliers) == (-1, -1, 0) and not res.Tcw.any() and len(res.inliers) == 0, w
        for _ in range(draws):
            ref.next()
        assert call.rng_state == ref.state(), w
    return worst
