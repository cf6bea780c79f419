"""What tests/test_sim3solver_emu.py (the host build of csrc/sim3_core.hpp) and tests/test_gpu_sim3solver.py (the device) have in common:
the host build's loader, a driver that runs one scripted session on any implementation of the solver set, and the layers of the
Sim3Solver contract that hold for any implementation, stated once.  Test infrastructure only."""
import ctypes

import numpy as np

import host_build
import sim3_model as sm

MUTATIONS = ("SIM3_MUT_OR", "SIM3_MUT_GT", "SIM3_MUT_THRESHOLD", "SIM3_MUT_DRAW")
FIND = "find"


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


class Emu:
    """tests/emu/sim3solver_emu.cpp, built on first use with the library's contract: no FMA contraction.  `mutation`: one of MUTATIONS,
    compiled into a library of its own (the seeded faults the checks below must catch)."""
    _libs = {}

    def __init__(self, mutation=None):
        assert mutation is None or mutation in MUTATIONS
        if mutation not in Emu._libs:
            variant = (["-D" + mutation], "_" + mutation.lower()) if mutation else ()
            L = ctypes.CDLL(host_build.build("sim3solver_emu", *variant))
            vp, ci, cf, u32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_uint32
            L.emu_sim3_derive.argtypes = [ci, vp]
            L.emu_sim3_max_error.argtypes = [cf]
            L.emu_sim3_max_error.restype = cf
            L.emu_sim3_subsets.argtypes = [u32, ci, ci, vp]
            L.emu_sim3_subsets.restype = None
            L.emu_sim3_prepare.argtypes = [vp, vp, ci, vp, vp]
            L.emu_sim3_prepare.restype = None
            L.emu_sim3_compute_t.argtypes = [vp, vp, vp, vp]
            L.emu_sim3_check_inliers.argtypes = [vp] * 8 + [ci, vp, vp, vp]
            L.emu_sim3_check_inliers.restype = None
            L.emu_sim3_iterations_ahead.argtypes = [ci, ci, ci]
            L.emu_sim3_replay.argtypes = [vp, vp, ci, ci, ci, vp]
            L.emu_sim3_replay.restype = None
            L.emu_sim3_sincos.argtypes = [ci, vp, vp, vp]
            L.emu_sim3_sincos.restype = None
            L.emu_sim3_atan2_pos.argtypes = [ci, vp, vp, vp]
            L.emu_sim3_atan2_pos.restype = None
            L.emu_sim3_rotation.argtypes = [ci, vp, vp]
            L.emu_sim3_rotation.restype = None
            L.emu_sim3solver_set_create.argtypes = [vp, ci, ci, vp]
            L.emu_sim3solver_set_destroy.argtypes = [vp]
            L.emu_sim3solver_set_destroy.restype = None
            L.emu_sim3solver_set_clear.argtypes = [vp]
            L.emu_sim3solver_add.argtypes = [vp, vp, vp, vp, vp, vp, ci, ci, vp, vp, vp, vp]
            L.emu_sim3solver_set_ransac_parameters.argtypes = [vp, ci, vp]
            L.emu_sim3solver_query.argtypes = [vp, ci, vp]
            L.emu_sim3solver_iterate.argtypes = [vp, vp, ci, ci, vp, vp]
            L.emu_sim3solver_find.argtypes = [vp, ci, vp, vp]
            L.emu_sim3solver_hypotheses.argtypes = [vp, ci, vp, vp, vp, vp, ci, vp]
            Emu._libs[mutation] = L
        self.L = Emu._libs[mutation]

    def derive(self, n, params):
        return int(self.L.emu_sim3_derive(n, ctypes.byref(params)))

    def max_error(self, sigma2):
        return np.array([self.L.emu_sim3_max_error(float(v)) for v in np.asarray(sigma2, np.float32)], np.float32)

    def subsets(self, seed, n, count):
        out = np.zeros((count, 3), np.int32)
        self.L.emu_sim3_subsets(seed, n, count, _p(out))
        return out

    def prepare(self, uvo, kf, xw):
        xw = np.ascontiguousarray(xw, np.float32).reshape(-1, 3)
        k = uvo.Sim3KeyFrame.make(*kf)
        xc, uv = np.zeros((len(xw), 3), np.float32), np.zeros((len(xw), 2), np.float32)
        self.L.emu_sim3_prepare(ctypes.byref(k), _p(xw), len(xw), _p(xc), _p(uv))
        return xc, uv

    def compute_t(self, x1c, x2c, idx):
        x1c, x2c, idx = np.ascontiguousarray(x1c, np.float32), np.ascontiguousarray(x2c, np.float32), np.ascontiguousarray(idx, np.int32)
        out = np.zeros(48, np.float32)
        ok = self.L.emu_sim3_compute_t(_p(x1c), _p(x2c), _p(idx), _p(out))
        return bool(ok), dict(T12=out[:16].reshape(4, 4).copy(), T21=out[16:32].reshape(4, 4).copy(), R=out[32:41].reshape(3, 3).copy(), t=out[41:44].copy(),
                              s=out[44])

    def check_inliers(self, T12, T21, x1c, x2c, p1, p2, e1, e2, K1, K2):
        a = [np.ascontiguousarray(v, np.float32) for v in (T12, T21, x1c, x2c, p1, p2, e1, e2)]
        k1, k2 = np.array(K1, np.float32), np.array(K2, np.float32)
        inl = np.zeros(len(a[2]), np.uint8)
        self.L.emu_sim3_check_inliers(*[_p(v) for v in a], len(a[2]), _p(k1), _p(k2), _p(inl))
        return inl.astype(bool)

    def replay(self, iterations, best, counts, n_iterations, max_its, min_inliers):
        state, out = np.array([iterations, best], np.int32), np.zeros(5, np.int32)
        counts = np.ascontiguousarray(counts, np.int32)
        self.L.emu_sim3_replay(_p(state), _p(counts), n_iterations, max_its, min_inliers, _p(out))
        return dict(performed=int(out[0]), returned=int(out[1]), no_more=int(out[2]), inliers=int(out[3]), best_from=int(out[4]), iterations=int(state[0]),
                    best=int(state[1]))

    def sincos(self, th):
        th = np.ascontiguousarray(th, np.float64)
        s, c = np.zeros_like(th), np.zeros_like(th)
        self.L.emu_sim3_sincos(len(th), _p(th), _p(s), _p(c))
        return s, c

    def atan2_pos(self, y, x):
        y, x = np.ascontiguousarray(y, np.float64), np.ascontiguousarray(x, np.float64)
        out = np.zeros_like(y)
        self.L.emu_sim3_atan2_pos(len(y), _p(y), _p(x), _p(out))
        return out

    def rotation(self, q):
        q = np.ascontiguousarray(q, np.float32).reshape(-1, 4)
        R = np.zeros((len(q), 9), np.float32)
        self.L.emu_sim3_rotation(len(q), _p(q), _p(R))
        return R

    def make_set(self, uvo, max_solvers, max_points):
        """The host build behind the product's own Python class."""
        cls = type("EmuSim3SolverSet", (uvo.Sim3SolverSet,), {"_prefix": "emu_sim3solver_"})
        return cls(None, max_solvers, max_points, _api=self.L)


# ---- one scripted session on any implementation ----------------------------------------------------------------------------------
class Call:
    """What one iterate call gave: the result, the generator state afterwards, each listed solver's tap and counters."""

    def __init__(self, ids, n_iterations, result, rng_state, taps, infos):
        self.ids, self.n_iterations, self.result, self.rng_state, self.taps, self.infos = ids, n_iterations, result, rng_state, taps, infos


def add_candidate(sset, cand, params):
    x1w, x2w, sg1, sg2, index1, nm, kf1, kf2 = cand[:8]
    return sset.add(x1w, x2w, sg1, sg2, index1, nm, kf1, kf2, params)


def run_session(uvo, sset, candidates, calls, params=None, seed=1):
    """Add `candidates` (sm.candidate tuples) to the empty set, then make the listed calls on one generator seeded with `seed`:
    (ids, n_iterations) is iterate, (ids, FIND) is find() on ids[0], ("set", id, params) is SetRansacParameters again.  -> [Call]
    (a "set" entry gives a Call with result None and the solver's counters afterwards)."""
    prm = params if params is not None else uvo.Sim3SolverParams()
    sset.clear()
    for c in candidates:
        add_candidate(sset, c, prm)
    rng = uvo.GlibcRand(seed)
    out = []
    tup = lambda f: (f.n, f.max_its, f.iterations, f.best_inliers)
    for call in calls:
        if call[0] == "set":
            sset.set_ransac_parameters(call[1], call[2])
            out.append(Call([call[1]], call[2], None, rng.state(), [], [tup(sset.query(call[1]))]))
            continue
        ids, n_it = call
        res = sset.find(ids[0], rng) if n_it == FIND else sset.iterate(ids, n_it, rng)
        taps = [sset.hypotheses(i) for i in ids]
        out.append(Call(list(ids), n_it, res, rng.state(), taps, [tup(sset.query(i)) for i in ids]))
    return out


def _key(r):
    return (r.returned, r.solver, r.n_inliers, r.draws)


def assert_sessions_equal(a, b, what=""):
    """Two implementations' sessions, bit for bit: subsets, every hypothesis T12 / T21 and count, masks, T12, R, t, s, nInliers, bNoMore,
    mnIterations, the generator state handed back."""
    assert len(a) == len(b), what
    for k, (x, y) in enumerate(zip(a, b)):
        w = "%s call %d" % (what, k)
        assert x.rng_state == y.rng_state, w
        assert x.infos == y.infos, (w, x.infos, y.infos)
        if x.result is None:
            assert y.result is None, w
            continue
        rx, ry = x.result, y.result
        assert _key(rx) == _key(ry), (w, _key(rx), _key(ry))
        for name in ("T12", "R", "t", "s"):
            assert np.asarray(getattr(rx, name)).tobytes() == np.asarray(getattr(ry, name)).tobytes(), (w, name, getattr(rx, name), getattr(ry, name))
        np.testing.assert_array_equal(rx.status, ry.status, err_msg=w)
        np.testing.assert_array_equal(rx.inliers, ry.inliers, err_msg=w)
        for j, (tx, ty) in enumerate(zip(x.taps, y.taps)):
            np.testing.assert_array_equal(tx[0], ty[0], err_msg="%s solver %d subsets" % (w, x.ids[j]))
            np.testing.assert_array_equal(tx[3], ty[3], err_msg="%s solver %d counts" % (w, x.ids[j]))
            for e, name in ((1, "T12"), (2, "T21")):
                assert tx[e].tobytes() == ty[e].tobytes(), ("%s solver %d %s" % (w, x.ids[j], name), np.abs(tx[e] - ty[e]).max())


# ---- the layers --------------------------------------------------------------------------------------------------------------------
def check_tables(uvo, emu):
    """Layer 2: the derived parameters and the thresholds, exactly."""
    for n, want in sm.CALL_SITE_TABLE.items():
        assert emu.derive(n, uvo.Sim3SolverParams(**sm.CALL_SITE)) == sm.derive_params(n, **sm.CALL_SITE) == want, n
    for n, want in sm.HEADER_TABLE.items():
        assert emu.derive(n, uvo.Sim3SolverParams(**sm.HEADER_DEFAULT)) == sm.derive_params(n, **sm.HEADER_DEFAULT) == want, n
    for prm in (sm.CALL_SITE, sm.HEADER_DEFAULT, dict(probability=0.999, min_inliers=20, max_iterations=50), dict(probability=0.5, min_inliers=0, max_iterations=7)):
        for n in range(3, 400):
            assert emu.derive(n, uvo.Sim3SolverParams(**prm)) == sm.derive_params(n, **prm), (prm, n)
    sigma2 = np.concatenate([(np.float32(1.2) ** (2 * np.arange(8))).astype(np.float32), np.float32([1.0, 1.44, 0.0, 0.1, 2.5, 1e6])])
    np.testing.assert_array_equal(emu.max_error(sigma2), sm.thresholds(sigma2))
    assert emu.max_error([1.0])[0] == 9 and emu.max_error([1.44])[0] == 13


def check_subsets(emu, ns=(3, 4, 5, 8, 15, 40), count=3000):
    """Layer 1, the draw alone: `count` triples from seed 1 per N, and the repeating triples among them."""
    for n in ns:
        g = sm.GlibcRand(1)
        want = np.array([sm.draw_subset(g, n, 3) for _ in range(count)], np.int32)
        got = emu.subsets(1, n, count)
        np.testing.assert_array_equal(got, want, err_msg="N = %d" % n)
        repeats = int(sum(len(set(r)) < 3 for r in got.tolist()))
        if count == 3000 and n in sm.REPEATS_OF_3000:
            assert repeats == sm.REPEATS_OF_3000[n], (n, repeats)


def _row_bound(T):
    """2 float ulp of the larger magnitude of each row."""
    return 2 * np.spacing(np.abs(np.asarray(T, np.float32)).max(1)).astype(np.float64)[:, None]


def check_session_against_model(uvo, emu, session, candidates, params=None, seed=1, what=""):
    """Layers 1-5 at the session's own hypotheses: the random stream and its continuity from solver to solver and call to call; the
    derived parameters; every T12 against sm.compute_t on the same triple (2 float ulp of its row) and against sm.horn64 on the
    well-conditioned triples (sm.HORN_TOL); CheckInliers at the run's own T12 / T21 up to the model's near mask; the replay at the
    run's own counts.  -> dict(hypotheses, horn_checked, worst_horn, worst_ulp)."""
    prm = params if params is not None else uvo.Sim3SolverParams()
    g = sm.GlibcRand(seed)
    ref = uvo.GlibcRand(seed)
    cur = {}     # solver id -> its parameters now
    state = {}   # solver id -> [mnIterations, best]
    prep = {}
    stats = dict(hypotheses=0, horn_checked=0, worst_horn=0.0, worst_ulp=0.0)
    for k, call in enumerate(session):
        w = "%s call %d" % (what, k)
        if call.result is None:      # SetRansacParameters again: iterations zeroed, the best kept, max_its anew
            sid, p = call.ids[0], call.n_iterations
            cur[sid] = p
            n = len(candidates[sid][0])
            it0, best0 = state.setdefault(sid, [0, 0])
            state[sid] = [0, best0]
            assert call.infos[0] == (n, sm.derive_params(n, p.probability, p.min_inliers, p.max_iterations), 0, best0), (w, call.infos)
            assert call.rng_state == ref.state(), w
            continue
        res = call.result
        for name in ("T12", "R", "t", "s"):
            assert np.isfinite(getattr(res, name)).all(), (w, name)
        draws = 0
        stopped = False
        for j, sid in enumerate(call.ids):
            x1w, x2w, sg1, sg2, index1, nm, kf1, kf2 = candidates[sid][:8]
            n = len(x1w)
            p = cur.get(sid, prm)
            it0, best0 = state.setdefault(sid, [0, 0])
            sub, T12s, T21s, cnt = call.taps[j]
            touched, no_more, its_after = (int(v) for v in res.status[j])
            if stopped:
                assert (touched, no_more, its_after, len(cnt)) == (0, 0, it0, 0), (w, sid)
                continue
            assert touched == 1, (w, sid)
            max_its = sm.derive_params(n, p.probability, p.min_inliers, p.max_iterations)
            assert call.infos[j][:2] == (n, max_its), (w, sid, call.infos[j])
            if n < p.min_inliers or n < 3:
                assert (no_more, its_after, len(cnt)) == (1, it0, 0) and res.returned != j, (w, sid)
                continue
            n_it = max_its if call.n_iterations == FIND else call.n_iterations
            # layer 1: this solver's subsets continue where the last one stopped
            performed = len(cnt)
            want = [sm.draw_subset(g, n, 3) for _ in range(performed)]
            np.testing.assert_array_equal(sub, np.array(want, np.int32).reshape(performed, 3), err_msg="%s solver %d subsets" % (w, sid))
            draws += 3 * performed
            assert np.isfinite(T12s).all() and np.isfinite(T21s).all() and its_after == it0 + performed == call.infos[j][2], (w, sid)
            if sid not in prep:
                (x1c, p1), (x2c, p2) = sm.prepare(kf1, x1w), sm.prepare(kf2, x2w)
                prep[sid] = (x1c, x2c, p1, p2, sm.thresholds(sg1), sm.thresholds(sg2))
            x1c, x2c, p1, p2, e1, e2 = prep[sid]
            for h in range(performed):
                stats["hypotheses"] += 1
                P1, P2 = x1c[sub[h]].T, x2c[sub[h]].T
                m = sm.compute_t(P1, P2)
                T12, T21 = T12s[h].reshape(4, 4), T21s[h].reshape(4, 4)
                # layer 3: the transform
                if not m["finite"]:
                    assert not T12.any() and not T21.any() and cnt[h] == 0, (w, sid, h, "the model's transform is not finite")
                    continue
                assert T12.any(), (w, sid, h, "no transform where the model has one", m["T12"])
                d = np.abs(T12.astype(np.float64) - m["T12"].astype(np.float64))
                bound = _row_bound(m["T12"])
                stats["worst_ulp"] = max(stats["worst_ulp"], float((d[:3] / bound[:3] * 2).max()))
                assert (d <= bound).all(), (w, sid, h, sub[h], T12, m["T12"])
                if sm.well_conditioned(P1, P2, sub[h]):
                    s64, R64, t64 = sm.horn64(P1, P2)
                    dev = sm.sim3_deviation(1.0, T12[:3, :3], T12[:3, 3], s64, R64, t64)
                    stats["horn_checked"] += 1
                    stats["worst_horn"] = max(stats["worst_horn"], dev)
                    assert dev <= sm.HORN_TOL, (w, sid, h, sub[h], dev, sm.HORN_TOL)
                # layer 4: CheckInliers at the run's own transform
                _, _, inl, near = sm.check_inliers(T12, T21, x1c, x2c, p1, p2, kf1[2], kf2[2], e1, e2)
                lo, hi = int((inl & ~near).sum()), int((inl | near).sum())
                assert lo <= cnt[h] <= hi, (w, sid, h, int(cnt[h]), lo, hi)
            # layer 5: the replay at the run's own counts
            returned_here = res.returned == j
            m = sm.replay(it0, best0, list(cnt) + [0] * 400, n_it, max_its, p.min_inliers)
            assert m["performed"] == performed, (w, sid, m, performed)
            assert (m["returned"] >= 0) == returned_here, (w, sid, m)
            assert (m["no_more"], m["iterations"], m["best"]) == (no_more, its_after, call.infos[j][3]), (w, sid, m, call.infos[j])
            state[sid] = [m["iterations"], m["best"]]
            if not returned_here:
                continue
            stopped = True
            h = m["returned"]
            assert (res.solver, res.n_inliers) == (sid, m["inliers"]) and res.n_inliers > p.min_inliers, (w, sid, m)
            assert res.T12.tobytes() == T12s[h].tobytes(), (w, sid)
            assert res.T12[:3, 3].tobytes() == res.t.tobytes() and (res.T12[3] == [0, 0, 0, 1]).all(), (w, sid)
            assert res.T12[:3, :3].tobytes() == (np.float64(res.s) * res.R.astype(np.float64)).astype(np.float32).tobytes(), (w, sid)
            assert abs(np.linalg.det(res.R.astype(np.float64)) - 1) < 1e-5, (w, sid)
            assert len(res.inliers) == nm and int(res.inliers.sum()) == res.n_inliers, (w, sid)
            assert not np.delete(res.inliers, index1).any(), (w, sid)          # nothing outside mvnIndices1
            got = res.inliers[index1].astype(bool)
            np.testing.assert_array_equal(got, emu.check_inliers(T12s[h], T21s[h], x1c, x2c, p1, p2, e1, e2, kf1[2], kf2[2]), err_msg=w)
            _, _, inl, near = sm.check_inliers(T12s[h], T21s[h], x1c, x2c, p1, p2, kf1[2], kf2[2], e1, e2)
            assert ((got == inl) | near).all(), (w, sid)
        assert res.draws == draws, (w, res.draws, draws)
        if not stopped:
            assert (res.returned, res.solver, res.n_inliers) == (-1, -1, 0) and not res.T12.any() and not res.R.any() and len(res.inliers) == 0, w
        for _ in range(draws):
            ref.next()
        assert call.rng_state == ref.state(), w
    return stats
