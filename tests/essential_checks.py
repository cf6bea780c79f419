"""The checks that hold an implementation of the essential-graph optimisation to tests/essential_model.py, layer by layer, and the
driver of the host build (tests/emu/essential_emu.cpp).  tests/test_essential_emu.py runs them on the host build and on its eight
seeded mutations, tests/test_gpu_essential.py on the device (the layers the trace and the result show).

Every bound is derived beside its check from the precision of the formats (u = 2^-53) and an operation count; T alone is measured,
and it is measured on the MODEL (measure_spread), never on the code under test.

    layer 0  log_ against math.log at the bound stated beside essential::log_; acos_ieee against math.acos
    layer 1  g2o::Sim3: product, inverse, log() in its four branches, the update Sim3(dx) * S
    layer 2  one linearisation: measurements, errors and Jacobian columns against the model (2a); H's blocks, b and chi2 against what
             numpy assembles from the build's OWN errors and Jacobians (2b: rounding only, so a wrong block cannot hide in 2a's noise)
    layer 3  (a) the envelope solve against ba::ldlt_solve on the same matrix, bit for bit; (b) one trial on the model's estimate and
             lambda: the residual of the solve, the update, tmp and scale; (c) the driver's rules replayed exactly on the trace's own
             records; (d) the trajectory against the model's, trial by trial, over the prefix on which the model's margins allow it
    layer 4  the call: Scw, poses and points within T, counts"""
import ctypes
import math
import os

import numpy as np

import essential_model as em
import host_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
DBL_MAX = em.DBL_MAX
MUTATIONS = {"MEASURE_SCW": 1, "ONESIDED": 2, "SWAPPED": 3, "LAMBDA_TAU": 4, "FIXED_KEPT": 5, "ENVELOPE_SHORT": 6, "ORDER_REVERSED": 7, "POINTS_UNCORRECTED": 8}

# the artefacts of this feature, declared here (tests/host_build.py's table is not edited) and built by its function
EMU = host_build.Artefact("tests/emu/libessential_emu.so", "tests/emu/essential_emu.cpp", host_build.CXX, host_build.SHARED + host_build.NO_FMA, [])
EMU_MAIN = host_build.Artefact("tests/emu/essential_emu", "tests/emu/essential_emu.cpp", host_build.CXX, host_build.PROGRAM + ["-DESSENTIAL_EMU_MAIN"], [])

# ---- T -------------------------------------------------------------------------------------------------------------------------------------
# measure_spread(list(em.SCENES), orders=8, ext=("mp",)) on the model (`python tests/essential_checks.py`; minutes: too slow for the
# suite, which repeats it on the scenes that set the maxima, tests/test_essential_model.py): the largest difference of the final
# (q, t, s) and of the corrected points between the model as written and (a) the model over 8 random orders of the edges, (b) the model
# with every EdgeSim3 error evaluated in mpmath at 50 digits and rounded to double where g2o stores a double.  (b) removes the rounding
# noise of the evaluation, which the 1e-9 difference amplifies by 5e8.  A variant whose accept / reject sequence differs from the
# model's is counted apart (UNCLEAR) and sets no maximum.  Times four: the code under test differs from the model in more ways at once
# than either variant does (the sums' shapes AND its own log / acos / sin / cos / exp AND another solver order).
EST_SPREAD = 2.3e-4         # measured 2.297e-04 (rejected)
PTS_SPREAD = 5.9e-4         # measured 5.884e-04 (rejected): the points of a key frame that moves by EST_SPREAD, mapped back through its inverse
CHI2_REL_SPREAD = 1.7e-5    # measured 1.673e-05 (rejected): the chi2 an accepted trial reaches, relative to the chi2 it started from
SPREAD_SCENES = ("rejected",)
T_EST = 4 * EST_SPREAD
T_PTS = 4 * PTS_SPREAD
M_REL = 4 * CHI2_REL_SPREAD


def model(name, _cache={}):
    if name not in _cache:
        sc = em.make(name)
        _cache[name] = (sc, em.optimize(sc))
    return _cache[name]


def measure_spread(names, orders=8, ext=("mp",), seed=7, detail=None):
    """-> (estimate spread, points spread, unclear scenes) of the model over `orders` random edge orders and the evaluations in `ext`.
    detail: a dict that receives per scene the two spreads and the relative spread of the trials' chi2 (tmp)."""
    est = pts = 0.0
    unclear = []
    for name in names:
        sc, base = model(name)
        E = len(sc["edge_i"])
        g = np.random.default_rng([seed, list(em.SCENES).index(name)])
        variants = [em.optimize(sc, order=g.permutation(E)) for _ in range(orders)] + [em.optimize(sc, ext=e) for e in ext]
        e_here = p_here = c_here = 0.0
        for v in variants:
            if [t["accepted"] for t in v.trials] != [t["accepted"] for t in base.trials]:
                if name not in unclear:
                    unclear.append(name)
                continue
            e_here = max(e_here, float(np.abs(v.S - base.S).max()))
            c_here = max([c_here] + [abs(a["tmp"] - b["tmp"]) / abs(b["cur"]) for a, b in zip(v.trials, base.trials) if b["accepted"]])
            if len(base.points):
                p_here = max(p_here, float(np.abs(v.points.astype(np.float64) - base.points.astype(np.float64)).max()))
        if detail is not None:
            detail[name] = (e_here, p_here, c_here)
        est, pts = max(est, e_here), max(pts, p_here)
    return est, pts, unclear


# ---- the host build ------------------------------------------------------------------------------------------------------------------------
class Run:
    def __init__(self, S, Tcw, points, counts, trace):
        self.S, self.Tcw, self.points = S, Tcw, points
        self.iterations, self.n_trials, self.n_syncs, self.envelope_blocks = [int(v) for v in counts]
        self.trace = trace


def of_result(r, trace):
    """A uvo.EssentialResult and its trace as a Run."""
    return Run(r.Scw, r.kf_Tcw, r.points, (r.iterations, r.n_trials, r.n_syncs, r.envelope_blocks), trace)


class Emu:
    """tests/emu/essential_emu.cpp, built on first use with the library's contract: no FMA contraction.  `mutation`: a key of
    MUTATIONS, compiled into a library of its own."""
    _libs = {}

    def __init__(self, uvo, mutation=None):
        assert mutation is None or mutation in MUTATIONS
        self.uvo = uvo
        if mutation not in Emu._libs:
            variant = dict(extra=["-DESSENTIAL_MUT=%d" % MUTATIONS[mutation]], suffix="_" + mutation.lower()) if mutation else {}
            L = ctypes.CDLL(host_build.compile_artefact(EMU, **variant))
            vp, ci, cd = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
            L.emu_essential_log.argtypes, L.emu_essential_log.restype = [cd], cd
            L.emu_essential_acos.argtypes, L.emu_essential_acos.restype = [cd], cd
            L.emu_essential_mul.argtypes = [vp, vp, vp]
            L.emu_essential_inv.argtypes = [vp, vp]
            L.emu_essential_log7.argtypes = [vp, vp]
            L.emu_essential_oplus.argtypes = [vp, vp, vp]
            L.emu_essential_optimize.argtypes = [vp, ci, vp, vp]
            L.emu_essential_one_trial.argtypes = [vp, vp, cd] + [vp] * 9
            L.emu_essential_envelope_solve.argtypes = [ci, vp, vp, vp, vp, vp]
            L.emu_essential_dense_solve.argtypes = [ci, vp, vp, vp]
            assert L.emu_essential_mutation() == (MUTATIONS[mutation] if mutation else 0)
            Emu._libs[mutation] = L
        self.L = Emu._libs[mutation]

    def log(self, x):
        return float(self.L.emu_essential_log(float(x)))

    def acos(self, x):
        return float(self.L.emu_essential_acos(float(x)))

    def _sim(self, fn, *args, n=8):
        args = [np.ascontiguousarray(a, np.float64) for a in args]
        out = np.zeros(n)
        fn(*[a.ctypes.data for a in args], out.ctypes.data)
        return out

    def mul(self, a, b):
        return self._sim(self.L.emu_essential_mul, a, b)

    def inv(self, a):
        return self._sim(self.L.emu_essential_inv, a)

    def log7(self, a):
        return self._sim(self.L.emu_essential_log7, a, n=7)

    def oplus(self, dx, a):
        return self._sim(self.L.emu_essential_oplus, dx, a)

    def optimize(self, sc, max_blocks=1 << 22, n_iterations=None):
        """-> Run, or the integer code of a refused graph."""
        c, r, arrays, keep = self.uvo.essential_marshal(sc, n_iterations)
        t = self.uvo.BaTraceC()
        rc = self.L.emu_essential_optimize(ctypes.addressof(c), max_blocks, ctypes.addressof(r), ctypes.addressof(t))
        if rc:
            return rc
        return Run(arrays[0], arrays[1], arrays[2], (r.iterations, r.n_trials, r.n_syncs, r.envelope_blocks), self.uvo.BaTrace(t))

    def one_trial(self, sc, est, lam):
        c, r, arrays, keep = self.uvo.essential_marshal(sc)
        K, E = c.n_keyframes, c.n_edges
        N = 7 * (K - 1)
        est = np.ascontiguousarray(est, np.float64)
        dims, meas, lin, H, first = np.zeros(4, np.int32), np.zeros((max(E, 1), 8)), np.zeros((max(E, 1), 105)), np.zeros((max(N, 1), max(N, 1))), np.zeros(max(K, 1), np.int32)
        b, x, est_try, scal = np.zeros(max(N, 1)), np.zeros(max(N, 1)), np.zeros((K, 8)), np.zeros(4)
        rc = self.L.emu_essential_one_trial(ctypes.addressof(c), est.ctypes.data, float(lam), dims.ctypes.data, meas.ctypes.data, lin.ctypes.data, H.ctypes.data,
                                            first.ctypes.data, b.ctypes.data, x.ctypes.data, est_try.ctypes.data, scal.ctypes.data)
        assert rc == 0, rc
        lin = lin[:E]
        return dict(F=int(dims[0]), NP=int(dims[1]), NB=int(dims[2]), ok=bool(dims[3]), meas=meas[:E], e=lin[:, :7], Ji=lin[:, 7:56].reshape(E, 7, 7),
                    Jj=lin[:, 56:].reshape(E, 7, 7), H=H[:N, :N], first=first[:K - 1], b=b[:N], x=x[:N], est_try=est_try, chi2=scal[0], maxdiag=scal[1],
                    tmp=scal[2], scale=scal[3])

    def envelope_solve(self, first, A, rhs):
        """-> ok, x, the factor (dense lower triangle)."""
        first, A, rhs = np.ascontiguousarray(first, np.int32), np.ascontiguousarray(A, np.float64), np.ascontiguousarray(rhs, np.float64)
        x, Lo = np.zeros(len(rhs)), np.zeros_like(A)
        ok = self.L.emu_essential_envelope_solve(len(first), first.ctypes.data, A.ctypes.data, rhs.ctypes.data, x.ctypes.data, Lo.ctypes.data)
        assert ok >= 0
        return bool(ok), x, Lo

    def dense_solve(self, A, rhs):
        A, rhs = np.array(np.tril(A), np.float64, order="C"), np.ascontiguousarray(rhs, np.float64)
        x = np.zeros(len(rhs))
        ok = self.L.emu_essential_dense_solve(len(rhs), A.ctypes.data, rhs.ctypes.data, x.ctypes.data)
        return bool(ok), x, np.tril(A)


def same_bits(a, b):
    """Equal bit for bit, non-finite values by class, zeros of either sign alike."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return False
    return bool(np.array_equal(a, b, equal_nan=a.dtype.kind == "f"))


def same_run(x, y):
    """-> the list of fields in which two runs differ."""
    bad = [k for k in ("S", "Tcw", "points") if not same_bits(getattr(x, k), getattr(y, k))]
    bad += [k for k in ("iterations", "n_trials", "n_syncs", "envelope_blocks") if getattr(x, k) != getattr(y, k)]
    for rec in ("lin", "trial"):
        a, b = getattr(x.trace, rec), getattr(y.trace, rec)
        if len(a) != len(b):
            bad.append("trace.%s count" % rec)
        else:
            bad += ["trace.%s.%s" % (rec, f) for f in a.dtype.names if not same_bits(a[f], b[f])]
    return bad


# ---- layer 0 ---------------------------------------------------------------------------------------------------------------------------------
LOG_BOUND = 2.0 ** -50    # relative to |log x|; derived beside essential::log_, with math.log's own ulp inside it


def check_log(f):
    g = [1.0, 1 + 1e-9, 1 - 1e-9, 1 + 1e-5, 1 - 1e-5, math.exp(1e-5), math.exp(-1e-5), 2.0 ** -60, 2.0 ** 60, math.sqrt(2), math.sqrt(0.5), math.nextafter(math.sqrt(2), 2),
         math.nextafter(math.sqrt(0.5), 0), 0.8, 1.3, 2.0, 0.5, 4.0, 1e-3, 1e3]
    g += list(np.exp(np.linspace(-41, 41, 4001))) + list(1 + np.random.default_rng(1).normal(size=2000) * 1e-3) + list(np.linspace(0.7, 1.42, 2001))
    worst = 0.0
    for x in g:
        got, ref = f(x), math.log(x)
        err = abs(got - ref)
        assert err <= LOG_BOUND * abs(ref), (x, got, ref)
        worst = max(worst, err / (LOG_BOUND * abs(ref)) if ref else 0.0)
    assert f(1.0) == 0.0
    for x in (0.0, -1.0, 2.0 ** -61, 2.0 ** 61, float("inf"), float("nan")):
        assert math.isnan(f(x)), x
    return worst


def check_acos(f):
    """sim3::atan2_pos is accurate to 2^-51 absolute (stated beside it); the root of (1 - x)(1 + x) carries 2 u relative, which the
    arctangent passes on at most as 2 u * pi: together below 1e-15 + 4 eps pi, the bound tests/test_initializer_emu.py holds it to."""
    x = np.concatenate([np.linspace(-1, 1, 4001), 1 - np.logspace(-16, -1, 200), [1 - 1e-5, 1 - 1e-5 * (1 + 1e-6), 1 - 1e-5 * (1 - 1e-6)]])
    got = np.array([f(v) for v in x])
    assert np.abs(got - np.arccos(x)).max() < 1e-15 + 4 * np.finfo(np.float64).eps * np.pi
    assert all(math.isnan(f(v)) for v in (1.0000001, -2.0, float("nan")))


# ---- layer 1 ---------------------------------------------------------------------------------------------------------------------------------
def random_sim(g, rot=1.0, tr=5.0, smin=0.8, smax=1.3):
    q = em.quat_of(em._rodrigues(g.normal(size=3) * rot)) * (1 + 1e-3 * g.normal())   # not normalised, as g2o's are after products
    return np.concatenate([q, g.normal(size=3) * tr, [g.uniform(smin, smax)]])


def sim_bound(*sims):
    """An absolute bound on a short chain of Sim3 operations on these operands: 64 roundings, each of half an ulp of a value that is at
    most the product of the operands' magnitudes (|q|^2 <= 1.01, a scale, the largest translation + 1)."""
    mag = 1.0
    for s in sims:
        s = np.asarray(s)
        mag *= max(1.0, float(np.abs(s[..., 7]).max()), 1.0 / float(np.abs(s[..., 7]).min())) * 1.01
    t = 1.0 + sum(float(np.abs(np.asarray(s)[..., 4:7]).max()) for s in sims)
    return 64 * U * mag * t


def log_bound(S):
    """log() of S: d carries 4 u; acos amplifies it by 1 / sin(theta), at most 1 / 0.0045 at the branch limit, and omega = f(theta) dR
    follows with less than 1024 u.  upsilon = W^-1 t: W = A Omega + B Omega^2 + C I moves by dW = (|A| + 2 |B| |omega|) 3 d(omega) + 16 u |W|
    (A, B, C themselves: 64 u relative, inside the 16 u |W| with room where they are of order one, and counted apart where B is
    large), t carries sim_bound's rounding, and the solve passes both on through |W^-1|: d(upsilon) <= |W^-1| (dW |upsilon| + 64 u |t|)
    + 64 u cond(W) |upsilon| for the partial-pivot LU itself.  (Where the rotation is below the branch limit and |sigma| above 1e-5 the
    reference's B is of order 1 / sigma^3 and W close to rank 2: the bound follows it.)  sigma is log_'s."""
    S = np.asarray(S, np.float64)
    out, A, B, W = em.sim_log(S[None], parts=True)
    om, ups, W = out[0, :3], out[0, 3:6], W[0]
    t = 1.0 + float(np.abs(S[4:7]).max())
    d_om = 1024 * U
    if not np.isfinite(W).all() or not np.isfinite(ups).all():
        return np.full(7, np.inf)
    Wi = float(np.abs(np.linalg.inv(W)).sum(1).max())
    Wn = float(np.abs(W).sum(1).max())
    dW = (abs(float(A[0])) + 2 * abs(float(B[0])) * float(np.abs(om).max())) * 3 * d_om + 16 * U * Wn + 64 * U * abs(float(B[0])) * float(om @ om)
    d_ups = Wi * (dW * float(np.abs(ups).max()) + 64 * U * t) + 64 * U * Wi * Wn * float(np.abs(ups).max())
    return np.array([d_om] * 3 + [max(d_ups, 64 * U * t)] * 3 + [LOG_BOUND * abs(math.log(S[7])) + 4 * U])


def check_sim_ops(emu, n=300):
    g = np.random.default_rng(11)
    worst = 0.0
    for k in range(n):
        a, b = random_sim(g), random_sim(g)
        for got, ref, bound in ((emu.mul(a, b), em.sim_mul(a, b), sim_bound(a, b)), (emu.inv(a), em.sim_inv(a), sim_bound(a, a))):
            worst = max(worst, float(np.abs(got - ref).max() / bound))
        # log() in its four branches: rotation below and above the branch limit, sigma below and above 1e-5
        rot, s = (1e-4, 1.0) if k % 4 == 0 else (1e-4, 1.2) if k % 4 == 1 else (0.7, 1.0 + 1e-7) if k % 4 == 2 else (0.7, 0.85)
        c = random_sim(g, rot=rot, smin=s, smax=s)
        c[:4] /= np.linalg.norm(c[:4])
        ref = em.sim_log(c)[0]
        branch = (abs(math.log(c[7])) < 1e-5, 0.5 * (em.rotmat(c[:4])[[0, 4, 8]].sum() - 1) > 1 - 1e-5)
        assert branch == (k % 4 in (0, 2), k % 4 in (0, 1)), (k, branch)
        worst = max(worst, float((np.abs(emu.log7(c) - ref) / log_bound(c)).max()))
        # the update in its four branches
        dx = g.normal(size=7) * np.array([1e-7] * 3 + [1] * 3 + [1e-7]) if k % 4 == 0 else g.normal(size=7) * np.array([1e-7] * 3 + [1] * 3 + [0.1]) if k % 4 == 1 else \
            g.normal(size=7) * np.array([0.3] * 3 + [1] * 3 + [1e-7]) if k % 4 == 2 else g.normal(size=7) * np.array([0.3] * 3 + [1] * 3 + [0.1])
        ref = em.sim_mul(em.sim_from_update(dx), a)
        worst = max(worst, float(np.abs(emu.oplus(dx, a) - ref).max() / (4 * sim_bound(a, ref))))
    return worst


# ---- layer 2 ---------------------------------------------------------------------------------------------------------------------------------
def check_linearisation(emu, sc, L, lam):
    """L: the model's linearisation (em.Lin) -> (worst ratio of 2a, worst ratio of 2b, the build's answer)."""
    got = emu.one_trial(sc, L.est, lam)
    meas = em.measure(sc)
    i, j = sc["edge_i"], sc["edge_j"]
    K = len(L.est)
    free = em.free_index(K, sc["fixed"])
    w1 = float(np.abs(got["meas"] - meas).max() / sim_bound(sc["Scw"], sc["Scwn"]))
    # 2a: an error is log() of two products; a Jacobian column is the difference of two such errors times 5e8, in the model and in the
    # build: four evaluations' bounds
    E7 = em.sim_mul(em.sim_mul(meas, L.est[i]), em.sim_inv(L.est[j]))
    eb = np.array([log_bound(s) + sim_bound(meas, L.est, L.est) for s in E7])
    w1 = max(w1, float((np.abs(got["e"] - L.e) / eb).max()))
    jb = 4 * em.SCALAR * eb[:, :, None] * 1.5      # the perturbed estimates' errors are bounded as the unperturbed one's, with room for their own rounding
    for J, Jm, v in ((got["Ji"], L.Ji, i), (got["Jj"], L.Jj, j)):
        on = free[v] >= 0
        if on.any():
            w1 = max(w1, float((np.abs(J[on] - Jm[on]) / jb[on]).max()))
    # 2b: H, b, chi2 from the build's own e and J, in numpy: each entry a sum of n products of 7 terms, (7 n + 2) u times the sum of magnitudes
    F = K - 1
    H, Ha, b, ba = np.zeros((7 * F, 7 * F)), np.zeros((7 * F, 7 * F)), np.zeros(7 * F), np.zeros(7 * F)
    cnt = np.zeros(F)
    for e in range(len(i)):
        a, c = free[i[e]], free[j[e]]
        Ji, Jj = got["Ji"][e], got["Jj"][e]
        for f, J in ((a, Ji), (c, Jj)):
            if f >= 0:
                H[7 * f:7 * f + 7, 7 * f:7 * f + 7] += J.T @ J
                Ha[7 * f:7 * f + 7, 7 * f:7 * f + 7] += np.abs(J).T @ np.abs(J)
                b[7 * f:7 * f + 7] += J.T @ -got["e"][e]
                ba[7 * f:7 * f + 7] += np.abs(J).T @ np.abs(got["e"][e])
                cnt[f] += 1
        if a >= 0 and c >= 0:
            H[7 * a:7 * a + 7, 7 * c:7 * c + 7] += Ji.T @ Jj
            H[7 * c:7 * c + 7, 7 * a:7 * a + 7] += Jj.T @ Ji
            Ha[7 * a:7 * a + 7, 7 * c:7 * c + 7] += np.abs(Ji).T @ np.abs(Jj)
            Ha[7 * c:7 * c + 7, 7 * a:7 * a + 7] += np.abs(Jj).T @ np.abs(Ji)
    n = 7 * (cnt.max() if F else 0) + 2
    low = np.tril(np.ones_like(H, bool))
    w2 = 0.0
    if F:
        w2 = float((np.abs(got["H"] - H)[low] / (2 * n * U * Ha[low] + 1e-300)).max())
        w2 = max(w2, float((np.abs(got["b"] - b) / (2 * n * U * ba + 1e-300)).max()))
        # outside the envelope the graph has no block: the build stores nothing there, and numpy's sum must be zero
        for f in range(F):
            assert not H[7 * f:7 * f + 7, :7 * got["first"][f]].any(), "an edge reaches outside the envelope"
    chi = float((got["e"] ** 2).sum())
    w2 = max(w2, abs(got["chi2"] - chi) / (2 * (7 * len(i) + 2) * U * chi + 1e-300))
    return w1, w2, got


# ---- layer 3 ---------------------------------------------------------------------------------------------------------------------------------
def check_solver(emu, first, A, rhs):
    """The envelope solve and ba::ldlt_solve on the same matrix: x, the factor inside the envelope, ok -- compared with ==."""
    ok1, x1, L1 = emu.envelope_solve(first, A, rhs)
    ok2, x2, L2 = emu.dense_solve(A, rhs)
    N = len(rhs)
    inside = np.zeros((N, N), bool)
    for f, f0 in enumerate(first):
        inside[7 * f:7 * f + 7, 7 * f0:7 * f + 7] = True
    inside &= np.tril(np.ones((N, N), bool))
    assert ok1 == ok2, (ok1, ok2)
    assert np.array_equal(x1, x2, equal_nan=True), float(np.nanmax(np.abs(x1 - x2)))
    assert np.array_equal(L1[inside], L2[inside], equal_nan=True)
    return ok1


def check_trial(emu, sc, got, L, lam):
    """One trial of the build at the model's estimate: the envelope solve equals the dense one on the build's H; the residual of the solve
    is a backward-stable factorisation's, |r| <= 8 N u (|A| |x| + |b|) by norm; the update, tmp and scale follow from the build's own x."""
    N = len(got["b"])
    A = got["H"] + lam * np.eye(N)
    ok = check_solver(emu, got["first"], A, got["b"])
    assert ok == got["ok"]
    if not ok:
        return 0.0
    Af = np.tril(A) + np.tril(A, -1).T
    x = got["x"]
    r = Af @ x - got["b"]
    w = float(np.abs(r).max() / (8 * N * U * (np.abs(Af) @ np.abs(x) + np.abs(got["b"])).max()))
    est = em.apply(sc, L.est, x)
    w = max(w, float(np.abs(got["est_try"] - est).max() / (4 * sim_bound(L.est, est))))
    meas = em.measure(sc)
    e = em.edge_errors(meas, got["est_try"][sc["edge_i"]], got["est_try"][sc["edge_j"]])
    E7 = em.sim_mul(em.sim_mul(meas, got["est_try"][sc["edge_i"]]), em.sim_inv(got["est_try"][sc["edge_j"]]))
    eb = np.array([log_bound(s) + sim_bound(meas, got["est_try"], got["est_try"]) for s in E7])
    chi, chib = float((e ** 2).sum()), float((2 * np.abs(e) * eb + eb ** 2).sum())
    w = max(w, abs(got["tmp"] - chi) / (chib + 2 * (7 * len(e) + 2) * U * chi))
    terms = x * (lam * x + got["b"])
    w = max(w, abs(got["scale"] - (terms.sum() + 1e-3)) / (2 * (N + 4) * U * (np.abs(x) * (lam * np.abs(x) + np.abs(got["b"]))).sum() + 2 * U))
    return w


def check_layers(emu, name):
    """Layers 2 and 3 on the model's own estimates: at its first linearisation with the user's lambda, at its last with its last
    trial's, and at its first rejected trial with that trial's -> [(2a, 2b, 3b)] worst difference / bound each."""
    sc, res = model(name)
    cases = [(res.lin[0], em.LAMBDA_INIT), (res.lin[-1], res.trials[-1]["lam"])]
    rej = [t for t in res.trials if t["ok"] and not t["accepted"]]
    if rej:
        cases.append((res.lin[rej[0]["lin"]], rej[0]["lam"]))
    out = []
    for L, lam in cases:
        w1, w2, got = check_linearisation(emu, sc, L, lam)
        out.append((w1, w2, check_trial(emu, sc, got, L, lam)))
    return out


def replay(run, n_iterations):
    """The driver's rules on the trace's own records, exactly -> the list of what does not follow."""
    lin, tr, bad = run.trace.lin, run.trace.trial, []
    if run.iterations != len(lin) or run.n_trials != len(tr) or run.n_syncs != len(tr) + 1 or len(lin) > n_iterations:
        bad.append("counts")
    lam, ni, n_bad, k, stop = em.LAMBDA_INIT, 2.0, 0, 0, False
    for it in range(len(lin)):
        if stop:
            bad.append("linearisation %d after the driver stops" % it)
        cur = ini = lin["chi2"][it]
        if lin["iteration"][it] != it:
            bad.append("lin %d iteration" % it)
        q, rho = 0, 0.0
        while True:
            if k >= len(tr):
                bad.append("the trace ends inside iteration %d" % it)
                return bad
            t = tr[k]
            k += 1
            if t["lin"] != it or t["lambda"] != lam or not (t["cur"] == cur):
                bad.append("trial %d: lin, lambda or cur (%r, %r)" % (k - 1, float(t["lambda"]), lam))
            if not t["ok"] and t["tmp"] != DBL_MAX:
                bad.append("trial %d: a failed solve's tmp" % (k - 1))
            with np.errstate(all="ignore"):
                rho = (cur - t["tmp"]) / t["scale"]
            accepted = bool(rho > 0 and np.isfinite(t["tmp"]))
            if bool(t["accepted"]) != accepted:
                bad.append("trial %d: accepted" % (k - 1))
            if accepted:
                alpha = min(1.0 - (2 * rho - 1) * (2 * rho - 1) * (2 * rho - 1), 2.0 / 3.0)
                lam, ni, cur = lam * max(1.0 / 3.0, alpha), 2.0, t["tmp"]
            else:
                lam, ni = lam * ni, ni * 2
            q += 1
            if not (rho < 0 and q < em.MAX_TRIALS):
                break
        if q == em.MAX_TRIALS or rho == 0:
            stop = True
            continue
        n_bad = n_bad + 1 if (ini - cur) * 1e3 < ini else 0
        if n_bad >= 3:
            stop = True
    if k != len(tr):
        bad.append("trials after the driver stops")
    if not stop and len(lin) != n_iterations and len(lin) > 0:
        bad.append("the driver stops early")
    return bad


# A decision of the model is CLEAR when it stands whatever a build within M_REL of the model's chi2 computes: a trial is followed only
# while |cur - tmp| exceeds M_REL of cur, and the stall criterion while its two sides differ by more than M_REL of ini.
CLEAR = M_REL


def clear_prefix(res):
    """-> the number of the model's trials whose decisions are clear, all earlier ones being clear too."""
    n = 0
    for t in res.trials:
        if not t["ok"] or not np.isfinite(t["tmp"]) or abs(t["cur"] - t["tmp"]) <= CLEAR * abs(t["cur"]):
            break
        if "stall_margin" in t and t["stall_margin"] <= CLEAR:
            break
        n += 1
    return n


def check_trajectory(name, run):
    """Trial by trial against the model over the clear prefix: the same linearisation, the same verdict, lambda within the relative
    spread an accepted trial's rho passes on (alpha is clipped to [1/3, 2/3] and sits on a limit wherever rho is not within 0.2 of
    1/2: M_REL else), and the chi2 an accepted trial reaches within M_REL of the chi2 it started from."""
    sc, res = model(name)
    n = min(clear_prefix(res), len(run.trace.trial))
    bad = []
    for k in range(n):
        m, t = res.trials[k], run.trace.trial[k]
        if t["lin"] != m["lin"] or bool(t["accepted"]) != m["accepted"] or bool(t["ok"]) != m["ok"]:
            bad.append("trial %d: lin / ok / accepted" % k)
            break
        if abs(t["lambda"] - m["lam"]) > M_REL * m["lam"]:
            bad.append("trial %d: lambda %r against %r" % (k, float(t["lambda"]), m["lam"]))
        if m["accepted"] and abs(t["tmp"] - m["tmp"]) > M_REL * abs(m["cur"]):
            bad.append("trial %d: tmp %r against %r" % (k, float(t["tmp"]), m["tmp"]))
    return bad, n, len(res.trials)


# ---- layer 4 ---------------------------------------------------------------------------------------------------------------------------------
def check_final(name, run):
    sc, res = model(name)
    bad = []
    d = float(np.abs(run.S - res.S).max())
    if not d <= T_EST:
        bad.append("estimate off by %.3e (T %.3e)" % (d, T_EST))
    # the float poses and points: T, and the float's own half ulp at their magnitude
    Tm = float(np.abs(res.Tcw).max()) if len(res.Tcw) else 1.0
    d = float(np.abs(run.Tcw.astype(np.float64) - res.Tcw.astype(np.float64)).max())
    if not d <= 2 * T_EST * max(1.0, Tm) + 2.0 ** -23 * Tm:
        bad.append("poses off by %.3e" % d)
    if len(res.points):
        Pm = float(np.abs(res.points).max())
        d = float(np.abs(run.points.astype(np.float64) - res.points.astype(np.float64)).max())
        if not d <= T_PTS + 2.0 ** -23 * Pm:
            bad.append("points off by %.3e (T %.3e)" % (d, T_PTS))
    K = len(sc["Scw"])
    first = np.arange(K - 1)
    free = em.free_index(K, sc["fixed"])
    for a, c in zip(free[sc["edge_i"]], free[sc["edge_j"]]):
        if a >= 0 and c >= 0:
            first[max(a, c)] = min(first[max(a, c)], min(a, c))
    if run.envelope_blocks != int((np.arange(K - 1) - first + 1).sum()):
        bad.append("envelope blocks")
    return bad


def check_call(name, run):
    sc, res = model(name)
    bad = replay(run, sc["n_iterations"]) + check_final(name, run)
    tb, n, total = check_trajectory(name, run)
    assert not bad + tb, (name, bad + tb)
    return n, total


if __name__ == "__main__":
    detail = {}
    est, pts, unclear = measure_spread(list(em.SCENES), detail=detail)
    for k, v in detail.items():
        print("%-16s estimate spread %.3e  points spread %.3e  chi2 spread %.3e%s" % (k, v[0], v[1], v[2], "  UNCLEAR" if k in unclear else ""))
    print("estimate spread %.3e, points spread %.3e" % (est, pts))
    for name in em.SCENES:
        res = model(name)[1]
        print("%-16s trials %d, clear prefix %d, solves ok where accepted: %s" % (name, len(res.trials), clear_prefix(res), all(t["ok"] for t in res.trials if t["accepted"])))
