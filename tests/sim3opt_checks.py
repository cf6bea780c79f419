"""The checks that hold an implementation of the Sim3 optimisation to tests/sim3opt_model.py, layer by layer, and the driver of the
host build (tests/emu/sim3opt_emu.cpp).  tests/test_sim3opt_emu.py runs them on the host build and on its seven seeded mutations,
tests/test_gpu_sim3opt.py on the device (the layers the trace tap shows).

Every bound is derived beside its check from the precision of the formats (u = 2^-53) and an operation count; T and M alone are
measured, and they are measured on the MODEL (measure_spread), never on the code under test.

    layer 0  exp against math.exp at the bound stated beside sim3opt::exp_
    layer 1  the update Sim3(dx) * S in its four branches, and the 24 words of map() / inverse()
    layer 2  one linearisation: H, b, chi2 under the numeric Jacobian's column bound
    layer 3  the Levenberg driver: (a) one trial on the model's own H, b, lambda, estimate and currentChi, for every trial of the model
             (host build only: the device has no such entry); (b) the driver's rules replayed exactly on the trace's own records;
             (c) the trajectory against the model's, trial by trial, over the prefix on which the model's margins exceed what
             layers 1-2 allow
    layer 4  the call: counts, more_iterations, the mask outside the margin M, the estimate within T, the early return's estimate"""
import ctypes
import math
import os

import numpy as np

import host_build
import sim3opt_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
MUTATIONS = {"FORWARD21": 1, "ONESIDED": 2, "ALWAYS10": 3, "READMIT": 4, "INFO2": 5, "EXP": 6, "WRITEEARLY": 7, "SCALE": 8, "NIONCE": 9}

# ---- T and M -------------------------------------------------------------------------------------------------------------------------
# measure_spread(list(sm.SCENES), orders=8, ext=("mp",)) on the model (`python tests/sim3opt_checks.py`, 90 s: too slow for the suite,
# which repeats it on the three scenes that set the maxima, test_recorded_spreads_are_what_the_model_shows): the largest difference of the
# final (q, t, s) and of the chi2 the two checks judge, between the model as written and (a) the model over 8 random orders of the
# pairs, (b) the model with every projection error evaluated in mpmath at 50 digits and rounded to double where g2o stores a double.
# (b) removes the rounding noise of the evaluation that the 1e-9 difference amplifies by 5e8; under (b) alone the spreads are 7.14e-08
# and 4.09e-05, under numpy.longdouble in its place 7.15e-08 and 4.1e-05: the maxima below come from (a).
# The chi2 spread is taken relative to max(chi2, th2): far above the threshold a chi2 moves by more and decides nothing.
# Times four: the code under test differs from the model in more ways at once than either variant does (the tree AND other roundings
# of map() AND its own sin / cos / exp), and a spread over nine samples underestimates the range.
EST_SPREAD = 1.2e-7        # measured 1.133e-07 (plain_65)
CHI2_REL_SPREAD = 4.9e-5   # measured 4.821e-05 of max(chi2, th2) (all_bad_12)
T_EST = 4 * EST_SPREAD
M_REL = 4 * CHI2_REL_SPREAD


def model(name, _cache={}):
    if name not in _cache:
        sc = sm.make(name)
        _cache[name] = (sc, sm.optimize(sc))
    return _cache[name]


def rel_margin(res, th2=sm.TH2):
    """min over judged edges of |chi2 - th2| / max(chi2, th2)."""
    th, m = float(np.float32(th2)), float("inf")
    for a, b, live in res.checks:
        c = np.concatenate([a[live], b[live]])
        c = c[np.isfinite(c)]
        if len(c):
            m = min(m, float((np.abs(c - th) / np.maximum(c, th)).min()))
    return m


def thin(name):
    return rel_margin(model(name)[1]) < M_REL


def measure_spread(names, orders=8, ext=("mp",), seed=7, detail=None):
    """-> (estimate spread, relative chi2 spread, mask changes) of the model over `orders` random orders and the evaluations named in
    `ext` ("mp": mpmath at 50 digits, the measurement of record; True: numpy.longdouble, the suite's quick stand-in).  detail: a dict
    that receives the two spreads per scene."""
    est = chi = 0.0
    flips = 0
    for name in names:
        sc, base = model(name)
        if sm.not_finite(base) or not base.lin:
            continue
        n, g = base.n_correspondences, np.random.default_rng(seed)
        th = float(np.float32(sc["th2"]))
        variants = [sm.optimize(sc, order=g.permutation(n)) for _ in range(orders)] + [sm.optimize(sc, ext=e) for e in ext]
        e0, c0 = est, chi
        est = chi = 0.0
        for v in variants:
            est = max(est, float(np.abs(v.S.vec() - base.S.vec()).max()))
            flips += int((v.removed != base.removed).sum())
            for (a, b, live), (a2, b2, live2) in zip(base.checks, v.checks):
                if (live != live2).any():
                    continue
                c, c2 = np.concatenate([a[live], b[live]]), np.concatenate([a2[live], b2[live]])
                ok = np.isfinite(c) & np.isfinite(c2)
                if ok.any():
                    chi = max(chi, float((np.abs(c - c2)[ok] / np.maximum(c[ok], th)).max()))
        if detail is not None:
            detail[name] = (est, chi)
        est, chi = max(est, e0), max(chi, c0)
    return est, chi, flips


# ---- the host build ------------------------------------------------------------------------------------------------------------------
class Run:
    def __init__(self, est, estf, counts, removed, trace):
        self.q, self.t, self.s = est[:4].copy(), est[4:7].copy(), float(est[7])
        self.R12, self.t12, self.scale = estf[:9].reshape(3, 3).copy(), estf[9:12].copy(), np.float32(estf[12])
        self.n_inliers, self.n_correspondences, self.n_bad, self.more_iterations = [int(v) for v in counts]
        self.removed, self.trace = removed, trace


class Emu:
    """tests/emu/sim3opt_emu.cpp, built on first use with the library's contract: no FMA contraction.  `mutation`: a key of MUTATIONS,
    compiled into a library of its own."""
    _libs = {}

    def __init__(self, uvo, mutation=None):
        assert mutation is None or mutation in MUTATIONS
        self.uvo = uvo
        if mutation not in Emu._libs:
            variant = (["-DSIM3OPT_MUT=%d" % MUTATIONS[mutation]], "_" + mutation.lower()) if mutation else ()
            L = ctypes.CDLL(host_build.build("sim3opt_emu", *variant))
            vp, ci, cd, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_float
            L.emu_sim3opt_exp.argtypes, L.emu_sim3opt_exp.restype = [cd], cd
            L.emu_sim3opt_from_floats.argtypes = [vp, vp, cf, vp]
            L.emu_sim3opt_oplus.argtypes = [vp, vp, vp]
            L.emu_sim3opt_mats.argtypes = [vp, vp]
            L.emu_sim3opt_pack_pair.argtypes = [vp] * 8 + [cf, cf, vp]
            L.emu_sim3opt_linearise.argtypes = [vp, vp, vp, vp, vp, ci, cf, vp, vp]
            L.emu_sim3opt_solve.argtypes = [vp, cd, vp, vp]
            L.emu_sim3opt_trial.argtypes = [vp, cd, vp, vp, cd, vp, vp, vp, vp, ci, cf, vp, vp, vp]
            L.emu_sim3opt_optimize.argtypes = [vp, ci, vp, vp, vp, vp, cf, cf, vp, vp, vp, vp, vp]
            assert L.emu_sim3opt_mutation() == (MUTATIONS[mutation] if mutation else 0)
            Emu._libs[mutation] = L
        self.L = Emu._libs[mutation]

    def exp(self, x):
        return float(self.L.emu_sim3opt_exp(float(x)))

    def from_floats(self, R12, t12, s12):
        out = np.zeros(8)
        R, t = np.ascontiguousarray(R12, np.float32).reshape(9), np.ascontiguousarray(t12, np.float32)
        self.L.emu_sim3opt_from_floats(R.ctypes.data, t.ctypes.data, float(np.float32(s12)), out.ctypes.data)
        return out

    def oplus(self, dx, sim):
        dx, sim, out = np.ascontiguousarray(dx, np.float64), np.ascontiguousarray(sim, np.float64), np.zeros(8)
        self.L.emu_sim3opt_oplus(dx.ctypes.data, sim.ctypes.data, out.ctypes.data)
        return out

    def mats(self, sim):
        sim, out = np.ascontiguousarray(sim, np.float64), np.zeros(24)
        self.L.emu_sim3opt_mats(sim.ctypes.data, out.ctypes.data)
        return out

    def pairs(self, sc):
        """The library's gather of a scene: [n, 12] float32."""
        n = len(sc["x1w"])
        P = np.zeros((n, 12), np.float32)
        R1, t1, R2, t2 = [np.ascontiguousarray(a, np.float32).reshape(-1) for a in (sc["kf1"][0], sc["kf1"][1], sc["kf2"][0], sc["kf2"][1])]
        for i in range(n):
            self.L.emu_sim3opt_pack_pair(R1.ctypes.data, t1.ctypes.data, R2.ctypes.data, t2.ctypes.data, sc["x1w"][i].ctypes.data, sc["x2w"][i].ctypes.data,
                                         sc["obs1"][i].ctypes.data, sc["obs2"][i].ctypes.data, float(sc["info1"][i]), float(sc["info2"][i]), P[i].ctypes.data)
        return P

    @staticmethod
    def _k(K):
        return np.ascontiguousarray([np.float32(v) for v in K], np.float32)

    def linearise(self, sim, sc, P, state):
        n = len(P)
        sums, chi2 = np.zeros(36), np.zeros((max(n, 1), 2))
        K1, K2, sim = self._k(sc["kf1"][2]), self._k(sc["kf2"][2]), np.ascontiguousarray(sim, np.float64)
        P, state = np.ascontiguousarray(P, np.float32), np.ascontiguousarray(state, np.uint8)
        self.L.emu_sim3opt_linearise(sim.ctypes.data, K1.ctypes.data, K2.ctypes.data, P.ctypes.data, state.ctypes.data, n, float(np.float32(sc["th2"])),
                                     sums.ctypes.data, chi2.ctypes.data)
        return sums, chi2[:n]

    def solve(self, H28, lam, b):
        x = np.zeros(7)
        H28, b = np.ascontiguousarray(H28, np.float64), np.ascontiguousarray(b, np.float64)
        return bool(self.L.emu_sim3opt_solve(H28.ctypes.data, float(lam), b.ctypes.data, x.ctypes.data)), x

    def trial(self, H, lam, b, sim, cur, sc, P, state, dx_prev):
        """-> ok, dx, the tried estimate (8 words), tmp, scale, rho."""
        n = len(P)
        H28, b, sim = np.ascontiguousarray(np.asarray(H)[np.triu_indices(7)], np.float64), np.ascontiguousarray(b, np.float64), np.ascontiguousarray(sim, np.float64)
        K1, K2, P, state = self._k(sc["kf1"][2]), self._k(sc["kf2"][2]), np.ascontiguousarray(P, np.float32), np.ascontiguousarray(state, np.uint8)
        dx, out_sim, out = np.array(dx_prev, np.float64), np.zeros(8), np.zeros(3)
        ok = self.L.emu_sim3opt_trial(H28.ctypes.data, float(lam), b.ctypes.data, sim.ctypes.data, float(cur), K1.ctypes.data, K2.ctypes.data, P.ctypes.data,
                                      state.ctypes.data, n, float(np.float32(sc["th2"])), dx.ctypes.data, out_sim.ctypes.data, out.ctypes.data)
        return bool(ok), dx, out_sim, float(out[0]), float(out[1]), float(out[2])

    def optimize_pairs(self, P, K1, K2, R12, t12, s12, th2):
        n = len(P)
        P = np.ascontiguousarray(P, np.float32)
        K1, K2 = self._k(K1), self._k(K2)
        R, t = np.ascontiguousarray(R12, np.float32).reshape(9), np.ascontiguousarray(t12, np.float32)
        est, estf, counts, mask = np.zeros(8), np.zeros(13, np.float32), np.zeros(4, np.int32), np.zeros(max(n, 1), np.uint8)
        c = self.uvo.Sim3OptTraceC()
        self.L.emu_sim3opt_optimize(P.ctypes.data, n, K1.ctypes.data, K2.ctypes.data, R.ctypes.data, t.ctypes.data, float(np.float32(s12)), float(np.float32(th2)),
                                    est.ctypes.data, estf.ctypes.data, counts.ctypes.data, mask.ctypes.data, ctypes.addressof(c))
        return Run(est, estf, counts, mask[:n].copy(), self.uvo.Sim3OptTrace(c))

    def optimize(self, sc):
        return self.optimize_pairs(self.pairs(sc), sc["kf1"][2], sc["kf2"][2], sc["R12"], sc["t12"], sc["s12"], sc["th2"])


def of_result(r, trace):
    """A uvo.Sim3OptResult and its trace as a Run."""
    est = np.concatenate([r.q, r.t, [r.s]])
    estf = np.concatenate([r.R12.reshape(9), r.t12, [r.scale]]).astype(np.float32)
    return Run(est, estf, (r.n_inliers, r.n_correspondences, r.n_bad, r.more_iterations), r.removed, trace)


def same_bits(a, b):
    """Equal bit for bit, non-finite values by class (NaN payloads and signs are not part of the contract)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return False
    if a.dtype.kind != "f":
        return bool((a == b).all())
    na, nb = np.isnan(a), np.isnan(b)
    return bool((na == nb).all() and (a[~na] == b[~nb]).all())


def same_run(x, y):
    """-> the list of fields in which two runs differ."""
    bad = [k for k in ("q", "t", "R12", "t12", "removed") if not same_bits(getattr(x, k), getattr(y, k))]
    bad += [k for k in ("s", "scale") if not same_bits(np.float64(getattr(x, k)), np.float64(getattr(y, k)))]
    bad += [k for k in ("n_inliers", "n_correspondences", "n_bad", "more_iterations") if getattr(x, k) != getattr(y, k)]
    tx, ty = x.trace, y.trace
    if tx is not None and ty is not None:
        bad += [k for k in ("q", "t") if not same_bits(getattr(tx, k), getattr(ty, k))]
        if not same_bits(np.float64(tx.s), np.float64(ty.s)):
            bad.append("trace.s")
        for rec in ("lin", "trial"):
            a, b = getattr(tx, rec), getattr(ty, rec)
            if len(a) != len(b):
                bad.append("trace.%s count" % rec)
            else:
                bad += ["trace.%s.%s" % (rec, f) for f in a.dtype.names if not same_bits(a[f], b[f])]
    return bad


# ---- layer 0: exp --------------------------------------------------------------------------------------------------------------------
EXP_LIMIT = 40.0
EXP_BOUND = 2.0 ** -51     # relative; derived beside sim3opt::exp_


def exp_grid():
    g = [0.0, 1e-9, -1e-9, 1e-5, -1e-5, 1e-5 * (1 - 1e-6), 1e-5 * (1 + 1e-6), -1e-5 * (1 - 1e-6), -1e-5 * (1 + 1e-6), EXP_LIMIT, -EXP_LIMIT,
         math.log(2) / 2, -math.log(2) / 2, math.nextafter(math.log(2) / 2, 1), 0.3466, -0.3466]
    g += list(np.linspace(-EXP_LIMIT, EXP_LIMIT, 4001)) + list(np.linspace(-1, 1, 2001)) + list(np.random.default_rng(1).normal(size=2000) * 0.05)
    return g


def check_exp(f):
    """-> worst error / bound.  math.exp is itself within an ulp; the bound has that room (see the derivation: 1.3 * 2^-52)."""
    worst = 0.0
    for x in exp_grid():
        got, ref = f(x), math.exp(x)
        err = abs(got - ref) / ref
        assert err <= EXP_BOUND, (x, got, ref, err / EXP_BOUND)
        worst = max(worst, err / EXP_BOUND)
    for x in (math.nextafter(EXP_LIMIT, 100), -math.nextafter(EXP_LIMIT, 100), 1e3, float("inf"), float("-inf"), float("nan")):
        assert math.isnan(f(x)), x
    return worst


# ---- layer 1: the update and the maps ---------------------------------------------------------------------------------------------
UPDATE_CASES = {
    # branch: dx.  0: |sigma| < eps, theta < eps; 1: theta large; 2: sigma large; 3: both large
    0: [0.5e-5, -0.3e-5, 0.2e-5, 0.3, -0.2, 0.1, 0.9e-5],
    1: [0.05, -0.08, 0.03, 0.3, -0.2, 0.1, -0.9e-5],
    2: [0.5e-5, -0.3e-5, 0.2e-5, 0.3, -0.2, 0.1, 0.05],
    3: [0.05, -0.08, 0.03, 0.3, -0.2, 0.1, -0.05],
}


def update_bound(dx, S):
    """Sim3(dx) * S against the model.  Every output is a sum of at most 8 products of quantities below m = max(1, |t|, s, |upsilon|)
    after at most 16 roundings, sin / cos / exp within 2^-51 of libm's: 64 u m^2.  The coefficients A, B, C of W cancel: a numerator
    known to 2^-50 s absolutely is divided by theta^k or sigma^k, and the quotient multiplies Omega^j (|Omega^j| <= theta^j) and upsilon:
    branch 1: A, B give 2^-49 / theta; branch 2: C, A, B give 2^-50 s (1 / |sigma| + theta / sigma^2 + theta^2 / |sigma|^3);
    branch 3: C gives 2^-50 s / |sigma|, A and B 2^-48 s / sqrt(theta^2 + sigma^2) -- each times |upsilon|_1, on t alone."""
    dx = np.asarray(dx, np.float64)
    theta, sigma, ups = float(np.linalg.norm(dx[:3])), abs(float(dx[6])), float(np.abs(dx[3:6]).sum())
    s = math.exp(dx[6])
    m = max(1.0, float(np.abs(S.t).max()), S.s, float(np.abs(dx[3:6]).max()))
    base = 64 * U * m * m
    big_t, big_s = theta >= 1e-5, sigma >= 1e-5
    c = 0.0
    if big_t and not big_s:
        c = 2.0 ** -49 / theta
    elif big_s and not big_t:
        c = 2.0 ** -50 * s * (1 / sigma + theta / sigma ** 2 + theta ** 2 / sigma ** 3)
    elif big_s and big_t:
        c = 2.0 ** -50 * s / sigma + 2.0 ** -48 * s / math.sqrt(theta * theta + sigma * sigma)
    return base, base + c * ups * max(1.0, S.s)


def check_update(oplus_f, mats_f):
    """oplus_f(dx, sim8) -> sim8, mats_f(sim8) -> 24 words.  -> worst difference / bound."""
    S = sm.Sim(sm.quat_of(sm.rot_of_vec(np.array([0.2, -0.1, 0.3]))), [0.4, -0.3, 0.2], 1.07)
    worst = 0.0
    for br, dx in UPDATE_CASES.items():
        want, took = sm.sim_exp(dx)
        assert took == br, (br, took)
        want = want * S
        got = oplus_f(dx, S.vec())
        bq, bt = update_bound(dx, S)
        d = np.abs(got - want.vec())
        assert (d[:4] <= bq).all() and (d[4:7] <= bt).all() and d[7] <= bq, (br, d, bq, bt)
        worst = max(worst, float((d / np.array([bq] * 4 + [bt] * 3 + [bq])).max()))
        # map() and inverse().map() as matrices: 3 products and 3 sums on top of the rotation matrix (4 roundings an entry) -> 16 u m^2
        M = mats_f(got)
        G = sm.Sim(got[:4], got[4:7], got[7])
        X = np.array([[0.7, -1.1, 5.0], [-2.0, 0.4, 3.5]])
        for off, T in ((0, G), (12, G.inverse())):
            Y = X @ M[off:off + 9].reshape(3, 3).T + M[off + 9:off + 12]
            assert np.abs(Y - T.map(X)).max() <= 64 * U * 8 * 8, (br, off)
    return worst


# ---- layer 2: one linearisation --------------------------------------------------------------------------------------------------------
def edge_error_bound(S, P, K1, K2):
    """de [n_pairs, 2 edges, 2 rows]: the rounding error of one projection error in either implementation.
    map(): each coordinate is s (r x) + t: at most 12 roundings on terms bounded by s |X|_1 + |t|_inf (the inverse carries the rounded
    -t / s through a rotation: twice that) -> dm = 16 u (s |X|_1 + |t|_inf), 32 u for the inverse.  x / z: (dm + |x / z| dm) / |z| and
    one rounding; times f, plus the principal point, minus from the observation: one rounding each on |f x / z|, |f x / z + pp|, |e|."""
    out = np.zeros((len(P), 2, 2))
    P = P.astype(np.float64)
    Si = S.inverse()
    for e, (T, X, K, obs, c) in enumerate(((S, P[:, 3:6], K1, P[:, 6:8], 16), (Si, P[:, 0:3], K2, P[:, 8:10], 32))):
        with np.errstate(all="ignore"):
            Y = T.map(X)
            dm = c * U * (abs(T.s) * np.abs(X).sum(1) + np.abs(T.t).max())
            for r in range(2):
                f, pp = float(np.float32(K[r])), float(np.float32(K[2 + r]))
                ratio = np.abs(Y[:, r] / Y[:, 2])
                out[:, e, r] = f * ((dm + ratio * dm) / np.abs(Y[:, 2]) + U * ratio) + U * (2 * f * ratio + 2 * abs(pp) + np.abs(obs[:, r]) + 1)
    return out


def linearisation_bounds(name, li=0):
    """Bounds on |H - H_model|, |b - b_model|, |chi2 - chi2_model| of linearisation `li` of the model (the first by default) AT THE
    MODEL'S ESTIMATE, from the model's own terms.
    The numeric Jacobian: a column entry is (e(+) - e(-)) * 5e8, so an error bound de on each error is (de(+) + de(-)) * 5e8 = de * 1e9
    on the entry, in the model and in the code under test alike: dJ = 2e9 de between them.  With J, w, rho1, e of the model:
        |dH_ij| <= sum_edges sum_rows w rho1 (|J_i| dJ + |J_j| dJ + dJ^2) + drho |H terms| + (N + 8) u |H terms|
        |db_i|  <= sum w rho1 (|e| dJ + |J_i| de + dJ de)                 + drho |b terms| + (N + 8) u |b terms|
        |dchi2| <= sum 2 w |e| de rho1 + w de^2                                             + (N + 8) u |chi2 terms|
    drho: rho1 = delta / sqrt(chi2) on the Huber branch moves by half the relative error of chi2, 2 de / |e|: de / |e|_2 there, 0
    elsewhere (an edge AT the kink would flip branch: the scenes keep clear of it, which the margin test covers).
    N: the number of edges summed; the tree and the serial sum both stay below N u times the sum of absolute terms."""
    sc, res = model(name)
    l0 = res.lin[li]
    L, S = l0["L"], l0["S"]
    P = sm.pairs_of(sc)
    idx = np.flatnonzero(l0["active"])
    de = edge_error_bound(S, P, sc["kf1"][2], sc["kf2"][2])[idx].reshape(-1, 2)   # per edge in graph order, per row
    dJ = 2e9 * de
    J, e, w, rho1 = np.abs(L["J"]), np.abs(L["e"]), L["w"], L["rho1"]
    N = len(w)
    with np.errstate(all="ignore"):
        enorm = np.sqrt((e * e).sum(1))
        drho = np.where(rho1 < 1, de.max(1) / enorm, 0.0) + 4 * U
        wr = (w * rho1)[:, None, None, None]
        Hb = (wr * (J[:, :, :, None] * dJ[:, :, None, None] + J[:, :, None, :] * dJ[:, :, None, None] + (dJ * dJ)[:, :, None, None])).sum((0, 1))
        Hterms = (wr * J[:, :, :, None] * J[:, :, None, :]).sum(1)
        Hb = Hb + (drho[:, None, None] * Hterms).sum(0) + (N + 8) * U * L["abs_H"]
        wr2 = (w * rho1)[:, None]
        bterm = (wr2[:, :, None] * e[:, :, None] * J).sum(1)
        bb = (wr2[:, :, None] * (e[:, :, None] * dJ[:, :, None] + J * de[:, :, None] + (dJ * de)[:, :, None])).sum((0, 1))
        bb = bb + (drho[:, None] * bterm).sum(0) + (N + 8) * U * L["abs_b"]
        cb = float((rho1[:, None] * w[:, None] * (2 * e * de + de * de)).sum()) + (N + 8) * U * L["abs_chi2"]
    return Hb, bb, cb


def unpack_sums(sums):
    H = np.zeros((7, 7))
    H[np.triu_indices(7)] = sums[:28]
    H = H + np.triu(H, 1).T
    return H, sums[28:35].copy(), float(sums[35])


def check_linearisation(name, sums):
    """sums: H[28] b[7] chi2 of the implementation at the start estimate over all pairs -> worst difference / bound."""
    sc, res = model(name)
    l0 = res.lin[0]
    H, b, chi = unpack_sums(np.asarray(sums, np.float64))
    if not np.isfinite(l0["chi2"]):
        assert not np.isfinite(chi) and not np.isfinite(H).all(), name
        return 0.0
    Hb, bb, cb = linearisation_bounds(name)
    dH, db, dc = np.abs(H - l0["H"]), np.abs(b - l0["b"]), abs(chi - l0["chi2"])
    assert (dH <= Hb).all(), (name, "H", float((dH / Hb).max()))
    assert (db <= bb).all(), (name, "b", float((db / bb).max()))
    assert dc <= cb, (name, "chi2", dc / cb)
    return max(float((dH / Hb).max()), float((db / bb).max()), dc / cb)


# ---- layer 3: the Levenberg trajectory ------------------------------------------------------------------------------------------------
def chi2_bound(name, S, active):
    """Bound on the difference of the robust chi2 over the active pairs at S between the model and the code, both AT S: per edge
    rho1 w (2 |e| de + de^2) (the Huber branch's slope is rho1 <= 1), plus (N + 8) u times the sum of the absolute terms."""
    sc, _ = model(name)
    P = sm.pairs_of(sc)
    idx = np.flatnonzero(active)
    de = edge_error_bound(S, P, sc["kf1"][2], sc["kf2"][2])[idx].reshape(-1, 2)
    e12, e21 = sm.edge_errors(S, P, sc["kf1"][2], sc["kf2"][2])
    e = np.abs(np.stack([e12[idx], e21[idx]], 1).reshape(-1, 2))
    w = np.stack([P[idx, 10], P[idx, 11]], 1).reshape(-1).astype(np.float64)
    with np.errstate(all="ignore"):
        c = sm.chi2_of(e, w)
        rho0, rho1 = sm.huber(c, sm.delta_of(sc["th2"]))
        return float((rho1[:, None] * w[:, None] * (2 * e * de + de * de)).sum()) + (len(w) + 8) * U * float(np.abs(rho0).sum())


def trajectory_bounds(name, _cache={}):
    """Walks the model's trials and derives, to first order in the errors, how far the code's figures may lie from the model's at each:
    -> (k, lam_rtol [k], last): the number of leading trials whose decision the bounds cannot move, the relative tolerance on lambda at
    each, and the last linearisation whose (round, iteration) is thereby fixed.
    At a linearisation the code's H, b, chi2 differ from the model's by layer 2's bounds (Hb, bb, cb) plus what a drift dS of the
    estimate (tangent units, accumulated below) moves them: b by |H| dS (db/dS = -H), H by 8 |H| dS (each entry a product of two
    Jacobian entries, each moving relatively by at most 4 dS: the projection's second derivative is below 4 / z times its first on
    scenes with z >= 1), chi2 by 2 |b|_1 dS.  lambda = 1e-5 max |H_jj| carries H's relative bound.  A trial's step solves A dx = b,
    A = H + lambda I: ddx = |A^-1| (db + dH |dx| + dlambda |dx|).  The tried chi2 moves by its own evaluation bound at the tried
    estimate plus its gradient, bounded by 2 (|b| + |H| |dx|), times (ddx + dS).  The decision rho > 0 is the sign of cur - tmp:
    it stands while the model's margin |cur - tmp| exceeds the two bounds together.  rho = (cur - tmp) / scale moves by
    (that + |rho| dscale) / |scale|; an accepted trial multiplies lambda by max(1/3, min(2/3, 1 - (2 rho - 1)^3)), whose derivative in
    rho is at most 6: between the clamps the relative tolerance grows by 6 drho / alpha; a rejected trial multiplies by ni exactly.
    An accepted step adds max(ddx) to dS.  The iteration's end is decided by (ini - cur) * 1e3 < ini: when that difference is within
    1001 d(ini) + 1000 d(cur) the prefix ends there, whatever follows."""
    if name in _cache:
        return _cache[name]
    sc, res = model(name)
    k, tol, dS, lam_r, last, cur_lin = 0, [], 0.0, 0.0, -1, -1
    for i, tr in enumerate(res.trials):
        L = res.lin[tr["lin"]]
        H, b, lam, dx = np.abs(L["H"]), np.abs(L["b"]), tr["lam"], np.abs(tr["dx"])
        if tr["lin"] != cur_lin:
            cur_lin = tr["lin"]
            Hb, bb, cb = linearisation_bounds(name, cur_lin)
            Hb, bb, cb = Hb + 8 * dS * H, bb + H @ np.full(7, dS), cb + 2 * float(b.sum()) * dS
            if L["iteration"] == 0:
                mx = float(np.abs(np.diag(L["H"])).max())
                if not mx > 0:
                    break
                lam_r = float(np.diag(Hb).max()) / mx + 4 * U
        if not (tr["ok"] and math.isfinite(tr["margin"])):
            break
        Ainv = np.abs(np.linalg.inv(L["H"] + lam * np.eye(7)))
        ddx = Ainv @ (bb + Hb @ dx + lam_r * lam * dx)
        dtmp = chi2_bound(name, tr["S"], L["active"]) + 2 * float((b + H @ dx) @ (ddx + dS))
        if not tr["margin"] > cb + dtmp:
            break
        tol.append(lam_r)
        k, last = k + 1, tr["lin"]
        dscale = float(dx @ (lam * ddx + bb + lam_r * lam * dx) + ddx @ np.abs(lam * tr["dx"] + L["b"]))
        drho = (cb + dtmp + abs(tr["rho"]) * dscale) / abs(tr["scale"])
        if tr["accepted"]:
            alpha = 1.0 - (2 * tr["rho"] - 1) ** 3
            if 1.0 / 3.0 < alpha < 2.0 / 3.0:
                lam_r += 6 * drho / alpha
            elif min(abs(alpha - 1.0 / 3.0), abs(alpha - 2.0 / 3.0)) <= 6 * drho:
                break                                   # the clamp itself is within the bound: lambda may take either form
            dS += float(ddx.max())
        ends = i + 1 == len(res.trials) or res.trials[i + 1]["lin"] != tr["lin"]
        if ends:
            ini, cur = L["chi2"], tr["tmp"] if tr["accepted"] else tr["cur"]
            if abs((ini - cur) * 1e3 - ini) <= 1001 * cb + 1000 * dtmp:
                break
    _cache[name] = (k, tol, last)
    return _cache[name]


def check_trials(emu, name, limit=None):
    """One trial of the code on the MODEL's own H, b, lambda, estimate and currentChi, for every trial the model made (or the first
    `limit`): nothing of the numeric Jacobian's noise enters, so the bounds are rounding bounds.  -> worst difference / bound.
    dx: both solvers are backward stable, the computed x solves (A + dA) x = b with |dA| <= g |A|, g <= 3 n u x growth; n = 7, growth 1
    for the LDL^T of a positive definite matrix and at most 2^(n - 1) = 64 for partial pivoting: |ddx| <= (21 + 1344) u cond |dx|.
    The tried estimate: layer 1's bound at (dx, S), plus ddx carried through the product (each output moves by at most
    m = max(1, |t|, s) times it, twice for t: omega and upsilon both reach it).  scale = dx . (lambda dx + b) + 1e-3: 16 roundings on
    the sum of absolute terms plus |lambda dx + b| . ddx + |dx| . lambda ddx.  tmp: its evaluation bound at the tried estimate plus its
    gradient, bounded by 2 (|b| + |H| |dx|), times the estimate's bound (in tangent units: the bound on S divided by nothing -- the
    tangent moves S by at most m per unit).  rho: (dtmp + |rho| dscale) / |scale|."""
    sc, res = model(name)
    P = sm.pairs_of(sc)
    worst, prev = 0.0, {}
    for i, tr in enumerate(res.trials[:limit]):
        L = res.lin[tr["lin"]]
        dx_prev = res.trials[i - 1]["dx"] if i and res.lin[res.trials[i - 1]["lin"]]["round"] == L["round"] else np.zeros(7)
        state = (~L["active"]).astype(np.uint8)
        ok, dx, S1, tmp, scale, rho = emu.trial(L["H"], tr["lam"], L["b"], tr["S0"].vec(), tr["cur"], sc, P, state, dx_prev)
        assert ok == tr["ok"], (name, i, "ok")
        if not ok:
            assert tmp == sm.DBL_MAX and np.array_equal(dx, dx_prev), (name, i)
            continue
        A = L["H"] + tr["lam"] * np.eye(7)
        adx = np.abs(tr["dx"])
        ddx = 1365 * U * float(np.linalg.cond(A)) * float(adx.max())
        assert np.abs(dx - tr["dx"]).max() <= ddx, (name, i, "dx", float(np.abs(dx - tr["dx"]).max()), ddx)
        S0 = tr["S0"]
        m = max(1.0, float(np.abs(S0.t).max()), S0.s)
        bq, bt = update_bound(tr["dx"], S0)
        bq, bt = bq + 2 * m * ddx, bt + 4 * m * ddx
        d = np.abs(S1 - tr["S"].vec())
        assert (d[:4] <= bq).all() and (d[4:7] <= bt).all() and d[7] <= bq, (name, i, "estimate", d, bq, bt)
        terms = float(adx @ (tr["lam"] * adx + np.abs(L["b"]))) + 1e-3
        dscale = 16 * U * terms + float(np.abs(tr["lam"] * tr["dx"] + L["b"]).sum()) * ddx + float(adx.sum()) * tr["lam"] * ddx
        assert abs(scale - tr["scale"]) <= dscale, (name, i, "scale", scale, tr["scale"], dscale)
        g = float((np.abs(L["b"]) + np.abs(L["H"]) @ adx).sum())
        dtmp = chi2_bound(name, tr["S"], L["active"]) + 2 * g * (bt + ddx)
        assert abs(tmp - tr["tmp"]) <= dtmp, (name, i, "tmp", tmp, tr["tmp"], dtmp)
        drho = (dtmp + abs(tr["rho"]) * dscale) / abs(tr["scale"]) + 4 * U * abs(tr["rho"])
        assert abs(rho - tr["rho"]) <= drho, (name, i, "rho", rho, tr["rho"], drho)
        worst = max(worst, float(np.abs(dx - tr["dx"]).max()) / ddx, abs(scale - tr["scale"]) / dscale, abs(tmp - tr["tmp"]) / dtmp)
    return worst


def check_replay(name, run):
    """The driver's rules replayed EXACTLY on the trace's own records -- no tolerance, no model: what the trace says happened must be
    what optimization_algorithm_levenberg.cpp does with the figures the trace shows.  Per linearisation: lambda of its first trial is
    1e-5 max |H_jj| at iteration 0 of a round and the carried value otherwise, currentChi is the linearisation's chi2; per trial:
    a failed solve has tmp = DBL_MAX; rho = (cur - tmp) / scale; accepted exactly when rho > 0 and tmp is finite; then
    lambda *= max(1/3, min(2/3, 1 - (2 rho - 1)^3)) and ni = 2, else lambda *= ni and ni *= 2; another trial follows exactly when
    rho < 0 and fewer than 10 were made; the iteration Terminates on 10 trials or rho == 0; the stall count moves by
    (ini - cur) * 1e3 < ini and ends the round at 3; a round has 5 iterations, the second `more_iterations`; nothing follows the
    second round.  The departure pow(x, 3) = x * x * x is replayed as the library states it."""
    tr, li = run.trace.trial, run.trace.lin
    f = np.float64
    i, lam, ni, stalled, cur = 0, f(0), f(2), 0, f(0)
    with np.errstate(all="ignore"):
        for j in range(len(li)):
            rnd, it = int(li["round"][j]), int(li["iteration"][j])
            if it == 0:
                mx = f(0)
                for v in np.diag(unpack_sums(np.concatenate([li["H"][j], li["b"][j], [li["chi2"][j]]]))[0]):
                    mx = mx if abs(v) < mx else abs(v)
                lam, ni, stalled = f(1e-5) * mx, f(2), 0
            ini = cur = f(li["chi2"][j])
            q, rho = 0, f(0)
            while True:
                assert i < len(tr) and int(tr["lin"][i]) == j, (name, j, i, "a trial is missing")
                assert same_bits(tr["lambda"][i], lam) and same_bits(tr["cur"][i], cur), (name, i, "lambda / cur", tr["lambda"][i], lam)
                tmp, scale = f(tr["tmp"][i]), f(tr["scale"][i])
                assert tr["ok"][i] or tmp == sm.DBL_MAX, (name, i)
                rho = (cur - tmp) / scale
                accept = bool(rho > 0 and np.isfinite(tmp))
                assert bool(tr["accepted"][i]) == accept, (name, i, "decision", rho)
                if accept:
                    u = f(2) * rho - f(1)
                    alpha = f(1) - u * u * u
                    alpha = f(2) / f(3) if f(2) / f(3) < alpha else alpha
                    lam, ni, cur = lam * (alpha if f(1) / f(3) < alpha else f(1) / f(3)), f(2), tmp
                else:
                    lam, ni = lam * ni, ni * f(2)
                q, i = q + 1, i + 1
                if not (rho < 0 and q < 10):
                    break
            ends = q == 10 or rho == 0
            if not ends:
                stalled = stalled + 1 if (ini - cur) * f(1e3) < ini else 0
                ends = stalled >= 3
            its = 5 if rnd == 0 else run.more_iterations
            assert it < its, (name, j, "more iterations than the round has")
            if j + 1 < len(li):
                nxt = (int(li["round"][j + 1]), int(li["iteration"][j + 1]))
                assert nxt == ((rnd + 1, 0) if ends or it + 1 == its else (rnd, it + 1)), (name, j, "what follows", nxt, ends)
                assert nxt[0] <= 1 and (nxt[0] == rnd or run.more_iterations in (5, 10)), (name, j)
            else:
                # the last linearisation: its round ended here, and no second round followed only if there was none to run
                assert ends or it + 1 == its, (name, j, "the round stopped early")
                assert rnd == 1 or run.more_iterations == 0 or run.n_correspondences - run.n_bad == 0, (name, "the second round is missing")
    assert i == len(tr), (name, "trials beyond the last linearisation")
    return len(tr)


def compared_prefix(name):
    return trajectory_bounds(name)[0]


def first_iteration_trials(res):
    return sum(1 for tr in res.trials if tr["lin"] == 0)


def same_class(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return bool((np.isnan(a) == np.isnan(b)).all() and (np.isposinf(a) == np.isposinf(b)).all() and (np.isneginf(a) == np.isneginf(b)).all())


def check_trajectory(name, run):
    """The trace's trials against the model's over the compared prefix: the linearisation each belongs to, whether the solve succeeded,
    the decision, lambda within its derived tolerance; the (round, iteration) of every linearisation the prefix reaches; the trace's
    own consistency (currentChi of a linearisation's first trial is that linearisation's robust chi2; at the start within layer 2).
    A scene whose sums are not finite is compared over its whole length, by class.  -> the number of trials compared."""
    sc, res = model(name)
    tr, li = run.trace.trial, run.trace.lin
    if sm.not_finite(res):
        assert len(tr) == len(res.trials) and len(li) == len(res.lin), (name, len(tr), len(res.trials))
        for i, m in enumerate(res.trials):
            assert (int(tr["lin"][i]), bool(tr["ok"][i]), bool(tr["accepted"][i])) == (m["lin"], m["ok"], m["accepted"]), (name, i)
            assert same_class(tr["lambda"][i], m["lam"]) and same_class(tr["cur"][i], m["cur"]) and same_class(tr["tmp"][i], m["tmp"]), (name, i)
        for j, m in enumerate(res.lin):
            assert (int(li["round"][j]), int(li["iteration"][j])) == (m["round"], m["iteration"]), (name, j)
        return len(tr)
    k, tol, last = trajectory_bounds(name)
    assert len(tr) >= k, (name, len(tr), k)
    for i in range(k):
        m = res.trials[i]
        assert int(tr["lin"][i]) == m["lin"], (name, i, "linearisation index")
        assert bool(tr["ok"][i]) == m["ok"] and bool(tr["accepted"][i]) == m["accepted"], (name, i, "decision", tr[i], m["rho"])
        assert abs(tr["lambda"][i] - m["lam"]) <= tol[i] * m["lam"], (name, i, "lambda", tr["lambda"][i], m["lam"], tol[i])
    if len(tr) and len(res.trials):
        first = [i for i in range(len(tr)) if i == 0 or tr["lin"][i] != tr["lin"][i - 1]]
        assert all(tr["cur"][i] == li["chi2"][tr["lin"][i]] for i in first), (name, "cur")
        assert abs(tr["cur"][0] - res.trials[0]["cur"]) <= linearisation_bounds(name)[2], (name, "cur of the first trial")
    for j in range(last + 1):
        assert (int(li["round"][j]), int(li["iteration"][j])) == (res.lin[j]["round"], res.lin[j]["iteration"]), (name, j)
    return k


# ---- layer 4: the call -------------------------------------------------------------------------------------------------------------------
def check_result(name, run):
    """Counts, more_iterations, mask and estimate of an implementation's call against the model's."""
    sc, res = model(name)
    assert run.n_correspondences == res.n_correspondences, name
    th = float(np.float32(sc["th2"]))
    if sm.not_finite(res):
        # decided by class: the NaN pair stays and counts, every sum is NaN, no step is taken
        assert run.n_inliers == res.n_inliers and run.n_bad == res.n_bad and run.more_iterations == res.more_iterations, name
        assert (run.removed == res.removed).all(), name
        assert np.abs(np.concatenate([run.q, run.t, [run.s]]) - res.S.vec()).max() <= 8 * U * 4, name
        if run.trace is not None:
            assert len(run.trace.lin) == len(res.lin) and np.isnan(run.trace.lin["chi2"]).all() and not run.trace.trial["ok"].any(), name
        return
    if rel_margin(res) >= M_REL:
        assert (run.n_bad, run.more_iterations, run.n_inliers) == (res.n_bad, res.more_iterations, res.n_inliers), (name, run.n_bad, run.more_iterations, run.n_inliers)
        assert (run.removed == res.removed).all(), (name, np.flatnonzero(run.removed != res.removed))
    else:
        # pairs within the margin may fall either way; every other pair's mask is compared
        near = np.zeros(len(res.removed), bool)
        for a, b, live in res.checks:
            for c in (a, b):
                with np.errstate(all="ignore"):
                    near |= live & (np.abs(c - th) < M_REL * np.maximum(c, th))
        assert (run.removed[~near] == res.removed[~near]).all(), name
    est = np.concatenate([run.q, run.t, [run.s]])
    if res.early:
        # the input's round trip: a square root, a division and three products -- and nothing else
        assert run.n_inliers == 0 and run.more_iterations == 0, name
        assert np.abs(est - res.S.vec()).max() <= 8 * U * max(1.0, float(np.abs(res.S.vec()).max())), (name, est, res.S.vec())
    else:
        d = float(np.abs(est - res.S.vec()).max())
        assert d <= T_EST, (name, d, T_EST)
    # the float outputs are the double estimate's roundings
    assert np.abs(run.t12.astype(np.float64) - run.t).max() <= 2.0 ** -24 * max(1.0, float(np.abs(run.t).max())), name
    assert abs(float(run.scale) - run.s) <= 2.0 ** -24 * max(1.0, run.s), name
    assert np.abs(run.R12.astype(np.float64) - sm.rot_of(run.q)).max() <= 2.0 ** -23, name


def check_all(name, run, first_sums=None):
    if first_sums is not None:
        check_linearisation(name, first_sums)
    elif run.trace is not None and len(run.trace.lin):
        l = run.trace.lin[0]
        check_linearisation(name, np.concatenate([l["H"], l["b"], [l["chi2"]]]))
    k = 0
    if run.trace is not None:
        check_replay(name, run)
        k = check_trajectory(name, run)
    check_result(name, run)
    return k


if __name__ == "__main__":
    # the measurement of record for T and M: every scene, 8 orders, mpmath at 50 digits
    detail = {}
    print("estimate spread %.4e, relative chi2 spread %.4e, mask changes %d" % measure_spread(list(sm.SCENES), orders=8, ext=("mp",), detail=detail))
    for k, v in detail.items():
        print("%-20s %.3e %.3e" % (k, v[0], v[1]))
