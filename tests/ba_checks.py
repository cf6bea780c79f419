"""The layer checks of the bundle adjustment: the host build of csrc/ba_core.hpp (tests/emu/ba_emu.cpp) and the device (through the same
functions) against the numpy model tests/ba_model.py.  DESIGN.md section 4 states the contract; the bounds are derived here.

  1. per edge: error, chi2, both Jacobians at the start.
  2. the assembled Hpp, Hll, b at the model's own estimates.
  3. one trial on the model's figures: Dinv, Hschur, bschur, x_p, x_l, scale, tmp.
  4. the driver's rules replayed exactly on the trace: rho, accept / restore, lambda, ni, the stop.
  5. the first linearisation's chi2 and largest diagonal, the final estimates, masks and counts.

EPS = 2^-53.  A sum of n terms computed in any order differs from another order by at most (n - 1) EPS sum|term| to first order
(Higham 4.2), and each term carries the roundings of its own products: a term of k operations has at most k EPS |term|.  The bounds
below are those counts, with the magnitudes taken from the model.

T_EST and M_REL, the tolerances of layer 5, are MEASURED ON THE MODEL, never on the code under test: `python tests/ba_checks.py` runs
the model over every scene under ORDERS random permutations of the edge order (within and across points) with numpy.linalg.solve
exchanged for Cholesky and scipy.linalg.ldl, and prints the largest spread of the final estimates and of the linearisations' chi2;
the tolerance is that spread times MARGIN.  Scenes whose model decisions differ between those runs (a mask or an accept flag
changes) are reported as `unclear` and are held to layers 1 to 4 only."""
import ctypes
import os
import sys

import numpy as np

import ba_model as bm
import host_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -53
DBL_MAX = bm.DBL_MAX

MUTATIONS = {"LAMBDA_POSE_ONLY": 1, "DINV_PLAIN": 2, "FIXED_W": 3, "SCHUR_ADD": 4, "NO_WX": 5, "REEVAL": 6, "RETURN": 7, "STEP_IDLE": 8, "TAU_POSES": 9}

# measured by `python tests/ba_checks.py` (seed 1, ORDERS = 4 permutations x 3 solvers, every scene of ba_model.SCENES); see DESIGN.md section 4
SEED, ORDERS, MARGIN = 1, 4, 4
EST_SPREAD = 5.1e-9           # largest |difference| of a final estimate (quaternion, t, point) between two model runs of a clear scene
CHI2_REL_SPREAD = 6.6e-10     # largest relative difference of a linearisation's or trial's chi2
T_EST, M_REL = MARGIN * EST_SPREAD, MARGIN * CHI2_REL_SPREAD
UNCLEAR = ()                  # scenes whose decisions change between the model's own runs


class Run:
    """One answered problem, from whichever build."""

    def __init__(self, res, trace):
        self.kf_estimate, self.kf_Tcw, self.point_estimate, self.points = res.kf_estimate, res.kf_Tcw, res.point_estimate, res.points
        self.removed1, self.removed2, self.n_removed1, self.n_removed2 = res.removed1, res.removed2, res.n_removed1, res.n_removed2
        self.iterations, self.n_trials, self.n_syncs, self.trace = tuple(res.iterations), res.n_trials, res.n_syncs, trace


def of_result(res, trace):
    return Run(res, trace)


def same_bits(a, b):
    """Equal bit for bit; non-finite values by class (NaN, +inf, -inf)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    fin = np.isfinite(a)
    if not np.array_equal(fin, np.isfinite(b)):
        return False
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    if not np.array_equal(a[fin].view(u), b[fin].view(u)):
        return False
    return bool(np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.sign(a[~fin & ~np.isnan(a)]), np.sign(b[~fin & ~np.isnan(b)])))


def same_run(a, b):
    """The names of what differs between two runs: estimates in double and float, both masks, counts, every trace record."""
    bad = [k for k in ("kf_estimate", "kf_Tcw", "point_estimate", "points", "removed1", "removed2") if not same_bits(getattr(a, k), getattr(b, k))]
    bad += [k for k in ("n_removed1", "n_removed2", "iterations", "n_trials", "n_syncs") if getattr(a, k) != getattr(b, k)]
    for part in ("lin", "trial"):
        x, y = getattr(a.trace, part), getattr(b.trace, part)
        if len(x) != len(y):
            bad.append(part + " count")
            continue
        bad += ["%s.%s" % (part, f) for f in x.dtype.names if not same_bits(x[f], y[f])]
    return bad


class Emu:
    """tests/emu/ba_emu.cpp, built on first use with the library's contract: no FMA contraction.  `mutation`: a key of MUTATIONS,
    compiled into a library of its own."""
    _libs = {}

    def __init__(self, uvo, mutation=None):
        assert mutation is None or mutation in MUTATIONS
        self.uvo = uvo
        if mutation not in Emu._libs:
            variant = (["-DBA_MUT=%d" % MUTATIONS[mutation]], "_" + mutation.lower()) if mutation else ()
            L = ctypes.CDLL(host_build.build("ba_emu", *variant))
            vp = ctypes.c_void_p
            L.emu_ba_adjust.argtypes = [vp, vp, vp]
            L.emu_ba_one_trial.argtypes = [vp, vp, vp, vp, ctypes.c_double] + [vp] * 13
            assert L.emu_ba_mutation() == (MUTATIONS[mutation] if mutation else 0)
            Emu._libs[mutation] = L
        self.L = Emu._libs[mutation]

    def adjust(self, sc):
        uvo = self.uvo
        c, r, arrays, keep = uvo.ba_marshal(sc, sc.get("mode", bm.LOCAL), sc.get("n_iterations", 0))
        t = uvo.BaTraceC()
        assert self.L.emu_ba_adjust(ctypes.byref(c), ctypes.byref(r), ctypes.byref(t)) == 0
        return Run(uvo.BaResult(r, arrays), uvo.BaTrace(t))

    def one_trial(self, sc, est, X, off, lam):
        """One linearisation and one trial at given estimates -> a dict of everything the phases leave."""
        c, r, arrays, keep = self.uvo.ba_marshal(sc)
        a = bm.arrays(sc)
        K, P, E, F = len(a["T"]), len(a["pts"]), len(a["ekf"]), a["F"]
        N = 6 * F
        o = dict(chi2=np.zeros(E), lin=np.zeros((E, 22)), Hll=np.zeros((P, 9)), Hpp=np.zeros((F, 27)), Dinv=np.zeros((P, 9)), Hs=np.zeros((N, N)), bs=np.zeros(N),
                 xp=np.zeros(N), xl=np.zeros((P, 3)), est_try=np.zeros((K, 7)), X_try=np.zeros((P, 3)), chi2_try=np.zeros(E), scal=np.zeros(5))
        est, X, off = np.ascontiguousarray(est, np.float64), np.ascontiguousarray(X, np.float64), np.ascontiguousarray(off, np.uint8)
        rc = self.L.emu_ba_one_trial(ctypes.byref(c), est.ctypes.data, X.ctypes.data, off.ctypes.data, float(lam), *[o[k].ctypes.data for k in
                                     ("chi2", "lin", "Hll", "Hpp", "Dinv", "Hs", "bs", "xp", "xl", "est_try", "X_try", "chi2_try", "scal")])
        assert rc == 0
        return o


_models = {}


def model(name):
    """(scene, the model's result), computed once and left unchanged."""
    if name not in _models:
        sc = bm.make(name)
        with np.errstate(all="ignore"):
            _models[name] = (sc, bm.optimize(sc))
    return _models[name]


def sym6(u21):
    """The 21 upper entries, row-major -> [6, 6]."""
    H = np.zeros((6, 6))
    H[np.triu_indices(6)] = u21
    return H + np.triu(H, 1).T


def sym3(u6):
    H = np.zeros((3, 3))
    H[np.triu_indices(3)] = u6
    return H + np.triu(H, 1).T


# ---- layer 1 ---------------------------------------------------------------------------------------------------------------------------
def check_edges(name, got, est, X, active, jac=True):
    """error -> chi2 and the Jacobians per active edge.  The camera point costs 15 operations on |q| = 1 and the point (18 EPS |X| + EPS |t|),
    the projection 3 more; the Jacobian entries are rational in the camera point with at most 6 operations each, plus the rotation's 12
    for the point's block: a relative bound of (24 + 6 + 12) EPS x the entry's conditioning 1 + |x/z| + |y/z| with respect to the camera
    point, which enters through x/z, y/z and 1/z only.  Returns the worst ratio difference / bound."""
    sc, _ = model(name)
    a = bm.arrays(sc)
    S = bm.System(a, est, X, active)
    pc = S.pc
    with np.errstate(all="ignore"):
        c = a["cams"][a["ecam"]].astype(np.float64)
        mag = np.linalg.norm(X[a["ept"]], axis=1) + np.linalg.norm(est[a["ekf"], 4:], axis=1)
        cond = (1 + np.abs(pc[:, 0] / pc[:, 2]) + np.abs(pc[:, 1] / pc[:, 2])) * mag / np.abs(pc[:, 2])
        be = 24 * EPS * (np.maximum(c[:, 0], c[:, 1]) * cond + np.abs(a["obs"]).max(1) + np.abs(c[:, 2:]).max(1))      # the error, per component
        err_mag = np.abs(S.err).max(1)
        bchi = a["w"] * (2 * err_mag * be * 2 + 8 * EPS * err_mag ** 2)
        rel = 42 * EPS * cond
    worst = 0.0
    idx = np.flatnonzero(active & np.isfinite(S.chi2))
    d = np.abs(got["chi2"][idx] - S.chi2[idx]) / (bchi[idx] + 1e-300)
    worst = max(worst, float(d.max()) if len(d) else 0.0)
    if not jac:
        return worst, S
    Jp, Jl = got["lin"][:, :12].reshape(-1, 2, 6), got["lin"][:, 12:18].reshape(-1, 2, 3)
    for G, M in ((Jp, S.Jp), (Jl, S.Jl)):
        scale = np.abs(M[idx]).max(axis=(1, 2))
        d = np.abs(G[idx] - M[idx]).max(axis=(1, 2)) / (rel[idx] * scale + 1e-300)
        worst = max(worst, float(d.max()) if len(d) else 0.0)
    return worst, S


# ---- layer 2 ---------------------------------------------------------------------------------------------------------------------------
def check_assembly(got, S):
    """Hpp, b_p, Hll, b_l: each entry is a sum over n edges of terms of 4 operations on Jacobian entries that carry layer 1's relative
    bound r, so |difference| <= ((n - 1) + 4 + 3 r / EPS) EPS sum|term|, the magnitudes from the model.  Returns the worst ratio."""
    a = S.a
    with np.errstate(all="ignore"):
        pc = S.pc
        cond = (1 + np.abs(pc[:, 0] / pc[:, 2]) + np.abs(pc[:, 1] / pc[:, 2])) / np.abs(pc[:, 2])
    worst = 0.0
    F, P = len(S.Hpp), len(S.Hll)
    rho1 = bm.pom.huber(S.chi2)[1]
    w = a["w"].astype(np.float64) * rho1
    r = np.abs(w[:, None] * S.err)
    e = S.to_free
    absH, absb = np.zeros((F, 6, 6)), np.zeros((F, 6))
    np.add.at(absH, S.f[e], np.einsum("eia,e,eib->eab", np.abs(S.Jp[e]), w[e], np.abs(S.Jp[e])))
    np.add.at(absb, S.f[e], np.einsum("eia,ei->ea", np.abs(S.Jp[e]), r[e]))
    n_f = np.bincount(S.f[e], minlength=F)
    absL, absl = np.zeros((P, 3, 3)), np.zeros((P, 3))
    np.add.at(absL, a["ept"][S.idx], np.einsum("eia,e,eib->eab", np.abs(S.Jl[S.idx]), w[S.idx], np.abs(S.Jl[S.idx])))
    np.add.at(absl, a["ept"][S.idx], np.einsum("eia,ei->ea", np.abs(S.Jl[S.idx]), r[S.idx]))
    n_p = np.bincount(a["ept"][S.idx], minlength=P)
    # a term's own roundings: its 4 operations; its three factors (two Jacobian entries and the weight, or one and the residual) each with
    # layer 1's relative bound 42 EPS x the edge's conditioning, the worst edge taken for all; and rho1 = delta / sqrt(chi2) in the
    # weight: chi2's 8 operations halved by the root, the root, the divide and the product with the information -- 8 at the most
    k = 4 + 3 * 42 * float(np.nanmax(np.where(S.active, cond * (np.linalg.norm(S.pc, axis=1) + 1), 0))) + 8
    for f in range(F):
        if not S.f_on[f]:
            continue
        d = np.abs(sym6(got["Hpp"][f, :21]) - S.Hpp[f]) / ((n_f[f] + k) * EPS * absH[f] + 1e-300)
        db = np.abs(got["Hpp"][f, 21:] - S.bp[f]) / ((n_f[f] + k) * EPS * absb[f] + 1e-300)
        worst = max(worst, float(d.max()), float(db.max()))
    on = np.flatnonzero(S.p_on)
    for j in on:
        d = np.abs(sym3(got["Hll"][j, :6]) - S.Hll[j]) / ((n_p[j] + k) * EPS * absL[j] + 1e-300)
        db = np.abs(got["Hll"][j, 6:] - S.bl[j]) / ((n_p[j] + k) * EPS * absl[j] + 1e-300)
        worst = max(worst, float(d.max()), float(db.max()))
    return worst, k


# ---- layer 3 ---------------------------------------------------------------------------------------------------------------------------
def check_trial(got, S, lam, k):
    """One trial at lambda: Dinv, the reduced system, x_p, x_l.  The inputs differ by layer 2's relative bound u = (n + k) EPS; a solve of
    A x = b answers perturbations of relative size u in A and b, and its own backward error (3 n^2 EPS for an LDL^T of order n without
    growth), with |dx| / |x| <= 2 kappa(A) (u + 3 n^2 EPS) / (1 - kappa ...), first order.  Returns the worst ratio."""
    a = S.a
    ok, xp, xl = S.trial(lam)
    F, P = len(S.Hpp), len(S.Hll)
    n_max = int(max(np.bincount(S.f[S.to_free], minlength=F).max(), 1))
    u = (n_max + k) * EPS
    worst = 0.0
    on = np.flatnonzero(S.p_on)
    kap_l = np.array([np.linalg.cond(S.Hll[j] + lam * np.eye(3)) for j in on]) if len(on) else np.zeros(0)
    for n, j in enumerate(on):
        D = sym3(got["Dinv"][j, :6])
        worst = max(worst, float(np.abs(D - S.Dinv[j]).max() / (2 * kap_l[n] * (u + 32 * EPS) * np.abs(S.Dinv[j]).max())))
    act = np.flatnonzero(S.f_on)
    N = 6 * len(act)
    A = S.Hs[np.ix_(act, act)].transpose(0, 2, 1, 3).reshape(N, N)
    A = np.triu(A) + np.triu(A, 1).T
    G = got["Hs"].reshape(6 * F, 6 * F)
    G = np.tril(G) + np.tril(G, -1).T
    rows = np.concatenate([np.arange(6 * f, 6 * f + 6) for f in act]) if len(act) else np.zeros(0, int)
    G = G[np.ix_(rows, rows)]
    kl = float(kap_l.max()) if len(kap_l) else 1.0
    # An entry of a Schur term W Dinv W^T is 9 products w d w'.  Each carries Dinv's relative error, 2 kappa_l (u + 32 EPS) as above,
    # and W's on both sides, 2 u.  Their magnitudes: sum_j W Dinv W^T is at most Hpp in the positive semi-definite order, so an entry is
    # at most the largest diagonal entry of Hpp + lambda I, scale_A; cancellation among the 9 is not counted, hence 9 scale_A.  Hpp's own
    # entry adds u scale_A.  bschur's correction W Dinv b_l is 9 products of the same kind, on the scale of b_p and bschur.
    scale_A = np.abs(S.Hpp).max() + lam
    rel_term = 2 * kl * (u + 32 * EPS) + 2 * u
    tolA = (9 * rel_term + u) * scale_A
    worst = max(worst, float(np.abs(G - A).max() / tolA))
    worst = max(worst, float(np.abs(got["bs"][rows] - S.bs[act].reshape(N)).max() / ((9 * rel_term + u) * (np.abs(S.bp).max() + np.abs(S.bs).max()))))
    if ok:
        kap = np.linalg.cond(A)
        rel = 2 * kap * (tolA / scale_A + 3 * N * N * EPS)
        xpn = np.abs(xp).max()
        worst = max(worst, float(np.abs(got["xp"].reshape(F, 6)[act] - xp[act]).max() / (rel * xpn + 1e-300)))
        xln = np.abs(xl).max()
        worst = max(worst, float(np.abs(got["xl"][on] - xl[on]).max() / ((rel * kl + 2 * kl * u) * (xln + xpn) + 1e-300)))
        assert got["scal"][2] == 1.0
    else:
        assert got["scal"][2] == 0.0 and got["scal"][3] == DBL_MAX
    return worst, ok


# ---- layer 4 ---------------------------------------------------------------------------------------------------------------------------
def replay(run, mode=bm.LOCAL, n_iterations=0):
    """The driver's rules replayed exactly on the trace: every trial's accept flag, the next lambda, ni, which trial follows which, the
    stop of each optimize() and the iteration counts follow from the records' own cur, tmp, scale by the rules of
    optimization_algorithm_levenberg.cpp.  Returns the list of violations."""
    lin, tr = run.trace.lin, run.trace.trial
    bad = []
    t = 0
    its = [0, 0]
    pos = 0
    rounds = 2 if mode == bm.LOCAL else 1
    for rnd in range(rounds):
        cap = (5, 10)[rnd] if mode == bm.LOCAL else n_iterations
        lam = ni = None
        stalled = 0
        stopped = False
        it = 0
        while pos < len(lin) and lin[pos]["round"] == rnd:
            L = lin[pos]
            if stopped or it >= cap or L["iteration"] != it:
                bad.append("linearisation %d runs after the stop, or out of turn" % pos)
            if it == 0:
                lam, ni, stalled = 1e-5 * L["maxdiag"], 2.0, 0
            cur = ini = L["chi2"]
            q, rho = 0, 0.0
            while True:
                if t >= len(tr) or tr[t]["lin"] != pos:
                    bad.append("linearisation %d: a trial is missing" % pos)
                    return bad
                r = tr[t]
                if not (same_bits(r["lambda"], lam) and same_bits(r["cur"], cur)):
                    bad.append("trial %d: lambda or currentChi is not what the rules give" % t)
                if (not r["ok"]) != (r["tmp"] == DBL_MAX and not r["ok"]):
                    bad.append("trial %d: a failed solve without DBL_MAX" % t)
                with np.errstate(all="ignore"):
                    rho = (np.float64(r["cur"]) - r["tmp"]) / r["scale"]
                accept = bool(rho > 0 and np.isfinite(r["tmp"]))
                if accept != bool(r["accepted"]):
                    bad.append("trial %d: accepted %d against the rule" % (t, r["accepted"]))
                if accept:
                    u = 2.0 * rho - 1.0
                    alpha = min(1.0 - u * u * u, 2.0 / 3.0)
                    lam, ni, cur = r["lambda"] * max(1.0 / 3.0, alpha), 2.0, r["tmp"]
                else:
                    lam, ni = r["lambda"] * ni, ni * 2.0
                q += 1
                t += 1
                if not (rho < 0 and q < 10):
                    break
            its[rnd] += 1
            it += 1
            pos += 1
            if q == 10 or rho == 0:
                stopped = True
            else:
                stalled = stalled + 1 if (ini - cur) * 1e3 < ini else 0
                stopped = stalled >= 3
        if not stopped and it < cap and it > 0:
            bad.append("round %d stops after %d of %d iterations without a reason" % (rnd, it, cap))
    if t != len(tr) or pos != len(lin):
        bad.append("records left over")
    if tuple(its) != tuple(run.iterations) or run.n_trials != len(tr):
        bad.append("the counts %s %d are not the trace's %s %d" % (run.iterations, run.n_trials, its, len(tr)))
    return bad


# ---- layer 5 ---------------------------------------------------------------------------------------------------------------------------
def clear(name):
    """Whether the model's decisions in the scene are clear of the thresholds: estimates that differ by T_EST in each of an edge's nine
    coordinates move its error by at most 9 G T_EST (G the largest Jacobian entry of the scene) and its chi2 near 5.991 by at most
    2 sqrt(5.991) times that (w <= 1); the depth moves by at most (|X| + 2) T_EST < 1e-6; rho is held away from 0 by 1e-3, its scale
    being bounded below by the 1e-3 the driver adds.  And the scene is not listed as unclear by the measurement."""
    if name in UNCLEAR:
        return False
    _, res = model(name)
    if bm_not_finite(res):
        return False
    sc = model(name)[0]
    a = bm.arrays(sc)
    L0 = res.lin[0]
    J = bm.jacobians(a, L0["est"], bm.edge_errors(a, L0["est"], L0["X"])[0])
    G = max(float(np.abs(J[0][L0["active"]]).max()), float(np.abs(J[1][L0["active"]]).max()))
    for c in res.checks:
        ex = c["examined"]
        if np.any(np.abs(c["stored"][ex] - bm.TH) <= 2 * bm.TH ** 0.5 * 9 * G * T_EST) or np.any(np.abs(c["depth"][ex]) <= 1e-6):
            return False
    return all(abs(t["rho"]) > 1e-3 for t in res.trials)


def bm_not_finite(res):
    return not all(np.isfinite(t["tmp"]) and t["ok"] for t in res.trials) or not all(np.isfinite(l["chi2"]) for l in res.lin)


def check_final(name, run):
    """The first linearisation against the model's within M_REL; in a clear scene the trajectory's chi2 within M_REL, the final estimates
    within T_EST, masks, counts and iteration counts equal."""
    sc, res = model(name)
    bad = []
    if len(run.trace.lin) and np.isfinite(res.lin[0]["chi2"]):
        l0, m0 = run.trace.lin[0], res.lin[0]
        if abs(l0["chi2"] - m0["chi2"]) > M_REL * abs(m0["chi2"]) or abs(l0["maxdiag"] - m0["maxdiag"]) > M_REL * abs(m0["maxdiag"]):
            bad.append("first linearisation: chi2 %r against %r, maxdiag %r against %r" % (l0["chi2"], m0["chi2"], l0["maxdiag"], m0["maxdiag"]))
        if (l0["n_edges"], l0["n_free"], l0["n_points"]) != (m0["n_edges"], m0["n_free"], m0["n_points"]):
            bad.append("first linearisation: the active counts differ")
    if not clear(name):
        return bad
    if tuple(run.iterations) != tuple(res.iterations) or run.n_trials != len(res.trials):
        bad.append("iterations %s trials %d, the model %s %d" % (run.iterations, run.n_trials, res.iterations, len(res.trials)))
        return bad
    for k, (l, m) in enumerate(zip(run.trace.lin, res.lin)):
        if abs(l["chi2"] - m["chi2"]) > M_REL * abs(m["chi2"]) or (l["n_edges"], l["n_free"], l["n_points"]) != (m["n_edges"], m["n_free"], m["n_points"]):
            bad.append("linearisation %d: chi2 %r against %r" % (k, l["chi2"], m["chi2"]))
    for k, (r, m) in enumerate(zip(run.trace.trial, res.trials)):
        if bool(r["accepted"]) != m["accepted"] or bool(r["ok"]) != m["ok"]:
            bad.append("trial %d: the verdict differs" % k)
    if not (np.array_equal(run.removed1, res.removed1) and np.array_equal(run.removed2, res.removed2)):
        bad.append("masks: %d %d against the model's %d %d" % (run.n_removed1, run.n_removed2, res.n_removed1, res.n_removed2))
    if (run.n_removed1, run.n_removed2) != (int(run.removed1.sum()), int(run.removed2.sum())):
        bad.append("the counts are not the masks'")
    d = max(float(np.abs(run.kf_estimate - res.est).max()), float(np.abs(run.point_estimate - res.X).max()))
    if not d <= T_EST:
        bad.append("final estimates differ by %.3e, T = %.1e" % (d, T_EST))
    if np.abs(run.kf_Tcw.astype(np.float64) - res.kf_Tcw).max() > T_EST + 2.0 ** -23 * 16 or np.abs(run.points.astype(np.float64) - res.points).max() > T_EST + 2.0 ** -23 * 16:
        bad.append("the float outputs are not the estimates rounded")
    return bad


def check_layers(emu, name):
    """Layers 1 to 3 on the model's own estimates: at its first and last linearisation with the lambda it starts that optimize() with, and
    at its first rejected trial with that trial's lambda.  In each the stored error after the trial, accepted or not, must be the error
    at the TRIED estimates (layer 1's bound at the build's own tried estimates), and the verdict the model's."""
    sc, res = model(name)
    out = []
    cases = [(res.lin[0], None), (res.lin[-1], None)]
    rej = [t for t in res.trials if t["ok"] and not t["accepted"] and abs(t["rho"]) > 1e-3]
    if rej:
        cases.append((res.lin[rej[0]["lin"]], rej[0]))
    for L, t in cases:
        if not np.isfinite(L["chi2"]):
            continue
        lam = t["lam"] if t else L["lam0"] if np.isfinite(L["lam0"]) and L["lam0"] > 0 else 1.0
        got = emu.one_trial(sc, L["est"], L["X"], (~L["active"]).astype(np.uint8), lam)
        w1, S = check_edges(name, got, L["est"], L["X"], L["active"])
        w2, k = check_assembly(got, S)
        w3, ok = check_trial(got, S, lam, k)
        w4, _ = check_edges(name, dict(chi2=got["chi2_try"]), got["est_try"], got["X_try"], L["active"], jac=False)
        if t:
            assert got["scal"][3] > L["chi2"] or not np.isfinite(got["scal"][3]), "the model rejects this trial"
        out.append((max(w1, w4), w2, w3))
    return out


def check_all(name, run):
    sc, _ = model(name)
    bad = replay(run, sc.get("mode", bm.LOCAL), sc.get("n_iterations", 0)) + check_final(name, run)
    assert not bad, (name, bad)


# ---- the measurement -------------------------------------------------------------------------------------------------------------------
def measure_spread(names, orders=ORDERS, seed=SEED):
    """The model's own spread under permuted edge orders and exchanged solvers -> (estimate spread, relative chi2 spread, unclear scenes)."""
    est_s = chi_s = 0.0
    unclear = []
    for name in names:
        sc, ref = model(name)
        if bm_not_finite(ref):
            continue
        E = len(sc["edge_kf"])
        rng = np.random.RandomState([seed, list(bm.SCENES).index(name)])      # a scene's orders do not depend on which others are measured
        flips = False
        e_here = c_here = 0.0
        for k in range(orders):
            order = rng.permutation(E)
            for solver in ("solve", "cholesky", "ldl"):
                with np.errstate(all="ignore"):
                    r = bm.optimize(sc, order=order, solver=solver)
                if (len(r.trials) != len(ref.trials) or [t["accepted"] for t in r.trials] != [t["accepted"] for t in ref.trials] or
                        not np.array_equal(r.removed1, ref.removed1) or not np.array_equal(r.removed2, ref.removed2)):
                    flips = True
                    continue
                e_here = max(e_here, float(np.abs(r.est - ref.est).max()), float(np.abs(r.X - ref.X).max()))
                c_here = max(c_here, max(abs(x["chi2"] - y["chi2"]) / abs(y["chi2"]) for x, y in zip(r.lin, ref.lin)))
        print("%-18s estimate spread %.3e  relative chi2 spread %.3e%s" % (name, e_here, c_here, "  UNCLEAR" if flips else ""))
        if flips:
            unclear.append(name)
        else:
            est_s, chi_s = max(est_s, e_here), max(chi_s, c_here)
    return est_s, chi_s, unclear


if __name__ == "__main__":
    e, c, u = measure_spread(list(bm.SCENES))
    print("estimate spread %.3e, relative chi2 spread %.3e, unclear %s (seed %d, %d orders x 3 solvers); recorded %.1e %.1e %s" %
          (e, c, u, SEED, ORDERS, EST_SPREAD, CHI2_REL_SPREAD, list(UNCLEAR)))
    sys.exit(0)
