"""The layer checks of the visual-inertial bundle adjustment: the host build of csrc/navba_core.hpp (tests/emu/navba_emu.cpp) and the
device (through the same functions) against the numpy model tests/navba_model.py.  DESIGN.md section 4 (contract 13) states the
contract; the bounds are derived here.

  1. per edge -- mono, PVR, bias, depth: error, chi2, every Jacobian block.
  2. the assembled blocks at the model's own estimates: the mono sums per key frame and per point, every inertial edge's (rho1 Omega) J
     and (rho1 Omega) e, and b of the 15-blocks before the points' correction.
  3. one whole trial on the model's figures: the reduced 15F x 15F system as assembled, its right-hand side, x_p, x_l, scale, tmp.
  4. the driver's rules replayed exactly on the trace.
  5. the first linearisation's chi2 and largest diagonal entry, the final states and points, both masks, counts.

EPS = 2^-53.  A sum of n terms computed in any order differs from another order by at most (n - 1) EPS sum|term| to first order
(Higham 4.2), and each term carries the roundings of its own products.  The bounds below are those counts with the magnitudes taken
from the model; the derivations of the per-edge bounds are tests/navopt_checks.py's (single_bounds, reproj_bounds), restated where used.

T_EST and M_REL, the tolerances of layer 5, are MEASURED ON THE MODEL, never on the code under test: `python tests/navba_checks.py`
runs the model over every scene under ORDERS random permutations of the mono edge order with the reduced solve exchanged ("solve",
"cholesky", "full": no Schur complement at all), and prints the largest spread of the final estimates and of the linearisations'
chi2; the tolerance is that spread times MARGIN.  A scene whose model decisions differ between those runs would be `unclear` and held to
layers 1 to 4 only: none is."""
import ctypes
import os
import sys

import numpy as np

import ba_checks as bc
import host_build
import navba_model as vm
import navopt_model as nm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -53
DBL_MAX = vm.DBL_MAX
IE_WORDS, IE_J, IE_WJ, IE_E, IE_WE, IE_CHI = 562, 0, 270, 540, 549, 558

MUTATIONS = {"V_COLUMNS": 1, "SCATTER_0_5": 2, "BACKWARD_PREINT": 3, "CHECK_FLOAT": 4, "KEEP_KERNEL": 5, "FLAGGED_KERNEL_OFF": 6, "FINAL_SKIPS_EXCLUDED": 7,
             "ORDER": 8, "BIAS_NO_DT": 9, "TAU_POSES": 10}

build = host_build.build        # "navba_emu", "navba_emu_main" and "compat_navba" are rows of tests/host_build.py's table

# measured by `python tests/navba_checks.py` (seed 1, ORDERS = 4 permutations x 3 solvers, every scene of navba_model.SCENES); DESIGN.md section 4
SEED, ORDERS, MARGIN = 1, 4, 4
EST_SPREAD = 3.5e-10          # largest |difference| of a final state or point between two model runs of a scene: 3.329e-10, free1_p8
CHI2_REL_SPREAD = 9.2e-11     # largest relative difference of a linearisation's chi2: 8.763e-11, far_start
SETS_SPREAD = ("free1_p8", "far_start")     # the scenes that set the two maxima
T_EST, M_REL = MARGIN * EST_SPREAD, MARGIN * CHI2_REL_SPREAD
UNCLEAR = ()

same_bits = bc.same_bits


class Run:
    """One answered window, from whichever build."""

    def __init__(self, res, trace):
        self.kf_state, self.kf_Tcw, self.point_estimate, self.points = res.kf_state, res.kf_Tcw, res.point_estimate, res.points
        self.excluded, self.erased, self.n_excluded, self.n_erased = res.excluded, res.erased, res.n_excluded, res.n_erased
        self.iterations, self.n_trials, self.n_syncs, self.trace = tuple(res.iterations), res.n_trials, res.n_syncs, trace


def of_result(res, trace):
    return Run(res, trace)


def same_run(a, b):
    """The names of what differs between two runs: states and points in double and float, both masks, counts, every trace record."""
    bad = [k for k in ("kf_state", "kf_Tcw", "point_estimate", "points", "excluded", "erased") if not same_bits(getattr(a, k), getattr(b, k))]
    bad += [k for k in ("n_excluded", "n_erased", "iterations", "n_trials", "n_syncs") if getattr(a, k) != getattr(b, k)]
    for part in ("lin", "trial"):
        x, y = getattr(a.trace, part), getattr(b.trace, part)
        if len(x) != len(y):
            bad.append(part + " count")
            continue
        bad += ["%s.%s" % (part, f) for f in x.dtype.names if not same_bits(x[f], y[f])]
    return bad


class Emu:
    """tests/emu/navba_emu.cpp, built on first use with the library's contract: no FMA contraction.  `mutation`: a key of MUTATIONS,
    compiled into a library of its own."""
    _libs = {}

    def __init__(self, uvo, mutation=None):
        assert mutation is None or mutation in MUTATIONS
        self.uvo = uvo
        if mutation not in Emu._libs:
            variant = (["-DNAVBA_MUT=%d" % MUTATIONS[mutation]], "_" + mutation.lower()) if mutation else ()
            L = ctypes.CDLL(build("navba_emu", *variant))
            vp = ctypes.c_void_p
            L.emu_navba_adjust.argtypes = [vp, vp, vp]
            L.emu_navba_one_trial.argtypes = [vp, vp, vp, vp, vp, ctypes.c_double] + [vp] * 14
            assert L.emu_navba_mutation() == (MUTATIONS[mutation] if mutation else 0)
            Emu._libs[mutation] = L
        self.L = Emu._libs[mutation]

    def adjust(self, sc):
        uvo = self.uvo
        c, r, arrays, keep = uvo.navba_marshal(sc)
        t = uvo.NavBaTraceC()
        assert self.L.emu_navba_adjust(ctypes.byref(c), ctypes.byref(r), ctypes.byref(t)) == 0
        return Run(uvo.NavBaResult(r, arrays), uvo.NavBaTrace(t))

    def one_trial(self, sc, est, X, off, rob, lam):
        """One linearisation and one trial at given estimates -> a dict of everything the phases leave."""
        c, r, arrays, keep = self.uvo.navba_marshal(sc)
        a = vm.arrays(sc)
        K, P, E, F, G = len(a["st"]), len(a["pts"]), len(a["ekf"]), a["F"], 2 * len(a["links"]) + len(a["depth"])
        N = 15 * F
        o = dict(chi2=np.zeros(E + 1), lin=np.zeros((E + 1, 22)), ie=np.zeros((G + 1, IE_WORDS)), Hll=np.zeros((P + 1, 9)), Hpp=np.zeros((F, 27)), Hs=np.zeros((N, N)),
                 bs=np.zeros(N), bfull=np.zeros(N), xp=np.zeros(N), xl=np.zeros((P + 1, 3)), est_try=np.zeros((K, 22)), X_try=np.zeros((P + 1, 3)),
                 chi2_try=np.zeros(E + 1), scal=np.zeros(5))
        est = np.ascontiguousarray(np.stack([nm.state_vec(s) for s in est]), np.float64)
        X, off, rob = np.ascontiguousarray(X, np.float64), np.ascontiguousarray(off, np.uint8), np.ascontiguousarray(rob, np.uint8)
        rc = self.L.emu_navba_one_trial(ctypes.byref(c), est.ctypes.data, X.ctypes.data, off.ctypes.data, rob.ctypes.data, float(lam), *[o[k].ctypes.data for k in
                                        ("chi2", "lin", "ie", "Hll", "Hpp", "Hs", "bs", "bfull", "xp", "xl", "est_try", "X_try", "chi2_try", "scal")])
        assert rc == 0
        for k in ("chi2", "chi2_try"):
            o[k] = o[k][:E]
        o["lin"], o["ie"], o["Hll"], o["xl"], o["X_try"] = o["lin"][:E], o["ie"][:G], o["Hll"][:P], o["xl"][:P], o["X_try"][:P]
        return o


_models = {}


def model(name):
    """(scene, the model's result), computed once and left unchanged."""
    if name not in _models:
        sc = vm.make(name) if name in vm.SCENES else getattr(vm, name)()
        with np.errstate(all="ignore"):
            _models[name] = (sc, vm.optimize(sc))
    return _models[name]


sym6, sym3 = bc.sym6, bc.sym3


def S_X(S):
    return S.X


# ---- layer 1 ---------------------------------------------------------------------------------------------------------------------------
def mono_bounds(a, est, X, S):
    """tests/navopt_checks.py's reproj_bounds for Pc = (Rcb Rwb^T) (Pw - Pwb) - Rcb Pbc: the matrix product's entries are good to 8 EPS, the
    difference to EPS |d|, the three products and two sums of a row add 5 EPS each on 3 |d|: dp = 64 EPS (|Pw| + |Pwb| + |Pbc|) per
    coordinate.  chi2 = w (e0^2 + e1^2), good to 2 w (|e0| + |e1| + de) de, with de = f (dp / |z|) (1 + |x / z|) + 5 EPS (|obs| + f |x / z| + |c|).  A Jacobian entry is
    (f / z) (1, x / z or y / z) times an entry of Rcb, of hat(Paux) Rcb (|.| <= 2 |Paux|) or of Rcb Rwb^T: relative 16 EPS + 9 dp / |z| on the
    scale (f / |z|) (1 + |x / z| + |y / z|) (1 + 2 |Paux|)."""
    pc = S.pc
    with np.errstate(all="ignore"):
        c = a["cams"][a["ecam"]].astype(np.float64)
        Pwb = np.stack([s["P"] for s in est])
        dp = 64 * EPS * (np.abs(X[a["ept"]]).max(1) + np.abs(Pwb[a["ekf"]]).max(1) + float(np.abs(a["Pbc"]).max()))
        x, y, z = pc[:, 0], pc[:, 1], pc[:, 2]
        f = np.maximum(c[:, 0], c[:, 1])
        de = f * (dp / np.abs(z)) * (1 + np.maximum(np.abs(x / z), np.abs(y / z))) + 5 * EPS * (np.abs(a["obs"]).max(1) + f * np.maximum(np.abs(x / z), np.abs(y / z)) + np.abs(c[:, 2:]).max(1))
        dchi = 2 * a["w"] * (np.abs(S.err[:, 0]) + np.abs(S.err[:, 1]) + de) * de + 5 * EPS * S.chi2
        aux = np.linalg.norm(pc, axis=1) + float(np.abs(a["Pbc"]).max())
        dJ = (16 * EPS + 9 * dp / np.abs(z)) * (f / np.abs(z)) * (1 + np.abs(x / z) + np.abs(y / z)) * (1 + 2 * aux)
    return de, dchi, dJ


def inertial_bounds(a, est):
    """de (per row) and dJ (one number) of every inertial edge, tests/navopt_checks.py's single_bounds: a position, velocity, bias or depth
    row is a chain of at most 64 additions and products of quantities whose absolute values sum to at most m, rotated (x 4): 256 EPS
    (1 + m); a rotation row is the log of a product of four unit quaternions: 1024 EPS; a Jacobian entry is at most a product of four
    3 x 3 matrices with entries bounded by 1 + m: 1024 EPS (1 + m).  m is taken over the edge's states and its link.  One factor needs more:
    JacobianR(theta_b), theta_b = |JRg dbg|, holds (1 - cos theta_b) / theta_b, and two cosines good to 4 EPS absolute differ by 8 EPS there:
    8 EPS / theta_b on a factor of the PVR edge's bias block, whenever theta_b is above JacobianR's own threshold of 1e-5."""
    ab = lambda v: float(np.abs(np.asarray(v, np.float64)).max())
    out = []

    def mag(states, lk, extra=0.0):
        dT = float(lk["dT"])
        m = sum(ab(s["P"]) + ab(s["V"]) * (1 + dT) + ab(s["bg"]) + ab(s["ba"]) + ab(s["dbg"]) + ab(s["dba"]) for s in states)
        db = max(max(ab(s["dbg"]), ab(s["dba"])) for s in states)
        m += ab(a["gw"]) * (dT + dT * dT) + 9.81 * dT * dT + ab(lk["dP"]) + ab(lk["dV"]) + (ab(lk["JPg"]) + ab(lk["JPa"]) + ab(lk["JVg"]) + ab(lk["JVa"]) + ab(lk["JRg"])) * 3 * db
        return m + extra + dT

    for lk in a["links"]:
        m = mag([est[int(lk["kf0"])], est[int(lk["kf1"])]], lk)
        de = np.full(9, 256 * EPS * (1 + m))
        de[6:9] = 1024 * EPS
        theta_b = float(np.linalg.norm(nm.M3(lk["JRg"]) @ est[int(lk["kf0"])]["dbg"]))
        out.append((de, (1024 + (8 / theta_b if theta_b >= 1e-5 else 0.0)) * EPS * (1 + m)))
        out.append((np.full(6, 256 * EPS * (1 + m)), 0.0))              # the bias edge's Jacobian is -I, I: exact
    for d in a["depth"]:
        lk = a["links"][int(d["link"])]
        m = mag([est[int(d["ka"])], est[int(d["kb"])], est[int(d["kc"])]], lk, abs(float(d["meas"])) * (1 + abs(float(d["shi"]))))
        out.append((np.full(1, 256 * EPS * (1 + m) * (1 + abs(float(d["shi"])))), 1024 * EPS * (1 + m)))
    return out


SLOT = {"p0": 0, "p1": 9, "b0": 18, "b1": 24}


def slots_of(kind):
    """Where the model's blocks, in its order, stand among the 30 columns of the build's Jacobian."""
    return {"pvr": (0, 9, 18), "bias": (18, 24), "depth": (0, 9, 18)}[kind]


def kinds(a):
    return ["pvr", "bias"] * len(a["links"]) + ["depth"] * len(a["depth"])


def dense_edge(kind, blocks, m):
    J = np.zeros((m, 30))
    for base, (key, blk) in zip(slots_of(kind), blocks):
        J[:, base:base + blk.shape[1]] = blk
    return J


def check_edges(name, got, est, X, active, rob, jac=True):
    """Layer 1.  Returns the worst ratio difference / bound, and the model's system at these estimates."""
    sc, _ = model(name)
    a = vm.arrays(sc)
    S = vm.System(a, est, X, active, rob)
    de, dchi, dJ = mono_bounds(a, est, X, S)
    worst = 0.0
    idx = np.flatnonzero(active & np.isfinite(S.chi2))
    d = np.abs(got["chi2"][idx] - S.chi2[idx]) / (dchi[idx] + 1e-300)
    worst = max(worst, float(d.max()) if len(d) else 0.0)
    if not jac:
        return worst, S
    Jp, Jl = got["lin"][:, :12].reshape(-1, 2, 6), got["lin"][:, 12:18].reshape(-1, 2, 3)
    assert (S.Jp[idx][:, :, 3:6] == 0).all()
    for G, M in ((Jp, S.Jp[:, :, vm.PVR_MONO]), (Jl, S.Jl)):
        d = np.abs(G[idx] - M[idx]).max(axis=(1, 2)) / (dJ[idx] + 1e-300)
        worst = max(worst, float(d.max()) if len(d) else 0.0)
    for g, ((e, info, delta, blocks), (dee, dJs), kind) in enumerate(zip(S.inert, inertial_bounds(a, est), kinds(a))):
        m = len(e)
        I = got["ie"][g]
        worst = max(worst, float((np.abs(I[IE_E:IE_E + m] - e) / dee).max()))
        Jm, Jg = dense_edge(kind, blocks, m), I[IE_J:IE_J + 270].reshape(9, 30)
        assert (Jg[m:] == 0).all() and (Jg[:m][Jm == 0] == 0).all() if kind != "pvr" else (Jg[m:] == 0).all(), (name, g, "a Jacobian entry outside the edge's blocks")
        worst = max(worst, float(np.abs(Jg[:m] - Jm).max() / (dJs + 1e-300)) if dJs else float((Jg[:m] != Jm).any()) * 2)
        with np.errstate(all="ignore"):
            c2 = float(e @ (info @ e))
            rel_om = float(np.linalg.cond(info)) * (3 * 9 + 3 * 81) * EPS if kind == "pvr" else 4 * EPS
            dchi2 = float(2 * np.abs(e) @ (np.abs(info) @ dee) + np.abs(e) @ (np.abs(info) @ np.abs(e)) * (rel_om + (m + 2) * EPS))
        worst = max(worst, abs(I[IE_CHI] - c2) / (dchi2 + 1e-300))
    return worst, S


# ---- layer 2 ---------------------------------------------------------------------------------------------------------------------------
def check_assembly(got, S, est):
    """The mono sums (tests/ba_checks.py's check_assembly: ((n - 1) + 4 + 3 r / EPS) EPS sum|term| with r layer 1's relative bound; the
    residual's own error de is absolute, not relative -- a point with one edge ends with a residual of exactly zero -- so b's bound adds
    sum |J| w rho1 de), every
    inertial edge's WJ = (rho1 Omega) J and We: a sum over s < m of products of three factors, dWJ <= |W| dJ + dW |J| + (m + 2) EPS |W| |J|
    with dW = |W| (dOmega / Omega + drho1 / rho1) -- dOmega / Omega = cond(CovPVPhi) (3 n + 3 n^2) EPS at n = 9 for the PVR edge (two
    different inverses), 4 EPS else -- and b of the 15-blocks: the mono sum's bound plus, per inertial edge,
    dJ^T |We| + |J|^T dWe + (m + n_edges) EPS |J|^T |We|.  Returns the worst ratio and k."""
    a = S.a
    with np.errstate(all="ignore"):
        pc = S.pc
        cond = (1 + np.abs(pc[:, 0] / pc[:, 2]) + np.abs(pc[:, 1] / pc[:, 2])) / np.abs(pc[:, 2])
    worst = 0.0
    F, P = a["F"], len(S.Hll)
    rho1 = np.where(S.chi2 <= nm.D_MONO ** 2, 1.0, nm.D_MONO / np.sqrt(np.maximum(S.chi2, 1e-300)))
    w = a["w"].astype(np.float64) * np.where(np.isfinite(rho1), rho1, 1.0)
    r = np.abs(w[:, None] * S.err)
    e = S.to_free
    Jp6 = np.abs(S.Jp[:, :, vm.PVR_MONO])
    absH, absb = np.zeros((F, 6, 6)), np.zeros((F, 6))
    np.add.at(absH, S.f[e], np.einsum("eia,e,eib->eab", Jp6[e], w[e], Jp6[e]))
    np.add.at(absb, S.f[e], np.einsum("eia,ei->ea", Jp6[e], r[e]))
    n_f = np.bincount(S.f[e], minlength=F)
    de = mono_bounds(a, est, S_X(S), S)[0]
    rde = (w * de)[:, None] * np.ones((1, 2))
    addb, addl = np.zeros((F, 6)), np.zeros((P, 3))
    np.add.at(addb, S.f[e], np.einsum("eia,ei->ea", Jp6[e], rde[e]))
    np.add.at(addl, a["ept"][S.idx], np.einsum("eia,ei->ea", np.abs(S.Jl[S.idx]), rde[S.idx]))
    absL, absl = np.zeros((P, 3, 3)), np.zeros((P, 3))
    np.add.at(absL, a["ept"][S.idx], np.einsum("eia,e,eib->eab", np.abs(S.Jl[S.idx]), w[S.idx], np.abs(S.Jl[S.idx])))
    np.add.at(absl, a["ept"][S.idx], np.einsum("eia,ei->ea", np.abs(S.Jl[S.idx]), r[S.idx]))
    n_p = np.bincount(a["ept"][S.idx], minlength=P)
    k = 4 + 3 * 64 * float(np.nanmax(np.where(S.active, cond * (np.linalg.norm(S.pc, axis=1) + 1), 0), initial=0.0)) * 4 + 8
    for f in range(F):
        d = np.abs(sym6(got["Hpp"][f, :21]) - S.H6[f]) / ((n_f[f] + k) * EPS * absH[f] + 1e-300)
        db = np.abs(got["Hpp"][f, 21:] - S.b6[f]) / ((n_f[f] + k) * EPS * absb[f] + addb[f] + 1e-300)
        worst = max(worst, float(d.max()), float(db.max()))
    for j in np.flatnonzero(S.p_on):
        d = np.abs(sym3(got["Hll"][j, :6]) - S.Hll[j]) / ((n_p[j] + k) * EPS * absL[j] + 1e-300)
        db = np.abs(got["Hll"][j, 6:] - S.bl[j]) / ((n_p[j] + k) * EPS * absl[j] + addl[j] + 1e-300)
        worst = max(worst, float(d.max()), float(db.max()))
    # the inertial edges
    N = 15 * F
    bb = np.zeros(N)
    for c in range(F):
        cols = 15 * c + np.array(vm.PVR_MONO)
        bb[cols] = (n_f[c] + k) * EPS * absb[c] + addb[c]
    bH = np.zeros((N, N))
    G = len(S.inert)
    for g, ((e_, info, delta, blocks), (dee, dJs), kind) in enumerate(zip(S.inert, inertial_bounds(a, est), kinds(a))):
        m = len(e_)
        I = got["ie"][g]
        with np.errstate(all="ignore"):
            c2 = float(e_ @ (info @ e_))
            rho0, rho1_ = [float(v) for v in nm.huber(c2, delta)]
            rel_om = float(np.linalg.cond(info)) * (3 * 9 + 3 * 81) * EPS if kind == "pvr" else 4 * EPS
            dchi2 = float(2 * np.abs(e_) @ (np.abs(info) @ dee) + np.abs(e_) @ (np.abs(info) @ np.abs(e_)) * (rel_om + (m + 2) * EPS))
            drho1 = rho1_ * (dchi2 / (2 * max(c2, delta * delta - dchi2)) + 3 * EPS) if c2 + dchi2 > delta * delta else 0.0
        Jm = dense_edge(kind, blocks, m)
        Wm = rho1_ * info
        dW = np.abs(Wm) * rel_om + np.abs(info) * drho1
        dJ = dJs * (Jm != 0)
        dWJ = np.abs(Wm) @ dJ + dW @ np.abs(Jm) + (m + 2) * EPS * (np.abs(Wm) @ np.abs(Jm))
        dWe = np.abs(Wm) @ dee + dW @ np.abs(e_) + (m + 2) * EPS * (np.abs(Wm) @ np.abs(e_))
        WJg, Weg = I[IE_WJ:IE_WJ + 270].reshape(9, 30)[:m], I[IE_WE:IE_WE + m]
        worst = max(worst, float((np.abs(WJg - Wm @ Jm) / (dWJ + 1e-300))[Jm != 0].max(initial=0.0)), float((np.abs(Weg - Wm @ e_) / (dWe + 1e-300)).max()))
        # this edge's share of the bounds of H and b, scattered as the model scatters the blocks
        aJ, aWJ, aWe = np.abs(Jm), np.abs(Wm) @ np.abs(Jm), np.abs(Wm) @ np.abs(e_)
        tH = dJ.T @ aWJ + aJ.T @ dWJ + (m + G) * EPS * (aJ.T @ aWJ)
        tb = dJ.T @ aWe + aJ.T @ dWe + (m + G) * EPS * (aJ.T @ aWe)
        for base1, (k1, b1) in zip(slots_of(kind), blocks):
            c1 = vm.col_of(a, k1)
            if c1 < 0:
                continue
            n1 = b1.shape[1]
            bb[c1:c1 + n1] += tb[base1:base1 + n1]
            for base2, (k2, b2) in zip(slots_of(kind), blocks):
                c2_ = vm.col_of(a, k2)
                if c2_ >= 0:
                    bH[c1:c1 + n1, c2_:c2_ + b2.shape[1]] += tH[base1:base1 + n1, base2:base2 + b2.shape[1]]
    worst = max(worst, float((np.abs(got["bfull"] - S.bp) / (bb + 1e-300)).max()) if N else 0.0)
    return worst, k, bH + bH.T


# ---- layer 3 ---------------------------------------------------------------------------------------------------------------------------
def check_trial(got, S, lam, k, bH):
    """One trial at lambda, as tests/ba_checks.py's check_trial: the Schur term's entries are bounded on the scale of the MONO part of the
    diagonal (sum_j W Dinv W^T is at most the mono Hpp in the positive semi-definite order), the inertial entries by layer 2's bH; the
    solve answers perturbations of relative size tol / scale with 2 kappa, plus its own 3 n^2 EPS.  Returns the worst ratio, ok."""
    a = S.a
    ok, xp, xl = S.trial(lam)
    F, P = a["F"], len(S.Hll)
    N = 15 * F
    n_max = int(max(np.bincount(S.f[S.to_free], minlength=F).max(initial=0), 1))
    u = (n_max + k) * EPS
    on = np.flatnonzero(S.p_on)
    kap_l = np.array([np.linalg.cond(S.Hll[j] + lam * np.eye(3)) for j in on]) if len(on) else np.zeros(0)
    kl = float(kap_l.max()) if len(kap_l) else 1.0
    A = np.triu(S.Hs) + np.triu(S.Hs, 1).T
    G = np.tril(got["Hs"]) + np.tril(got["Hs"], -1).T
    scale_mono = float(np.abs(S.H6).max(initial=0.0)) + lam
    rel_term = 2 * kl * (u + 32 * EPS) + 2 * u
    tolA = (9 * rel_term + u) * scale_mono + bH + 4 * EPS * np.abs(A)
    worst = float((np.abs(G - A) / tolA).max())
    tolb = (9 * rel_term + u) * (float(np.abs(S.b6).max(initial=0.0)) + float(np.abs(S.bs).max())) + 1e-300
    worst = max(worst, float(np.abs(got["bs"] - S.bs).max() / tolb))
    if ok:
        kap = np.linalg.cond(A)
        rel = 2 * kap * (float((tolA / (np.abs(A).max())).max()) + 3 * N * N * EPS)
        xpn = np.abs(xp).max()
        worst = max(worst, float(np.abs(got["xp"] - xp).max() / (rel * xpn + 1e-300)))
        xln = np.abs(xl).max(initial=0.0)
        if len(on):
            worst = max(worst, float(np.abs(got["xl"][on] - xl[on]).max() / ((rel * kl + 2 * kl * u) * (xln + xpn) + 1e-300)))
        assert got["scal"][2] == 1.0
    else:
        assert got["scal"][2] == 0.0 and got["scal"][3] == DBL_MAX
    return worst, ok


# ---- layer 4 ---------------------------------------------------------------------------------------------------------------------------
def replay(run):
    """tests/ba_checks.py's replay in local mode: optimize(5), optimize(10)."""
    return bc.replay(run, 0, 0)


# ---- layer 5 ---------------------------------------------------------------------------------------------------------------------------
def not_finite(res):
    return not all(np.isfinite(t["tmp"]) and t["ok"] for t in res.trials) or not all(np.isfinite(l["chi2"]) for l in res.lin)


def clear(name):
    """As tests/ba_checks.py's clear: no stored chi2 within 2 sqrt(5.991) 9 G T_EST of 5.991, no depth within 1e-6 of zero, no rho within
    1e-3 of zero; the scene is not listed as unclear."""
    if name in UNCLEAR:
        return False
    sc, res = model(name)
    if not_finite(res):
        return False
    a = vm.arrays(sc)
    L0 = res.lin[0]
    _, _, _, Jp, Jl = vm.mono(a, L0["est"], L0["X"])
    G = max(float(np.abs(Jp[L0["active"]]).max(initial=0.0)), float(np.abs(Jl[L0["active"]]).max(initial=0.0)))
    for c in res.checks:
        ex = c["examined"]
        if np.any(np.abs(c["stored"][ex] - vm.TH) <= 2 * vm.TH ** 0.5 * 9 * G * T_EST) or np.any(np.abs(c["depth"][ex]) <= 1e-6):
            return False
    return all(abs(t["rho"]) > 1e-3 for t in res.trials)


def check_final(name, run):
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
    if not (np.array_equal(run.excluded, res.excluded) and np.array_equal(run.erased, res.erased)):
        bad.append("masks: %d %d against the model's %d %d" % (run.n_excluded, run.n_erased, res.n_excluded, res.n_erased))
    if (run.n_excluded, run.n_erased) != (int(run.excluded.sum()), int(run.erased.sum())):
        bad.append("the counts are not the masks'")
    d = max(float(np.abs(run.kf_state - res.states).max()), float(np.abs(run.point_estimate - res.X).max(initial=0.0)))
    if not d <= T_EST:
        bad.append("final states and points differ by %.3e, T = %.1e" % (d, T_EST))
    scale = 1 + float(np.abs(res.states[:, :3]).max())
    if np.abs(run.kf_Tcw.astype(np.float64) - res.kf_Tcw).max() > (T_EST + 2.0 ** -23 * 16) * scale or \
            np.abs(run.points.astype(np.float64) - res.points).max(initial=0.0) > T_EST + 2.0 ** -23 * 16:
        bad.append("the float outputs are not the estimates rounded")
    return bad


def check_layers(emu, name):
    """Layers 1 to 3 on the model's own estimates: at its first and last linearisation with the lambda it starts that optimize() with, and
    at its first rejected trial with that trial's lambda.  The stored error after the trial, accepted or not, must be the error at the
    TRIED estimates, and the verdict the model's."""
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
        got = emu.one_trial(sc, L["est"], L["X"], (~L["active"]).astype(np.uint8), L["rob"].astype(np.uint8), lam)
        w1, S = check_edges(name, got, L["est"], L["X"], L["active"], L["rob"])
        w2, k, bH = check_assembly(got, S, L["est"])
        w3, ok = check_trial(got, S, lam, k, bH)
        est_try = [nm.state_of_vec(v) for v in got["est_try"]]
        w4, _ = check_edges(name, dict(chi2=got["chi2_try"]), est_try, got["X_try"], L["active"], L["rob"], jac=False)
        if abs(got["scal"][0] - L["chi2"]) > M_REL * abs(L["chi2"]):         # the robust chi2 of the linearisation, at equal estimates
            w2 = max(w2, 2.0)
        if t:
            assert got["scal"][3] > L["chi2"] or not np.isfinite(got["scal"][3]), "the model rejects this trial"
        out.append((max(w1, w4), w2, w3))
    return out


def check_all(name, run):
    bad = replay(run) + check_final(name, run)
    assert not bad, (name, bad)


# ---- the measurement -------------------------------------------------------------------------------------------------------------------
SOLVERS = ("solve", "cholesky", "full")


def measure_spread(names, orders=ORDERS, seed=SEED):
    """The model's own spread under permuted edge orders and exchanged solvers -> (estimate spread, relative chi2 spread, unclear scenes)."""
    est_s = chi_s = 0.0
    unclear = []
    for name in names:
        sc, ref = model(name)
        if not_finite(ref):
            continue
        E = len(sc["edge_kf"])
        rng = np.random.RandomState([seed, list(vm.SCENES).index(name)])
        flips = False
        e_here = c_here = 0.0
        for k in range(orders):
            order = rng.permutation(E)
            for solver in SOLVERS:
                with np.errstate(all="ignore"):
                    r = vm.optimize(sc, order=order, solver=solver)
                if (len(r.trials) != len(ref.trials) or [t["accepted"] for t in r.trials] != [t["accepted"] for t in ref.trials] or
                        not np.array_equal(r.excluded, ref.excluded) or not np.array_equal(r.erased, ref.erased)):
                    flips = True
                    continue
                e_here = max(e_here, float(np.abs(r.states - ref.states).max()), float(np.abs(r.X - ref.X).max(initial=0.0)))
                c_here = max(c_here, max(abs(x["chi2"] - y["chi2"]) / abs(y["chi2"]) for x, y in zip(r.lin, ref.lin)))
        print("%-18s estimate spread %.3e  relative chi2 spread %.3e%s" % (name, e_here, c_here, "  UNCLEAR" if flips else ""))
        if flips:
            unclear.append(name)
        else:
            est_s, chi_s = max(est_s, e_here), max(chi_s, c_here)
    return est_s, chi_s, unclear


if __name__ == "__main__":
    e, c, u = measure_spread(list(vm.SCENES))
    print("estimate spread %.3e, relative chi2 spread %.3e, unclear %s (seed %d, %d orders x 3 solvers); recorded %.1e %.1e %s" %
          (e, c, u, SEED, ORDERS, EST_SPREAD, CHI2_REL_SPREAD, list(UNCLEAR)))
    sys.exit(0)
