"""The checks that hold an implementation of the pose-only optimisation to tests/poseopt_model.py, layer by layer, and the driver of the
host build (tests/emu/poseopt_emu.cpp).  tests/test_poseopt_emu.py runs them on the host build and on its six seeded mutations,
tests/test_gpu_poseopt.py on the device (layers 2, 4 and 5: what the trace tap shows).

Every bound of layers 1 to 3 is DERIVED: (number of rounding operations on the path) x u x (the model's sum of absolute terms), u = 2^-53,
or x cond for the solve; none is fitted to an observed difference.  T and M of layer 5 cannot be derived and are MEASURED ON THE MODEL
(measure_spread below), never on the code under test; DESIGN.md section 4 records the measurement."""
import ctypes
import math
import os

import numpy as np

import host_build
import poseopt_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
MUTATIONS = {"HUBER_B": 1, "NO_REEVAL": 2, "BREAK_ACTIVE": 3, "LAMBDA_ONCE": 4, "NO_RESTORE": 5, "SCALE": 6}

# Layer 5, measured on the model over every scene of pm.SCENES under 8 random edge orders (measure_spread):
# the largest spread of the final double pose (any entry of R or t) was 2.2e-9, the largest change of any edge's chi2 at a
# classification 6.5e-6, and no mask changed in the 256 runs.  The smallest margin |chi2 - th| of any scene is 6.8e-3.
POSE_SPREAD, CHI2_SPREAD = 2.2e-9, 6.5e-6
T_POSE, M_CHI2 = 4 * POSE_SPREAD, 4 * CHI2_SPREAD


class Run:
    """What one call gave: Tcw float32[4, 4], n_inliers, rounds, outlier uint8[n], and the trace (R, t, lin, trial as uvo.PoseTrace)."""

    def __init__(self, Tcw, n_inliers, rounds, outlier, trace):
        self.Tcw, self.n_inliers, self.rounds, self.outlier, self.trace = Tcw, n_inliers, rounds, outlier, trace


class Emu:
    """tests/emu/poseopt_emu.cpp, built on first use with the library's contract: no FMA contraction.  `mutation`: a key of MUTATIONS,
    compiled into a library of its own."""
    _libs = {}

    def __init__(self, uvo, mutation=None):
        assert mutation is None or mutation in MUTATIONS
        self.uvo = uvo
        if mutation not in Emu._libs:
            variant = (["-DPOSEOPT_MUT=%d" % MUTATIONS[mutation]], "_" + mutation.lower()) if mutation else ()
            L = ctypes.CDLL(host_build.build("poseopt_emu", *variant))
            vp, ci, cd = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
            L.emu_pose_from_T.argtypes = [vp, vp]
            L.emu_pose_to_T.argtypes = [vp, vp, vp]
            L.emu_pose_edge.argtypes = [vp, vp, vp, vp]
            L.emu_pose_linearise.argtypes = [vp, vp, vp, vp, ci, vp]
            L.emu_pose_trial.argtypes = [vp, cd, vp, vp, cd, vp, vp, vp, ci, vp, vp, vp]
            L.emu_pose_optimize.argtypes = [vp, ci, vp, vp, vp, vp, vp, vp, vp]
            L.emu_pose_optimize.restype = None
            assert L.emu_pose_mutation() == (MUTATIONS[mutation] if mutation else 0)
            Emu._libs[mutation] = L
        self.L = Emu._libs[mutation]

    @staticmethod
    def edges(p3d, p2d, w):
        return np.ascontiguousarray(np.concatenate([np.asarray(p3d, np.float32).reshape(-1, 3), np.asarray(p2d, np.float32).reshape(-1, 2),
                                                    np.asarray(w, np.float32).reshape(-1, 1)], 1))

    def pose_of(self, Tcw):
        qt = np.zeros(7)
        T = np.ascontiguousarray(Tcw, np.float32)
        self.L.emu_pose_from_T(T.ctypes.data, qt.ctypes.data)
        return qt

    def matrix_of(self, qt):
        T, R = np.zeros(16, np.float32), np.zeros(9)
        qt = np.ascontiguousarray(qt, np.float64)
        self.L.emu_pose_to_T(qt.ctypes.data, T.ctypes.data, R.ctypes.data)
        return T.reshape(4, 4), R.reshape(3, 3)

    def edge(self, qt, K, edge):
        out, qt, K, edge = np.zeros(17), np.ascontiguousarray(qt, np.float64), np.asarray(K, np.float32), np.ascontiguousarray(edge, np.float32)
        self.L.emu_pose_edge(qt.ctypes.data, K.ctypes.data, edge.ctypes.data, out.ctypes.data)
        return out

    def linearise(self, qt, K, edges, state):
        out, qt, K = np.zeros(28), np.ascontiguousarray(qt, np.float64), np.asarray(K, np.float32)
        state = np.ascontiguousarray(state, np.uint8)
        self.L.emu_pose_linearise(qt.ctypes.data, K.ctypes.data, edges.ctypes.data, state.ctypes.data, len(edges), out.ctypes.data)
        return out

    def trial(self, H21, lam, b, qt, cur, K, edges, state, dx_prev=None):
        dx = np.zeros(6) if dx_prev is None else np.array(dx_prev, np.float64)
        H21, b, qt = np.ascontiguousarray(H21, np.float64), np.ascontiguousarray(b, np.float64), np.ascontiguousarray(qt, np.float64)
        K, state, qo, out = np.asarray(K, np.float32), np.ascontiguousarray(state, np.uint8), np.zeros(7), np.zeros(3)
        ok = self.L.emu_pose_trial(H21.ctypes.data, lam, b.ctypes.data, qt.ctypes.data, cur, K.ctypes.data, edges.ctypes.data, state.ctypes.data, len(edges),
                                   dx.ctypes.data, qo.ctypes.data, out.ctypes.data)
        return bool(ok), dx, qo, out

    def optimize(self, sc):
        p3d, p2d, w, K, Tcw = sc
        e = self.edges(p3d, p2d, w)
        n = len(e)
        K, T = np.asarray(K, np.float32), np.ascontiguousarray(Tcw, np.float32)
        To, ni, nr, mask, tr = np.zeros(16, np.float32), ctypes.c_int32(), ctypes.c_int32(), np.zeros(n + 1, np.uint8), self.uvo.PoseTraceC()
        self.L.emu_pose_optimize(e.ctypes.data, n, K.ctypes.data, T.ctypes.data, To.ctypes.data, ctypes.byref(ni), ctypes.byref(nr), mask.ctypes.data,
                                 ctypes.byref(tr))
        return Run(To.reshape(4, 4), ni.value, nr.value, mask[:n].copy(), self.uvo.PoseTrace(tr))


def triu(H):
    return np.asarray(H)[np.triu_indices(6)]


_MODEL = {}


def model(name):
    """The model's run of a named scene: computed once, shared, never changed."""
    if name not in _MODEL:
        _MODEL[name] = (pm.make(name), pm.optimize(*pm.make(name)))
    return _MODEL[name]


# ---- layer 1: one edge ----------------------------------------------------------------------------------------------------------------
def edge_bounds(q, t, K, p3d, p2d, w):
    """The bounds of layer 1 for every edge at pose (q, t), as arrays, and the model's values they belong to.
    Derivation (first order in u; V = |p|_inf, |q_k| <= 1).  rotate(): a component of u = 2 (q x v) is two products and a difference,
    |.| <= 4 V after the exact doubling, error 8 u V; w u: 12 u V; v + w u (<= 5 V): 17 u V; a component of q x u is two products
    of error 12 u V each and a difference of magnitude <= 8 V: 32 u V; their sum (<= 13 V): 62 u V; + t: dp = u (75 V + |t|_inf) per
    coordinate.  x / z: relative 2 u + dp / |x| + dp / |z|; the projection fx * x / z + cx and the subtraction from obs add 3
    roundings on |obs| + |u| + |cx|:   de <= fx (dp / |z|) (1 + |x / z|) + 5 u (|obs| + fx |x / z| + |cx|).
    chi2 = w (e0^2 + e1^2): d chi2 <= 2 w (|e0| de0 + |e1| de1) + 5 u chi2.  rho: sqrt and two operations: d rho0 <= 2 delta d chi2 /
    (2 sqrt chi2) + 4 u |rho0| <= d chi2 + 4 u (|rho0| + delta^2); d rho1 <= rho1 (d chi2 / (2 chi2) + 3 u) on the outlier branch (taken
    as reached when chi2 + d chi2 > delta^2), 0 on the inlier branch.
    A Jacobian entry is a product / quotient of at most 6 factors in x, y, z: relative 8 u + 4 dp / |z| + 2 dp / min(|x|, |y|, |z|) --
    taken as 8 u + 6 dp / |z| on |J| + fx (the entries with 1 + ...), plus fx dp / |z| for the numerators that pass through zero."""
    ev = pm.edge_eval(q, t, K, p3d, p2d, w)
    J = pm.jacobian(ev, K)
    rho0, rho1 = pm.huber(ev["chi2"])
    fx, fy, cx, cy = [float(v) for v in K]
    x, y, z = ev["x"], ev["y"], ev["z"]
    p2d = np.asarray(p2d, np.float64)
    with np.errstate(all="ignore"):
        dp = U * (75 * np.abs(np.asarray(p3d, np.float64)).max(1) + float(np.abs(t).max()))
        de0 = fx * (dp / np.abs(z)) * (1 + np.abs(x / z)) + 5 * U * (np.abs(p2d[:, 0]) + fx * np.abs(x / z) + abs(cx))
        de1 = fy * (dp / np.abs(z)) * (1 + np.abs(y / z)) + 5 * U * (np.abs(p2d[:, 1]) + fy * np.abs(y / z) + abs(cy))
        c2 = ev["chi2"]
        dchi = 2 * ev["w"] * (np.abs(ev["e0"]) * de0 + np.abs(ev["e1"]) * de1) + 5 * U * c2
        drho0 = dchi + 4 * U * (np.abs(rho0) + pm.DSQR)
        drho1 = np.where(c2 + dchi > pm.DSQR, rho1 * (dchi / (2 * np.maximum(c2, pm.DSQR - dchi)) + 3 * U), 0.0)
        f = max(fx, fy)
        dJ = (8 * U + 6 * dp / np.abs(z))[:, None, None] * (np.abs(J) + f) + (f * dp / np.abs(z))[:, None, None]
    return dict(ev=ev, J=J, rho0=rho0, rho1=rho1, de0=de0, de1=de1, dchi=dchi, drho0=drho0, drho1=drho1, dJ=dJ)


def check_edges(emu, name, count=40):
    """e, chi2, rho[0..1] and the 2 x 6 Jacobian of single edges at the scene's start pose, within edge_bounds."""
    sc, _ = model(name)
    p3d, p2d, w, K, Tcw = sc
    q, t = pm.pose_of(Tcw)
    assert np.abs(emu.pose_of(Tcw) - np.concatenate([q, t])).max() <= 8 * U, "toSE3Quat"
    qt = np.concatenate([q, t])          # the model's pose in: the bounds are for equal inputs
    B = edge_bounds(q, t, K, p3d, p2d, w)
    ev, J = B["ev"], B["J"]
    E = Emu.edges(p3d, p2d, w)
    worst = 0.0
    for i in range(min(count, len(E))):
        got = emu.edge(qt, K, E[i])
        if not np.isfinite([ev["x"][i] / ev["z"][i], ev["y"][i] / ev["z"][i]]).all():
            continue
        assert abs(got[0] - ev["e0"][i]) <= B["de0"][i] and abs(got[1] - ev["e1"][i]) <= B["de1"][i], (name, i)
        assert abs(got[2] - ev["chi2"][i]) <= B["dchi"][i], (name, i)
        assert abs(got[3] - B["rho0"][i]) <= B["drho0"][i], (name, i)
        assert abs(got[4] - B["rho1"][i]) <= B["drho1"][i], (name, i)
        Jg = got[5:].reshape(2, 6)
        assert (np.abs(Jg - J[i]) <= B["dJ"][i]).all(), (name, i)
        worst = max(worst, float((np.abs(Jg - J[i]) / B["dJ"][i]).max()))
    return worst


# ---- layer 2: one linearisation -------------------------------------------------------------------------------------------------------
def lin_bounds(sc, q, t, active):
    """The bounds on H[21], b[6] and the robust chi2 of one linearisation against the model's, at the same pose over the same edges.
    Derivation.  Both sides add n terms in different orders: each order's result is within (n - 1) u sum|t| of the exact sum of its
    own terms (Higham, Accuracy and Stability, 4.2: any order), 2 (n - 1) u sum|t| together.  The terms themselves differ by what
    layer 1 allows their factors (edge_bounds) plus their own roundings:
        H_ab term = sum_r (J_ra wo) J_rb, wo = rho1 w:  sum_r [dJ_ra wo |J_rb| + |J_ra| wo dJ_rb + |J_ra| |J_rb| w drho1] + 4 u |term|
        b_a term  = sum_r J_ra r_r, r_r = -(w e_r) rho1:  dr_r = w (de_r rho1 + |e_r| drho1) + 2 u |r_r|;
                    sum_r [dJ_ra |r_r| + |J_ra| dr_r] + 2 u |term|
        chi2 term = rho0:  drho0
    summed over the active edges."""
    p3d, p2d, w, K, Tcw = sc
    idx = np.flatnonzero(active)
    B = edge_bounds(q, t, K, p3d, p2d, w)
    n = len(idx)
    with np.errstate(all="ignore"):
        J, dJ = np.abs(B["J"][idx]), B["dJ"][idx]
        wd, rho1, drho1 = B["ev"]["w"][idx], B["rho1"][idx], B["drho1"][idx]
        wo = (rho1 * wd)[:, None, None, None]
        tH = (J[:, :, :, None] * wo * J[:, :, None, :]).sum(1)                                  # [n, 6, 6]: sum_r |J_ra| wo |J_rb|
        eH = (dJ[:, :, :, None] * wo * J[:, :, None, :] + J[:, :, :, None] * wo * dJ[:, :, None, :] +
              J[:, :, :, None] * J[:, :, None, :] * (wd * drho1)[:, None, None, None]).sum(1) + 4 * U * tH
        e = np.abs(np.stack([B["ev"]["e0"][idx], B["ev"]["e1"][idx]], 1))                       # [n, 2]
        de = np.stack([B["de0"][idx], B["de1"][idx]], 1)
        r = wd[:, None] * e * rho1[:, None]
        dr = wd[:, None] * (de * rho1[:, None] + e * drho1[:, None]) + 2 * U * r
        tb = (J * r[:, :, None]).sum(1)                                                          # [n, 6]
        eb = (dJ * r[:, :, None] + J * dr[:, :, None]).sum(1) + 2 * U * tb
        tc, ec = np.abs(B["rho0"][idx]), B["drho0"][idx]
        c = 2 * max(n - 1, 0) * U
        bH = c * tH.sum(0) + eH.sum(0)
        return bH[np.triu_indices(6)], c * tb.sum(0) + eb.sum(0), float(c * tc.sum() + ec.sum())


def check_linearisation(name, sums, L=None):
    """sums: H[21] b[6] chi2 of the implementation's linearisation L of the model (default: the first: start pose, every edge active)."""
    sc, res = model(name)
    if L is None:
        L = res.lin[0]
    bH, bb, bc = lin_bounds(sc, L["q"], L["t"], L["active"])
    dH, db, dc = np.abs(sums[:21] - triu(L["H"])), np.abs(sums[21:27] - L["b"]), abs(sums[27] - L["chi2"])
    assert (dH <= bH).all(), (name, "H", dH / bH)
    assert (db <= bb).all(), (name, "b", db / bb)
    assert dc <= bc, (name, "chi2", dc, bc)


# ---- layer 3: one trial ---------------------------------------------------------------------------------------------------------------
def check_trial(emu, name, trial=0):
    """dx against numpy.linalg.solve, the updated pose, tmp, scale and rho, on the model's own H, b, lambda, pose and currentChi of a
    trial.
    Derivation.  Both solvers are backward stable: the computed x solves (A + dA) x = b with |dA| <= g |A|, g <= 3 n u x growth; n = 6,
    growth 1 for the LDL^T of a positive definite matrix and at most 2^(n - 1) = 32 for partial pivoting, so g <= 18 u and 576 u, and
    the forward errors add: |dx_emu - dx_np| <= cond(A) (18 + 576) u |x| in norm.
    The pose: exp and the product are 120 operations on |omega| <= |dx|, |t|, 1; sincos is good to 2^-51 = 4 u absolute, and dx's error
    enters with weight 1 (quaternion: 1/2; translation: 1 + |t|): |dpose| <= (1 + |t|) |ddx| + (120 + 8) u (1 + |t| + |dx|).
    scale = sum x (lambda x + b) + 1e-3: |dscale| <= sum |ddx| (2 lambda |x| + |b|) + 20 u sum |x| (lambda |x| + |b|).
    tmp: the layer-2 bound on a robust chi2 at the tried pose, plus what the pose's error moves it: the gradient of sum rho in the
    six tangent directions is -2 b' (b' of a linearisation at the tried pose, which the model computes), and a pose error dpose in
    (q, t) is a tangent error of at most 2 dpose in rotation and (1 + |t|) dpose in translation, within the 2 (1 + |t|) taken here:
    |dtmp| <= layer 2 + 2 |b'|_1 2 (1 + |t|) dpose.  rho = (cur - tmp) / scale with cur given: |drho| <= (|dtmp| + |rho| |dscale|) / |scale|."""
    sc, res = model(name)
    p3d, p2d, w, K, Tcw = sc
    tr = res.trials[trial]
    L = res.lin[tr["lin"]]
    qt0 = np.concatenate([tr["q0"], tr["t0"]])
    ok, dx, qt1, (tmp, scale, rho) = emu.trial(triu(L["H"]), tr["lam"], L["b"], qt0, tr["cur"], K, Emu.edges(p3d, p2d, w), (~L["active"]).astype(np.uint8))
    assert ok == tr["ok"] and ok
    ddx = tr["cond"] * (18 + 576) * U * float(np.linalg.norm(tr["dx"]))
    assert float(np.linalg.norm(dx - tr["dx"])) <= ddx, (name, dx - tr["dx"], ddx)
    tn = float(np.abs(tr["t0"]).max())
    dpose = (1 + tn) * ddx + 128 * U * (1 + tn + float(np.abs(tr["dx"]).max()))
    assert np.abs(qt1 - np.concatenate([tr["q"], tr["t"]])).max() <= dpose, (name, qt1 - np.concatenate([tr["q"], tr["t"]]), dpose)
    x, b, lam = np.abs(tr["dx"]), np.abs(L["b"]), tr["lam"]
    dscale = float((ddx * (2 * lam * x + b)).sum() + 20 * U * (x * (lam * x + b)).sum()) + 2 * U
    assert abs(scale - tr["scale"]) <= dscale, (name, scale - tr["scale"], dscale)
    b1 = pm.linearise(tr["q"], tr["t"], K, p3d, p2d, w, L["active"])["b"]
    dtmp = lin_bounds(sc, tr["q"], tr["t"], L["active"])[2] + 2 * float(np.abs(b1).sum()) * 2 * (1 + tn) * dpose
    assert abs(tmp - tr["tmp"]) <= dtmp, (name, tmp - tr["tmp"], dtmp)
    drho = (dtmp + abs(tr["rho"]) * dscale) / abs(tr["scale"])
    assert abs(rho - tr["rho"]) <= drho * (1 + 1e-6), (name, rho - tr["rho"], drho)
    return ddx, drho


# ---- layer 4: the Levenberg trajectory ------------------------------------------------------------------------------------------------
def chi2_bound(name, q, t, active):
    return lin_bounds(model(name)[0], q, t, active)[2]


_PREFIX = {}


def compared_prefix(name):
    if name not in _PREFIX:
        _PREFIX[name] = _compared_prefix(name)
    return _PREFIX[name]


def _compared_prefix(name):
    """The number of leading trials whose model margin |cur - tmp| exceeds the layer-2 bound on the two robust chi2 it is the
    difference of: that at the linearisation's pose plus that at the tried pose."""
    _, res = model(name)
    k = 0
    for tr in res.trials:
        L = res.lin[tr["lin"]]
        if not (tr["ok"] and math.isfinite(tr["margin"])):
            break
        bound = chi2_bound(name, L["q"], L["t"], L["active"]) + chi2_bound(name, tr["q"], tr["t"], L["active"])
        if not tr["margin"] > bound:
            break
        k += 1
    return k


def first_iteration_trials(res):
    return sum(1 for tr in res.trials if tr["lin"] == 0)


# lambda over the compared prefix.  It moves by factors that are exact (ni: 2, 4, ...; the clamps 1/3 and 2/3) or, between the clamps,
# 1 - (2 rho - 1)^3, whose derivative in rho is at most 6; rho's own error is that of (cur - tmp) / scale, layers 2 and 3, of the order
# cond x 600 u <= 1e-9 for cond <= 1e4.  1e-6 relative leaves three orders of magnitude and is six below what a wrong rule changes.
LAMBDA_RTOL = 1e-6


def not_finite(res):
    """A scene whose sums are not finite from the first linearisation on: no margin exists, and nothing is decided by one either -- every
    trial fails its solve and is rejected by class.  Its whole trajectory is compared, by class."""
    return len(res.lin) > 0 and not math.isfinite(res.lin[0]["chi2"])


def check_trajectory(name, run):
    _, res = model(name)
    k = compared_prefix(name)
    tr = run.trace.trial
    if not_finite(res):
        assert len(tr) == len(res.trials) and len(run.trace.lin) == len(res.lin), (name, len(tr), len(res.trials))
        for i, m in enumerate(res.trials):
            assert (int(tr["lin"][i]), bool(tr["ok"][i]), bool(tr["accepted"][i])) == (m["lin"], m["ok"], m["accepted"]), (name, i)
            assert same_class(tr["lambda"][i], m["lam"]) and same_class(tr["cur"][i], m["cur"]) and same_class(tr["tmp"][i], m["tmp"]), (name, i)
        return len(tr)
    assert len(tr) >= min(k, len(res.trials)), (name, len(tr), k)
    for i in range(k):
        m = res.trials[i]
        assert int(tr["lin"][i]) == m["lin"], (name, i, "linearisation index")
        assert bool(tr["ok"][i]) == m["ok"] and bool(tr["accepted"][i]) == m["accepted"], (name, i, "decision", tr[i], m["rho"])
        assert abs(tr["lambda"][i] - m["lam"]) <= LAMBDA_RTOL * m["lam"], (name, i, "lambda", tr["lambda"][i], m["lam"])
    if len(tr) and len(res.trials):
        # the trace's own figures: currentChi of a linearisation's first trial is that linearisation's robust chi2, and at the start
        # pose, where both sides sum the same edges at the same pose, it is the model's within the layer-2 bound
        first = [i for i in range(len(tr)) if i == 0 or tr["lin"][i] != tr["lin"][i - 1]]
        assert all(tr["cur"][i] == run.trace.lin["chi2"][tr["lin"][i]] for i in first), (name, "cur")
        L0 = res.lin[0]
        assert abs(tr["cur"][0] - res.trials[0]["cur"]) <= chi2_bound(name, L0["q"], L0["t"], L0["active"]), (name, "cur of the first trial")
    if k:
        li = run.trace.lin
        last = res.trials[k - 1]["lin"]
        for j in range(last + 1):
            assert (int(li["round"][j]), int(li["iteration"][j])) == (res.lin[j]["round"], res.lin[j]["iteration"]), (name, j)
    return k


# ---- layer 5: results -----------------------------------------------------------------------------------------------------------------
def thin(name):
    """Whether the scene's smallest model margin |chi2 - th| is within M: its masks are then not compared."""
    _, res = model(name)
    return not pm.min_class_margin(res) > M_CHI2


def same_class(a, b):
    """Non-finite values compare by class (NaN, +inf, -inf), finite ones by value."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return bool((np.isnan(a) == np.isnan(b)).all() and (np.isposinf(a) == np.isposinf(b)).all() and (np.isneginf(a) == np.isneginf(b)).all())


def check_result(name, run):
    _, res = model(name)
    assert run.rounds == res.rounds, (name, run.rounds, res.rounds)
    if not thin(name):
        assert run.outlier.tobytes() == res.outlier.tobytes(), (name, np.flatnonzero(run.outlier != res.outlier))
        assert run.n_inliers == res.n_inliers, (name, run.n_inliers, res.n_inliers)
    got = np.concatenate([run.trace.R.reshape(-1), run.trace.t])
    want = np.concatenate([res.R.reshape(-1), res.t])
    assert same_class(got, want), name
    f = np.isfinite(want)
    assert np.abs(got[f] - want[f]).max() <= T_POSE if f.any() else True, (name, np.abs(got[f] - want[f]).max())
    # the float pose is the double one rounded: at most one float ulp apart where the doubles straddle a rounding boundary
    Tm = res.Tcw.astype(np.float64)
    assert same_class(run.Tcw, Tm)
    fin = np.isfinite(Tm)
    assert (np.abs(run.Tcw.astype(np.float64) - Tm)[fin] <= np.spacing(np.abs(res.Tcw[fin])).astype(np.float64) + T_POSE).all(), name


def check_all(name, run, sums0=None):
    """Layers 2 (when the first linearisation is given), 4 and 5 on one run of a named scene."""
    _, res = model(name)
    if sums0 is not None and len(res.lin):
        check_linearisation(name, sums0)
    k = check_trajectory(name, run)
    check_result(name, run)
    return k


def first_sums(run):
    li = run.trace.lin
    return np.concatenate([li["H"][0], li["b"][0], [li["chi2"][0]]]) if len(li) else None


# ---- measuring T and M on the model ---------------------------------------------------------------------------------------------------
def measure_spread(names, orders=8, seed=2024):
    """The model on each scene under `orders` random permutations of the edge order -> (largest pose spread, largest change of any
    edge's chi2 at a classification, mask changes)."""
    g = np.random.default_rng(seed)
    pose, chi, flips = 0.0, 0.0, 0
    for name in names:
        sc, base = model(name)
        n = len(sc[0])
        for _ in range(orders):
            r = pm.optimize(*sc, order=g.permutation(n))
            a, b = np.concatenate([r.R.reshape(-1), r.t]), np.concatenate([base.R.reshape(-1), base.t])
            f = np.isfinite(b)
            if f.any():
                pose = max(pose, float(np.abs(a[f] - b[f]).max()))
            for ca, cb in zip(r.class_chi2, base.class_chi2):
                f = np.isfinite(cb) & np.isfinite(ca)
                if f.any():
                    chi = max(chi, float(np.abs(ca[f] - cb[f]).max()))
            flips += int((r.outlier != base.outlier).sum())
    return pose, chi, flips
