"""The two IMU overloads of Optimizer::PoseOptimization restated in numpy from the reference's sources -- src/Optimizer.cc:319-777 (the
frame form) and :779-1103 (the key-frame form), src/IMU/g2otypes.{h,cpp} (the edges), NavState.cpp:71-123 (the increments), so3.cpp
(exp, log, JacobianR, JacobianRInv), FrameKTL.cc:160-181 (UpdatePoseFromNS) and, of g2o, optimization_algorithm_levenberg.cpp,
sparse_optimizer.cpp, base_{unary,binary,multi}_edge.hpp, robust_kernel_impl.cpp (Huber), sparse_optimizer.h:153-159 with
block_solver.hpp:490 (computeMarginals on _Hpp as the last buildSystem left it) -- not from csrc/navopt_core.hpp.
Where the library departs, the model keeps the reference: sums over edges are SERIAL in edge order (np.cumsum), every system goes to
numpy.linalg.solve / inv, sin, cos and atan are math's.  A NavState is P, V, a unit quaternion (x y z w), the biases and delta biases.

Two defects of the reference are stated, not reproduced: the frame form's spinv.block(0,1) is read as the joint
15 x 15 block of inv(H); the depth edge's information is a scalar the scene gives.

Eigen is recalled as in tests/poseopt_model.py [EIGEN-RECALL], whose quaternion helpers this file uses."""
import copy
import math

import numpy as np

import poseopt_model as pm

KEYFRAME, FRAME = 0, 1
CHI2 = np.float32(5.991)                                   # const float chi2Mono[4] = {5.991, ...}
F32 = lambda x: float(np.float32(math.sqrt(x)))            # const float th = sqrt(x); setDelta(th)
D_PRIOR, D_IMU, D_BIAS, D_DEPTH, D_MONO = F32(30.5779), F32(21.666), F32(16.812), F32(16.812), F32(5.991)
DBL_MAX = float(np.finfo(np.float64).max)
K_DEFAULT = (458.654, 457.296, 367.215, 248.375)
STATE_KEYS = ("P", "V", "q", "bg", "ba", "dbg", "dba")


def state(P=(0, 0, 0), V=(0, 0, 0), q=(0, 0, 0, 1), bg=(0, 0, 0), ba=(0, 0, 0), dbg=(0, 0, 0), dba=(0, 0, 0)):
    return dict(P=np.array(P, np.float64), V=np.array(V, np.float64), q=np.array(q, np.float64), bg=np.array(bg, np.float64), ba=np.array(ba, np.float64),
                dbg=np.array(dbg, np.float64), dba=np.array(dba, np.float64))


def state_vec(s):
    return np.concatenate([s[k] for k in STATE_KEYS])


def state_of_vec(v):
    v = np.asarray(v, np.float64)
    return dict(P=v[0:3].copy(), V=v[3:6].copy(), q=v[6:10].copy(), bg=v[10:13].copy(), ba=v[13:16].copy(), dbg=v[16:19].copy(), dba=v[19:22].copy())


# ---- so3.cpp ---------------------------------------------------------------------------------------------------------------------------
def hat(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def qnorm(q):
    q = np.asarray(q, np.float64)
    with np.errstate(all="ignore"):
        return q / math.sqrt(float(q @ q)) if np.isfinite(q).all() else q * np.nan


def qmul(a, b):
    w = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]
    x = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1]
    y = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2]
    z = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0]
    return qnorm([x, y, z, w])


def qinv(q):
    return qnorm([-q[0], -q[1], -q[2], q[3]])


def q_of_matrix(R):
    return qnorm(pm.quat_of(np.asarray(R, np.float64).reshape(3, 3)))


def so3_exp(om):
    om = np.asarray(om, np.float64)
    theta = math.sqrt(float(om @ om)) if np.isfinite(om).all() else float("nan")
    if not math.isfinite(theta):
        return np.full(4, np.nan)
    half = 0.5 * theta
    if theta < 1e-10:
        imag = 0.5 - 0.0208333 * theta * theta + 0.000260417 * theta ** 4
    else:
        imag = math.sin(half) / theta
    return qnorm([imag * om[0], imag * om[1], imag * om[2], math.cos(half)])


def so3_log(q):
    if not np.isfinite(q).all():
        return np.full(3, np.nan)
    n = math.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2])
    w = q[3]
    if n < 1e-10:
        f = 2.0 / w - 2.0 * (n * n) / (w * w * w)
    else:
        f = 2.0 * math.atan(n / w) / n if w != 0 else math.pi / n     # the fabs(w) < SMALL_EPS branch is overwritten by this line
    return f * np.asarray(q[:3])


def so3_jr(w):
    w = np.asarray(w, np.float64)
    theta = math.sqrt(float(w @ w))
    if not theta >= 0.00001:
        return np.eye(3) if theta < 0.00001 else np.full((3, 3), np.nan)
    K = hat(w / theta)
    return np.eye(3) - (1 - math.cos(theta)) / theta * K + (1 - math.sin(theta) / theta) * K @ K


def so3_jrinv(w):
    w = np.asarray(w, np.float64)
    theta = math.sqrt(float(w @ w)) if np.isfinite(w).all() else float("nan")
    if not theta >= 0.00001:
        return np.eye(3) if theta < 0.00001 else np.full((3, 3), np.nan)
    K = hat(w / theta)
    return np.eye(3) + 0.5 * hat(w) + (1.0 - (1.0 + math.cos(theta)) * theta / (2.0 * math.sin(theta))) * K @ K


def rot(q):
    return pm.rotation_of(q)


# ---- the scene -------------------------------------------------------------------------------------------------------------------------
def nd_of(sc):
    return 30 if sc["form"] == FRAME else 15


def n_edges(sc):
    """optimizer.edges().size(): every edge of the graph."""
    nl = len(sc["edges_last"]) if sc["form"] == FRAME else 0
    return len(sc["edges"]) + nl + 2 + (1 if sc["form"] == FRAME else 0) + (1 if sc["has_depth"] else 0)


# ---- EdgeNavStatePVRPointXYZOnlyPose ------------------------------------------------------------------------------------------------------
def reproj(s, sc, edges):
    """computeError, chi2 and the 2 x 9 Jacobian of every edge of one frame at state s -> dict of arrays."""
    e = np.asarray(edges, np.float32).reshape(-1, 6).astype(np.float64)
    fx, fy, cx, cy = [float(v) for v in sc["K"]]
    Rcb = np.asarray(sc["Rbc"], np.float64).reshape(3, 3).T
    Rwb = rot(s["q"])
    n = len(e)
    with np.errstate(all="ignore"):
        aux = (e[:, :3] - s["P"]) @ (Rcb @ Rwb.T).T
        pc = aux - Rcb @ np.asarray(sc["Pbc"], np.float64)
        x, y, z = pc[:, 0], pc[:, 1], pc[:, 2]
        e0 = e[:, 3] - ((x / z) * fx + cx)
        e1 = e[:, 4] - ((y / z) * fy + cy)
        w = e[:, 5]
        chi2 = e0 * (w * e0 + 0.0 * e1) + e1 * (0.0 * e0 + w * e1)
        J = np.zeros((n, 2, 9))
        for i in range(n):
            Maux = np.array([[fx, 0.0, -x[i] / z[i] * fx], [0.0, fy, -y[i] / z[i] * fy]])
            Jpi = Maux / z[i]
            J[i, :, 0:3] = -Jpi @ (-Rcb)
            J[i, :, 6:9] = -Jpi @ (hat(aux[i]) @ Rcb)
    return dict(x=x, y=y, z=z, e0=e0, e1=e1, w=w, chi2=chi2, J=J, aux=aux)


def huber(e, delta, robust=True):
    e = np.asarray(e, np.float64)
    dsqr = delta * delta
    with np.errstate(all="ignore"):
        sq = np.sqrt(e)
        out = ~(e <= dsqr) if robust else np.zeros(e.shape, bool)
        return np.where(out, 2.0 * sq * delta - dsqr, e), np.where(out, delta / sq, 1.0)


# ---- the single edges -> (name, error, information, {column: Jacobian block}, delta) ------------------------------------------------------
def corrected(d, Jg, Ja, b):
    return np.asarray(d, np.float64) + M3(Jg) @ b["dbg"] + M3(Ja) @ b["dba"]


def M3(a):
    return np.asarray(a, np.float64).reshape(3, 3)


COLS = dict(cur_pvr=0, cur_bias=9, last_pvr=15, last_bias=24)


def edge_imu(est, sc):
    """EdgeNavStatePVR: vertex 0 the last (key) frame's PVR, 1 the current frame's, 2 the last's bias."""
    si, sj = est[1], est[0]
    dT = float(sc["dT"])
    dT2 = dT * dT
    g = np.asarray(sc["gw"], np.float64)
    RiT = qinv(si["q"])
    u = sj["P"] - si["P"] - si["V"] * dT - 0.5 * g * dT2
    v = sj["V"] - si["V"] - g * dT
    rP = pm.rotate(RiT, u) - corrected(sc["dP"], sc["JPg"], sc["JPa"], si)
    rV = pm.rotate(RiT, v) - corrected(sc["dV"], sc["JVg"], sc["JVa"], si)
    jb = M3(sc["JRg"]) @ si["dbg"]
    rR = qmul(qmul(qinv(qmul(q_of_matrix(sc["dR"]), so3_exp(jb))), RiT), sj["q"])
    rPhi = so3_log(rR)
    e = np.concatenate([rP, rV, rPhi])
    Ri, Rj = rot(si["q"]), rot(sj["q"])
    Ji = so3_jrinv(rPhi)
    Jj = np.zeros((9, 9))
    Jj[0:3, 0:3], Jj[3:6, 3:6], Jj[6:9, 6:9] = Ri.T @ Rj, Ri.T, Ji
    J = {COLS["cur_pvr"]: Jj}
    if sc["form"] == FRAME:
        A = np.zeros((9, 9))
        A[0:3, 0:3], A[0:3, 3:6], A[0:3, 6:9] = -np.eye(3), -Ri.T * dT, hat(Ri.T @ u)
        A[3:6, 3:6], A[3:6, 6:9] = -Ri.T, hat(Ri.T @ v)
        A[6:9, 6:9] = -Ji @ Rj.T @ Ri
        B = np.zeros((9, 6))
        B[0:3, 0:3], B[0:3, 3:6], B[3:6, 0:3], B[3:6, 3:6] = -M3(sc["JPg"]), -M3(sc["JPa"]), -M3(sc["JVg"]), -M3(sc["JVa"])
        B[6:9, 0:3] = -Ji @ rot(qinv(so3_exp(rPhi))) @ so3_jr(jb) @ M3(sc["JRg"])
        J[COLS["last_pvr"]], J[COLS["last_bias"]] = A, B
    with np.errstate(all="ignore"):
        info = np.linalg.inv(np.asarray(sc["cov"], np.float64).reshape(9, 9))
    return "imu", e, info, J, D_IMU


def edge_bias(est, sc):
    si, sj = est[1], est[0]
    e = np.concatenate([(sj["bg"] + sj["dbg"]) - (si["bg"] + si["dbg"]), (sj["ba"] + sj["dba"]) - (si["ba"] + si["dba"])])
    info = np.eye(6)
    info[:3, :3], info[3:, 3:] = np.eye(3) / sc["gyr_rw2"], np.eye(3) / sc["acc_rw2"]
    info = info / sc["dT"]
    J = {COLS["cur_bias"]: np.eye(6)}
    if sc["form"] == FRAME:
        J[COLS["last_bias"]] = -np.eye(6)
    return "bias", e, info, J, D_BIAS


def edge_prior(est, sc):
    s, pr = est[1], sc["prior"]
    e = np.concatenate([pr["P"] - s["P"], pr["V"] - s["V"], so3_log(qmul(qinv(qnorm(pr["q"])), s["q"])), (pr["bg"] + pr["dbg"]) - (s["bg"] + s["dbg"]),
                        (pr["ba"] + pr["dba"]) - (s["ba"] + s["dba"])])
    A = np.zeros((15, 9))
    A[0:3, 0:3], A[3:6, 3:6], A[6:9, 6:9] = -rot(s["q"]), -np.eye(3), so3_jrinv(e[6:9])
    B = np.zeros((15, 6))
    B[9:12, 0:3], B[12:15, 3:6] = -np.eye(3), -np.eye(3)
    return "prior", e, np.asarray(sc["prior_info"], np.float64).reshape(15, 15), {COLS["last_pvr"]: A, COLS["last_bias"]: B}, D_PRIOR


def edge_depth(est, sc):
    """EdgeNavStateDepthProjected, literally: gravity (0, 0, 9.81), dT2 * Gravity without the 1/2; key-frame form: vertices (key frame,
    frame, key frame's bias); frame form: (CURRENT frame, last frame, last frame's bias)."""
    cur_first = sc["form"] == FRAME
    s0, s1, sb = (est[0], est[1], est[1]) if cur_first else (est[1], est[0], est[1])
    dT = float(sc["dT"])
    dT2 = dT * dT
    proj = sc["shi"] * (sc["depth_meas"] - s0["P"][2]) + s0["P"][2]
    r1 = proj - s1["P"][2]
    R0 = rot(s0["q"])
    c = corrected(sc["dP"], sc["JPg"], sc["JPa"], sb)
    kf = s0["P"] + dT * s0["V"] + dT2 * np.array([0.0, 0.0, 9.81]) + R0 @ c
    r2 = proj - kf[2]
    e = np.array([r1 + r2])
    e3 = np.array([0.0, 0.0, 1.0])
    J0 = np.zeros((1, 9))
    J0[0, 2], J0[0, 5] = 2 * (1 - sc["shi"]) - 1, -dT
    J0[0, 6:9] = hat(R0 @ c) @ e3
    J1 = np.zeros((1, 9))
    J1[0, 2] = -1
    J2 = np.zeros((1, 6))
    J2[0, 0:3], J2[0, 3:6] = (-R0 @ M3(sc["JPg"])) @ e3, (-R0 @ M3(sc["JPa"])) @ e3
    if cur_first:
        J = {COLS["cur_pvr"]: J0, COLS["last_pvr"]: J1, COLS["last_bias"]: J2}
    else:
        J = {COLS["cur_pvr"]: J1}          # the key frame's vertices are fixed
    return "depth", e, np.array([[float(sc["depth_info"])]]), J, D_DEPTH


def single_edges(est, sc):
    """In the order they were added to the graph."""
    out = []
    if sc["form"] == FRAME:
        out.append(edge_prior(est, sc))
    out += [edge_imu(est, sc), edge_bias(est, sc)]
    if sc["has_depth"]:
        out.append(edge_depth(est, sc))
    return out


# ---- one linearisation ---------------------------------------------------------------------------------------------------------------
def _serial(terms):
    return np.cumsum(terms, axis=0)[-1] if len(terms) else np.zeros(terms.shape[1:])


def frames_of(sc):
    return [(0, sc["edges"])] + ([(1, sc["edges_last"])] if sc["form"] == FRAME else [])


def linearise(est, sc, active, robust):
    """computeActiveErrors, activeRobustChi2, buildSystem.  active: per frame a bool array.  -> dict H [nd, nd], b, chi2, absH, absb, abschi2,
    ev (per frame), singles."""
    nd = nd_of(sc)
    H, b, aH, ab = np.zeros((nd, nd)), np.zeros(nd), np.zeros((nd, nd)), np.zeros(nd)
    chi, achi = 0.0, 0.0
    singles = single_edges(est, sc)
    with np.errstate(all="ignore"):
        for name, e, info, J, delta in singles:
            c = float(e @ (info @ e))
            rho0, rho1 = [float(v) for v in huber(c, delta)]
            chi, achi = chi + rho0, achi + abs(rho0)
            Jf = np.zeros((len(e), nd))
            for col, blk in J.items():
                Jf[:, col:col + blk.shape[1]] = blk
            H += Jf.T @ (rho1 * info) @ Jf
            b += Jf.T @ (rho1 * (-info @ e))
            aH += np.abs(Jf).T @ np.abs(rho1 * info) @ np.abs(Jf)
            ab += np.abs(Jf).T @ (np.abs(rho1 * info) @ np.abs(e))
        evs = []
        for f, edges in frames_of(sc):
            ev = reproj(est[f], sc, edges)
            evs.append(ev)
            idx = np.flatnonzero(active[f])
            rho0, rho1 = huber(ev["chi2"][idx], D_MONO, robust)
            J = ev["J"][idx]
            wo = rho1 * ev["w"][idx]
            r0 = -(ev["w"][idx] * ev["e0"][idx]) * rho1
            r1 = -(ev["w"][idx] * ev["e1"][idx]) * rho1
            Ht = (J[:, 0, :, None] * wo[:, None, None]) * J[:, 0, None, :] + (J[:, 1, :, None] * wo[:, None, None]) * J[:, 1, None, :]
            bt = J[:, 0, :] * r0[:, None] + J[:, 1, :] * r1[:, None]
            c0 = 15 * f
            H[c0:c0 + 9, c0:c0 + 9] += _serial(Ht)
            b[c0:c0 + 9] += _serial(bt)
            aH[c0:c0 + 9, c0:c0 + 9] += np.abs(Ht).sum(0)
            ab[c0:c0 + 9] += np.abs(bt).sum(0)
            if len(idx):
                chi, achi = chi + float(_serial(rho0)), achi + float(np.abs(rho0).sum())
    return dict(H=H, b=b, chi2=chi, absH=aH, absb=ab, abschi2=achi, ev=evs, singles=singles)


def robust_chi2(est, sc, active, robust):
    chi, achi, evs = 0.0, 0.0, []
    with np.errstate(all="ignore"):
        for name, e, info, J, delta in single_edges(est, sc):
            rho0 = float(huber(float(e @ (info @ e)), delta)[0])
            chi, achi = chi + rho0, achi + abs(rho0)
        for f, edges in frames_of(sc):
            ev = reproj(est[f], sc, edges)
            evs.append(ev)
            idx = np.flatnonzero(active[f])
            if len(idx):
                rho0 = huber(ev["chi2"][idx], D_MONO, robust)[0]
                chi, achi = chi + float(_serial(rho0)), achi + float(np.abs(rho0).sum())
    return chi, evs, achi


def solve(H, lam, b):
    """Cholmod on H + lambda I: fails unless positive definite."""
    A = H + lam * np.eye(len(b))
    if not np.isfinite(A).all() or not np.isfinite(b).all():
        return False, None, float("inf")
    ev = np.linalg.eigvalsh(A)
    if not (ev > 0).all():
        return False, None, float("inf")
    return True, np.linalg.solve(A, b), float(ev.max() / ev.min())


def oplus(s, dpvr, dbias):
    """IncSmallPVR, IncSmallBias: P += R dP with the rotation BEFORE the update, then R = R exp(dPhi)."""
    s = copy.deepcopy(s)
    with np.errstate(all="ignore"):
        R = rot(s["q"])
        s["P"] = s["P"] + R @ dpvr[0:3]
        s["V"] = s["V"] + dpvr[3:6]
        s["q"] = qmul(s["q"], so3_exp(dpvr[6:9]))
        s["dbg"] = s["dbg"] + dbias[0:3]
        s["dba"] = s["dba"] + dbias[3:6]
    return s


def oplus_all(est, sc, x):
    out = [oplus(est[0], x[0:9], x[9:15]), est[1]]
    if sc["form"] == FRAME:
        out[1] = oplus(est[1], x[15:24], x[24:30])
    return out


def pose_from_ns(s, sc):
    """UpdatePoseFromNS: CV_32F matrices."""
    Rwb, Pwb = rot(s["q"]).astype(np.float32), s["P"].astype(np.float32)
    Rbc, Pbc = M3(sc["Rbc"]).astype(np.float32), np.asarray(sc["Pbc"], np.float32)
    with np.errstate(all="ignore"):
        Rcw = (Rwb.astype(np.float64) @ Rbc.astype(np.float64)).astype(np.float32).T
        Pwc = (Rwb.astype(np.float64) @ Pbc.astype(np.float64) + Pwb).astype(np.float32)
        Pcw = -(Rcw.astype(np.float64) @ Pwc.astype(np.float64)).astype(np.float32)
    T = np.eye(4, dtype=np.float32)
    T[:3, :3], T[:3, 3] = Rcw, Pcw
    return T


def marginals(H, sc):
    """computeMarginals on H as the last buildSystem left it -> (the 15 x 15 block of the current frame, mMargCovInv, ok)."""
    with np.errstate(all="ignore"):
        try:
            if not np.isfinite(H).all() or not (np.linalg.eigvalsh(H) > 0).all():
                raise np.linalg.LinAlgError
            cov = np.linalg.inv(H)[:15, :15]
            if sc["form"] == FRAME:
                inv = np.linalg.inv(cov)                       # :752-757, spinv.block(0,1) read as the joint block
            else:
                inv = np.zeros((15, 15))                       # :1083-1085
                inv[:9, :9], inv[9:, 9:] = np.linalg.inv(cov[:9, :9]), np.linalg.inv(cov[9:, 9:])
            return cov, inv, True
        except np.linalg.LinAlgError:
            return np.full((15, 15), np.nan), np.full((15, 15), np.nan), False


class Result:
    pass


def optimize(sc, order=None):
    """The call.  order: per frame a permutation of its edges -- the sums then run in that order; every output is in the scene's order."""
    if order is not None:
        sc2 = dict(sc)
        sc2["edges"] = np.asarray(sc["edges"])[order[0]]
        if sc["form"] == FRAME:
            sc2["edges_last"] = np.asarray(sc["edges_last"])[order[1]]
        r = optimize(sc2)
        inv = [np.argsort(o) for o in order]
        r.outlier = [m[inv[f]] for f, m in enumerate(r.outlier)]
        r.class_chi2 = [[c[inv[f]] for f, c in enumerate(cs)] for cs in r.class_chi2]
        r.flags = [[c[inv[f]] for f, c in enumerate(cs)] for cs in r.flags]
        return r
    fr = frames_of(sc)
    n = len(sc["edges"])
    nd = nd_of(sc)
    start = [copy.deepcopy(sc["cur"]), copy.deepcopy(sc["last"])]
    for s in start:
        s["q"] = qnorm(s["q"])
    est = copy.deepcopy(start)
    level = [np.zeros(len(e), bool) for _, e in fr]
    flag = [np.zeros(len(e), bool) for _, e in fr]
    stored = [np.zeros(len(e)) for _, e in fr]
    res = Result()
    res.lin, res.trials, res.class_chi2, res.flags = [], [], [], []
    n_bad, lam, rounds = 0, 0.0, 0
    H_last = None
    if n >= (4 if sc["form"] == FRAME else 3):
        for rnd in range(4):
            rounds = rnd + 1
            robust = rnd < 3                                     # setRobustKernel(0) when it == 2, after that round's classification
            est = copy.deepcopy(start)                           # Reset estimates
            active = [~l for l in level]
            ni, stalled, x = 2.0, 0, np.zeros(nd)
            for it in range(10):
                L = linearise(est, sc, active, robust)
                H_last = L["H"]
                for f in range(len(fr)):
                    stored[f][active[f]] = L["ev"][f]["chi2"][active[f]]
                cur = ini = L["chi2"]
                if it == 0:
                    mx = 0.0
                    for j in range(nd):
                        h = abs(L["H"][j, j])
                        mx = mx if h < mx else h
                    lam, ni, stalled = 1e-5 * mx, 2.0, 0
                li = len(res.lin)
                res.lin.append(dict(round=rnd, iteration=it, H=L["H"], b=L["b"], chi2=L["chi2"], absH=L["absH"], absb=L["absb"], abschi2=L["abschi2"],
                                    est=copy.deepcopy(est), active=[a.copy() for a in active], robust=robust))
                rho, qmax = 0.0, 0
                while True:
                    backup = est
                    ok, sol, cond = solve(L["H"], lam, L["b"])
                    if ok:
                        x = sol
                    est = oplus_all(est, sc, x)
                    tmp, evs, abs_tmp = robust_chi2(est, sc, active, robust)
                    for f in range(len(fr)):
                        stored[f][active[f]] = evs[f]["chi2"][active[f]]
                    if not ok:
                        tmp = DBL_MAX
                    scale = 0.0
                    for j in range(nd):
                        scale += x[j] * (lam * x[j] + L["b"][j])
                    scale += 1e-3
                    with np.errstate(all="ignore"):
                        rho = float((np.float64(cur) - np.float64(tmp)) / np.float64(scale))
                    accept = rho > 0 and math.isfinite(tmp)
                    res.trials.append(dict(lin=li, ok=ok, accepted=accept, lam=lam, cur=cur, tmp=tmp, scale=scale, rho=rho, cond=cond, dx=x.copy(),
                                           margin=abs(cur - tmp), abs_tmp=abs_tmp, est=copy.deepcopy(est), est0=copy.deepcopy(backup)))
                    if accept:
                        alpha = 1.0 - math.pow(2 * rho - 1, 3)
                        alpha = min(alpha, 2.0 / 3.0)
                        lam *= max(1.0 / 3.0, alpha)
                        ni = 2.0
                        cur = tmp
                    else:
                        lam *= ni
                        ni *= 2
                        est = backup
                    qmax += 1
                    if not (rho < 0 and qmax < 10):
                        break
                if qmax == 10 or rho == 0:
                    break
                stalled = stalled + 1 if (ini - cur) * 1e3 < ini else 0
                if stalled >= 3:
                    break
            # classification of both frames' edges
            for f, (_, edges) in enumerate(fr):
                if flag[f].any():
                    ev = reproj(est[f], sc, edges)
                    stored[f][flag[f]] = ev["chi2"][flag[f]]
                with np.errstate(all="ignore"):
                    gt = stored[f].astype(np.float32) > CHI2       # const float chi2 = e->chi2(); `else`: a NaN is an inlier
                flag[f], level[f] = gt.copy(), gt.copy()
            n_bad = int(flag[0].sum())
            res.class_chi2.append([s.copy() for s in stored])
            res.flags.append([f.copy() for f in flag])
            if n_edges(sc) < 10:                                 # optimizer.edges().size(): ALL edges
                break
    res.ns, res.est = est[0], est
    res.Tcw = pose_from_ns(est[0], sc)
    res.n_inliers, res.rounds = (n - n_bad if rounds else 0), rounds
    res.outlier = [f.astype(np.uint8) for f in flag]
    res.H_last = H_last
    res.marg_cov, res.marg_cov_inv, res.marg_ok = (None, None, False)
    if sc["compute_marg"] and H_last is not None:
        res.marg_cov, res.marg_cov_inv, res.marg_ok = marginals(H_last, sc)
    return res


def min_class_margin(res):
    m = float("inf")
    for c in res.class_chi2:
        for s in c:
            d = np.abs(s - float(CHI2))
            d = d[np.isfinite(d)]
            if len(d):
                m = min(m, float(d.min()))
    return m


def reentries(res):
    total = 0
    for f in range(len(res.outlier)):
        was, back = np.zeros(len(res.outlier[f]), bool), np.zeros(len(res.outlier[f]), bool)
        for fl in res.flags:
            back |= was & ~fl[f]
            was |= fl[f]
        total += int(back.sum())
    return total


# ---- scenes ----------------------------------------------------------------------------------------------------------------------------
def scene(seed, form=KEYFRAME, n=100, n_last=None, shifted=0, shift=None, has_depth=False, marg=False, off=(0.1, 0.3, 0.5), bias_step=0.0, garbage=False,
          degenerate=False, K=K_DEFAULT):
    """A last (key) frame and a current frame dT apart, moving under gravity, the preintegration consistent with the two true states up
    to noise; n (n_last) map points seen by each frame with half a pixel of noise at pyramid levels 0..3; the current frame's start
    `off` = (rad, m, m/s) away from the truth.  shifted: the first observations of both frames moved by a common shift px; garbage: every
    observation a random pixel; bias_step: the current frame's delta biases start this far from the last frame's; degenerate: identity
    rotations and extrinsics, point 0 exactly on the camera plane of the start (its chi2 is NaN and so is every sum)."""
    g = np.random.default_rng(seed)
    n_last = (n if n_last is None else n_last) if form == FRAME else 0
    dT = float(g.uniform(0.05, 0.4))
    gw = np.array([0.0, 0.0, -9.81]) if not degenerate else np.array([0.0, -9.81, 0.0])
    Ri = pm.rot_of_vec(g.normal(size=3) * (0.0 if degenerate else 0.3))
    Pi, Vi = g.normal(size=3) * 0.5, g.normal(size=3) * 0.5
    acc, omg = g.normal(size=3) * 0.5, g.normal(size=3) * (0.0 if degenerate else 0.3)
    Rj = Ri @ pm.rot_of_vec(omg * dT)
    Vj = Vi + gw * dT + Ri @ acc * dT
    Pj = Pi + Vi * dT + 0.5 * gw * dT * dT + 0.5 * (Ri @ acc) * dT * dT
    dP = Ri.T @ (Pj - Pi - Vi * dT - 0.5 * gw * dT * dT) + g.normal(size=3) * 1e-3
    dV = Ri.T @ (Vj - Vi - gw * dT) + g.normal(size=3) * 1e-3
    dR = Ri.T @ Rj @ pm.rot_of_vec(g.normal(size=3) * 1e-3)
    A = g.normal(size=(9, 9))
    cov = (A @ A.T * 0.02 + np.diag([1.0] * 3 + [4.0] * 3 + [0.25] * 3)) * 1e-4 * dT
    Rbc = np.eye(3) if degenerate else pm.rot_of_vec(np.array([0.01, -0.02, 1.55]) + g.normal(size=3) * 0.01)
    Pbc = np.zeros(3) if degenerate else np.array([-0.02, -0.06, 0.01])
    sc = dict(form=form, has_depth=bool(has_depth), compute_marg=bool(marg), dT=dT, dP=dP, dV=dV, dR=dR, gw=gw, Rbc=Rbc, Pbc=Pbc, K=tuple(float(v) for v in K),
              JPg=g.normal(size=(3, 3)) * dT * dT * 0.3, JPa=-np.eye(3) * 0.5 * dT * dT + g.normal(size=(3, 3)) * 1e-3,
              JVg=g.normal(size=(3, 3)) * dT * 0.3, JVa=-np.eye(3) * dT + g.normal(size=(3, 3)) * 1e-3, JRg=-np.eye(3) * dT + g.normal(size=(3, 3)) * 1e-3,
              cov=cov, gyr_rw2=1e-6, acc_rw2=1e-4)
    bg, ba = g.normal(size=3) * 0.01, g.normal(size=3) * 0.05
    last = state(Pi, Vi, q_of_matrix(Ri), bg, ba, g.normal(size=3) * 1e-3, g.normal(size=3) * 1e-2)

    def off_dir(m):
        v = g.normal(size=3)
        return v / np.linalg.norm(v) * m

    Rs = Rj if degenerate else Rj @ pm.rot_of_vec(off_dir(off[0]))
    cur = state(Pj + off_dir(off[1]), Vj + off_dir(off[2]), q_of_matrix(Rs), bg, ba, last["dbg"] + off_dir(bias_step) if bias_step else last["dbg"].copy(),
                last["dba"] + off_dir(bias_step * 5) if bias_step else last["dba"].copy())
    if degenerate:
        cur["q"], last["q"] = np.array([0.0, 0.0, 0.0, 1.0]), np.array([0.0, 0.0, 0.0, 1.0])
        cur["P"] = np.round(cur["P"] * 64) / 64          # exactly representable in float: Pw - Pwb is then exactly zero
    sc["cur"], sc["last"] = cur, last
    # the prior: the last frame's state a little off, a positive definite information
    sc["prior"] = state(Pi + g.normal(size=3) * 0.01, Vi + g.normal(size=3) * 0.02, q_of_matrix(Ri @ pm.rot_of_vec(g.normal(size=3) * 0.005)), bg, ba,
                        last["dbg"] + g.normal(size=3) * 1e-4, last["dba"] + g.normal(size=3) * 1e-3)
    B = g.normal(size=(15, 15))
    sc["prior_info"] = B @ B.T * 20.0 + np.diag([4e3] * 3 + [1e3] * 3 + [2e4] * 3 + [1e5] * 3 + [1e4] * 3)
    sc["depth_meas"] = float(Pj[2] + g.normal() * 0.02)
    sc["shi"] = float(g.uniform(0.9, 1.1))
    sc["depth_info"] = 400.0

    def observe(Rwb, Pwb, m):
        pc = np.stack([g.uniform(-3, 3, m), g.uniform(-2, 2, m), g.uniform(2, 10, m)], 1)
        Rcb = Rbc.T
        pw = (pc + Rcb @ Pbc) @ (Rcb @ Rwb.T) + Pwb            # Pc = Rcb Rwb^T (Pw - Pwb) - Rcb Pbc
        lvl = g.integers(0, 4, m)
        sig = 1.2 ** lvl
        uv = np.stack([K[0] * pc[:, 0] / pc[:, 2] + K[2], K[1] * pc[:, 1] / pc[:, 2] + K[3]], 1) + g.normal(size=(m, 2)) * 0.5 * sig[:, None]
        k = min(shifted, m)
        if k:
            s = g.uniform(5, 8) if shift is None else shift
            ang = g.uniform(0, 2 * math.pi)
            uv[:k] += s * np.array([math.cos(ang), math.sin(ang)])
        if garbage:
            uv = np.stack([g.uniform(0, 752, m), g.uniform(0, 480, m)], 1)
        return np.concatenate([pw, uv, (1.0 / (sig * sig))[:, None]], 1).astype(np.float32)

    sc["edges"] = observe(Rj, Pj, n)
    sc["edges_last"] = observe(Ri, Pi, n_last)
    if degenerate and n:
        sc["edges"][0, 2] = np.float32(cur["P"][2])
    return sc


# name -> scene arguments
SCENES = {}
FAR = (0.4, 1.0, 2.0)
for _i, (_f, _n) in enumerate(((KEYFRAME, 20), (KEYFRAME, 64), (KEYFRAME, 100), (KEYFRAME, 257), (KEYFRAME, 600), (FRAME, 20), (FRAME, 65), (FRAME, 100),
                               (FRAME, 256), (FRAME, 400))):
    SCENES["%s_plain_%d" % ("kf" if _f == KEYFRAME else "fr", _n)] = dict(seed=100 + _i, form=_f, n=_n, shifted=_n // 10, off=FAR)
for _i, (_f, _n) in enumerate(((KEYFRAME, 60), (KEYFRAME, 100), (KEYFRAME, 150), (KEYFRAME, 300), (FRAME, 60), (FRAME, 100), (FRAME, 150), (FRAME, 300))):
    SCENES["%s_shift_%d" % ("kf" if _f == KEYFRAME else "fr", _n)] = dict(seed=200 + _i, form=_f, n=_n, shifted=_n // 3, has_depth=_i % 2 == 1, marg=_i % 4 >= 2)
for _i, (_f, _n) in enumerate(((KEYFRAME, 30), (KEYFRAME, 120), (FRAME, 30), (FRAME, 120))):
    SCENES["%s_depth_marg_%d" % ("kf" if _f == KEYFRAME else "fr", _n)] = dict(seed=300 + _i, form=_f, n=_n, has_depth=True, marg=True, off=FAR)
for _i, _f in enumerate((KEYFRAME, FRAME)):
    _p = "kf" if _f == KEYFRAME else "fr"
    SCENES[_p + "_marg_only_80"] = dict(seed=320 + _i, form=_f, n=80, shifted=8, marg=True)
    SCENES[_p + "_depth_only_80"] = dict(seed=330 + _i, form=_f, n=80, has_depth=True)
    SCENES[_p + "_bias_step_100"] = dict(seed=340 + _i, form=_f, n=100, shifted=10, bias_step=0.02, marg=True)     # a large bias step
    SCENES[_p + "_none_left_12"] = dict(seed=350 + _i, form=_f, n=12, garbage=True)                     # every edge flagged after round 0
    SCENES[_p + "_degenerate_50"] = dict(seed=360 + _i, form=_f, n=50, degenerate=True, marg=True)      # decided by NaN class
    SCENES[_p + "_few_5"] = dict(seed=370 + _i, form=_f, n=5, n_last=0, shifted=1, off=FAR)                        # fewer than 10 edges: one round
    SCENES[_p + "_too_few"] = dict(seed=380 + _i, form=_f, n=2 if _f == KEYFRAME else 3, n_last=20)     # the early return
REENTRY = ("kf_shift_100", "fr_shift_150")     # an edge flagged in one round comes back in a later one (asserted by tests/test_navopt_model.py)


def make(name):
    return scene(**SCENES[name])


# ---- the C record (navopt::Problem) and the scene list as the stand-alone host build reads it --------------------------------------------
PROBLEM_DTYPE = np.dtype([("form", "<i4"), ("has_depth", "<i4"), ("compute_marg", "<i4"), ("n", "<i4"), ("n_last", "<i4"), ("off", "<i4"), ("pad_", "<i4", 2),
                          ("cur", "<f8", 22), ("last", "<f8", 22), ("prior", "<f8", 22), ("dT", "<f8"), ("dP", "<f8", 3), ("dV", "<f8", 3), ("dR", "<f8", 9),
                          ("JPg", "<f8", 9), ("JPa", "<f8", 9), ("JVg", "<f8", 9), ("JVa", "<f8", 9), ("JRg", "<f8", 9), ("cov", "<f8", 81), ("gw", "<f8", 3),
                          ("Rbc", "<f8", 9), ("Pbc", "<f8", 3), ("fx", "<f8"), ("fy", "<f8"), ("cx", "<f8"), ("cy", "<f8"), ("gyr_rw2", "<f8"), ("acc_rw2", "<f8"),
                          ("prior_info", "<f8", 225), ("depth_meas", "<f8"), ("shi", "<f8"), ("depth_info", "<f8")])


def record(sc):
    r = np.zeros(1, PROBLEM_DTYPE)
    r["form"], r["has_depth"], r["compute_marg"] = sc["form"], int(sc["has_depth"]), int(sc["compute_marg"])
    r["n"], r["n_last"] = len(sc["edges"]), len(sc["edges_last"]) if sc["form"] == FRAME else 0
    for k in ("cur", "last", "prior"):
        r[k] = state_vec(sc[k])
    for k in ("dT", "gyr_rw2", "acc_rw2", "depth_meas", "shi", "depth_info"):
        r[k] = float(sc[k])
    for k in ("dP", "dV", "dR", "JPg", "JPa", "JVg", "JVa", "JRg", "cov", "gw", "Rbc", "Pbc", "prior_info"):
        r[k] = np.asarray(sc[k], np.float64).reshape(-1)
    r["fx"], r["fy"], r["cx"], r["cy"] = sc["K"]
    return r


def all_edges(sc):
    e = np.asarray(sc["edges"], np.float32).reshape(-1, 6)
    if sc["form"] == FRAME:
        e = np.concatenate([e, np.asarray(sc["edges_last"], np.float32).reshape(-1, 6)])
    return np.ascontiguousarray(e)


def dump(path):
    """tests/golden/navopt_scenes.bin: int32 count, int32 record size; per scene the record, then float edges[n + n_last][6]."""
    with open(path, "wb") as f:
        f.write(np.array([len(SCENES), PROBLEM_DTYPE.itemsize], np.int32).tobytes())
        for name in SCENES:
            sc = make(name)
            f.write(record(sc).tobytes() + all_edges(sc).tobytes())


def load(path):
    """-> [(record, edges)] in SCENES' order."""
    raw, out = open(path, "rb").read(), []
    count, size = np.frombuffer(raw, np.int32, 2)
    off = 8
    for _ in range(int(count)):
        r = np.frombuffer(raw, PROBLEM_DTYPE, 1, off)
        m = int(r["n"][0] + r["n_last"][0])
        out.append((r.copy(), np.frombuffer(raw, np.float32, 6 * m, off + size).reshape(m, 6).copy()))
        off += size + 24 * m
    return out


if __name__ == "__main__":
    import sys
    dump(sys.argv[1])
