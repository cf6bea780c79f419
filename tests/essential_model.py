"""numpy / math restatement of Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:2409-2658 of the reference) for a gathered graph,
with the parts of g2o it runs, written from the reference's sources and not from csrc/essential_core.hpp:

    g2o::Sim3 (Thirdparty/g2o/g2o/types/sim3.h): the constructor from an update, operator*, inverse(), map(), log() in its four branches
    (W.lu().solve(t) is numpy.linalg.solve: LAPACK's partial-pivot LU), Eigen's Quaternion(Matrix3), toRotationMatrix, q * v;
    VertexSim3Expmap::oplusImpl with _fix_scale false, as the constructor leaves it (types_seven_dof_expmap.cpp:31-35);
    EdgeSim3::computeError = log(C * S_i * S_j^-1), information I_7, no robust kernel;
    BaseBinaryEdge::linearizeOplus (core/base_binary_edge.hpp:131-205): delta 1e-9, central, scalar 1 / 2e-9, a fixed vertex's columns
    not computed; constructQuadraticForm: H_ii += Ji^T Ji, H_ij += Ji^T Jj, b_i += Ji^T (-e);
    OptimizationAlgorithmLevenberg::solve with setUserLambdaInit(1e-16) and the stop criterion of :154-162, optimize(20);
    the pose recovery [R | t / s] and correctedSwr.map(Srw.map(X)), narrowed to float as Converter::toCvMat does.

The linear solve is dense (numpy.linalg.cholesky on H + lambda I: "ok" when it is positive definite); sums run over the edges in the
order of insertion (`order` permutes them, for the spread measurement); `ext="mp"` evaluates every EdgeSim3 error in mpmath at 50
digits and rounds it to double where g2o stores a double.

A similarity is a row of 8 doubles: q (x y z w, NOT normalised), t, s.  Scenes come from make(name); dump() / load() are the fixture
tests/golden/essential_scenes.bin (data only)."""
import math
import os
import struct

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "essential_scenes.bin")
DELTA = 1e-9
SCALAR = 1.0 / (2 * DELTA)
LAMBDA_INIT = 1e-16
MAX_TRIALS = 10
DBL_MAX = float(np.finfo(np.float64).max)


# ---- quaternions and similarities, on rows ------------------------------------------------------------------------------------------------
def qmul(a, b):
    """Eigen's quaternion product, x y z w."""
    ax, ay, az, aw = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
    bx, by, bz, bw = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    return np.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz, aw * bz + az * bw + ax * by - ay * bx,
                     aw * bw - ax * bx - ay * by - az * bz], -1)


def qrot(q, v):
    """Eigen's q * v: uv = 2 (q.vec x v); v + w uv + q.vec x uv.  No normalisation."""
    u = q[..., :3]
    uv = 2 * np.cross(u, v)
    return v + q[..., 3:4] * uv + np.cross(u, uv)


def rotmat(q):
    """toRotationMatrix, rows of 9."""
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz, txx, txy, txz, tyy, tyz, tzz = tx * w, ty * w, tz * w, tx * x, ty * x, tz * x, ty * y, tz * y, tz * z
    return np.stack([1 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1 - (txx + tzz), tyz - twx, txz - twy, tyz + twx, 1 - (txx + tyy)], -1)


def quat_of(R):
    """Eigen's Quaternion(Matrix3) on one 3 x 3 matrix -> x y z w."""
    R = np.asarray(R, np.float64).reshape(3, 3)
    t = R[0, 0] + R[1, 1] + R[2, 2]
    q = np.zeros(4)
    if t > 0:
        t = math.sqrt(t + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[0], q[1], q[2] = (R[2, 1] - R[1, 2]) * t, (R[0, 2] - R[2, 0]) * t, (R[1, 0] - R[0, 1]) * t
    else:
        i = 0
        if R[1, 1] > R[0, 0]:
            i = 1
        if R[2, 2] > R[i, i]:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        t = math.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0)
        q[i] = 0.5 * t
        t = 0.5 / t
        q[3] = (R[k, j] - R[j, k]) * t
        q[j] = (R[j, i] + R[i, j]) * t
        q[k] = (R[k, i] + R[i, k]) * t
    return q


def sim_mul(A, B):
    """operator*: r = a.r * b.r, t = a.s (a.r * b.t) + a.t, s = a.s * b.s."""
    return np.concatenate([qmul(A[..., :4], B[..., :4]), A[..., 7:8] * qrot(A[..., :4], B[..., 4:7]) + A[..., 4:7], A[..., 7:8] * B[..., 7:8]], -1)


def sim_inv(A):
    """inverse(): (r*, r* ((-1 / s) t), 1 / s)."""
    qc = A[..., :4] * np.array([-1.0, -1.0, -1.0, 1.0])
    return np.concatenate([qc, qrot(qc, (-1.0 / A[..., 7:8]) * A[..., 4:7]), 1.0 / A[..., 7:8]], -1)


def sim_map(A, X):
    return A[..., 7:8] * qrot(A[..., :4], X) + A[..., 4:7]


def skew(v):
    z = np.zeros_like(v[..., 0])
    return np.stack([z, -v[..., 2], v[..., 1], v[..., 2], z, -v[..., 0], -v[..., 1], v[..., 0], z], -1).reshape(v.shape[:-1] + (3, 3))


def sim_from_update(u):
    """Sim3(const Vector7d& update), sim3.h:70-142, on one update (omega, upsilon, sigma)."""
    u = np.asarray(u, np.float64)
    omega, upsilon, sigma = u[:3], u[3:6], float(u[6])
    theta = math.sqrt(float(omega @ omega))
    Om = skew(omega)
    s = math.exp(sigma)
    Om2 = Om @ Om
    I = np.eye(3)
    eps = 0.00001
    if abs(sigma) < eps:
        C = 1.0
        if theta < eps:
            A, B, R = 0.5, 1.0 / 6.0, I + Om + Om @ Om
        else:
            theta2 = theta * theta
            A, B = (1 - math.cos(theta)) / theta2, (theta - math.sin(theta)) / (theta2 * theta)
            R = I + math.sin(theta) / theta * Om + (1 - math.cos(theta)) / (theta * theta) * Om2
    else:
        C = (s - 1) / sigma
        if theta < eps:
            sigma2 = sigma * sigma
            A, B, R = ((sigma - 1) * s + 1) / sigma2, ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma), I + Om + Om2
        else:
            R = I + math.sin(theta) / theta * Om + (1 - math.cos(theta)) / (theta * theta) * Om2
            a, b, theta2, sigma2 = s * math.sin(theta), s * math.cos(theta), theta * theta, sigma * sigma
            c = theta2 + sigma2
            A = (a * sigma + (1 - b) * theta) / (theta * c)
            B = (C - ((b - 1) * sigma + a * theta) / c) * 1.0 / theta2
    W = A * Om + B * Om2 + C * I
    return np.concatenate([quat_of(R), W @ upsilon, [s]])


def sim_log(S, parts=False):
    """log(), sim3.h:148-230, on rows [n, 8] -> [n, 7] (omega, upsilon, sigma); parts: also A, B and W."""
    S = np.atleast_2d(S)
    s = S[:, 7]
    with np.errstate(all="ignore"):
        sigma = np.log(s)
        R = rotmat(S[:, :4]).reshape(-1, 3, 3)
        d = 0.5 * (R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2] - 1)
        dR = np.stack([R[:, 2, 1] - R[:, 1, 2], R[:, 0, 2] - R[:, 2, 0], R[:, 1, 0] - R[:, 0, 1]], -1)
        eps = 0.00001
        small, near = np.abs(sigma) < eps, d > 1 - eps
        theta = np.arccos(d)
        theta2, sigma2 = theta * theta, sigma * sigma
        omega = np.where(near[:, None], 0.5 * dR, (theta / (2 * np.sqrt(1 - d * d)))[:, None] * dR)
        a, b, c = s * np.sin(theta), s * np.cos(theta), theta2 + sigma * sigma
        Cg = (s - 1) / sigma
        C = np.where(small, 1.0, Cg)
        A = np.where(small, np.where(near, 0.5, (1 - np.cos(theta)) / theta2),
                     np.where(near, ((sigma - 1) * s + 1) / sigma2, (a * sigma + (1 - b) * theta) / (theta * c)))
        B = np.where(small, np.where(near, 1.0 / 6.0, (theta - np.sin(theta)) / (theta2 * theta)),
                     np.where(near, ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma), (Cg - ((b - 1) * sigma + a * theta) / c) * 1.0 / theta2))
        Om = skew(omega)
        W = A[:, None, None] * Om + B[:, None, None] * (Om @ Om) + C[:, None, None] * np.eye(3)
        ups = np.full((len(S), 3), np.nan)
        good = np.isfinite(W).all((1, 2)) & np.isfinite(S[:, 4:7]).all(1) & (np.abs(np.linalg.det(np.where(np.isfinite(W), W, 0.0))) > 0)
        if good.any():
            ups[good] = np.linalg.solve(W[good], S[good, 4:7, None])[:, :, 0]
    out = np.concatenate([omega, ups, sigma[:, None]], 1)
    return (out, A, B, W) if parts else out


def edge_errors(C, Si, Sj):
    """EdgeSim3::computeError on rows: log(C * S_i * S_j^-1)."""
    return sim_log(sim_mul(sim_mul(C, Si), sim_inv(Sj)))


# ---- the same error in mpmath, one edge -----------------------------------------------------------------------------------------------------
def edge_error_mp(C, Si, Sj, digits=50):
    import mpmath as mp
    with mp.workdps(digits):
        def sim(r):
            return [mp.mpf(float(v)) for v in r]

        def cross(a, b):
            return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]

        def rot(q, v):
            uv = [2 * c for c in cross(q[:3], v)]
            c2 = cross(q[:3], uv)
            return [v[i] + q[3] * uv[i] + c2[i] for i in range(3)]

        def mul(A, B):
            a, b = A[:4], B[:4]
            q = [a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1], a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2],
                 a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0], a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]]
            r = rot(a, B[4:7])
            return q + [A[7] * r[i] + A[4 + i] for i in range(3)] + [A[7] * B[7]]

        def inv(A):
            qc = [-A[0], -A[1], -A[2], A[3]]
            return qc + rot(qc, [(-1 / A[7]) * A[4 + i] for i in range(3)]) + [1 / A[7]]

        E = mul(mul(sim(C), sim(Si)), inv(sim(Sj)))
        x, y, z, w = E[:4]
        R = [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
             [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]
        s = E[7]
        sigma = mp.log(s)
        d = (R[0][0] + R[1][1] + R[2][2] - 1) / 2
        dR = [R[2][1] - R[1][2], R[0][2] - R[2][0], R[1][0] - R[0][1]]
        eps = mp.mpf("0.00001")
        if d > 1 - eps:
            om = [v / 2 for v in dR]
            if abs(sigma) < eps:
                A, B, Cc = mp.mpf(1) / 2, mp.mpf(1) / 6, mp.mpf(1)
            else:
                Cc, A, B = (s - 1) / sigma, ((sigma - 1) * s + 1) / sigma ** 2, ((sigma ** 2 / 2 - sigma + 1) * s) / sigma ** 3
        else:
            th = mp.acos(d)
            om = [th / (2 * mp.sqrt(1 - d * d)) * v for v in dR]
            if abs(sigma) < eps:
                Cc, A, B = mp.mpf(1), (1 - mp.cos(th)) / th ** 2, (th - mp.sin(th)) / th ** 3
            else:
                Cc = (s - 1) / sigma
                a, b, c = s * mp.sin(th), s * mp.cos(th), th ** 2 + sigma ** 2
                A, B = (a * sigma + (1 - b) * th) / (th * c), (Cc - ((b - 1) * sigma + a * th) / c) / th ** 2
        Om = mp.matrix([[0, -om[2], om[1]], [om[2], 0, -om[0]], [-om[1], om[0], 0]])
        W = A * Om + B * (Om * Om) + Cc * mp.eye(3)
        ups = mp.lu_solve(W, mp.matrix(E[4:7]))
        return np.array([float(v) for v in om] + [float(ups[i]) for i in range(3)] + [float(sigma)])


def _errors(C, Si, Sj, ext):
    if ext == "mp":
        return np.array([edge_error_mp(C[e], Si[e], Sj[e]) for e in range(len(C))]).reshape(-1, 7)
    return edge_errors(C, Si, Sj)


# ---- the graph ----------------------------------------------------------------------------------------------------------------------------
def free_index(K, fixed):
    f = np.arange(K) - (np.arange(K) > fixed)
    f[fixed] = -1
    return f


def measure(sc):
    """setMeasurement(Sjw * Swi): from vScw for an edge of LoopConnections, from NonCorrectedSim3 (else vScw) for the others."""
    i, j, conn = sc["edge_i"], sc["edge_j"], sc["conn"].astype(bool)
    Sj = np.where(conn[:, None], sc["Scw"][j], sc["Scwn"][j])
    Si = np.where(conn[:, None], sc["Scw"][i], sc["Scwn"][i])
    return sim_mul(Sj, sim_inv(Si)).reshape(-1, 8)


class Lin:
    """One linearisation at est: e [E, 7], Ji, Jj [E, 7, 7] (zero for a fixed vertex), chi2, H [7F, 7F], b [7F]."""


def linearise(sc, meas, est, order=None, ext=None):
    K, E = len(est), len(meas)
    i, j = sc["edge_i"], sc["edge_j"]
    free = free_index(K, sc["fixed"])
    F = K - 1
    L = Lin()
    L.est = est.copy()
    L.e = _errors(meas, est[i], est[j], ext).reshape(E, 7)
    L.Ji, L.Jj = np.zeros((E, 7, 7)), np.zeros((E, 7, 7))
    for d in range(7):
        u = np.zeros(7)
        u[d] = DELTA
        plus, minus = sim_from_update(u), sim_from_update(-u)
        ei = free[i] >= 0
        if ei.any():
            ep = _errors(meas[ei], sim_mul(plus[None], est[i[ei]]), est[j[ei]], ext)
            em = _errors(meas[ei], sim_mul(minus[None], est[i[ei]]), est[j[ei]], ext)
            L.Ji[ei, :, d] = SCALAR * (ep - em)
        ej = free[j] >= 0
        if ej.any():
            ep = _errors(meas[ej], est[i[ej]], sim_mul(plus[None], est[j[ej]]), ext)
            em = _errors(meas[ej], est[i[ej]], sim_mul(minus[None], est[j[ej]]), ext)
            L.Jj[ej, :, d] = SCALAR * (ep - em)
    H, b = np.zeros((7 * F, 7 * F)), np.zeros(7 * F)
    chi2 = 0.0
    for e in (range(E) if order is None else order):
        chi2 += float(L.e[e] @ L.e[e])
        a, c = free[i[e]], free[j[e]]
        if a >= 0:
            H[7 * a:7 * a + 7, 7 * a:7 * a + 7] += L.Ji[e].T @ L.Ji[e]
            b[7 * a:7 * a + 7] += L.Ji[e].T @ -L.e[e]
        if c >= 0:
            H[7 * c:7 * c + 7, 7 * c:7 * c + 7] += L.Jj[e].T @ L.Jj[e]
            b[7 * c:7 * c + 7] += L.Jj[e].T @ -L.e[e]
        if a >= 0 and c >= 0:
            blk = L.Ji[e].T @ L.Jj[e]
            H[7 * a:7 * a + 7, 7 * c:7 * c + 7] += blk
            H[7 * c:7 * c + 7, 7 * a:7 * a + 7] += blk.T
    L.H, L.b, L.chi2 = H, b, chi2
    return L


def chi2_at(sc, meas, est, order=None, ext=None):
    e = _errors(meas, est[sc["edge_i"]], est[sc["edge_j"]], ext).reshape(-1, 7)
    c = 0.0
    for k in (range(len(e)) if order is None else order):
        c += float(e[k] @ e[k])
    return c


def solve(H, b, lam):
    """(H + lambda I) x = b by a dense Cholesky -> (ok, x)."""
    A = H + lam * np.eye(len(H))
    if not np.isfinite(A).all():
        return False, None
    try:
        Lc = np.linalg.cholesky(A)
    except np.linalg.LinAlgError:
        return False, None
    return True, np.linalg.solve(Lc.T, np.linalg.solve(Lc, b))


def apply(sc, est, x):
    """oplusImpl of every free vertex: Sim3(update) * estimate."""
    free = free_index(len(est), sc["fixed"])
    out = est.copy()
    for k in range(len(est)):
        if free[k] >= 0:
            out[k] = sim_mul(sim_from_update(x[7 * free[k]:7 * free[k] + 7]), est[k])
    return out


def one_trial(sc, meas, L, lam, cur, x_prev, order=None, ext=None):
    """-> dict(ok, x, est_try, tmp, scale, rho, accepted)."""
    ok, x = solve(L.H, L.b, lam)
    if not ok:
        x = x_prev
    est_try = apply(sc, L.est, x)
    with np.errstate(all="ignore"):
        tmp = chi2_at(sc, meas, est_try, order, ext)
    if not ok:
        tmp = DBL_MAX
    scale = float(np.sum(x * (lam * x + L.b))) + 1e-3
    rho = (cur - tmp) / scale
    return dict(ok=ok, x=x, est_try=est_try, tmp=tmp, scale=scale, rho=rho, accepted=bool(rho > 0 and np.isfinite(tmp)), lam=lam, cur=cur)


class Result:
    pass


def recover(sc, est):
    """-> (Tcw float32 [K, 4, 4], points float32 [P, 3])."""
    K = len(est)
    T = np.zeros((K, 4, 4), np.float32)
    T[:, :3, :3] = rotmat(est[:, :4]).reshape(K, 3, 3).astype(np.float32)
    T[:, :3, 3] = (est[:, 4:7] * (1.0 / est[:, 7:8])).astype(np.float32)
    T[:, 3, 3] = 1
    ref = sc["ref"]
    X = sc["points"].astype(np.float64).reshape(-1, 3)
    pts = sim_map(sim_inv(est)[ref], sim_map(sc["Scw"][ref], X)).astype(np.float32) if len(X) else np.zeros((0, 3), np.float32)
    return T, pts


def optimize(sc, order=None, ext=None):
    """optimize(n_iterations) under OptimizationAlgorithmLevenberg, then the recovery -> Result with S [K, 8], Tcw, points, lin (the
    Lin records), trials (one_trial's dicts with `lin`), iterations."""
    meas = measure(sc)
    est = sc["Scw"].copy()
    K, E = len(est), len(meas)
    r = Result()
    r.lin, r.trials, r.meas = [], [], meas
    if K > 1 and E > 0:
        lam, ni, n_bad = LAMBDA_INIT, 2.0, 0
        x = np.zeros(7 * (K - 1))
        for it in range(sc["n_iterations"]):
            with np.errstate(all="ignore"):
                L = linearise(sc, meas, est, order, ext)
            cur = ini = L.chi2
            if it == 0:
                lam, ni, n_bad = LAMBDA_INIT, 2.0, 0
            r.lin.append(L)
            rho, q = 0.0, 0
            while True:
                t = one_trial(sc, meas, L, lam, cur, x, order, ext)
                t["lin"] = len(r.lin) - 1
                r.trials.append(t)
                x, rho = t["x"], t["rho"]
                if t["accepted"]:
                    alpha = min(1.0 - (2 * rho - 1) ** 3, 2.0 / 3.0)
                    lam *= max(1.0 / 3.0, alpha)
                    ni, cur, est = 2.0, t["tmp"], t["est_try"]
                else:
                    lam *= ni
                    ni *= 2
                q += 1
                if not (rho < 0 and q < MAX_TRIALS):
                    break
            t["cur_after"] = cur
            if q == MAX_TRIALS or rho == 0:
                break
            n_bad = n_bad + 1 if (ini - cur) * 1e3 < ini else 0
            t["stall_margin"] = abs((ini - cur) * 1e3 - ini) / max(abs(ini), 1e-300)
            if n_bad >= 3:
                break
    r.S = est
    r.Tcw, r.points = recover(sc, est)
    r.iterations = len(r.lin)
    return r


# ---- scenes -------------------------------------------------------------------------------------------------------------------------------
def _rodrigues(v):
    th = float(np.linalg.norm(v))
    if th < 1e-12:
        return np.eye(3)
    k = skew(np.asarray(v, np.float64) / th)
    return np.eye(3) + math.sin(th) * k + (1 - math.cos(th)) * (k @ k)


def _sim(R, t, s):
    return np.concatenate([quat_of(R), np.asarray(t, np.float64), [s]])


def _from_floats(R, t):
    """Sim3(Rcw, tcw, 1.0) of a key frame's float pose."""
    return _sim(np.asarray(R, np.float32).astype(np.float64), np.asarray(t, np.float32).astype(np.float64), 1.0)


def _trajectory(g, K, radius=6.0, drift_r=0.004, drift_t=0.02):
    """Key frames on a circle looking inwards, with a drift that accumulates along the chain -> the drifted float poses [K] of (R, t)."""
    poses, Rd, td = [], np.eye(3), np.zeros(3)
    for k in range(K):
        a = 2 * math.pi * k / max(K, 8)
        Rwc = _rodrigues([0, a, 0]) @ _rodrigues(g.normal(size=3) * 0.02)
        c = np.array([radius * math.sin(a), 0.1 * g.normal(), radius * (1 - math.cos(a))])
        Rd, td = _rodrigues(g.normal(size=3) * drift_r) @ Rd, td + g.normal(size=3) * drift_t
        Rcw = (Rd @ Rwc).T
        poses.append((Rcw.astype(np.float32), (-Rcw @ (c + td)).astype(np.float32)))
    return poses


def _scene(g, K, loops, extra=0, P=0, gaps=False, isolated=None, duplicates=0, correction=(0.05, 0.3, 1.1), n_corrected=3, consistent=False, drift=(0.004, 0.02)):
    """loops: (current, loop) index pairs, the first one's `loop` is the fixed key frame.  correction: rotation (rad), translation, scale
    of the loop's Sim3 correction."""
    poses = _trajectory(g, K, drift_r=drift[0], drift_t=drift[1])
    Scwn = np.array([_from_floats(R, t) for R, t in poses])
    Scw = Scwn.copy()
    conn_pairs = []
    for n, (cur, lp) in enumerate(loops):
        if not consistent:
            rot, tr, sc = correction
            corr = _sim(_rodrigues(g.normal(size=3) * rot), g.normal(size=3) * tr, sc * (1 + 0.05 * n))
            # CorrectedSim3 of the current key frame and its neighbours: Sic * corrected Scw of the current one
            Scur = sim_mul(corr, Scwn[cur])
            for k in range(max(cur - n_corrected + 1, 0), cur + 1):
                Scw[k] = sim_mul(sim_mul(Scwn[k], sim_inv(Scwn[cur])), Scur)
        for k in range(max(cur - 1, 0), cur + 1):
            for l in range(lp, min(lp + 2, K)):
                if k != l and (k, l) not in conn_pairs:
                    conn_pairs.append((k, l))
    ei, ej, conn = [], [], []
    for k, l in conn_pairs:
        ei.append(k), ej.append(l), conn.append(1)
    for k in range(K):
        if isolated is not None and k == isolated:
            continue
        parent = k - 1 if k - 1 != isolated else k - 2
        if k > 0 and parent >= 0:
            ei.append(k), ej.append(parent), conn.append(0)
        for back in range(2, 2 + extra):
            l = k - back
            if l >= 0 and l != isolated and g.random() < 0.8 and (k, l) not in conn_pairs:
                ei.append(k), ej.append(l), conn.append(0)
    for _ in range(duplicates):
        e = int(g.integers(len(ei)))
        ei.append(ei[e]), ej.append(ej[e]), conn.append(conn[e])
    mnid = np.arange(K) * (3 if gaps else 1) + (np.arange(K) > K // 2) * (5 if gaps else 0)
    ref = g.integers(0, K, P).astype(np.int32)
    pts = np.zeros((P, 3), np.float32)
    for p in range(P):
        S = Scwn[ref[p]]
        pts[p] = sim_map(sim_inv(S), np.array([g.normal(), g.normal(), 4 + g.random() * 4])).astype(np.float32)
    return dict(mnid=mnid.astype(np.int32), Scw=Scw, Scwn=Scwn, edge_i=np.array(ei, np.int32), edge_j=np.array(ej, np.int32), conn=np.array(conn, np.uint8),
                points=pts, ref=ref, fixed=int(loops[0][1]) if loops else 0, n_iterations=20)


def _make(name):
    g = np.random.default_rng(sum(ord(c) for c in name) * 7919)
    if name == "kf2":
        return dict(_scene(g, 2, [(1, 0)], P=3, n_corrected=1), n_iterations=2)      # the cap ends it: beyond, chi2 moves by rounding noise alone
    if name == "chain3":
        sc = _scene(g, 3, [], P=5)
        sc["Scw"][2] = sim_mul(_sim(_rodrigues([0.01, -0.02, 0.015]), [0.05, -0.02, 0.04], 1.05), sc["Scwn"][2])
        sc["fixed"], sc["n_iterations"] = 0, 1       # a tree has a zero minimum and one step reaches the rounding noise: the cap ends it there
        return sc
    if name == "ring12":
        return _scene(g, 12, [(11, 0)], P=20)
    if name == "kf40":
        return _scene(g, 40, [(39, 2), (25, 8)], extra=2, P=60, gaps=True, isolated=17, duplicates=4, correction=(0.04, 0.25, 0.8), n_corrected=4)
    if name == "kf150":
        return _scene(g, 150, [(149, 5)], extra=4, P=300, correction=(0.03, 0.3, 1.2), n_corrected=5, drift=(0.002, 0.01))
    if name == "rejected":
        return _scene(np.random.default_rng(0), 10, [(9, 0)], P=8, correction=(3.0, 1.0, 1.0))   # nine trials of its third iteration are rejected, the tenth accepted
    if name == "no_points":
        return _scene(g, 8, [(7, 1)], extra=1, P=0)
    if name == "large_rotation":
        return _scene(g, 9, [(8, 0)], P=6, correction=(0.5, 0.5, 1.0))
    if name == "zero_error":
        return dict(_scene(g, 7, [(6, 0)], extra=1, P=4, consistent=True), n_iterations=1)
    raise KeyError(name)


SCENES = ("kf2", "chain3", "ring12", "kf40", "kf150", "rejected", "no_points", "large_rotation", "zero_error")


def make(name, _cache={}):
    """The scene as committed when the fixture is there (the tests' input), else as generated."""
    if name not in _cache:
        if not _cache.get("__loaded__") and os.path.exists(FIXTURE):
            _cache.update(load(FIXTURE))
            _cache["__loaded__"] = True
        if name not in _cache:
            _cache[name] = _make(name)
    return _cache[name]


def dump(path=FIXTURE, names=SCENES, fresh=True):
    with open(path, "wb") as fh:
        fh.write(struct.pack("<i", len(names)))
        for name in names:
            sc = _make(name) if fresh else make(name)
            K, E, P = len(sc["Scw"]), len(sc["edge_i"]), len(sc["points"])
            fh.write(struct.pack("<5i", K, E, P, sc["fixed"], sc["n_iterations"]))
            for a, t in ((sc["mnid"], "<i4"), (sc["Scw"], "<f8"), (sc["Scwn"], "<f8"), (sc["edge_i"], "<i4"), (sc["edge_j"], "<i4"), (sc["conn"], "u1"),
                         (sc["points"], "<f4"), (sc["ref"], "<i4")):
                fh.write(np.ascontiguousarray(a, t).tobytes())


def load(path=FIXTURE, names=SCENES):
    out = {}
    with open(path, "rb") as fh:
        (count,) = struct.unpack("<i", fh.read(4))
        assert count == len(names)
        for name in names:
            K, E, P, fixed, its = struct.unpack("<5i", fh.read(20))

            def rd(t, n, shape):
                return np.frombuffer(fh.read(np.dtype(t).itemsize * n), t).reshape(shape).copy()
            out[name] = dict(mnid=rd("<i4", K, (K,)), Scw=rd("<f8", 8 * K, (K, 8)), Scwn=rd("<f8", 8 * K, (K, 8)), edge_i=rd("<i4", E, (E,)), edge_j=rd("<i4", E, (E,)),
                             conn=rd("u1", E, (E,)), points=rd("<f4", 3 * P, (P, 3)), ref=rd("<i4", P, (P,)), fixed=fixed, n_iterations=its)
    return out


if __name__ == "__main__":
    dump()
    for n in SCENES:
        s = make(n)
        print(n, len(s["Scw"]), len(s["edge_i"]), len(s["points"]))
