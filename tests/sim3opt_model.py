"""Optimizer::OptimizeSim3 restated in numpy from the reference's sources (src/Optimizer.cc:2660-2856; g2o: types_seven_dof_expmap.h,
sim3.h, se3_ops.hpp, core/base_binary_edge.hpp:131-205 (the numeric Jacobian), optimization_algorithm_levenberg.cpp,
robust_kernel_impl.cpp (Huber), linear_solver_dense.h) -- not from csrc/sim3opt_core.hpp.  Sums are serial in edge order (e12 of pair 0,
e21 of pair 0, e12 of pair 1, ...), the solve is numpy.linalg.solve, sin / cos / exp are math's, map() rotates every point by the
quaternion as Eigen does.  Nothing here is fast.

    1. the Jacobian is the central difference of linearizeOplus: delta 1e-9, scalar 1 / (2 delta), seven columns, estimates
       Sim3(+-delta e_d) * estimate;
    2. two edges per pair: obs1 - cam_map1(project(S.map(X2c))) and obs2 - cam_map2(project(S.inverse().map(X1c))); X1c, X2c are the
       float products R X + t widened;
    3. the informations are taken as given (the caller passes GetInvSigma2(octave1) and GetSigma2(octave2));
    4. the state is (quaternion, t, s) in double from Eigen's Quaternion(Matrix3), never normalised; the update is Sim3(dx) * estimate
       with the four-branch exponential, eps 1e-5 on |sigma| and theta;
    5. Huber at (double)(float)sqrt(th2); optimize(5), the check, optimize(10 if nBad else 5); lambda, ni and the stall count anew per
       optimize, the estimate kept;
    6. a pair is bad when either STORED chi2 (last evaluated trial, accepted or not) exceeds th2; removed for good; NaN stays;
    7. nCorrespondences - nBad < 10 returns 0 and leaves g2oS12 as it was;
    8. (skipped matches are the adaptor's business)
    9. Eigen's LDLT on 7 x 7: succeeds on a positive (semi-)definite matrix.

`ext="mp"` evaluates every projection error in mpmath at 50 digits and rounds it to double where g2o stores a double (the _error
vector): the same function without the evaluation's rounding noise under the 1e-9 difference (what is left is the rounding of the
stored estimate and of the stored error).  `ext=True` does the same in numpy.longdouble (64-bit significand): a quick stand-in that the
suite uses for a partial re-measurement.  `order` permutes the pairs."""
import math

import numpy as np

DBL_MAX = float(np.finfo(np.float64).max)
STEP = 1e-9
SCALAR = 1.0 / (2 * STEP)
K1_DEFAULT = (458.654, 457.296, 367.215, 248.375)
K2_DEFAULT = (460.1, 459.3, 365.4, 250.9)
TH2 = 10.0   # what LoopClosing::ComputeSim3 passes


# ---- Eigen's quaternion, g2o::Sim3 ---------------------------------------------------------------------------------------------------
def quat_of(R):
    """Eigen's Quaternion(Matrix3) -> (x, y, z, w)."""
    R = np.asarray(R, np.float64)
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
        with np.errstate(all="ignore"):
            t = float(np.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0))
            q[i] = 0.5 * t
            t = np.float64(0.5) / t
        q[3] = (R[k, j] - R[j, k]) * t
        q[j] = (R[j, i] + R[i, j]) * t
        q[k] = (R[k, i] + R[i, k]) * t
    return q


def rot_of(q):
    """Eigen's toRotationMatrix."""
    x, y, z, w = q
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.array([[1 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1 - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, 1 - (txx + tyy)]])


def quat_mul(a, b):
    return np.array([a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1],
                     a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2],
                     a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0],
                     a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]])


def quat_rotate(q, v):
    """Eigen's quaternion * vector on v [..., 3]: uv = 2 (q.vec x v); v + w uv + q.vec x uv.  The dtype of v is kept."""
    dt = v.dtype
    qv, w = q[:3].astype(dt), dt.type(q[3])
    uv = np.cross(np.broadcast_to(qv, v.shape), v)
    uv = uv + uv
    return v + w * uv + np.cross(np.broadcast_to(qv, v.shape), uv)


class Sim:
    """g2o::Sim3: r (x y z w), t, s."""

    def __init__(self, q, t, s):
        self.q, self.t, self.s = np.asarray(q, np.float64), np.asarray(t, np.float64), float(s)

    def vec(self):
        return np.concatenate([self.q, self.t, [self.s]])

    def map(self, X):
        dt = X.dtype
        return dt.type(self.s) * quat_rotate(self.q, X) + self.t.astype(dt)

    def inverse(self):
        qc = np.array([-self.q[0], -self.q[1], -self.q[2], self.q[3]])
        with np.errstate(all="ignore"):
            ms, si = np.float64(-1.0) / np.float64(self.s), np.float64(1.0) / np.float64(self.s)
            return Sim(qc, quat_rotate(qc, ms * self.t), si)

    def __mul__(self, o):
        with np.errstate(all="ignore"):
            return Sim(quat_mul(self.q, o.q), self.s * quat_rotate(self.q, o.t) + self.t, np.float64(self.s) * np.float64(o.s))


def sim_from_floats(R12, t12, s12):
    """Sim3(Matrix3d, Vector3d, double) from the caller's floats."""
    R = np.asarray(R12, np.float32).reshape(3, 3).astype(np.float64)
    return Sim(quat_of(R), np.asarray(t12, np.float32).astype(np.float64), float(np.float32(s12)))


def skew(o):
    return np.array([[0, -o[2], o[1]], [o[2], 0, -o[0]], [-o[1], o[0], 0]], np.float64)


def _exp(x):
    try:
        return math.exp(x)
    except OverflowError:
        return float("inf")


def sim_exp(update):
    """Sim3(const Vector7d&), sim3.h:70-142 -> Sim, and the branch taken (0..3: sigma small/large x theta small/large)."""
    u = np.asarray(update, np.float64)
    omega, upsilon, sigma = u[:3], u[3:6], float(u[6])
    if not np.isfinite(u).all():
        nan = np.full(3, np.nan)
        return Sim(np.full(4, np.nan), nan, np.nan), -1
    theta = math.sqrt(float(omega @ omega))
    Om = skew(omega)
    s = _exp(sigma)
    Om2 = Om @ Om
    I = np.eye(3)
    eps = 0.00001
    with np.errstate(all="ignore"):
        if abs(sigma) < eps:
            C = 1.0
            if theta < eps:
                A, B, R, br = 1.0 / 2.0, 1.0 / 6.0, I + Om + Om2, 0
            else:
                theta2 = theta * theta
                A = (1 - math.cos(theta)) / theta2
                B = (theta - math.sin(theta)) / (theta2 * theta)
                R, br = I + math.sin(theta) / theta * Om + (1 - math.cos(theta)) / (theta * theta) * Om2, 1
        else:
            C = (s - 1) / sigma
            if theta < eps:
                sigma2 = sigma * sigma
                A = ((sigma - 1) * s + 1) / sigma2
                B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma)
                R, br = I + Om + Om2, 2
            else:
                R = I + math.sin(theta) / theta * Om + (1 - math.cos(theta)) / (theta * theta) * Om2
                a, b = s * math.sin(theta), s * math.cos(theta)
                theta2, sigma2 = theta * theta, sigma * sigma
                c = theta2 + sigma2
                A = (a * sigma + (1 - b) * theta) / (theta * c)
                B = (C - ((b - 1) * sigma + a * theta) / c) * 1.0 / theta2
                br = 3
        W = A * Om + B * Om2 + C * I
        return Sim(quat_of(R), W @ upsilon, s), br


def oplus(dx, S):
    """VertexSim3Expmap::oplusImpl: Sim3(update) * estimate."""
    return sim_exp(dx)[0] * S


# ---- the scene as the optimiser sees it -------------------------------------------------------------------------------------------------
def camera_points(Rcw, tcw, xw):
    """R * X + t in CV_32F [OCV-RECALL 1 of csrc/sim3_core.hpp]: products and sums in double in index order, one rounding to float."""
    R, t, x = np.asarray(Rcw, np.float32).reshape(3, 3).astype(np.float64), np.asarray(tcw, np.float32).astype(np.float64), np.asarray(xw, np.float32).astype(np.float64)
    x = x.reshape(-1, 3)
    return np.stack([((R[r, 0] * x[:, 0] + R[r, 1] * x[:, 1]) + R[r, 2] * x[:, 2]) + t[r] for r in range(3)], 1).astype(np.float32)


def pairs_of(sc):
    """[n, 12] float32: X1c, X2c, obs1, obs2, info1, info2."""
    n = len(sc["x1w"])
    if n == 0:
        return np.zeros((0, 12), np.float32)
    return np.concatenate([camera_points(sc["kf1"][0], sc["kf1"][1], sc["x1w"]), camera_points(sc["kf2"][0], sc["kf2"][1], sc["x2w"]),
                           sc["obs1"], sc["obs2"], sc["info1"][:, None], sc["info2"][:, None]], 1).astype(np.float32)


def _edge_errors_mp(S, P, K1, K2):
    """edge_errors with every operation in mpmath at 50 digits; the inputs are the doubles g2o holds (the estimate, the points, the
    observations, the intrinsics), the outputs are rounded to double where g2o stores the _error vector."""
    import mpmath
    mp = mpmath.mp.clone()
    mp.dps = 50
    f = mp.mpf
    q, t, s = [f(float(v)) for v in S.q], [f(float(v)) for v in S.t], f(float(S.s))
    x, y, z, w = q
    R = [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
         [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
         [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]           # toRotationMatrix: q * v for any q
    si = 1 / s
    ti = [-si * sum(R[k][r] * t[k] for k in range(3)) for r in range(3)]                # r* ((-1 / s) t)
    k1, k2 = [f(float(np.float32(v))) for v in K1], [f(float(np.float32(v))) for v in K2]
    e12, e21 = np.zeros((len(P), 2)), np.zeros((len(P), 2))
    for i, row in enumerate(np.asarray(P, np.float64)):
        X1, X2 = [f(v) for v in row[0:3]], [f(v) for v in row[3:6]]
        a = [s * sum(R[r][k] * X2[k] for k in range(3)) + t[r] for r in range(3)]
        b = [si * sum(R[k][r] * X1[k] for k in range(3)) + ti[r] for r in range(3)]
        for r in range(2):
            try:
                e12[i, r] = float(f(row[6 + r]) - (a[r] / a[2] * k1[r] + k1[2 + r]))
            except ZeroDivisionError:
                e12[i, r] = -np.inf if (a[r] > 0) == (k1[r] > 0) else np.inf if a[r] != 0 else np.nan
            try:
                e21[i, r] = float(f(row[8 + r]) - (b[r] / b[2] * k2[r] + k2[2 + r]))
            except ZeroDivisionError:
                e21[i, r] = -np.inf if (b[r] > 0) == (k2[r] > 0) else np.inf if b[r] != 0 else np.nan
    return e12, e21


def edge_errors(S, P, K1, K2, ext=False):
    """computeError of both edges of every pair at S -> e12 [n, 2], e21 [n, 2] in double.  ext: False, True (numpy.longdouble) or "mp"
    (mpmath at 50 digits)."""
    if ext == "mp":
        return _edge_errors_mp(S, P, K1, K2)
    dt = np.longdouble if ext else np.float64
    P = P.astype(dt)
    k1, k2 = [dt(np.float32(v)) for v in K1], [dt(np.float32(v)) for v in K2]
    with np.errstate(all="ignore"):
        a = S.map(P[:, 3:6])
        b = S.inverse().map(P[:, 0:3])
        e12 = P[:, 6:8] - np.stack([a[:, 0] / a[:, 2] * k1[0] + k1[2], a[:, 1] / a[:, 2] * k1[1] + k1[3]], 1)
        e21 = P[:, 8:10] - np.stack([b[:, 0] / b[:, 2] * k2[0] + k2[2], b[:, 1] / b[:, 2] * k2[1] + k2[3]], 1)
    return e12.astype(np.float64), e21.astype(np.float64)


def chi2_of(e, w):
    """_error.dot(information() * _error) with the information's zeros kept."""
    with np.errstate(all="ignore"):
        return e[:, 0] * (w * e[:, 0] + 0.0 * e[:, 1]) + e[:, 1] * (0.0 * e[:, 0] + w * e[:, 1])


def delta_of(th2):
    """const float deltaHuber = sqrt(th2), widened by setDelta."""
    return float(np.sqrt(np.float32(th2)))


def huber(e, delta):
    dsqr = delta * delta
    with np.errstate(all="ignore"):
        sq = np.sqrt(e)
        inl = e <= dsqr
        return np.where(inl, e, 2 * sq * delta - dsqr), np.where(inl, 1.0, delta / sq)


def numeric_jacobians(S, P, K1, K2, ext=False):
    """BaseBinaryEdge::linearizeOplus for the Sim3 vertex -> J12, J21 [n, 2, 7]."""
    n = len(P)
    J12, J21 = np.zeros((n, 2, 7)), np.zeros((n, 2, 7))
    for d in range(7):
        add = np.zeros(7)
        add[d] = STEP
        p12, p21 = edge_errors(oplus(add, S), P, K1, K2, ext)
        add[d] = -STEP
        m12, m21 = edge_errors(oplus(add, S), P, K1, K2, ext)
        with np.errstate(all="ignore"):
            J12[:, :, d] = SCALAR * (p12 - m12)
            J21[:, :, d] = SCALAR * (p21 - m21)
    return J12, J21


def _serial(terms):
    return np.cumsum(terms, axis=0)[-1] if len(terms) else np.zeros(terms.shape[1:])


def linearise(S, P, K1, K2, th2, active, ext=False):
    """computeActiveErrors, activeRobustChi2, buildSystem over the active pairs -> dict H [7, 7], b [7], chi2, c12, c21 [n] (of all
    pairs), J12, J21, e12, e21, rho1 [n, 2]."""
    delta = delta_of(th2)
    e12, e21 = edge_errors(S, P, K1, K2, ext)
    w1, w2 = P[:, 10].astype(np.float64), P[:, 11].astype(np.float64)
    c12, c21 = chi2_of(e12, w1), chi2_of(e21, w2)
    J12, J21 = numeric_jacobians(S, P, K1, K2, ext)
    idx = np.flatnonzero(active)
    with np.errstate(all="ignore"):
        # the edges in graph order: e12 and e21 of a pair are adjacent
        e = np.stack([e12[idx], e21[idx]], 1).reshape(-1, 2)
        J = np.stack([J12[idx], J21[idx]], 1).reshape(-1, 2, 7)
        w = np.stack([w1[idx], w2[idx]], 1).reshape(-1)
        c = np.stack([c12[idx], c21[idx]], 1).reshape(-1)
        rho0, rho1 = huber(c, delta)
        wo = rho1 * w
        r0, r1 = -(w * e[:, 0]) * rho1, -(w * e[:, 1]) * rho1
        Ht = (J[:, 0, :, None] * wo[:, None, None]) * J[:, 0, None, :] + (J[:, 1, :, None] * wo[:, None, None]) * J[:, 1, None, :]
        bt = J[:, 0, :] * r0[:, None] + J[:, 1, :] * r1[:, None]
        H, b, chi = _serial(Ht), _serial(bt), float(_serial(rho0)) if len(idx) else 0.0
    return dict(H=H, b=b, chi2=chi, c12=c12, c21=c21, J=J, e=e, w=w, rho1=rho1, abs_H=np.abs(Ht).sum(0), abs_b=np.abs(bt).sum(0), abs_chi2=float(np.abs(rho0).sum()))


def robust_chi2(S, P, K1, K2, th2, active, ext=False):
    delta = delta_of(th2)
    e12, e21 = edge_errors(S, P, K1, K2, ext)
    c12, c21 = chi2_of(e12, P[:, 10].astype(np.float64)), chi2_of(e21, P[:, 11].astype(np.float64))
    idx = np.flatnonzero(active)
    c = np.stack([c12[idx], c21[idx]], 1).reshape(-1)
    rho0, _ = huber(c, delta)
    return (float(_serial(rho0)) if len(idx) else 0.0), c12, c21


def dense_solve(H, lam, b):
    """LinearSolverDense::solve on H + lambda I -> ok, x.  Eigen's LDLT succeeds on a positive (semi-)definite matrix."""
    A = H + lam * np.eye(7)
    if not np.isfinite(A).all() or not np.isfinite(b).all():
        return False, None
    ev = np.linalg.eigvalsh(A)
    if not (ev >= 0).all() or ev.min() == 0:
        return False, None
    return True, np.linalg.solve(A, b)


class Result:
    pass


def optimize(sc, order=None, ext=False):
    """The call on a scene dict (see scene()).  order: a permutation of the pairs -- the sums then run in that order; every output is
    in the caller's order."""
    P = pairs_of(sc)
    n = len(P)
    if order is not None:
        order = np.asarray(order)
        sub = dict(sc)
        for k in ("x1w", "x2w", "obs1", "obs2", "info1", "info2"):
            sub[k] = sc[k][order]
        r = optimize(sub, None, ext)
        inv = np.argsort(order)
        r.removed = r.removed[inv]
        r.checks = [(a[inv], b[inv], live[inv]) for a, b, live in r.checks]
        return r
    K1, K2, th2f = sc["kf1"][2], sc["kf2"][2], float(np.float32(sc["th2"]))
    S0 = sim_from_floats(sc["R12"], sc["t12"], sc["s12"])
    S = S0
    removed, mask = np.zeros(n, bool), np.zeros(n, bool)
    s12, s21 = np.zeros(n), np.zeros(n)        # chi2 of each edge's stored _error
    res = Result()
    res.lin, res.trials, res.checks = [], [], []
    n_bad, more, n_in, early, lam = 0, 0, 0, False, 0.0
    for rnd in range(2):
        active = ~removed
        its = 5 if rnd == 0 else more
        if active.any():                        # else initializeOptimization finds no vertex and optimize() returns at once
            ni, stalled, x = 2.0, 0, np.zeros(7)
            for it in range(its):
                L = linearise(S, P, K1, K2, th2f, active, ext)
                s12[active], s21[active] = L["c12"][active], L["c21"][active]   # linearizeOplus restores _error
                cur = ini = L["chi2"]
                if it == 0:
                    mx = 0.0
                    for j in range(7):          # std::max(fabs(h), maxDiagonal)
                        f = abs(L["H"][j, j])
                        mx = mx if f < mx else f
                    lam, ni, stalled = 1e-5 * mx, 2.0, 0
                li = len(res.lin)
                res.lin.append(dict(round=rnd, iteration=it, H=L["H"], b=L["b"], chi2=L["chi2"], S=S, active=active.copy(), L=L))
                rho, qmax = 0.0, 0
                while True:
                    backup = S
                    ok, sol = dense_solve(L["H"], lam, L["b"])
                    if ok:
                        x = sol
                    S = oplus(x, S)
                    tmp, c12, c21 = robust_chi2(S, P, K1, K2, th2f, active, ext)
                    s12[active], s21[active] = c12[active], c21[active]
                    if not ok:
                        tmp = DBL_MAX
                    scale = 0.0
                    for j in range(7):
                        scale += x[j] * (lam * x[j] + L["b"][j])
                    scale += 1e-3
                    with np.errstate(all="ignore"):
                        rho = float((np.float64(cur) - np.float64(tmp)) / np.float64(scale))
                    accept = rho > 0 and math.isfinite(tmp)
                    res.trials.append(dict(lin=li, ok=ok, accepted=accept, lam=lam, cur=cur, tmp=tmp, scale=scale, rho=rho, dx=x.copy(),
                                           margin=abs(cur - tmp), S=S, S0=backup))
                    if accept:
                        alpha = 1.0 - math.pow(2 * rho - 1, 3)
                        alpha = min(alpha, 2.0 / 3.0)
                        lam *= max(1.0 / 3.0, alpha)
                        ni = 2.0
                        cur = tmp
                    else:
                        lam *= ni
                        ni *= 2
                        S = backup
                    qmax += 1
                    if not (rho < 0 and qmax < 10):
                        break
                if qmax == 10 or rho == 0:
                    break
                stalled = stalled + 1 if (ini - cur) * 1e3 < ini else 0
                if stalled >= 3:
                    break
        with np.errstate(all="ignore"):
            bad = active & ((s12 > th2f) | (s21 > th2f))
        res.checks.append((s12.copy(), s21.copy(), active.copy()))
        mask |= bad
        if rnd == 0:
            removed = bad.copy()
            n_bad = int(bad.sum())
            more = 10 if n_bad > 0 else 5
            if n - n_bad < 10:
                early, more = True, 0
                break
        else:
            n_in = int((active & ~bad).sum())
    res.S = S0 if early else S
    res.R12, res.t12, res.scale = rot_of(res.S.q).astype(np.float32), res.S.t.astype(np.float32), np.float32(res.S.s)
    res.n_inliers, res.n_correspondences, res.n_bad, res.more_iterations, res.early = (0 if early else n_in), n, n_bad, more, early
    res.removed = mask.astype(np.uint8)
    return res


def not_finite(res):
    return not np.isfinite(res.S.vec()).all() or any(not np.isfinite(l["chi2"]) for l in res.lin)


# ---- scenes ----------------------------------------------------------------------------------------------------------------------------
def rot_of_vec(v):
    th = float(np.linalg.norm(v))
    if th == 0:
        return np.eye(3)
    k = np.asarray(v) / th
    Kx = skew(k)
    return np.eye(3) + math.sin(th) * Kx + (1 - math.cos(th)) * Kx @ Kx


def scene(seed, n, shifted2=0, shift=8.0, gross=0, garbage=False, zero_z=False, sigma_step=None, octave=None, noise=0.3,
          off=(0.03, 0.05, 0.03), th2=TH2):
    """n pairs of map points: X1c = s R X2c + t for a true similarity, seen in key frame 1 and key frame 2 with `noise` px times the level's
    sigma, at pyramid levels 0..3 (octave: all at that level).  info1 = 1 / sigma1^2 (GetInvSigma2), info2 = sigma2^2 (GetSigma2, as the
    reference passes it).  The start is `off` = (rad, m, log scale) away from the truth.
    shifted2: the first `shifted2` observations in image 2 moved by `shift` / sigma2 px, which costs e21 a chi2 of shift^2 and e12 nothing;
    gross: further pairs with both observations moved by 40..80 px; garbage: every observation a random pixel;
    sigma_step: no noise, the start exact but for the scale, which is off by exp(-sigma_step): the first step's sigma is that;
    zero_z: key frame 2 at the origin, the start rotation the identity and scale 1, pair 0's X2c put where the start maps it to z = 0.
    -> dict x1w, x2w, obs1, obs2, info1, info2, kf1 = (Rcw, tcw, K), kf2, R12, t12, s12, th2: all float32."""
    g = np.random.default_rng(seed)
    K1, K2 = K1_DEFAULT, K2_DEFAULT
    R_true = np.eye(3) if zero_z else rot_of_vec(g.normal(size=3) * 0.1)
    t_true, s_true = g.normal(size=3) * 0.3, float(np.exp(g.normal() * 0.1))
    if zero_z:
        s_true = 1.0
    R_true32, t_true32, s_true32 = R_true.astype(np.float32), t_true.astype(np.float32), np.float32(s_true)
    X2c = np.stack([g.uniform(-3, 3, n), g.uniform(-2, 2, n), g.uniform(3, 9, n)], 1)
    X1c = float(s_true32) * X2c @ R_true32.astype(np.float64).T + t_true32.astype(np.float64)
    R1w, t1w = rot_of_vec(g.normal(size=3) * 0.3), g.normal(size=3)
    R2w, t2w = (np.eye(3), np.zeros(3)) if zero_z else (rot_of_vec(g.normal(size=3) * 0.3), g.normal(size=3))
    lvl1, lvl2 = g.integers(0, 4, n), g.integers(0, 4, n)
    if octave is not None:
        lvl1[:], lvl2[:] = octave, octave
    sig1, sig2 = np.float32(1.2) ** lvl1, np.float32(1.2) ** lvl2
    nz = 0.0 if sigma_step is not None else noise
    obs1 = np.stack([K1[0] * X1c[:, 0] / X1c[:, 2] + K1[2], K1[1] * X1c[:, 1] / X1c[:, 2] + K1[3]], 1) + g.normal(size=(n, 2)) * nz * sig1[:, None]
    obs2 = np.stack([K2[0] * X2c[:, 0] / X2c[:, 2] + K2[2], K2[1] * X2c[:, 1] / X2c[:, 2] + K2[3]], 1) + g.normal(size=(n, 2)) * nz * sig2[:, None]
    if shifted2:
        ang = g.uniform(0, 2 * math.pi)
        obs2[:shifted2] += shift / sig2[:shifted2, None] * np.array([math.cos(ang), math.sin(ang)])
    if gross:
        obs1[shifted2:shifted2 + gross] += g.uniform(40, 80, (gross, 2)) * g.choice([-1, 1], (gross, 2))
        obs2[shifted2:shifted2 + gross] += g.uniform(40, 80, (gross, 2)) * g.choice([-1, 1], (gross, 2))
    if garbage:
        obs1 = np.stack([g.uniform(0, 752, n), g.uniform(0, 480, n)], 1)
        obs2 = np.stack([g.uniform(0, 752, n), g.uniform(0, 480, n)], 1)
    x1w = ((X1c - t1w) @ R1w).astype(np.float32)
    x2w = ((X2c - t2w) @ R2w).astype(np.float32)
    if sigma_step is not None:
        R0, t0, s0 = R_true32, t_true32, np.float32(float(s_true32) * math.exp(-sigma_step))
    elif zero_z:
        dt = g.normal(size=3)
        R0, t0, s0 = np.eye(3, dtype=np.float32), (t_true + dt / np.linalg.norm(dt) * 0.01).astype(np.float32), np.float32(1.0)
        if n:
            x2w[0, 2] = -t0[2]     # key frame 2 is at the origin: X2c = x2w, and 1 * X2c.z + t.z = 0 exactly
    else:
        dv, dt = g.normal(size=3), g.normal(size=3)
        R0 = (rot_of_vec(dv / np.linalg.norm(dv) * off[0]) @ R_true).astype(np.float32)
        t0 = (t_true + dt / np.linalg.norm(dt) * off[1]).astype(np.float32)
        s0 = np.float32(s_true * math.exp(off[2]))
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    return dict(x1w=f32(x1w), x2w=f32(x2w), obs1=f32(obs1), obs2=f32(obs2), info1=f32(1.0 / (sig1 * sig1)), info2=f32(sig2 * sig2),
                kf1=(f32(R1w), f32(t1w), tuple(np.float32(v) for v in K1)), kf2=(f32(R2w), f32(t2w), tuple(np.float32(v) for v in K2)),
                R12=f32(R0), t12=f32(t0), s12=np.float32(s0), th2=np.float32(th2))


# name -> scene arguments.  The plain ones cover the sizes at which the reduction shape changes; the named ones are the special cases.
SCENES = {}
for _i, _n in enumerate((10, 11, 30, 63, 64, 65, 100, 255, 256, 257, 300, 513)):
    SCENES["plain_%d" % _n] = dict(seed={64: 150}.get(_n, 100 + _i), n=_n)  # nBad == 0: 5 more iterations (seed 104 has |t12| = 0.06: scale barely observable)
for _i, _n in enumerate((30, 60, 100, 150, 300)):
    SCENES["shift_%d" % _n] = dict(seed=200 + _i, n=_n, shifted2=_n // 5)    # bad through e21 alone; nBad > 0: 10 more iterations
for _i, _n in enumerate((40, 100, 257)):
    SCENES["gross_%d" % _n] = dict(seed=300 + _i, n=_n, gross=_n // 5)
SCENES["left_10"] = dict(seed=400, n=14, gross=4)                            # exactly 10 pairs left: the second round runs
SCENES["left_9"] = dict(seed=401, n=13, gross=4)                             # exactly 9 left: the early return
SCENES["all_bad_12"] = dict(seed=402, n=12, garbage=True)                    # every pair bad
SCENES["none_0"] = dict(seed=403, n=0)                                       # optimize(5) on an empty graph, then return 0
SCENES["sigma_below"] = dict(seed=405, n=40, sigma_step=0.8e-5)              # the first step's |sigma| just below eps = 1e-5
SCENES["sigma_above"] = dict(seed=405, n=40, sigma_step=1.25e-5)             # and just above
SCENES["zero_z_30"] = dict(seed=406, n=30, zero_z=True)                      # pair 0 maps to z = 0: its chi2 is NaN, it stays and counts
SCENES["octave3_60"] = dict(seed=407, n=60, octave=3, noise=0.2)             # info2 / info1 = 1.2^12 on every pair
SCENES["octave3_shift_60"] = dict(seed=408, n=60, octave=3, noise=0.2, shifted2=10, shift=12.0)
E21_ONLY = ("shift_30", "shift_60", "shift_100", "shift_150", "shift_300")


def make(name):
    return scene(**SCENES[name])


def dump(path):
    """The scene list as the stand-alone host build reads it (tests/golden/sim3opt_scenes.bin): int32 count; per scene int32 n, float
    th2, K1[4], K2[4], R12[9], t12[3], s12, then the pairs [n][12] as the library gathers them."""
    with open(path, "wb") as f:
        f.write(np.int32(len(SCENES)).tobytes())
        for name in SCENES:
            sc = make(name)
            P = pairs_of(sc)
            head = np.concatenate([[sc["th2"]], sc["kf1"][2], sc["kf2"][2], sc["R12"].reshape(9), sc["t12"], [sc["s12"]]]).astype(np.float32)
            f.write(np.int32(len(P)).tobytes() + head.tobytes() + np.ascontiguousarray(P, np.float32).tobytes())


def load(path):
    """-> [(pairs [n, 12], th2, K1, K2, R12, t12, s12)] in SCENES' order."""
    raw, out = open(path, "rb").read(), []
    off = 4
    for _ in range(int(np.frombuffer(raw, np.int32, 1)[0])):
        n = int(np.frombuffer(raw, np.int32, 1, off)[0])
        h = np.frombuffer(raw, np.float32, 22, off + 4)
        P = np.frombuffer(raw, np.float32, 12 * n, off + 92).reshape(n, 12)
        out.append((P.copy(), h[0], h[1:5].copy(), h[5:9].copy(), h[9:18].reshape(3, 3).copy(), h[18:21].copy(), h[21]))
        off += 92 + 48 * n
    return out


if __name__ == "__main__":
    import sys
    dump(sys.argv[1])
