"""Optimizer::PoseOptimization(Frame*) restated in numpy from the reference's sources (src/Optimizer.cc:2012-2145, src/Converter.cc:76-92
and, of g2o: optimization_algorithm_levenberg.cpp:61-190, sparse_optimizer.cpp:354-419, base_binary_edge.hpp:55-120, base_edge.h:96-102,
robust_kernel_impl.cpp (Huber), types_six_dof_expmap.{h,cpp}, se3quat.h, linear_solver_dense.h:65-113) -- not from csrc/poseopt_core.hpp.
Where the library departs, the model keeps the reference: sums over edges are SERIAL in edge order (np.cumsum), the 6 x 6 system goes
to numpy.linalg.solve, sin and cos are math.sin / math.cos, pow is math.pow.  The pose state is a unit quaternion (x y z w) and a
translation in double.

Besides the result the model returns what the checks need to bound rounding (tests/poseopt_checks.py): the sum of absolute terms of
every sum, cond(H + lambda I) of every solve, and every decision margin (|cur - tmp| per trial, |chi2 - th| per edge and round).

Eigen is recalled, not read [EIGEN-RECALL]: Quaternion(Matrix3) (the trace branch and the three largest-diagonal branches),
toRotationMatrix, quaternion * vector as v + w (2 q x v) + q x (2 q x v), the Hamilton product, normalize() as coeffs / norm()."""
import math

import numpy as np

ITS = (10, 10, 7, 5)
CHI2 = tuple(float(np.float32(v)) for v in (9.210, 7.378, 5.991, 5.991))   # const float chi2[4]
DELTA = float(np.float32(math.sqrt(5.991)))                                # const float delta = sqrt(5.991)
DSQR = DELTA * DELTA
K_DEFAULT = (458.654, 457.296, 367.215, 248.375)
DBL_MAX = float(np.finfo(np.float64).max)


# ---- SE3Quat ---------------------------------------------------------------------------------------------------------------------------
def normalize_rotation(q):
    q = np.array(q, np.float64)
    if q[3] < 0:
        q = q * -1.0
    return q / math.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])


def quat_of(R):
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
        j = (i + 1) % 3
        k = (j + 1) % 3
        t = math.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0)
        q[i] = 0.5 * t
        t = 0.5 / t
        q[3] = (R[k, j] - R[j, k]) * t
        q[j] = (R[j, i] + R[i, j]) * t
        q[k] = (R[k, i] + R[i, k]) * t
    return q


def rotation_of(q):
    x, y, z, w = q
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.array([[1.0 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1.0 - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, 1.0 - (txx + tyy)]])


def rotate(q, v):
    """q * v for one vector or an [n, 3] array of them."""
    v = np.asarray(v, np.float64)
    v0, v1, v2 = v[..., 0], v[..., 1], v[..., 2]
    u0, u1, u2 = q[1] * v2 - q[2] * v1, q[2] * v0 - q[0] * v2, q[0] * v1 - q[1] * v0
    u0, u1, u2 = u0 + u0, u1 + u1, u2 + u2
    return np.stack([(v0 + q[3] * u0) + (q[1] * u2 - q[2] * u1), (v1 + q[3] * u1) + (q[2] * u0 - q[0] * u2), (v2 + q[3] * u2) + (q[0] * u1 - q[1] * u0)], -1)


def pose_of(Tcw):
    """Converter::toSE3Quat on the float matrix -> (q, t)."""
    T = np.asarray(Tcw, np.float32).reshape(4, 4).astype(np.float64)
    return normalize_rotation(quat_of(T[:3, :3])), T[:3, 3].copy()


def matrix_of(q, t):
    """Converter::toCvMat(SE3Quat) -> float32 [4, 4], and R in double."""
    R = rotation_of(q)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T.astype(np.float32), R


def se3_exp(dx):
    om, up = np.asarray(dx[:3], np.float64), np.asarray(dx[3:], np.float64)
    theta = math.sqrt(om[0] * om[0] + om[1] * om[1] + om[2] * om[2])
    Om = np.array([[0.0, -om[2], om[1]], [om[2], 0.0, -om[0]], [-om[1], om[0], 0.0]])
    Om2 = np.zeros((3, 3))
    for i in range(3):
        for j in range(3):
            Om2[i, j] = (Om[i, 0] * Om[0, j] + Om[i, 1] * Om[1, j]) + Om[i, 2] * Om[2, j]
    I = np.eye(3)
    if theta < 0.00001:
        R = (I + Om) + Om2
        V = R
    else:
        R = (I + math.sin(theta) / theta * Om) + (1.0 - math.cos(theta)) / (theta * theta) * Om2
        V = (I + (1.0 - math.cos(theta)) / (theta * theta) * Om) + (theta - math.sin(theta)) / math.pow(theta, 3) * Om2
    t = np.array([(V[i, 0] * up[0] + V[i, 1] * up[1]) + V[i, 2] * up[2] for i in range(3)])
    return normalize_rotation(quat_of(R)), t


def oplus(dx, q, t):
    """VertexSE3Expmap::oplusImpl: exp(dx) * estimate."""
    a, ta = se3_exp(dx)
    tn = ta + rotate(a, t)
    b = q
    w = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]
    x = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1]
    y = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2]
    z = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0]
    with np.errstate(all="ignore"):
        return normalize_rotation([x, y, z, w]), tn


# ---- edges -----------------------------------------------------------------------------------------------------------------------------
def huber(e):
    """RobustKernelHuber::robustify -> rho[0], rho[1] (arrays)."""
    e = np.asarray(e, np.float64)
    with np.errstate(all="ignore"):
        sq = np.sqrt(e)
        out = ~(e <= DSQR)
        rho0 = np.where(out, 2.0 * sq * DELTA - DSQR, e)
        rho1 = np.where(out, DELTA / sq, 1.0)
    return rho0, rho1


def edge_eval(q, t, K, p3d, p2d, w):
    """computeError and chi2 of every edge -> dict of arrays."""
    fx, fy, cx, cy = [float(np.float32(v)) for v in K]
    with np.errstate(all="ignore"):
        pc = rotate(q, np.asarray(p3d, np.float32).astype(np.float64)) + t
        x, y, z = pc[:, 0], pc[:, 1], pc[:, 2]
        obs = np.asarray(p2d, np.float32).astype(np.float64)
        e0 = obs[:, 0] - ((x / z) * fx + cx)
        e1 = obs[:, 1] - ((y / z) * fy + cy)
        wd = np.asarray(w, np.float32).astype(np.float64)
        chi2 = e0 * (wd * e0 + 0.0 * e1) + e1 * (0.0 * e0 + wd * e1)   # _error.dot(information * _error), the zeros of information included
    return dict(x=x, y=y, z=z, e0=e0, e1=e1, w=wd, chi2=chi2)


def jacobian(ev, K):
    """EdgeSE3ProjectXYZ::linearizeOplus, _jacobianOplusXj -> [n, 2, 6]."""
    fx, fy = float(np.float32(K[0])), float(np.float32(K[1]))
    x, y, z = ev["x"], ev["y"], ev["z"]
    with np.errstate(all="ignore"):
        z_2 = z * z
        J = np.zeros((len(x), 2, 6))
        J[:, 0, 0] = x * y / z_2 * fx
        J[:, 0, 1] = -(1.0 + (x * x / z_2)) * fx
        J[:, 0, 2] = y / z * fx
        J[:, 0, 3] = -1.0 / z * fx
        J[:, 0, 5] = x / z_2 * fx
        J[:, 1, 0] = (1.0 + y * y / z_2) * fy
        J[:, 1, 1] = -x * y / z_2 * fy
        J[:, 1, 2] = -x / z * fy
        J[:, 1, 4] = -1.0 / z * fy
        J[:, 1, 5] = y / z_2 * fy
    return J


def _serial(terms):
    """Sum over axis 0 in index order."""
    return np.cumsum(terms, axis=0)[-1] if len(terms) else np.zeros(terms.shape[1:])


def linearise(q, t, K, p3d, p2d, w, active):
    """computeActiveErrors, activeRobustChi2, buildSystem over the active edges in index order.  -> dict: H [6, 6], b [6], chi2, the
    per-edge evaluation, and abs_H, abs_b, abs_chi2: the sums of the absolute terms."""
    ev = edge_eval(q, t, K, p3d, p2d, w)
    idx = np.flatnonzero(active)
    with np.errstate(all="ignore"):
        rho0, rho1 = huber(ev["chi2"][idx])
        J = jacobian(ev, K)[idx]
        wo = rho1 * ev["w"][idx]                       # robustInformation: rho[1] * information
        r0 = -(ev["w"][idx] * ev["e0"][idx]) * rho1    # omega_r = -omega * error; omega_r *= rho[1]
        r1 = -(ev["w"][idx] * ev["e1"][idx]) * rho1
        Ht = (J[:, 0, :, None] * wo[:, None, None]) * J[:, 0, None, :] + (J[:, 1, :, None] * wo[:, None, None]) * J[:, 1, None, :]
        bt = J[:, 0, :] * r0[:, None] + J[:, 1, :] * r1[:, None]
        H, b, chi = _serial(Ht), _serial(bt), float(_serial(rho0)) if len(idx) else 0.0
        out = dict(H=H, b=b, chi2=chi, ev=ev, abs_H=np.abs(Ht).sum(0), abs_b=np.abs(bt).sum(0), abs_chi2=float(np.abs(rho0).sum()))
    return out


def robust_chi2(q, t, K, p3d, p2d, w, active):
    ev = edge_eval(q, t, K, p3d, p2d, w)
    idx = np.flatnonzero(active)
    with np.errstate(all="ignore"):
        rho0, _ = huber(ev["chi2"][idx])
        return (float(_serial(rho0)) if len(idx) else 0.0), ev, float(np.abs(rho0).sum())


def dense_solve(H, lam, b):
    """LinearSolverDense::solve on H + lambda I -> ok, x, cond.  Eigen's LDLT succeeds on a positive (semi-)definite matrix."""
    A = H + lam * np.eye(6)
    if not np.isfinite(A).all() or not np.isfinite(b).all():
        return False, None, float("inf")
    ev = np.linalg.eigvalsh(A)
    if not (ev >= 0).all() or ev.min() == 0:
        return False, None, float("inf")
    return True, np.linalg.solve(A, b), float(np.linalg.cond(A))


class Result:
    pass


def optimize(p3d, p2d, w, K, Tcw, order=None):
    """The call.  order: a permutation of the edges -- the sums then run in that order; every output is in the caller's order."""
    p3d, p2d, w = np.asarray(p3d, np.float32).reshape(-1, 3), np.asarray(p2d, np.float32).reshape(-1, 2), np.asarray(w, np.float32).reshape(-1)
    n = len(p3d)
    if order is not None:
        order = np.asarray(order)
        r = optimize(p3d[order], p2d[order], w[order], K, Tcw)
        inv = np.argsort(order)
        r.outlier = r.outlier[inv]
        r.class_chi2 = [c[inv] for c in r.class_chi2]
        r.flags = [f[inv] for f in r.flags]
        return r
    q, t = pose_of(Tcw)
    level, flag = np.zeros(n, bool), np.zeros(n, bool)
    stored = np.zeros(n)                # chi2 of each edge's stored _error
    res = Result()
    res.lin, res.trials, res.class_chi2, res.flags, res.active_after = [], [], [], [], []
    n_bad, lam, rounds = 0, 0.0, 0
    for rnd in range(4):
        rounds = rnd + 1
        active = ~level
        if active.any():                # else initializeOptimization finds no vertex and optimize() returns at once
            ni, stalled, x = 2.0, 0, np.zeros(6)
            for it in range(ITS[rnd]):
                L = linearise(q, t, K, p3d, p2d, w, active)
                stored[active] = L["ev"]["chi2"][active]
                cur = ini = L["chi2"]
                if it == 0:
                    mx = 0.0
                    for j in range(6):  # std::max(fabs(h), maxDiagonal)
                        f = abs(L["H"][j, j])
                        mx = mx if f < mx else f
                    lam, ni, stalled = 1e-5 * mx, 2.0, 0
                li = len(res.lin)
                res.lin.append(dict(round=rnd, iteration=it, H=L["H"], b=L["b"], chi2=L["chi2"], abs_H=L["abs_H"], abs_b=L["abs_b"], abs_chi2=L["abs_chi2"],
                                    q=q.copy(), t=t.copy(), active=active.copy()))
                rho, qmax = 0.0, 0
                while True:
                    backup = (q, t)
                    ok, sol, cond = dense_solve(L["H"], lam, L["b"])
                    if ok:
                        x = sol
                    q, t = oplus(x, q, t)
                    tmp, ev, abs_tmp = robust_chi2(q, t, K, p3d, p2d, w, active)
                    stored[active] = ev["chi2"][active]
                    if not ok:
                        tmp = DBL_MAX
                    scale = 0.0
                    for j in range(6):
                        scale += x[j] * (lam * x[j] + L["b"][j])
                    scale += 1e-3
                    with np.errstate(all="ignore"):
                        rho = float((np.float64(cur) - np.float64(tmp)) / np.float64(scale))
                    accept = rho > 0 and math.isfinite(tmp)
                    res.trials.append(dict(lin=li, ok=ok, accepted=accept, lam=lam, cur=cur, tmp=tmp, scale=scale, rho=rho, cond=cond, dx=x.copy(),
                                           margin=abs(cur - tmp), abs_tmp=abs_tmp, q=q.copy(), t=t.copy(), q0=backup[0].copy(), t0=backup[1].copy()))
                    if accept:
                        alpha = 1.0 - math.pow(2 * rho - 1, 3)
                        alpha = min(alpha, 2.0 / 3.0)
                        lam *= max(1.0 / 3.0, alpha)
                        ni = 2.0
                        cur = tmp
                    else:
                        lam *= ni
                        ni *= 2
                        q, t = backup
                    qmax += 1
                    if not (rho < 0 and qmax < 10):
                        break
                if qmax == 10 or rho == 0:
                    break
                stalled = stalled + 1 if (ini - cur) * 1e3 < ini else 0
                if stalled >= 3:
                    break
        # classification
        if flag.any():
            ev = edge_eval(q, t, K, p3d, p2d, w)
            stored[flag] = ev["chi2"][flag]
        th = CHI2[rnd]
        with np.errstate(all="ignore"):
            gt, le = stored > th, stored <= th
        flag = np.where(gt, True, np.where(le, False, flag))
        level = np.where(gt, True, np.where(le, False, level))
        n_bad = int(gt.sum())
        res.class_chi2.append(stored.copy())
        res.flags.append(flag.copy())
        res.active_after.append(int((~level).sum()))
        if n < 10:                      # optimizer.edges().size() < 10: ALL edges
            break
    res.Tcw, res.R = matrix_of(q, t)
    res.q, res.t = q, t
    res.n_inliers, res.rounds, res.outlier = n - n_bad, rounds, flag.astype(np.uint8)
    return res


def min_class_margin(res):
    """The smallest |chi2 - th| over all edges and rounds run (inf without edges; NaN entries ignored: they decide nothing)."""
    m = float("inf")
    for rnd, c in enumerate(res.class_chi2):
        d = np.abs(c - CHI2[rnd])
        d = d[np.isfinite(d)]
        if len(d):
            m = min(m, float(d.min()))
    return m


def reentries(res):
    """Edges flagged after one round and not flagged after a later one."""
    was = np.zeros(len(res.outlier), bool)
    back = np.zeros(len(res.outlier), bool)
    for f in res.flags:
        back |= was & ~f
        was |= f
    return int(back.sum())


# ---- scenes ----------------------------------------------------------------------------------------------------------------------------
def rot_of_vec(v):
    th = float(np.linalg.norm(v))
    if th == 0:
        return np.eye(3)
    k = np.asarray(v) / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(th) * Kx + (1 - math.cos(th)) * Kx @ Kx


def scene(seed, n, shifted=0, shift=None, gross=0, garbage=False, plane=False, off=(0.04, 0.08), K=K_DEFAULT):
    """n map points seen by a camera, observed with half a pixel of noise at pyramid levels 0..3, and a start pose `off` = (rad, m)
    away from the true one.  shifted: the first `shifted` observations moved by a common `shift` px (default drawn from 5..8);
    gross: further observations moved by 40..80 px; garbage: every observation replaced by a random pixel; plane: point 0 is moved onto
    the camera plane of the start pose exactly ("exact"; true and start rotation are then the identity).  -> (p3d, p2d, inv_sigma2, K, Tcw0) in float32."""
    g = np.random.default_rng(seed)
    Rt, tt = rot_of_vec(g.normal(size=3) * (0.0 if plane == "exact" else 0.2)), g.normal(size=3) * 0.5
    pc = np.stack([g.uniform(-3, 3, n), g.uniform(-2, 2, n), g.uniform(2, 10, n)], 1)
    pw = (pc - tt) @ Rt                              # Rt^T (pc - tt)
    lvl = g.integers(0, 4, n)
    sig = 1.2 ** lvl
    uv = np.stack([K[0] * pc[:, 0] / pc[:, 2] + K[2], K[1] * pc[:, 1] / pc[:, 2] + K[3]], 1) + g.normal(size=(n, 2)) * 0.5 * sig[:, None]
    if shifted:
        s = g.uniform(5, 8) if shift is None else shift
        ang = g.uniform(0, 2 * math.pi)
        uv[:shifted] += s * np.array([math.cos(ang), math.sin(ang)])
    if gross:
        uv[shifted:shifted + gross] += g.uniform(40, 80, (gross, 2)) * g.choice([-1, 1], (gross, 2))
    if garbage:
        uv = np.stack([g.uniform(0, 752, n), g.uniform(0, 480, n)], 1)
    dv = g.normal(size=3)
    dR = rot_of_vec(dv / np.linalg.norm(dv) * (0.0 if plane == "exact" else off[0]))
    dt = g.normal(size=3)
    dt = dt / np.linalg.norm(dt) * off[1]
    T0 = np.eye(4)
    T0[:3, :3], T0[:3, 3] = dR @ Rt, dR @ tt + dt
    T0 = T0.astype(np.float32)
    pw = pw.astype(np.float32)
    if plane == "exact" and n:
        # the start rotation is the identity, which the quaternion product applies exactly: z_c = -t[2] + t[2] = 0, x / z = +-inf, and
        # chi2 = NaN through information's zeros
        pw[0, 2] = -T0[2, 3]
    return pw, uv.astype(np.float32), (1.0 / (sig * sig)).astype(np.float32), tuple(np.float32(v) for v in K), T0


# name -> scene arguments.  The plain ones cover the sizes at which the reduction shape changes; the named ones are the special cases.
SCENES = {}
FAR = (0.5, 1.2)    # a start this far off keeps the Levenberg decisions well clear of rounding for five trials and more
for _i, _n in enumerate((10, 11, 30, 63, 64, 65, 100, 150, 255, 256, 257, 300, 513, 1000)):
    SCENES["plain_%d" % _n] = dict(seed={65: 521, 257: 520, 300: 504, 513: 508, 1000: 503}.get(_n, 100 + _i), n=_n, off=FAR)
for _i, _n in enumerate((30, 60, 100, 100, 100, 150, 200, 300)):
    SCENES["shift_%d_%d" % (_n, _i)] = dict(seed=200 + _i, n=_n, shifted=_n // 3)
for _i, _n in enumerate((40, 100, 257, 600)):
    SCENES["gross_%d" % _n] = dict(seed=300 + _i, n=_n, gross=_n // 5, off=FAR)
SCENES["few_1"] = dict(seed=403, n=1, off=(0.8, 2.0))
SCENES["few_5"] = dict(seed=402, n=5, off=FAR)
SCENES["few_9"] = dict(seed=403, n=9, gross=2)                       # N < 10: one round
SCENES["thin_12"] = dict(seed=404, n=12, gross=5)                    # N >= 10, fewer than 10 active after round 0: four rounds all the same
SCENES["none_left_12"] = dict(seed=600, n=12, garbage=True)          # every edge flagged after round 0
SCENES["plane_exact_50"] = dict(seed=407, n=50, plane="exact")       # exactly: its chi2 is NaN and so is every sum
REENTRY = ("shift_100_2", "shift_150_5")                            # a correspondence flagged in one round comes back in a later one


def make(name):
    return scene(**SCENES[name])


def dump(path):
    """The scene list as the stand-alone host build reads it (tests/golden/poseopt_scenes.bin): int32 count; per scene int32 n,
    float K[4], float Tcw[16], float edges[n][6] (point, observation, invSigma2)."""
    with open(path, "wb") as f:
        f.write(np.int32(len(SCENES)).tobytes())
        for name in SCENES:
            p3d, p2d, w, K, Tcw = make(name)
            f.write(np.int32(len(p3d)).tobytes() + np.asarray(K, np.float32).tobytes() + np.ascontiguousarray(Tcw, np.float32).tobytes())
            f.write(np.ascontiguousarray(np.concatenate([p3d, p2d, w[:, None]], 1), np.float32).tobytes())


def load(path):
    """-> [(p3d, p2d, inv_sigma2, K, Tcw)] in SCENES' order."""
    raw, out = open(path, "rb").read(), []
    off = 4
    for _ in range(int(np.frombuffer(raw, np.int32, 1)[0])):
        n = int(np.frombuffer(raw, np.int32, 1, off)[0])
        K, T = np.frombuffer(raw, np.float32, 4, off + 4), np.frombuffer(raw, np.float32, 16, off + 20).reshape(4, 4)
        e = np.frombuffer(raw, np.float32, 6 * n, off + 84).reshape(n, 6)
        out.append((e[:, :3].copy(), e[:, 3:5].copy(), e[:, 5].copy(), tuple(K), T.copy()))
        off += 84 + 24 * n
    return out


if __name__ == "__main__":
    import sys
    dump(sys.argv[1])
