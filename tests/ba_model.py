"""Optimizer::LocalBundleAdjustment (src/Optimizer.cc:2147-2405 of the reference) and Optimizer::BundleAdjustment (:1896-2010) restated in
numpy from the reference's files: the graph and the two checks from Optimizer.cc, the edge from
Thirdparty/g2o/g2o/types/types_six_dof_expmap.cpp:103-147 (computeError in the header: obs - cam_project(T.map(X))), the Schur
complement from g2o/core/block_solver.hpp:354-486 and :502-590, the driver from g2o/core/optimization_algorithm_levenberg.cpp, SE3Quat
and the Huber kernel from tests/poseopt_model.py (the same g2o files).

Sums are serial in edge order (numpy.add.at adds in the order of its index list), Dinv is numpy.linalg.inv, the reduced system goes
through numpy.linalg.solve over the key frames that have an active edge, sin and cos are math's.  `order` permutes the order in which
the edges are added, `solver` exchanges the reduced solve ("solve", "cholesky", "ldl"): the spread of the answers under both is what
tests/ba_checks.py measures its tolerances on."""
import math
import struct

import numpy as np

import poseopt_model as pom

LOCAL, FULL = 0, 1
TH = 5.991
DBL_MAX = pom.DBL_MAX
CAM = (458.654, 457.296, 367.215, 248.375)


def arrays(sc):
    """The scene's arrays in the library's types, and every edge's point."""
    f32, i32, u8 = np.float32, np.int32, np.uint8
    a = dict(T=np.asarray(sc["Tcw"], f32).reshape(-1, 12), fixed=np.asarray(sc["fixed"], u8), pts=np.asarray(sc["points"], f32).reshape(-1, 3),
             begin=np.asarray(sc["begin"], i32), ekf=np.asarray(sc["edge_kf"], i32), obs=np.asarray(sc["edge_obs"], f32).reshape(-1, 2),
             w=np.asarray(sc["edge_inv_sigma2"], f32), ecam=np.asarray(sc["edge_camera"], i32), cams=np.asarray(sc["cameras"], f32).reshape(-1, 4))
    P = len(a["pts"])
    a["bad"] = np.zeros(P, u8) if sc.get("point_bad") is None else np.asarray(sc["point_bad"], u8)
    a["ept"] = np.repeat(np.arange(P, dtype=i32), np.diff(a["begin"]))
    free = np.cumsum(a["fixed"] == 0) - 1
    a["kf_free"] = np.where(a["fixed"] == 0, free, -1).astype(i32)
    a["F"] = int((a["fixed"] == 0).sum())
    return a


def start(a):
    """Converter::toSE3Quat per key frame -> est [K, 7] (q x y z w, t); the points widened."""
    est = np.zeros((len(a["T"]), 7))
    for k, T in enumerate(a["T"]):
        M = np.eye(4, dtype=np.float32)
        M[:3, :] = T.reshape(3, 4)
        q, t = pom.pose_of(M)
        est[k, :4], est[k, 4:] = q, t
    return est, a["pts"].astype(np.float64)


def rotate_each(q, v):
    """q[e] * v[e]: Eigen's quaternion * vector, edge by edge."""
    u = 2.0 * np.cross(q[:, :3], v)
    return v + q[:, 3:4] * u + np.cross(q[:, :3], u)


def rotations(q):
    """toRotationMatrix() of each quaternion [n, 4] -> [n, 3, 3]."""
    return np.stack([pom.rotation_of(x) for x in q]) if len(q) else np.zeros((0, 3, 3))


def edge_errors(a, est, X):
    """computeError of every edge: the point in the camera [E, 3], the error [E, 2], chi2 [E]."""
    q, t = est[a["ekf"], :4], est[a["ekf"], 4:]
    with np.errstate(all="ignore"):
        pc = rotate_each(q, X[a["ept"]]) + t
        c = a["cams"][a["ecam"]].astype(np.float64)
        proj = np.stack([pc[:, 0] / pc[:, 2] * c[:, 0] + c[:, 2], pc[:, 1] / pc[:, 2] * c[:, 1] + c[:, 3]], 1)
        err = a["obs"].astype(np.float64) - proj
        w = a["w"].astype(np.float64)
        chi2 = w * err[:, 0] * err[:, 0] + w * err[:, 1] * err[:, 1]
    return pc, err, chi2


def jacobians(a, est, pc):
    """linearizeOplus: _jacobianOplusXj [E, 2, 6] (the pose) and _jacobianOplusXi [E, 2, 3] (the point)."""
    E = len(pc)
    c = a["cams"][a["ecam"]].astype(np.float64)
    fx, fy = c[:, 0], c[:, 1]
    x, y, z = pc[:, 0], pc[:, 1], pc[:, 2]
    with np.errstate(all="ignore"):
        z2 = z * z
        Jp = np.zeros((E, 2, 6))
        Jp[:, 0, 0], Jp[:, 0, 1], Jp[:, 0, 2], Jp[:, 0, 3], Jp[:, 0, 5] = x * y / z2 * fx, -(1 + (x * x / z2)) * fx, y / z * fx, -1.0 / z * fx, x / z2 * fx
        Jp[:, 1, 0], Jp[:, 1, 1], Jp[:, 1, 2], Jp[:, 1, 4], Jp[:, 1, 5] = (1 + y * y / z2) * fy, -x * y / z2 * fy, -x / z * fy, -1.0 / z * fy, y / z2 * fy
        tmp = np.zeros((E, 2, 3))
        tmp[:, 0, 0], tmp[:, 0, 2], tmp[:, 1, 1], tmp[:, 1, 2] = fx, -x / z * fx, fy, -y / z * fy
        R = rotations(est[:, :4])[a["ekf"]]
        Jl = np.einsum("eij,ejk->eik", (-1.0 / z)[:, None, None] * tmp, R)
    return Jp, Jl


class System:
    """buildSystem at the estimates: what constructQuadraticForm leaves in Hpp, Hll, Hpl and b, summed serially in the order `order`."""

    def __init__(self, a, est, X, active, order=None):
        self.a, self.active = a, active
        F, P, E = a["F"], len(X), len(active)
        self.pc, self.err, self.chi2 = edge_errors(a, est, X)
        self.rho0, rho1 = pom.huber(self.chi2)
        self.Jp, self.Jl = jacobians(a, est, self.pc)
        w = a["w"].astype(np.float64)
        with np.errstate(all="ignore"):
            wo = rho1 * w                                            # robustInformation
            r = -(w[:, None] * self.err) * rho1[:, None]             # omega_r = -(rho[1] * information * error)
            self.W = np.einsum("eia,e,eib->eab", self.Jp, wo, self.Jl)   # Hpl's block: 6 x 3
            App = np.einsum("eia,e,eib->eab", self.Jp, wo, self.Jp)
            All = np.einsum("eia,e,eib->eab", self.Jl, wo, self.Jl)
            bp = np.einsum("eia,ei->ea", self.Jp, r)
            bl = np.einsum("eia,ei->ea", self.Jl, r)
        idx = np.flatnonzero(active) if order is None else np.array([e for e in order if active[e]], int)
        self.idx = idx
        f = a["kf_free"][a["ekf"]]
        self.f = f
        self.Hpp, self.bp, self.Hll, self.bl = np.zeros((F, 6, 6)), np.zeros((F, 6)), np.zeros((P, 3, 3)), np.zeros((P, 3))
        to_free = idx[f[idx] >= 0]
        with np.errstate(all="ignore"):
            np.add.at(self.Hpp, f[to_free], App[to_free])
            np.add.at(self.bp, f[to_free], bp[to_free])
            np.add.at(self.Hll, a["ept"][idx], All[idx])
            np.add.at(self.bl, a["ept"][idx], bl[idx])
        self.f_on, self.p_on = np.zeros(F, bool), np.zeros(P, bool)
        self.f_on[f[to_free]] = True
        self.p_on[a["ept"][idx]] = True
        self.to_free = to_free
        self.robust = float(np.sum(np.cumsum(self.rho0[idx])[-1:])) if len(idx) else 0.0     # activeRobustChi2: serial

    def max_diagonal(self, poses_only=False):
        """computeLambdaInit's maximum over the vertices of the system; a NaN entry makes it NaN."""
        d = [np.abs(np.diagonal(self.Hpp[self.f_on], axis1=1, axis2=2)).ravel()]
        if not poses_only:
            d.append(np.abs(np.diagonal(self.Hll[self.p_on], axis1=1, axis2=2)).ravel())
        d = np.concatenate(d)
        return float("nan") if np.isnan(d).any() else float(d.max()) if len(d) else 0.0

    def trial(self, lam, solver="solve"):
        """BlockSolver::solve with lambda on both diagonals -> ok, x_p [F, 6], x_l [P, 3], and Dinv, Hschur, bschur for the checks."""
        a, F, P = self.a, len(self.Hpp), len(self.Hll)
        I3 = np.eye(3)
        Dinv = np.zeros((P, 3, 3))
        on = np.flatnonzero(self.p_on)
        with np.errstate(all="ignore"):
            try:
                Dinv[on] = np.linalg.inv(self.Hll[on] + lam * I3)
            except np.linalg.LinAlgError:
                Dinv[on] = np.nan
            Hs = np.zeros((F, F, 6, 6))
            for i in range(F):
                Hs[i, i] = self.Hpp[i] + lam * np.eye(6)
            coeff = np.zeros((F, 6))
            e = self.to_free
            pt = a["ept"][e]
            BD = np.einsum("eab,ebc->eac", self.W[e], Dinv[pt])
            np.add.at(coeff, self.f[e], np.einsum("eab,eb->ea", self.W[e], np.einsum("eab,eb->ea", Dinv[pt], self.bl[pt])))
            # pairs of edges of one point, both to free key frames
            if not hasattr(self, "_pairs"):
                by_point = {}
                for k in range(len(e)):
                    by_point.setdefault(int(pt[k]), []).append(k)
                self._pairs = (np.array([x for ks in by_point.values() for x in ks for y in ks], int), np.array([y for ks in by_point.values() for x in ks for y in ks], int))
            k1, k2 = self._pairs
            if len(k1):
                np.add.at(Hs, (self.f[e[k1]], self.f[e[k2]]), -np.einsum("eab,ecb->eac", BD[k1], self.W[e[k2]]))
            bs = self.bp - coeff
            act = np.flatnonzero(self.f_on)
            n = 6 * len(act)
            A = Hs[np.ix_(act, act)].transpose(0, 2, 1, 3).reshape(n, n)
            A = np.triu(A) + np.triu(A, 1).T                          # the solver reads the upper triangle
            rhs = bs[act].reshape(n)
            ok = bool(np.isfinite(A).all() and np.isfinite(rhs).all())
            xp = np.zeros((F, 6))
            if ok:
                try:
                    xp[act] = dense(A, rhs, solver).reshape(-1, 6)
                    ok = bool(np.isfinite(xp).all())
                except np.linalg.LinAlgError:
                    ok = False
            xl = np.zeros((P, 3))
            if ok:
                c = self.bl.copy()
                np.add.at(c, pt, -np.einsum("eab,ea->eb", self.W[e], xp[self.f[e]]))
                xl[on] = np.einsum("pab,pb->pa", Dinv[on], c[on])
        self.Dinv, self.Hs, self.bs = Dinv, Hs, bs
        return ok, xp, xl


def dense(A, b, solver):
    if solver == "solve":
        return np.linalg.solve(A, b)
    if solver == "cholesky":
        L = np.linalg.cholesky(A)
        return np.linalg.solve(L.T, np.linalg.solve(L, b))
    import scipy.linalg
    L, D, perm = scipy.linalg.ldl(A)
    return np.linalg.solve(L.T, np.linalg.solve(D, np.linalg.solve(L, b)))


def apply(a, est, X, xp, xl, sysm):
    """update(): oplus of every vertex of the system."""
    est2, X2 = est.copy(), X.copy()
    for k in range(len(est)):
        f = a["kf_free"][k]
        if f >= 0 and sysm.f_on[f]:
            q, t = pom.oplus(xp[f], est[k, :4], est[k, 4:])
            est2[k, :4], est2[k, 4:] = q, t
    X2[sysm.p_on] = X[sysm.p_on] + xl[sysm.p_on]
    return est2, X2


class Result:
    pass


def optimize(sc, mode=None, n_iterations=None, order=None, solver="solve", tau_poses_only=False):
    a = arrays(sc)
    mode = sc.get("mode", LOCAL) if mode is None else mode
    n_iterations = sc.get("n_iterations", 0) if n_iterations is None else n_iterations
    est, X = start(a)
    E = len(a["ekf"])
    active = np.ones(E, bool)
    stored = np.zeros(E)                       # chi2 of the stored error
    res = Result()
    res.lin, res.trials, res.iterations = [], [], [0, 0]
    res.removed1, res.removed2 = np.zeros(E, np.uint8), np.zeros(E, np.uint8)
    res.checks = []
    rounds = 2 if mode == LOCAL else 1
    for rnd in range(rounds):
        its = (5, 10)[rnd] if mode == LOCAL else n_iterations
        lam, ni, stalled = 0.0, 2.0, 0
        xp, xl = np.zeros((a["F"], 6)), np.zeros((len(X), 3))
        for it in range(its if active.any() else 0):
            S = System(a, est, X, active, order)
            stored[active] = S.chi2[active]
            cur = ini = S.robust
            if it == 0:
                lam, ni, stalled = 1e-5 * S.max_diagonal(tau_poses_only), 2.0, 0
            res.lin.append(dict(round=rnd, iteration=it, chi2=cur, maxdiag=S.max_diagonal(), n_edges=int(active.sum()), n_free=int(S.f_on.sum()),
                                n_points=int(S.p_on.sum()), est=est.copy(), X=X.copy(), active=active.copy(), lam0=lam))
            res.iterations[rnd] += 1
            rho, q = 0.0, 0
            while True:
                ok, xp_new, xl_new = S.trial(lam, solver)
                if ok:
                    xp, xl = xp_new, xl_new
                est_try, X_try = apply(a, est, X, xp, xl, S)
                _, _, chi_try = edge_errors(a, est_try, X_try)
                stored[active] = chi_try[active]
                r0, _ = pom.huber(chi_try[S.idx])
                tmp = float(np.cumsum(r0)[-1]) if len(r0) else 0.0
                if not ok:
                    tmp = DBL_MAX
                with np.errstate(all="ignore"):
                    scale = float(np.sum(xp[S.f_on] * (lam * xp[S.f_on] + S.bp[S.f_on])) + np.sum(xl[S.p_on] * (lam * xl[S.p_on] + S.bl[S.p_on]))) + 1e-3
                    rho = (cur - tmp) / scale
                accept = rho > 0 and math.isfinite(tmp)
                res.trials.append(dict(lin=len(res.lin) - 1, ok=ok, accepted=accept, lam=lam, cur=cur, tmp=tmp, scale=scale, rho=rho, xp=xp.copy(), xl=xl.copy(),
                                       est_try=est_try, X_try=X_try))
                if accept:
                    alpha = min(1.0 - (2 * rho - 1) ** 3, 2.0 / 3.0)
                    lam *= max(1.0 / 3.0, alpha)
                    ni = 2.0
                    cur = tmp
                    est, X = est_try, X_try
                else:
                    lam *= ni
                    ni *= 2
                q += 1
                if not (rho < 0 and q < 10):
                    break
            if q == 10 or rho == 0:
                break
            stalled = stalled + 1 if (ini - cur) * 1e3 < ini else 0
            if stalled >= 3:
                break
        if mode == LOCAL:
            pc, _, _ = edge_errors(a, est, X)
            with np.errstate(all="ignore"):
                bad = active & (a["bad"][a["ept"]] == 0) & ((stored > TH) | ~(pc[:, 2] > 0.0))
            res.checks.append(dict(stored=stored.copy(), depth=pc[:, 2].copy(), examined=active & (a["bad"][a["ept"]] == 0), restored=edge_errors(a, est, X)[2]))
            (res.removed1 if rnd == 0 else res.removed2)[bad] = 1
            active = active & ~bad
    res.est, res.X = est, X
    res.kf_Tcw = np.stack([pom.matrix_of(e[:4], e[4:])[0] for e in est]) if len(est) else np.zeros((0, 4, 4), np.float32)
    res.points = X.astype(np.float32)
    res.n_removed1, res.n_removed2 = int(res.removed1.sum()), int(res.removed2.sum())
    return res


# ---- scenes ----------------------------------------------------------------------------------------------------------------------------
def scene(seed, free, fixed, P, sees, shifted=0.1, noise=0.5, pose_off=0.01, point_off=0.03, fixed_first=False, mode=LOCAL, n_iterations=0, near=None):
    """free + fixed key frames along a baseline looking down +z at P points 4..10 m away.  sees(j, K) -> the key frames that observe
    point j, in the order the caller lists them.  A fraction `shifted` of the observations is moved by 5..8 px.  near: the depth of point 0,
    placed on the baseline's axis."""
    rng = np.random.RandomState(seed)
    K = free + fixed
    fix = np.zeros(K, np.uint8)
    if fixed:
        fix[:fixed] = 1 if fixed_first else 0
        fix[K - fixed:] = 0 if fixed_first else 1
    true_T = []
    for k in range(K):
        R = pom.rot_of_vec(rng.uniform(-0.05, 0.05, 3))
        t = np.array([-0.25 * (k - K / 2.0), 0.0, 0.0]) + rng.uniform(-0.05, 0.05, 3)
        true_T.append((R, t))
    Xw = np.stack([rng.uniform(-3, 3, P), rng.uniform(-2, 2, P), rng.uniform(4, 10, P)], 1)
    if near is not None:
        Xw[0] = [0.0, 0.0, near]
    cams = np.array([CAM, (CAM[0] + 2, CAM[1] + 2, CAM[2] - 2, CAM[3] + 2)], np.float32)
    begin, ekf, obs, w, ecam = [0], [], [], [], []
    for j in range(P):
        for k in sees(j, K):
            R, t = true_T[k]
            pc = R @ Xw[j] + t
            c = cams[k % 2]
            uv = np.array([c[0] * pc[0] / pc[2] + c[2], c[1] * pc[1] / pc[2] + c[3]]) + rng.normal(0, noise, 2)
            if rng.uniform() < shifted:
                ang = rng.uniform(0, 2 * math.pi)
                uv = uv + rng.uniform(5, 8) * np.array([math.cos(ang), math.sin(ang)])
            ekf.append(k), obs.append(uv), ecam.append(k % 2)
            w.append(1.0 / 1.2 ** (2 * rng.randint(0, 4)))                       # GetInvSigma2(octave)
        begin.append(len(ekf))
    Tcw = np.zeros((K, 12), np.float32)
    for k, (R, t) in enumerate(true_T):
        if not fix[k]:
            R = pom.rot_of_vec(rng.uniform(-pose_off, pose_off, 3)) @ R
            t = t + rng.uniform(-pose_off, pose_off, 3)
        Tcw[k] = np.concatenate([R, t[:, None]], 1).reshape(12)
    pts = (Xw + rng.uniform(-point_off, point_off, (P, 3))).astype(np.float32)
    return dict(Tcw=Tcw, fixed=fix, points=pts, point_bad=np.zeros(P, np.uint8), begin=np.array(begin, np.int32), edge_kf=np.array(ekf, np.int32),
                edge_obs=np.array(obs, np.float32).reshape(-1, 2), edge_inv_sigma2=np.array(w, np.float32), edge_camera=np.array(ecam, np.int32), cameras=cams,
                mode=mode, n_iterations=n_iterations)


def sees_all(j, K):
    return list(range(K))


def sees_random(mean, seed):
    def f(j, K):
        rng = np.random.RandomState(seed * 100003 + j)
        n = int(np.clip(rng.poisson(mean - 2) + 2, 2, K))
        return [int(k) for k in rng.permutation(K)[:n]]
    return f


def sees_prefix(counts, extra):
    """Key frame i sees the first counts[i] points; the key frames `extra` see every point."""
    return lambda j, K: [i for i, c in enumerate(counts) if j < c] + list(extra)


def edges_of(sc, j):
    return range(int(sc["begin"][j]), int(sc["begin"][j + 1]))


def small_specials(seed=3):
    """2 free + 2 fixed key frames and 8 points with everything that can drop out: point 0 has a single edge; point 1 is seen only from
    the fixed key frames; every edge of point 2 is a gross outlier; point 3 lies behind key frame 0; point 4 is flagged bad and carries a
    gross outlier that must survive both checks."""
    sc = scene(seed, 2, 2, 8, sees_all, shifted=0.0)
    keep = np.ones(len(sc["edge_kf"]), bool)
    for e in edges_of(sc, 0):
        keep[e] = sc["edge_kf"][e] == 0
    for e in edges_of(sc, 1):
        keep[e] = sc["fixed"][sc["edge_kf"][e]] == 1
    for n, e in enumerate(edges_of(sc, 2)):
        sc["edge_obs"][e] += np.float32([40.0, -35.0, -45.0, 38.0][n % 4]), np.float32([30.0, 42.0, -33.0, -36.0][n % 4])
    sc["points"][3] = np.float32([0.2, 0.1, -3.0])
    sc["point_bad"][4] = 1
    sc["edge_obs"][sc["begin"][4]] += np.float32(60.0)
    return prune(sc, keep)


def prune(sc, keep):
    out = dict(sc)
    counts = np.add.reduceat(keep.astype(np.int64), sc["begin"][:-1]) if len(keep) else np.zeros(0, int)
    counts[np.diff(sc["begin"]) == 0] = 0
    out["begin"] = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    for k in ("edge_kf", "edge_obs", "edge_inv_sigma2", "edge_camera"):
        out[k] = sc[k][keep]
    return out


def lonely_keyframe(seed=5):
    """3 free + 1 fixed: free key frame 2 has one edge, to a point that lies behind every camera, so that the first check leaves the key
    frame without any edge (one gross outlier would not do: six degrees of freedom fit one observation exactly)."""
    sc = scene(seed, 3, 1, 12, sees_all, shifted=0.0)
    sc["points"][5] = np.float32([0.3, -0.2, -4.0])
    keep = np.ones(len(sc["edge_kf"]), bool)
    for e in range(len(keep)):
        if sc["edge_kf"][e] == 2:
            keep[e] = e in edges_of(sc, 5)
    return prune(sc, keep)


def zero_depth(seed=9):
    """2 free + 1 fixed, 8 points: key frame 0 has the identity rotation and t_z = 0, point 0 has z = 0, so that edge's projection divides
    by zero: every sum it enters is NaN, the solve fails in each trial of the first optimize(), the first check removes the edge (its
    depth is not positive) and the second optimize() is an ordinary one."""
    sc = scene(seed, 2, 1, 8, sees_all, shifted=0.0)
    t = sc["Tcw"][0].reshape(3, 4)[:, 3].copy()
    sc["Tcw"][0] = np.float32([1, 0, 0, t[0], 0, 1, 0, t[1], 0, 0, 1, 0])
    sc["points"][0, 2] = 0.0
    return sc


LIST_COUNTS = (513, 257, 256, 255, 65, 64, 1)      # key-frame edge lists; the Schur lists of the pairs are the minima


def make_scenes():
    s = {}
    s["kf2_fixed1_p8"] = scene(1, 2, 1, 8, sees_all, shifted=0.0)
    s["kf3_first_fixed"] = scene(2, 2, 1, 8, sees_all, shifted=0.0, fixed_first=True)         # 3 + 0, key frame 0 fixed by the id rule
    s["specials"] = small_specials()
    s["lonely_keyframe"] = lonely_keyframe()
    s["far_start"] = scene(22, 3, 2, 40, sees_random(3, 22), shifted=0.15, pose_off=0.5, point_off=2.5)     # rejected trials
    s["zero_depth"] = zero_depth()
    # point 0 half a metre away and seen by all nine key frames: the largest diagonal entry is the point's, not a pose's
    s["near_point"] = scene(12, 8, 1, 12, lambda j, K: list(range(K)) if j == 0 else sees_random(3, 12)(j, K), shifted=0.0, near=0.5, point_off=0.005)
    s["lists"] = scene(6, len(LIST_COUNTS), 1, 513, sees_prefix(LIST_COUNTS, (7,)), shifted=0.05)
    for P in (255, 256, 257):
        s["points_%d" % P] = scene(10 + P, 3, 1, P, sees_random(2, P), shifted=0.1)
    s["realistic"] = scene(7, 12, 8, 400, sees_random(6.25, 7), shifted=0.1)
    s["full_20"] = dict(scene(1, 2, 1, 8, sees_all, shifted=0.0), mode=FULL, n_iterations=20)
    return s


def widest():
    """F = 64 with 4 points per key-frame pair, the largest reduced system (built on demand: 8064 points)."""
    pairs = [(i, j) for i in range(64) for j in range(i + 1, 64)]
    return scene(8, 64, 2, 4 * len(pairs), lambda j, K: list(pairs[j // 4]) + [64 + j % 2], shifted=0.02, n_iterations=0)


SCENES = make_scenes()


def make(name):
    return SCENES[name]


# ---- the committed scene list ----------------------------------------------------------------------------------------------------------
def pack(sc):
    a = arrays(sc)
    K, P, E, C = len(a["T"]), len(a["pts"]), len(a["ekf"]), len(a["cams"])
    return b"".join([struct.pack("<6i", sc.get("mode", LOCAL), sc.get("n_iterations", 0), K, P, E, C), a["T"].tobytes(), a["fixed"].tobytes(), a["pts"].tobytes(),
                     a["bad"].tobytes(), a["begin"].tobytes(), a["ekf"].tobytes(), a["obs"].tobytes(), a["w"].tobytes(), a["ecam"].tobytes(), a["cams"].tobytes()])


def dump(path):
    with open(path, "wb") as fh:
        fh.write(struct.pack("<i", len(SCENES)))
        for name in SCENES:
            fh.write(pack(SCENES[name]))


def packed():
    return struct.pack("<i", len(SCENES)) + b"".join(pack(SCENES[n]) for n in SCENES)


if __name__ == "__main__":
    import os
    dump(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ba_scenes.bin"))
