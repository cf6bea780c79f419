"""Test model of cv::solvePnPRansac(obj, img, K, dist, rvec, tvec, false, iterations, reproj_err, conf, inliers, SOLVEPNP_EPNP) as
OpenCV 3.4 computes it (calib3d/src/solvepnp.cpp, epnp.cpp, ptsetreg.cpp, calibration.cpp for projectPoints / Rodrigues).  The
reference calls it at src/Tracking.cc:1864 with (300, 3, 0.99).  numpy, float64.  Test infrastructure only: the product
(csrc/pnp.hip, csrc/epnp_core.hpp) never imports it.

This repository holds no OpenCV, so every detail below is recalled, not read.  [OCV-RECALL] -- to be pinned on an OpenCV machine:
  1. model_points = 5 for EPnP and the RANSAC kernel's method is EPnP.  npoints == model_points takes a direct path: one solvePnP on
     all points, every point an inlier.  The caller only calls with more than 4 points (:1863).
  2. RANSACPointSetRegistrator::run as items 3, 4 and 9 of fundamental_model.py with modelPoints = 5, maxIters = iterationsCount and
     no checkSubset: only a repeated index is redrawn, so subset h is a pure function of (n, h).  One model per hypothesis, taken iff
     count > max(best, 4), then niters = RANSACUpdateNumIters(conf, (n - count)/n, 5, niters).
  3. runKernel = solvePnP on the 5 float points: undistortPoints(ipoints, und, K, dist) without P (normalised coordinates, stored in
     the input's type: float for the subsets), epnp(K, opoints, und) whose init_points re-applies fu, uc, fv, vc in double,
     compute_pose, Rodrigues(R, rvec).
  4. computeError: projectPoints in double with k1 k2 p1 p2 (k3..k6 when given), the projection stored as float, its difference with
     the float image point in float, the squared norm accumulated in double and stored as float; inlier iff err <= (float)(thr*thr).
  5. After RANSAC the winner's inliers are compressed, converted to double, and solvePnP(EPNP) runs once more on them; its pose is
     what is returned.  The returned inlier list is the RANSAC winner's, not re-evaluated with the refitted pose.  A run without an
     accepted hypothesis returns false and no inliers.
  6. Rodrigues matrix -> vector: R is first replaced by U*Vt of its SVD, then r = (R32 - R23, R13 - R31, R21 - R12),
     s = |r|/2, c = (trace - 1)/2 clamped, theta = acos(c); s < 1e-5: zero for c > 0, else the diagonal form near pi; otherwise
     r * theta/(2 s).
  7. EPnP: control points = centroid + sqrt(eigenvalue/n) * principal axis; barycentric coordinates through the (pseudo-)inverse of
     the axes; M (2n x 12), MtM, the rows of Ut for the four smallest singular values; L_6x10 and rho over the six control-point
     pairs; three closed-form starts for the betas (columns (0,1,3,6), (0,1,2), (0..4) of L), each followed by 5 Gauss-Newton steps;
     per start the camera-frame points, the sign fixed by the first point's depth, R and t by the 3 x 3 SVD of the correlation with
     the determinant fix (third row of R negated); the start with the smallest mean reprojection error wins.
  8. The sign of each principal axis is whatever OpenCV's SVD of the 3 x 3 scatter matrix returns.  It matters: the control points
     c0 + axis and c0 - axis parametrise the same space, but the two 12-vectors are no orthogonal transform of each other, so with
     noisy data the least-squares null vector, and with it the pose, differs (measured by test_pnp_model.py: 2e-3 .. 2e-2 at
     0.3 - 1 px, the size of the noise-induced pose error itself; the order of the axes is an orthogonal change and does not
     matter).  OpenCV's signs cannot be recalled; the model and the product fix them by convention -- the largest component of
     each axis is positive -- and `axis_signs` flips them for that measurement.  The pin has to record OpenCV's.

A fact that shapes every test: with 5 points M is 10 x 12, MtM has a two-dimensional null space, and the two
rows of Ut that span it are an arbitrary basis fixed only by the rounding of whichever solver computed them.  The three starts use
those rows one by one, so a hypothesis's pose is NOT a function of the data alone; from 6 points on it is.  `basis` selects among four
equally legitimate solvers ("svd": SVD of MtM, "eigh": its symmetric eigen-decomposition, "svdM": SVD of M, "rot": "svd" with the two
smallest rows rotated by an arbitrary angle) so that tests can measure that spread instead of believing it.
"""
import math

import numpy as np

import fundamental_model as fmod

MODEL_POINTS = 5
BASES = ("svd", "eigh", "svdM", "rot")
SENS_RTOL = 1e-6           # an error within this (relative) of the threshold may fall either way
PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))

# cameras: (fx, fy, cx, cy, (k1, k2, p1, p2), (width, height)); the library takes mK and mDistCoef as float32
EUROC = (458.654, 457.296, 367.215, 248.375, (-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05), (752, 480))
PLAIN = (576.0, 576.0, 320.0, 256.0, (), (640, 512))
# not a camera of the reference: five coefficients with tangential terms large enough that dropping one moves projections by pixels
STRONG = (500.0, 505.0, 318.0, 243.0, (-0.12, 0.03, 0.012, -0.015, 0.004), (640, 480))
# scenes in which a later hypothesis ties the winner's count with a different inlier set (what `>=` instead of `>` at acceptance would take)
TIE_SCENES = ((201, 64, 0.5, 1.0, EUROC), (213, 64, 0.5, 1.0, EUROC), (217, 20, 0.7, 1.0, EUROC))

# The refit tolerance: measured on this model alone, never on the code under test.  REFIT_SPREAD_MEASURED is the largest deviation
# (max of ||Ra - Rb||_F and |ta - tb| / max(|tb|, 1)) between the basis variants over every refit of refit_scenes() (lists of at
# least 6 points); the bound is 4 times that -- two correct factorizations associate differently, a third should sit within a small
# multiple of their distance (the margin of triangulation_model.py).  test_pnp_model.py fails when a scene change moves the measured
# value past REFIT_SPREAD_MEASURED.
REFIT_SPREAD_MEASURED = 2.5e-13          # measured 2.36e-13 (20 points, noise-free, the distortion-free camera)
REFIT_TOL = 4 * REFIT_SPREAD_MEASURED    # 1e-12
# for the record, against that bound (not used by any assertion): the host build of csrc/epnp_core.hpp on refit_scenes(), and the device
# on the RANSAC inlier lists of the whole grid (an MI355X; profiles/LOG.md)
REFIT_HOST_BUILD_WORST = 1.2e-13
REFIT_DEVICE_WORST = 3.3e-13


class Camera:
    def __init__(self, spec):
        f32 = lambda v: float(np.float32(v))
        self.fx, self.fy, self.cx, self.cy = (f32(v) for v in spec[:4])
        self.k = [f32(v) for v in spec[4]] + [0.0] * (8 - len(spec[4]))   # k1 k2 p1 p2 k3 k4 k5 k6
        self.n_dist = len(spec[4])
        self.size = spec[5]

    @property
    def K(self):
        return (self.fx, self.fy, self.cx, self.cy)

    def as_doubles(self):
        return np.array([self.fx, self.fy, self.cx, self.cy] + self.k, np.float64)


# ---- the random stream ----------------------------------------------------------------------------------------------------------
def subsets(n, count):
    """The first `count` subsets of a run over n points and the draws consumed after each: ([count][5], [count])."""
    rng = fmod.Rng()
    out, ends = [], []
    for _ in range(count):
        idx = []
        for _i in range(MODEL_POINTS):
            while True:
                v = rng.next() % n
                if v not in idx:
                    break
            idx.append(v)
        out.append(idx)
        ends.append(rng.draws)
    return np.array(out, np.int32).reshape(count, MODEL_POINTS), np.array(ends, np.uint32)


def subset(n, h):
    """Subset h of a run over n points and the RNG draws consumed once it is drawn."""
    s, e = subsets(n, h + 1)
    return s[h], int(e[h])


# ---- camera model -----------------------------------------------------------------------------------------------------------------
def distort(cam, x, y):
    """Normalised -> pixel, cv::projectPoints' lens model."""
    k = cam.k
    r2 = x * x + y * y
    r4 = r2 * r2
    r6 = r4 * r2
    a1 = 2 * x * y
    a2 = r2 + 2 * x * x
    a3 = r2 + 2 * y * y
    cdist = 1 + k[0] * r2 + k[1] * r4 + k[4] * r6
    icdist2 = 1.0 / (1 + k[5] * r2 + k[6] * r4 + k[7] * r6)
    xd = x * cdist * icdist2 + k[2] * a1 + k[3] * a2
    yd = y * cdist * icdist2 + k[2] * a3 + k[3] * a1
    return xd * cam.fx + cam.cx, yd * cam.fy + cam.cy


def project_points(cam, R, t, obj):
    """cv::projectPoints in double: (n, 2) float64 pixels."""
    P = np.asarray(obj, np.float64)
    with np.errstate(all="ignore"):
        X = P @ np.asarray(R, np.float64).reshape(3, 3).T + np.asarray(t, np.float64)
        z = np.where(X[:, 2] != 0, 1.0 / X[:, 2], 1.0)
        u, v = distort(cam, X[:, 0] * z, X[:, 1] * z)
    return np.stack([u, v], 1)


def undistort(cam, img):
    """cv::undistortPoints without P: five fixed-point iterations; (n, 2) float64 normalised coordinates."""
    m = np.asarray(img, np.float64)
    k = cam.k
    x = (m[:, 0] - cam.cx) * (1.0 / cam.fx)
    y = (m[:, 1] - cam.cy) * (1.0 / cam.fy)
    x0, y0 = x.copy(), y.copy()
    for _ in range(5):
        r2 = x * x + y * y
        icdist = (1 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2) / (1 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2)
        dx = 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x)
        dy = k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y
        x = (x0 - dx) * icdist
        y = (y0 - dy) * icdist
    return np.stack([x, y], 1)


def errors(cam, R, t, obj, img):
    """computeError: float32 errors of all points against the pose."""
    proj = project_points(cam, R, t, obj).astype(np.float32)
    d = np.asarray(img, np.float32) - proj
    with np.errstate(all="ignore"):
        return (d[:, 0].astype(np.float64) ** 2 + d[:, 1].astype(np.float64) ** 2).astype(np.float32)


def count(cam, R, t, obj, img, thr=3.0):
    """Inliers of a pose: (count, lowest and highest count the margin rule admits, the float32 errors, the inlier mask)."""
    err = errors(cam, R, t, obj, img)
    tt = np.float32(thr * thr)
    with np.errstate(all="ignore"):
        inl = err <= tt
        near = np.abs(err.astype(np.float64) - float(tt)) <= SENS_RTOL * float(tt)
    sure = int((inl & ~near).sum())
    return int(inl.sum()), sure, sure + int(near.sum()), err, inl


# ---- RANSAC bookkeeping -----------------------------------------------------------------------------------------------------------
def replay(counts, n, conf=0.99, max_iters=300):
    """The RANSAC loop over given per-hypothesis inlier counts: (winner or -1, iterations)."""
    niters, best, best_count, it = max_iters, -1, 0, 0
    while it < niters:
        c = int(counts[it])
        if c > max(best_count, MODEL_POINTS - 1):
            best_count, best = c, it
            niters = fmod.update_num_iters(conf, (n - c) / n, MODEL_POINTS, niters)
        it += 1
    return best, it


# ---- EPnP -------------------------------------------------------------------------------------------------------------------------
def _null_rows(M, basis, rng):
    """The four rows v[0..3] that EPnP reads: singular vectors of the four smallest singular values, smallest first."""
    MtM = M.T @ M
    if basis == "eigh":
        V = np.linalg.eigh(MtM)[1].T[:4]
    elif basis == "svdM":
        V = np.linalg.svd(M, full_matrices=True)[2][::-1][:4]
    else:
        V = np.linalg.svd(MtM)[2][::-1][:4]
        if basis == "rot" and len(M) == 2 * MODEL_POINTS:   # only there do the two rows span a null space; elsewhere "rot" is "svd"
            a = (rng or np.random.default_rng(0)).uniform(0, 2 * np.pi)
            c, s = math.cos(a), math.sin(a)
            V = V.copy()
            V[0], V[1] = c * V[0] + s * V[1], -s * V[0] + c * V[1]
    return np.array(V)


def _beta_pair(b0, b1, b2):
    if b0 < 0:
        x0 = math.sqrt(-b0)
        x1 = math.sqrt(-b2) if b2 < 0 else 0.0
    else:
        x0 = math.sqrt(b0)
        x1 = math.sqrt(b2) if b2 > 0 else 0.0
    return (-x0 if b1 < 0 else x0), x1


def epnp(pw, uv, K, basis="svd", rng=None, axis_signs=(1, 1, 1)):
    """EPnP on world points pw (m, 3) and pixel points uv (m, 2), K = (fu, fv, uc, vc); axis_signs flips the principal axes (largest
    first) against the convention of item 8.  Returns (R, t, mean reprojection error) of the
    best start, or None when no start gives a finite pose."""
    pw = np.asarray(pw, np.float64)
    uv = np.asarray(uv, np.float64)
    fu, fv, uc, vc = K
    m = len(pw)
    with np.errstate(all="ignore"):
        c0 = pw.mean(0)
        w, v = np.linalg.eigh((pw - c0).T @ (pw - c0))
        v = v * np.array([-1.0 if v[np.argmax(np.abs(v[:, i])), i] < 0 else 1.0 for i in range(3)])   # item 8
        v = v * np.asarray(axis_signs, np.float64)[::-1]
        cws = np.vstack([c0] + [c0 + math.sqrt(max(w[i], 0.0) / m) * v[:, i] for i in (2, 1, 0)])
        axes = (cws[1:] - cws[0]).T
        a123 = (np.linalg.pinv(axes) @ (pw - cws[0]).T).T
        al = np.hstack([1 - a123.sum(1, keepdims=True), a123])
        M = np.zeros((2 * m, 12))
        for j in range(4):
            M[0::2, 3 * j] = al[:, j] * fu
            M[0::2, 3 * j + 2] = al[:, j] * (uc - uv[:, 0])
            M[1::2, 3 * j + 1] = al[:, j] * fv
            M[1::2, 3 * j + 2] = al[:, j] * (vc - uv[:, 1])
        if not np.isfinite(M).all():
            return None
        V = _null_rows(M, basis, rng)
        dv = np.array([[V[i, 3 * a:3 * a + 3] - V[i, 3 * b:3 * b + 3] for (a, b) in PAIRS] for i in range(4)])
        L = np.zeros((6, 10))
        for r in range(6):
            d = dv[:, r]
            L[r] = [d[0] @ d[0], 2 * d[0] @ d[1], d[1] @ d[1], 2 * d[0] @ d[2], 2 * d[1] @ d[2], d[2] @ d[2], 2 * d[0] @ d[3],
                    2 * d[1] @ d[3], 2 * d[2] @ d[3], d[3] @ d[3]]
        rho = np.array([np.sum((cws[a] - cws[b]) ** 2) for (a, b) in PAIRS])

        def lsq(A, b):
            if not (np.isfinite(A).all() and np.isfinite(b).all()):
                return np.full(A.shape[1], np.nan)
            return np.linalg.lstsq(A, b, rcond=None)[0]

        starts = []
        b4 = lsq(L[:, [0, 1, 3, 6]], rho)
        r0 = math.sqrt(abs(b4[0])) if np.isfinite(b4[0]) else float("nan")
        sg = -1.0 if b4[0] < 0 else 1.0
        starts.append(np.array([r0, sg * b4[1] / r0, sg * b4[2] / r0, sg * b4[3] / r0]))
        b3 = lsq(L[:, [0, 1, 2]], rho)
        if np.isfinite(b3).all():
            x0, x1 = _beta_pair(b3[0], b3[1], b3[2])
            starts.append(np.array([x0, x1, 0.0, 0.0]))
        b5 = lsq(L[:, [0, 1, 2, 3, 4]], rho)
        if np.isfinite(b5).all():
            x0, x1 = _beta_pair(b5[0], b5[1], b5[2])
            starts.append(np.array([x0, x1, b5[3] / x0, 0.0]))
        best = None
        for bt in starts:
            for _ in range(5):
                b = bt
                A = np.stack([2 * L[:, 0] * b[0] + L[:, 1] * b[1] + L[:, 3] * b[2] + L[:, 6] * b[3],
                              L[:, 1] * b[0] + 2 * L[:, 2] * b[1] + L[:, 4] * b[2] + L[:, 7] * b[3],
                              L[:, 3] * b[0] + L[:, 4] * b[1] + 2 * L[:, 5] * b[2] + L[:, 8] * b[3],
                              L[:, 6] * b[0] + L[:, 7] * b[1] + L[:, 8] * b[2] + 2 * L[:, 9] * b[3]], 1)
                res = rho - (L[:, 0] * b[0] ** 2 + L[:, 1] * b[0] * b[1] + L[:, 2] * b[1] ** 2 + L[:, 3] * b[0] * b[2] + L[:, 4] * b[1] * b[2] +
                             L[:, 5] * b[2] ** 2 + L[:, 6] * b[0] * b[3] + L[:, 7] * b[1] * b[3] + L[:, 8] * b[2] * b[3] + L[:, 9] * b[3] ** 2)
                bt = bt + lsq(A, res)
            if not np.isfinite(bt).all():
                continue
            ccs = (bt[:, None] * V).sum(0).reshape(4, 3)
            pcs = al @ ccs
            if pcs[0, 2] < 0:
                ccs, pcs = -ccs, -pcs
            pc0, pw0 = pcs.mean(0), pw.mean(0)
            U, _, Vt = np.linalg.svd((pcs - pc0).T @ (pw - pw0))
            R = U @ Vt
            if np.linalg.det(R) < 0:
                R[2] = -R[2]
            t = pc0 - R @ pw0
            pc = pw @ R.T + t
            e = float(np.mean(np.hypot(uv[:, 0] - (uc + fu * pc[:, 0] / pc[:, 2]), uv[:, 1] - (vc + fv * pc[:, 1] / pc[:, 2]))))
            if not (np.isfinite(e) and np.isfinite(R).all() and np.isfinite(t).all()):
                continue
            if best is None or e < best[2]:
                best = (R, t, e)
    return best


def solve_pnp(cam, obj, img, idx, as_float, basis="svd", rng=None):
    """solvePnP(EPNP) on the listed points: as_float = the RANSAC kernel's view (undistorted points stored as float), else double."""
    idx = np.asarray(idx, np.int64)
    und = undistort(cam, np.asarray(img)[idx])   # float32 in the product's calls; a test may keep a scene in double
    if as_float:
        und = und.astype(np.float32).astype(np.float64)
    uv = und * [cam.fx, cam.fy] + [cam.cx, cam.cy]
    return epnp(np.asarray(obj)[idx].astype(np.float64), uv, cam.K, basis, rng)


def refit(cam, obj, img, inlier_indices, basis="svd", rng=None):
    """Item 5: EPnP once more on the inliers, in double.  Returns (R, t) or None."""
    r = solve_pnp(cam, obj, img, inlier_indices, False, basis, rng)
    return None if r is None else (r[0], r[1])


def pose_deviation(Ra, ta, Rb, tb):
    """max(||Ra - Rb||_F, |ta - tb| / max(|tb|, 1)) -- rotation differences as a norm, not as an angle (arccos near 1 has a 3e-8 floor)."""
    return max(float(np.linalg.norm(np.asarray(Ra).reshape(3, 3) - np.asarray(Rb).reshape(3, 3))),
               float(np.linalg.norm(np.asarray(ta) - np.asarray(tb)) / max(np.linalg.norm(tb), 1.0)))


def rodrigues(R):
    """cv::Rodrigues, matrix -> vector (item 6)."""
    U, _, Vt = np.linalg.svd(np.asarray(R, np.float64).reshape(3, 3))
    R = U @ Vt
    r = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s = math.sqrt((r @ r) * 0.25)
    c = min(max((R[0, 0] + R[1, 1] + R[2, 2] - 1) * 0.5, -1.0), 1.0)
    theta = math.acos(c)
    if s < 1e-5:
        if c > 0:
            return np.zeros(3)
        rx = math.sqrt(max((R[0, 0] + 1) * 0.5, 0.0))
        ry = math.sqrt(max((R[1, 1] + 1) * 0.5, 0.0)) * (-1.0 if R[0, 1] < 0 else 1.0)
        rz = math.sqrt(max((R[2, 2] + 1) * 0.5, 0.0)) * (-1.0 if R[0, 2] < 0 else 1.0)
        if abs(rx) < abs(ry) and abs(rx) < abs(rz) and (R[1, 2] > 0) != (ry * rz > 0):
            rz = -rz
        r = np.array([rx, ry, rz])
        return r * (theta / math.sqrt(r @ r))
    return r * (theta / (2 * s))


def rodrigues_to_matrix(rvec):
    r = np.asarray(rvec, np.float64)
    th = float(np.linalg.norm(r))
    if th < 1e-300:
        return np.eye(3)
    k = r / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(th) * Kx + (1 - math.cos(th)) * (Kx @ Kx)


class Result:
    def __init__(self):
        self.ok = False
        self.iterations = 0
        self.inliers = np.zeros(0, np.int32)
        self.rng_draws = 0
        self.R, self.t, self.rvec = np.zeros((3, 3)), np.zeros(3), np.zeros(3)
        self.winner = -1
        self.counts = []


def run(cam, obj, img, iterations=300, thr=3.0, conf=0.99, basis="svd", rot_seed=0, accept_ge=False, update_points=MODEL_POINTS,
        refit_all=False):
    """The whole call for one basis variant.  accept_ge / update_points / refit_all exist for the tests' mutation checks."""
    obj = np.ascontiguousarray(obj, np.float32).reshape(-1, 3)
    img = np.ascontiguousarray(img, np.float32).reshape(-1, 2)
    n = len(obj)
    res = Result()
    rng = np.random.default_rng(rot_seed)
    if n < MODEL_POINTS:
        return res
    if n == MODEL_POINTS:
        r = solve_pnp(cam, obj, img, range(5), True, basis, rng)
        if r is not None:
            res.ok, res.R, res.t, res.inliers = True, r[0], r[1], np.arange(5, dtype=np.int32)
            res.rvec = rodrigues(res.R)
        return res
    subs, ends = subsets(n, iterations)
    niters, best, best_mask, it = iterations, 0, None, 0
    while it < niters:
        r = solve_pnp(cam, obj, img, subs[it], True, basis, rng)
        c = 0
        if r is not None:
            c, _, _, _, inl = count(cam, r[0], r[1], obj, img, thr)
            if (c >= max(best, MODEL_POINTS - 1)) if accept_ge else (c > max(best, MODEL_POINTS - 1)):
                best, best_mask, res.winner = c, inl, it
                niters = fmod.update_num_iters(conf, (n - c) / n, update_points, niters)
        res.counts.append(c)
        it += 1
    res.iterations = it
    res.rng_draws = int(ends[it - 1]) if it else 0
    if best_mask is None:
        return res
    idx = np.flatnonzero(best_mask).astype(np.int32)
    r = refit(cam, obj, img, np.arange(n) if refit_all else idx, basis, rng)
    if r is None:
        return res
    res.ok, res.R, res.t, res.inliers = True, r[0], r[1], idx
    res.rvec = rodrigues(res.R)
    return res


# ---- scenes -----------------------------------------------------------------------------------------------------------------------
def scene(seed, n, inlier_ratio, noise_px, camera=EUROC, dtype=np.float32, spread=1.0):
    """Map points 1 - 20 m in front of a camera with a random pose, projected with the camera's distortion; Gaussian pixel noise on the
    inliers, uniform image positions for the outliers.  spread < 1 keeps the
    projections in the central part of the image.  Returns (Camera, obj (n, 3), img (n, 2), R_true, t_true, is_inlier)."""
    cam = Camera(camera)
    rng = np.random.default_rng(seed)
    w, h = cam.size
    ax = rng.normal(size=3)
    ax *= rng.uniform(0.05, 0.5) / np.linalg.norm(ax)
    R = rodrigues_to_matrix(ax)
    t = rng.normal(size=3) * 0.5
    uv = np.stack([w * (0.5 + spread * rng.uniform(-0.5, 0.5, n)), h * (0.5 + spread * rng.uniform(-0.5, 0.5, n))], 1)
    und = undistort(cam, uv)
    z = rng.uniform(1, 20, n)
    pc = np.stack([und[:, 0] * z, und[:, 1] * z, z], 1)
    pw = (pc - t) @ R                      # R^T (pc - t)
    obj = pw.astype(dtype)
    img = project_points(cam, R, t, obj.astype(np.float64)) + rng.normal(size=(n, 2)) * noise_px
    inl = np.zeros(n, bool)
    inl[rng.permutation(n)[:int(round(inlier_ratio * n))]] = True
    k = int((~inl).sum())
    img[~inl] = np.stack([rng.uniform(0, w, k), rng.uniform(0, h, k)], 1)
    return cam, obj, img.astype(dtype), R, t, inl


GRID_N = (5, 6, 8, 20, 64, 400, 1000)      # + the handle's max_points in the GPU tests
GRID_RATIO = (0.95, 0.7, 0.5, 0.3)
GRID_NOISE = (0.3, 1.0)


def refit_scenes():
    """The committed scenes whose refits define REFIT_SPREAD_MEASURED: all-inlier lists of 6 .. 2048 points at 0, 0.3 and 1 px."""
    out = []
    for n in (6, 7, 8, 12, 20, 50, 400, 2048):
        for noise in (0.0, 0.3, 1.0):
            for seed in range(8 if n <= 50 else 2):
                for camera in (EUROC, PLAIN):
                    out.append((1000 * n + seed, n, 1.0, noise, camera))
    return out


def grid_scenes(extra_n=()):
    """The scenes of the contract's grid at the call site's parameters (300, 3, 0.99): scene() arguments, both cameras."""
    out = []
    for n in tuple(GRID_N) + tuple(extra_n):
        for ri, ratio in enumerate(GRID_RATIO):
            for ni, noise in enumerate(GRID_NOISE):
                for ci, camera in enumerate((EUROC, PLAIN)):
                    out.append((n * 100 + ri * 10 + ni * 2 + ci, n, ratio, noise, camera))
    return out


def band(values, degenerate):
    """Layer 6: the interval the variants span, widened by its own width on each side -- by `degenerate` (one inlier, 1e-9) where the
    band is degenerate, which is wherever it is narrower than that: four variants that agree to 1e-14 coincide, they do not span 1e-14."""
    lo, hi = min(values), max(values)
    w = max(hi - lo, degenerate)
    return lo - w, hi + w
