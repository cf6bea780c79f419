"""Test model of cv::findFundamentalMat(p0, p1, FM_RANSAC, thr, conf, mask) as OpenCV 3.4 computes it (calib3d/src/fundam.cpp,
ptsetreg.cpp; core/src/mathfuncs.cpp for solveCubic).  The reference calls it at src/Tracking.cc:1062 with thr 1, conf 0.999.
Test infrastructure only: the product (csrc/fundamental.hip) never imports it.

This repository holds no OpenCV, so every detail below is recalled, not read.  [OCV-RECALL] -- to be pinned on an OpenCV machine:
  1. thr <= 0 becomes 3; conf outside [DBL_EPSILON, 1 - DBL_EPSILON] becomes 0.99.
  2. n < 7: no model, mask untouched.  n == 7: run7Point once, mask all 1 whatever it returns.  8 <= n <= 14: LMedS although
     FM_RANSAC was asked for.  n >= 15: RANSAC.
  3. cv::RNG seeded with (uint64)-1; next(): state = (uint64)(uint32)state * 4164903690 + (state >> 32), returns (uint32)state;
     uniform(0, n) = next() % n.
  4. getSubset (checkPartialSubsets = false): 7 indices, each redrawn until it differs from the earlier ones; the subset is
     rejected when haveCollinearPoints holds for p0's or for p1's seven points and then redrawn in full; at most 10 000 (RANSAC)
     resp. 1 000 (LMedS) attempts.  A failed getSubset at iteration 0 gives no model, later it ends the loop.
  5. haveCollinearPoints tests only the last point against every pair k < j < 6; the differences are float (Point2f members),
     widened to double: fabs(dx2*dy1 - dy2*dx1) <= FLT_EPSILON*(fabs(dx1) + fabs(dy1) + fabs(dx2) + fabs(dy2)).
  6. run7Point: rows (x1x0, x1y0, x1, y1x0, y1y0, y1, x0, y0, 1) of the raw points (no normalisation), f1 / f2 = the last two
     rows of Vt of a full SVD, f1 -= f2, the closed-form coefficients of det(lambda*f1 + f2) (c[0] leading), solveCubic, and
     per root s = f1[8]*lambda + f2[8]: |s| > DBL_EPSILON scales to F[8] = 1, else F[8] = 0.  A count < 1 means no model.
  7. solveCubic (double): a0 == 0 -> quadratic (q1/q2 form, d >= 0, 2 roots if d > 0 else 1) or linear (-a3/a2), all-zero -> -1;
     otherwise d = Q^3 - R^2: d > 0 three trigonometric roots in the order t1, t1 + 2pi/3, t1 - 2pi/3; d == 0 the pow(R, 1/3)
     pair (one root if they coincide); otherwise (NaN included) one root e + Q/e - a1/3 with e = pow(sqrt(-d) + |R|, 1/3),
     negated for R > 0.
  8. computeError: err = (float)std::max(d1*d1*s1, d2*d2*s2) in double, std::max(a, b) = a < b ? b : a; inlier iff
     err <= (float)(thr*thr).
  9. RANSAC: niters = 1000; a model is taken iff its count > max(best, 6); then niters = RANSACUpdateNumIters(conf,
     (n - count)/n, 7, niters) (log / pow, cvRound = round half to even); no model at the end releases the mask (all 0 here).
 10. LMedS: niters = max(RANSACUpdateNumIters(conf, 0.45, 7, 1000), 3); score = the float error at position n/2 after
     std::nth_element on the error bits read as int; the strictly smallest score wins; sigma = max(2.5*1.4826*(1 + 5/(n - 7))*
     sqrt(minMedian), 0.001); the mask is the inliers at sigma whatever their number, F only when >= 7 of them.
 11. findFundamentalMat returns all models of the n == 7 kernel (9 x 3); this restatement keeps the first.

Sensitivity flags name the places where the product may differ legitimately: an evaluated error within 1e-6
(relative) of its threshold, two models of one hypothesis tied at a new RANSAC maximum (root order depends on the null-space basis),
an LMedS median within 1e-4 of the running minimum (an error within 1e-4 of sigma^2), and LMedS below 14 points ("median_is_fit_residual"): there the median, the
error at position n/2 <= 6, is one of the seven residuals of the exact 7-point fit -- rounding noise of the basis, so which model
wins (and the mask that follows) is not fixed by the data at all.
"""
import math

import numpy as np

FLT_EPSILON = float(np.finfo(np.float32).eps)
DBL_EPSILON = float(np.finfo(np.float64).eps)
DBL_MIN = float(np.finfo(np.float64).tiny)
DBL_MAX = float(np.finfo(np.float64).max)
MWC_A = 4164903690
MWC_M = MWC_A * (1 << 32) - 1
SEED = (1 << 64) - 1
METHOD_NONE, METHOD_7POINT, METHOD_RANSAC, METHOD_LMEDS = 0, 1, 2, 3
SENS_RTOL = 1e-6
LMEDS_RTOL = 1e-4   # an LMedS median is a small error: its relative rounding is larger than an inlier count's threshold test


class Rng:
    """cv::RNG (multiply-with-carry), counting next() calls."""

    def __init__(self, state=SEED):
        self.state = state
        self.draws = 0

    def next(self):
        s = self.state
        self.state = (s & 0xFFFFFFFF) * MWC_A + (s >> 32)
        self.draws += 1
        return self.state & 0xFFFFFFFF


def state_after(k):
    """The RNG state after k next() calls, by jump-ahead: for k >= 2 the state is A^(k-2) * S_2 mod M (M = A * 2^32 - 1)."""
    r = Rng()
    if k < 2:
        for _ in range(k):
            r.next()
        return r.state
    r.next(), r.next()
    return pow(MWC_A, k - 2, MWC_M) * r.state % MWC_M


def cv_round(x):
    return int(np.rint(x))


def update_num_iters(p, ep, model_points, max_iters):
    """RANSACUpdateNumIters."""
    p = min(max(p, 0.0), 1.0)
    ep = min(max(ep, 0.0), 1.0)
    num = max(1.0 - p, DBL_MIN)
    denom = 1.0 - math.pow(1.0 - ep, model_points)
    if denom < DBL_MIN:
        return 0
    num = math.log(num)
    denom = math.log(denom)
    return max_iters if (denom >= 0 or -num >= max_iters * (-denom)) else cv_round(num / denom)


def solve_cubic(c):
    """cv::solveCubic for 4 double coefficients (c[0] leading); returns (n, [x0, x1, x2])."""
    a0, a1, a2, a3 = (float(v) for v in c)
    x0 = x1 = x2 = 0.0
    n = 0
    if a0 == 0:
        if a1 == 0:
            if a2 == 0:
                n = -1 if a3 == 0 else 0
            else:
                x0 = -a3 / a2
                n = 1
        else:
            d = a2 * a2 - 4 * a1 * a3
            if d >= 0:
                d = math.sqrt(d)
                q1 = (-a2 + d) * 0.5
                q2 = (a2 + d) * -0.5
                if abs(q1) > abs(q2):
                    x0 = q1 / a1
                    x1 = a3 / q1
                else:
                    x0 = q2 / a1
                    x1 = a3 / q2
                n = 2 if d > 0 else 1
    else:
        a0 = 1.0 / a0
        a1 *= a0
        a2 *= a0
        a3 *= a0
        Q = (a1 * a1 - 3 * a2) * (1.0 / 9)
        R = (2 * a1 * a1 * a1 - 9 * a1 * a2 + 27 * a3) * (1.0 / 54)
        Qcubed = Q * Q * Q
        d = Qcubed - R * R
        if d > 0:
            theta = math.acos(R / math.sqrt(Qcubed))
            sqrtQ = math.sqrt(Q)
            t0 = -2 * sqrtQ
            t1 = theta * (1.0 / 3)
            t2 = a1 * (1.0 / 3)
            x0 = t0 * math.cos(t1) - t2
            x1 = t0 * math.cos(t1 + (2.0 * math.pi / 3)) - t2
            x2 = t0 * math.cos(t1 - (2.0 * math.pi / 3)) - t2
            n = 3
        elif d == 0:
            if R >= 0:
                x0 = -2 * math.pow(R, 1.0 / 3) - a1 / 3
                x1 = math.pow(R, 1.0 / 3) - a1 / 3
            else:
                x0 = 2 * math.pow(-R, 1.0 / 3) - a1 / 3
                x1 = -math.pow(-R, 1.0 / 3) - a1 / 3
            x2 = 0.0
            n = 1 if x0 == x1 else 2
            x1 = 0.0 if x0 == x1 else x1
        else:
            if d == d and R == R and Q == Q:
                d = math.sqrt(-d)
                e = math.pow(d + abs(R), 1.0 / 3)
                if R > 0:
                    e = -e
                x0 = (e + Q / e) - a1 * (1.0 / 3)
            else:                       # NaN takes this branch in C++ too; Python's math would raise instead of returning NaN
                x0 = float("nan")
            n = 1
    return n, [x0, x1, x2]


def null_basis(A):
    """f1, f2 = the last two rows of Vt of a full SVD of the 7 x 9 system (NaN when the system is not finite)."""
    if not np.isfinite(A).all():
        nan = np.full(9, np.nan)
        return nan, nan.copy()
    vt = np.linalg.svd(A, full_matrices=True)[2]
    return vt[7].copy(), vt[8].copy()


def ata_basis(A):
    """The normal-equations null space (eigenvectors of A^T A): the basis the contract forbids -- a mutation for the tests."""
    if not np.isfinite(A).all():
        nan = np.full(9, np.nan)
        return nan, nan.copy()
    v = np.linalg.eigh(A.T @ A)[1]
    return v[:, 1].copy(), v[:, 0].copy()


def system_7pt(p0, p1, idx):
    x0, y0 = p0[idx, 0].astype(np.float64), p0[idx, 1].astype(np.float64)
    x1, y1 = p1[idx, 0].astype(np.float64), p1[idx, 1].astype(np.float64)
    return np.stack([x1 * x0, x1 * y0, x1, y1 * x0, y1 * y0, y1, x0, y0, np.ones(7)], 1)


def run_7point(p0, p1, idx, basis=null_basis):
    """run7Point on the seven points idx (float32 or float64 arrays); returns the list of models (float64 arrays of 9)."""
    with np.errstate(all="ignore"):
        f1, f2 = basis(system_7pt(p0, p1, idx))
    f1 = [float(v) for v in f1]
    f2 = [float(v) for v in f2]
    for i in range(9):
        f1[i] -= f2[i]
    t0 = f2[4] * f2[8] - f2[5] * f2[7]
    t1 = f2[3] * f2[8] - f2[5] * f2[6]
    t2 = f2[3] * f2[7] - f2[4] * f2[6]
    c3 = f2[0] * t0 - f2[1] * t1 + f2[2] * t2
    c2 = (f1[0] * t0 - f1[1] * t1 + f1[2] * t2 - f1[3] * (f2[1] * f2[8] - f2[2] * f2[7]) + f1[4] * (f2[0] * f2[8] - f2[2] * f2[6]) -
          f1[5] * (f2[0] * f2[7] - f2[1] * f2[6]) + f1[6] * (f2[1] * f2[5] - f2[2] * f2[4]) - f1[7] * (f2[0] * f2[5] - f2[2] * f2[3]) +
          f1[8] * (f2[0] * f2[4] - f2[1] * f2[3]))
    t0 = f1[4] * f1[8] - f1[5] * f1[7]
    t1 = f1[3] * f1[8] - f1[5] * f1[6]
    t2 = f1[3] * f1[7] - f1[4] * f1[6]
    c1 = (f2[0] * t0 - f2[1] * t1 + f2[2] * t2 - f2[3] * (f1[1] * f1[8] - f1[2] * f1[7]) + f2[4] * (f1[0] * f1[8] - f1[2] * f1[6]) -
          f2[5] * (f1[0] * f1[7] - f1[1] * f1[6]) + f2[6] * (f1[1] * f1[5] - f1[2] * f1[4]) - f2[7] * (f1[0] * f1[5] - f1[2] * f1[3]) +
          f2[8] * (f1[0] * f1[4] - f1[1] * f1[3]))
    c0 = f1[0] * t0 - f1[1] * t1 + f1[2] * t2
    n, r = solve_cubic([c0, c1, c2, c3])
    if n < 1 or n > 3:
        return []
    out = []
    for k in range(n):
        lam, mu = r[k], 1.0
        s = f1[8] * r[k] + f2[8]
        F = np.zeros(9)
        if abs(s) > DBL_EPSILON:
            mu = 1.0 / s
            lam *= mu
            F[8] = 1.0
        else:
            F[8] = 0.0
        for i in range(8):
            F[i] = f1[i] * lam + f2[i] * mu
        out.append(F)
    return out


def errors(p0, p1, F):
    """FMEstimatorCallback::computeError: float32 errors of all points against F."""
    x0, y0 = p0[:, 0].astype(np.float64), p0[:, 1].astype(np.float64)
    x1, y1 = p1[:, 0].astype(np.float64), p1[:, 1].astype(np.float64)
    with np.errstate(all="ignore"):
        a = F[0] * x0 + F[1] * y0 + F[2]
        b = F[3] * x0 + F[4] * y0 + F[5]
        c = F[6] * x0 + F[7] * y0 + F[8]
        s2 = 1.0 / (a * a + b * b)
        d2 = x1 * a + y1 * b + c
        a = F[0] * x1 + F[3] * y1 + F[6]
        b = F[1] * x1 + F[4] * y1 + F[7]
        c = F[2] * x1 + F[5] * y1 + F[8]
        s1 = 1.0 / (a * a + b * b)
        d1 = x0 * a + y0 * b + c
        e1, e2 = d1 * d1 * s1, d2 * d2 * s2
        return np.where(e1 < e2, e2, e1).astype(np.float32)


def _near(err, t, rtol=SENS_RTOL):
    with np.errstate(all="ignore"):
        return bool((np.abs(err.astype(np.float64) - float(t)) <= rtol * abs(float(t))).any())


def _collinear(xs, ys, idx):
    """haveCollinearPoints of the seven points idx (float differences, double products)."""
    i = idx[6]
    xi, yi = xs[i], ys[i]
    f32 = np.float32
    for j in range(6):
        dx1 = float(f32(xs[idx[j]] - xi))   # two floats subtracted in double and rounded once to float = their float difference
        dy1 = float(f32(ys[idx[j]] - yi))
        for k in range(j):
            dx2 = float(f32(xs[idx[k]] - xi))
            dy2 = float(f32(ys[idx[k]] - yi))
            if abs(dx2 * dy1 - dy2 * dx1) <= FLT_EPSILON * (abs(dx1) + abs(dy1) + abs(dx2) + abs(dy2)):
                return True
    return False


class SubsetDrawer:
    """getSubset over one RNG stream."""

    def __init__(self, p0, p1, collinear_check=True, rng=None):
        self.n = len(p0)
        self.c0 = ([float(v) for v in p0[:, 0]], [float(v) for v in p0[:, 1]])
        self.c1 = ([float(v) for v in p1[:, 0]], [float(v) for v in p1[:, 1]])
        self.rng = rng or Rng()
        self.check = collinear_check

    def draw(self, max_attempts):
        n, rng = self.n, self.rng
        for _ in range(max_attempts):
            idx = []
            for i in range(7):
                while True:
                    v = rng.next() % n
                    if v not in idx:
                        break
                idx.append(v)
            if self.check and (_collinear(*self.c0, idx) or _collinear(*self.c1, idx)):
                continue
            return idx
        return None


class Result:
    def __init__(self, n):
        self.mask = np.zeros(n, np.uint8)
        self.F = np.zeros(9)
        self.method = METHOD_NONE
        self.iterations = 0
        self.inliers = 0
        self.rng_draws = 0
        self.hypotheses = []   # (subset, [models], [scores]) per iteration run, in draw order
        self.flags = []        # sensitivity: (kind, iteration)

    @property
    def info(self):
        return (self.method, self.iterations, self.inliers, self.rng_draws)


def find_fundamental(p0, p1, thr=1.0, conf=0.999, accept_ge=False, collinear_check=True, basis=null_basis, rng=None):
    """The whole call.  accept_ge / collinear_check / basis / rng exist for the tests' mutation checks."""
    p0 = np.ascontiguousarray(p0, np.float32).reshape(-1, 2)
    p1 = np.ascontiguousarray(p1, np.float32).reshape(-1, 2)
    n = len(p0)
    res = Result(n)
    if thr <= 0:
        thr = 3.0
    if conf < DBL_EPSILON or conf > 1 - DBL_EPSILON:
        conf = 0.99
    if n < 7:
        return res
    if n == 7:
        res.method = METHOD_7POINT
        models = run_7point(p0, p1, list(range(7)), basis)
        res.mask[:] = 1
        res.inliers = 7
        if models:
            res.F = models[0]
        return res
    ransac = n >= 15
    res.method = METHOD_RANSAC if ransac else METHOD_LMEDS
    drawer = SubsetDrawer(p0, p1, collinear_check, rng)
    t = np.float32(thr * thr)
    best, best_F, min_median = 0, None, DBL_MAX
    niters = 1000 if ransac else max(update_num_iters(conf, 0.45, 7, 1000), 3)
    if not ransac and n // 2 < 7:
        res.flags.append(("median_is_fit_residual", -1))
    it = 0
    while it < niters:
        idx = drawer.draw(10000 if ransac else 1000)
        if idx is None:
            if it == 0:
                res.rng_draws = drawer.rng.draws
                return res
            break
        models = run_7point(p0, p1, idx, basis)
        scores = []
        level = best
        for F in models:
            err = errors(p0, p1, F)
            if ransac:
                if _near(err, t):
                    res.flags.append(("error_at_threshold", it))
                good = int((err <= t).sum())
                scores.append(good)
                if (good >= max(best, 6)) if accept_ge else (good > max(best, 6)):
                    best, best_F, res.mask = good, F, (err <= t).astype(np.uint8)
                    niters = update_num_iters(conf, (n - good) / n, 7, niters)
            else:
                med = float(np.sort(err.view(np.int32))[n // 2:n // 2 + 1].view(np.float32)[0])
                scores.append(med)
                if min_median < DBL_MAX and abs(med - min_median) <= LMEDS_RTOL * abs(min_median):
                    res.flags.append(("median_near_minimum", it))
                if med < min_median:
                    min_median, best_F = med, F
        if ransac:
            new_max = [s for s in scores if s > max(level, 6)]
            if len(new_max) > 1 and new_max.count(max(new_max)) > 1:
                res.flags.append(("tie_at_new_maximum", it))
        res.hypotheses.append((idx, models, scores))
        it += 1
    res.iterations = it
    res.rng_draws = drawer.rng.draws
    if ransac:
        if best > 0:
            res.F = best_F
            res.inliers = int(res.mask.sum())
        else:
            res.mask[:] = 0
        return res
    if min_median < DBL_MAX:
        sigma = 2.5 * 1.4826 * (1 + 5.0 / (n - 7)) * math.sqrt(min_median)
        sigma = 0.001 if sigma < 0.001 else sigma
        ts = np.float32(sigma * sigma)
        err = errors(p0, p1, best_F)
        if _near(err, ts, LMEDS_RTOL):
            res.flags.append(("error_at_threshold", -1))
        res.mask = (err <= ts).astype(np.uint8)
        res.inliers = int(res.mask.sum())
        if res.inliers >= 7:
            res.F = best_F
    return res


def normalized_F(F):
    """F scaled to unit Frobenius norm with its largest-magnitude entry positive (for comparisons to a tolerance)."""
    F = np.asarray(F, np.float64).reshape(9)
    nrm = np.linalg.norm(F)
    if nrm == 0 or not np.isfinite(nrm):
        return F
    F = F / nrm
    return F if F[np.argmax(np.abs(F))] > 0 else -F


def scene(seed, n, inlier_ratio, noise, size=(640, 512), dtype=np.float32):
    """Correspondences of a random rigid motion seen by a pin-hole camera of `size`, in pixel coordinates: a fraction inlier_ratio
    of them projections plus Gaussian noise (px), the rest gross outliers -- moved 8 to 80 px off their epipolar line.  Returns
    (p0, p1, is_inlier, F_true) with p1^T F_true p0 = 0 for the noise-free projections."""
    rng = np.random.default_rng(seed)
    w, h = size
    f = 0.9 * w
    K = np.array([[f, 0, w / 2], [0, f, h / 2], [0, 0, 1.0]])
    ang = rng.normal(0, 0.05, 3)
    th = np.linalg.norm(ang)
    kx = np.array([[0, -ang[2], ang[1]], [ang[2], 0, -ang[0]], [-ang[1], ang[0], 0]]) / th
    R = np.eye(3) + math.sin(th) * kx + (1 - math.cos(th)) * kx @ kx
    t = rng.normal(0, 1, 3)
    t = t / np.linalg.norm(t) * 0.3
    u = np.stack([rng.uniform(0, w, n), rng.uniform(0, h, n), np.ones(n)], 1)
    X = (np.linalg.inv(K) @ u.T).T * rng.uniform(3, 12, (n, 1))
    u2 = (K @ ((R @ X.T).T + t).T).T
    u2 = u2[:, :2] / u2[:, 2:]
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    Ki = np.linalg.inv(K)
    F = Ki.T @ tx @ R @ Ki
    p0 = u[:, :2] + rng.normal(0, noise, (n, 2))
    p1 = u2 + rng.normal(0, noise, (n, 2))
    inl = np.zeros(n, bool)
    inl[rng.permutation(n)[:int(round(inlier_ratio * n))]] = True
    line = (F @ u.T).T[:, :2]
    normal = line / np.linalg.norm(line, axis=1, keepdims=True)
    off = rng.uniform(8, 80, n) * rng.choice([-1.0, 1.0], n)
    p1[~inl] += normal[~inl] * off[~inl, None]
    return p0.astype(dtype), p1.astype(dtype), inl, F.reshape(9)
