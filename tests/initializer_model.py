"""numpy model of USLAM::Initializer::Initialize (src/Initializer.cc), the F path that the reference executes (:110 returns
ReconstructF unconditionally), written from the source and from recall of the OpenCV internals it calls [OCV-RECALL]; nothing here
reads the product.  Two computations live side by side:

  * `Model`: the reference's roundings -- fp32 where the reference is fp32, double where OpenCV is.  JacobiSVDImpl_<float> (one-sided
    Jacobi on the rows of At, W in double, eps = 2 FLT_EPSILON, at most 30 sweeps, selection sort descending) and its completion loop
    (cv::RNG(0x12345678), +-1/m by bit 8, two Gram-Schmidt passes with an L1 renormalisation each, then L2) are restated, batched
    over hypotheses: a hypothesis that has converged skips every pair of every later sweep, so running the batch until nobody changes
    is the same as the per-matrix early exit.
  * `independent_*`: double precision throughout and other algorithms: numpy.linalg.svd for the null vector, the rank-2 projection
    and the essential decomposition, a DLT triangulation by numpy.linalg.svd.

tests/test_initializer_model.py measures the distance between the two; four times the worst distances are the tolerances the product
is held to (the constants at the end of this file)."""
import numpy as np

f32, f64 = np.float32, np.float64
FLT_EPSILON = np.float32(1.1920928955078125e-7)
FLT_MIN = 1.1754943508222875e-38
TH, TH_SCORE = np.float32(3.841), np.float32(5.991)
CV_PI = 3.1415926535897932384626433832795


# ---- glibc rand() and DUtils::Random::RandomInt (Thirdparty/DBoW2/DUtils/Random.cpp:47-50) ------------------------------------------
class GlibcRand:
    """TYPE_3 additive feedback generator, srand(seed); the process is never seeded, so seed 1."""

    def __init__(self, seed=1):
        r = [0] * 34
        w = 1 if seed == 0 else seed
        r[0] = w
        for i in range(1, 31):
            hi, lo = divmod(w, 127773)
            w = 16807 * lo - 2836 * hi
            if w < 0:
                w += 2147483647
            r[i] = w
        for i in range(31, 34):
            r[i] = r[i - 31]
        self.r, self.n = r, 0
        for _ in range(310):
            self.next()

    def next(self):
        o = (self.r[-31] + self.r[-3]) & 0xffffffff
        self.r.append(o)
        self.r.pop(0)
        self.n += 1
        return o >> 1

    def random_int(self, lo, hi):
        return int((self.next() / 2147483648.0) * (hi - lo + 1)) + lo


def draw_sets(g, n, iterations):
    """:73-90: eight draws without replacement per iteration, swap with the back."""
    sets = np.zeros((iterations, 8), np.int32)
    for it in range(iterations):
        avail = list(range(n))
        for j in range(8):
            randi = g.random_int(0, len(avail) - 1)
            sets[it, j] = avail[randi]
            avail[randi] = avail[-1]
            avail.pop()
    return sets


# ---- Normalize :741-787 -------------------------------------------------------------------------------------------------------------
def normalize(keys):
    """Serial fp32 sums over ALL keys -> (meanX, meanY, sX, sY) as float32."""
    k = np.asarray(keys, f32)
    mean = np.zeros(2, f32)
    for p in k:
        mean += p
    mean = mean / f32(len(k))
    dev = np.zeros(2, f32)
    for p in k:
        dev += np.abs(p - mean)
    dev = dev / f32(len(k))
    s = (1.0 / dev.astype(f64)).astype(f32)
    return f32(mean[0]), f32(mean[1]), f32(s[0]), f32(s[1])


def normalized(T, pts):
    p = np.asarray(pts, f32)
    return np.stack([(p[..., 0] - T[0]) * T[2], (p[..., 1] - T[1]) * T[3]], -1)


def t_matrix(T):
    return np.array([[T[2], 0, -T[0] * T[2]], [0, T[3], -T[1] * T[3]], [0, 0, 1]], f32)


# ---- JacobiSVDImpl_<float>, batched [OCV-RECALL] -------------------------------------------------------------------------------------
def _hypot(a, b):
    a, b = np.abs(a), np.abs(b)
    hi, lo = np.maximum(a, b), np.minimum(a, b)
    with np.errstate(all="ignore"):
        r = np.where(hi == 0, 0.0, lo / np.where(hi == 0, 1.0, hi))
    return np.where(hi == 0, 0.0, hi * np.sqrt(1.0 + r * r))


def _sumsq(rows):
    """double sum of squares along the last axis, in index order"""
    s = np.zeros(rows.shape[:-1], f64)
    for k in range(rows.shape[-1]):
        s = s + rows[..., k].astype(f64) * rows[..., k].astype(f64)
    return s


def _cv_rng_bits(count):
    s, out = 0x12345678, []
    for _ in range(count):
        s = ((s & 0xffffffff) * 4294883355 + (s >> 32)) & 0xffffffffffffffff
        out.append((s & 0xffffffff) & 256 != 0)
    return out


def jacobi_svd(At, n1):
    """At: [B, n, m] -> (rows [B, n1, m] orthonormal, W [B, n] descending, Vt [B, n, n])."""
    At = np.array(At, f32)
    B, n, m = At.shape
    eps = f32(FLT_EPSILON * f32(2))
    W = _sumsq(At)
    Vt = np.broadcast_to(np.eye(n, dtype=f32), (B, n, n)).copy()
    with np.errstate(all="ignore"):
        for _ in range(30):
            changed = False
            for i in range(n - 1):
                for j in range(i + 1, n):
                    a, b = W[:, i], W[:, j]
                    p = np.zeros(B, f64)
                    for k in range(m):
                        p = p + At[:, i, k].astype(f64) * At[:, j, k].astype(f64)
                    act = ~(np.abs(p) <= f64(eps) * np.sqrt(a * b))
                    if not act.any():
                        continue
                    changed = True
                    p = p * 2
                    beta = a - b
                    gamma = _hypot(p, beta)
                    delta = (gamma - beta) * 0.5
                    s_n = np.sqrt(delta / gamma).astype(f32)
                    c_n = (p / (gamma * s_n.astype(f64) * 2)).astype(f32)
                    c_p = np.sqrt((gamma + beta) / (gamma * 2)).astype(f32)
                    s_p = (p / (gamma * c_p.astype(f64) * 2)).astype(f32)
                    c, s = np.where(beta < 0, c_n, c_p)[:, None], np.where(beta < 0, s_n, s_p)[:, None]
                    x, y = At[:, i, :].copy(), At[:, j, :].copy()
                    t0, t1 = c * x + s * y, -s * x + c * y
                    At[:, i, :] = np.where(act[:, None], t0, x)
                    At[:, j, :] = np.where(act[:, None], t1, y)
                    W[:, i] = np.where(act, _sumsq(t0), a)
                    W[:, j] = np.where(act, _sumsq(t1), b)
                    x, y = Vt[:, i, :].copy(), Vt[:, j, :].copy()
                    Vt[:, i, :] = np.where(act[:, None], c * x + s * y, x)
                    Vt[:, j, :] = np.where(act[:, None], -s * x + c * y, y)
            if not changed:
                break
    W = np.sqrt(_sumsq(At))
    ar = np.arange(B)
    for i in range(n - 1):
        j = np.full(B, i)
        for k in range(i + 1, n):
            j = np.where(W[ar, j] < W[ar, k], k, j)
        wi, wj = W[ar, i].copy(), W[ar, j].copy()
        W[ar, i], W[ar, j] = wj, wi
        ri, rj = At[ar, i].copy(), At[ar, j].copy()
        At[ar, i], At[ar, j] = rj, ri
        vi, vj = Vt[ar, i].copy(), Vt[ar, j].copy()
        Vt[ar, i], Vt[ar, j] = vj, vi
    if (W <= FLT_MIN).any():
        raise NotImplementedError("a singular value at FLT_MIN: the completion loop would also rebuild one of the first n rows")
    rows = np.zeros((B, n1, m), f32)
    rows[:, :n] = At * (1.0 / W).astype(f32)[:, :, None]
    bits = _cv_rng_bits((n1 - n) * m)
    val0 = f32(1.0 / m)
    for i in range(n, n1):
        r = np.array([val0 if bits[(i - n) * m + k] else -val0 for k in range(m)], f32)
        r = np.broadcast_to(r, (B, m)).copy()
        for _ in range(2):
            for j in range(i):
                sd = np.zeros(B, f64)
                for k in range(m):
                    sd = sd + (r[:, k] * rows[:, j, k]).astype(f64)
                r = (r.astype(f64) - sd[:, None] * rows[:, j].astype(f64)).astype(f32)
                asum = np.zeros(B, f32)
                for k in range(m):
                    asum = asum + np.abs(r[:, k])
                with np.errstate(all="ignore"):
                    asum = np.where(asum > eps * f32(100), f32(1) / asum, f32(0)).astype(f32)
                r = r * asum[:, None]
        sd = np.sqrt(_sumsq(r))
        with np.errstate(all="ignore"):
            rows[:, i] = r * np.where(sd > FLT_MIN, 1 / sd, 0.0).astype(f32)[:, None]
    return rows, W, Vt


def svd33(M):
    """cv::SVDecomp of [B, 3, 3] fp32 -> u, w, vt."""
    rows, W, Vt = jacobi_svd(np.swapaxes(np.asarray(M, f32), 1, 2), 3)
    return np.swapaxes(rows, 1, 2).copy(), W.astype(f32), Vt


def mul_small(a, b):
    """cv::gemm's small-matrix path: the fp32 row sum, left to right."""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    out = a[..., :, 0, None] * b[..., 0, None, :]
    for k in range(1, a.shape[-1]):
        out = out + a[..., :, k, None] * b[..., k, None, :]
    return out.astype(f32)


def mul_general(a, b):
    """cv::gemm's general path: double products and sums in index order, one rounding."""
    a, b = np.asarray(a, f32).astype(f64), np.asarray(b, f32).astype(f64)
    out = a[..., :, 0, None] * b[..., 0, None, :]
    for k in range(1, a.shape[-1]):
        out = out + a[..., :, k, None] * b[..., k, None, :]
    return out.astype(f32)


# ---- ComputeF21 :260-295 + :204 -------------------------------------------------------------------------------------------------------
def design_rows(pn1, pn2):
    u1, v1, u2, v2 = pn1[..., 0], pn1[..., 1], pn2[..., 0], pn2[..., 1]
    return np.stack([u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, np.ones_like(u1)], -1).astype(f32)


def compute_f21(pn1, pn2, T1, T2):
    """pn1, pn2: [B, 8, 2] normalised fp32 -> (F21i [B, 3, 3], the completion row [B, 9])."""
    rows, _, _ = jacobi_svd(design_rows(pn1, pn2), 9)
    fpre = rows[:, 8].reshape(-1, 3, 3)
    u, w, vt = svd33(fpre)
    D = np.zeros_like(u)
    D[:, 0, 0], D[:, 1, 1] = w[:, 0], w[:, 1]
    Fn = mul_small(mul_small(u, D), vt)
    F = mul_small(mul_small(t_matrix(T2).T.copy(), Fn), t_matrix(T1))
    return F, rows[:, 8]


# ---- CheckFundamental :381-460 ----------------------------------------------------------------------------------------------------------
def score_terms(F, k1, k2, sigma):
    """F [3, 3] fp32; k1, k2 [N, 2] the matched raw keys -> (terms [N, 2] fp32 with 0 where nothing is added, inlier mask)."""
    F = np.asarray(F, f32).reshape(3, 3)
    inv = f32(1.0 / f64(f32(sigma) * f32(sigma)))
    u1, v1, u2, v2 = k1[:, 0], k1[:, 1], k2[:, 0], k2[:, 1]
    with np.errstate(all="ignore"):
        a2, b2, c2 = F[0, 0] * u1 + F[0, 1] * v1 + F[0, 2], F[1, 0] * u1 + F[1, 1] * v1 + F[1, 2], F[2, 0] * u1 + F[2, 1] * v1 + F[2, 2]
        num2 = a2 * u2 + b2 * v2 + c2
        chi1 = (num2 * num2 / (a2 * a2 + b2 * b2)) * inv
        a1, b1, c1 = F[0, 0] * u2 + F[1, 0] * v2 + F[2, 0], F[0, 1] * u2 + F[1, 1] * v2 + F[2, 1], F[0, 2] * u2 + F[1, 2] * v2 + F[2, 2]
        num1 = a1 * u1 + b1 * v1 + c1
        chi2 = (num1 * num1 / (a1 * a1 + b1 * b1)) * inv
        out1, out2 = chi1 > TH, chi2 > TH
    terms = np.stack([np.where(out1, f32(0), TH_SCORE - chi1), np.where(out2, f32(0), TH_SCORE - chi2)], -1).astype(f32)
    return terms, ~out1 & ~out2


def serial_sum(terms):
    s = f32(0)
    for t in np.asarray(terms, f32).reshape(-1):
        s = f32(s + t)
    return s


def score_bound(terms):
    """What a serial fp32 sum of these terms may differ by from their exact sum (n u sum|t|, u = 2^-24), and the exact sum."""
    t = np.asarray(terms, f64).reshape(-1)
    n = int((t != 0).sum())
    return n * 2.0 ** -24 * np.abs(t).sum(), t.sum()


# ---- DecomposeE :1062-1082, CheckRT :790-904 ----------------------------------------------------------------------------------------------
def k_matrix(cam):
    fx, fy, cx, cy = cam
    return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], f32)


def decompose_e(F, cam):
    K = k_matrix(cam)
    E = mul_small(mul_general(K.T.copy(), np.asarray(F, f32).reshape(3, 3)), K)
    u, _, vt = svd33(E[None])
    u, vt = u[0], vt[0]
    t = u[:, 2].copy()
    t = t * f32(1.0 / np.sqrt((t.astype(f64) ** 2)[0] + (t.astype(f64) ** 2)[1] + (t.astype(f64) ** 2)[2]))
    Wm = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], f32)
    R1 = mul_small(mul_small(u, Wm), vt)
    R2 = mul_small(mul_general(u, Wm.T.copy()), vt)
    if np.linalg.det(R1.astype(f64)) < 0:
        R1 = -R1
    if np.linalg.det(R2.astype(f64)) < 0:
        R2 = -R2
    return R1, R2, t.astype(f32)


def motions(R1, R2, t):
    return [(R1, t), (R2, t), (R1, -t), (R2, -t)]


def check_rt(R, t, cam, k1, k2, inliers, sigma):
    """-> (nGood, parallax fp32, p3d [N, 3], vbGood [N], cosParallax of the counted)."""
    N = len(k2)
    fx, fy, cx, cy = (f32(v) for v in cam)
    K = k_matrix(cam)
    th2 = f32(4.0 * f64(f32(sigma) * f32(sigma)))
    P1 = np.zeros((3, 4), f32)
    P1[:, :3] = K
    P2 = mul_small(K, np.concatenate([R, t[:, None]], 1).astype(f32))
    O2 = (-(R.astype(f64).T[:, 0] * f64(t[0]) + R.astype(f64).T[:, 1] * f64(t[1]) + R.astype(f64).T[:, 2] * f64(t[2]))).astype(f32)
    idx = np.flatnonzero(inliers)
    p3d, good = np.zeros((N, 3), f32), np.zeros(N, bool)
    if len(idx) == 0:
        return 0, f32(0), p3d, good, np.zeros(0, f32)
    a, b = k1[idx], k2[idx]
    A = np.stack([a[:, 0, None] * P1[2] - P1[0], a[:, 1, None] * P1[2] - P1[1], b[:, 0, None] * P2[2] - P2[0], b[:, 1, None] * P2[2] - P2[1]], 1).astype(f32)
    _, _, Vt = jacobi_svd(np.swapaxes(A, 1, 2), 4)
    v = Vt[:, 3]
    with np.errstate(all="ignore"):
        X = (v[:, :3] * (1.0 / v[:, 3].astype(f64)).astype(f32)[:, None]).astype(f32)
        fin = np.isfinite(X).all(1)
        n2 = X - O2
        Xd, n2d = X.astype(f64), n2.astype(f64)
        dist1 = np.sqrt(Xd[:, 0] * Xd[:, 0] + Xd[:, 1] * Xd[:, 1] + Xd[:, 2] * Xd[:, 2]).astype(f32)
        dist2 = np.sqrt(n2d[:, 0] * n2d[:, 0] + n2d[:, 1] * n2d[:, 1] + n2d[:, 2] * n2d[:, 2]).astype(f32)
        cosp = ((Xd[:, 0] * n2d[:, 0] + Xd[:, 1] * n2d[:, 1] + Xd[:, 2] * n2d[:, 2]) / (dist1 * dist2).astype(f64)).astype(f32)
        low = cosp.astype(f64) < 0.99998
        X2 = ((R[:, 0] * X[:, 0, None] + R[:, 1] * X[:, 1, None] + R[:, 2] * X[:, 2, None]).astype(f64) + t.astype(f64)).astype(f32)
        ok = fin & ~((X[:, 2] <= 0) & low) & ~((X2[:, 2] <= 0) & low)
        iz1, iz2 = (1.0 / X[:, 2].astype(f64)).astype(f32), (1.0 / X2[:, 2].astype(f64)).astype(f32)
        e1x, e1y = (fx * X[:, 0] * iz1 + cx) - a[:, 0], (fy * X[:, 1] * iz1 + cy) - a[:, 1]
        e2x, e2y = (fx * X2[:, 0] * iz2 + cx) - b[:, 0], (fy * X2[:, 1] * iz2 + cy) - b[:, 1]
        ok &= ~((e1x * e1x + e1y * e1y) > th2) & ~((e2x * e2x + e2y * e2y) > th2)
    p3d[idx[ok]] = X[ok]
    good[idx[ok & low]] = True
    cs = cosp[ok]
    n_good = int(ok.sum())
    parallax = f32(0)
    if n_good > 0:
        c = np.sort(cs)[min(50, n_good - 1)]
        parallax = f32(f64(f32(np.arccos(f64(c))) * f32(180)) / CV_PI)
    return n_good, parallax, p3d, good, cs


def verdict(n_inliers, n_good, parallax):
    """:491-561 -> (initialized, deciding)."""
    max_good = max(n_good)
    n_min = max(int(0.9 * n_inliers), 50)
    nsimilar = sum(1 for g in n_good if g > 0.7 * max_good)
    deciding = list(n_good).index(max_good)
    if max_good < n_min or nsimilar > 1:
        return False, deciding
    return bool(parallax[deciding] > 1.0), deciding


class Result:
    pass


def initialize(keys1, keys2, matches12, cam, sigma=1.0, iterations=200, g=None, sets=None):
    """The whole call.  -> Result, or None for n2 < 8 (departure: no result, no draws)."""
    keys1, keys2, m12 = np.asarray(keys1, f32), np.asarray(keys2, f32), np.asarray(matches12, np.int64)
    r = Result()
    N = len(keys2)
    r.draws = 0
    if N < 8:
        return None
    r.sets = draw_sets(g, N, iterations) if sets is None else np.asarray(sets)
    r.draws = 8 * iterations
    T1, T2 = normalize(keys1), normalize(keys2)
    pn1, pn2 = normalized(T1, keys1), normalized(T2, keys2)
    r.F, r.null_row = compute_f21(pn1[m12[r.sets]], pn2[r.sets], T1, T2)
    k1 = keys1[m12]
    r.scores, masks = np.zeros(iterations, f32), []
    for it in range(iterations):
        terms, mask = score_terms(r.F[it], k1, keys2, sigma)
        r.scores[it] = serial_sum(terms)
        masks.append(mask)
    r.best, best_score = -1, f32(0)
    for it in range(iterations):
        if r.scores[it] > best_score:
            r.best, best_score = it, r.scores[it]
    order = np.sort(r.scores[np.isfinite(r.scores)])[::-1]
    r.top_gap = float((order[0] - order[1]) / order[0]) if len(order) > 1 and order[0] > 0 else 1.0
    r.initialized, r.deciding, r.n_inliers = False, -1, 0
    r.n_good, r.parallax = [0] * 4, [f32(0)] * 4
    r.R21, r.t21, r.p3d, r.triangulated = np.zeros((3, 3), f32), np.zeros(3, f32), np.zeros((N, 3), f32), np.zeros(N, bool)
    r.inliers = np.zeros(N, bool)
    if r.best < 0:
        return r
    r.score, r.F21, r.inliers = best_score, r.F[r.best], masks[r.best]
    r.n_inliers = int(r.inliers.sum())
    r.R1, r.R2, r.t = decompose_e(r.F21, cam)
    per = [check_rt(R, t, cam, k1, keys2, r.inliers, sigma) for R, t in motions(r.R1, r.R2, r.t)]
    r.n_good, r.parallax = [p[0] for p in per], [p[1] for p in per]
    r.initialized, r.deciding = verdict(r.n_inliers, r.n_good, r.parallax)
    if r.initialized:
        r.R21, r.t21 = motions(r.R1, r.R2, r.t)[r.deciding]
        r.p3d, r.triangulated = per[r.deciding][2], per[r.deciding][3]
    return r


# ---- the independent double-precision computation ------------------------------------------------------------------------------------------
def unit(v):
    v = np.asarray(v, f64)
    return v / np.linalg.norm(v)


def sign_free_distance(a, b):
    """Distance between two directions known up to sign (both scaled to unit norm)."""
    a, b = unit(np.ravel(a)), unit(np.ravel(b))
    return float(min(np.linalg.norm(a - b), np.linalg.norm(a + b)))


def independent_f21(pn1, pn2, T1, T2):
    """One hypothesis, doubles: (F21 [3, 3], null vector [9]) from the fp32 normalised points the reference's SVD sees."""
    A = design_rows(np.asarray(pn1, f32), np.asarray(pn2, f32)).astype(f64)
    null = np.linalg.svd(A)[2][8]
    u, w, vt = np.linalg.svd(null.reshape(3, 3))
    Fn = u @ np.diag([w[0], w[1], 0.0]) @ vt
    return t_matrix(T2).astype(f64).T @ Fn @ t_matrix(T1).astype(f64), null


def independent_pose(F, cam, keys1, keys2, matches12, inliers):
    """Essential decomposition and DLT in doubles; the motion of the four with most points in front of both cameras.
    -> (R, t, points [N, 3] (NaN where not an inlier))."""
    K = k_matrix(cam).astype(f64)
    E = K.T @ np.asarray(F, f64).reshape(3, 3) @ K
    u, _, vt = np.linalg.svd(E)
    Wm = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], f64)
    cands = []
    for R in (u @ Wm @ vt, u @ Wm.T @ vt):
        R = R if np.linalg.det(R) > 0 else -R
        for t in (u[:, 2], -u[:, 2]):
            cands.append((R, t / np.linalg.norm(t)))
    k1, k2 = np.asarray(keys1, f64)[np.asarray(matches12)], np.asarray(keys2, f64)
    best = None
    for R, t in cands:
        P1, P2 = K @ np.eye(3, 4), K @ np.concatenate([R, t[:, None]], 1)
        pts = np.full((len(k2), 3), np.nan)
        front = 0
        for i in np.flatnonzero(inliers):
            A = np.stack([k1[i, 0] * P1[2] - P1[0], k1[i, 1] * P1[2] - P1[1], k2[i, 0] * P2[2] - P2[0], k2[i, 1] * P2[2] - P2[1]])
            v = np.linalg.svd(A)[2][3]
            X = v[:3] / v[3]
            pts[i] = X
            front += int(X[2] > 0 and (R @ X + t)[2] > 0)
        if best is None or front > best[0]:
            best = (front, R, t, pts)
    return best[1], best[2], best[3]


# ---- tolerances: four times the worst distance between Model and independent_* over the scene set of tests/initializer_checks.py
# (model_scenes()), measured by tests/test_initializer_model.py, which asserts that the measured values do not exceed these yardsticks.
# The factor four is Sim3Solver's Horn margin: it covers a legal difference in OpenCV-internal operation order nobody here can pin.
# F and the completion row are compared as unit vectors up to sign; R by the largest element difference, t as a unit vector, points
# relative to their norm.
MEASURED_NULL_ROW = 2.320e-4   # measured 2.3191e-4: an ill-conditioned minimal set of a 200-point scene
MEASURED_F = 1.232e-3          # measured 1.2314e-3: the same kind of set after the rank-2 projection and the denormalisation
MEASURED_R = 1.609e-7          # measured 1.6088e-7 (7 accepted scenes)
MEASURED_T = 3.092e-8          # measured 3.0917e-8
MEASURED_POINT = 2.525e-6      # measured 2.5249e-6, relative to the point's norm
TOL_NULL_ROW, TOL_F, TOL_R, TOL_T, TOL_POINT = (4 * v for v in (MEASURED_NULL_ROW, MEASURED_F, MEASURED_R, MEASURED_T, MEASURED_POINT))
