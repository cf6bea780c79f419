"""Test model of USLAM::PnPsolver as Tracking::Relocalisation drives it, written from the reference's src/PnPsolver.cc and
Thirdparty/DBoW2/DUtils/Random.cpp (line numbers below are theirs) and from glibc's random_r.c for the generator.  Python ints and
numpy; independent of csrc/pnpsolver_core.hpp, which never imports it.  Test infrastructure only.

What is modelled exactly: the random stream, the subset draw (with its repeated points), SetRansacParameters, CheckInliers of a given
pose, and iterate()'s loop over given counts and given Refine() outcomes.  What is not: the EPnP of a minimal set -- on 4 points the
system has a null space of dimension four and the pose is rounding noise of the eigen-solver; refits on 6 points
or more are compared with pnp_model.epnp.
"""
import math

import numpy as np

import pnp_model as pm

RAND_MAX = 2147483647
SENS_RTOL = 1e-5          # CheckInliers: an error within this (relative) of its threshold may fall either way
CALL_SITE = dict(probability=0.99, min_inliers=10, max_iterations=300, min_set=4, epsilon=0.5, th2=5.991)   # Tracking.cc:2425
# SetRansacParameters at the call site's arguments: N -> (nMinInliers, mRansacMaxIts)
CALL_SITE_TABLE = {10: (10, 1), 15: (10, 14), 19: (10, 30), 20: (10, 35), 21: (10, 35), 40: (20, 35), 100: (50, 35), 1000: (500, 35)}
NONE, REFINED, BEST_AT_EXHAUSTION = 0, 1, 2


# ---- glibc srand / rand: TYPE_3, degree 31, separation 3 (random_r.c) ------------------------------------------------------------
class GlibcRand:
    def __init__(self, seed=1):
        seed = 1 if seed == 0 else seed
        r = [seed]
        for _ in range(30):
            w = r[-1]
            hi, lo = int(w / 127773), w - 127773 * int(w / 127773)     # C division truncates; w >= 0 here
            w = 16807 * lo - 2836 * hi
            if w < 0:
                w += 2147483647
            r.append(w)
        self.hist = r + r[:3]            # 34 words
        self.outputs = 0
        for _ in range(310):
            self._step()

    def _step(self):
        o = (self.hist[-31] + self.hist[-3]) & 0xffffffff
        self.hist.append(o)
        del self.hist[0]
        return o >> 1

    def next(self):
        self.outputs += 1
        return self._step()

    def random_int(self, lo, hi):
        """DUtils::Random::RandomInt, Random.cpp:47-50."""
        d = self.next() / (RAND_MAX + 1.0)
        return int(d * (hi - lo + 1)) + lo


def draw_subset(g, n, min_set):
    """:189-202 as written: slot idx is overwritten, not slot randi.  The vector's storage keeps n slots; pop_back only shortens it."""
    avail = list(range(n))
    live = n
    out = []
    for _ in range(min_set):
        randi = g.random_int(0, live - 1)
        idx = avail[randi]
        out.append(idx)
        avail[idx] = avail[live - 1]
        live -= 1
    return out


def draw_subset_intended(g, n, min_set):
    """What the code means to do (remove the drawn slot): the same draws give the same set until a point would repeat."""
    avail = list(range(n))
    out = []
    for _ in range(min_set):
        randi = g.random_int(0, len(avail) - 1)
        out.append(avail[randi])
        avail[randi] = avail[-1]
        avail.pop()
    return out


# ---- SetRansacParameters :122-158 --------------------------------------------------------------------------------------------------
def derive_params(n, probability, min_inliers, max_iterations, min_set, epsilon, th2=None):
    """-> (nMinInliers, mRansacMaxIts)."""
    f32 = np.float32
    eps = f32(epsilon)
    m = int(f32(n) * eps)
    m = max(m, min_inliers, min_set)
    if eps < f32(m) / f32(n):
        eps = f32(m) / f32(n)
    if m == n:
        its = 1
    else:
        with np.errstate(all="ignore"):
            den = math.log(1.0 - math.pow(float(eps), 3)) if float(eps) < 1.0 else -math.inf
            q = math.log(1.0 - probability) / den if den != 0 else math.inf
        its = max_iterations if not (q < max_iterations) else int(math.ceil(q))
    return m, max(1, min(its, max_iterations))


# ---- CheckInliers :309-340 ---------------------------------------------------------------------------------------------------------
def check_inliers(pose, p3d, p2d, K, max_err):
    """pose float64[12] (R row-major, t) -> (error2 float32[n], inlier mask, near mask: within SENS_RTOL of the threshold)."""
    f32, f64 = np.float32, np.float64
    R, t = np.asarray(pose[:9], f64).reshape(3, 3), np.asarray(pose[9:], f64)
    P, m = np.asarray(p3d, f32).astype(f64), np.asarray(p2d, f32)
    fu, fv, uc, vc = (float(f32(v)) for v in K)
    with np.errstate(all="ignore"):
        Xc = (R[0, 0] * P[:, 0] + R[0, 1] * P[:, 1] + R[0, 2] * P[:, 2] + t[0]).astype(f32)
        Yc = (R[1, 0] * P[:, 0] + R[1, 1] * P[:, 1] + R[1, 2] * P[:, 2] + t[1]).astype(f32)
        iZ = (1.0 / (R[2, 0] * P[:, 0] + R[2, 1] * P[:, 1] + R[2, 2] * P[:, 2] + t[2])).astype(f32)
        ue = uc + fu * Xc.astype(f64) * iZ.astype(f64)
        ve = vc + fv * Yc.astype(f64) * iZ.astype(f64)
        dx = (m[:, 0].astype(f64) - ue).astype(f32)
        dy = (m[:, 1].astype(f64) - ve).astype(f32)
        e2 = (dx * dx).astype(f32) + (dy * dy).astype(f32)
        thr = np.asarray(max_err, f32)
        inl = e2 < thr
        near = np.abs(e2.astype(f64) - thr.astype(f64)) <= SENS_RTOL * thr.astype(f64)
    return e2, inl, near


def max_error(sigma2, th2):
    return np.asarray(sigma2, np.float32) * np.float32(th2)


# ---- iterate :166-259 over given counts and given Refine() outcomes ----------------------------------------------------------------
def iterations_ahead(iterations, max_its, n_iterations):
    return max(max_its - iterations, n_iterations, 0)


def replay(iterations, best, counts, script, carried, n_iterations, max_its, min_inliers):
    """One iterate(n_iterations) call on a solver with N >= nMinInliers.  counts[h]: inliers of the h-th hypothesis of this call;
    script[h]: what Refine() counts on the best set taken at hypothesis h; carried: the same for the set kept from earlier calls.
    -> dict(performed, returned, no_more, inliers, iterations, best, best_from (hypothesis whose set is the best now, -1: carried),
    refines (how often Refine() was consulted))."""
    cur, current, best_from, refines = 0, carried, -1, 0
    while iterations < max_its or cur < n_iterations:
        c = int(counts[cur])
        cur += 1
        iterations += 1
        if c >= min_inliers:
            if c > best:
                best, current, best_from = c, int(script[cur - 1]), cur - 1
            refines += 1
            if current > min_inliers:
                return dict(performed=cur, returned=REFINED, no_more=0, inliers=current, iterations=iterations, best=best, best_from=best_from,
                            refines=refines)
    out = dict(performed=cur, returned=NONE, no_more=1, inliers=0, iterations=iterations, best=best, best_from=best_from, refines=refines)
    if best >= min_inliers:
        out.update(returned=BEST_AT_EXHAUSTION, inliers=best)
    return out


# ---- scenes ------------------------------------------------------------------------------------------------------------------------
def candidate(seed, n, inlier_ratio, noise_px=0.5, n_matches=None):
    """One candidate key frame's correspondences: (p3d, p2d, sigma2, kp_index, n_matches, K, R_true, t_true).  The key points are
    undistorted already (mvKeysUn), so the camera has no distortion; sigma2 is 1.2^(2 octave) for octaves 0..7."""
    cam, obj, img, R, t, _ = pm.scene(seed, n, inlier_ratio, noise_px, pm.PLAIN)
    rng = np.random.default_rng(seed + 7919)
    sigma2 = (np.float32(1.2) ** (2 * rng.integers(0, 8, n))).astype(np.float32)
    nm = n if n_matches is None else n_matches
    kp = np.sort(rng.permutation(nm)[:n]).astype(np.int32)
    return obj, img, sigma2, kp, nm, cam.K, R, t


def refit(p3d, p2d, K, inlier_indices):
    """Refine()'s EPnP on the listed points by the independent model (pnp_model.epnp): (R, t) or None."""
    idx = np.asarray(inlier_indices, np.int64)
    r = pm.epnp(np.asarray(p3d, np.float32)[idx].astype(np.float64), np.asarray(p2d, np.float32)[idx].astype(np.float64),
                tuple(float(np.float32(v)) for v in K))
    return None if r is None else (r[0], r[1])
