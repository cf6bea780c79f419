"""The projection prologues of the ORBmatcher search loops, restated in numpy from the reference source, a real-valued evaluator of the
same quantities, and the scenes that tests/test_projection_model.py (CPU) and tests/test_gpu_projection.py (GPU) run them on.

The six prologues (what uvo_project_points' five modes and uvo_project_sim3 compute per map point):
  FRUSTUM        FrameKTL::isInFrustum src/FrameKTL.cc:299-357 with MapPoint::PredictScale src/MapPoint.cc:373-388
  KF_RELOC       SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) src/ORBmatcher.cc:1626-1669
  FUSE           Fuse(pKF, vpMapPoints, th) src/ORBmatcher.cc:1043-1080 with KeyFrame::IsInImage src/KeyFrame.cc:994-997
  PIXEL_BOUNDED  SearchByProjection(CurrentFrame, LastFrame, th) src/ORBmatcher.cc:1529-1542
  PIXEL          SearchByProjection(F1, F2, windowSize, ...) src/ORBmatcher.cc:541-549
  SIM3           SearchBySim3, either direction, src/ORBmatcher.cc:1329-1360 (model-only mode number 5)
The invariance distances are the C ABI's: MapPoint::GetMin/MaxDistanceInvariance() (src/MapPoint.cc:344-354) as given, and the raw
mfMaxDistance for PredictScale.  Outputs are as the ABI writes them: u, v, level and view_cos are 0 where valid is 0.

Arithmetic.  Every fp32 step is an np.float32 operation in the reference's expression order.  The double intermediates are np.float64
in index order: `1.0 / z`, cv::norm and cv::Mat::dot (double accumulators), the `+ t` of the 3x3 product (cv::gemm's small-matrix
path: fp32 row sum, then `t0 * alpha + t * beta` in double; the unpinned assumption of DESIGN.md section 4) and `-Rcw.t() * tcw`
(general path: double accumulation, times alpha = -1).  The logarithm is the platform's logf through ctypes.  `(int)` of a float
that is not below 2^31 (+inf and NaN included) is INT_MIN, as x86-64's cvttss2si gives it.

The evaluator takes the inputs as exact fp32 values and works in np.longdouble.  Per point and per test it returns the signed margin
to the boundary: the test passes iff margin >= 0, or margin > 0 for a test in STRICT (the open upper image bounds of IsInImage).
"""
import ctypes
import ctypes.util

import numpy as np

f32, f64, LD = np.float32, np.float64, np.longdouble
FRUSTUM, KF_RELOC, FUSE, PIXEL_BOUNDED, PIXEL, SIM3 = range(6)
MODE_NAMES = ("frustum", "kf_reloc", "fuse", "pixel_bounded", "pixel", "sim3")
INT_MIN = -2 ** 31
EPS = 2.0 ** -24

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.logf.restype = ctypes.c_float
_libm.logf.argtypes = [ctypes.c_float]


def logf(x):
    """libm's logf on every element of a float32 array."""
    x = np.asarray(x, f32)
    return np.array([_libm.logf(ctypes.c_float(float(v))) for v in x.ravel()], f32).reshape(x.shape)


class Cam:
    """uvo_camera_pose.  array() is its memory image: rcw[9], tcw[3], ow[3], fx, fy, cx, cy, min_x, max_x, min_y, max_y."""

    def __init__(self, rcw, tcw, ow, fx=256.0, fy=256.0, cx=320.0, cy=240.0, bounds=(0.0, 640.0, 0.0, 480.0)):
        self.rcw, self.tcw, self.ow = np.array(rcw, f32).reshape(9), np.array(tcw, f32).reshape(3), np.array(ow, f32).reshape(3)
        self.fx, self.fy, self.cx, self.cy = f32(fx), f32(fy), f32(cx), f32(cy)
        self.min_x, self.max_x, self.min_y, self.max_y = [f32(b) for b in bounds]

    def array(self):
        return np.concatenate([self.rcw, self.tcw, self.ow, f32([self.fx, self.fy, self.cx, self.cy, self.min_x, self.max_x, self.min_y, self.max_y])]).astype(f32)

    def with_ow(self, ow):
        return Cam(self.rcw, self.tcw, ow, self.fx, self.fy, self.cx, self.cy, (self.min_x, self.max_x, self.min_y, self.max_y))


# ---- the model ---------------------------------------------------------------------------------------------------------------------

def _affine(R, P, t):
    """cv::Mat 3x3 * 3x1 + 3x1 (CV_32F): the row sum in fp32, left to right; `+ t` through double."""
    out = []
    for i in range(3):
        t0 = (R[3 * i] * P[:, 0] + R[3 * i + 1] * P[:, 1]) + R[3 * i + 2] * P[:, 2]
        out.append((t0.astype(f64) * 1.0 + f64(t[i]) * 1.0).astype(f32))
    return out


def derived_ow(rcw, tcw):
    """Ow = -Rcw.t() * tcw, src/ORBmatcher.cc:1628"""
    ow = np.zeros(3, f32)
    for c in range(3):
        s = f64(0)
        for k in range(3):
            s = s + f64(rcw[3 * k + c]) * f64(tcw[k])
        ow[c] = f32(s * -1.0)
    return ow


def _to_int(q):
    """(int) of a float as x86-64 converts it: truncation; INT_MIN where the value does not fit (+-inf and NaN included)"""
    fits = (q < f32(2.0 ** 31)) & (q >= f32(-2.0 ** 31))
    return np.where(fits, np.where(fits, q, 0).astype(np.int64), INT_MIN)


def predict_scale(max_raw, dist, log_sf, nlevels):
    """MapPoint::PredictScale src/MapPoint.cc:373-388 -> (level, ratio, ceil(log(ratio) / mfLogScaleFactor))"""
    ratio = max_raw / dist
    q = np.ceil(logf(ratio) / f32(log_sf)).astype(f32)
    n = _to_int(q)
    return np.where(n < 0, 0, np.where(n >= nlevels, nlevels - 1, n)).astype(np.int32), ratio, q


def lower_bound(sf, ratio):
    """std::lower_bound(sf.begin(), sf.end(), ratio) - sf.begin(): libstdc++'s bisection, per element of ratio"""
    n = len(ratio)
    first, count = np.zeros(n, np.int64), np.full(n, len(sf), np.int64)
    while (count > 0).any():
        act = count > 0
        step = count // 2
        it = first + step
        lt = act & (sf[np.minimum(it, len(sf) - 1)] < ratio)
        first = np.where(lt, it + 1, first)
        count = np.where(lt, count - step - 1, np.where(act, step, count))
    return first


def _finish(ok, u, v, level, vc, inter, full):
    ok = ok.astype(np.uint8)
    z = ok == 0
    out = (ok, np.where(z, f32(0), u).astype(f32), np.where(z, f32(0), v).astype(f32), np.where(z, 0, level).astype(np.int32),
           np.where(z, f32(0), vc).astype(f32))
    return out + (inter,) if full else out


def project_points(mode, cam, xyz, normal, min_inv, max_inv, max_raw, usable, sf, scale_factor=1.2, cos_limit=0.5, full=False):
    """uvo_project_points -> (valid u8, u, v, level i32, view_cos)[, the intermediates].  Arrays the mode does not read may be None."""
    xyz = np.asarray(xyz, f32).reshape(-1, 3)
    n, sf, nlevels = len(xyz), np.asarray(sf, f32), len(sf)
    ok = np.ones(n, bool) if usable is None else np.asarray(usable) != 0
    level, vc = np.zeros(n, np.int32), np.zeros(n, f32)
    inter = {}
    with np.errstate(all="ignore"):
        X, Y, Z = _affine(cam.rcw, xyz, cam.tcw)
        inter.update(X=X, Y=Y, Z=Z)
        if mode == FUSE:
            ok &= ~(Z < f32(0.0))                                    # :1047
            invz = f32(1) / Z                                        # :1050
            u, v = cam.fx * (X * invz) + cam.cx, cam.fy * (Y * invz) + cam.cy
            ok &= (u >= cam.min_x) & (u < cam.max_x) & (v >= cam.min_y) & (v < cam.max_y)     # KeyFrame::IsInImage
        else:
            if mode == FRUSTUM:
                ok &= ~(Z.astype(f64) < 0.0)                         # src/FrameKTL.cc:313
            invz = (1.0 / Z.astype(f64)).astype(f32)                 # :317
            u, v = cam.fx * X * invz + cam.cx, cam.fy * Y * invz + cam.cy
            if mode != PIXEL:
                ok &= ~((u < cam.min_x) | (u > cam.max_x)) & ~((v < cam.min_y) | (v > cam.max_y))
        inter.update(u=u, v=v)
        if mode in (FRUSTUM, KF_RELOC, FUSE):
            ow = derived_ow(cam.rcw, cam.tcw) if mode == KF_RELOC else cam.ow
            PO = xyz - ow[None, :]
            s2 = np.zeros(n, f64)
            for k in range(3):
                s2 = s2 + PO[:, k].astype(f64) * PO[:, k].astype(f64)
            dist = np.sqrt(s2).astype(f32)
            inter.update(dist=dist)
            min_inv = np.asarray(min_inv, f32)
            if mode != KF_RELOC:
                max_inv, normal = np.asarray(max_inv, f32), np.asarray(normal, f32).reshape(-1, 3)
                ok &= ~((dist < min_inv) | (dist > max_inv))
                dot = np.zeros(n, f64)
                for k in range(3):
                    dot = dot + PO[:, k].astype(f64) * normal[:, k].astype(f64)
                inter.update(dot=dot)
                if mode == FUSE:
                    ok &= ~(dot < 0.5 * dist.astype(f64))            # :1073
                else:
                    vc = (dot / dist.astype(f64)).astype(f32)        # src/FrameKTL.cc:338
                    ok &= ~(vc < f32(cos_limit))
                    inter.update(vc=vc)
            if mode == FRUSTUM:
                level, ratio, q = predict_scale(np.asarray(max_raw, f32), dist, logf(f32(scale_factor)), nlevels)
                inter.update(ratio=ratio, q=q)
            else:
                ratio = dist / min_inv
                level = np.minimum(lower_bound(sf, ratio), nlevels - 1)
                inter.update(ratio=ratio)
    return _finish(ok, u, v, level, vc, inter, full)


def project_sim3(r_own, t_own, s_r, t, cam, xyz, min_inv, max_inv, usable, sf, full=False):
    """uvo_project_sim3 -> (valid u8, u, v, level i32)[, the intermediates]"""
    xyz = np.asarray(xyz, f32).reshape(-1, 3)
    n, sf = len(xyz), np.asarray(sf, f32)
    r_own, t_own, s_r, t = np.asarray(r_own, f32).reshape(9), np.asarray(t_own, f32).reshape(3), np.asarray(s_r, f32).reshape(9), np.asarray(t, f32).reshape(3)
    min_inv, max_inv = np.asarray(min_inv, f32), np.asarray(max_inv, f32)
    ok = np.ones(n, bool) if usable is None else np.asarray(usable) != 0
    with np.errstate(all="ignore"):
        Q = np.stack(_affine(r_own, xyz, t_own), 1)                  # :1330
        X, Y, Z = _affine(s_r, Q, t)                                 # :1331
        ok &= ~(Z.astype(f64) < 0.0)                                 # :1334
        invz = (1.0 / Z.astype(f64)).astype(f32)                     # :1337
        u, v = cam.fx * (X * invz) + cam.cx, cam.fy * (Y * invz) + cam.cy
        ok &= (u >= cam.min_x) & (u < cam.max_x) & (v >= cam.min_y) & (v < cam.max_y)
        s2 = np.zeros(n, f64)
        for c in (X, Y, Z):
            s2 = s2 + c.astype(f64) * c.astype(f64)
        dist = np.sqrt(s2).astype(f32)                               # cv::norm(p3Dc2) :1350
        ok &= ~((dist < min_inv) | (dist > max_inv))
        ratio = dist / min_inv
        level = np.minimum(lower_bound(sf, ratio), len(sf) - 1)
    inter = dict(X=X, Y=Y, Z=Z, u=u, v=v, dist=dist, ratio=ratio)
    out = _finish(ok, u, v, level, np.zeros(n, f32), inter, full)
    return out[:4] + out[5:]


# ---- the real-valued evaluator -----------------------------------------------------------------------------------------------------

STRICT = ("u_max_open", "v_max_open")


def _aff_ld(R, P, t):
    """-> the three components of R P + t, and of |R| |P| + |t| (what one rounding error of the fp32 evaluation is relative to)"""
    R, t = np.asarray(R, LD).reshape(3, 3), np.asarray(t, LD)
    return [R[i, 0] * P[:, 0] + R[i, 1] * P[:, 1] + R[i, 2] * P[:, 2] + t[i] for i in range(3)], \
           [abs(R[i, 0] * P[:, 0]) + abs(R[i, 1] * P[:, 1]) + abs(R[i, 2] * P[:, 2]) + abs(t[i]) for i in range(3)]


def evaluate(mode, cam, xyz, normal, min_inv, max_inv, max_raw, sf, scale_factor=1.2, cos_limit=0.5, chain=None):
    """The quantities of the prologue in np.longdouble from the inputs as exact fp32 values.  chain = (r_own, t_own, s_r, t) for SIM3.
    -> dict: u, v, Z, dist, cos (FRUSTUM: dot / dist; FUSE: dot - dist / 2), ratio, q, level, valid, margins {test: array}, and
    forms {quantity: array}: the magnitude that one fp32 rounding error of that quantity is relative to (the forward-error form)."""
    P = np.asarray(xyz, f32).reshape(-1, 3).astype(LD)
    n, sf = len(P), np.asarray(sf, f32)
    E, M, F = {}, {}, {}
    with np.errstate(all="ignore"):
        if mode == SIM3:
            (Q0, Q1, Q2), aq = _aff_ld(chain[0], P, chain[1])
            Q = np.stack([Q0, Q1, Q2], 1)
            (X, Y, Z), a = _aff_ld(chain[2], Q, chain[3])
            S = np.abs(np.asarray(chain[2], LD).reshape(3, 3))
            a = [a[i] + S[i, 0] * aq[0] + S[i, 1] * aq[1] + S[i, 2] * aq[2] for i in range(3)]
        else:
            (X, Y, Z), a = _aff_ld(cam.rcw, P, cam.tcw)
        fx, fy, cx, cy = LD(cam.fx), LD(cam.fy), LD(cam.cx), LD(cam.cy)
        u, v = fx * X / Z + cx, fy * Y / Z + cy
        E.update(X=X, Y=Y, Z=Z, u=u, v=v)
        F["u"] = fx * a[0] / abs(Z) + fx * abs(X) * a[2] / (Z * Z) + abs(u)
        F["v"] = fy * a[1] / abs(Z) + fy * abs(Y) * a[2] / (Z * Z) + abs(v)
        F["Z"] = a[2]
        if mode in (FRUSTUM, FUSE, SIM3):
            M["depth"] = Z + LD(0)
        half_open = mode in (FUSE, SIM3)
        if mode != PIXEL:
            M["u_min"], M["v_min"] = u - LD(cam.min_x), v - LD(cam.min_y)
            M["u_max_open" if half_open else "u_max"], M["v_max_open" if half_open else "v_max"] = LD(cam.max_x) - u, LD(cam.max_y) - v
        level = np.zeros(n, np.int64)
        if mode in (FRUSTUM, KF_RELOC, FUSE, SIM3):
            if mode == SIM3:
                dist = np.sqrt(X * X + Y * Y + Z * Z)
                F["dist"] = np.sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2])
            else:
                if mode == KF_RELOC:
                    R, t = np.asarray(cam.rcw, LD).reshape(3, 3), np.asarray(cam.tcw, LD)
                    ow = -(R.T @ t)
                    aow = np.abs(R.T) @ np.abs(t)
                else:
                    ow = np.asarray(cam.ow, LD)
                    aow = np.abs(ow)
                PO = P - ow[None, :]
                dist = np.sqrt((PO * PO).sum(1))
                F["dist"] = (np.abs(P) + aow[None, :]).sum(1)
            E["dist"] = dist
            mn = np.asarray(min_inv, f32).astype(LD)
            if mode != KF_RELOC:
                mx = np.asarray(max_inv, f32).astype(LD)
                M["dist_min"], M["dist_max"] = dist - mn, mx - dist
            if mode in (FRUSTUM, FUSE):
                N = np.asarray(normal, f32).reshape(-1, 3).astype(LD)
                dot = (PO * N).sum(1)
                adot = (np.abs(PO) * np.abs(N)).sum(1)
                if mode == FRUSTUM:
                    E["cos"] = dot / dist
                    M["cos"] = E["cos"] - LD(f32(cos_limit))
                    F["cos"] = adot / dist
                else:
                    E["cos"] = dot - dist / 2
                    M["cos"] = E["cos"]
                    F["cos"] = adot + dist / 2
            if mode == FRUSTUM:
                ratio = np.asarray(max_raw, f32).astype(LD) / dist
                lsf = np.log2(LD(f32(scale_factor)))
                q = np.log2(ratio) / lsf
                E.update(ratio=ratio, q=q)
                F["q"] = (1 + abs(np.log(ratio))) / np.log(LD(f32(scale_factor))) * (1 + F["dist"] / dist)
                c = np.ceil(q)
                M["level"] = np.minimum(q - np.floor(q), c - q)          # distance to the nearest integer (never negative)
                level = np.where(np.isfinite(c), np.clip(np.where(np.isfinite(c), c, 0), 0, len(sf) - 1), 0).astype(np.int64)
            else:
                ratio = dist / mn
                E["ratio"] = ratio
                F["ratio"] = F["dist"] / mn + ratio
                level = np.minimum((sf.astype(LD)[None, :] < ratio[:, None]).sum(1), len(sf) - 1)
                M["level"] = np.abs(sf.astype(LD)[None, :] - ratio[:, None]).min(1)  # distance to the nearest table entry
        valid = np.ones(n, bool)
        for k, m in M.items():
            if k != "level":
                valid &= (m > 0) if k in STRICT else (m >= 0)
    E.update(level=level, valid=valid, margins=M, forms=F)
    return E


# ---- scenes --------------------------------------------------------------------------------------------------------------------------
# A scene is a dict of the arrays for a direct call of the C entry points:
#   cam (Cam), chain (r_own, t_own, s_r, t) or None, xyz, normal, min_inv, max_inv, max_raw, usable (all ones; tests mask it), and
#   mf_min / mf_max: the MapPoint members mfMinDistance / mfMaxDistance that give these bounds (0.8f x, 1.2f x) where such members
#   exist, and `linked`: whether they do -- the oracle takes the members, so only linked points can be put to it.

T8 = f32([1, 1.25, 1.5, 2, 2.5, 3, 4, 5])                     # ascending, dyadic
T8_REPEATED = f32([1, 1, 1.5, 1.5, 2, 2, 4, 4])
T1 = f32([1])
SF12 = (f32(1.2) ** np.arange(8)).astype(f32)                 # the table of the generic scenes


def members_for(min_inv, max_inv, max_raw):
    """-> mf_min, mf_max, linked: members with 0.8f * mf_min == min_inv and 1.2f * mf_max == max_inv, mf_max == max_raw"""
    min_inv, max_inv, max_raw = np.asarray(min_inv, f32), np.asarray(max_inv, f32), np.asarray(max_raw, f32)
    with np.errstate(all="ignore"):
        guess = (min_inv.astype(f64) / f64(f32(0.8))).astype(f32)
        mf_min, found = guess.copy(), np.zeros(len(guess), bool)
        for cand in (guess, np.nextafter(guess, f32(np.inf)), np.nextafter(guess, f32(-np.inf))):
            hit = ~found & ((f32(0.8) * cand).view(np.uint32) == min_inv.view(np.uint32))
            mf_min[hit], found = cand[hit], found | hit
        linked = found & ((f32(1.2) * max_raw).view(np.uint32) == max_inv.view(np.uint32))
    return mf_min, max_raw.copy(), linked


def _scene(cam, chain, xyz, normal, min_inv, max_inv, max_raw, **extra):
    xyz, normal = np.ascontiguousarray(xyz, f32).reshape(-1, 3), np.ascontiguousarray(normal, f32).reshape(-1, 3)
    s = dict(cam=cam, chain=chain, xyz=xyz, normal=normal, min_inv=np.ascontiguousarray(min_inv, f32), max_inv=np.ascontiguousarray(max_inv, f32),
             max_raw=np.ascontiguousarray(max_raw, f32), usable=np.ones(len(xyz), np.uint8))
    s["mf_min"], s["mf_max"], s["linked"] = members_for(s["min_inv"], s["max_inv"], s["max_raw"])
    s.update(extra)
    return s


def run_model(s, mode, sf, scale_factor=2.0, cos_limit=0.5, usable=None, full=False, sel=None):
    """The model on a scene (on its rows `sel`) in one mode -> what project_points returns (SIM3: view_cos all zero)"""
    a = {k: (s[k] if sel is None else s[k][sel]) for k in ("xyz", "normal", "min_inv", "max_inv", "max_raw")}
    if mode == SIM3:
        r = project_sim3(*s["chain"], s["cam"], a["xyz"], a["min_inv"], a["max_inv"], usable, sf, full=full)
        return r[:4] + (np.zeros(len(a["xyz"]), f32),) + r[4:]
    return project_points(mode, s["cam"], a["xyz"], a["normal"], a["min_inv"], a["max_inv"], a["max_raw"], usable, sf, scale_factor, cos_limit, full=full)


def run_evaluator(s, mode, sf, scale_factor=2.0, cos_limit=0.5):
    return evaluate(mode, s["cam"], s["xyz"], s["normal"], s["min_inv"], s["max_inv"], s["max_raw"], sf, scale_factor, cos_limit, chain=s["chain"])


# -- the exact scene --
# Pose of the plain modes: a signed permutation and an integer translation, so Ow = -R^T t is an integer vector and |P - Ow| = |Pc|.
# The Sim3 chains: own pose the same, then s_r = 2 x a signed permutation (direction 12) or 1/2 x its transpose (21) and integer t.
EXACT_R = f32([0, -1, 0, 0, 0, 1, -1, 0, 0])
EXACT_T = f32([1, -2, 3])
SIM_P = f32([0, 0, 1, 1, 0, 0, 0, 1, 0])
SIM3_12 = (f32(2) * SIM_P, f32([2, -4, 6]))
SIM3_21 = (f32(0.5) * SIM_P.reshape(3, 3).T.reshape(9), f32([2, -3, -1]))     # t21 = -sR21 t12


def _world_from_camera(R, t, Pc):
    """P with R P + t = Pc for a scaled signed permutation R (a power-of-two scale): exact for the dyadic values used here"""
    R = np.asarray(R, f64).reshape(3, 3)
    return (np.linalg.inv(R) @ (np.asarray(Pc, f64) - np.asarray(t, f64)).T).T


# One row = one camera-frame point.  Columns: tag, Pc, camera-frame normal, min_inv, max_inv (None: 1.2f x max_raw), max_raw,
# then what is walked to make the two neighbours (None: no neighbours; "x" / "y" / "z": the world coordinate that feeds that camera
# axis; "n": the normal's camera-z component; "raw": max_raw), the quantity that must move, the modes the neighbours are for,
# and the hand-derived verdicts "FKUBPS" (FRUSTUM, KF_RELOC, FUSE, PIXEL_BOUNDED, PIXEL, SIM3) of the row itself, of its neighbour
# with the smaller value of the quantity and of the one with the larger, and the row's level in the lower-bound modes on T8 (K, U, S)
# and in PredictScale with scale factor 2 (None where fp32 log decides: kernel == model there).
# Derivations: u = 256 X / Z + 320, v = 256 Y / Z + 240, dist = |Pc| (a Pythagorean quadruple), cos = n_z Z / dist.
#   slack rows use (2,1,2) -> u 576, v 368, dist 3;  (1,4,8) -> u 352, v 368, dist 9;  (0,3,4) -> u 320, v 432, dist 5;  (0,0,4) -> 320, 240, 4
#   default bounds: min_inv = 2, max_raw = 6 dist (PredictScale: log2 6 = 2.58 -> 3), max_inv = 1.2f x max_raw = 7.2 dist, normal (0,0,1)
_N1 = (0, 0, 1)
EXACT_ROWS = [
    # tag            Pc              normal        min  max_inv raw   walk  watch    modes                     on        below     above     lvlT8 lvlPS2
    ("slack3",       (2, 1, 2),      _N1,          2,   None,   18,   None, None,    (),                       "111111", None,     None,     2,    3),     # ratio 1.5 -> entry 2
    ("slack9",       (1, 4, 8),      _N1,          2,   None,   54,   None, None,    (),                       "111111", None,     None,     7,    3),     # ratio 4.5 -> 7
    # image bounds: u = 640 <=> X = 1.25 Z; u = 0 <=> X = -1.25 Z; v = 480 <=> Y = 0.9375 Z; v = 0 <=> Y = -0.9375 Z.  Closed in F, K, B;
    # half-open in U, S; none in P.  dist: (5,0,4) -> sqrt 41, (0,15,16) -> sqrt 481: min_inv 2 gives ratio 3.2 / 10.97 -> 6 / 7
    ("u_max",        (5, 0, 4),      _N1,          2,   None,   36,   "x",  "u",     (0, 1, 2, 3, 5),          "110110", "111111", "000010", 6,    None),
    ("u_min",        (-5, 0, 4),     _N1,          2,   None,   36,   "x",  "u",     (0, 1, 2, 3, 5),          "111111", "000010", "111111", 6,    None),
    ("v_max",        (0, 15, 16),    _N1,          2,   None,   128,  "y",  "v",     (0, 1, 2, 3, 5),          "110110", "111111", "000010", 7,    None),
    ("v_min",        (0, -15, 16),   _N1,          2,   None,   128,  "y",  "v",     (0, 1, 2, 3, 5),          "111111", "000010", "111111", 7,    None),
    # distance: closed [min_inv, max_inv] in F, U, S; none in K (B, P: not applicable).  (0,0,4): dist 4 = min_inv, ratio 1 -> entry 0
    ("dist_min",     (0, 0, 4),      _N1,          4,   None,   24,   "z",  "dist",  (0, 2, 5),                "111111", "010110", "111111", 0,    3),
    # (1,4,8): dist 9 = 1.2f x 7.5 = max_inv; PredictScale: 7.5 / 9 < 1 -> 0
    ("dist_max",     (1, 4, 8),      _N1,          2,   9,      7.5,  "z",  "dist",  (0, 2, 5),                "111111", "111111", "010110", 7,    0),
    # cosine: (2,1,2) with n_z = 0.75: dot = 1.5 = dist / 2, cos = 0.5 = the limit: passes both forms.  The frustum neighbour is the first
    # n_z whose fp32 quotient moves; Fuse compares in double, so its neighbours are one step of n_z away.
    ("cos_frustum",  (2, 1, 2),      (0, 0, 0.75), 2,   None,   18,   "n",  "vc",    (0,),                     "111111", "010111", "111111", 2,    3),
    ("cos_fuse",     (2, 1, 2),      (0, 0, 0.75), 2,   None,   18,   "n",  "dot",   (2,),                     "111111", "010111", "111111", 2,    3),
    # lower bound on T8 = 1, 1.25, 1.5, 2, 2.5, 3, 4, 5: ratio = dist / min_inv ON entry k -> k (sf[k] < ratio fails); above it -> k + 1
    ("ratio_1.25",   (0, 3, 4),      _N1,          4,   None,   30,   "z",  "ratio", (1, 2, 5),                "111111", "111111", "111111", 1,    3),
    ("ratio_1.5",    (2, 1, 2),      _N1,          2,   None,   18,   "z",  "ratio", (1, 2, 5),                "111111", "111111", "111111", 2,    3),
    ("ratio_2",      (0, 0, 4),      _N1,          2,   None,   24,   "z",  "ratio", (1, 2, 5),                "111111", "111111", "111111", 3,    3),
    ("ratio_2.5",    (0, 3, 4),      _N1,          2,   None,   30,   "z",  "ratio", (1, 2, 5),                "111111", "111111", "111111", 4,    3),
    ("ratio_3",      (2, 1, 2),      _N1,          1,   None,   18,   "z",  "ratio", (1, 2, 5),                "111111", "111111", "111111", 5,    3),
    ("ratio_4",      (0, 0, 4),      _N1,          1,   None,   24,   "z",  "ratio", (1, 2, 5),                "111111", "111111", "111111", 6,    3),
    ("ratio_5",      (0, 3, 4),      _N1,          1,   None,   30,   "z",  "ratio", (1, 2, 5),                "111111", "111111", "111111", 7,    3),
    ("ratio_below",  (2, 1, 2),      _N1,          4,   None,   18,   None, None,    (),                       "010110", None,     None,     0,    3),     # 0.75: dist < min_inv
    ("ratio_above",  (2, 1, 2),      _N1,          0.5, None,   18,   None, None,    (),                       "111111", None,     None,     7,    3),     # 6 -> 8 -> clamped
    # a point behind the camera inside the image: Z = -2, u = 64, v = 112; normal (0,0,-1) so the cosine passes where it is asked
    ("behind",       (2, 1, -2),     (0, 0, -1),   2,   None,   18,   None, None,    (),                       "010110", None,     None,     2,    3),
]
# PredictScale at ratio = 2^k, k = -1 .. nlevels + 1 = 9, on (2,1,2) (dist 3): max_raw = 3 x 2^k, max_inv left wide (k = -1 has no
# members: 1.2f x 1.5 < 3).  Real arithmetic: ceil(k) clamped to [0, 7].  With float32(1.2): max_raw = float32(3 x 1.2f^k).
PS_K = list(range(-1, 10))
PS_LEVEL_REAL = [0, 0, 1, 2, 3, 4, 5, 6, 7, 7, 7]
_CAMERA_AXIS = {"x": 0, "y": 1, "z": 2}
_WATCH_KEY = {"u": "u", "v": "v", "dist": "dist", "ratio": "ratio", "vc": "vc", "dot": "dot"}


def _exact_pose(mode):
    """-> cam, chain, the 3x3 matrix and translation that take a world point to the camera point of this mode"""
    R, t = EXACT_R.reshape(3, 3).astype(f64), EXACT_T.astype(f64)
    ow = -(R.T @ t)
    cam = Cam(EXACT_R, EXACT_T, ow)
    if mode < SIM3:
        return cam, None, R, t
    s_r, tt = SIM3_21 if mode == SIM3 else SIM3_12
    S = s_r.reshape(3, 3).astype(f64)
    return cam, (EXACT_R, EXACT_T, s_r, tt), S @ R, S @ t + tt.astype(f64)


def _row_arrays(cam_R, cam_t, rows):
    Pc = np.array([r[1] for r in rows], f64)
    xyz = _world_from_camera(cam_R, cam_t, Pc)
    nrm = (EXACT_R.reshape(3, 3).astype(f64).T @ np.array([r[2] for r in rows], f64).T).T     # world normal = Rcw^T n_c (the Sim3 chains read none)
    mn = f32([r[3] for r in rows])
    raw = f32([r[5] for r in rows])
    mx = np.array([f32(1.2) * f32(r[5]) if r[4] is None else f32(r[4]) for r in rows], f32)
    return xyz.astype(f32), nrm.astype(f32), mn, mx, raw


def exact_scene(mode, scale_factor=2.0):
    """The exact scene for one mode (SIM3 + 1 = 6 stands for the Sim3 chain of the other direction).  Rows: EXACT_ROWS, then for every row
    with a walk its two neighbours (below, above) in the modes they are for, then the PredictScale rows.  Extra keys: tag[], side[]
    (0 on the boundary / plain row, -1 / +1 neighbours), row[] (index into EXACT_ROWS, -1 for the PredictScale rows), ps_k[]."""
    cam, chain, A, b = _exact_pose(mode)
    m = min(mode, SIM3)
    xyz, nrm, mn, mx, raw = _row_arrays(A, b, EXACT_ROWS)
    assert (xyz.astype(f64) == _world_from_camera(A, b, np.array([r[1] for r in EXACT_ROWS], f64))).all()
    tags, side, rowi, psk = [r[0] for r in EXACT_ROWS], [0] * len(EXACT_ROWS), list(range(len(EXACT_ROWS))), [None] * len(EXACT_ROWS)
    X, N, MN, MX, RAW = [xyz], [nrm], [mn], [mx], [raw]
    probe = dict(cam=cam, chain=chain)

    def watched(i, x, nv, key):
        probe.update(xyz=x[None], normal=nv[None], min_inv=mn[i:i + 1], max_inv=mx[i:i + 1], max_raw=raw[i:i + 1])
        return run_model(probe, m, T8, scale_factor, full=True)[5][key][0]

    for i, r in enumerate(EXACT_ROWS):
        walk, watch, modes = r[6], r[7], r[8]
        if walk is None or m not in modes:
            continue
        if walk == "n":
            arr, j = nrm[i].copy(), int(np.argmax(np.abs(nrm[i])))
        else:
            arr, j = xyz[i].copy(), int(np.argmax(np.abs(A[_CAMERA_AXIS[walk]])))
        base = watched(i, xyz[i], nrm[i], _WATCH_KEY[watch])
        found = {}
        def moved(x_j):
            a = arr.copy()
            a[j] = x_j
            return watched(i, a if walk != "n" else xyz[i], a if walk == "n" else nrm[i], _WATCH_KEY[watch]), a

        for direction in (-1.0, 1.0):
            # the nearest value of the input, this side of it, at which the model's quantity differs: a step that moves it, then bisection
            lo, step = arr[j], f64(direction * 2.0 ** -30)
            hi = f32(f64(lo) + step)
            while hi == lo or moved(hi)[0] == base:
                step *= 2
                hi = f32(f64(lo) + step)
                assert abs(step) < 1e6, r[0]
            while True:
                mid = f32((f64(lo) + f64(hi)) / 2)
                if mid == lo or mid == hi:
                    break
                lo, hi = (lo, mid) if moved(mid)[0] != base else (mid, hi)
            val, a = moved(hi)
            found[-1 if val < base else 1] = a
        assert sorted(found) == [-1, 1], r[0]
        for sd in (-1, 1):
            X.append((found[sd] if walk != "n" else xyz[i])[None])
            N.append((found[sd] if walk == "n" else nrm[i])[None])
            MN.append(mn[i:i + 1]), MX.append(mx[i:i + 1]), RAW.append(raw[i:i + 1])
            tags.append(r[0]), side.append(sd), rowi.append(i), psk.append(None)
    # PredictScale rows
    base_row = [("ps", (2, 1, 2), _N1, 2, 1e6, 0)]
    bx, bn, bmn, bmx, _ = _row_arrays(A, b, base_row)
    for k in PS_K:
        r_ = f32(3.0 * 2.0 ** k) if float(scale_factor) == 2.0 else f32(f64(3.0) * f64(f32(scale_factor)) ** k)
        X.append(bx), N.append(bn), MN.append(bmn), RAW.append(f32([r_]))
        MX.append(f32([f32(1.2) * r_]) if k >= 0 else bmx)
        tags.append("ps_%d" % k), side.append(0), rowi.append(-1), psk.append(k)
    s = _scene(cam, chain, np.concatenate(X), np.concatenate(N), np.concatenate(MN), np.concatenate(MX), np.concatenate(RAW),
               tag=tags, side=np.array(side), row=np.array(rowi), ps_k=psk)
    return s


def expected_valid(s, mode):
    """The hand table's verdict for every row of an exact scene that has one (-1: none, a neighbour made for other modes)"""
    m = min(mode, SIM3)
    out = np.full(len(s["tag"]), -1)
    for i, (sd, ri) in enumerate(zip(s["side"], s["row"])):
        if ri < 0:
            out[i] = 1                                                # every PredictScale row is in view
            continue
        r = EXACT_ROWS[ri]
        out[i] = int(r[9 + (0 if sd == 0 else 1 if sd < 0 else 2)][m])
    return out


# -- the depth boundary (part of the exact scene; its pose is the identity with t = -0 so that Z can be -0 and the smallest subnormals) --
# P = (0,0,Z): X = Y = 0, u = 256 * 0 * (1 / Z) + 320.  Z = +-0: invz = +-inf, u = v = NaN: `Z < 0` does not reject either zero, the
# closed bounds do not reject NaN and IsInImage does; dist = 0 = min_inv passes, cos = 0 / 0 = NaN passes, ratio = 1 / 0 = +inf.
# Z = +-2^-149: invz = +-inf again (1 / 2^-149 overflows fp32), u = NaN; dist = 2^-149, cos = 1, ratio = +inf.
DEPTH_Z = f32([0.0, -0.0, -2.0 ** -149, 2.0 ** -149])
DEPTH_VALID = ["110110", "110110", "010110", "110110"]           # FKUBPS; on the boundary twice, then the two neighbours


def depth_scene(mode):
    cam = Cam(np.eye(3), f32([-0.0, -0.0, -0.0]), np.zeros(3))
    chain = None if mode < SIM3 else (np.eye(3, dtype=f32).reshape(9), f32([-0.0] * 3), np.eye(3, dtype=f32).reshape(9), f32([-0.0] * 3))
    xyz = np.stack([np.where(DEPTH_Z == 0, DEPTH_Z, f32(0)), np.where(DEPTH_Z == 0, DEPTH_Z, f32(0)), DEPTH_Z], 1)
    n = len(xyz)
    return _scene(cam, chain, xyz, np.tile(f32(_N1), (n, 1)), np.zeros(n, f32), np.full(n, f32(1.2), f32), np.ones(n, f32))


# -- the degenerate scene: finite inputs with non-finite intermediates, and non-finite coordinates --

def degenerate_scene(mode):
    """Identity rotation, t = (0, 0, 1) (Ow = (0, 0, -1)); camera point = P + (0, 0, 1).  Rows: tag -> P, min_inv, max_inv, max_raw"""
    big, fmax = f32(3e38), np.finfo(f32).max
    rows = [
        ("z0_x0",        (0, 0, -1),          0,    1.2,      1),      # P == Ow: Pc = 0, u = NaN, dist = 0, ratio = 1 / 0
        ("z0_x1",        (1, 0, -1),          0,    1.2,      1),      # Z = 0, X = 1: u = +inf
        ("z0_x-1",       (-1, -1, -1),        0,    1.2,      1),      # u = v = -inf
        ("ratio_inf",    (0, 0, -1 + 2.0 ** -20), 0, np.inf,  big),    # dist 2^-20, max_raw / dist overflows
        ("raw_0",        (0, 0, 3),           1,    0,        0),      # max_raw = 0: log 0 = -inf; max_inv = 0 rejects
        ("raw_0_wide",   (0, 0, 3),           1,    100,      0),      # the same with a wide max_inv: level from -inf
        ("raw_inf",      (0, 0, 3),           1,    np.inf,   np.inf),
        ("dist_inf",     (1e36, 1e36, fmax),  1,    np.inf,   big),    # |P - Ow| overflows fp32 while u and v stay in the image
        ("min_0",        (0, 0, 3),           0,    4.8,      4),      # ratio = dist / 0 = +inf in the lower-bound modes
        ("x_nan",        (np.nan, 0, 3),      1,    4.8,      4),
        ("z_nan",        (0, 0, np.nan),      1,    4.8,      4),
        ("x_inf",        (np.inf, 0, 3),      1,    4.8,      4),
        ("z_inf",        (0, 0, np.inf),      1,    np.inf,   np.inf),
        ("z_-inf",       (1, 1, -np.inf),     1,    np.inf,   np.inf),
        ("tiny",         (0, 0, -1 + 2.0 ** -23), 0, 1.2,     1),      # the closest point in front of the centre
        ("min_nan",      (0, 0, 3),           np.nan, 4.8,    4),
        ("ok",           (0, 0, 3),           1,    4.8,      4),
    ]
    cam = Cam(np.eye(3), f32([0, 0, 1]), f32([0, 0, -1]))
    I = np.eye(3, dtype=f32).reshape(9)
    chain = None if mode < SIM3 else (I, f32([0, 0, 1]), I, np.zeros(3, f32))
    n = len(rows)
    return _scene(cam, chain, [r[1] for r in rows], np.tile(f32(_N1), (n, 1)), [r[2] for r in rows], [r[3] for r in rows], [r[4] for r in rows],
                  tag=[r[0] for r in rows])


# -- the generic scene: the distribution of tests/test_gpu_parity.py::test_project_points --

def random_pose(rng):
    a = rng.normal(0, 0.15, 3)
    th = np.linalg.norm(a)
    k = a / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = (np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K).astype(f32)
    t = rng.normal(0, 0.5, 3).astype(f32)
    return R, t, (-(R.T.astype(f64) @ t.astype(f64))).astype(f32)


GENERIC_N = 4096
GENERIC_POSES = 2


def generic_scene(mode, pose, n=GENERIC_N):
    """mode SIM3 + 1 = the other direction of the Sim3 chain.  The members mfMinDistance / mfMaxDistance are drawn as in
    test_project_points; the bounds are 0.8f x / 1.2f x of them, so every point is linked."""
    rng = np.random.default_rng(1000 + 10 * mode + pose)
    R, t, ow = random_pose(rng)
    K = (458.654, 457.296, 367.215, 248.375, (0.0, 752.0, 0.0, 480.0))
    xyz = (rng.normal(0, 1, (n, 3)) * [4, 3, 4] + [0, 0, 6]).astype(f32)
    chain = None
    if mode >= SIM3:
        R12, t12, _ = random_pose(rng)
        s12 = f32(rng.uniform(0.5, 2.0))
        inv = f32(1.0 / f64(s12))
        sR12, sR21 = (R12 * s12).astype(f32), (R12.T * inv).astype(f32)
        t21 = np.array([f32(f64((sR21[i, 0] * t12[0] + sR21[i, 1] * t12[1]) + sR21[i, 2] * t12[2]) * -1.0) for i in range(3)], f32)
        s_r, tt = (sR21, t21) if mode == SIM3 else (sR12, t12)
        chain = (R.reshape(9), t, s_r.reshape(9), tt)
        cam = Cam(np.eye(3), np.zeros(3), np.zeros(3), *K)
        Pc = (s_r.astype(f64) @ (R.astype(f64) @ xyz.T.astype(f64) + t[:, None]) + tt[:, None]).T
        d = np.linalg.norm(Pc, axis=1)
    else:
        cam = Cam(R, t, np.full(3, np.nan) if mode == KF_RELOC else ow, *K)          # KF_RELOC must not read cam->ow
        d = np.linalg.norm(xyz - ow, axis=1)
    nrm = rng.normal(0, 1, (n, 3))
    nrm[: n // 2] = (xyz[: n // 2] - ow) + rng.normal(0, 1.0, (n // 2, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(f32)
    mf_min = (d * rng.uniform(0.3, 1.4, n)).astype(f32)
    mf_max = (mf_min * rng.uniform(1.5, 6.0, n)).astype(f32)
    s = _scene(cam, chain, xyz, nrm, f32(0.8) * mf_min, f32(1.2) * mf_max, mf_max)
    assert s["linked"].all()
    return s


def tiled(s, n):
    """The first n rows of the scene repeated as often as needed (launch shapes)"""
    idx = np.arange(n) % len(s["xyz"])
    out = dict(s)
    for k in ("xyz", "normal", "min_inv", "max_inv", "max_raw", "usable", "mf_min", "mf_max", "linked"):
        out[k] = np.ascontiguousarray(s[k][idx])
    return out


LAUNCH_SHAPES = (0, 1, 255, 256, 257, 65537)
ALL_MODES = (FRUSTUM, KF_RELOC, FUSE, PIXEL_BOUNDED, PIXEL, SIM3, SIM3 + 1)
MODE_IDS = ("frustum", "kf_reloc", "fuse", "pixel_bounded", "pixel", "sim3_21", "sim3_12")


def usable_mask(n, seed=5):
    """A mask that drops about a quarter of the points (and certainly the first, when there is one)"""
    u = (np.random.default_rng(seed).random(n) < 0.75).astype(np.uint8)
    u[:1] = 0
    return u
