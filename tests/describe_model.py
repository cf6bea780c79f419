"""numpy model of the extractor's last stage: IC_Angle (src/ORBextractor.cc:125-152) and computeOrbDescriptor (:156-195), float32 step by step in
the reference's operation order.  Planes are padded planes (16 pixels of border on every side); x, y are keypoint coordinates of the level.

Nothing here calls the oracle: the polynomial of cv::fastAtan2 and its octant folding, the sine / cosine (glibc's sinf / cosf algorithm, in
double like the original) and cvRound are all stated below.  tests/test_describe_model.py holds every function to the oracle."""
import numpy as np

PAD = 16
HALF_PATCH_SIZE = 15
F = np.float32


def umax_table():
    """ORBextractor::ORBextractor, :495-512: the half width of the circular patch per row |v|."""
    umax = np.zeros(HALF_PATCH_SIZE + 1, np.int64)
    vmax = int(np.floor(HALF_PATCH_SIZE * np.sqrt(2.0) / 2 + 1))
    vmin = int(np.ceil(HALF_PATCH_SIZE * np.sqrt(2.0) / 2))
    for v in range(vmax + 1):
        umax[v] = int(np.rint(np.sqrt(float(HALF_PATCH_SIZE * HALF_PATCH_SIZE - v * v))))
    v0 = 0
    for v in range(HALF_PATCH_SIZE, vmin - 1, -1):
        while umax[v0] == umax[v0 + 1]:
            v0 += 1
        umax[v] = v0
        v0 += 1
    return umax


UMAX = umax_table()
_V, _U = np.mgrid[-HALF_PATCH_SIZE:HALF_PATCH_SIZE + 1, -HALF_PATCH_SIZE:HALF_PATCH_SIZE + 1]
DISC = np.abs(_U) <= UMAX[np.abs(_V)]          # the pixels IC_Angle sums: row v, |u| <= umax[|v|]


def cv_round(v):
    """cvRound(float) on x86-64: cvtss2si, round half to even."""
    return np.rint(np.asarray(v, F)).astype(np.int64)


def fast_atan2(y, x):
    """cv::fastAtan2 (OpenCV 3.4 atan_f32), degrees.  Every operation rounds to float32."""
    y, x = np.asarray(y, F), np.asarray(x, F)
    k = F(180.0 / np.pi)
    p1, p3, p5, p7 = F(0.9997878412794807) * k, F(-0.3258083974640975) * k, F(0.1555786518463281) * k, F(-0.04432655554792128) * k
    eps = F(2.220446049250313e-16)
    ax, ay = np.abs(x), np.abs(y)
    steep = ~(ax >= ay)
    num, den = np.where(steep, ax, ay), np.where(steep, ay, ax)
    c = (num / (den + eps)).astype(F)
    c2 = c * c
    a = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c
    a = np.where(steep, F(90.0) - a, a)             # the octant next to the y axis
    a = np.where(x < 0, F(180.0) - a, a)            # left half plane
    a = np.where(y < 0, F(360.0) - a, a)            # lower half plane
    return a.astype(F)


def moments(plane, x, y):
    """(m01, m10) of the circular patch around (cvRound(x), cvRound(y)): exact integers."""
    cx, cy = int(cv_round(x)) + PAD, int(cv_round(y)) + PAD
    patch = plane[cy - HALF_PATCH_SIZE:cy + HALF_PATCH_SIZE + 1, cx - HALF_PATCH_SIZE:cx + HALF_PATCH_SIZE + 1].astype(np.int64)
    assert patch.shape == DISC.shape, "patch leaves the padded plane"
    patch = patch * DISC
    return int((patch * _V).sum()), int((patch * _U).sum())


def ic_angle(plane, x, y):
    m01, m10 = moments(plane, x, y)
    return F(fast_atan2(F(m01), F(m10)))


def ic_angles(plane, xs, ys):
    m = np.array([moments(plane, x, y) for x, y in zip(xs, ys)], np.int64).reshape(-1, 2)
    return fast_atan2(m[:, 0].astype(F), m[:, 1].astype(F))


def _abstop12(f):
    return (np.asarray(f, F).view(np.uint32) >> 20) & 0x7ff


def _poly(x, x2, neg, n):
    """glibc 2.28 sysdeps/ieee754/flt-32/s_sincosf.h, sinf_poly / the cosine branch: all in double, one rounding to float at the end."""
    s = -1.0 if neg else 1.0
    c0, c1, c2, c3, c4 = s * 1.0, s * float.fromhex("-0x1.ffffffd0c621cp-2"), s * float.fromhex("0x1.55553e1068f19p-5"), \
        s * float.fromhex("-0x1.6c087e89a359dp-10"), s * float.fromhex("0x1.99343027bf8c3p-16")
    s1, s2, s3 = float.fromhex("-0x1.555545995a603p-3"), float.fromhex("0x1.1107605230bc4p-7"), float.fromhex("-0x1.994eb3774cf24p-13")
    if (n & 1) == 0:
        x3 = x * x2
        t1 = s2 + x2 * s3
        x7 = x3 * x2
        return F((x + x3 * s1) + x7 * t1)
    x4 = x2 * x2
    t2 = c3 + x2 * c4
    t1 = c0 + x2 * c1
    x6 = x4 * x2
    return F((t1 + x4 * c2) + x6 * t2)


def sincosf(a):
    """(sinf(a), cosf(a)) of glibc >= 2.28 for 0 <= a < 120 (the extractor passes [0, 2 pi])."""
    a = F(a)
    x = float(a)
    if _abstop12(a) < _abstop12(F(float.fromhex("0x1.921FB6p-1"))):       # |a| < pi / 4
        if _abstop12(a) < _abstop12(F(2.0 ** -12)):
            return a, F(1.0)
        return _poly(x, x * x, False, 0), _poly(x, x * x, False, 1)
    r = x * float.fromhex("0x1.45F306DC9C883p+23")                          # 2 / pi * 2^24
    n = (int(r) + 0x800000) >> 24
    x = x - n * float.fromhex("0x1.921FB54442D18p0")
    sgn = -1.0 if (n & 3) in (1, 2) else 1.0
    neg = (n & 2) != 0
    return _poly(x * sgn, x * x, neg, n), _poly(x * sgn, x * x, neg, n ^ 1)


def sample_offsets(pattern, angle):
    """(row, column) offsets of the 512 steered sample points: cvRound(x b + y a), cvRound(x a - y b) with a = cos, b = sin of
    angle * factorPI (:160-168), each product and sum rounded to float32."""
    factor_pi = F(np.pi / 180.0)                                            # (float)(CV_PI / 180.f): a double quotient, rounded once
    b, a = sincosf(F(angle) * factor_pi)
    p = np.asarray(pattern, np.int32).reshape(512, 2).astype(F)
    px, py = p[:, 0], p[:, 1]
    return cv_round(px * b + py * a), cv_round(px * a - py * b)


def descriptor(blurred_plane, x, y, angle, pattern):
    """The 32 descriptor bytes: bit j of byte i = t0 < t1 of pattern pair 8 i + j."""
    cx, cy = int(cv_round(x)) + PAD, int(cv_round(y)) + PAD
    dr, dc = sample_offsets(pattern, angle)
    r, c = cy + dr, cx + dc
    assert r.min() >= 0 and c.min() >= 0 and r.max() < blurred_plane.shape[0] and c.max() < blurred_plane.shape[1], "sample leaves the padded plane"
    t = blurred_plane[r, c].astype(np.int32).reshape(256, 2)
    return np.packbits(t[:, 0] < t[:, 1], bitorder="little")


def describe(plane, blurred_plane, xs, ys, pattern):
    """Angles (float32) and descriptors (n, 32) of keypoints of one level: what k_describe computes from the two planes."""
    angles = ic_angles(plane, xs, ys) if len(xs) else np.zeros(0, F)
    desc = np.zeros((len(xs), 32), np.uint8)
    for i, (x, y, a) in enumerate(zip(xs, ys, angles)):
        desc[i] = descriptor(blurred_plane, x, y, a, pattern)
    return angles, desc
