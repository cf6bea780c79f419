"""Test model of the triangulation of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:1096-1180) and of the pair loop around it
(:1058-1199).  Test infrastructure only: the product (csrc/triangulate.hip) never imports it.

triangulate(..., precision="f32") restates :1106-1180 in numpy.float32 / float64 exactly as typed in the reference: every value is
float except where the reference's expression is double (cv::norm and cv::Mat::dot return double, `1.0 / z`, the comparisons against
0.9998 and 5.991 * sigma2); the 4 x 4 SVD is numpy's single-precision one (LAPACK sgesdd), a stand-in for OpenCV's fp32 Jacobi SVD --
this repository holds no OpenCV.  precision="f64" evaluates the same expressions in float64 throughout.  How OpenCV evaluates the
cv::Mat expressions is recalled [OCV-RECALL], as in csrc/triangulate.hip: 3x3 * 3x1 as an fp32 row sum, `a * row - row` in fp32,
`v / w` as a multiplication by the fp32 reciprocal of w.

Besides verdict and x3D every evaluated test reports its signed margin to its threshold (positive = passed), in the units of the
tolerance contract: the cosine absolute, the reprojection and scale-ratio tests relative to their threshold, the
depths relative to the scene depth.  A match is SENSITIVE when any margin either model evaluated is smaller in magnitude than the
contract's margin; a sensitive match may take either verdict.

chain() restates the loop: per pair the acceptance loop of SearchForTriangulation through the oracle with the has_mp1 of that moment,
the triangulation of the pair's matches, has_mp1 = 1 for the accepted ones.  Given the device's per-pair results it follows the device
on sensitive matches only.

make_scene() builds the test scenes (fixed seeds): one current key frame, n_pairs neighbours, points seen by all of them.
"""
import numpy as np

ACCEPTED, PARALLAX, W_ZERO, BEHIND_1, BEHIND_2, REPROJ_1, REPROJ_2, ZERO_DIST, SCALE = range(9)

# the contract's margins
MARGIN_COS = 2e-6        # absolute, on cosParallaxRays
MARGIN_REL = 1e-3        # relative, on the two reprojection tests and the two scale-ratio tests
MARGIN_DEPTH = 1e-3      # z1, z2 relative to the scene depth
SENSITIVE_CAP = 0.01     # at most this share of a scene's matches may be sensitive

# Largest relative deviation |x3D_f32 - x3D_f64| / |x3D_f64| of the float32 model from the float64 model over all matches of the committed
# scenes (SCENES and GRID_SCENES below; measured by tests/test_triangulation_model.py::test_float32_model_deviation_is_the_recorded_one,
# which fails when a scene changes it), and the kernel's bound: 4 x that (a Jacobi sweep and LAPACK's bidiagonalisation are different
# backward-stable methods at the same precision; neither is "the reference's").
X3D_F32_MODEL_DEVIATION = 4.44e-6   # measured: 4.43e-6 (match-list scene seed 251: 1000 matches, 0.5 px noise, 2 degrees of parallax)
X3D_BOUND = 4.0 * X3D_F32_MODEL_DEVIATION

KP = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])


class Camera:
    """Pose, intrinsics and level tables of a key frame.  Ow = -Rwc * tcw as KeyFrame::SetPose forms it: an fp32 row sum, negated."""

    def __init__(self, R, t, fx=458.0, fy=457.0, cx=367.0, cy=248.0, scale_factor=1.2, nlevels=8):
        self.rcw = np.asarray(R, np.float64).astype(np.float32).reshape(3, 3)
        self.tcw = np.asarray(t, np.float64).astype(np.float32).reshape(3)
        rwc = self.rcw.T
        self.ow = np.array([-np.float32(np.float32(np.float32(rwc[i, 0] * self.tcw[0]) + np.float32(rwc[i, 1] * self.tcw[1])) +
                                        np.float32(rwc[i, 2] * self.tcw[2])) for i in range(3)], np.float32)
        self.fx, self.fy, self.cx, self.cy = (np.float32(v) for v in (fx, fy, cx, cy))
        self.sf = np.array([np.float32(scale_factor) ** l for l in range(nlevels)], np.float32)
        for l in range(1, nlevels):                        # mvScaleFactor[i] = mvScaleFactor[i-1] * scaleFactor (fp32)
            self.sf[l] = np.float32(self.sf[l - 1] * np.float32(scale_factor))
        self.sigma2 = (self.sf * self.sf).astype(np.float32)
        self.scale_factor = np.float32(scale_factor)

    def project(self, X):
        """float64 pixel coordinates and depth of world points X[n][3]"""
        Xc = np.asarray(X, np.float64) @ self.rcw.astype(np.float64).T + self.tcw.astype(np.float64)
        z = Xc[:, 2]
        return np.float64(self.fx) * Xc[:, 0] / z + np.float64(self.cx), np.float64(self.fy) * Xc[:, 1] / z + np.float64(self.cy), z


def ratio_factor(cam1):
    return np.float32(np.float32(1.5) * cam1.scale_factor)        # :1055


def compute_f12(cam1, cam2):
    """LocalMapping::ComputeF12 (src/LocalMapping.cc:1277-1294): K1^-T [t12]x R12 K2^-1, in float64, rounded to float32 at the end."""
    R1, R2 = cam1.rcw.astype(np.float64), cam2.rcw.astype(np.float64)
    t1, t2 = cam1.tcw.astype(np.float64), cam2.tcw.astype(np.float64)
    R12 = R1 @ R2.T
    t12 = -R12 @ t2 + t1
    tx = np.array([[0, -t12[2], t12[1]], [t12[2], 0, -t12[0]], [-t12[1], t12[0], 0]])
    K = lambda c: np.array([[c.fx, 0, c.cx], [0, c.fy, c.cy], [0, 0, 1]], np.float64)
    return (np.linalg.inv(K(cam1)).T @ tx @ R12 @ np.linalg.inv(K(cam2))).astype(np.float32)


def _one(C1, C2, rf, k1x, k1y, o1, k2x, k2y, o2, f64, depth):
    """:1106-1180 for one match -> (verdict, x3D, {test: margin})"""
    F = np.float64 if f64 else np.float32
    D = np.float64
    R1, R2, t1, t2 = C1.rcw.astype(F), C2.rcw.astype(F), C1.tcw.astype(F), C2.tcw.astype(F)
    k1x, k1y, k2x, k2y, rf = F(k1x), F(k1y), F(k2x), F(k2y), F(rf)
    fx1, fy1, cx1, cy1, fx2, fy2, cx2, cy2 = (F(v) for v in (C1.fx, C1.fy, C1.cx, C1.cy, C2.fx, C2.fy, C2.cx, C2.cy))
    margins = {}
    x3d = np.zeros(3, F)
    invfx1, invfy1, invfx2, invfy2 = F(1) / fx1, F(1) / fy1, F(1) / fx2, F(1) / fy2
    xn1 = [F((k1x - cx1) * invfx1), F((k1y - cy1) * invfy1), F(1)]
    xn2 = [F((k2x - cx2) * invfx2), F((k2y - cy2) * invfy2), F(1)]
    row = lambda a, b, c, p: F(F(F(a * p[0]) + F(b * p[1])) + F(c * p[2]))
    ray1 = [row(R1[0, i], R1[1, i], R1[2, i], xn1) for i in range(3)]        # Rwc1 * xn1
    ray2 = [row(R2[0, i], R2[1, i], R2[2, i], xn2) for i in range(3)]
    ddot = lambda a, b: D(a[0]) * D(b[0]) + D(a[1]) * D(b[1]) + D(a[2]) * D(b[2])
    cosp = F(ddot(ray1, ray2) / (np.sqrt(ddot(ray1, ray1)) * np.sqrt(ddot(ray2, ray2))))
    margins["cos"] = min(D(cosp), 0.9998 - D(cosp))
    if cosp < 0 or D(cosp) > 0.9998:
        return PARALLAX, x3d, margins
    T1, T2 = np.concatenate([R1, t1[:, None]], 1), np.concatenate([R2, t2[:, None]], 1)
    A = np.stack([F(xn1[0]) * T1[2] - T1[0], F(xn1[1]) * T1[2] - T1[1], F(xn2[0]) * T2[2] - T2[0], F(xn2[1]) * T2[2] - T2[1]]).astype(F)
    v = np.linalg.svd(A)[2][3].astype(F)
    if v[3] == 0:
        return W_ZERO, x3d, margins
    rinv = F(D(1.0) / D(v[3]))
    x3d = (v[:3] * rinv).astype(F)
    z1 = F(ddot(R1[2], x3d) + D(t1[2]))
    margins["z1"] = D(z1) / depth
    if z1 <= 0:
        return BEHIND_1, x3d, margins
    z2 = F(ddot(R2[2], x3d) + D(t2[2]))
    margins["z2"] = D(z2) / depth
    if z2 <= 0:
        return BEHIND_2, x3d, margins
    for name, code, R, t, z, fx, fy, cx, cy, kx, ky, s2 in (("reproj1", REPROJ_1, R1, t1, z1, fx1, fy1, cx1, cy1, k1x, k1y, C1.sigma2[o1]),
                                                           ("reproj2", REPROJ_2, R2, t2, z2, fx2, fy2, cx2, cy2, k2x, k2y, C2.sigma2[o2])):
        x = F(ddot(R[0], x3d) + D(t[0]))
        y = F(ddot(R[1], x3d) + D(t[1]))
        invz = F(D(1.0) / D(z))
        u, w = F(F(F(fx * x) * invz) + cx), F(F(F(fy * y) * invz) + cy)
        ex, ey = F(u - kx), F(w - ky)
        e2, lim = D(F(F(ex * ex) + F(ey * ey))), 5.991 * D(F(s2))
        margins[name] = (lim - e2) / lim
        if e2 > lim:
            return code, x3d, margins
    n1, n2 = (x3d - C1.ow.astype(F)).astype(F), (x3d - C2.ow.astype(F)).astype(F)
    dist1, dist2 = F(np.sqrt(ddot(n1, n1))), F(np.sqrt(ddot(n2, n2)))
    if dist1 == 0 or dist2 == 0:
        return ZERO_DIST, x3d, margins
    ratioDist = F(dist1 / dist2)
    ratioOctave = F(F(C1.sf[o1]) / F(C2.sf[o2]))
    lo, hi = F(ratioDist * rf), F(ratioOctave * rf)
    margins["scale_lo"] = (D(lo) - D(ratioOctave)) / D(ratioOctave)
    margins["scale_hi"] = (D(hi) - D(ratioDist)) / D(hi)
    if lo < ratioOctave or ratioDist > hi:
        return SCALE, x3d, margins
    return ACCEPTED, x3d, margins


_LIMIT = {"cos": MARGIN_COS, "z1": MARGIN_DEPTH, "z2": MARGIN_DEPTH, "reproj1": MARGIN_REL, "reproj2": MARGIN_REL, "scale_lo": MARGIN_REL,
          "scale_hi": MARGIN_REL}


def triangulate(cam1, cam2, rf, kp1, kp2, precision="f32", depth=1.0):
    """-> verdict[n] int32, x3d[n][3] (float32 or float64), margins: list of {test: signed margin}"""
    n = len(kp1)
    f64 = precision == "f64"
    verdict, x3d, margins = np.zeros(n, np.int32), np.zeros((n, 3), np.float64 if f64 else np.float32), []
    with np.errstate(all="ignore"):
        for j in range(n):
            v, x, mg = _one(cam1, cam2, rf, kp1["x"][j], kp1["y"][j], int(kp1["octave"][j]), kp2["x"][j], kp2["y"][j], int(kp2["octave"][j]), f64,
                            float(depth))
            verdict[j], x3d[j] = v, x
            margins.append(mg)
    return verdict, x3d, margins


def sensitive(margins):
    """bool[n]: any evaluated margin inside the contract's margin (NaN counts as inside)"""
    return np.array([any(not (abs(m) >= _LIMIT[k]) for k, m in mg.items()) for mg in margins], bool).reshape(len(margins))


def both(cam1, cam2, rf, kp1, kp2, depth):
    """the two models on one match list -> dict(v32, x32, v64, x64, sensitive)"""
    v32, x32, m32 = triangulate(cam1, cam2, rf, kp1, kp2, "f32", depth)
    v64, x64, m64 = triangulate(cam1, cam2, rf, kp1, kp2, "f64", depth)
    return dict(v32=v32, x32=x32, v64=v64, x64=x64, sensitive=sensitive(m32) | sensitive(m64))


def rel_dev(x, x64):
    """|x - x64| / |x64| per row (0 where both are zero)"""
    d = np.linalg.norm(np.asarray(x, np.float64) - x64, axis=1)
    n = np.linalg.norm(x64, axis=1)
    return np.where(n > 0, d / np.where(n > 0, n, 1), d)


# ---- scenes ----------------------------------------------------------------------------------------------------------------------
def _rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    return (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @
            np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]))


def bow_groups(node_of):
    """{node id: [feature indices in insertion order]} -- a stand-in DBoW2::FeatureVector"""
    g = {}
    for i, nd in enumerate(node_of):
        g.setdefault(int(nd) * 7 + 3, []).append(int(i))
    return g


def make_scene(seed, n_pairs, n_points=500, noise=0.5, parallax_deg=(2.0, 10.0), n_nodes=40, clutter=80, has1_share=0.25, empty_pair=None,
               W=752, H=480):
    """One current key frame, n_pairs neighbours on a baseline that gives the stated parallax at the scene depth, n_points world points
    seen by key frame 1 and (about 80 % each) by every neighbour, `noise` px of Gaussian noise on every observation, descriptors that
    differ by a few bits between views, clutter key points, and a vocabulary node per world point."""
    rng = np.random.default_rng(seed)
    depth = 8.0
    cam1 = Camera(_rot(*rng.normal(0, 0.02, 3)), rng.normal(0, 0.05, 3))
    # world points: sample pixels + depth in camera 1
    u, v, z = rng.uniform(20, W - 20, n_points), rng.uniform(20, H - 20, n_points), rng.uniform(0.5 * depth, 1.5 * depth, n_points)
    Xc = np.stack([(u - cam1.cx) / cam1.fx * z, (v - cam1.cy) / cam1.fy * z, z], 1)
    Xw = (Xc - cam1.tcw.astype(np.float64)) @ cam1.rcw.astype(np.float64)
    base_desc = rng.integers(0, 256, (n_points, 32), dtype=np.uint8)
    node = rng.integers(0, n_nodes, n_points)
    oct1 = rng.integers(0, 4, n_points)

    def observe(cam, idx, octv, angle0):
        pu, pv, pz = cam.project(Xw[idx])
        kp = np.zeros(len(idx), KP)
        kp["x"], kp["y"] = pu + rng.normal(0, noise, len(idx)), pv + rng.normal(0, noise, len(idx))
        kp["octave"], kp["size"] = octv, 31.0
        kp["angle"] = (angle0 + rng.normal(0, 3.0, len(idx))) % 360.0
        flips = rng.random((len(idx), 256)) < rng.uniform(0.0, 0.05, (len(idx), 1))
        desc = base_desc[idx] ^ np.packbits(flips, axis=1)
        return kp, desc

    def add_clutter(kp, desc, nd, m):
        ck = np.zeros(m, KP)
        ck["x"], ck["y"], ck["octave"], ck["size"] = rng.uniform(0, W, m), rng.uniform(0, H, m), rng.integers(0, 8, m), 31.0
        ck["angle"] = rng.uniform(0, 360, m)
        return np.concatenate([kp, ck]), np.concatenate([desc, rng.integers(0, 256, (m, 32), dtype=np.uint8)]), np.concatenate([nd, rng.integers(0, n_nodes, m)])

    ang1 = rng.uniform(0, 360, n_points)
    kp1, de1 = observe(cam1, np.arange(n_points), oct1, ang1)
    kp1, de1, node1 = add_clutter(kp1, de1, node, clutter)
    perm = rng.permutation(len(kp1))
    kp1, de1, node1 = kp1[perm], de1[perm], node1[perm]
    pairs, cams2 = [], []
    for k in range(n_pairs):
        par = np.deg2rad(rng.uniform(*parallax_deg))
        direction = rng.normal(0, 1, 3) * np.array([1.0, 1.0, 0.15])
        centre = direction / np.linalg.norm(direction) * depth * np.tan(par)
        R2 = _rot(*rng.normal(0, 0.03, 3)) @ cam1.rcw.astype(np.float64)
        cam2 = Camera(R2, -R2 @ (centre - cam1.rcw.astype(np.float64).T @ cam1.tcw.astype(np.float64)))
        pu, pv, pz = cam2.project(Xw)
        vis = np.nonzero((pu > 5) & (pu < W - 5) & (pv > 5) & (pv < H - 5) & (pz > 0.1) & (rng.random(n_points) < 0.8))[0]
        # mostly the same octave as in key frame 1, sometimes far off (breaks the scale ratio)
        oct2 = np.where(rng.random(len(vis)) < 0.9, np.clip(oct1[vis] + rng.integers(-1, 2, len(vis)), 0, 7), rng.integers(0, 8, len(vis)))
        kp2, de2 = observe(cam2, vis, oct2, ang1[vis] + rng.uniform(0, 360))
        kp2, de2, node2 = add_clutter(kp2, de2, node[vis], clutter)
        perm2 = rng.permutation(len(kp2))
        kp2, de2, node2 = kp2[perm2], de2[perm2], node2[perm2]
        if empty_pair is not None and k == empty_pair:
            kp2, de2, node2 = kp2[:0], de2[:0], node2[:0]
        has2 = (rng.random(len(kp2)) < 0.2).astype(np.uint8)
        pairs.append(dict(groups=bow_groups(node2), kp=kp2, desc=de2, has_mp=has2, F12=compute_f12(cam1, cam2), sigma2=cam2.sigma2))
        cams2.append(cam2)
    has1 = (rng.random(len(kp1)) < has1_share).astype(np.uint8)
    return dict(cam1=cam1, cams2=cams2, kp1=kp1, desc1=de1, groups1=bow_groups(node1), has_mp1=has1, pairs=pairs, depth=depth,
                ratio_factor=ratio_factor(cam1))


# the committed chain scenes: name -> make_scene arguments
SCENES = {
    "one_pair": dict(seed=101, n_pairs=1),
    "two_pairs": dict(seed=102, n_pairs=2),
    "twenty_pairs": dict(seed=103, n_pairs=20),
    "twenty_pairs_b": dict(seed=104, n_pairs=20, noise=1.0, parallax_deg=(0.5, 10.0), empty_pair=7),
    "twenty_pairs_c": dict(seed=105, n_pairs=20, noise=0.3, has1_share=0.5),
}
# the one whose 20-pair chain must hold no sensitive match at all
SCENE_WITHOUT_SENSITIVE = "twenty_pairs"


def match_list_scene(seed, n, noise=0.5, parallax_deg=5.0, wrong_share=0.15):
    """A caller-given match list for uvo_triangulate_matches: n matches between two key frames, most of them true correspondences with
    `noise` px of noise, some deliberately wrong (another point's observation; a far-off octave; the same ray twice) so that every
    rejection reason that finite data can reach occurs."""
    rng = np.random.default_rng(seed)
    depth = 8.0
    cam1 = Camera(_rot(*rng.normal(0, 0.02, 3)), rng.normal(0, 0.05, 3))
    centre = np.array([1.0, 0.2, 0.05]) / np.linalg.norm([1.0, 0.2, 0.05]) * depth * np.tan(np.deg2rad(parallax_deg))
    R2 = _rot(*rng.normal(0, 0.03, 3)) @ cam1.rcw.astype(np.float64)
    cam2 = Camera(R2, -R2 @ (centre - cam1.rcw.astype(np.float64).T @ cam1.tcw.astype(np.float64)))
    u, v, z = rng.uniform(20, 732, n), rng.uniform(20, 460, n), rng.uniform(0.5 * depth, 1.5 * depth, n)
    Xc = np.stack([(u - cam1.cx) / cam1.fx * z, (v - cam1.cy) / cam1.fy * z, z], 1)
    Xw = (Xc - cam1.tcw.astype(np.float64)) @ cam1.rcw.astype(np.float64)
    kp1, kp2 = np.zeros(n, KP), np.zeros(n, KP)
    pu, pv, _ = cam1.project(Xw)
    kp1["x"], kp1["y"] = pu + rng.normal(0, noise, n), pv + rng.normal(0, noise, n)
    pu, pv, _ = cam2.project(Xw)
    kp2["x"], kp2["y"] = pu + rng.normal(0, noise, n), pv + rng.normal(0, noise, n)
    kp1["octave"] = rng.integers(0, 4, n)
    kp2["octave"] = np.clip(kp1["octave"] + rng.integers(-1, 2, n), 0, 7)
    kind = rng.random(n)
    w = wrong_share / 3
    for j in np.nonzero(kind < w)[0]:                      # another point's observation: behind a camera, or off the pixel
        kp2["x"][j], kp2["y"][j] = rng.uniform(0, 752), rng.uniform(0, 480)
    for j in np.nonzero((kind >= w) & (kind < 2 * w))[0]:  # far-off octave
        kp1["octave"][j], kp2["octave"][j] = (0, 7) if rng.random() < 0.5 else (7, 0)
    for j in np.nonzero((kind >= 2 * w) & (kind < 3 * w))[0]:  # (almost) the same ray: no parallax
        ray = (np.array([(kp1["x"][j] - cam1.cx) / cam1.fx, (kp1["y"][j] - cam1.cy) / cam1.fy, 1.0]) @ cam1.rcw.astype(np.float64))
        rc2 = cam2.rcw.astype(np.float64) @ ray
        kp2["x"][j], kp2["y"][j] = cam2.fx * rc2[0] / rc2[2] + cam2.cx, cam2.fy * rc2[1] / rc2[2] + cam2.cy
    return dict(cam1=cam1, cam2=cam2, kp1=kp1, kp2=kp2, depth=depth, ratio_factor=ratio_factor(cam1), Xw=Xw)


def pile_scene(n_a=1030, n_b=120, k=60, extra2=0):
    """The pile of tests/resolve_model.py as a CreateNewMapPoints scene: two vocabulary nodes, each one all-to-all group.  Node 3 holds
    features 0..n_a-1 of key frame 1 and key points 0..k-1 of key frame 2, node 10 the n_b features behind them and key points k..2k-1.
    Every feature of key frame 1 has the zero descriptor, key point j of a node its first j bits set: distance j from every feature.
    The cameras differ by a sideways translation and every key point lies on the row y = cy, so CheckDistEpipolarLine passes for every
    pair and the acceptance loop of SearchForTriangulation is left to its order alone: the i-th free feature of a node ends on the
    node's key point i while i <= TH_LOW.  Key point j of a node is the true observation of the world point of the node's feature j, so
    the first pair's matches triangulate; two pairs, the second one sees the map points the first one made.  extra2 key points of a node
    that key frame 1 does not have stand in FRONT of key frame 2's others: never candidates, they only make the frame large."""
    import resolve_model as rm
    I = np.eye(3)
    cam1, cams2 = Camera(I, [0, 0, 0]), [Camera(I, [-1.0, 0, 0]), Camera(I, [-0.7, 0, 0])]
    n1 = n_a + n_b
    u = 40.0 + (np.arange(n1) * 37 % 660).astype(np.float64)
    z = 4.0 + (np.arange(n1) * 13 % 80) / 10.0
    Xw = np.stack([(u - float(cam1.cx)) / float(cam1.fx) * z, np.zeros(n1), z], 1)
    kp1 = np.zeros(n1, KP)
    kp1["x"], kp1["y"], kp1["size"] = u, float(cam1.cy), 31.0
    desc1, pile_t = rm.pile_descriptors(n1, k)
    seen = np.r_[np.arange(k), n_a + np.arange(k)]                       # the features whose world points key frame 2 observes
    pairs = []
    for cam2 in cams2:
        pu, _, _ = cam2.project(Xw[seen])
        kp2 = np.zeros(extra2 + 2 * k, KP)
        kp2["x"], kp2["y"], kp2["size"] = np.r_[np.arange(extra2) % 700, pu], float(cam2.cy), 31.0
        groups = {3: list(range(extra2, extra2 + k)), 10: list(range(extra2 + k, extra2 + 2 * k))}
        if extra2:
            groups[99] = list(range(extra2))
        pairs.append(dict(groups=groups, kp=kp2, desc=np.concatenate([np.zeros((extra2, 32), np.uint8), pile_t, pile_t]),
                          has_mp=np.zeros(extra2 + 2 * k, np.uint8), F12=compute_f12(cam1, cam2), sigma2=cam2.sigma2))
    return dict(cam1=cam1, cams2=cams2, kp1=kp1, desc1=desc1, groups1={3: list(range(n_a)), 10: list(range(n_a, n1))},
                has_mp1=np.zeros(n1, np.uint8), pairs=pairs, depth=8.0, ratio_factor=ratio_factor(cam1))


# the committed match-list scenes of the GPU grid: (seed, n, noise px, parallax degrees)
GRID_SCENES = [(200 + 10 * i + j, n, noise, par) for i, n in enumerate((0, 1, 63, 64, 65, 1000))
               for j, (noise, par) in enumerate(((0.0, 5.0), (0.5, 2.0), (1.5, 10.0)))]


def hand_cases():
    """Hand-built matches, one per `continue` of the loop body that finite data can reach: [(name, expected verdict, cam1, cam2, kp1, kp2)].
    Camera 1 at the origin looking along +z; camera 2 one unit to its right (epipolar lines horizontal) unless stated."""
    I = np.eye(3)
    cam1, cam2 = Camera(I, [0, 0, 0]), Camera(I, [-1.0, 0, 0])

    def kps(cam_a, cam_b, X, oct1=0, oct2=0, d1=(0, 0), d2=(0, 0)):
        a, b = np.zeros(1, KP), np.zeros(1, KP)
        (u, v, _), (u2, v2, _) = cam_a.project(np.array([X])), cam_b.project(np.array([X]))
        a["x"], a["y"], a["octave"] = u[0] + d1[0], v[0] + d1[1], oct1
        b["x"], b["y"], b["octave"] = u2[0] + d2[0], v2[0] + d2[1], oct2
        return a, b

    def from_dirs(cam_a, cam_b, da, db):
        a, b = np.zeros(1, KP), np.zeros(1, KP)
        a["x"], a["y"] = cam_a.fx * da[0] / da[2] + cam_a.cx, cam_a.fy * da[1] / da[2] + cam_a.cy
        b["x"], b["y"] = cam_b.fx * db[0] / db[2] + cam_b.cx, cam_b.fy * db[1] / db[2] + cam_b.cy
        return a, b

    X = [0.3, -0.2, 6.0]
    ahead = Camera(I, [-0.5, 0, -10.0])                      # camera 2 in front of the point, looking away from it
    return [
        ("noise-free", ACCEPTED, cam1, cam2) + kps(cam1, cam2, X),
        ("zero parallax", PARALLAX, cam1, cam2) + from_dirs(cam1, cam2, (0.1, 0.05, 1.0), (0.1, 0.05, 1.0)),
        ("behind camera 1", BEHIND_1, cam1, cam2) + from_dirs(cam1, cam2, (-0.2, 0.0, 1.0), (0.2, 0.0, 1.0)),     # the rays diverge
        ("behind camera 2", BEHIND_2, cam1, ahead) + kps(cam1, ahead, [0.0, 0.0, 5.0]),
        ("outlier in key frame 1 only", REPROJ_1, cam1, cam2) + kps(cam1, cam2, X, oct1=0, oct2=7, d1=(0, 6.0)),   # 3 px each: 9 > 5.991 but < 5.991 * 12.8
        ("outlier in key frame 2 only", REPROJ_2, cam1, cam2) + kps(cam1, cam2, X, oct1=7, oct2=0, d2=(0, 6.0)),
        ("octaves break the scale ratio", SCALE, cam1, cam2) + kps(cam1, cam2, X, oct1=0, oct2=7),
        ("octaves break the scale ratio, other side", SCALE, cam1, cam2) + kps(cam1, cam2, X, oct1=7, oct2=0),
    ]


# ---- the chain -------------------------------------------------------------------------------------------------------------------
def chain(oracle, scene, check_orientation, device=None):
    """The loop of :1058-1199 on a scene.  device: the per-pair results of uvo_create_new_map_points (list of dicts with idx1, idx2,
    verdict); when given, the match lists are compared pair by pair (AssertionError) and the model takes the device's verdict on
    sensitive matches.  -> list of per-pair dicts (idx1, idx2, verdict = the verdicts the chain went on with, v32, v64, x32, x64,
    sensitive), and has_mp1 at the end."""
    has1 = scene["has_mp1"].copy()
    out = []
    for p, P in enumerate(scene["pairs"]):
        if len(P["kp"]):
            match, _ = oracle.search_for_triangulation(scene["groups1"], scene["kp1"], scene["desc1"], has1, P["groups"], P["kp"], P["desc"],
                                                       P["has_mp"], P["F12"], P["sigma2"], check_orientation)
        else:
            match = np.full(len(has1), -1, np.int32)
        idx1 = np.nonzero(match >= 0)[0].astype(np.int32)
        idx2 = match[idx1].astype(np.int32)
        r = both(scene["cam1"], scene["cams2"][p], scene["ratio_factor"], scene["kp1"][idx1], P["kp"][idx2], scene["depth"])
        verdict = r["v32"].copy()
        if device is not None:
            np.testing.assert_array_equal(device[p]["idx1"], idx1, err_msg="pair %d: idx1 of the match list" % p)
            np.testing.assert_array_equal(device[p]["idx2"], idx2, err_msg="pair %d: idx2 of the match list" % p)
            verdict[r["sensitive"]] = device[p]["verdict"][r["sensitive"]]
        has1[idx1[verdict == ACCEPTED]] = 1
        r.update(idx1=idx1, idx2=idx2, verdict=verdict)
        out.append(r)
    return out, has1


def write_scene_file(path, scene, check_orientation):
    """The scene as tests/cpp/compat_newpoints.cpp reads it (layout: see that file's header)."""
    def node_of(groups, n):
        node = np.zeros(n, np.int32)
        for nd, feats in groups.items():
            node[feats] = nd
        return node

    with open(path, "wb") as f:
        f.write(np.array([1 if check_orientation else 0, 1 + len(scene["pairs"])], np.int32).tobytes())
        kfs = [(scene["cam1"], scene["kp1"], scene["desc1"], scene["has_mp1"], scene["groups1"], np.zeros(9, np.float32))]
        kfs += [(c, P["kp"], P["desc"], P["has_mp"], P["groups"], P["F12"]) for c, P in zip(scene["cams2"], scene["pairs"])]
        for cam, kp, desc, has, groups, F12 in kfs:
            f.write(np.array([len(kp), len(cam.sf)], np.int32).tobytes())
            f.write(np.concatenate([cam.rcw.reshape(9), cam.tcw, cam.ow, [cam.fx, cam.fy, cam.cx, cam.cy]]).astype(np.float32).tobytes())
            f.write(cam.sf.astype(np.float32).tobytes() + cam.sigma2.astype(np.float32).tobytes())
            f.write(np.ascontiguousarray(kp, KP).tobytes() + np.ascontiguousarray(desc, np.uint8).tobytes())
            f.write(np.ascontiguousarray(has, np.uint8).tobytes() + node_of(groups, len(kp)).tobytes())
            f.write(np.asarray(F12, np.float32).reshape(9).tobytes())


def read_new_points_file(path, n_pairs):
    """-> [one call, host loop], each a list over pairs of (idx1[n], idx2[n], x3d[n][3])"""
    raw = open(path, "rb").read()
    rec = np.dtype([("idx1", "<i4"), ("idx2", "<i4"), ("x3d", "<f4", 3)])
    off, out = 0, []
    for _ in range(2):
        per = []
        for _ in range(n_pairs):
            n = int(np.frombuffer(raw, np.int32, 1, off)[0])
            a = np.frombuffer(raw, rec, n, off + 4)
            off += 4 + n * rec.itemsize
            per.append((a["idx1"].copy(), a["idx2"].copy(), a["x3d"].copy()))
        out.append(per)
    assert off == len(raw)
    return out
