"""The C++ compat adaptors (include/uvo/compat/) held to the oracle on non-degenerate scenes.

tests/cpp/compat_scenes.cpp runs a list of adaptor calls on behavioural stand-ins of the reference's Frame / KeyFrame / MapPoint and
dumps every result and the map after each mutating call.  The expected values are computed here from the same scene, straight through
the oracle primitives in the reference's order (src/ORBmatcher.cc, src/LocalMapping.cc), with the map mutation restated on
tests/compat_model.py.  Poses are not the identity, key frames have their own intrinsics and negative bounds, frames carry distorted
key points next to the undistorted ones, and points are bad, slots NULL, sets already found and observations outliers -- so a slip in
the adaptors' marshalling or write-back changes a compared value.  Coverage counters keep the scenes from turning degenerate."""
import os
import struct
import subprocess

import numpy as np
import pytest

import compat_model as cm
import host_build
import oracle_lib

TAKEN = 0x7FFFFFFF
W, H = 752, 480
INTR_A = (458.654, 457.296, 367.215, 248.375)                  # Data/Settings_VIORB.yaml
INTR_B = (466.10, 451.80, 373.60, 244.40)                      # a second camera: SearchBySim3 projects with pKF1's (:1270-1273)
DIST = (-0.28340811, 0.07395907)

(OP_MATCHER, OP_SBP_LOCAL, OP_SBP_KF, OP_BOW_KF_FRAME, OP_BOW_KF_KF, OP_TRIANG, OP_FUSE, OP_TRI_BEGIN, OP_TRI_NEXT, OP_FUSE_TARGETS,
 OP_SBP_SCW, OP_FUSE_SCW, OP_SIM3, OP_WINDOW, OP_SBP_FRAMES, OP_INIT, OP_SBP_LAST, OP_EXTRACTOR, OP_EXTRACT, OP_GRIDER) = range(20)


def build_scenes_driver():
    return host_build.build("compat_scenes")


def test_scene_driver_compiles_warning_free():
    """-std=c++11 -Wall -Werror, without a GPU"""
    assert os.path.exists(build_scenes_driver())


# ---------------------------------------------------------------------------------------------------------------------------- scene

def _rot(rng, deg):
    a = rng.normal(0, 1, 3)
    a *= np.deg2rad(deg) / np.linalg.norm(a)
    th = np.linalg.norm(a)
    k = a / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


class Pose:
    def __init__(self, R, t):
        self.R = np.asarray(R, np.float32)
        self.t = np.asarray(t, np.float32)
        self.Ow = (-(self.R.T.astype(np.float64) @ self.t.astype(np.float64))).astype(np.float32)

    def near(self, rng, deg, dist):
        """a pose `deg` degrees and `dist` metres away"""
        d = rng.normal(0, 1, 3)
        c = self.Ow.astype(np.float64) + d / np.linalg.norm(d) * dist
        R = (_rot(rng, deg) @ self.R.astype(np.float64)).astype(np.float32)
        return Pose(R, -(R.astype(np.float64) @ c))

    def cam23(self, intr, bounds):
        """the oracle's camera: Rcw, tcw, Ow, fx, fy, cx, cy, minX, maxX, minY, maxY (bounds given as minX, minY, maxX, maxY)"""
        return np.concatenate([self.R.reshape(9), self.t, self.Ow, np.float32(intr), np.float32([bounds[0], bounds[2], bounds[1], bounds[3]])]).astype(np.float32)


def _noisy(rng, de, flip):
    return np.packbits(np.unpackbits(de, axis=1) ^ (rng.random((len(de), 256)) < flip), axis=1)


def _bow_groups(rng, de, n_nodes=60):
    """as tests/test_gpu_parity.py: node id = a hash of 6 descriptor bits, features of a node in random insertion order"""
    bits = np.unpackbits(de, axis=1)[:, [3, 41, 77, 130, 201, 250]]
    node = (bits * (1 << np.arange(6))).sum(1) % n_nodes
    groups = {}
    for i in rng.permutation(len(de)):
        groups.setdefault(int(node[i]) * 7 + 3, []).append(int(i))
    return groups


def _distort(kp, intr):
    fx, fy, cx, cy = intr
    out = kp.copy()
    xn, yn = (kp["x"].astype(np.float64) - cx) / fx, (kp["y"].astype(np.float64) - cy) / fy
    r2 = xn * xn + yn * yn
    f = 1 + DIST[0] * r2 + DIST[1] * r2 * r2
    out["x"], out["y"] = (xn * f * fx + cx).astype(np.float32), (yn * f * fy + cy).astype(np.float32)
    return out


class Scene:
    def __init__(self, oracle, sf):
        self.o, self.sf = oracle, np.asarray(sf, np.float32)
        self.sigma2 = (self.sf * self.sf).astype(np.float32)
        self.kfs, self.frames, self.images, self.calls = [], [], [], []
        self.pos = np.zeros((0, 3), np.float32)
        self.normal = np.zeros((0, 3), np.float32)
        self.mind = np.zeros(0, np.float32)
        self.maxd = np.zeros(0, np.float32)
        self.desc = np.zeros((0, 32), np.uint8)
        self.bad = np.zeros(0, bool)
        self.track = np.zeros((0, 5), np.float32)             # inview, level, viewcos, projx, projy

    def add_points(self, pos, normal, mind, maxd, desc, bad):
        first = len(self.mind)
        self.pos = np.concatenate([self.pos, np.float32(pos)])
        self.normal = np.concatenate([self.normal, np.float32(normal)])
        self.mind = np.concatenate([self.mind, np.float32(mind)])
        self.maxd = np.concatenate([self.maxd, np.float32(maxd)])
        self.desc = np.concatenate([self.desc, np.asarray(desc, np.uint8)])
        self.bad = np.concatenate([self.bad, np.asarray(bad, bool)])
        self.track = np.concatenate([self.track, np.zeros((len(mind), 5), np.float32)])
        return np.arange(first, len(self.mind))

    def add_kf(self, rng, pose, intr, bounds, keys, desc, slots):
        self.kfs.append(dict(pose=pose, intr=intr, bounds=tuple(int(b) for b in bounds), keys=keys, desc=desc, slots=np.int32(slots),
                             groups=_bow_groups(rng, desc)))
        return len(self.kfs) - 1

    def add_frame(self, rng, pose, intr, bounds, keys_un, desc, mps, outlier):
        Tcw = np.eye(4, dtype=np.float32)
        Tcw[:3, :3], Tcw[:3, 3] = pose.R, pose.t
        self.frames.append(dict(pose=pose, intr=intr, bounds=tuple(float(b) for b in bounds), Tcw=Tcw, keys=_distort(keys_un, intr),
                                keys_un=keys_un, desc=desc, mps=np.int32(mps), outlier=np.asarray(outlier, np.uint8), groups=_bow_groups(rng, desc)))
        return len(self.frames) - 1

    def call(self, op, i=(), f=(), lists=()):
        self.calls.append((op, [int(x) for x in i], [float(x) for x in np.asarray(f, np.float32).ravel()], [[int(x) for x in l] for l in lists]))

    # -- serialisation (layout: the comment at the top of tests/cpp/compat_scenes.cpp) --
    def write(self, path):
        b = [struct.pack("<ii", 0x43535655, 1)]
        i32 = lambda *v: b.append(struct.pack("<%di" % len(v), *v))
        raw = lambda a, dt: b.append(np.ascontiguousarray(a, dt).tobytes())

        def fv(groups):
            i32(len(groups))
            for node in sorted(groups):
                b.append(struct.pack("<Ii", node, len(groups[node])))
                raw(groups[node], "<i4")
        i32(len(self.kfs))
        for k in self.kfs:
            i32(len(k["keys"]), len(self.sf))
            raw(k["intr"], "<f4"), i32(*k["bounds"]), raw(self.sf, "<f4"), raw(self.sigma2, "<f4")
            raw(k["pose"].R, "<f4"), raw(k["pose"].t, "<f4"), raw(k["pose"].Ow, "<f4")
            raw(k["keys"], oracle_lib.KP), raw(k["desc"], np.uint8), raw(k["slots"], "<i4")
            fv(k["groups"])
        i32(len(self.mind))
        for p in range(len(self.mind)):
            raw(self.pos[p], "<f4"), raw(self.normal[p], "<f4"), raw([self.mind[p], self.maxd[p]], "<f4"), raw(self.desc[p], np.uint8)
            i32(int(self.bad[p]), int(self.track[p, 0]), int(self.track[p, 1])), raw(self.track[p, 2:], "<f4")
        i32(len(self.frames))
        for fr in self.frames:
            i32(len(fr["keys"]), len(self.sf))
            raw(fr["intr"], "<f4"), raw([fr["bounds"][0], fr["bounds"][1], fr["bounds"][2], fr["bounds"][3]], "<f4"), raw(self.sf, "<f4"), raw(fr["Tcw"], "<f4")
            raw(fr["keys"], oracle_lib.KP), raw(fr["keys_un"], oracle_lib.KP), raw(fr["desc"], np.uint8), raw(fr["mps"], "<i4"), raw(fr["outlier"], np.uint8)
            fv(fr["groups"])
        i32(len(self.images))
        for img, stride in self.images:
            h, w = img.shape
            buf = np.zeros((h, stride), np.uint8)
            buf[:, :w] = img
            buf[:, w:] = 77                                   # padding the adaptor must not read as pixels
            i32(w, h, stride), raw(buf, np.uint8)
        i32(len(self.calls))
        for op, ii, ff, ll in self.calls:
            i32(op, len(ii), *ii), i32(len(ff)), raw(ff, "<f4"), i32(len(ll))
            for l in ll:
                i32(len(l), *l)
        with open(path, "wb") as fp:
            fp.write(b"".join(b))


def _view(rng, sc, pts, pose, intr, bounds, oct_src, ang_src, base_desc, n_distract, flip=0.06, rand_frac=0.1, noise=0.7):
    """key points of a view of world points `pts`: projections with pixel noise, octave jitter of +-1, angle jitter (some far off),
    noisy descriptor copies, distractors (oct_src, ang_src, base_desc: per point id); returns (keys, desc, src point per key or -1) in shuffled order"""
    fx, fy, cx, cy = intr
    pc = sc.pos[pts].astype(np.float64) @ pose.R.T.astype(np.float64) + pose.t
    z = pc[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        u = fx * pc[:, 0] / z + cx + rng.normal(0, noise, len(pts))
        v = fy * pc[:, 1] / z + cy + rng.normal(0, noise, len(pts))
    vis = (z > 0.1) & (u >= bounds[0]) & (u < bounds[2]) & (v >= bounds[1]) & (v < bounds[3])
    idx = np.nonzero(vis)[0]
    n = len(idx) + n_distract
    keys = np.zeros(n, oracle_lib.KP)
    keys["x"][:len(idx)], keys["y"][:len(idx)] = u[idx], v[idx]
    keys["x"][len(idx):] = rng.uniform(bounds[0], bounds[2] - 1, n_distract)
    keys["y"][len(idx):] = rng.uniform(bounds[1], bounds[3] - 1, n_distract)
    pid = pts[idx]
    oct_ = np.concatenate([np.clip(oct_src[pid] + rng.integers(-1, 2, len(idx)), 0, len(sc.sf) - 1), rng.integers(0, len(sc.sf), n_distract)])
    ang = np.concatenate([ang_src[pid] + rng.normal(0, 2.0, len(idx)) + np.where(rng.random(len(idx)) < 0.12, rng.uniform(40, 180, len(idx)), 0),
                          rng.uniform(0, 360, n_distract)])
    keys["octave"], keys["angle"] = oct_, np.mod(ang, 360).astype(np.float32)
    keys["size"] = (31 * sc.sf[oct_]).astype(np.float32)
    keys["response"], keys["class_id"] = rng.uniform(0, 1e-3, n).astype(np.float32), -1
    desc = np.concatenate([_noisy(rng, base_desc[pid], flip), rng.integers(0, 256, (n_distract, 32), dtype=np.uint8)])
    rnd = rng.random(len(idx)) < rand_frac
    desc[:len(idx)][rnd] = rng.integers(0, 256, (int(rnd.sum()), 32), dtype=np.uint8)
    src = np.concatenate([pid, np.full(n_distract, -1)])
    perm = rng.permutation(n)
    return keys[perm], desc[perm], src[perm].astype(np.int64)


def _slots(rng, src, dup_of, p_orig, p_dup):
    """slot assignment of a view: with probability p_orig the key point's own point, p_dup a duplicate of it, else NULL"""
    r = rng.random(len(src))
    s = np.full(len(src), -1, np.int64)
    own = (src >= 0) & (r < p_orig)
    s[own] = src[own]
    dup = (src >= 0) & (r >= p_orig) & (r < p_orig + p_dup)
    s[dup] = [dup_of.get(int(x), -1) for x in src[dup]]
    return s


def _f12(p1, intr1, p2, intr2):
    """ComputeF12 (src/LocalMapping.cc): K1^-T [t12]x R12 K2^-1"""
    R1, t1, R2, t2 = (p.astype(np.float64) for p in (p1.R, p1.t, p2.R, p2.t))
    R12 = R1 @ R2.T
    t12 = -R1 @ R2.T @ t2 + t1
    tx = np.array([[0, -t12[2], t12[1]], [t12[2], 0, -t12[0]], [-t12[1], t12[0], 0]])
    K = lambda i: np.array([[i[0], 0, i[2]], [0, i[1], i[3]], [0, 0, 1.0]])
    return (np.linalg.inv(K(intr1)).T @ tx @ R12 @ np.linalg.inv(K(intr2))).astype(np.float32)


def build_scene(oracle, synth):
    rng = np.random.default_rng(20261016)
    oe = oracle.extractor(1000, 1.2, 8, 7)
    img = synth.make_frame(4242, W, H)
    kpA, deA = oe(img)                                        # view A comes from the oracle extractor, not the product
    sc = Scene(oracle, oe.scale)
    n = len(kpA)
    # -- world: A's key points back-projected at 2-20 m through pose A --
    pA = Pose(_rot(rng, 8), rng.normal(0, 0.5, 3))
    fx, fy, cx, cy = INTR_A
    z = rng.uniform(2, 20, n)
    pc = np.stack([(kpA["x"] - cx) / fx * z, (kpA["y"] - cy) / fy * z, z], 1)
    Xw = (pc - pA.t.astype(np.float64)) @ pA.R.astype(np.float64)
    nrm = Xw - pA.Ow
    dist = np.linalg.norm(nrm, axis=1)
    # mfMinDistance such that Fuse's dist / GetMinDistanceInvariance() (src/ORBmatcher.cc:1059-1062) predicts A's octave
    mind = dist * 1.1 / (0.8 * sc.sf[kpA["octave"]])
    maxd = dist * 2.0
    pdesc = _noisy(rng, deA, 0.04)
    stale = rng.random(n) < 0.25                              # descriptors far from every view: only a Replace makes them findable
    pdesc[stale] = rng.integers(0, 256, (int(stale.sum()), 32), dtype=np.uint8)
    orig = sc.add_points(Xw, nrm / dist[:, None], mind, maxd, pdesc, rng.random(n) < 0.08)
    # duplicates of a third of the points (same place, own descriptor): what Fuse merges
    has_dup = np.nonzero(rng.random(n) < 0.35)[0]
    dups = sc.add_points(Xw[has_dup] + rng.normal(0, 0.005, (len(has_dup), 3)), nrm[has_dup] / dist[has_dup, None], mind[has_dup],
                         maxd[has_dup], _noisy(rng, deA[has_dup], 0.04), np.zeros(len(has_dup), bool))
    dup_of = dict(zip(has_dup.tolist(), dups.tolist()))
    oct_src = np.concatenate([kpA["octave"], kpA["octave"][has_dup]])
    ang_src = np.concatenate([kpA["angle"], kpA["angle"][has_dup]])
    base = np.concatenate([deA, deA[has_dup]])
    # -- key frames --
    bounds_A = (-9, -6, 761, 487)
    slotsA = np.where(rng.random(n) < 0.75, orig, -1)
    # duplicates of some of A's own points also sit in free slots of A: FuseTargets merges them into the original in B or C, which
    # recomputes the original's descriptor before C (or D) searches it
    free = list(rng.permutation(np.nonzero(slotsA < 0)[0]))
    for p in rng.permutation(has_dup):
        if slotsA[p] >= 0 and free and rng.random() < 0.5:
            slotsA[free.pop()] = dup_of[int(p)]
    K0 = sc.add_kf(rng, pA, INTR_A, bounds_A, kpA, deA, slotsA)
    poses = [pA.near(rng, rng.uniform(2, 5), rng.uniform(0.2, 0.5)) for _ in range(4)]
    views = []
    for j, (pose, intr, bnd) in enumerate(zip(poses, (INTR_B, INTR_A, INTR_A, INTR_B), ((-7, -11, 758, 484), (-9, -6, 761, 487),
                                                                                       (-4, -8, 755, 490), (-7, -11, 758, 484)))):
        pts = np.concatenate([orig, dups]) if j < 2 else orig
        views.append((pose, intr, bnd) + _view(rng, sc, pts, pose, intr, bnd, oct_src, ang_src, base, 150))
    (pB, iB, bB, kB, dB, sB), (pC, iC, bC, kC, dC, sC), (pD, iD, bD, kD, dD, sD), (pE, iE, bE, kE, dE, sE) = views
    K1 = sc.add_kf(rng, pB, iB, bB, kB, dB, _slots(rng, sB, dup_of, 0.6, 0.15))
    K2 = sc.add_kf(rng, pC, iC, bC, kC, dC, _slots(rng, sC, dup_of, 0.45, 0.2))
    K3 = sc.add_kf(rng, pD, iD, bD, kD, dD, _slots(rng, sD, dup_of, 0.0, 0.45))      # Fuse target: duplicates or free
    K4 = sc.add_kf(rng, pE, iE, bE, kE, dE, _slots(rng, sE, dup_of, 0.0, 0.45))      # Fuse(Scw) target
    # -- a key frame above the adaptor's initial capacities (4096 key points, 8192 map points) --
    m_big = 9000
    pF = Pose(_rot(rng, 3), rng.normal(0, 0.3, 3))
    zb = rng.uniform(2, 20, m_big)
    ub, vb = rng.uniform(-9, 760, m_big), rng.uniform(-6, 486, m_big)
    pcb = np.stack([(ub - cx) / fx * zb, (vb - cy) / fy * zb, zb], 1)
    Xb = (pcb - pF.t.astype(np.float64)) @ pF.R.astype(np.float64)
    octb = rng.integers(0, 8, m_big)
    db = np.linalg.norm(Xb - pF.Ow, axis=1)
    base_b = rng.integers(0, 256, (m_big, 32), dtype=np.uint8)
    big = sc.add_points(Xb, (Xb - pF.Ow) / db[:, None], db * sc.sf[octb] / sc.sf[-1], db * sc.sf[octb], _noisy(rng, base_b, 0.04), rng.random(m_big) < 0.05)
    kF, dF, sF = _view(rng, sc, big[:5200], pF, INTR_A, bounds_A, np.concatenate([np.zeros(big[0], np.int64), octb]), np.zeros(len(sc.mind)),
                       np.concatenate([np.zeros((big[0], 32), np.uint8), base_b]), 300)
    assert len(kF) > 4096
    K5 = sc.add_kf(rng, pF, INTR_A, bounds_A, kF, dF, np.where((sF >= 0) & (rng.random(len(sF)) < 0.3), sF, -1))
    # -- frames: B, C and A as frames (distorted mvKeys next to mvKeysUn) --
    fb = (-8.0, -5.0, 760.0, 486.0)
    FB = sc.add_frame(rng, pB, iB, fb, kB, dB, np.where((sB >= 0) & (rng.random(len(sB)) < 0.1), sB, -1), np.zeros(len(kB)))
    FC = sc.add_frame(rng, pC, INTR_A, fb, kC, dC, np.where((sC >= 0) & (rng.random(len(sC)) < 0.1), sC, -1), np.zeros(len(kC)))
    FD = sc.add_frame(rng, pD, iD, fb, kD, dD, np.where((sD >= 0) & (rng.random(len(sD)) < 0.1), sD, -1), np.zeros(len(kD)))
    FA = sc.add_frame(rng, pA, INTR_A, fb, kpA, deA, np.where(rng.random(n) < 0.85, orig, -1), rng.random(n) < 0.15)
    # tracking fields (isInFrustum's outputs) for frame B: its own projections, with noise
    pcB = Xw @ pB.R.T.astype(np.float64) + pB.t
    uB, vB = iB[0] * pcB[:, 0] / pcB[:, 2] + iB[2], iB[1] * pcB[:, 1] / pcB[:, 2] + iB[3]
    inB = (pcB[:, 2] > 0) & (uB > fb[0]) & (uB < fb[2]) & (vB > fb[1]) & (vB < fb[3]) & (rng.random(n) < 0.9)
    sc.track[orig, 0] = inB
    sc.track[orig, 1] = np.clip(kpA["octave"] + rng.integers(-1, 2, n), 0, 7)
    sc.track[orig, 2] = np.where(rng.random(n) < 0.5, 0.999, 0.9)
    sc.track[orig, 3] = np.where(inB, uB + rng.normal(0, 1.0, n), 0)
    sc.track[orig, 4] = np.where(inB, vB + rng.normal(0, 1.0, n), 0)
    # -- images for the extractor: stride > width, and a wider but shorter one --
    sc.images.append((img, 768))
    sc.images.append((synth.make_frame(4243, 800, 400), 800))
    ids = dict(K0=K0, K1=K1, K2=K2, K3=K3, K4=K4, K5=K5, FA=FA, FB=FB, FC=FC, FD=FD, orig=orig, dups=dups, big=big, oe=oe, rng=rng)
    return sc, ids


def add_calls(sc, ids):
    rng = ids["rng"]
    K0, K1, K2, K3, K4, K5, FA, FB, FC, FD = (ids[k] for k in ("K0", "K1", "K2", "K3", "K4", "K5", "FA", "FB", "FC", "FD"))
    orig = ids["orig"]
    kf = sc.kfs
    # tracking (src/Tracking.cc): motion model th 15 / 7, reference key frame by BoW, relocalisation 10 / 100 and 3 / 64, local map 1 / 3 / 5
    sc.call(OP_MATCHER, [1], [0.75])
    sc.call(OP_BOW_KF_FRAME, [K0, FB])
    in_a = [int(p) for p in kf[K0]["slots"] if p >= 0]
    sc.call(OP_SBP_KF, [FC, K0, 100], [10], [[p for p in in_a if rng.random() < 0.25]])
    sc.call(OP_SBP_KF, [FC, K0, 64], [3], [[p for p in in_a if rng.random() < 0.25]])
    sc.call(OP_MATCHER, [1], [0.9])
    sc.call(OP_SBP_LAST, [FB, FA], [15])
    sc.call(OP_MATCHER, [0], [0.9])
    sc.call(OP_SBP_LAST, [FC, FA], [7])
    sc.call(OP_MATCHER, [1], [0.8])
    sc.call(OP_SBP_LOCAL, [FB], [1], [orig])
    sc.call(OP_MATCHER, [0], [0.6])
    sc.call(OP_SBP_LOCAL, [FB], [5], [orig])
    # the four members nothing in the reference calls
    sc.call(OP_MATCHER, [1], [0.9])
    sc.call(OP_WINDOW, [FA, FB, 100])
    sc.call(OP_WINDOW, [FA, FB, 100, 1, 3])
    sc.call(OP_MATCHER, [0], [0.9])
    sc.call(OP_WINDOW, [FA, FD, 10])
    sc.call(OP_SBP_FRAMES, [FA, FD, 10])
    prev = np.stack([sc.frames[FA]["keys_un"]["x"], sc.frames[FA]["keys_un"]["y"]], 1) + rng.normal(0, 3, (len(sc.frames[FA]["keys_un"]), 2))
    sc.call(OP_INIT, [FA, FB, 100], prev)
    # key frame to key frame: BoW, Sim3 (loop detection), triangulation
    sc.call(OP_MATCHER, [1], [0.75])
    sc.call(OP_BOW_KF_KF, [K0, K1])
    pa, pb = kf[K0]["pose"], kf[K1]["pose"]
    R12 = (pa.R.astype(np.float64) @ pb.R.T.astype(np.float64)).astype(np.float32)
    t12 = (pa.t - R12.astype(np.float64) @ pb.t).astype(np.float32)
    m12 = np.full(len(kf[K0]["keys"]), -1)
    s1 = np.nonzero(rng.random(len(m12)) < 0.15)[0]
    b_pts = [int(p) for p in kf[K1]["slots"] if p >= 0]
    m12[s1] = rng.choice(b_pts, len(s1))                    # wrong pairings: vpMatches12 as a previous loop search left it
    sc.call(OP_SIM3, [K0, K1], np.concatenate([[1.0], R12.ravel(), t12, [7.5]]), [m12])
    sc.call(OP_MATCHER, [0], [0.6])
    sc.call(OP_TRIANG, [K3, K4], _f12(kf[K3]["pose"], kf[K3]["intr"], kf[K4]["pose"], kf[K4]["intr"]))
    # local mapping: the fuse loop of SearchInNeighbors, then Fuse run small then above the initial capacities on one object
    sc.call(OP_MATCHER, [1], [0.6])
    sc.call(OP_FUSE_TARGETS, [], [3], [[K1, K2], kf[K0]["slots"]])
    sc.call(OP_FUSE, [K3], [3], [list(orig) + [-1, -1]])
    sc.call(OP_FUSE, [K5], [3], [ids["big"]])
    # loop closing: SearchByProjection(pKF, Scw, ..., 10) and Fuse(pKF, Scw, ..., 4) with s = 1.7
    pe = kf[K4]["pose"]
    Scw = np.eye(4, dtype=np.float32)
    Scw[:3, :3], Scw[:3, 3] = np.float32(1.7) * pe.R, np.float32(1.7) * pe.t
    loop_pts = [int(p) for p in orig]
    vm = np.where(rng.random(len(kf[K4]["keys"])) < 0.15, rng.choice(orig, len(kf[K4]["keys"])), -1)
    sc.call(OP_MATCHER, [1], [0.75])
    sc.call(OP_SBP_SCW, [K4, 10], Scw, [loop_pts, vm])
    sc.call(OP_FUSE_SCW, [K4], np.concatenate([Scw.ravel(), [4]]), [loop_pts])
    # triangulation batch with a Fuse that grows the handle between two Next calls (a fresh object: initial capacities)
    sc.call(OP_MATCHER, [0], [0.6])
    sc.call(OP_TRI_BEGIN, [K0], np.concatenate([_f12(pa, kf[K0]["intr"], kf[k]["pose"], kf[k]["intr"]).ravel() for k in (K1, K2)]), [[K1, K2]])
    sc.call(OP_TRI_NEXT, [K0, K1, 0, 1])
    sc.call(OP_FUSE, [K5], [3], [ids["big"][::-1]])
    sc.call(OP_TRI_NEXT, [K0, K2, 1, 1])
    # the contract of a Next without a Begin on this object
    sc.call(OP_MATCHER, [0], [0.6])
    sc.call(OP_TRI_NEXT, [K0, K1, 0, 1])
    # extractor and grider adaptors
    sc.call(OP_EXTRACTOR, [1000, 8, 7], [1.2])
    sc.call(OP_EXTRACT, [0, W, H, 768, 20, 1, 0, 0, 0])
    min_px = 20
    rows, cols = H // min_px + 2, W // min_px + 2
    kin = np.zeros(300, oracle_lib.KP)
    kin["x"], kin["y"] = rng.uniform(20, W - 21, 300), rng.uniform(20, H - 21, 300)
    kin["size"], kin["angle"], kin["response"], kin["octave"], kin["class_id"] = 31, -1, rng.uniform(0, 99, 300), 0, np.arange(300)
    grid = np.zeros((rows, cols), np.int32, order="F")
    for k in kin:
        grid[int(k["y"] / min_px), int(k["x"] / min_px)] += 1
    ids["topup"] = (kin, grid)
    sc.call(OP_EXTRACT, [0, W, H, 768, min_px, 0, 500, rows, cols], [], [np.frombuffer(kin.tobytes(), np.int32), grid.ravel(order="F")])
    sc.call(OP_EXTRACT, [1, 800, 400, 800, 20, 1, 0, 0, 0])
    sc.call(OP_EXTRACT, [-1, 0, 0, 0, 20, 1, 0, 0, 0], [], [np.frombuffer(kin[:5].tobytes(), np.int32)])
    sc.call(OP_GRIDER, [0, 200, 8, 5, 20, 1])
    sc.call(OP_GRIDER, [1, 400, 5, 3, 10, 0])


# ------------------------------------------------------------------------------------------------------------------- expected values

class Expect:
    """runs the scene's calls on the Python model through the oracle primitives; records what the driver must dump"""

    def __init__(self, oracle, sc, ids):
        self.o, self.sc, self.ids = oracle, sc, ids
        self.model = cm.MapModel([cm.KeyFrame(k["desc"], k["slots"]) for k in sc.kfs],
                                 [cm.MapPoint(i, sc.desc[i], sc.bad[i]) for i in range(len(sc.mind))])
        self.frame_mps = [list(f["mps"]) for f in sc.frames]
        self.cover = {}
        self.records = []
        self.tri = None

    def bump(self, key, n):
        self.cover[key] = self.cover.get(key, 0) + int(n)

    def mp(self, pid):
        return self.model.mps[pid]

    def bad(self, pid):
        return pid >= 0 and self.model.mps[pid].bad

    def ibounds(self, b):
        return tuple(int(x) for x in b)

    def kf_cam(self, k):
        kf = self.sc.kfs[k]
        return kf["pose"].cam23(kf["intr"], kf["bounds"])

    def frame_cam(self, f):
        fr = self.sc.frames[f]
        c = fr["pose"].cam23(fr["intr"], fr["bounds"])
        c[12:15] = 0                                          # Ow: derived by the projection (:1628); the frame carries none
        return c

    def fuse_search_one(self, k, p, cam=None):
        """the per-point body of both Fuse forms with the point's descriptor as it is now"""
        kf = self.sc.kfs[k]
        cam = self.kf_cam(k) if cam is None else cam
        i = p.id
        # the oracle takes mfMinDistance / mfMaxDistance and forms GetMin/MaxDistanceInvariance itself
        valid, u, v, lvl, _ = self.o.project_points(2, cam, self.sc.pos[i:i + 1], self.sc.normal[i:i + 1], self.sc.mind[i:i + 1], self.sc.maxd[i:i + 1],
                                                    None, self.sc.sf, 0.0, 0.0)
        best, _ = self.o.fuse_search(kf["keys"], kf["desc"], kf["bounds"], u, v, lvl, valid, p.desc[None], self.sc.sf, self.th)
        return int(best[0])

    def ids_of(self, lst):
        return " ".join(str(int(x)) for x in lst)

    def run(self):
        sc = self.sc
        for ci, (op, I, F, L) in enumerate(sc.calls):
            rec = dict(op=op, v={}, map=False)
            ret = getattr(self, "op%d" % op)(I, F, L, rec)
            rec["ret"] = ret
            if op not in (OP_MATCHER, OP_EXTRACTOR):
                rec["v"].setdefault("err", "-")
            if rec["map"]:
                rec["kf"], rec["mp"] = self.model.dump()
            self.records.append(rec)
        return self.records

    # -- ops --
    def op0(self, I, F, L, rec):
        self.nnratio, self.check_ori = F[0], bool(I[0])
        self.tri = None                                        # a new object holds no triangulation batch
        return 0

    def op17(self, I, F, L, rec):
        self.oe = self.o.extractor(I[0], F[0], I[1], I[2])
        return 0

    def op1(self, I, F, L, rec):                               # SearchByProjection(F, vpMapPoints, th) :49-125
        f, th, pts = I[0], F[0], np.asarray(L[0])
        fr, sc = self.sc.frames[f], self.sc
        assigned = np.where(np.asarray(self.frame_mps[f]) >= 0, TAKEN, -1).astype(np.int32)
        inview = np.array([sc.track[p, 0] > 0 and not self.bad(p) for p in pts], np.uint8)
        desc = np.stack([self.mp(p).desc for p in pts])
        n = self.o.search_by_projection(fr["keys_un"], fr["desc"], self.ibounds(fr["bounds"]), assigned, sc.track[pts, 3], sc.track[pts, 4],
                                        sc.track[pts, 1].astype(np.int32), sc.track[pts, 2], inview, desc, sc.sf, th, self.nnratio)
        bad_in = np.array([sc.track[p, 0] > 0 for p in pts], np.uint8)
        a2 = np.where(np.asarray(self.frame_mps[f]) >= 0, TAKEN, -1).astype(np.int32)
        self.o.search_by_projection(fr["keys_un"], fr["desc"], self.ibounds(fr["bounds"]), a2, sc.track[pts, 3], sc.track[pts, 4],
                                    sc.track[pts, 1].astype(np.int32), sc.track[pts, 2], bad_in, desc, sc.sf, th, self.nnratio)
        self.bump("skip:bad", (a2 != assigned).sum())
        for k in range(len(assigned)):
            if 0 <= assigned[k] < TAKEN:
                self.frame_mps[f][k] = int(pts[assigned[k]])
        rec["v"]["frame"] = self.ids_of(self.frame_mps[f])
        self.bump("matches:sbp_local", n)
        return n

    def op2(self, I, F, L, rec):                               # SearchByProjection(F, pKF, sAlreadyFound, th, ORBdist) :1622-1746
        f, k, orb, th = I[0], I[1], I[2], F[0]
        fr, kf, sc = self.sc.frames[f], self.sc.kfs[k], self.sc
        vp = list(self.model.kfs[k].slots)

        def search(found):
            usable = np.array([p >= 0 and not self.bad(p) and p not in found for p in vp], np.uint8)
            pts = np.maximum(vp, 0)
            valid, u, v, lvl, _ = self.o.project_points(1, self.frame_cam(f), sc.pos[pts], None, sc.mind[pts], sc.maxd[pts], usable, sc.sf)
            desc = np.stack([self.mp(p).desc for p in pts])
            assigned = np.where(np.asarray(self.frame_mps[f]) >= 0, TAKEN, -1).astype(np.int32)
            n = self.o.search_by_projection_kf(fr["keys_un"], fr["desc"], self.ibounds(fr["bounds"]), assigned, u, v, lvl, valid, desc,
                                               kf["keys"]["angle"], sc.sf, th, orb, self.check_ori)
            return assigned, n
        assigned, n = search(set(L[0]))
        self.bump("skip:already_found", (search(set())[0] != assigned).sum())
        for i in range(len(assigned)):
            if 0 <= assigned[i] < TAKEN:
                self.frame_mps[f][i] = vp[assigned[i]]
        rec["v"]["frame"] = self.ids_of(self.frame_mps[f])
        self.bump("matches:sbp_kf", n)
        return n

    def _bow(self, kf_kf, k1, side2, usable2, check_ori=None):
        kf = self.sc.kfs[k1]
        vp1 = self.model.kfs[k1].slots
        u1 = np.array([p >= 0 and not self.bad(p) for p in vp1], np.uint8)
        return self.o.search_by_bow(kf_kf, kf["groups"], kf["desc"], kf["keys"]["angle"], u1, side2["groups"], side2["desc"], side2["angle"],
                                    usable2, self.nnratio, self.check_ori if check_ori is None else check_ori)

    def op3(self, I, F, L, rec):                               # SearchByBoW(pKF, F) :155-284
        k, f = I
        fr = self.sc.frames[f]
        side2 = dict(groups=fr["groups"], desc=fr["desc"], angle=fr["keys"]["angle"])
        match, n = self._bow(False, k, side2, None)
        if self.check_ori:
            self.bump("rotation_filter", (self._bow(False, k, side2, None, False)[0] != match).sum())
        out = [-1] * len(fr["keys"])
        for i, j in enumerate(match):
            if j >= 0:
                out[j] = self.model.kfs[k].slots[i]
        rec["v"]["matches"] = self.ids_of(out)
        self.bump("matches:bow_kf_frame", n)
        return n

    def op4(self, I, F, L, rec):                               # SearchByBoW(pKF1, pKF2) :715-850
        k1, k2 = I
        kf2 = self.sc.kfs[k2]
        vp2 = self.model.kfs[k2].slots
        side2 = dict(groups=kf2["groups"], desc=kf2["desc"], angle=kf2["keys"]["angle"])
        match, n = self._bow(True, k1, side2, np.array([p >= 0 and not self.bad(p) for p in vp2], np.uint8))
        m_bad, _ = self.o.search_by_bow(True, self.sc.kfs[k1]["groups"], self.sc.kfs[k1]["desc"], self.sc.kfs[k1]["keys"]["angle"],
                                        np.array([p >= 0 for p in self.model.kfs[k1].slots], np.uint8), side2["groups"], side2["desc"],
                                        side2["angle"], np.array([p >= 0 for p in vp2], np.uint8), self.nnratio, self.check_ori)
        self.bump("skip:bad", (m_bad != match).sum())
        rec["v"]["matches"] = self.ids_of([vp2[j] if j >= 0 else -1 for j in match])
        self.bump("matches:bow_kf_kf", n)
        return n

    def _triang(self, k1, k2, f12, has1):
        a, b = self.sc.kfs[k1], self.sc.kfs[k2]
        has2 = np.array([p >= 0 for p in self.model.kfs[k2].slots], np.uint8)
        return self.o.search_for_triangulation(a["groups"], a["keys"], a["desc"], has1, b["groups"], b["keys"], b["desc"], has2, f12,
                                               self.sc.sigma2, self.check_ori)

    def _pairs(self, k2, match, rec):
        pairs = [(i, int(j)) for i, j in enumerate(match) if j >= 0]
        rec["v"]["pairs"] = " ".join("%d %d" % p for p in pairs)
        rec["v"]["keys2"] = b"".join(self.sc.kfs[k2]["keys"][j].tobytes() for _, j in pairs).hex()
        return pairs

    def op5(self, I, F, L, rec):                               # SearchForTriangulation :852-1014
        k1, k2 = I
        has1 = np.array([p >= 0 for p in self.model.kfs[k1].slots], np.uint8)
        match, n = self._triang(k1, k2, np.float32(F).reshape(3, 3), has1)
        pairs = self._pairs(k2, match, rec)
        rec["v"]["keys1"] = b"".join(self.sc.kfs[k1]["keys"][i].tobytes() for i, _ in pairs).hex()
        self.bump("matches:triangulation", n)
        return n

    def op7(self, I, F, L, rec):                               # SearchForTriangulationBegin
        self.tri = dict(k1=I[0], f12=[np.float32(F[9 * j:9 * j + 9]).reshape(3, 3) for j in range(len(L[0]))],
                        has1=np.array([p >= 0 for p in self.model.kfs[I[0]].slots], np.uint8))
        return 0

    def op8(self, I, F, L, rec):                               # SearchForTriangulationNext, then the creation rule of compat_scenes.cpp
        k1, k2, j, create = I
        rec["map"] = True
        if self.tri is None:                                   # Next without Begin: 0 matches and last_error() set (ORBmatcher.h)
            rec["v"].update(pairs="", keys2="", err="set")
            return 0
        has1 = np.array([p >= 0 for p in self.model.kfs[k1].slots], np.uint8)
        match, n = self._triang(k1, k2, self.tri["f12"][j], has1)
        self.bump("tri_next:gained_between_calls", (self._triang(k1, k2, self.tri["f12"][j], self.tri["has1"])[0] != match).sum())
        pairs = self._pairs(k2, match, rec)
        if create:
            for i1, i2 in pairs:
                if i1 % 3:
                    continue
                p = self.model.new_point(self.sc.kfs[k1]["desc"][i1])
                self.model.add_observation(p, k1, i1), self.model.add_observation(p, k2, i2)
                self.model.kfs[k1].slots[i1], self.model.kfs[k2].slots[i2] = p.id, p.id
        rec["map"] = True
        self.bump("matches:tri_next", n)
        return n

    def op6(self, I, F, L, rec):                               # Fuse(pKF, vpMapPoints, th)
        self.th = F[0]
        c0 = dict(self.model.counts)
        n = self.model.fuse(I[0], L[0], lambda k, p: self.fuse_search_one(k, p))
        self._fuse_cover("fuse", c0)
        rec["map"] = True
        self.bump("matches:fuse", n)
        return n

    def _fuse_cover(self, form, c0):
        for key in ("replace", "add", "redescribed_searched", "redescribed_changed"):
            self.bump("%s:%s" % (form, key), self.model.counts.get("%s:%s" % (form, key), 0) - c0.get("%s:%s" % (form, key), 0))

    def op9(self, I, F, L, rec):                               # FuseTargets = the loop of src/LocalMapping.cc:1228-1236
        self.th = F[0]
        c0 = dict(self.model.counts)
        n = self.model.fuse_targets(L[0], L[1], lambda k, p: self.fuse_search_one(k, p))
        self._fuse_cover("fuse_targets", c0)
        rec["map"] = True
        self.bump("matches:fuse_targets", n)
        return n

    def _scw_cam(self, k, Scw):
        r, t, o = self.o.sim3_decompose(np.float32(Scw).reshape(4, 4))
        kf = self.sc.kfs[k]
        b = kf["bounds"]
        return np.concatenate([r, t, o, np.float32(kf["intr"]), np.float32([b[0], b[2], b[1], b[3]])]).astype(np.float32)

    def op10(self, I, F, L, rec):                              # SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) :286-407
        k, th = I
        kf, sc = self.sc.kfs[k], self.sc
        cam = self._scw_cam(k, F)
        pts, vm = np.asarray(L[0]), list(L[1])

        def search(matched_in):
            found = {p for p in matched_in if p >= 0}
            usable = np.array([not self.bad(p) and p not in found for p in pts], np.uint8)
            valid, u, v, lvl, _ = self.o.project_points(2, cam, sc.pos[pts], sc.normal[pts], sc.mind[pts], sc.maxd[pts], usable, sc.sf, 0.0, 0.0)
            matched = np.where(np.asarray(matched_in) >= 0, TAKEN, -1).astype(np.int32)
            n = self.o.search_by_projection_sim3(kf["keys"], kf["desc"], kf["bounds"], matched, u, v, lvl, valid,
                                                 np.stack([self.mp(p).desc for p in pts]), sc.sf, th)
            return matched, n
        matched, n = search(vm)
        self.bump("skip:already_found", (search([-1] * len(vm))[0] != matched).sum())
        for i in range(len(vm)):
            if 0 <= matched[i] < TAKEN:
                vm[i] = int(pts[matched[i]])
        rec["v"]["matched"] = self.ids_of(vm)
        self.bump("matches:sbp_scw", n)
        return n

    def op11(self, I, F, L, rec):                              # Fuse(pKF, Scw, vpPoints, th) :1136-1265
        self.th = F[16]
        cam = self._scw_cam(I[0], F[:16])
        c0 = dict(self.model.counts)
        n = self.model.fuse_scw(I[0], L[0], lambda k, p: self.fuse_search_one(k, p, cam))
        self._fuse_cover("fuse_scw", c0)
        rec["map"] = True
        self.bump("matches:fuse_scw", n)
        return n

    def op12(self, I, F, L, rec):                              # SearchBySim3 :1267-1505
        k1, k2 = I
        s12, R12, t12, th = F[0], np.float32(F[1:10]).reshape(3, 3), np.float32(F[10:13]), F[13]
        sc, a, b = self.sc, self.sc.kfs[k1], self.sc.kfs[k2]
        vp1, vp2 = self.model.kfs[k1].slots, self.model.kfs[k2].slots
        vm = list(L[0])
        sR12, sR21, t21 = self.o.sim3_relative(s12, R12, t12)
        # both directions project with pKF1's intrinsics (:1270-1273) into the bounds of the target key frame
        cam1 = np.concatenate([np.zeros(15, np.float32), np.float32(a["intr"]), np.float32([a["bounds"][0], a["bounds"][2], a["bounds"][1], a["bounds"][3]])])
        cam2 = np.concatenate([np.zeros(15, np.float32), np.float32(a["intr"]), np.float32([b["bounds"][0], b["bounds"][2], b["bounds"][1], b["bounds"][3]])])

        def search(use_already2, cam2=cam2):
            already1 = [p >= 0 for p in vm]
            already2 = [False] * len(vp2)
            if use_already2:
                for p in vm:
                    if p >= 0 and k2 in self.mp(p).obs:
                        already2[self.mp(p).obs[k2]] = True

            def side(vp, already, R, t, sR, tt, cam, sf):
                pts = np.maximum(vp, 0)
                usable = np.array([p >= 0 and not al and not self.bad(p) for p, al in zip(vp, already)], np.uint8)
                proj = self.o.project_sim3(R, t, sR, tt, cam, sc.pos[pts], sc.mind[pts], sc.maxd[pts], usable, sf)
                return proj, np.stack([self.mp(p).desc for p in pts])
            p12, md1 = side(vp1, already1, a["pose"].R, a["pose"].t, sR21, t21, cam2, sc.sf)
            p21, md2 = side(vp2, already2, b["pose"].R, b["pose"].t, sR12, t12, cam1, sc.sf)
            return self.o.search_by_sim3(a["keys"], a["desc"], np.int32(a["bounds"]), b["keys"], b["desc"], np.int32(b["bounds"]), p12, md1, p21, md2,
                                         sc.sf, sc.sf, th)
        match, n = search(True)
        self.bump("skip:already_found", (search(False)[0] != match).sum())
        own = cam2.copy()
        own[15:19] = b["intr"]
        self.bump("sim3:first_kf_intrinsics", (search(True, own)[0] != match).sum())
        for i in range(len(vm)):
            if match[i] >= 0:
                vm[i] = vp2[match[i]]
        rec["v"]["matches"] = self.ids_of(vm)
        self.bump("matches:sim3", n)
        return n

    def op13(self, I, F, L, rec):                              # WindowSearch :409-516
        f1, f2, win = I[:3]
        lo, hi = (I[3], I[4]) if len(I) > 3 else (-1, 0x7FFFFFFF)
        a, b = self.sc.frames[f1], self.sc.frames[f2]
        has = np.array([p >= 0 and not self.bad(p) for p in self.frame_mps[f1]], np.uint8)
        m21, n = self.o.window_search(a["keys_un"], a["desc"], has, b["keys_un"], b["desc"], self.ibounds(b["bounds"]), win, lo, hi, self.nnratio,
                                      self.check_ori)
        if len(I) > 3:
            self.bump("skip:out_of_level", (self.o.window_search(a["keys_un"], a["desc"], has, b["keys_un"], b["desc"], self.ibounds(b["bounds"]), win,
                                                                 -1, 0x7FFFFFFF, self.nnratio, self.check_ori)[0] != m21).sum())
        rec["v"]["matches"] = self.ids_of([self.frame_mps[f1][j] if j >= 0 else -1 for j in m21])
        self.bump("matches:window", n)
        return n

    def op14(self, I, F, L, rec):                              # SearchByProjection(F1, F2, windowSize) :519-594
        f1, f2, win = I
        a, b, sc = self.sc.frames[f1], self.sc.frames[f2], self.sc
        vp1, out = self.frame_mps[f1], list(self.frame_mps[f2])
        found = set(out)
        usable = np.array([p >= 0 and not self.bad(p) and p not in found for p in vp1], np.uint8)
        assigned = np.where(np.asarray(out) >= 0, TAKEN, -1).astype(np.int32)
        n = self.o.search_by_projection_frames(a["keys_un"], a["desc"], usable, sc.pos[np.maximum(vp1, 0)], self.frame_cam(f2), b["keys_un"], b["desc"],
                                               assigned, win, self.nnratio)
        for k in range(len(out)):
            if 0 <= assigned[k] < TAKEN:
                out[k] = vp1[assigned[k]]
        rec["v"]["matches"] = self.ids_of(out)
        self.bump("matches:sbp_frames", n)
        return n

    def op15(self, I, F, L, rec):                              # SearchForInitialization :598-713
        f1, f2, win = I
        a, b = self.sc.frames[f1], self.sc.frames[f2]
        prev = np.float32(F).reshape(-1, 2).copy()
        m12, n = self.o.search_for_initialization(a["keys_un"], a["desc"], b["keys_un"], b["desc"], self.ibounds(b["bounds"]), prev, win,
                                                  self.nnratio, self.check_ori)
        rec["v"]["m12"] = self.ids_of(m12)
        rec["v"]["prev"] = prev.tobytes().hex()
        self.bump("matches:init", n)
        return n

    def op16(self, I, F, L, rec):                              # SearchByProjection(CurrentFrame, LastFrame, th) :1507-1620
        fc, fl, th = I[0], I[1], F[0]
        cur, last, sc = self.sc.frames[fc], self.sc.frames[fl], self.sc
        vpl = self.frame_mps[fl]

        def search(outl):
            usable = np.array([p >= 0 and not o for p, o in zip(vpl, outl)], np.uint8)
            assigned = np.where(np.asarray(self.frame_mps[fc]) >= 0, TAKEN, -1).astype(np.int32)
            n = self.o.search_by_projection_last(self.frame_cam(fc), cur["keys_un"], cur["desc"], assigned, usable, sc.pos[np.maximum(vpl, 0)],
                                                 last["keys"]["octave"], last["keys_un"]["angle"], last["desc"], sc.sf, th, self.check_ori)
            return assigned, n
        assigned, n = search(last["outlier"])
        self.bump("skip:outlier", (search(np.zeros(len(vpl)))[0] != assigned).sum())
        for k in range(len(assigned)):
            if 0 <= assigned[k] < TAKEN:
                self.frame_mps[fc][k] = vpl[assigned[k]]
        rec["v"]["frame"] = self.ids_of(self.frame_mps[fc])
        self.bump("matches:sbp_last", n)
        return n

    def op18(self, I, F, L, rec):                              # ORBextractor::extract
        img_i, w, h, stride, min_px, full, need, rows, cols = I
        kin = np.frombuffer(np.int32(L[0]).tobytes(), oracle_lib.KP) if L and L[0] else np.zeros(0, oracle_lib.KP)
        grid = np.int32(L[1]).reshape((rows, cols), order="F").copy(order="F") if len(L) > 1 else None
        if img_i < 0:                                          # empty image: the outputs stay as they were
            rec["v"].update(kps=kin.tobytes().hex(), desc="ab" * 5, grid="")
            return 0
        img = self.sc.images[img_i][0]
        kp, de = self.oe(img, kin.copy() if len(kin) else None, grid, min_px, bool(full), need)
        rec["v"].update(kps=kp.tobytes().hex(), desc=de.tobytes().hex(), grid="" if grid is None else " ".join(str(x) for x in grid.ravel(order="F")))
        self.bump("matches:extract", len(kp))
        return 0

    def op19(self, I, F, L, rec):                              # Grider_FAST::perform_griding: appended to three caller points
        img = self.sc.images[I[0]][0]
        pts = np.zeros(3, oracle_lib.KP)
        pts["class_id"] = [1000, 1001, 1002]
        got = self.o.grider_fast(img, I[1], I[2], I[3], I[4], bool(I[5]))
        rec["v"]["kps"] = np.concatenate([pts, got]).tobytes().hex()
        self.bump("matches:grider", len(got))
        return 0


def parse_dump(path):
    recs = []
    for line in open(path).read().splitlines():
        tag, _, rest = line.partition(" ")
        if tag == "call":
            _, op, ret = rest.split(" ")
            recs.append(dict(op=int(op), ret=int(ret), v={}, kf={}, mp={}))
        elif tag == "v":
            name, _, val = rest.partition(" ")
            recs[-1]["v"][name] = val
        elif tag == "kf":
            f, *ids = rest.split(" ")
            recs[-1]["kf"][int(f)] = [int(x) for x in ids]
        elif tag == "mp":
            t = rest.split(" ")
            nobs = int(t[3])
            obs = [tuple(int(x) for x in o.split(":")) for o in t[4:4 + nobs]]
            recs[-1]["mp"][int(t[0])] = (int(t[1]), int(t[2]), obs, t[4 + nobs])
    return recs


OP_NAMES = {v: k for k, v in globals().items() if k.startswith("OP_")}


@pytest.fixture(scope="module")
def scene_run(tmp_path_factory, oracle, synth):
    sc, ids = build_scene(oracle, synth)
    add_calls(sc, ids)
    ex = Expect(oracle, sc, ids)
    exp = ex.run()
    d = tmp_path_factory.mktemp("scenes")
    sc.write(str(d / "scene.bin"))
    r = subprocess.run([build_scenes_driver(), str(d / "scene.bin"), str(d / "dump.txt")], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    return sc, ex, exp, parse_dump(str(d / "dump.txt")), r.stderr


@pytest.mark.gpu
def test_adaptors_equal_the_oracle_on_the_scene(scene_run):
    """every call of the scene: return value, every output vector, and the whole map after each mutating call, exactly"""
    sc, ex, exp, got, stderr = scene_run
    assert len(got) == len(exp), stderr
    for ci, (e, g) in enumerate(zip(exp, got)):
        what = "call %d %s" % (ci, OP_NAMES[e["op"]])
        assert g["op"] == e["op"], what
        assert set(g["v"]) == set(e["v"]), (what, sorted(g["v"]), sorted(e["v"]))
        for name in e["v"]:
            assert g["v"][name] == e["v"][name], "%s: output %s differs (%s)" % (what, name, stderr)
        assert g["ret"] == e["ret"], "%s: returned %d, expected %d" % (what, g["ret"], e["ret"])
        if e["map"]:
            assert g["kf"] == e["kf"], what + ": key-frame slots differ"
            bad = [i for i in e["mp"] if g["mp"].get(i) != e["mp"][i]]
            assert not bad and len(g["mp"]) == len(e["mp"]), "%s: map points differ, first %s: got %s expected %s" % (
                what, bad[:1], [g["mp"].get(i) for i in bad[:1]], [e["mp"][i] for i in bad[:1]])


def test_scene_reaches_every_branch(oracle, synth):
    """coverage counters of the expected-value run (CPU only): the scene is not degenerate"""
    sc, ids = build_scene(oracle, synth)
    add_calls(sc, ids)
    ex = Expect(oracle, sc, ids)
    ex.run()
    c = ex.cover
    for member in ("sbp_local", "sbp_kf", "bow_kf_frame", "bow_kf_kf", "triangulation", "tri_next", "fuse", "fuse_targets", "sbp_scw",
                   "fuse_scw", "sim3", "window", "sbp_frames", "init", "sbp_last"):
        assert c.get("matches:" + member, 0) >= 100, (member, c)
    for form in ("fuse", "fuse_targets", "fuse_scw"):
        assert c.get(form + ":replace", 0) >= 10 and c.get(form + ":add", 0) >= 10, (form, c)
    assert c.get("fuse_targets:redescribed_changed", 0) >= 1, c
    assert c.get("sim3:first_kf_intrinsics", 0) >= 1, c
    for skip in ("already_found", "bad", "outlier", "out_of_level"):
        assert c.get("skip:" + skip, 0) >= 10, (skip, c)
    assert c.get("rotation_filter", 0) >= 1, c
    assert c.get("tri_next:gained_between_calls", 0) >= 1, c
    assert len(sc.kfs[ids["K5"]]["keys"]) > 4096 and len(ids["big"]) > 8192          # the second Fuse grows the handle
