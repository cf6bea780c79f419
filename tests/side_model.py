"""A third statement, in numpy, of four operations that the kernels and the C++ oracle were both written for from one reading of
OpenCV 3.4 / DBoW2 / haloc: cv::CLAHE::apply, Tracking::undistort_point, TemplatedVocabulary::transform and haloc::Hash::getHash.
Nothing here calls the oracle or the product.  tests/test_side_model.py holds these models to the oracle on the CPU,
tests/test_gpu_side.py holds the kernels to them; the case lists both run are in tests/side_cases.py."""
import math

import numpy as np


# ---- cv::CLAHE::apply, 8-bit (OpenCV 3.4 imgproc/src/clahe.cpp; src/Tracking.cc:425-431) ---------------------------------
def clahe(img, clip_limit, tiles):
    """Independent numpy statement of OpenCV 3.4's 8-bit CLAHE (vectorised differently from the oracle's loops)."""
    tx, ty = tiles
    h, w = img.shape
    if w % tx == 0 and h % ty == 0:
        ext = img
    else:
        ext = np.pad(img, ((0, ty - h % ty), (0, tx - w % tx)), mode="reflect")
    tw, th = ext.shape[1] // tx, ext.shape[0] // ty
    total = tw * th
    scale = np.float32(255) / np.float32(total)
    clip = max(int(clip_limit * total / 256), 1) if clip_limit > 0 else 0
    luts = np.zeros((ty, tx, 256), np.float32)
    for j in range(ty):
        for i in range(tx):
            hist = np.bincount(ext[j * th:(j + 1) * th, i * tw:(i + 1) * tw].ravel(), minlength=256).astype(np.int64)
            if clip > 0:
                clipped = int(np.maximum(hist - clip, 0).sum())
                hist = np.minimum(hist, clip) + clipped // 256
                residual = clipped % 256
                if residual:
                    step = max(256 // residual, 1)
                    idx = np.arange(0, 256, step)[:residual]
                    hist[idx] += 1
            luts[j, i] = np.clip(np.rint(np.cumsum(hist).astype(np.float32) * scale), 0, 255)
    xs, ys = np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32)
    txf = xs * (np.float32(1) / np.float32(tw)) - np.float32(0.5)
    tyf = ys * (np.float32(1) / np.float32(th)) - np.float32(0.5)
    tx1, ty1 = np.floor(txf).astype(int), np.floor(tyf).astype(int)
    xa, ya = (txf - tx1.astype(np.float32)).astype(np.float32), (tyf - ty1.astype(np.float32)).astype(np.float32)
    xa1, ya1 = np.float32(1) - xa, np.float32(1) - ya
    tx2, ty2 = np.minimum(tx1 + 1, tx - 1), np.minimum(ty1 + 1, ty - 1)
    tx1, ty1 = np.maximum(tx1, 0), np.maximum(ty1, 0)
    v = img.astype(int)
    p11, p12 = luts[ty1[:, None], tx1[None, :], v], luts[ty1[:, None], tx2[None, :], v]
    p21, p22 = luts[ty2[:, None], tx1[None, :], v], luts[ty2[:, None], tx2[None, :], v]
    res = (p11 * xa1[None, :] + p12 * xa[None, :]) * ya1[:, None] + (p21 * xa1[None, :] + p22 * xa[None, :]) * ya[:, None]
    return np.clip(np.rint(res.astype(np.float32)), 0, 255).astype(np.uint8)


def clahe_clipped_count(img, clip_limit, tiles):
    """Per tile, the number of pixels above the clip limit (what the redistribution spreads); for the tests' own checks of their cases."""
    tx, ty = tiles
    h, w = img.shape
    ext = img if (w % tx == 0 and h % ty == 0) else np.pad(img, ((0, ty - h % ty), (0, tx - w % tx)), mode="reflect")
    tw, th = ext.shape[1] // tx, ext.shape[0] // ty
    clip = max(int(clip_limit * tw * th / 256), 1) if clip_limit > 0 else 0
    out = np.zeros((ty, tx), np.int64)
    for j in range(ty):
        for i in range(tx):
            hist = np.bincount(ext[j * th:(j + 1) * th, i * tw:(i + 1) * tw].ravel(), minlength=256)
            out[j, i] = np.maximum(hist - clip, 0).sum() if clip > 0 else 0
    return out, clip


# ---- Tracking::undistort_point (src/Tracking.cc:1265-1283) ---------------------------------------------------------------
def undistort(pts, fx, fy, cx, cy, dist, fisheye=False):
    """cv::undistortPoints(pt, pt, K, D, noArray(), K) resp. cv::fisheye::undistortPoints(pt, pt, K, D, Mat(), K) of OpenCV 3.4.
    mK and mDistCoef are CV_32F: camera values and points are float32 widened to float64; all arithmetic is float64, in the expression
    order of csrc/klt.hip k_undistort; results are rounded to float32."""
    p = np.ascontiguousarray(pts, np.float32).reshape(-1, 2).astype(np.float64)
    fx, fy, cx, cy = (np.float64(np.float32(v)) for v in (fx, fy, cx, cy))
    k = np.zeros(8, np.float64)
    d = np.asarray(dist, np.float32).astype(np.float64)
    k[:len(d)] = d
    u, v = p[:, 0], p[:, 1]
    one = np.float64(1.0)
    with np.errstate(all="ignore"):
        if not fisheye:
            ifx, ify = one / fx, one / fy
            x, y = (u - cx) * ifx, (v - cy) * ify
            x0, y0 = x, y
            for _ in range(5):                                   # criteria (ITER, 5, 0.01): no epsilon test
                r2 = x * x + y * y
                icdist = (1 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2) / (1 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2)
                dx = 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x)
                dy = k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y
                x, y = (x0 - dx) * icdist, (y0 - dy) * icdist
            xx, yy = fx * x + 0. * y + cx, 0. * x + fy * y + cy   # the 3 x 3 product keeps its zero entries: 0 * inf is NaN
            ww = one / (0. * x + 0. * y + 1.)
            out = np.stack([xx * ww, yy * ww], 1)
        else:
            pwx, pwy = (u - cx) / fx, (v - cy) / fy
            theta_d = np.sqrt(pwx * pwx + pwy * pwy)
            half_pi = np.float64(3.1415926535897932384626433832795) / 2.
            theta_d = np.fmin(np.fmax(-half_pi, theta_d), half_pi)     # C fmin / fmax: a NaN operand yields the other one
            go = theta_d > 1e-8
            theta = theta_d.copy()
            active = go.copy()
            for _ in range(10):
                t2 = theta * theta
                t4 = t2 * t2
                t6 = t4 * t2
                t8 = t6 * t2
                a, b, c, e = k[0] * t2, k[1] * t4, k[2] * t6, k[3] * t8
                fix = (theta * (1 + a + b + c + e) - theta_d) / (1 + 3 * a + 5 * b + 7 * c + 9 * e)
                theta = np.where(active, theta - fix, theta)
                active = active & ~(np.abs(fix) < 1e-8)               # a NaN step never ends the loop
            scale = np.where(go, np.tan(theta) / theta_d, one)
            x, y = pwx * scale, pwy * scale
            pr0, pr1 = fx * x + 0. * y + cx * 1.0, 0. * x + fy * y + cy * 1.0
            pr2 = 0. * x + 0. * y + 1. * 1.0
            out = np.stack([pr0 / pr2, pr1 / pr2], 1)
        return out.astype(np.float32)


def fisheye_clamped(pts, fx, fy, cx, cy):
    """Which points the fisheye model clamps (|pw| > pi / 2)."""
    p = np.ascontiguousarray(pts, np.float32).reshape(-1, 2).astype(np.float64)
    fx, fy, cx, cy = (np.float64(np.float32(v)) for v in (fx, fy, cx, cy))
    with np.errstate(all="ignore"):
        return np.hypot((p[:, 0] - cx) / fx, (p[:, 1] - cy) / fy) > math.pi / 2


# ---- DBoW2 TemplatedVocabulary::transform (Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1125-1258) -----------------------
_POP = np.array([bin(i).count("1") for i in range(256)], np.int64)


def bow_descend(voc, feats, levelsup):
    """Per feature (leaf node, node id at level L - levelsup): the descent of :1207-1258, all features one level at a time."""
    cs, ch, de = np.asarray(voc["child_start"]), np.asarray(voc["children"]), np.asarray(voc["descriptor"], np.uint8)
    feats = np.ascontiguousarray(feats, np.uint8).reshape(-1, 32)
    n = len(feats)
    nid_level = int(voc["L"]) - int(levelsup)
    cur = np.zeros(n, np.int64)
    nid = np.full(n, 0 if nid_level <= 0 else -1, np.int64)
    level = 0
    moving = np.arange(n)
    while len(moving):
        moving = moving[cs[cur[moving] + 1] > cs[cur[moving]]]          # isLeaf ends the descent
        if not len(moving):
            break
        level += 1
        for node in np.unique(cur[moving]):
            who = moving[cur[moving] == node]
            kids = ch[cs[node]:cs[node + 1]]
            dists = _POP[feats[who][:, None, :] ^ de[kids][None, :, :]].sum(-1)
            cur[who] = kids[np.argmin(dists, axis=1)]                     # argmin: the first minimum, as `d < best_d` keeps it
        if level == nid_level:
            nid[moving] = cur[moving]
    nid = np.where(nid < 0, cur, nid)                                      # the descent ended above that level: the leaf (uvo.h)
    return cur, nid


def bow_transform(voc, feats, levelsup, descent=None):
    """-> (word_id, weight, node_id, (BowVector ids, values), {node: [features]}), the form of oracle_lib.Oracle.bow_transform.
    descent: a bow_descend() result to reuse (it does not depend on the weighting or the normalisation)."""
    leaf, nid = bow_descend(voc, feats, levelsup) if descent is None else descent
    wid = np.asarray(voc["word_id"], np.int32)[leaf]
    ww = np.asarray(voc["weight"], np.float64)[leaf]
    weighting, normalize = int(voc["weighting"]), int(voc["normalize"])
    tf = weighting in (0, 1)
    bow, fv = {}, {}
    for i in range(len(leaf)):
        w = float(ww[i])
        if not w > 0:
            continue                                                       # a stopped word: in neither container
        key = int(np.uint32(wid[i]))
        if tf:
            bow[key] = bow[key] + w if key in bow else w                   # BowVector::addWeight
        elif key not in bow:
            bow[key] = w                                                   # addIfNotExist
        fv.setdefault(int(np.uint32(nid[i])), []).append(i)
    ids = sorted(bow)
    vals = [bow[i] for i in ids]
    if tf and ids and normalize == 0:
        nd = float(len(ids))
        vals = [v / nd for v in vals]
    if normalize != 0:                                                     # BowVector::normalize: the sum runs in ascending id order
        norm = 0.0
        if normalize == 1:
            for v in vals:
                norm += abs(v)
        else:
            for v in vals:
                norm += v * v
            norm = math.sqrt(norm)
        if norm > 0.0:
            vals = [v / norm for v in vals]
    return wid, ww, nid.astype(np.int32), (np.asarray(ids, np.uint32), np.asarray(vals, np.float64)), {k: fv[k] for k in sorted(fv)}


# ---- haloc::Hash::getHash (src/hash.cpp:57-85) ---------------------------------------------------------------------------
def haloc_hash(proj, desc):
    """proj [num_proj][>= n] float32, desc [n][32] uint8 -> hash [num_proj * 32] float32: one float32 accumulator per (projection,
    column), updated row by row, product and sum each rounded to float32; then the division by float32(n).  Zeros for n == 0."""
    proj = np.asarray(proj, np.float32)
    desc = np.asarray(desc, np.uint8).reshape(-1, 32)
    n = len(desc)
    acc = np.zeros((proj.shape[0], 32), np.float32)
    if n == 0:
        return acc.reshape(-1)
    d = desc.astype(np.float32)
    with np.errstate(all="ignore"):
        for m in range(n):
            acc = acc + proj[:, m, None] * d[m]
        return (acc / np.float32(n)).reshape(-1)


# ---- how the two test modules compare results --------------------------------------------------------------------------
def same_floats(a, b, bits):
    """Raw bits, except that a NaN equals any NaN."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    na, nb = np.isnan(a), np.isnan(b)
    return bool((na == nb).all() and (a.view(bits)[~na] == b.view(bits)[~nb]).all())


def same_bow(g, o):
    """Two results in the form of Oracle.bow_transform: ids exact, weights and BowVector values on their bits."""
    return (np.array_equal(g[0], o[0]) and np.array_equal(np.asarray(g[1]).view(np.uint64), np.asarray(o[1]).view(np.uint64)) and
            np.array_equal(g[2], o[2]) and np.array_equal(g[3][0], o[3][0]) and g[3][0].dtype == o[3][0].dtype and
            np.array_equal(np.asarray(g[3][1]).view(np.uint64), np.asarray(o[3][1]).view(np.uint64)) and g[4] == o[4])
