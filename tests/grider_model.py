"""Grider_FAST::perform_griding (include/Grider_FAST.h:81-137) stated in numpy from the definition of FAST-9/16, for
tests/test_grider_model.py (which ties it to the C++ oracle) and tests/test_gpu_grider.py (which holds uvo_grider_fast to it).  It shares
no code with oracle/orb_oracle.cpp: the ring is derived from the circle, the strength is computed for whole planes at once, and the
selection is a sort.

  strength(p)  = max over the 16 arcs of 9 contiguous ring pixels of  max(min(ring - p), min(p - ring))
  corner       : strength > t, t clamped to 0 .. 255;  score = strength - 1 (the largest threshold at which p still is a corner)
  NMS          : a corner stays iff its score is strictly above all 8 neighbours'; a non-corner counts as 0, and so does every pixel
                 outside the ROI's 3-pixel-inset interior (cv::FAST sees the ROI alone)
  per ROI      : response descending, then y, then x (the declared tie-break); the first num_features / (grid_x * grid_y) + 1
  ROIs         : size = (w / grid_x, h / grid_y); floor(w / size_x) x floor(h / size_y) of them, row-major; shifted by the ROI origin

A pixel's strength needs the pixel and its ring only, and the ring of an interior pixel lies inside the ROI, so the strength plane is
computed once for the whole image; what makes cv::FAST on a ROI differ from cv::FAST on the image is the interior and the NMS.

`mutant` names one deliberate mistake (MUTANTS); tests/test_grider_model.py shows that the committed cases tell each from the model."""
import numpy as np

KEYPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"),
                           ("class_id", "<i4")])

MUTANTS = ("global_nms", "nms_ge", "corner_ge", "ties_x_then_y", "keep_without_plus_one", "rois_from_grid", "inset_2", "threshold_unclamped",
           "response_is_strength")


def ring():
    """The 16 (dx, dy) of the radius-3 circle -- the lattice points whose distance from the centre rounds to 3 -- in the order of the angle."""
    pts = [(dx, dy) for dy in range(-4, 5) for dx in range(-4, 5) if round(float(np.hypot(dx, dy))) == 3]
    assert len(pts) == 16
    return sorted(pts, key=lambda p: np.arctan2(p[1], p[0]))


def strength(img):
    """The FAST-9/16 strength of every pixel, int32; the image is edge-padded by 3, which only the `inset_2` mutant ever looks at."""
    img = np.asarray(img)
    h, w = img.shape
    p = np.pad(img.astype(np.int32), 3, mode="edge")
    d = np.stack([p[3 + dy:3 + dy + h, 3 + dx:3 + dx + w] for dx, dy in ring()]) - p[3:3 + h, 3:3 + w]
    dd = np.concatenate([d, d[:8]])                                     # arcs wrap round the ring
    best = None
    for s in range(16):
        arc = dd[s:s + 9]
        m = np.maximum(arc.min(0), (-arc).min(0))                      # all nine brighter by at least m, or all nine darker
        best = m if best is None else np.maximum(best, m)
    return best


def _score_plane(S, x0, y0, x1, y1, t, inset, mutant):
    """Scores (0 = no corner) and corner flags of the whole image, for the corners inside the `inset` border of the window [x0, x1) x [y0, y1)."""
    score, corner = np.zeros(S.shape, np.int32), np.zeros(S.shape, bool)
    if x1 - x0 > 2 * inset and y1 - y0 > 2 * inset:
        win = (slice(y0 + inset, y1 - inset), slice(x0 + inset, x1 - inset))
        s = S[win]
        c = s >= t if mutant == "corner_ge" else s > t
        corner[win] = c
        score[win] = np.where(c, s if mutant == "response_is_strength" else s - 1, 0)
    return score, corner


def _strict_maximum(score, mutant):
    """True where a pixel's score is above (not below, for the mutant) all 8 neighbours', the plane continued by 0."""
    h, w = score.shape
    p = np.pad(score, 1)
    keep = np.ones(score.shape, bool)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx or dy:
                n = p[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
                keep &= score >= n if mutant == "nms_ge" else score > n
    return keep


def _threshold(t, mutant):
    return t if mutant == "threshold_unclamped" else min(max(t, 0), 255)


def roi_points(S, x0, y0, size_x, size_y, threshold, nms, mutant=None):
    """cv::FAST on the ROI at (x0, y0): rows (x, y, response) in ROI coordinates, row-major.  S is the image's strength plane."""
    t = _threshold(threshold, mutant)
    inset = 2 if mutant == "inset_2" else 3
    score, corner = _score_plane(S, x0, y0, x0 + size_x, y0 + size_y, t, inset, mutant)
    if nms:
        seen = score
        if mutant == "global_nms":          # the neighbours as cv::FAST on the whole image would see them
            seen = _score_plane(S, 0, 0, S.shape[1], S.shape[0], t, inset, mutant)[0]
        keep = corner & _strict_maximum(seen, mutant)
    else:
        keep = corner
    ys, xs = np.nonzero(keep)
    return np.stack([xs - x0, ys - y0, score[ys, xs]], 1).astype(np.int64).reshape(-1, 3)


def records(rows):
    out = np.zeros(len(rows), KEYPOINT_DTYPE)
    if len(rows):
        rows = np.asarray(rows)
        out["x"], out["y"], out["response"] = rows[:, 0], rows[:, 1], rows[:, 2]
    out["size"], out["angle"], out["octave"], out["class_id"] = 7, -1, 0, -1
    return out


def fast(img, threshold, nms=True, mutant=None):
    """cv::FAST(img, threshold, nms), type 9_16: KEYPOINT_DTYPE records, row-major."""
    h, w = np.asarray(img).shape
    return records(roi_points(strength(img), 0, 0, w, h, threshold, nms, mutant))


def geometry(w, h, grid_x, grid_y, mutant=None):
    """(size_x, size_y, ct_cols, ct_rows)"""
    size_x, size_y = w // grid_x, h // grid_y
    assert size_x > 0 and size_y > 0, "the reference asserts size > 0"
    if mutant == "rois_from_grid":
        return size_x, size_y, grid_x, grid_y
    return size_x, size_y, w // size_x, h // size_y


def keep_per_roi(num_features, grid_x, grid_y, mutant=None):
    return num_features // (grid_x * grid_y) + (0 if mutant == "keep_without_plus_one" else 1)


def grider_fast(img, num_features, grid_x, grid_y, threshold, nms=True, mutant=None):
    """Grider_FAST::perform_griding: KEYPOINT_DTYPE records, ROI-major."""
    assert mutant is None or mutant in MUTANTS
    img = np.asarray(img)
    h, w = img.shape
    size_x, size_y, ct_cols, ct_rows = geometry(w, h, grid_x, grid_y, mutant)
    keep = keep_per_roi(num_features, grid_x, grid_y, mutant)
    S = strength(img)
    out = []
    for r in range(ct_cols * ct_rows):
        x0, y0 = r % ct_cols * size_x, r // ct_cols * size_y
        pts = roi_points(S, x0, y0, size_x, size_y, threshold, nms, mutant).tolist()
        pts.sort(key=(lambda p: (-p[2], p[0], p[1])) if mutant == "ties_x_then_y" else (lambda p: (-p[2], p[1], p[0])))
        out += [(x + x0, y + y0, s) for x, y, s in pts[:keep]]
    return records(out)
