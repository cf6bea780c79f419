"""The inputs of tests/test_gpu_describe.py, shared with tests/test_describe_model.py, which shows on the oracle alone that they reach
what they are aimed at.  A case is (name, image, caller keypoints); every case is a top-up call with a grid of all ones and
num_featsneeded = 0, so the caller keypoints are all that comes back.  Images are 160 x 96 and 96 x 160: w + 32 is a multiple of 64
once each way, the shape at which the last tile column of a border keypoint's window equals the plane's tile count per row."""
import functools

import numpy as np

from oracle_lib import KP

SHAPES = ((160, 96), (96, 160))           # (w, h)
CFG = (300, 1.2, 3, 20)                   # nfeatures, scaleFactor, nlevels, fastTh


def cfg(w, h):
    """The extractor of a shape.  96 x 160 has two levels: its level 2 (67 x 111) has a detection window of 41 x 85, for which
    DistributeOctTree's nIni = round(41 / 85) is 0 and the reference divides by it (the library refuses such a geometry)."""
    return CFG if w >= h else CFG[:2] + (2,) + CFG[3:]
IN_CAP = 1200                             # the 33 x 33 centres of the orientation cases and some room
MIN_PX = 20


def keypoints(xy):
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    k = np.zeros(len(xy), KP)
    k["x"], k["y"] = xy[:, 0], xy[:, 1]
    k["size"], k["angle"], k["octave"] = 31, -1, 0
    k["response"], k["class_id"] = np.arange(len(xy)) % 97, np.arange(len(xy))
    return k


def ones_grid(w, h):
    return np.ones((h // MIN_PX + 2, w // MIN_PX + 2), np.int32, order="F")


def noise(seed, w, h):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def _cross(xs, ys):
    return [(x, y) for y in ys for x in xs]


def border_centres(w, h):
    """Every integer centre with cx in {2..19} u {w-20..w-3} crossed with a handful of cy, the transpose, the four corners among them."""
    bx, by = list(range(2, 20)) + list(range(w - 20, w - 2)), list(range(2, 20)) + list(range(h - 20, h - 2))
    some_y, some_x = [2, 3, 9, 13, 14, 40, h // 2, h - 15, h - 10, h - 3], [2, 3, 9, 13, 14, 40, w // 2, w - 15, w - 10, w - 3]
    return sorted(set(_cross(bx, some_y) + _cross(some_x, by)))


def tile_phase_centres(w, h):
    """A 16 x 8 block of integer centres in the interior and one touching each border band: every (x0 & 15, y0 & 7) of the window corner."""
    blocks = [(64, 40), (2, 40), (w - 18, 40), (40, 2), (40, h - 10)]
    return [(x0 + i, y0 + j) for x0, y0 in blocks for j in range(8) for i in range(16)]


def window_tiles(cx, cy):
    """k_describe's tile arithmetic for a centre: (x0 & 15, y0 & 7, tile columns, tile rows) of its blurred window."""
    x0, y0 = cx + 16 - 18, cy + 16 - 18
    return x0 & 15, y0 & 7, ((x0 + 39) >> 4) - (x0 >> 4) + 1, ((y0 + 36) >> 3) - (y0 >> 3) + 1


def rounding_values(n):
    """Accepted coordinates along an axis of length n at the rounding boundaries of the centre (float32)."""
    f = np.float32
    v = []
    for k in (40, 41):                                    # k + 0.5 rounds to the even neighbour; its float neighbours round to k / k + 1
        t = f(k + 0.5)
        v += [t, np.nextafter(t, f(0)), np.nextafter(t, f(1e9))]
    # (k + 0.49999997 and k + 0.50000006 as float32 sums round back to the tie for every k >= 1: the neighbours above are what they mean)
    v += [f(1.5), np.nextafter(f(1.5), f(1e9)), f(2.5), np.nextafter(f(2.5), f(1e9))]
    v += [np.nextafter(f(n - 2.5), f(0)), f(n - 3), f(n - 3.5)]    # the largest accepted float, the last centre, the tie below it
    return np.array(v, np.float32)


def rejected_values(n):
    """The first rejected coordinate on each side: rounds to 1, rounds to n - 2."""
    return np.array([np.nextafter(np.float32(1.5), np.float32(0)), np.float32(n - 2.5)], np.float32)


def _centre(w, h):
    return w // 2, h // 2


def _around(w, h, r):
    cx, cy = _centre(w, h)
    return [(cx + i, cy + j) for j in range(-r, r + 1) for i in range(-r, r + 1)]


def orientation_cases(w, h):
    """(name, image, centres): single pixels, pixel pairs, a point-symmetric patch and half-planes, seen from the centres around them."""
    cx, cy = _centre(w, h)
    out = []
    for val in (255, 1):
        img = np.zeros((h, w), np.uint8)
        img[cy, cx] = val
        out.append(("pixel%d" % val, img, _around(w, h, 16)))       # the centre at offset (-u, -v) sees the pixel at (u, v)
    for name, second in (("pair_plus", (cx, cy + 5)), ("pair_minus", (cx, cy - 5))):
        img = np.zeros((h, w), np.uint8)
        img[cy, cx + 5] = 200
        img[second[1], second[0]] = 200                             # from (cx, cy): m10 = 1000, m01 = +-1000
        out.append((name, img, _around(w, h, 6)))
    sym = noise(5, w, h)
    patch = sym[cy - 15:cy + 16, cx - 15:cx + 16]
    patch[:] = patch // 2 + patch[::-1, ::-1] // 2                  # the 31 x 31 patch of (cx, cy), point-symmetric about it: both moments 0
    assert patch.min() != patch.max()
    out.append(("symmetric", sym, _around(w, h, 1)))
    yy, xx = np.mgrid[0:h, 0:w]
    for name, mask in (("half_x+", xx >= cx), ("half_x-", xx <= cx), ("half_y+", yy >= cy), ("half_y-", yy <= cy),
                       ("half_d1+", (xx - cx) + (yy - cy) >= 0), ("half_d1-", (xx - cx) + (yy - cy) <= 0),
                       ("half_d2+", (xx - cx) - (yy - cy) >= 0), ("half_d2-", (xx - cx) - (yy - cy) <= 0)):
        out.append((name, np.where(mask, 255, 0).astype(np.uint8), _around(w, h, 2)))
    return out


def gradient_image(w, h, direction, of=16, slope=0.55):
    """I = clip(round(a x + b y + c)): neighbouring samples differ by at most one grey level, the gradient points along `direction`."""
    th = 2 * np.pi * direction / of
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    return np.clip(np.rint(slope * np.cos(th) * (xx - w / 2) + slope * np.sin(th) * (yy - h / 2) + 128), 0, 255).astype(np.uint8)


def tie_cases(w, h):
    pts = [(2, 2), (w - 3, h - 3), (2, h - 3), (w - 3, 2)] + _around(w, h, 1)
    out = [("const%d" % v, np.full((h, w), v, np.uint8), pts) for v in (0, 128, 255)]
    grid = [(x, y) for y in (24, h // 2, h - 25) for x in (24, w // 2 - 7, w // 2 + 8, w - 25)] + [(2, 2), (w - 3, h - 3)]
    out += [("gradient%02d" % d, gradient_image(w, h, d), grid) for d in range(16)]
    return out


@functools.lru_cache(maxsize=None)
def plain_cases():
    """Cases 2, 4 and 5 (and the accepted half of 3): (name, image, keypoints), both shapes."""
    out = []
    for w, h in SHAPES:
        tag = "%dx%d/" % (w, h)
        out.append((tag + "tile_phases", noise(31 + w, w, h), keypoints(tile_phase_centres(w, h))))
        rx, ry = rounding_values(w), rounding_values(h)
        xy = [(x, np.float32(h // 2 + 0.25)) for x in rx] + [(np.float32(w // 2 - 0.25), y) for y in ry] + list(zip(rx, ry))
        out.append((tag + "rounding", noise(37 + w, w, h), keypoints(xy)))
        for name, img, pts in orientation_cases(w, h) + tie_cases(w, h):
            out.append((tag + name, img, keypoints(pts)))
    return out


@functools.lru_cache(maxsize=None)
def border_case(w, h):
    """Case 1: (the image, another noise image of the same size, the keypoints of the border bands)."""
    return noise(11 + w, w, h), noise(12 + w, w, h), keypoints(border_centres(w, h))


# ---- case 6: group shapes.  Frames of one shape; per call the frames' caller keypoint counts ----
GROUP_SHAPE = (160, 96)
GROUP_CALLS = [(n,) for n in (0, 1, 2, 3, 4, 5, 7)] + [(5, 7), (0, 3)] + [(0, 1, 2, 4, 7)]   # batches of 1, 2 and 5
GROUP_NEED = 1000
GROUP_MIN_PX = 5                          # cells small enough that levels 1 and 2 still find free ones behind level 0


@functools.lru_cache(maxsize=None)
def group_frames(synth):
    """Five corner-rich frames (synth: the package's frame generator) and seven caller keypoints each, border positions among them; a call
    takes the first n_in of a frame's."""
    w, h = GROUP_SHAPE
    rng = np.random.default_rng(61)
    frames = [synth.make_frame(70 + i, w, h, n_shapes=60) for i in range(5)]
    kps = []
    for i in range(5):
        xy = np.stack([rng.uniform(1.5, w - 2.6, 7), rng.uniform(1.5, h - 2.6, 7)], 1).astype(np.float32)
        xy[0] = (2, 2 + i)
        xy[1] = (w - 3 - i, h - 3)
        kps.append(keypoints(xy))
    return frames, kps
