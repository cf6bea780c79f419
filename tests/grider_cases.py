"""The inputs of tests/test_gpu_grider.py, shared with tests/test_grider_model.py, which shows on the CPU that each of them holds the edge
it is named for.  Every image fits a 320 x 256 handle by area; nothing here needs a GPU or the oracle.

Why these (csrc/grider.hip):
  partial blocks      k_grid_score works in blocks of 64 x 4 pixels: 67 x 61 leaves a partial block in both directions
  leftover strips     the grid does not divide the image: the last column and the last two rows belong to no ROI
  more ROIs           w mod grid_x >= w / grid_x: floor(w / size_x) > grid_x, so there are more ROIs than grid cells (and the quota, which
                      divides by the grid cells, is handed to each of them)
  smallest interior   7 x 7 ROIs: one interior pixel each, all of its neighbours outside the interior
  no interior         ROIs below 7 px in one direction (the product of the interior's sides is <= 0) and in both (it is positive: the
                      defect k_grid_select had); each runs behind a call that leaves non-zero scores in the plane
  clamps              thresholds below 0, at 0 (score-0 corners exist: they are corners, and never survive NMS) and at 1
  saturated           strength 255 is stored in the uint8 plane as it is; thresholds 254, 255 and above
  ties                every corner has the same response and the cut runs through them: only the declared order decides
  num_features = 0    one point per ROI
  wider               wider than max_width, within the handle's area
  more points         quota x ROIs exceeds num_features + grid cells + 64, what the Python binding once sized its buffer by"""
import collections
import functools

import numpy as np

import grider_model as gm

HANDLE_W, HANDLE_H = 320, 256
# the GPU test's handle: (nfeatures, scaleFactor, nlevels, max_batch).  k_grid_select borrows the FAST stage's count scratch, which grows
# with the batch: with max_batch = 1 a handle of this size refuses more than 127 ROIs, and the 3 x 3 case has 441
HANDLE_CFG = (1000, 1.2, 1, 32)

# fill: the call made on the handle right in front of the case (None: whatever the previous case left)
Case = collections.namedtuple("Case", "name image num_features grid_x grid_y threshold nms fill")


def noise(seed, w, h, lo=0, hi=256):
    return np.random.default_rng(seed).integers(lo, hi, (h, w), dtype=np.uint8)


def dots(w, h):
    """255 at every (4 i, 4 j) on 0: each dot has strength 255, nothing else is a corner at any threshold >= 0."""
    img = np.zeros((h, w), np.uint8)
    img[::4, ::4] = 255
    return img


@functools.lru_cache(maxsize=None)
def fills():
    """The calls that leave known non-zero scores in the handle's plane: every dot of the interior is a corner, nms off.
    'full' is the handle's whole area; 'small' is 64 wide, so that the rows right behind a 32 x 32 or 16 x 16 image's plane (rows 16 and 4
    of this one) hold dots too -- behind those the full-width fill has only its rows 3 and 0, which hold none."""
    return {"full": Case("fill 320 x 256", dots(HANDLE_W, HANDLE_H), 50, 1, 1, 20, False, None),
            "small": Case("fill 64 x 64", dots(64, 64), 50, 1, 1, 20, False, None)}


# (w, h, grid_x, grid_y): ROIs of 6 x 6, 4 x 40, 4 x 4, 3 x 3, 2 x 2, 1 x 1
NO_INTERIOR = [(60, 60, 10, 10), (64, 80, 16, 2), (64, 64, 16, 16), (63, 63, 21, 21), (32, 32, 16, 16), (16, 16, 16, 16)]


@functools.lru_cache(maxsize=None)
def cases():
    c = [Case("partial blocks", noise(11, 67, 61), 40, 2, 2, 20, True, None),
         # (there the partial block, columns 64 .. 66, lies outside every interior; here one ROI's interior runs through it.  A partial
         # block of rows is at most 3 rows high, so it never holds an interior pixel)
         Case("corners in a partial block", noise(19, 75, 62), 100, 1, 1, 20, True, None),
         Case("leftover strips", noise(12, 100, 90), 60, 3, 4, 20, True, None),
         Case("more ROIs than grid cells", noise(13, 89, 88), 250, 10, 10, 15, False, None),
         Case("smallest interior", noise(14, 71, 64), 90, 10, 9, 10, True, None)]
    for i, (w, h, gx, gy) in enumerate(NO_INTERIOR):
        c.append(Case("no interior %d x %d" % (w // gx, h // gy), noise(20 + i, w, h), 100, gx, gy, 20, False, "full"))
    for w, h, gx, gy in NO_INTERIOR[4:]:
        c.append(Case("no interior %d x %d behind the small fill" % (w // gx, h // gy), noise(30 + w, w, h), 100, gx, gy, 20, False, "small"))
    flat = noise(15, 64, 64, 100, 104)
    c += [Case("clamps t=-5", flat, 300, 1, 1, -5, True, None),
          Case("clamps t=0", flat, 300, 1, 1, 0, True, None),
          Case("clamps t=0 nms off", flat, 300, 1, 1, 0, False, None),
          Case("clamps t=1", flat, 300, 1, 1, 1, True, None)]
    c += [Case("saturated t=%d" % t, dots(64, 64), 100, 2, 2, t, True, None) for t in (254, 255, 300)]
    c += [Case("ties at the cut" + ("" if nms else " nms off"), dots(96, 80), 20, 2, 2, 20, nms, None) for nms in (True, False)]
    c += [Case("num_features = 0", noise(16, 80, 70), 0, 3, 2, 20, True, None),
          Case("wider than max_width", noise(17, 400, 200), 200, 7, 3, 25, True, None),
          # 11 ROIs of 8 x 200 against 10 grid cells, 71 points each: more than num_features + grid cells + 64 come out
          Case("more points than num_features + cells + 64", noise(18, 89, 200), 700, 10, 1, 10, False, None)]
    assert len({k.name for k in c}) == len(c)
    return c


def by_name(name):
    return next(k for k in cases() if k.name == name)


@functools.lru_cache(maxsize=None)
def expected(name):
    """The model's records for a case or a fill, computed once."""
    k = fills()[name] if name in fills() else by_name(name)
    return gm.grider_fast(k.image, k.num_features, k.grid_x, k.grid_y, k.threshold, k.nms)


def handle_capacities(max_batch=HANDLE_CFG[3]):
    """(pixels, ROIs, ROIs x quota) that uvo_grider_fast accepts on the test's handle, from csrc/extractor_geom.cpp run on the host
    (tests/emu/grider_geom_emu.cpp)."""
    import ctypes
    import host_build
    lib = ctypes.CDLL(host_build.build("grider_geom_emu"))
    lib.emu_grider_capacities.argtypes = [ctypes.c_int, ctypes.c_float] + [ctypes.c_int] * 4 + [ctypes.c_void_p]
    out = (ctypes.c_longlong * 3)()
    rc = lib.emu_grider_capacities(HANDLE_CFG[0], HANDLE_CFG[1], HANDLE_CFG[2], HANDLE_W, HANDLE_H, max_batch, ctypes.addressof(out))
    assert rc == 0
    return tuple(out)


def plane_after(k):
    """What k_grid_score leaves for a call, as the flat w * h bytes at the start of the handle's plane: the strength (score + 1) of every
    corner inside a ROI's interior, 0 elsewhere."""
    h, w = k.image.shape
    size_x, size_y, ct_cols, ct_rows = gm.geometry(w, h, k.grid_x, k.grid_y)
    S = gm.strength(k.image)
    t = min(max(k.threshold, 0), 255)
    plane = np.zeros((h, w), np.uint8)
    if size_x > 6 and size_y > 6:
        for ry in range(ct_rows):
            for rx in range(ct_cols):
                win = (slice(ry * size_y + 3, (ry + 1) * size_y - 3), slice(rx * size_x + 3, (rx + 1) * size_x - 3))
                plane[win] = np.where(S[win] > t, S[win], 0)
    return plane.reshape(-1)


def unguarded_reads(w, h, grid_x, grid_y):
    """The linear plane indices that pass 0 of k_grid_select read at its centre pixel before it tested the sign of the interior's sides:
    i < iw * ih with lx = 3 + i % iw, ly = 3 + i / iw in C's truncating arithmetic."""
    size_x, size_y, ct_cols, ct_rows = gm.geometry(w, h, grid_x, grid_y)
    iw, ih = size_x - 6, size_y - 6
    trunc_div = lambda a, b: int(a / b) if b else 0
    idx = []
    for r in range(ct_cols * ct_rows):
        x0, y0 = r % ct_cols * size_x, r // ct_cols * size_y
        for i in range(max(iw * ih, 0)):
            q = trunc_div(i, iw)
            lx, ly = 3 + (i - q * iw), 3 + q
            idx.append(((y0 + ly) * w + x0 + lx, y0 + ly))
    return np.array(idx, np.int64).reshape(-1, 2).T       # the indices, and the y of the key point a non-zero byte there became
