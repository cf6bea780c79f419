"""The case lists of tests/test_side_model.py (model against oracle, CPU) and tests/test_gpu_side.py (kernels against model): inputs
only, built from fixed seeds, so that both modules run the same cases.  Shapes stay small: no image above 128 x 96, no point set above
a few hundred, no vocabulary above a few thousand nodes."""
import numpy as np

# ---- CLAHE ---------------------------------------------------------------------------------------------------------------
CLAHE_MAX_W, CLAHE_MAX_H, CLAHE_MAX_BATCH = 128, 96, 3
CLAHE_GEOMETRIES = [            # (w, h, tiles)
    (96, 64, (8, 8)),           # both divide
    (8, 8, (8, 8)),             # one-pixel tiles
    (97, 61, (4, 4)),           # neither divides
    (96, 61, (4, 4)),           # the width divides and is still padded by a full `tiles` (the copyMakeBorder quirk)
    (97, 64, (4, 4)),           # the same for the height
    (128, 96, (1, 1)),          # a single tile of 12 288 pixels: redistBatch > 0
    (44, 30, (7, 4)),
    (48, 40, (16, 2)),
    (24, 16, (8, 4)),           # 12-pixel tiles: the clip limit clamps to 1
]
CLAHE_CLIPS = [0.0, 0.01, 4.0, 40.0, 1000.0]
CLAHE_IMAGES = ["uniform", "bimodal", "flat0", "flat255", "ramp", "skewed"]


def clahe_image(kind, w, h, seed=0):
    rng = np.random.default_rng(1000 + seed)
    if kind == "uniform":
        return rng.integers(0, 256, (h, w), dtype=np.uint8)
    if kind == "bimodal":
        return np.where(rng.random((h, w)) < 0.5, 0, 255).astype(np.uint8)
    if kind == "flat0":
        return np.zeros((h, w), np.uint8)
    if kind == "flat255":
        return np.full((h, w), 255, np.uint8)
    if kind == "ramp":
        return ((np.arange(w)[None, :] * 3 + np.arange(h)[:, None] * 7) % 256).astype(np.uint8)
    if kind == "skewed":
        return (rng.integers(0, 256, (h, w)) * rng.random((h, w)) ** 2).astype(np.uint8)
    raise ValueError(kind)


def clahe_cases():
    """(name, image, clip limit, tiles): every geometry x clip limit x image kind."""
    for gi, (w, h, tiles) in enumerate(CLAHE_GEOMETRIES):
        for clip in CLAHE_CLIPS:
            for ki, kind in enumerate(CLAHE_IMAGES):
                yield "%dx%d/%s clip %g %s" % (w, h, tiles, clip, kind), clahe_image(kind, w, h, 10 * gi + ki), clip, tiles


# the residual classes of the redistribution: `clipped` = q * 256 + r; r decides the step 256 / r of the strided residual
RESIDUALS = [1, 2, 3, 85, 86, 127, 128, 129, 255]
RESIDUAL_GEOMETRIES = [          # (w, h, clip limit, the limit in pixels per bin): one tile each
    (128, 96, 4.0, 192),         # 12 288 pixels; lutScale ~ 1 / 48
    (16, 16, 8.0, 8),            # 256 pixels: lutScale ~ 1, so every single count of the redistribution moves the LUT
]


def residual_image(w, h, limit, clipped, seed):
    """One tile whose histogram has exactly `clipped` pixels above `limit`, all of them in bin 7; every other bin stays below."""
    rng = np.random.default_rng(2000 + seed)
    total = w * h
    rest = total - (limit + clipped)
    assert rest >= 0
    others = np.delete(np.arange(256), 7)
    counts = rng.multinomial(rest, np.full(255, 1 / 255.))
    assert counts.max() < limit
    px = np.concatenate([np.full(limit + clipped, 7), np.repeat(others, counts)]).astype(np.uint8)
    rng.shuffle(px)
    return px.reshape(h, w)


def residual_cases():
    """(name, image, clip limit, limit in pixels, clipped count)."""
    for gi, (w, h, clip, limit) in enumerate(RESIDUAL_GEOMETRIES):
        for r in RESIDUALS:
            for q in (0, 1):
                clipped = q * 256 + r
                if limit + clipped > w * h:
                    continue
                yield "%dx%d clipped %d" % (w, h, clipped), residual_image(w, h, limit, clipped, 1000 * gi + clipped), clip, limit, clipped


# ---- undistortion --------------------------------------------------------------------------------------------------------
KLT_MAX_POINTS = 192
VIORB = (458.654, 457.296, 367.215, 248.375, [-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05], False)        # Data/Settings_VIORB.yaml
HARBOR = (413.32595366596017, 413.70198739483686, 305.9507483284928, 259.4439948946375,                             # Settings_VI_Aqualoc_harbor.yaml
          [-0.06125568297136998, -0.003796743395135256, 0.027326634771204592, -0.030296403142887066], True)
CAMERAS = {                      # name -> (fx, fy, cx, cy, dist, fisheye)
    "viorb": VIORB,
    "harbor_fisheye": HARBOR,
    "pinhole8": (458.654, 457.296, 367.215, 248.375, [-0.28, 0.07, 2e-4, 1e-5, 0.01, 0.02, -0.01, 0.003], False),
    "pinhole6_negative_fy": (458.654, -457.296, 367.215, 248.375, [-0.28, 0.07, 2e-4, 1e-5, 0.01, 0.02], False),
    "pinhole_none": (300.0, 300.0, 320.0, 256.0, [], False),
    "fisheye_none": (300.0, 300.0, 320.0, 256.0, [], True),
    "fisheye1": (300.0, 300.0, 320.0, 256.0, [0.1], True),
    "fisheye_unsettled": (300.0, 300.0, 320.0, 256.0, [-0.9, 0.5, -2.0, 1.0], True),      # its Newton steps do not settle
    "fisheye_origin": (300.0, 300.0, 0.0, 0.0, [0.1], True),                               # (1e-6, 0): theta_d <= 1e-8 off the principal point
    # theta_d between 1e-8 and 1e-6 only shows in float32 when k1 * theta^2 is above 1e-7: a coefficient no lens has, but a legal input
    "fisheye_origin_huge_k1": (300.0, 300.0, 0.0, 0.0, [1e7], True),
}
UNDISTORT_COUNTS = [1, 255, 256, 257, 2 * KLT_MAX_POINTS]


def undistort_points():
    """2 * max_points points: the special ones first, then uniform in +-3000 px.  A prefix of any length is a case."""
    rng = np.random.default_rng(3000)
    nan, inf = np.nan, np.inf
    special = [[0.5, -0.25],                                          # (the one-point case)
               [VIORB[2], VIORB[3]], [HARBOR[2], HARBOR[3]], [320.0, 256.0], [0.0, 0.0],
               [1e-6, 0.0], [0.0, -1e-6], [3e-6, 0.0], [1e-5, 2e-5], [1e-4, 0.0], [2e-4, -1e-4], [2.9e-4, 0.0],
               [nan, 10.0], [10.0, nan], [nan, nan], [inf, 10.0], [10.0, inf], [-inf, 10.0], [10.0, -inf], [inf, -inf], [nan, inf]]
    pts = np.stack([rng.uniform(-3000, 3000, 2 * KLT_MAX_POINTS), rng.uniform(-3000, 3000, 2 * KLT_MAX_POINTS)], 1).astype(np.float32)
    pts[:len(special)] = np.asarray(special, np.float32)
    # some inside an ordinary image as well, where the pin-hole iteration converges
    pts[40:120] = np.stack([rng.uniform(-20, 772, 80), rng.uniform(-20, 500, 80)], 1).astype(np.float32)
    return pts


# ---- BoW transform -------------------------------------------------------------------------------------------------------
BRANCHINGS = [[], [1], [2, 2], [16, 3], [17, 2], [33, 5], [100], [3, 1, 40], [10, 10, 10]]
BOW_COUNTS = [0, 1, 3, 4, 5, 15, 16, 17, 130]
WEIGHTINGS = [0, 1, 2, 3]         # TF_IDF, TF, IDF, BINARY
NORMALIZES = [0, 1, 2]            # none, L1, L2


def bow_levelsups(L):
    return [-1, 0, 1, L, L + 2]


def _flips(rng, base, p):
    return np.packbits(np.unpackbits(base) ^ (rng.random(256) < p).astype(np.uint8))


def _finish(desc, children, level, L, weight=None, rng=None, stop=0.05):
    n = len(desc)
    child_start = np.zeros(n + 1, np.int32)
    flat = []
    for i in range(n):
        flat.extend(children[i])
        child_start[i + 1] = len(flat)
    word_id = np.full(n, -1, np.int32)
    leaves = [i for i in range(n) if not children[i]]
    word_id[leaves] = np.arange(len(leaves))
    if weight is None:
        weight = np.zeros(n)
        weight[leaves] = np.where(rng.random(len(leaves)) < stop, 0.0, rng.uniform(0.5, 9.0, len(leaves)))
    return dict(child_start=child_start, children=np.asarray(flat, np.int32), descriptor=np.stack(desc).astype(np.uint8), word_id=word_id,
                weight=np.asarray(weight, np.float64), L=L, weighting=0, normalize=1, level=np.asarray(level, np.int32))


def build_vocabulary(branching, seed=0):
    """A tree with branching[l] children per node of level l.  Children are noisy copies of their parent; about 10 % of the inner
    candidates stay leaves (the depth varies between neighbouring features), 30 % of the children are exact copies of a random earlier
    sibling (ties the first must win), 5 % of the words are stop words."""
    rng = np.random.default_rng(4000 + seed)
    desc, children, level = [np.zeros(32, np.uint8)], [[]], [0]
    frontier, L = [0], len(branching)
    for lvl, k in enumerate(branching, 1):
        nxt = []
        for p in frontier:
            base = rng.integers(0, 256, 32, dtype=np.uint8) if p == 0 else desc[p]
            for c in range(k):
                d = _flips(rng, base, 0.25 if lvl == 1 else 0.08)
                if c > 0 and rng.random() < 0.30:
                    d = desc[children[p][rng.integers(0, c)]].copy()
                desc.append(d), children.append([]), level.append(lvl)
                children[p].append(len(desc) - 1)
                if lvl < L and rng.random() >= 0.10:
                    nxt.append(len(desc) - 1)
        frontier = nxt
    return _finish(desc, children, level, L, rng=rng)


def with_scoring(voc, weighting, normalize):
    v = dict(voc)
    v["weighting"], v["normalize"] = weighting, normalize
    return v


def bow_features(voc, n, seed=0):
    """n descriptors: three quarters near a random node's descriptor (so that the descent is no coin toss), the rest random."""
    rng = np.random.default_rng(5000 + seed)
    de = voc["descriptor"]
    out = np.zeros((n, 32), np.uint8)
    for i in range(n):
        out[i] = _flips(rng, de[rng.integers(0, len(de))], 0.04) if rng.random() < 0.75 else rng.integers(0, 256, 32, dtype=np.uint8)
    return out


def tie_trees():
    """name -> (vocabulary, features, expected word of every feature): trees whose first level holds two or more equal minima."""
    rng = np.random.default_rng(6000)
    out = {}
    target = rng.integers(0, 256, 32, dtype=np.uint8)
    feats = np.stack([target] + [_flips(rng, target, 0.02) for _ in range(19)])

    def tree(k, equal_at):
        desc, children, level = [np.zeros(32, np.uint8)], [list(range(1, k + 1))], [0]
        for c in range(k):
            desc.append(target.copy() if c in equal_at else _flips(rng, target, 0.45))
            children.append([]), level.append(1)
        return _finish(desc, children, level, 1, weight=[0.0] + [1.0 + c for c in range(k)])
    out["all_children_identical"] = (tree(20, set(range(20))), feats, 0)
    for p in (0, 7, 15):
        out["minima_at_%d_and_%d" % (p, p + 16)] = (tree(40, {p, p + 16}), feats, p)          # one lane, first and second trip
    out["minima_at_15_and_16"] = (tree(33, {15, 16}), feats, 15)                              # last lane's first trip, first lane's second
    out["minima_at_16_and_31_and_32"] = (tree(40, {16, 31, 32}), feats, 16)                   # none in the first trip
    return out


def stop_word_vocabulary():
    v = build_vocabulary([10, 10], 77)
    v["weight"] = np.zeros_like(v["weight"])
    return v


# a node listed as a child more than once: uvo_vocabulary_create must refuse these (a descent through a cycle would not end)
def bad_vocabularies():
    """name -> (child_start, children, and the same nodes as a tree: child_start, children); n_nodes = len(child_start) - 1."""
    return {
        "own_child": ([0, 2, 3, 3], [1, 2, 1], [0, 2, 2, 2], [1, 2]),                     # node 1 lists itself
        "two_cycle": ([0, 1, 2, 3], [1, 2, 1], [0, 1, 2, 2], [1, 2]),                     # root -> 1 -> 2 -> 1
        "two_parents": ([0, 2, 3, 4, 4], [1, 2, 3, 3], [0, 2, 3, 3, 3], [1, 2, 3]),       # node 3 under 1 and under 2
    }


# ---- haloc ---------------------------------------------------------------------------------------------------------------
HALOC_COUNTS = [0, 1, 2, 63, 64, 65, 500]
HALOC_PROJS = [1, 2, 3, 5]
HALOC_PAD = 7


def haloc_descriptors(n, seed=0):
    rng = np.random.default_rng(7000 + seed)
    de = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    de[:, 3] = 0
    de[:, 17] = 255
    return de


def haloc_projections(num_proj, n, seed=0, kind="normal"):
    """[num_proj][n + 7] float32; the seven columns past n hold NaN, which must never be read."""
    rng = np.random.default_rng(8000 + seed)
    if kind == "normal":
        p = rng.normal(0, 1, (num_proj, n))
        p /= np.maximum(np.linalg.norm(p, axis=1, keepdims=True), 1e-30)
    elif kind == "subnormal":
        p = rng.integers(-40, 41, (num_proj, n)) * 1e-43
    elif kind == "cancel":
        p = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)[None, :] * 1e30 * rng.uniform(0.5, 1.5, (num_proj, n))
    elif kind == "inf":
        p = rng.normal(0, 1, (num_proj, n))
        p[:, n // 3] = np.inf
    else:
        raise ValueError(kind)
    out = np.full((num_proj, n + HALOC_PAD), np.nan, np.float32)
    with np.errstate(all="ignore"):
        out[:, :n] = p.astype(np.float32)
    return out


def haloc_cases():
    """(name, projections with NaN padding, descriptors)."""
    for i, n in enumerate(HALOC_COUNTS):
        for j, k in enumerate(HALOC_PROJS):
            yield "n %d x %d" % (n, k), haloc_projections(k, n, 10 * i + j), haloc_descriptors(n, 10 * i + j)
    for j, kind in enumerate(("subnormal", "cancel", "inf")):
        yield kind, haloc_projections(3, 300, 100 + j, kind), haloc_descriptors(300, 100 + j)
