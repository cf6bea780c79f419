"""Shared by the CPU and the GPU tests of the two-view initialisation: the scene generator, the loader of the host build
(tests/emu/initializer_emu.cpp), one way of running a call on either the library or the host build, and the comparisons."""
import ctypes
import functools

import numpy as np

import host_build
import initializer_model as im

CAM = (458.0, 458.0, 376.0, 240.0)
WIDTH, HEIGHT = 752, 480
EXTRA_REFERENCE_KEYS = 40   # unmatched keys of the reference frame: Normalize runs over all keys, not only the matched ones


def scene(seed, n, share, kind="general"):
    """-> (keys1 float32[n + 40, 2], keys2 float32[n, 2], matches12 int32[n], truth (R, t)).  kind: general | planar | rotation |
    duplicate.  Points uniform in x [-2, 2], y [-1.3, 1.3], z [2, 6]; 0.03 rad about y, t = (-0.3, 0.02, 0.01) (rotation: t scaled to
    1e-4 of that); 0.3 px Gaussian noise on both views, rounded to float32; `share` of the current points replaced by uniform ones."""
    rng = np.random.RandomState(seed)
    fx, fy, cx, cy = CAM
    X = np.stack([rng.uniform(-2, 2, n), rng.uniform(-1.3, 1.3, n), rng.uniform(2, 6, n)], 1)
    if kind == "planar":
        X[:, 2] = 4.0
    a = 0.03
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    t = np.array([-0.3, 0.02, 0.01]) * (1e-4 if kind == "rotation" else 1.0)
    X2 = X @ R.T + t
    p1 = np.stack([fx * X[:, 0] / X[:, 2] + cx, fy * X[:, 1] / X[:, 2] + cy], 1) + rng.normal(0, 0.3, (n, 2))
    p2 = np.stack([fx * X2[:, 0] / X2[:, 2] + cx, fy * X2[:, 1] / X2[:, 2] + cy], 1) + rng.normal(0, 0.3, (n, 2))
    n_out = int(round(share * n))
    out = rng.permutation(n)[:n_out]
    p2[out] = np.stack([rng.uniform(0, WIDTH, n_out), rng.uniform(0, HEIGHT, n_out)], 1)
    extra = np.stack([rng.uniform(0, WIDTH, EXTRA_REFERENCE_KEYS), rng.uniform(0, HEIGHT, EXTRA_REFERENCE_KEYS)], 1)
    perm = rng.permutation(n + EXTRA_REFERENCE_KEYS)          # where each reference key lands in the reference frame's list
    keys1 = np.zeros((n + EXTRA_REFERENCE_KEYS, 2), np.float32)
    keys1[perm] = np.concatenate([p1, extra]).astype(np.float32)
    matches12 = perm[:n].astype(np.int32)
    if kind == "duplicate" and n >= 2:
        matches12[1] = matches12[0]                            # two current keys name the same reference key
    return keys1, p2.astype(np.float32), matches12, (R, t)


# the scene set the tolerances are measured on and the emu is held to the model on: (seed, n, share, kind)
def model_scenes():
    return [(s, 64, 0.1, "general") for s in range(4)] + [(s, 200, 0.2, "general") for s in range(2)] + \
           [(0, 64, 0.1, "planar"), (1, 64, 0.1, "duplicate"), (0, 64, 0.1, "rotation")]


MODEL_ITERATIONS = 200


@functools.lru_cache(maxsize=None)
def model_run(spec, iterations=MODEL_ITERATIONS, rng_seed=1):
    """The model's whole call on a scene, computed once and shared; the result is not to be modified."""
    k1, k2, m12, _ = scene(*spec)
    return im.initialize(k1, k2, m12, CAM, 1.0, iterations, im.GlibcRand(rng_seed))


def conditioned(spec):
    """The input condition of the issue: the model itself finds the top two scores more than 1e-3 apart, relatively."""
    r = model_run(spec)
    return r is not None and r.best >= 0 and r.top_gap > 1e-3


class Emu:
    """tests/emu/initializer_emu.cpp, built on first use with the library's contract: no FMA contraction."""
    _lib = None

    def __init__(self):
        if Emu._lib is None:
            L = ctypes.CDLL(host_build.build("initializer_emu"))
            vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
            L.emu_initializer_create.argtypes = [vp, ci, vp]
            L.emu_initializer_destroy.argtypes = [vp]
            L.emu_initializer_destroy.restype = None
            L.emu_initializer_set_reference.argtypes = [vp, vp, ci, vp, cf, ci]
            L.emu_initializer_initialize.argtypes = [vp, vp, ci, vp, vp, vp]
            L.emu_initializer_hypotheses.argtypes = [vp, vp, vp, vp, ci, vp]
            L.emu_init_compute_f21.argtypes = [vp] * 6
            L.emu_init_compute_f21.restype = None
            L.emu_init_normalize.argtypes = [vp, ci, vp]
            L.emu_init_normalize.restype = None
            L.emu_init_acos.argtypes = [ci, vp, vp]
            L.emu_init_acos.restype = None
            L.emu_init_decompose.argtypes = [vp] * 5
            L.emu_init_decompose.restype = None
            L.emu_init_check_rt.argtypes = [vp] * 5 + [cf, vp, vp]
            L.emu_init_kth.argtypes = [vp, ci, ci]
            L.emu_init_kth.restype = cf
            Emu._lib = L
        self.lib = Emu._lib

    def make(self, uvo, max_keys):
        """The host build behind the library's own Python class."""
        cls = type("HostInitializer", (uvo.Initializer,), {"_prefix": "emu_initializer_"})
        return cls(None, max_keys, _api=self.lib)

    def acos(self, x):
        x = np.ascontiguousarray(x, np.float64)
        out = np.zeros_like(x)
        self.lib.emu_init_acos(len(x), x.ctypes.data, out.ctypes.data)
        return out

    def kth(self, values, idx):
        v = np.ascontiguousarray(values, np.float32)
        return np.float32(self.lib.emu_init_kth(v.ctypes.data, len(v), int(idx)))

    def normalize(self, keys):
        k, out = np.ascontiguousarray(keys, np.float32), np.zeros(4, np.float32)
        self.lib.emu_init_normalize(k.ctypes.data, len(k), out.ctypes.data)
        return out


class Call:
    """What one initialize call leaves behind, on either implementation."""

    def __init__(self, obj, uvo, keys2, matches12, rng):
        self.result = obj.initialize(keys2, matches12, rng)
        self.sets, self.F, self.scores = obj.hypotheses()
        self.rng_state = rng.state()


def run(obj, uvo, spec_or_scene, sigma=1.0, iterations=200, rng=None, set_reference=True):
    k1, k2, m12 = (scene(*spec_or_scene) if len(spec_or_scene) == 4 and isinstance(spec_or_scene[3], str) else spec_or_scene)[:3]
    if set_reference:
        obj.set_reference(k1, CAM, sigma, iterations)
    return Call(obj, uvo, k2, m12, rng if rng is not None else uvo.GlibcRand(1))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else a.dtype)


def assert_calls_equal(a, b, what=""):
    """Bit for bit: every set, every F21i, every score, the mask, the counts and parallaxes, verdict, pose, points, generator."""
    ra, rb = a.result, b.result
    assert (a.sets == b.sets).all(), what + ": sets"
    assert a.F.shape == b.F.shape and (_bits(a.F) == _bits(b.F)).all(), what + ": F21i of hypotheses %s" % np.flatnonzero((_bits(a.F) != _bits(b.F)).any(1))[:8]
    assert (_bits(a.scores) == _bits(b.scores)).all(), what + ": scores of hypotheses %s" % np.flatnonzero(_bits(a.scores) != _bits(b.scores))[:8]
    assert (ra.initialized, ra.best, ra.n_inliers, ra.draws, ra.deciding) == (rb.initialized, rb.best, rb.n_inliers, rb.draws, rb.deciding), \
        what + ": %s != %s" % ((ra.initialized, ra.best, ra.n_inliers, ra.draws, ra.deciding), (rb.initialized, rb.best, rb.n_inliers, rb.draws, rb.deciding))
    assert (ra.n_good == rb.n_good).all(), what + ": nGood %s != %s" % (ra.n_good, rb.n_good)
    for name in ("parallax", "R21", "t21", "F21", "p3d"):
        x, y = getattr(ra, name), getattr(rb, name)
        assert x.shape == y.shape and (_bits(x) == _bits(y)).all(), what + ": %s %s != %s" % (name, x.ravel()[:9], y.ravel()[:9])
    assert _bits(np.float32(ra.score)) == _bits(np.float32(rb.score)), what + ": SF"
    assert (ra.inliers == rb.inliers).all() and (ra.triangulated == rb.triangulated).all(), what + ": masks"
    assert a.rng_state == b.rng_state, what + ": generator state"


def rotation_distance(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


def point_distance(p, q, mask):
    p, q = np.asarray(p, np.float64)[mask], np.asarray(q, np.float64)[mask]
    return float((np.linalg.norm(p - q, axis=1) / np.linalg.norm(q, axis=1)).max()) if len(p) else 0.0


def assert_call_matches_model(call, spec, what=""):
    """The host build (or the library) against the model on a conditioned scene: sets and draws exact; every F up to sign within
    TOL_F; every score within the fp32-sum bound the model derives from that hypothesis's own F; the decisions equal; pose and
    points within tolerance."""
    m = model_run(spec)
    r = call.result
    k1, k2, m12, _ = scene(*spec)
    assert (call.sets == m.sets).all() and r.draws == m.draws, what + ": sets / draws"
    worst = max(im.sign_free_distance(call.F[h], m.F[h]) for h in range(len(m.F)))
    print("%s: worst F distance to the model %.3g (tolerance %.3g)" % (what, worst, im.TOL_F))
    assert worst <= im.TOL_F, what + ": F21i"
    for h in range(len(m.F)):
        terms, _ = im.score_terms(call.F[h], k1[m12], k2, 1.0)
        bound, exact = im.score_bound(terms)
        assert abs(float(call.scores[h]) - exact) <= bound, what + ": score of hypothesis %d: %r vs %r +- %g" % (h, call.scores[h], exact, bound)
    assert r.best == m.best and (r.inliers.astype(bool) == m.inliers).all() and r.n_inliers == m.n_inliers, what + ": best / mask"
    assert list(r.n_good) == list(m.n_good), what + ": nGood %s != %s" % (r.n_good, m.n_good)
    assert (bool(r.initialized), r.deciding) == (m.initialized, m.deciding), what + ": verdict"
    assert np.allclose(r.parallax, np.array(m.parallax, np.float32), rtol=1e-5, atol=1e-5), what + ": parallax %s != %s" % (r.parallax, m.parallax)
    if m.initialized:
        assert rotation_distance(r.R21, m.R21) <= im.TOL_R and im.sign_free_distance(r.t21, m.t21) <= im.TOL_T, what + ": pose"
        assert (r.triangulated.astype(bool) == m.triangulated).all(), what + ": vbTriangulated"
        assert point_distance(r.p3d, m.p3d, m.triangulated) <= im.TOL_POINT, what + ": points"
