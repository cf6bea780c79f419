"""USLAM::Initializer::Initialize on the device (csrc/initializer.hip) against the host build of the same source
(tests/emu/initializer_emu.cpp, which walks Initialize as the reference writes it), BIT FOR BIT: every set, every F21i and every score
through the test tap, the inlier mask, the four counts and parallaxes, the verdict, the pose, the points and the generator state
handed back.  The shapes are the smallest at which the call can still go wrong: N = 8 where every set is a permutation of all matches,
the edges of a ballot word, one N beyond a block of hypothesis lanes' worth of matches and one at the workload's size, the edges of a
hypothesis workgroup in the iteration count, the calls that return nothing."""
import numpy as np
import pytest

import initializer_checks as ic

pytestmark = pytest.mark.gpu

MAX_KEYS = 1100


@pytest.fixture(scope="module")
def emu():
    return ic.Emu()


@pytest.fixture(scope="module")
def klt(uvo):
    k = uvo.KLT(64, 64, max_points=256)
    yield k
    k.close()


@pytest.fixture(scope="module")
def pair(uvo, emu, klt):
    dev, host = uvo.Initializer(klt, MAX_KEYS), emu.make(uvo, MAX_KEYS)
    yield dev, host
    dev.close()
    host.close()


def both(uvo, pair, sc, iterations=200, seed=1, sigma=1.0, what=""):
    dev, host = pair
    a = ic.run(dev, uvo, sc, sigma, iterations, uvo.GlibcRand(seed))
    b = ic.run(host, uvo, sc, sigma, iterations, uvo.GlibcRand(seed))
    ic.assert_calls_equal(a, b, what)
    return a


@pytest.mark.parametrize("n,share", ((8, 0.0), (9, 0.0), (63, 0.1), (64, 0.1), (65, 0.1), (200, 0.2), (1000, 0.3)))
def test_sizes(uvo, pair, n, share):
    a = both(uvo, pair, (n, n, share, "general"), what="N=%d" % n)
    assert a.result.draws == 1600 and len(a.sets) == 200
    if n == 8:
        assert all(sorted(s) == list(range(8)) for s in a.sets.tolist())
    if n in (64, 200):
        assert a.result.best >= 0 and a.result.n_inliers >= 0.6 * n


@pytest.mark.parametrize("iterations", (1, 64, 65, 200))
def test_iterations(uvo, pair, iterations):
    a = both(uvo, pair, (5, 100, 0.2, "general"), iterations=iterations, what="%d iterations" % iterations)
    assert len(a.sets) == iterations and a.result.draws == 8 * iterations


def test_both_verdicts_and_the_model(uvo, pair):
    seen = set()
    for spec in ic.model_scenes()[:4] + [(0, 64, 0.1, "rotation")]:
        a = both(uvo, pair, spec, what=str(spec))
        ic.assert_call_matches_model(a, spec, what=str(spec))
        seen.add(bool(a.result.initialized))
    assert seen == {True, False}


def test_seven_matches_no_result_no_draws(uvo, pair):
    g = uvo.GlibcRand(1)
    for obj in pair:
        k1, k2, m12, _ = ic.scene(0, 7, 0.0)
        c = ic.run(obj, uvo, (k1, k2, m12), rng=g)
        assert not c.result.initialized and c.result.draws == 0 and c.result.best == -1 and len(c.sets) == 0
    assert g.state() == uvo.GlibcRand(1).state()


def test_all_outliers(uvo, pair):
    a = both(uvo, pair, (3, 100, 1.0, "general"), what="all outliers")
    assert not a.result.initialized


def test_zero_score_departure(uvo, pair):
    """Matches so far off every epipolar line that no hypothesis scores: best = -1, nothing decomposed, the draws still consumed."""
    k1, k2, m12, _ = ic.scene(4, 16, 0.0)
    a = both(uvo, pair, (k1, k2, m12), sigma=1e-4, iterations=20, what="zero score")
    assert a.result.best == -1 and not a.result.initialized and a.result.draws == 160 and a.result.deciding == -1
    assert not a.result.inliers.any() and not a.result.F21.any()


@pytest.mark.parametrize("kind", ("rotation", "planar", "duplicate"))
def test_special_scenes(uvo, pair, kind):
    a = both(uvo, pair, (0, 64, 0.1, kind), what=kind)
    if kind == "rotation":
        assert not a.result.initialized


def test_consecutive_calls_on_one_generator_and_a_new_reference(uvo, pair):
    dev, host = pair
    gd, gh = uvo.GlibcRand(7), uvo.GlibcRand(7)
    s1, s2 = ic.scene(11, 120, 0.2), ic.scene(12, 90, 0.1)
    for n, sc in enumerate((s1, s1, s2, s1)):            # the second call continues the stream; set_reference again between calls
        a = ic.run(dev, uvo, sc[:3], iterations=40, rng=gd, set_reference=n != 1)
        b = ic.run(host, uvo, sc[:3], iterations=40, rng=gh, set_reference=n != 1)
        ic.assert_calls_equal(a, b, "call %d" % n)
    ref = uvo.GlibcRand(7)
    for _ in range(4 * 320):
        ref.next()
    assert gd.state() == ref.state()


def test_an_object_filled_to_capacity_equals_one_with_room_to_spare(uvo, emu, klt):
    """max_keys = n1 = n2 = 65: the last element of every array of the object's block and of both exchanges is written and read, the mask
    spans two 64-bit words; the call equals, bit for bit, the one on an object of 256 keys and the host build's."""
    k1, k2, m12, _ = ic.scene(65, 65, 0.1)
    place = np.random.RandomState(65).permutation(65)         # the 65 matched reference keys alone, shuffled: every reference key is named
    ref = np.zeros((65, 2), np.float32)
    ref[place] = k1[m12]
    sc = (ref, k2, place.astype(np.int32))
    calls = []
    for make in (lambda: uvo.Initializer(klt, 65), lambda: uvo.Initializer(klt, 256), lambda: emu.make(uvo, 65)):
        obj = make()
        try:
            calls.append(ic.run(obj, uvo, sc, rng=uvo.GlibcRand(1)))
        finally:
            obj.close()
    ic.assert_calls_equal(calls[0], calls[1], "65 keys against 256")
    ic.assert_calls_equal(calls[0], calls[2], "65 keys against the host build")
    r = calls[0].result
    assert r.initialized and r.inliers[64] == 1 and r.triangulated[64] == 1 and r.p3d[64].any() and len(calls[0].sets) == 200


def test_out_of_range_match_and_capacity(uvo, pair):
    dev = pair[0]
    k1, k2, m12, _ = ic.scene(0, 16, 0.0)
    dev.set_reference(k1, ic.CAM, 1.0, 10)
    bad = m12.copy()
    bad[5] = -1
    with pytest.raises(uvo.UvoError) as ei:
        dev.initialize(k2, bad, uvo.GlibcRand(1))
    assert ei.value.code == uvo.UVO_E_BADARG
    with pytest.raises(uvo.UvoError):
        dev.set_reference(k1, ic.CAM, 1.0, 1025)
    with pytest.raises(uvo.UvoError):
        dev.initialize(np.zeros((MAX_KEYS + 1, 2), np.float32), np.zeros(MAX_KEYS + 1, np.int32), uvo.GlibcRand(1))
