"""The host build of csrc/initializer_core.hpp (tests/emu/initializer_emu.cpp, which walks Initialize as the reference writes it)
against the numpy model (tests/initializer_model.py): sets and draw count exact, every hypothesis's F within TOL_F up to sign, every
score within the fp32-sum bound the model derives, the chosen hypothesis, the inlier mask, the four nGood, the verdict and the
deciding index EQUAL on the conditioned scenes, pose and points within tolerance.  No GPU."""
import numpy as np
import pytest

import initializer_checks as ic
import initializer_model as im


@pytest.fixture(scope="module")
def emu():
    return ic.Emu()


@pytest.fixture(scope="module")
def host(uvo, emu):
    h = emu.make(uvo, 1024)
    yield h
    h.close()


SPECS = [s for s in ic.model_scenes()]


@pytest.mark.parametrize("spec", SPECS, ids=lambda s: "%s-n%d-seed%d" % (s[3], s[1], s[0]))
def test_host_build_against_model(uvo, host, spec):
    if not ic.conditioned(spec):
        pytest.fail("scene %r does not meet the input condition; the scene set was chosen so that all do" % (spec,))
    call = ic.run(host, uvo, spec, iterations=ic.MODEL_ITERATIONS)
    ic.assert_call_matches_model(call, spec, what=str(spec))


def test_normalize_runs_over_all_keys(uvo, emu):
    k1, _, m12, _ = ic.scene(3, 64, 0.1)
    assert emu.normalize(k1).tobytes() == np.array(im.normalize(k1), np.float32).tobytes()
    assert emu.normalize(k1[m12]).tobytes() != emu.normalize(k1).tobytes()          # the 40 unmatched keys show


def test_acos_from_ieee_operations(emu):
    x = np.concatenate([np.linspace(-1, 1, 20001), 1 - np.logspace(-12, -1, 200), [0.99998, 1.0, -1.0, 0.0]])
    assert np.abs(emu.acos(x) - np.arccos(x)).max() < 1e-15 + 4 * np.finfo(np.float64).eps * np.pi
    assert np.isnan(emu.acos(np.array([1.0000001, -2.0, np.nan]))).all()


def test_bitwise_selection_is_the_sorted_order_statistic(emu):
    """The device selects sorted[min(50, size - 1)] bit by bit over an order-preserving key; any exact selection gives that value."""
    rng = np.random.RandomState(9)
    for n in (1, 2, 50, 51, 52, 333):
        v = np.concatenate([rng.uniform(-1, 1, n), [0.99998, 0.99998, -0.5, -0.5]]).astype(np.float32)[:max(n, 1)]
        rng.shuffle(v)
        idx = min(50, len(v) - 1)
        assert emu.kth(v, idx).tobytes() == np.sort(v)[idx].tobytes()
        assert emu.kth(v, 0).tobytes() == v.min().tobytes() and emu.kth(v, len(v) - 1).tobytes() == v.max().tobytes()


def test_generator_advances_by_eight_per_iteration_and_continues(uvo, host):
    spec = (1, 64, 0.1, "general")
    g = uvo.GlibcRand(1)
    a = ic.run(host, uvo, spec, iterations=25, rng=g)
    ref = uvo.GlibcRand(1)
    for _ in range(200):
        ref.next()
    assert a.result.draws == 200 and g.state() == ref.state()
    b = ic.run(host, uvo, spec, iterations=25, rng=g, set_reference=False)
    k1, k2, m12, _ = ic.scene(*spec)
    mg = im.GlibcRand(1)
    im.draw_sets(mg, 64, 25)
    assert (b.sets == im.draw_sets(mg, 64, 25)).all()                              # the second call's sets are the stream's next 200


def test_fewer_than_eight_matches_no_result_no_draws(uvo, host):
    k1, k2, m12, _ = ic.scene(0, 7, 0.0)
    g = uvo.GlibcRand(1)
    c = ic.run(host, uvo, (k1, k2, m12), rng=g)
    assert not c.result.initialized and c.result.draws == 0 and c.result.best == -1 and len(c.sets) == 0
    assert g.state() == uvo.GlibcRand(1).state()


def test_bad_arguments(uvo, host):
    k1, k2, m12, _ = ic.scene(0, 16, 0.0)
    host.set_reference(k1, ic.CAM, 1.0, 10)
    bad = m12.copy()
    bad[3] = len(k1)
    with pytest.raises(uvo.UvoError):
        host.initialize(k2, bad, uvo.GlibcRand(1))
    with pytest.raises(uvo.UvoError):
        host.set_reference(k1, ic.CAM, 1.0, 1025)                                   # the iterations cap
