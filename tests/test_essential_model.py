"""The numpy model of the essential-graph optimisation (tests/essential_model.py) against closed forms: log() inverts the constructor
from an update, a consistent graph stays put, a perturbed consistent ring returns to consistency, the committed fixture is the
generator's, and the recorded spreads that set T (tests/essential_checks.py) are reproduced on the scene that sets them."""
import numpy as np
import pytest

import essential_checks as pc
import essential_model as em


@pytest.mark.parametrize("omega, sigma", [(1e-7, 1e-8), (1e-7, 0.2), (0.6, 1e-8), (0.6, -0.25), (2.5, 0.1)])
def test_log_inverts_the_constructor_from_an_update(omega, sigma):
    """In each of the four branches, and close to pi."""
    g = np.random.default_rng(2)
    for _ in range(50):
        w = g.normal(size=3)
        v = np.concatenate([w / np.linalg.norm(w) * omega, g.normal(size=3) * 2, [sigma * g.uniform(0.5, 1)]])
        back = em.sim_log(em.sim_from_update(v))[0]
        # Quaternion(R) of a rotation by theta and acos of its trace: 1e-15 / sin(theta), and the first-order omega of the near branch
        assert np.abs(back - v).max() < 1e-9, (v, back)


def test_product_inverse_and_map_agree():
    g = np.random.default_rng(3)
    a, b = pc.random_sim(g), pc.random_sim(g)
    a[:4], b[:4] = a[:4] / np.linalg.norm(a[:4]), b[:4] / np.linalg.norm(b[:4])      # a group only with unit quaternions
    X = g.normal(size=3)
    assert np.abs(em.sim_map(em.sim_mul(a, b), X) - em.sim_map(a, em.sim_map(b, X))).max() < 1e-13
    assert np.abs(em.sim_map(em.sim_inv(a), em.sim_map(a, X)) - X).max() < 1e-13


def _ring(g, K=8, perturb=0.0):
    """Exact similarities on a ring, every edge measured from them; the estimates of the free key frames perturbed in rotation and
    translation.  The scales are 1 and stay there: with a rotation error below 0.0045 rad and |log s| above 1e-5 log() takes the branch
    whose B is ((sigma^2 / 2 - sigma + 1) s) / sigma^3 (sim3.h:199, about 1 / sigma^3 where the limit is 1/6), W loses its rank and no
    Gauss-Newton step is accepted any more; that is the reference's arithmetic, restated, and not what this test is about."""
    S = np.array([em._sim(em._rodrigues([0, 2 * np.pi * k / K, 0.1 * k]), g.normal(size=3) * 3, 1.0) for k in range(K)])
    ei = np.array(list(range(1, K)) + [K - 1, K - 2], np.int32)
    ej = np.array(list(range(0, K - 1)) + [0, 1], np.int32)
    est = S.copy()
    for k in range(1, K):
        est[k] = em.sim_mul(em.sim_from_update(g.normal(size=7) * perturb * np.array([1, 1, 1, 1, 1, 1, 0])), S[k])
    return dict(Scw=est, Scwn=S, edge_i=ei, edge_j=ej, conn=np.zeros(len(ei), np.uint8), points=np.zeros((0, 3), np.float32), ref=np.zeros(0, np.int32),
                fixed=0, n_iterations=20), S


def test_consistent_graph_stays_put():
    sc, S = _ring(np.random.default_rng(4))
    r = em.optimize(sc)
    assert r.lin[0].chi2 < 1e-24 and np.abs(r.S - S).max() < 1e-9


def test_perturbed_consistent_ring_returns_to_consistency():
    """As far as the reference's arithmetic lets it: the first Gauss-Newton step takes chi2 down by four orders; it leaves every edge
    with a rotation error below 0.0045 rad and a |log s| above 1e-5, where _ring's note applies and the driver ends after ten rejected
    trials.  (tests/essential_checks.py's scenes show the same end: it is the reference's, not the model's.)"""
    sc, S = _ring(np.random.default_rng(5), perturb=0.05)
    r = em.optimize(sc)
    before = np.abs(sc["Scw"] - S).max()
    assert r.lin[0].chi2 > 1 and r.trials[-1]["cur_after"] < 1e-3 * r.lin[0].chi2 and r.trials[0]["accepted"]
    assert np.abs(r.S - S).max() < 0.25 * before
    T, _ = em.recover(sc, r.S)
    assert np.abs(T[:, :3, 3] - (r.S[:, 4:7] / r.S[:, 7:8])).max() < 1e-5 and np.abs(T[:, :3, :3] - em.rotmat(r.S[:, :4]).reshape(-1, 3, 3)).max() < 1e-6


def test_fixture_is_the_generators():
    got = em.load(em.FIXTURE)
    for name in em.SCENES:
        want = em._make(name)
        assert set(got[name]) == set(want)
        for k, v in want.items():
            assert np.array_equal(got[name][k], v), (name, k)


def test_recorded_spreads_are_what_the_model_shows():
    """T comes from the model under 8 permuted edge orders and the mpmath evaluation of every error.  The measurement over all scenes
    (`python tests/essential_checks.py`) is NOT repeated by the suite; what is repeated is the same measurement on the scene that sets
    the maxima: within the recorded spreads, and not below nine tenths of them."""
    detail = {}
    est, pts, unclear = pc.measure_spread(list(pc.SPREAD_SCENES), detail=detail)
    chi = max(v[2] for v in detail.values())
    print("estimate spread %.3e (recorded %.1e), points %.3e (%.1e), relative chi2 %.3e (%.1e)" % (est, pc.EST_SPREAD, pts, pc.PTS_SPREAD, chi, pc.CHI2_REL_SPREAD))
    assert 0.9 * pc.EST_SPREAD <= est <= pc.EST_SPREAD and 0.9 * pc.PTS_SPREAD <= pts <= pc.PTS_SPREAD and not unclear
    assert 0.9 * pc.CHI2_REL_SPREAD <= chi <= pc.CHI2_REL_SPREAD
    assert pc.T_EST == 4 * pc.EST_SPREAD and pc.T_PTS == 4 * pc.PTS_SPREAD and pc.M_REL == 4 * pc.CHI2_REL_SPREAD
