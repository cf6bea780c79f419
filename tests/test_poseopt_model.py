"""tests/poseopt_model.py held to cases that can be computed by hand: one edge, an exactly consistent scene, the Huber branch on either
side of delta^2, the classification rules (an outlier is re-evaluated and comes back, an inlier is judged on its stored error, a NaN
decides nothing) and the break test (all edges counted, not the active ones)."""
import math

import numpy as np
import pytest

import poseopt_model as pm

K = (400.0, 400.0, 320.0, 240.0)
I4 = np.eye(4, dtype=np.float32)


def test_constants_are_the_floats_of_the_source():
    assert pm.CHI2 == (float(np.float32(9.21)), float(np.float32(7.378)), float(np.float32(5.991)), float(np.float32(5.991)))
    assert pm.DELTA == float(np.float32(math.sqrt(5.991))) and pm.DELTA != math.sqrt(5.991)
    assert pm.ITS == (10, 10, 7, 5)


def test_one_edge_by_hand():
    """A point at (1, 2, 4) seen from the identity: u = 400 * 0.25 + 320 = 420, v = 400 * 0.5 + 240 = 440.  Observed at (423, 436) with
    invSigma2 0.5: e = (3, -4), chi2 = 0.5 * 25 = 12.5 > delta^2: rho = (2 sqrt(12.5) delta - delta^2, delta / sqrt(12.5))."""
    q, t = pm.pose_of(I4)
    assert q.tolist() == [0, 0, 0, 1] and t.tolist() == [0, 0, 0]
    ev = pm.edge_eval(q, t, K, [[1, 2, 4]], [[423, 436]], [0.5])
    assert (ev["e0"][0], ev["e1"][0], ev["chi2"][0]) == (3.0, -4.0, 12.5)
    rho0, rho1 = pm.huber(ev["chi2"])
    assert rho0[0] == 2 * math.sqrt(12.5) * pm.DELTA - pm.DSQR and rho1[0] == pm.DELTA / math.sqrt(12.5)
    J = pm.jacobian(ev, K)[0]
    x, y, z = 1.0, 2.0, 4.0
    want = [[x * y / 16 * 400, -(1 + x * x / 16) * 400, y / z * 400, -1 / z * 400, 0, x / 16 * 400],
            [(1 + y * y / 16) * 400, -x * y / 16 * 400, -x / z * 400, 0, -1 / z * 400, y / 16 * 400]]
    assert J.tolist() == want
    L = pm.linearise(q, t, K, [[1, 2, 4]], [[423, 436]], [0.5], np.array([True]))
    wo = rho1[0] * 0.5
    assert L["H"][0, 0] == (J[0, 0] * wo) * J[0, 0] + (J[1, 0] * wo) * J[1, 0]
    assert L["b"][3] == J[0, 3] * (-(0.5 * 3.0) * rho1[0]) + J[1, 3] * (-(0.5 * -4.0) * rho1[0])      # the Huber weight is on b as well
    assert L["chi2"] == rho0[0]


def test_huber_on_either_side_of_delta_squared():
    below, above = np.nextafter(pm.DSQR, 0), np.nextafter(pm.DSQR, 10)
    rho0, rho1 = pm.huber([below, pm.DSQR, above, 4 * pm.DSQR])
    assert rho0[0] == below and rho1[0] == 1 and rho0[1] == pm.DSQR and rho1[1] == 1        # e <= dsqr: the inlier branch, dsqr included
    assert rho0[2] == 2 * math.sqrt(above) * pm.DELTA - pm.DSQR and rho1[2] == pm.DELTA / math.sqrt(above)   # the outlier branch's formulas
    assert abs(rho0[2] - above) < 1e-14                                                       # rho is continuous at delta^2
    assert rho1[3] == 0.5 and rho0[3] == 3 * pm.DSQR                                          # at 4 delta^2: delta / (2 delta), 4 delta^2 - delta^2


def _consistent(n, seed=3):
    g = np.random.default_rng(seed)
    pc = np.stack([g.integers(-8, 9, n) / 4.0, g.integers(-8, 9, n) / 4.0, g.choice([2.0, 4.0, 8.0], n)], 1)
    uv = np.stack([K[0] * pc[:, 0] / pc[:, 2] + K[2], K[1] * pc[:, 1] / pc[:, 2] + K[3]], 1)     # exact in float and in double
    return pc.astype(np.float32), uv.astype(np.float32), np.ones(n, np.float32)


def test_consistent_scene_moves_nothing_and_flags_nothing():
    p3d, p2d, w = _consistent(40)
    r = pm.optimize(p3d, p2d, w, K, I4)
    assert r.rounds == 4 and r.n_inliers == 40 and not r.outlier.any()
    assert r.Tcw.tobytes() == I4.tobytes() and r.q.tolist() == [0, 0, 0, 1] and r.t.tolist() == [0, 0, 0]
    assert all(L["chi2"] == 0 and not L["b"].any() for L in r.lin)
    # rho == 0 at the first trial of every round: Terminate, one linearisation and one trial a round
    assert [(L["round"], L["iteration"]) for L in r.lin] == [(0, 0), (1, 0), (2, 0), (3, 0)] and len(r.trials) == 4
    assert all(t["rho"] == 0 and not t["accepted"] for t in r.trials)


def test_nothing_to_optimise_returns_the_round_trip_not_the_input():
    T = np.eye(4, dtype=np.float32)
    c, s = np.float32(math.cos(0.3)), np.float32(math.sin(0.3))
    T[:2, :2] = [[c, -s], [s, c]]                      # float entries: not exactly orthonormal
    T[:3, 3] = [0.1, 0.2, 0.3]
    r = pm.optimize(np.zeros((0, 3)), np.zeros((0, 2)), np.zeros(0), K, T)
    assert r.rounds == 1 and r.n_inliers == 0 and len(r.lin) == 0
    q, t = pm.pose_of(T)
    assert r.Tcw.tobytes() == pm.matrix_of(q, t)[0].tobytes()
    assert abs(float(np.linalg.norm(q)) - 1) < 1e-15
    assert np.abs(r.R @ r.R.T - np.eye(3)).max() < 1e-15 < np.abs(T[:3, :3].astype(np.float64) @ T[:3, :3].astype(np.float64).T - np.eye(3)).max()


def test_fewer_than_ten_edges_run_one_round_ten_run_four_whatever_is_active():
    p3d, p2d, w = _consistent(10)
    assert pm.optimize(p3d[:9], p2d[:9], w[:9], K, I4).rounds == 1
    bad = p2d.copy()
    bad[:4] += 60                                      # four gross outliers: six active edges after round 0
    r = pm.optimize(p3d, bad, w, K, I4)
    assert r.rounds == 4 and r.active_after[0] == 6 and r.n_inliers == 6 and r.outlier[:4].all() and not r.outlier[4:].any()
    assert any(L["round"] == 3 for L in r.lin)          # and the Levenberg work of the later rounds is done


def test_an_outlier_is_re_evaluated_and_comes_back():
    sc = pm.make("plain_1000")
    r = pm.optimize(*sc)
    assert r.active_after[0] < 10 and r.active_after[-1] == 1000 and pm.reentries(r) > 900 and r.n_inliers == 1000
    for name in pm.REENTRY:
        assert pm.reentries(pm.optimize(*pm.make(name))) >= 1, name


def test_no_active_edge_left_still_classifies():
    r = pm.optimize(*pm.make("none_left_12"))
    assert r.active_after == [0, 0, 0, 0] and r.rounds == 4 and r.n_inliers == 0
    assert all(L["round"] == 0 for L in r.lin)          # no Levenberg work after round 0 ...
    assert len(r.class_chi2) == 4                       # ... but four classifications


def test_an_inlier_is_judged_on_the_error_of_the_last_trial_accepted_or_not():
    r = pm.optimize(*pm.make("shift_60_1"))
    last = r.trials[-1]
    ev = pm.edge_eval(last["q"], last["t"], *[pm.make("shift_60_1")[i] for i in (3, 0, 1, 2)])
    active = r.lin[-1]["active"]
    assert (r.class_chi2[3][active] == ev["chi2"][active]).all()
    if not last["accepted"]:
        final = pm.edge_eval(r.q, r.t, *[pm.make("shift_60_1")[i] for i in (3, 0, 1, 2)])
        assert (final["chi2"][active] != ev["chi2"][active]).any()


def test_a_nan_chi2_decides_nothing():
    sc = pm.make("plane_exact_50")
    r = pm.optimize(*sc)
    assert math.isnan(r.class_chi2[0][0]) and not r.outlier[0] and r.rounds == 4
    assert all(not t["ok"] and not t["accepted"] and t["tmp"] == pm.DBL_MAX for t in r.trials)
    assert r.n_inliers == 50 - int(r.outlier.sum())
    assert r.Tcw.tobytes() == pm.matrix_of(*pm.pose_of(sc[4]))[0].tobytes()
