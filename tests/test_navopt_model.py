"""tests/navopt_model.py held to cases that can be computed by hand, and the scene list held to the conditions the checks rely on --
on the model alone, without the library: so3's maps against each other, the edges at a state where their residual is known, the
break test on the count of all edges, the reset of the estimates, the marginals taken from the last linearisation, and the list's
coverage (both forms, with and without depth and marginals, shifted correspondences, a re-entry, every edge flagged, NaN class,
a large bias step)."""
import math
import os

import numpy as np

import navopt_checks as nc
import navopt_model as nm

NAMES = list(nm.SCENES)
FIXTURE = os.path.join(nc.ROOT, "tests", "golden", "navopt_scenes.bin")


def test_so3_maps_agree_with_each_other():
    g = np.random.default_rng(5)
    for th in (1e-12, 1e-7, 1e-3, 0.3, 2.0, 3.0):
        v = g.normal(size=3)
        v = v / np.linalg.norm(v) * th
        q = nm.so3_exp(v)
        assert abs(np.linalg.norm(q) - 1) < 4 * nc.U and np.abs(nm.so3_log(q) - v).max() < 1e-14 * max(1, th)
        assert np.abs(nm.rot(q) - nm.pm.rot_of_vec(v)).max() < 1e-14
        assert np.abs(nm.so3_jr(v) @ nm.so3_jrinv(v) - np.eye(3)).max() < 1e-12
    assert nm.so3_jr(np.zeros(3)).tolist() == np.eye(3).tolist() and nm.so3_jrinv(np.ones(3) * 1e-6).tolist() == np.eye(3).tolist()
    # log of a quaternion with w < 0: atan(n / w) is negative, the vector is not flipped first
    q = nm.so3_exp(np.array([0.0, 0.0, 4.0]))
    assert q[3] < 0 and abs(nm.so3_log(q)[2] - (4.0 - 2 * math.pi)) < 1e-14


def test_edges_at_a_state_where_the_residual_is_known():
    sc = nm.scene(7, nm.FRAME, n=20, has_depth=True)
    # the preintegration was made from the two true states up to 1e-3 of noise: at the truth the IMU residual is that noise
    truth = [dict(sc["cur"]), sc["last"]]
    g, dT, Ri = np.asarray(sc["gw"]), sc["dT"], nm.rot(sc["last"]["q"])
    truth[0]["V"] = sc["last"]["V"] + g * dT + Ri @ np.asarray(sc["dV"])
    truth[0]["P"] = sc["last"]["P"] + sc["last"]["V"] * dT + 0.5 * g * dT * dT + Ri @ np.asarray(sc["dP"])
    truth[0]["q"] = nm.qmul(sc["last"]["q"], nm.q_of_matrix(sc["dR"]))
    zero = dict(sc["last"], dbg=np.zeros(3), dba=np.zeros(3))
    _, e, info, J, _ = nm.edge_imu([truth[0], zero], sc)
    assert np.abs(e).max() < 1e-12 and set(J) == {0, 15, 24}
    # the bias edge: (bias + delta bias) of the frame minus that of the last frame; the depth edge by hand
    _, e, info, J, _ = nm.edge_bias([sc["cur"], sc["last"]], sc)
    assert np.abs(e).max() < 1e-15 and info[0, 0] == 1 / sc["gyr_rw2"] / dT and info[5, 5] == 1 / sc["acc_rw2"] / dT
    s = nm.state(P=(1, 2, 3), V=(0.5, 0.25, -1))
    hand = dict(sc, shi=1.0, depth_meas=5.0, dT=0.5, dP=np.zeros(3), JPg=np.zeros(9), JPa=np.zeros(9))
    _, e, _, J, _ = nm.edge_depth([s, nm.state(P=(0, 0, 7))], hand)
    # frame form: vertex 0 is the CURRENT frame: projected = 5; r1 = 5 - 7; r2 = 5 - (3 + 0.5 * -1 + 0.25 * 9.81): no 1/2 on the gravity term
    assert abs(e[0] - ((5 - 7) + (5 - (3 - 0.5 + 0.25 * 9.81)))) < 1e-14 and J[0][0, 2] == -1 and J[0][0, 5] == -0.5 and J[15][0, 2] == -1
    _, e, _, J, _ = nm.edge_depth([nm.state(P=(0, 0, 7)), s], dict(hand, form=nm.KEYFRAME))
    assert abs(e[0] - ((5 - 7) + (5 - (3 - 0.5 + 0.25 * 9.81)))) < 1e-14 and set(J) == {0} and J[0][0, 2] == -1
    # a reprojection edge seen from the state that made it: the residual is the half pixel of noise
    clean = nm.scene(8, nm.KEYFRAME, n=30, off=(0.0, 0.0, 0.0))
    ev = nm.reproj(clean["cur"], clean, clean["edges"])
    assert np.abs(np.stack([ev["e0"], ev["e1"]])).max() < 5 and (ev["J"][:, :, 3:6] == 0).all()


def test_reprojection_jacobian_is_the_derivative_under_the_increment():
    """IncSmallPVR applies P += R dP with the rotation before the update, then R = R exp(dPhi): the 2 x 9 Jacobian is the derivative of
    the error under exactly that increment."""
    sc = nm.scene(9, nm.KEYFRAME, n=6)
    s = sc["cur"]
    J = nm.reproj(s, sc, sc["edges"])["J"]
    h = 1e-6
    for k in range(9):
        d = np.zeros(9)
        d[k] = h
        a, b = nm.reproj(nm.oplus(s, d, np.zeros(6)), sc, sc["edges"]), nm.reproj(nm.oplus(s, -d, np.zeros(6)), sc, sc["edges"])
        num = np.stack([(a["e0"] - b["e0"]) / (2 * h), (a["e1"] - b["e1"]) / (2 * h)], 1)
        assert np.abs(num - J[:, :, k]).max() < 1e-4 * (1 + np.abs(J[:, :, k]).max()), k


def test_scene_list_meets_the_conditions_on_the_model_alone():
    assert len(NAMES) >= 30
    for form in (nm.KEYFRAME, nm.FRAME):
        for depth in (False, True):
            for marg in (False, True):
                assert any((s.get("form", 0), bool(s.get("has_depth")), bool(s.get("marg"))) == (form, depth, marg) for s in nm.SCENES.values()), (form, depth, marg)
    thin, short = [n for n in NAMES if nc.thin(n)], []
    assert len(thin) * 10 <= len(NAMES), thin                      # the cap: at most 1 scene in 10 skipped for a thin margin
    for name in NAMES:
        _, res = nc.model(name)
        if nc.not_finite(res) or not res.trials or name in thin:
            continue
        k = nc.compared_prefix(name)
        if k < max(5, nc.first_iteration_trials(res)) and k < len(res.trials):
            short.append((name, k))
    assert not short, short                                         # the whole first iteration of round 0 and at least 5 trials
    assert sum(nc.not_finite(nc.model(n)[1]) for n in NAMES) == 2   # the scenes whose decisions are made by class, one of each form
    assert all(nm.reentries(nc.model(n)[1]) for n in nm.REENTRY)
    for p in ("kf", "fr"):
        r = nc.model(p + "_none_left_12")[1]
        assert r.rounds == 4 and r.n_inliers == 0 and all(f.all() for f in r.flags[0])      # every edge flagged, four rounds all the same
        assert nc.model(p + "_few_5")[1].rounds == 1 and nc.model(p + "_too_few")[1].rounds == 0
        sc, r = nc.model(p + "_bias_step_100")
        assert np.abs(r.ns["dbg"] - sc["cur"]["dbg"]).max() > 5e-3                            # the large bias step is taken back
        sc, r = nc.model(p + "_degenerate_50")
        assert math.isnan(r.lin[0]["chi2"]) and not any(t["ok"] for t in r.trials) and len(r.lin) == 40 and r.outlier[0][0] == 0


def test_the_estimates_are_reset_and_the_break_test_counts_all_edges():
    sc, res = nc.model("kf_shift_100")
    start = nm.state_vec(nc.start_of(sc)[0])
    firsts = [L for L in res.lin if L["iteration"] == 0]
    assert len(firsts) == 4 and all((nm.state_vec(L["est"][0]) == start).all() for L in firsts)
    # 9 edges of the graph: one round; 10: four -- whatever is still active
    for n, depth, rounds in ((7, False, 1), (8, False, 4), (6, True, 1), (7, True, 4)):
        assert nm.optimize(nm.scene(3, nm.KEYFRAME, n=n, has_depth=depth)).rounds == rounds, (n, depth)
    for n, depth, rounds in ((6, False, 1), (7, False, 4), (5, True, 1), (6, True, 4)):
        assert nm.optimize(nm.scene(3, nm.FRAME, n=n, n_last=0, has_depth=depth)).rounds == rounds, (n, depth)
    assert nm.optimize(nm.scene(3, nm.FRAME, n=3, n_last=50)).rounds == 0 and nm.optimize(nm.scene(3, nm.KEYFRAME, n=2)).rounds == 0


def test_marginals_come_from_the_last_linearisation_of_the_last_round():
    moved = 0
    for name in ("kf_depth_marg_30", "fr_depth_marg_30"):
        sc, res = nc.model(name)
        assert res.marg_ok and res.H_last is res.lin[-1]["H"] and res.lin[-1]["round"] == 3
        cov = np.linalg.inv(res.lin[-1]["H"])[:15, :15]
        assert np.abs(res.marg_cov - cov).max() == 0
        fresh = nm.linearise(res.est, sc, res.lin[-1]["active"], False)["H"]
        if res.trials[-1]["accepted"]:                              # a new linearisation at the final estimate is another matrix
            assert np.abs(fresh - res.H_last).max() > 1e-9 * np.abs(res.H_last).max()
            moved += 1
        if sc["form"] == nm.KEYFRAME:
            assert not res.marg_cov_inv[:9, 9:].any() and np.abs(res.marg_cov_inv[:9, :9] @ cov[:9, :9] - np.eye(9)).max() < 1e-6
        else:
            assert np.abs(res.marg_cov_inv @ cov - np.eye(15)).max() < 1e-6 and res.marg_cov_inv[:9, 9:].any()
    assert moved


def test_recorded_spreads_are_what_the_model_shows():
    """T and M come from the model under permuted edge orders.  The full measurement is the one DESIGN.md section 4 records; here a
    part of it is repeated, and has to stay within the recorded spreads."""
    st, chi, flips = nc.measure_spread(["kf_plain_64", "fr_shift_60", "kf_shift_100", "fr_depth_marg_30", "kf_bias_step_100"], orders=3)
    print("state spread %.3e (recorded %.1e), chi2 spread %.3e (recorded %.1e), mask changes %d" % (st, nc.STATE_SPREAD, chi, nc.CHI2_SPREAD, flips))
    assert st <= nc.STATE_SPREAD and chi <= nc.CHI2_SPREAD and flips == 0
    assert nc.T_STATE == 4 * nc.STATE_SPREAD and nc.M_CHI2 == 4 * nc.CHI2_SPREAD


def test_committed_scene_list_is_the_models():
    scenes = nm.load(FIXTURE)
    assert len(scenes) == len(NAMES)
    for name, (rec, edges) in zip(NAMES, scenes):
        sc = nc.model(name)[0]
        assert rec.tobytes() == nm.record(sc).tobytes() and edges.tobytes() == nm.all_edges(sc).tobytes(), name
