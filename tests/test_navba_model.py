"""The numpy model of Optimizer::LocalBundleAdjustmentNavState (tests/navba_model.py) against itself: the Jacobians of all four edge kinds
against central differences through the vertices' own oplus, a window without inertial weight against tests/ba_model.py on the same
geometry, and the scenes that pin the rules a reader would not guess."""
import numpy as np
import pytest

import ba_model as bm
import navba_model as vm
import navopt_model as nm


def perturbed(est, k, kind, i, h):
    d = np.zeros(15)
    d[(0 if kind == "p" else 9) + i] = h
    out = list(est)
    out[k] = nm.oplus(est[k], d[:9], d[9:])
    return out


def test_mono_jacobians_against_central_differences():
    """EdgeNavStatePVRPointXYZ: 2 x 9 with respect to the PVR vertex (the V columns zero) and 2 x 3 with respect to the point.  h = 1e-6:
    the truncation error is h^2 |f'''| / 6 ~ 1e-12 x (f / z) x |X|^2, the rounding error 2^-53 |f| / h ~ 1e-7 on errors of a few pixels."""
    sc = vm.make("free2_cov1_p8")
    a = vm.arrays(sc)
    est, X = vm.start(a)
    _, err, _, Jp, Jl = vm.mono(a, est, X)
    h = 1e-6
    assert (Jp[:, :, 3:6] == 0).all()
    for e in range(len(err)):
        k, j = int(a["ekf"][e]), int(a["ept"][e])
        for i in range(9):
            num = (vm.mono(a, perturbed(est, k, "p", i, h), X)[1][e] - vm.mono(a, perturbed(est, k, "p", i, -h), X)[1][e]) / (2 * h)
            assert np.abs(num - Jp[e, :, i]).max() <= 1e-6 * (1 + np.abs(Jp[e]).max()), (e, i)
        for i in range(3):
            d = np.zeros(X.shape)
            d[j, i] = h
            num = (vm.mono(a, est, X + d)[1][e] - vm.mono(a, est, X - d)[1][e]) / (2 * h)
            assert np.abs(num - Jl[e, :, i]).max() <= 1e-6 * (1 + np.abs(Jl[e]).max()), (e, i)


@pytest.mark.parametrize("name", ["depth_forward", "depth_backward"])
def test_inertial_jacobians_against_central_differences(name):
    """EdgeNavStatePVR (9 rows over PVR0, PVR1, Bias0), EdgeNavStateBias (Bias0, Bias1), EdgeNavStateDepthProjected (PVR a, PVR b, Bias c), every
    block.  The reference's Jacobians are first order in the residual's rotation part (JacobianRInv of the residual, not of its
    perturbation): they match differences to the size of that residual, so the states are the scene's start, a centimetre and a
    hundredth of a radian from the truth, and the tolerance is 5 % of the block's scale for the rotation rows and 1e-5 elsewhere.
    EdgeNavStateDepthProjected's Jacobian is the reference's, literally, and it is written for a WORLD-frame position increment and a
    world-frame rotation, not for IncSmallPVR's P += R dP, R = R exp(dPhi): its position columns are held to differences of P[i] += h, its
    velocity columns to the vertex's oplus; its rotation columns (hat(R c) e3)^T and its bias columns ((-R JPg) e3)^T -- a COLUMN of the
    matrix whose third ROW the derivative is -- are not derivatives of the error under the vertices' own increments.  That is the
    reference's behaviour and so the library's; tests/navba_checks.py holds those entries to the formulas."""
    sc = vm.make(name)
    a = vm.arrays(sc)
    est, _ = vm.start(a)
    h = 1e-6
    edges = vm.inertial_edges(a, est)
    assert len(edges) == 2 * len(a["links"]) + len(a["depth"])
    for g, (e, info, delta, blocks) in enumerate(edges):
        for (k, kind), J in blocks:
            for i in range(J.shape[1]):
                if len(e) == 1 and (kind == "b" or i < 3 or i >= 6):
                    if kind == "b" or i >= 6:
                        continue
                    up, dn = [dict(s) for s in est], [dict(s) for s in est]
                    up[k]["P"], dn[k]["P"] = est[k]["P"] + h * np.eye(3)[i], est[k]["P"] - h * np.eye(3)[i]
                    num = (vm.inertial_edges(a, up)[g][0] - vm.inertial_edges(a, dn)[g][0]) / (2 * h)
                    assert abs(num[0] - J[0, i]) <= 1e-5 * (1 + np.abs(J).max()), (name, g, k, i, num, J[0, i])
                    continue
                num = (vm.inertial_edges(a, perturbed(est, k, kind, i, h))[g][0] - vm.inertial_edges(a, perturbed(est, k, kind, i, -h))[g][0]) / (2 * h)
                scale = 1 + np.abs(J).max()
                tol = np.full(len(e), 1e-5 * scale)
                if len(e) == 9:
                    tol[6:9] = 0.05 * scale
                assert (np.abs(num - J[:, i]) <= tol).all(), (name, g, k, kind, i, num, J[:, i])


def test_backward_depth_entry_reads_the_older_links_preintegration():
    sc = vm.make("depth_backward")
    d = sc["depth"][0]
    assert (d["ka"], d["kb"], d["kc"], d["link"]) == (1, 0, 0, 0) and sc["links"][0]["kf1"] == 0 and sc["links"][2]["kf0"] == 1
    f = vm.make("depth_forward")["depth"][0]
    assert (f["ka"], f["kb"], f["kc"], f["link"]) == (1, 0, 0, 1)


def to_ba(sc):
    """The same geometry as tests/ba_model.py takes it: Tcw of every key frame from its state (UpdatePoseFromNS in double, rounded to
    float once), a key frame fixed as here."""
    a = vm.arrays(sc)
    T = np.zeros((len(a["st"]), 12), np.float32)
    for k, v in enumerate(a["st"]):
        s = nm.state_of_vec(v)
        Rwb = nm.rot(nm.qnorm(s["q"]))
        Rcw = (Rwb @ a["Rbc"]).T
        T[k] = np.concatenate([Rcw, (-Rcw @ (Rwb @ a["Pbc"] + s["P"]))[:, None]], 1).reshape(12)
    est = np.zeros((len(T), 7))
    for k, v in enumerate(a["st"]):
        s = nm.state_of_vec(v)
        Rwb = nm.rot(nm.qnorm(s["q"]))
        Rcw = (Rwb @ a["Rbc"]).T
        est[k, :4], est[k, 4:] = nm.q_of_matrix(Rcw), -Rcw @ (Rwb @ a["Pbc"] + s["P"])
    return dict(Tcw=T, fixed=sc["fixed"], points=sc["points"], point_bad=sc["point_bad"], begin=sc["begin"], edge_kf=sc["edge_kf"], edge_obs=sc["edge_obs"],
                edge_inv_sigma2=sc["edge_inv_sigma2"], edge_camera=sc["edge_camera"], cameras=sc["cameras"], mode=bm.LOCAL), est


def test_window_without_inertial_weight_is_the_vision_only_adjustment(monkeypatch):
    """Covariances and random walks of 1e12 leave the inertial edges no weight against the mono edges (information 1e-12 against 1e4):
    the window's poses and points must then be those of tests/ba_model.py on the same geometry.  The two parametrise a pose differently
    (P += R dP, R = R exp(dPhi) against exp(xi) T), so the Levenberg paths differ and only the converged answers meet: both run
    5 + 10 iterations from a centimetre away.  ba_model is handed the poses in double (its own start rounds Tcw to float, which alone
    would move the answer by 1e-5), so the two problems are one in exact arithmetic, and each answer is within its own last accepted step
    of the optimum (the steps shrink at least by half from one to the next near it): the tolerance is the sum of the two last steps."""
    sc = dict(vm.scene(3, 3, 2, 30, vm.sees_all, shifted=0.0, noise=0.1, speed=3.0))       # half a metre between key frames: every depth is well held
    sc["links"] = sc["links"].copy()
    sc["links"]["cov"] = (np.eye(9) * 1e12).reshape(81)
    sc["gyr_rw2"], sc["acc_rw2"] = 1e12, 1e12
    nav = vm.optimize(sc)
    ba_sc, est0 = to_ba(sc)
    monkeypatch.setattr(bm, "start", lambda a: (est0.copy(), a["pts"].astype(np.float64)))      # the poses in double, not rounded to float
    ba = bm.optimize(ba_sc)
    assert nav.n_excluded == 0 and ba.n_removed1 == 0 and nav.n_erased == 0 and ba.n_removed2 == 0
    last = lambda trials: [t for t in trials if t["accepted"]][-1]
    tol = float(np.abs(last(nav.trials)["xl"]).max() + np.abs(last(nav.trials)["xp"]).max() + np.abs(last(ba.trials)["xl"]).max() + np.abs(last(ba.trials)["xp"]).max())
    print("the last accepted steps: tolerance %.3e, points differ by %.3e" % (tol, np.abs(nav.X - ba.X).max()))
    assert tol <= 1e-4 and np.abs(nav.X - ba.X).max() <= tol
    for k, s in enumerate(nav.est):
        R, t = bm.pom.rotation_of(ba.est[k, :4]), ba.est[k, 4:]
        Rwb = nm.rot(s["q"])
        Rcw = (Rwb @ np.asarray(sc["Rbc"]).reshape(3, 3)).T
        tcw = -Rcw @ (Rwb @ np.asarray(sc["Pbc"]) + s["P"])
        assert np.abs(Rcw - R).max() <= tol and np.abs(tcw - t).max() <= tol * (1 + np.abs(t).max()), k
    # and the inertial unknowns no mono edge touches stay where they were
    a = vm.arrays(sc)
    assert np.abs(nav.states[:, 3:6] - a["st"][:, 3:6]).max() <= 1e-6 and np.abs(nav.states[:, 16:] - a["st"][:, 16:]).max() <= 1e-6


def test_excluded_for_its_depth_alone_is_not_erased():
    """returning_depth: the first check excludes the edge of fixed key frame A for its negative depth with a chi2 far below 5.991; the
    second optimize() brings the point in front of A; the final check reads the stored chi2 of round one and the new depth."""
    sc = vm.make("returning_depth")
    r = vm.optimize(sc)
    assert sc["edge_kf"][1] == 3
    c1, c2 = r.checks
    assert c1["depth"][1] < -0.1 and c1["stored"][1] < 1e-2 and r.excluded[1] == 1 and r.n_excluded == 1
    assert c2["depth"][1] > 0.4 and c2["stored"][1] == c1["stored"][1] and r.erased[1] == 0 and r.n_erased == 0
    assert r.iterations == [5, 10]


def test_flagged_point_keeps_kernel_and_level():
    sc = vm.make("specials")
    r = vm.optimize(sc)
    e4 = int(sc["begin"][4])
    assert r.excluded[e4] == 0 and r.erased[e4] == 0 and r.checks[1]["stored"][e4] > 100
    second = [l for l in r.lin if l["round"] == 1]
    assert all(l["rob"][e4] and l["active"][e4] for l in second) and not any(l["rob"][e] for l in second for e in range(len(l["rob"])) if not sc["point_bad"][vm.arrays(sc)["ept"][e]])


def test_threshold_scene_lies_between_the_double_and_the_float_threshold():
    sc = vm.threshold()
    r = vm.optimize(sc)
    e = int(sc["begin"][8])
    stored = float(r.checks[0]["stored"][e])
    assert 5.991 < stored < float(np.float32(5.991)) + 2e-7 and np.float32(stored) == np.float32(5.991) and r.excluded[e] == 1


def test_scene_list_is_the_issues():
    s = vm.SCENES
    a = {n: vm.arrays(s[n]) for n in s}
    assert (a["free1_p8"]["F"], len(a["free1_p8"]["st"]), len(a["free1_p8"]["pts"])) == (1, 2, 8)
    assert (a["free2_cov1_p8"]["F"], len(a["free2_cov1_p8"]["st"])) == (2, 4) and a["fixed_by_id"]["fixed"][0] == 1 and a["fixed_by_id"]["F"] == 2
    lists = a["lists"]
    counts = np.bincount(lists["kf_free"][lists["ekf"]][lists["kf_free"][lists["ekf"]] >= 0])
    assert sorted(counts.tolist()) == sorted(vm.LIST_COUNTS)
    assert [len(a["points_%d" % p]["pts"]) for p in (255, 256, 257)] == [255, 256, 257]
    r = a["realistic"]
    assert (r["F"], len(r["st"]), len(r["pts"]), len(r["depth"])) == (10, 19, 400, 2)
    w = vm.arrays(vm.widest())
    assert w["F"] == 24 and len(w["links"]) == 24
    assert len(vm.packed()) <= 277 * 1024
