"""The numpy model of the bundle adjustment (tests/ba_model.py) held to hand-computed cases, to the Gauss-Newton step of the full
unreduced system, and its scene list to the conditions the other tests rely on -- all on the model alone, no library involved."""
import os

import numpy as np

import ba_model as bm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def hand_scene():
    """One free key frame at the identity (and a fixed one without an edge), one point at (0, 0, 2), one edge: fx = fy = 100, cx = cy = 0,
    observation (1, 0), information 1."""
    I = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]
    return dict(Tcw=np.float32([I, I]), fixed=np.uint8([0, 1]), points=np.float32([[0, 0, 2]]), point_bad=np.uint8([0]), begin=np.int32([0, 1]),
                edge_kf=np.int32([0]), edge_obs=np.float32([[1, 0]]), edge_inv_sigma2=np.float32([1]), edge_camera=np.int32([0]), cameras=np.float32([[100, 100, 0, 0]]))


def test_one_edge_by_hand():
    a = bm.arrays(hand_scene())
    est, X = bm.start(a)
    assert np.array_equal(est, [[0, 0, 0, 1, 0, 0, 0]] * 2) and np.array_equal(X, [[0, 0, 2]])
    S = bm.System(a, est, X, np.ones(1, bool))
    # the point in the camera is (0, 0, 2): it projects to (0, 0), the error is (1, 0), chi2 = 1, inside the Huber radius
    assert np.array_equal(S.err, [[1, 0]]) and S.chi2[0] == 1.0 and S.robust == 1.0
    assert np.array_equal(S.Jp[0], [[0, -100, 0, -50, 0, 0], [100, 0, 0, 0, -50, 0]])
    assert np.array_equal(S.Jl[0], [[-50, 0, 0], [0, -50, 0]])
    W = np.zeros((6, 3))
    W[1, 0], W[3, 0], W[0, 1], W[4, 1] = 5000, 2500, -5000, 2500
    assert np.array_equal(S.W[0], W)
    assert np.array_equal(S.Hll[0], np.diag([2500.0, 2500.0, 0.0])) and np.array_equal(S.bl[0], [50, 0, 0])
    Hpp = np.zeros((6, 6))
    Hpp[0, 0] = Hpp[1, 1] = 10000
    Hpp[3, 3] = Hpp[4, 4] = 2500
    Hpp[1, 3] = Hpp[3, 1] = 5000
    Hpp[0, 4] = Hpp[4, 0] = -5000
    assert np.array_equal(S.Hpp[0], Hpp) and np.array_equal(S.bp[0], [0, 100, 0, 50, 0, 0])
    assert S.max_diagonal() == 10000.0 and S.max_diagonal(poses_only=True) == 10000.0
    ok, xp, xl = S.trial(1.0)
    assert ok
    Dinv = np.diag([1 / 2501.0, 1 / 2501.0, 1.0])
    assert np.allclose(S.Dinv[0], Dinv, rtol=1e-15, atol=0)
    want = Hpp + np.eye(6) - W @ Dinv @ W.T
    assert np.allclose(S.Hs[0, 0], want, rtol=1e-13, atol=1e-9)
    assert abs(S.Hs[0, 0][1, 1] - (10001 - 25e6 / 2501)) < 1e-9
    bs = np.array([0, 100, 0, 50, 0, 0]) - W @ Dinv @ np.array([50.0, 0, 0])
    assert np.allclose(S.bs[0], bs, rtol=1e-13, atol=1e-12)
    assert np.allclose(xp[0], np.linalg.solve(want, bs), rtol=1e-9) and np.allclose(xl[0], Dinv @ (np.array([50.0, 0, 0]) - W.T @ xp[0]), rtol=1e-9)


def test_fixed_key_frame_contributes_no_block_but_the_point_keeps_its_terms():
    sc = hand_scene()
    sc["edge_kf"] = np.int32([1])
    a = bm.arrays(sc)
    est, X = bm.start(a)
    S = bm.System(a, est, X, np.ones(1, bool))
    assert not S.Hpp.any() and not S.bp.any() and not S.f_on.any()
    assert np.array_equal(S.Hll[0], np.diag([2500.0, 2500.0, 0.0])) and S.p_on[0]
    ok, xp, xl = S.trial(1.0)
    assert ok and not xp.any() and np.allclose(xl[0], [50 / 2501.0, 0, 0], rtol=1e-14)


def test_small_lambda_gives_the_gauss_newton_step_of_the_full_system():
    """With lambda -> 0 and exact data the reduced solve's step is the step of the full system [[Hpp, W], [W^T, Hll]] solved densely."""
    sc = bm.scene(31, 2, 1, 10, bm.sees_all, shifted=0.0, noise=0.0)
    a = bm.arrays(sc)
    est, X = bm.start(a)
    E = len(a["ekf"])
    S = bm.System(a, est, X, np.ones(E, bool))
    F, P = a["F"], len(X)
    n = 6 * F + 3 * P
    H, b = np.zeros((n, n)), np.zeros(n)
    for f in range(F):
        H[6 * f:6 * f + 6, 6 * f:6 * f + 6] = S.Hpp[f]
        b[6 * f:6 * f + 6] = S.bp[f]
    for j in range(P):
        o = 6 * F + 3 * j
        H[o:o + 3, o:o + 3] = S.Hll[j]
        b[o:o + 3] = S.bl[j]
    for e in range(E):
        f, o = S.f[e], 6 * F + 3 * a["ept"][e]
        if f >= 0:
            H[6 * f:6 * f + 6, o:o + 3] += S.W[e]
            H[o:o + 3, 6 * f:6 * f + 6] += S.W[e].T
    # both are solves of the same system: each is off by about kappa x the unit roundoff x the growth of a dense elimination of order n.
    # The smaller lambda, the worse the conditioning (a point's depth is weakly seen), so the identity is held at three lambdas.
    for rel_lam in (1e-4, 1e-8, 1e-12):
        lam = rel_lam * S.max_diagonal()
        ok, xp, xl = S.trial(lam)
        assert ok
        x = np.linalg.solve(H + lam * np.eye(n), b)
        step = np.concatenate([xp.ravel(), xl.ravel()])
        kappa = np.linalg.cond(H + lam * np.eye(n))
        print("lambda %.1e max: kappa %.3g, difference %.3g" % (rel_lam, kappa, np.abs(step - x).max() / np.abs(x).max()))
        assert np.abs(step - x).max() <= 2 * n * kappa * 2.0 ** -53 * np.abs(x).max(), (rel_lam, np.abs(step - x).max())
    # and the step is the way to the truth: the error falls by orders of magnitude
    est2, X2 = bm.apply(a, est, X, xp, xl, S)
    assert bm.edge_errors(a, est2, X2)[2].sum() < 1e-3 * S.chi2.sum()


def test_committed_scene_list_is_the_generators():
    with open(os.path.join(ROOT, "tests", "golden", "ba_scenes.bin"), "rb") as fh:
        assert fh.read() == bm.packed()
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "ba_scenes.bin")) <= 160 * 1024


def test_scene_list_meets_its_conditions_on_the_model_alone():
    res = {}
    with np.errstate(all="ignore"):
        for n in bm.SCENES:
            res[n] = bm.optimize(bm.SCENES[n])
    assert any(any(not t["accepted"] and t["ok"] for t in r.trials) for r in res.values())          # a rejected trial
    assert any(r.n_removed1 > 0 for r in res.values())
    assert any(r.n_removed2 > 0 and not (r.removed1 & r.removed2).any() for r in res.values())      # removed2 beyond removed1
    assert any(any(not t["ok"] for t in r.trials) for r in res.values())                            # a failed solve: zero_depth
    z = res["zero_depth"]
    assert [t["ok"] for t in z.trials[:5]] == [False] * 5 and all(t["tmp"] == bm.DBL_MAX for t in z.trials[:5]) and z.removed1[0] == 1
    assert all(t["ok"] for t in z.trials[5:]) and z.iterations == [5, 10]
    sp, sc = res["specials"], bm.SCENES["specials"]
    b = sc["begin"]
    assert b[1] - b[0] == 1 and all(sc["fixed"][sc["edge_kf"][e]] for e in range(b[1], b[2]))          # a single edge; seen only from fixed key frames
    assert sp.removed1[b[2]:b[3]].all()                                                              # every edge of point 2 goes in the first check
    r1 = [l for l in sp.lin if l["round"] == 1]
    assert np.array_equal(sp.X[2], r1[0]["X"][2]) and sp.lin[0]["n_points"] == 8 and r1[0]["n_points"] < 8    # it drops out and keeps its estimate
    assert sp.removed1[b[3]:b[4]].all() and (sp.checks[0]["depth"][b[3]:b[4]] < 0).all()               # negative depth
    assert not sp.removed1[b[4]:b[5]].any() and not sp.removed2[b[4]:b[5]].any() and sp.checks[0]["stored"][b[4]] > 100     # flagged bad: it survives
    lk = res["lonely_keyframe"]
    assert lk.lin[0]["n_free"] == 3 and [l for l in lk.lin if l["round"] == 1][0]["n_free"] == 2
    k2 = np.flatnonzero(bm.SCENES["lonely_keyframe"]["fixed"] == 0)[2]
    assert np.array_equal(lk.est[k2], [l for l in lk.lin if l["round"] == 1][0]["est"][k2])
    ls = bm.SCENES["lists"]
    assert sorted(np.bincount(ls["edge_kf"], minlength=8)[:7].tolist()) == sorted(bm.LIST_COUNTS)
    assert res["full_20"].iterations[1] == 0 and res["full_20"].n_removed1 == 0
    first = bm.SCENES["kf3_first_fixed"]
    assert first["fixed"].tolist() == [1, 0, 0]
