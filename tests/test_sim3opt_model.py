"""tests/sim3opt_model.py held to cases that can be computed by hand or by other means: the four branches of the exponential against
the matrix exponential's series, inverse(), one numeric Jacobian column against the analytic derivative to what a 1e-9 central
difference allows, the Huber kernel's root, and the early return."""
import math

import numpy as np

import sim3opt_model as sm

U = 2.0 ** -53


def _expm(A, terms=40):
    out, term = np.eye(len(A)), np.eye(len(A))
    for k in range(1, terms):
        term = term @ A / k
        out = out + term
    return out


def _branch_case(omega, sigma):
    return np.array(list(omega) + [0.3, -0.2, 0.1, sigma])


CASES = {0: _branch_case([0.5e-5, -0.3e-5, 0.2e-5], 0.9e-5), 1: _branch_case([0.05, -0.08, 0.03], -0.9e-5),
         2: _branch_case([0.5e-5, -0.3e-5, 0.2e-5], 0.05), 3: _branch_case([0.05, -0.08, 0.03], -0.05)}


def test_the_four_branches_of_the_exponential_are_the_matrix_exponential():
    """exp of [[Omega + sigma I, upsilon], [0, 0]] is [[s R, t], [0, 1]].  The small-angle branches replace R by I + Omega + Omega^2,
    off by theta^2 / 2 at the most in Omega^2's place: 2.5e-11 at these cases; the coefficient formulas cancel to 1e-11 at |sigma|
    = 1e-5 (see update_bound in sim3opt_checks.py).  1e-10 separates all of that from a wrong branch or coefficient (1e-6 and more)."""
    for br, dx in CASES.items():
        S, took = sm.sim_exp(dx)
        assert took == br
        A = np.zeros((4, 4))
        A[:3, :3] = sm.skew(dx[:3]) + dx[6] * np.eye(3)
        A[:3, 3] = dx[3:6]
        E = _expm(A)
        assert np.abs(S.s * sm.rot_of(S.q) - E[:3, :3]).max() < 1e-10, br
        # with |sigma| < eps the reference takes C = 1 for (s - 1) / sigma = 1 + sigma / 2 + ...: t is off by |sigma| / 2 |upsilon|, its own
        # approximation; the wrong branch would be off by |sigma| |upsilon| / 2 * 1e4 there
        tol_t = 1e-10 + (0.51 * abs(dx[6]) * np.abs(dx[3:6]).max() if abs(dx[6]) < 1e-5 else 0.0)
        if br == 2:
            # sim3.h:116 has B = (sigma^2 / 2 - sigma + 1) s / sigma^3 where the integral gives ((sigma^2 / 2 - sigma + 1) s - 1) / sigma^3:
            # the reference's B is too large by 1 / sigma^3, which reaches t through Omega^2 (theta^2) and upsilon.  The model keeps it.
            tol_t += float(dx[:3] @ dx[:3]) * np.abs(dx[3:6]).sum() / abs(dx[6]) ** 3
        assert np.abs(S.t - E[:3, 3]).max() < tol_t, br
        assert abs(S.s - math.exp(dx[6])) == 0.0


def test_either_side_of_eps_takes_its_branch():
    for sigma, theta, br in ((0.99e-5, 0.99e-5, 0), (1.01e-5, 0.99e-5, 2), (0.99e-5, 1.01e-5, 1), (-1.01e-5, 1.01e-5, 3), (1e-9, 0.0, 0), (0.0, 1e-9, 0)):
        assert sm.sim_exp([theta, 0, 0, 0.1, 0.2, 0.3, sigma])[1] == br, (sigma, theta)


def test_the_quaternion_is_never_normalised():
    S = sm.Sim([0.1, 0.2, 0.3, 1.2], [1, 2, 3], 1.5)     # |q| = 1.26
    P = sm.oplus(np.zeros(7), S)
    assert np.array_equal(P.q, S.q) and np.array_equal(P.t, S.t) and P.s == S.s
    X = np.array([[0.3, -0.4, 2.0]])
    assert np.abs(S.map(X) - (1.5 * X @ sm.rot_of(S.q).T + [1, 2, 3])).max() < 1e-14    # Eigen's q * v is toRotationMatrix() * v for any q


def test_inverse():
    S = sm.Sim(sm.quat_of(sm.rot_of_vec(np.array([0.3, -0.2, 0.5]))), [0.4, -1.0, 2.0], 1.3)
    I = S.inverse()
    assert np.array_equal(I.q, S.q * [-1, -1, -1, 1]) and I.s == 1 / 1.3
    assert np.abs(I.t - (-(1 / 1.3) * sm.rot_of(S.q).T @ S.t)).max() < 1e-15
    X = np.array([[0.7, -1.1, 5.0], [2.0, 0.1, 3.0]])
    assert np.abs(I.map(S.map(X)) - X).max() < 1e-14
    P = S * I
    assert np.abs(P.vec() - [0, 0, 0, 1, 0, 0, 0, 1]).max() < 1e-15


def test_sim3_from_floats_is_eigens_quaternion_of_the_widened_matrix():
    R = sm.rot_of_vec(np.array([2.5, 0.3, -0.2])).astype(np.float32)       # trace < 0: the other branch
    assert float(np.trace(R)) < 0
    S = sm.sim_from_floats(R, [1, 2, 3], np.float32(1.1))
    assert np.abs(sm.rot_of(S.q) - R.astype(np.float64)).max() < 1e-6 and S.s == float(np.float32(1.1))
    assert abs(np.linalg.norm(S.q) - 1) < 1e-6 and abs(np.linalg.norm(S.q) - 1) > 0    # close to unit, and left as it falls


def test_a_numeric_jacobian_column_against_the_analytic_derivative():
    """Column 3 (upsilon_x): Sim3(d e_3) * S moves t by d e_x and nothing else (W = I), so e12's column is -(fx / z, 0) and e21's
    is the inverse map's: X' = (1 / s) R^T (X - t), dX'/dt_x = -(1 / s) R^T e_x, through the projection.
    What 1e-9 differencing allows: each error carries a rounding error of a few u times its largest intermediate (about 500 px),
    1e-13; the difference of two, times 5e8: 1e-4.  The bound below is that: 2 * 32 u (f |x / z| + |pp| + |obs|) * 5e8.  The
    truncation error of the central difference, f''' d^2 / 6, is 1e-18."""
    sc = sm.make("plain_30")
    P = sm.pairs_of(sc).astype(np.float64)
    S = sm.sim_from_floats(sc["R12"], sc["t12"], sc["s12"])
    K1, K2 = [float(v) for v in sc["kf1"][2]], [float(v) for v in sc["kf2"][2]]
    J12, J21 = sm.numeric_jacobians(S, sm.pairs_of(sc), sc["kf1"][2], sc["kf2"][2])
    Y = S.map(P[:, 3:6])
    bound = lambda f, pp, ratio, obs: 2 * 32 * U * (f * np.abs(ratio) + abs(pp) + np.abs(obs)) * 5e8
    assert (np.abs(J12[:, 0, 3] - (-K1[0] / Y[:, 2])) <= bound(K1[0], K1[2], Y[:, 0] / Y[:, 2], P[:, 6])).all()
    assert (np.abs(J12[:, 1, 3]) <= bound(K1[1], K1[3], Y[:, 1] / Y[:, 2], P[:, 7])).all()
    Z = S.inverse().map(P[:, 0:3])
    d = -(1 / S.s) * sm.rot_of(S.q).T[:, 0]          # dX' / dt_x
    a0 = -K2[0] * (d[0] / Z[:, 2] - Z[:, 0] * d[2] / Z[:, 2] ** 2)
    a1 = -K2[1] * (d[1] / Z[:, 2] - Z[:, 1] * d[2] / Z[:, 2] ** 2)
    assert (np.abs(J21[:, 0, 3] - a0) <= bound(K2[0], K2[2], Z[:, 0] / Z[:, 2], P[:, 8])).all()
    assert (np.abs(J21[:, 1, 3] - a1) <= bound(K2[1], K2[3], Z[:, 1] / Z[:, 2], P[:, 9])).all()
    assert np.abs(J12[:, 0, 3]).min() > 10      # the columns are not noise: fx / z is 50 and more


def test_huber_delta_is_the_float_root_and_either_root_gives_it():
    for th2 in (10.0, 5.991, 7.815, 0.3, 123.456):
        f = np.float32(th2)
        assert sm.delta_of(th2) == float(np.sqrt(f)) == float(np.float32(math.sqrt(float(f))))
    rho0, rho1 = sm.huber(np.array([4.0, 10.0, 40.0]), sm.delta_of(10.0))
    d = sm.delta_of(10.0)
    assert rho0[0] == 4.0 and rho1[0] == 1.0 and rho0[1] == 10.0 and rho1[1] == 1.0          # float(sqrt(10))^2 > 10: still the quadratic side
    assert rho0[2] == 2 * math.sqrt(40.0) * d - d * d and rho1[2] == d / math.sqrt(40.0)


def test_the_early_return_leaves_the_similarity_and_nulls_the_bad():
    sc = sm.make("left_9")
    r = sm.optimize(sc)
    S0 = sm.sim_from_floats(sc["R12"], sc["t12"], sc["s12"])
    assert r.early and r.n_inliers == 0 and r.n_correspondences - r.n_bad == 9 and r.more_iterations == 0
    assert np.array_equal(r.S.vec(), S0.vec()) and r.removed.sum() == r.n_bad == 4 and len(r.lin) == 5
    e = sm.optimize(sm.make("none_0"))
    assert e.early and e.n_inliers == 0 and not e.lin and not e.trials and len(e.removed) == 0


def test_exactly_ten_left_runs_the_second_round_with_ten_iterations():
    r = sm.optimize(sm.make("left_10"))
    assert not r.early and r.n_correspondences - r.n_bad == 10 and r.more_iterations == 10 and r.n_inliers == 10
    assert max(l["round"] for l in r.lin) == 1


def test_removed_pairs_never_come_back():
    sc = sm.make("gross_40")
    r = sm.optimize(sc)
    first = r.checks[0]
    bad0 = first[2] & ((first[0] > 10) | (first[1] > 10))
    assert bad0.sum() == r.n_bad == 8 and not (r.checks[1][2] & bad0).any() and (r.removed[bad0] == 1).all()


def test_dump_is_the_committed_fixture():
    import os
    import tempfile
    here = os.path.dirname(os.path.abspath(__file__))
    with tempfile.TemporaryDirectory() as d:
        sm.dump(os.path.join(d, "s.bin"))
        assert open(os.path.join(d, "s.bin"), "rb").read() == open(os.path.join(here, "golden", "sim3opt_scenes.bin"), "rb").read()
    got = sm.load(os.path.join(here, "golden", "sim3opt_scenes.bin"))
    assert len(got) == len(sm.SCENES) and np.array_equal(got[2][0], sm.pairs_of(sm.make(list(sm.SCENES)[2])))
