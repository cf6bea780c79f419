"""The visual-inertial pose optimisation without a GPU: the host build of csrc/navopt_core.hpp (tests/emu/navopt_emu.cpp, the source
k_nav_optimize runs, walking the same reduction shape) against the numpy model written from the reference's sources
(tests/navopt_model.py), layer by layer as DESIGN.md section 4 states the contract and tests/navopt_checks.py derives the bounds:
1 each edge's error and Jacobian, 2 the first linearisation, 3 one trial, 4 the driver replayed on the trace, 5 the result over the
derived prefix, 6 the marginals.  Ten seeded mutations of the host build each fail them."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import host_build
import navopt_checks as nc
import navopt_model as nm

NAMES = list(nm.SCENES)


@pytest.fixture(scope="module")
def emu(uvo):
    return nc.Emu(uvo)


@pytest.fixture(scope="module")
def runs(emu):
    return {name: emu.optimize(nc.model(name)[0]) for name in NAMES}


def test_new_symbols_are_declared_and_exported(uvo):
    names = ("uvo_nav_optimizer_create", "uvo_nav_optimizer_destroy", "uvo_nav_optimize", "uvo_nav_optimizer_trace")
    lib = ctypes.CDLL(uvo.LIB_PATH)
    header = open(os.path.join(nc.ROOT, "include", "uvo", "uvo.h")).read()
    for n in names:
        assert n in uvo.ABI_SYMBOLS and hasattr(lib, n) and n + "(" in header, n
    assert ctypes.sizeof(uvo.NavStateC) == 176 and ctypes.sizeof(uvo.NavTraceLin) == 8 + 496 * 8
    assert ctypes.sizeof(uvo.NavTraceC) == 8 + 40 * ctypes.sizeof(uvo.NavTraceLin) + 400 * 48 and uvo.NAV_LIN_DTYPE.itemsize == ctypes.sizeof(uvo.NavTraceLin)
    assert ctypes.sizeof(uvo.NavProblemC) == nm.PROBLEM_DTYPE.itemsize - 8 + 48      # the device record's off and pad for the six pointers
    assert hasattr(uvo, "NavOptimizer") and (uvo.NAV_KEYFRAME, uvo.NAV_FRAME) == (nm.KEYFRAME, nm.FRAME)


def test_so3_against_the_model(emu):
    g = np.random.default_rng(11)
    for th in (1e-12, 1e-7, 1e-3, 0.3, 2.0, 3.0):
        v = g.normal(size=3)
        v = v / np.linalg.norm(v) * th
        q = nm.so3_exp(v)
        assert np.abs(emu.so3(0, v, 4) - q).max() <= 16 * nc.U                       # sin, cos: 4 u absolute each; one normalisation
        assert np.abs(emu.so3(1, q, 3) - nm.so3_log(q)).max() <= 64 * nc.U * max(1.0, th)
        assert np.abs(emu.so3(2, v, 9).reshape(3, 3) - nm.so3_jr(v)).max() <= 64 * nc.U
        # 1 - (1 + cos) theta / (2 sin): the quotient's relative error 12 u is absolute on a value near 1
        assert np.abs(emu.so3(3, v, 9).reshape(3, 3) - nm.so3_jrinv(v)).max() <= 64 * nc.U * (1 + th / abs(np.sin(th)))
    q = nm.so3_exp(np.array([0.0, 0.0, 4.0]))                                         # w < 0
    assert np.abs(emu.so3(1, q, 3) - nm.so3_log(q)).max() <= 64 * nc.U


# ---- layers 1 to 3 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["kf_plain_64", "fr_plain_65", "kf_depth_marg_30", "fr_depth_marg_30", "fr_shift_100", "kf_bias_step_100", "fr_few_5", "kf_degenerate_50"])
def test_layer1_edges(emu, name):
    nc.check_edges(emu, name)


# the degenerate scenes' sums are NaN: compared by class in layer 4 (the model also multiplies the zero columns of a NaN Jacobian)
@pytest.mark.parametrize("name", [n for n in NAMES if "too_few" not in n and "degenerate" not in n])
def test_layer2_first_linearisation(emu, name):
    sc, res = nc.model(name)
    R = res.lin[0]
    H, b, chi = emu.linearise(sc, R["est"], R["active"], R["robust"])
    nc.check_linearisation(name, H, b, chi)


@pytest.mark.parametrize("name", ["kf_shift_150", "fr_shift_150"])
def test_layer2_with_inactive_edges_and_without_the_kernel(emu, name):
    """Later rounds' linearisations: the model's estimates and active sets, the skipped edges leaving the shape as it is; in round 3 the
    reprojection edges have lost their kernel and the single edges have kept theirs."""
    sc, res = nc.model(name)
    for rnd in (2, 3):
        j = [j for j, L in enumerate(res.lin) if L["round"] == rnd][0]
        R = res.lin[j]
        assert 0 < R["active"][0].sum() < len(sc["edges"]) and R["robust"] == (rnd < 3)
        H, b, chi = emu.linearise(sc, R["est"], R["active"], R["robust"])
        nc.check_linearisation(name, H, b, chi, j)


@pytest.mark.parametrize("name", ["kf_plain_20", "kf_plain_257", "fr_plain_100", "fr_shift_60", "kf_depth_marg_30", "fr_bias_step_100"])
def test_layer3_trial(emu, name):
    for trial in (0, 1, 2):
        print(name, trial, "dx bound %.3g, tmp bound %.3g" % nc.check_trial(emu, name, trial))


def test_layer3_failed_solve_keeps_the_previous_step(emu):
    sc, res = nc.model("kf_plain_20")
    R = res.lin[0]
    prev = np.arange(15) * 1e-4
    ok, dx, est1, (tmp, scale) = emu.trial(sc, R["est"], R["active"], True, -np.eye(15), np.ones(15), 0.5, dx_prev=prev)
    assert not ok and dx.tolist() == prev.tolist() and tmp == nm.DBL_MAX
    ok, dx, est1, (tmp, scale) = emu.trial(sc, R["est"], R["active"], True, np.full((15, 15), np.nan), np.ones(15), 0.5)
    assert not ok and not dx.any() and scale == 1e-3 and tmp == nm.DBL_MAX and (nm.state_vec(est1[0]) == nm.state_vec(R["est"][0])).all()


# ---- layers 4, 5 and 6 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_layers_4_5_and_6(runs, name):
    k = nc.check_all(name, runs[name])
    print(name, "compared prefix", k, "of", len(nc.model(name)[1].trials), "trials; thin" if nc.thin(name) else "trials")


def test_layer6_marginals_of_a_given_matrix(emu):
    for name in ("kf_depth_marg_30", "fr_depth_marg_30"):
        sc, res = nc.model(name)
        ok, cov, inv = emu.marginals(sc, res.H_last)
        assert ok
        c1 = float(np.linalg.cond(res.H_last)) * nc.solver_factor(nm.nd_of(sc))
        assert np.abs(cov - res.marg_cov).max() <= c1 * np.abs(res.marg_cov).max()
        assert (inv[:9, 9:] == 0).all() == (sc["form"] == nm.KEYFRAME)
        prod = inv @ res.marg_cov if sc["form"] == nm.FRAME else np.block([[inv[:9, :9] @ res.marg_cov[:9, :9], np.zeros((9, 6))], [np.zeros((6, 9)), inv[9:, 9:] @ res.marg_cov[9:, 9:]]])
        assert np.abs(prod - np.eye(15)).max() <= (float(np.linalg.cond(res.marg_cov)) * nc.solver_factor(15) + c1) * 15
    ok, cov, inv = emu.marginals(nc.model("kf_depth_marg_30")[0], -np.eye(15))
    assert not ok


def test_non_finite_values_follow_the_arithmetic(runs):
    for name in ("kf_degenerate_50", "fr_degenerate_50"):
        run, (sc, res) = runs[name], nc.model(name)
        assert np.isnan(run.trace.lin["chi2"]).all() and not run.trace.trial["ok"].any() and (run.trace.trial["tmp"] == nm.DBL_MAX).all()
        assert run.outlier[0][0] == 0 and all(a.tobytes() == b.tobytes() for a, b in zip(run.outlier, res.outlier))      # `else`: a NaN chi2 is an inlier
        assert run.marg_ok == 0 and (nm.state_vec(run.ns) == nm.state_vec(nc.start_of(sc)[0])).all()


def test_host_build_repeats_itself(emu, runs):
    for name in ("kf_shift_100", "fr_plain_256", "fr_degenerate_50"):
        again = emu.optimize(nc.model(name)[0])
        assert nm.state_vec(again.ns).tobytes() == nm.state_vec(runs[name].ns).tobytes() and again.trace.trial.tobytes() == runs[name].trace.trial.tobytes()
        assert again.trace.lin.tobytes() == runs[name].trace.lin.tobytes() and again.marg_cov_inv.tobytes() == runs[name].marg_cov_inv.tobytes()


# ---- the stand-alone program -----------------------------------------------------------------------------------------------------------
def test_stand_alone_program_runs_the_committed_scene_list():
    """tests/emu/navopt_emu.cpp with its own main (the form that is run under the sanitizers) over tests/golden/navopt_scenes.bin: the
    program's counts are the model's."""
    fixture = os.path.join(nc.ROOT, "tests", "golden", "navopt_scenes.bin")
    r = subprocess.run([host_build.build("navopt_emu_main"), fixture], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rows = re.findall(r"^scene (\d+) form (\d) n (\d+) \+ (\d+) inliers (\d+) rounds (\d+)", r.stdout, re.M)
    assert len(rows) == len(NAMES)
    for name, (_, form, n, nl, inl, rounds) in zip(NAMES, rows):
        sc, res = nc.model(name)
        assert (int(form), int(n), int(rounds)) == (sc["form"], len(sc["edges"]), res.rounds) and (nc.thin(name) or int(inl) == res.n_inliers), (name, n, inl, rounds)


# ---- the seeded mutations ---------------------------------------------------------------------------------------------------------------
def _fails(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


# the scenes each mutation is shown on (a mutation need not show on every scene: the depth edge exists only where has_depth is set, and
# in the key-frame form no edge joins the frame's PVR and bias vertices, so H is block diagonal and the joint inverse IS the two blocks')
SHOWN_ON = {"NO_RESET": ["kf_plain_20", "fr_plain_20"], "BREAK_ACTIVE": ["kf_none_left_12", "fr_none_left_12"], "IMU_NO_KERNEL": ["kf_plain_20", "fr_plain_20"],
            "DEPTH_SWAP": ["fr_depth_marg_30", "fr_depth_only_80"], "DEPTH_HALF": ["kf_depth_marg_30", "fr_depth_marg_30"], "MARG_FRESH": ["fr_depth_marg_30", "fr_shift_150"],
            "MARG_SWAP": ["fr_depth_marg_30", "fr_marg_only_80"], "ORDER": ["kf_plain_20", "fr_plain_20"], "HUBER_B": ["kf_plain_20", "fr_plain_20"],
            "JRINV": ["kf_plain_20", "fr_plain_20"]}


@pytest.mark.parametrize("mutation", sorted(nc.MUTATIONS))
def test_seeded_mutations_fail_the_checks(uvo, mutation):
    m = nc.Emu(uvo, mutation)
    caught = []
    for name in SHOWN_ON[mutation]:
        sc, res = nc.model(name)

        def checks():
            nc.check_edges(m, name)
            nc.check_trial(m, name, 0)
            nc.check_all(name, m.optimize(sc))
        if _fails(checks):
            caught.append(name)
    print(mutation, "caught on", caught)
    assert caught == SHOWN_ON[mutation], mutation
