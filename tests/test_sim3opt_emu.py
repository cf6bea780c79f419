"""Optimizer::OptimizeSim3 without a GPU: the host build of csrc/sim3opt_core.hpp (tests/emu/sim3opt_emu.cpp, the source
k_sim3_optimize runs, walking the same reduction shape) against the numpy model written from the reference's sources
(tests/sim3opt_model.py), layer by layer as DESIGN.md section 4 states the contract and tests/sim3opt_checks.py derives the bounds.
Nine seeded mutations of the host build (the issue's seven and two in the Levenberg driver) have to fail these same checks."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import host_build
import sim3opt_checks as pc
import sim3opt_model as sm

NAMES = list(sm.SCENES)


@pytest.fixture(scope="module")
def emu(uvo):
    return pc.Emu(uvo)


@pytest.fixture(scope="module")
def runs(emu):
    return {name: emu.optimize(pc.model(name)[0]) for name in NAMES}


def test_new_symbols_are_declared_and_exported(uvo):
    names = ("uvo_sim3_optimizer_create", "uvo_sim3_optimizer_destroy", "uvo_sim3_optimize", "uvo_sim3_optimizer_trace")
    lib = ctypes.CDLL(uvo.LIB_PATH)
    for n in names:
        assert n in uvo.ABI_SYMBOLS and hasattr(lib, n), n
    assert ctypes.sizeof(uvo.Sim3OptProblemC) == 240 and ctypes.sizeof(uvo.Sim3OptResultC) == 144
    assert ctypes.sizeof(uvo.Sim3OptTraceLin) == 296 and ctypes.sizeof(uvo.Sim3OptTraceC) == 8 + 64 + 15 * 296 + 150 * 48
    assert uvo.SIM3OPT_LIN_DTYPE.itemsize == 296 and hasattr(uvo, "Sim3Optimizer")


# ---- the scene list itself, and T and M, on the model alone ---------------------------------------------------------------------------
def test_scene_list_meets_the_conditions_on_the_model_alone():
    res = {n: pc.model(n)[1] for n in NAMES}
    thin = [n for n in NAMES if pc.thin(n)]
    assert not thin, thin                                                     # the cap is 1 in 10; the seeds are chosen so that none is
    assert any(r.n_bad == 0 and r.more_iterations == 5 and not r.early for r in res.values())
    assert any(r.n_bad > 0 and r.more_iterations == 10 for r in res.values())
    l10, l9 = res["left_10"], res["left_9"]
    assert l10.n_correspondences - l10.n_bad == 10 and not l10.early and l9.n_correspondences - l9.n_bad == 9 and l9.early
    assert res["all_bad_12"].n_bad == 12 and res["all_bad_12"].early
    assert res["none_0"].n_correspondences == 0 and res["none_0"].early and not res["none_0"].lin
    # the first step's |sigma| on either side of eps, and the branch it takes
    below, above = res["sigma_below"].trials[0]["dx"], res["sigma_above"].trials[0]["dx"]
    assert 0.5e-5 < abs(below[6]) < 1e-5 < abs(above[6]) < 2e-5
    assert sm.sim_exp(below)[1] in (0, 1) and sm.sim_exp(above)[1] in (2, 3)
    # z == 0 under the map: that pair's e12 has chi2 NaN, it stays and is counted
    z = res["zero_z_30"]
    assert sm.not_finite(z) and sum(sm.not_finite(r) for r in res.values()) == 1
    assert np.isnan(z.checks[0][0][0]) and z.removed[0] == 0 and z.n_inliers == 30 - z.removed.sum() and not z.early
    S0 = sm.sim_from_floats(*[pc.model("zero_z_30")[0][k] for k in ("R12", "t12", "s12")])
    assert S0.map(sm.pairs_of(pc.model("zero_z_30")[0])[:1, 3:6].astype(np.float64))[0, 2] == 0.0
    # bad through e21 alone
    for n in sm.E21_ONLY:
        a, b, live = res[n].checks[0]
        only21 = live & (b > 10) & (a <= 10)
        assert only21.sum() >= 1, n
    # the compared prefix of the trajectory covers the first iteration of the first round: derived on the model alone
    short = []
    for n in NAMES:
        if sm.not_finite(res[n]) or not res[n].trials:
            continue
        k = pc.compared_prefix(n)
        if k < pc.first_iteration_trials(res[n]):
            short.append((n, k))
    assert not short, short
    # GetSigma2 / GetInvSigma2 of octave 3
    sc = pc.model("octave3_60")[0]
    assert np.allclose(sc["info2"] / sc["info1"], 1.2 ** 12, rtol=1e-6) and res["octave3_60"].n_inliers >= 10


def test_recorded_spreads_are_what_the_model_shows():
    """T and M come from the model under 8 permuted pair orders and under projection errors evaluated in mpmath at 50 digits.  The
    measurement over all scenes (`python tests/sim3opt_checks.py`, 90 s) is NOT repeated by the suite; what is repeated is the same
    measurement on the three scenes that set its maxima, so the recorded figures themselves are reproduced here: within the
    recorded spreads, and not below nine tenths of them."""
    est, chi, flips = pc.measure_spread(["plain_65", "all_bad_12", "gross_40"], orders=8, ext=("mp",))
    print("estimate spread %.3e (recorded %.1e), relative chi2 spread %.3e (recorded %.1e), mask changes %d" % (est, pc.EST_SPREAD, chi, pc.CHI2_REL_SPREAD, flips))
    assert 0.9 * pc.EST_SPREAD <= est <= pc.EST_SPREAD and 0.9 * pc.CHI2_REL_SPREAD <= chi <= pc.CHI2_REL_SPREAD and flips == 0
    assert pc.T_EST == 4 * pc.EST_SPREAD and pc.M_REL == 4 * pc.CHI2_REL_SPREAD


# ---- layers 0 to 2 --------------------------------------------------------------------------------------------------------------------
def test_layer0_exp(emu):
    print("worst error / bound: %.3g" % pc.check_exp(emu.exp))
    assert emu.exp(0.0) == 1.0 and abs(emu.exp(1e-9) - emu.exp(-1e-9) - 2e-9) <= 2.0 ** -52


def test_layer1_update_and_maps(emu):
    print("worst difference / bound: %.3g" % pc.check_update(emu.oplus, emu.mats))
    S = np.array([0.1, 0.2, 0.3, 1.2, 1.0, 2.0, 3.0, 1.5])
    assert np.array_equal(emu.oplus(np.zeros(7), S), S)             # Sim3(0) * S is S, and nothing is normalised


def test_start_is_the_models(emu):
    for name in ("plain_30", "zero_z_30", "gross_40"):
        sc = pc.model(name)[0]
        assert np.array_equal(emu.from_floats(sc["R12"], sc["t12"], sc["s12"]), sm.sim_from_floats(sc["R12"], sc["t12"], sc["s12"]).vec()), name
        assert np.array_equal(emu.pairs(sc), sm.pairs_of(sc)), name


@pytest.mark.parametrize("name", [n for n in NAMES if n != "none_0"])
def test_layer2_first_linearisation(emu, name):
    sc, _ = pc.model(name)
    P = emu.pairs(sc)
    sums, _ = emu.linearise(emu.from_floats(sc["R12"], sc["t12"], sc["s12"]), sc, P, np.zeros(len(P), np.uint8))
    print(name, "worst difference / bound: %.3g" % pc.check_linearisation(name, sums))


def test_solve7_against_numpy(emu):
    """Backward stable both: relative difference below 4 n u cond (n = 7)."""
    g = np.random.default_rng(3)
    for _ in range(20):
        A = g.normal(size=(12, 7))
        H, b = A.T @ A, g.normal(size=7)
        ok, x = emu.solve(H[np.triu_indices(7)], 0.3, b)
        want = np.linalg.solve(H + 0.3 * np.eye(7), b)
        assert ok and np.abs(x - want).max() <= 28 * pc.U * np.linalg.cond(H + 0.3 * np.eye(7)) * np.abs(want).max()
    H = np.diag([1.0, 2, 3, -1, 5, 6, 7])
    assert not emu.solve(H[np.triu_indices(7)], 0.0, np.ones(7))[0]
    H[3, 3] = np.nan
    assert not emu.solve(H[np.triu_indices(7)], 0.0, np.ones(7))[0]


# ---- layer 3: the driver ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_layer3_one_trial_on_the_models_own_figures(emu, name):
    print(name, "worst difference / bound: %.3g" % pc.check_trials(emu, name))


@pytest.mark.parametrize("name", NAMES)
def test_layer3_replay_and_trajectory(runs, name):
    n = pc.check_replay(name, runs[name])
    k = pc.check_trajectory(name, runs[name])
    print(name, "replayed", n, "trials exactly; compared", k, "of", len(pc.model(name)[1].trials), "with the model")


# ---- layer 4 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_layer4_the_call(runs, name):
    pc.check_result(name, runs[name])
    r = runs[name]
    assert len(r.trace.lin) <= 15 and len(r.trace.trial) <= 150
    if len(r.trace.lin):
        l = r.trace.lin[0]
        pc.check_linearisation(name, np.concatenate([l["H"], l["b"], [l["chi2"]]]))      # the trace tap shows the same sums


def test_same_call_twice_is_the_same(emu):
    sc = pc.model("gross_40")[0]
    assert not pc.same_run(emu.optimize(sc), emu.optimize(sc))


# ---- the mutations ----------------------------------------------------------------------------------------------------------------------
# which check on which scene has to catch each (DESIGN.md section 4 carries the same table)
CATCH = {
    "FORWARD21": [("lin", "plain_30"), ("res", "plain_30")],
    "ONESIDED": [("lin", "plain_30"), ("res", "shift_30")],
    "ALWAYS10": [("res", "plain_30"), ("res", "octave3_60")],
    "READMIT": [("res", "shift_30"), ("res", "gross_40")],
    "INFO2": [("lin", "octave3_60"), ("res", "octave3_60")],
    "EXP": [("exp", None), ("upd", None), ("res", "plain_30")],
    "WRITEEARLY": [("res", "left_9"), ("res", "all_bad_12")],
    "SCALE": [("trial", "plain_30"), ("trial", "gross_40")],
    "NIONCE": [("replay", "plain_30"), ("replay", "gross_40")],
}


@pytest.mark.parametrize("mutation", list(pc.MUTATIONS))
def test_each_mutation_fails_its_checks(uvo, mutation):
    m = pc.Emu(uvo, mutation)
    for kind, name in CATCH[mutation]:
        with pytest.raises(AssertionError):
            if kind == "exp":
                pc.check_exp(m.exp)
            elif kind == "upd":
                pc.check_update(m.oplus, m.mats)
            elif kind == "trial":
                pc.check_trials(m, name)
            elif kind == "replay":
                pc.check_replay(name, m.optimize(pc.model(name)[0]))
            elif kind == "lin":
                sc = pc.model(name)[0]
                P = m.pairs(sc)
                pc.check_linearisation(name, m.linearise(m.from_floats(sc["R12"], sc["t12"], sc["s12"]), sc, P, np.zeros(len(P), np.uint8))[0])
            else:
                pc.check_result(name, m.optimize(pc.model(name)[0]))
        print(mutation, "caught by", kind, name)


# ---- the stand-alone program --------------------------------------------------------------------------------------------------------------
def test_standalone_program_runs_the_committed_scenes():
    """tests/emu/sim3opt_emu.cpp with its own main (the form that is run under the sanitizers) over tests/golden/sim3opt_scenes.bin:
    the counts it prints for the committed scenes are the model's."""
    fixture = os.path.join(pc.ROOT, "tests", "golden", "sim3opt_scenes.bin")
    out = subprocess.run([host_build.build("sim3opt_emu_main"), fixture], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-2000:] + out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("scene ")]
    assert len(lines) == len(NAMES)
    for line, name in zip(lines, NAMES):
        r = pc.model(name)[1]
        w = line.split()
        assert int(w[3].rstrip(":")) == r.n_correspondences and (int(w[5]), int(w[7]), int(w[9])) == (r.n_inliers, r.n_bad, r.more_iterations), (name, line)
