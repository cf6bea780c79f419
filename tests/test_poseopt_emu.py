"""Optimizer::PoseOptimization without a GPU: the host build of csrc/poseopt_core.hpp (tests/emu/poseopt_emu.cpp, the source
k_pose_optimize runs, walking the same reduction shape) against the numpy model written from the reference's sources
(tests/poseopt_model.py), layer by layer as DESIGN.md section 4 states the contract and tests/poseopt_checks.py derives the bounds.
Six seeded mutations of the host build have to fail these same checks."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import host_build
import poseopt_checks as pc
import poseopt_model as pm

NAMES = list(pm.SCENES)


@pytest.fixture(scope="module")
def emu(uvo):
    return pc.Emu(uvo)


@pytest.fixture(scope="module")
def runs(emu):
    return {name: emu.optimize(pc.model(name)[0]) for name in NAMES}


def test_new_symbols_are_declared_and_exported(uvo):
    names = ("uvo_pose_optimizer_create", "uvo_pose_optimizer_destroy", "uvo_pose_optimize", "uvo_pose_optimizer_trace")
    lib = ctypes.CDLL(uvo.LIB_PATH)
    for n in names:
        assert n in uvo.ABI_SYMBOLS and hasattr(lib, n), n
    assert ctypes.sizeof(uvo.PoseProblemC) == 112 and ctypes.sizeof(uvo.PoseResultC) == 88
    assert ctypes.sizeof(uvo.PoseTraceLin) == 232 and ctypes.sizeof(uvo.PoseTraceTrial) == 48 and ctypes.sizeof(uvo.PoseTraceC) == 8 + 96 + 32 * 232 + 320 * 48
    assert uvo.POSE_LIN_DTYPE.itemsize == 232 and uvo.POSE_TRIAL_DTYPE.itemsize == 48
    assert hasattr(uvo, "PoseOptimizer")


# ---- the scene list itself, on the model alone ----------------------------------------------------------------------------------------
def test_scene_list_meets_the_conditions_on_the_model_alone():
    assert len(NAMES) >= 30
    thin, short = [n for n in NAMES if pc.thin(n)], []
    assert len(thin) * 10 <= len(NAMES), thin                      # the cap: at most 1 scene in 10 skipped for a thin margin
    for name in NAMES:
        _, res = pc.model(name)
        if pc.not_finite(res) or not res.trials:
            continue
        k = pc.compared_prefix(name)
        if k < max(5, pc.first_iteration_trials(res)) and k < len(res.trials):
            short.append((name, k))
    assert not short, short                                         # the whole first iteration of round 0 and at least 5 trials
    assert sum(pc.not_finite(pc.model(n)[1]) for n in NAMES) == 1   # the one scene whose decisions are made by class
    assert any(pm.reentries(pc.model(n)[1]) for n in pm.REENTRY)
    _, r = pc.model("thin_12")
    assert len(pc.model("thin_12")[0][0]) >= 10 and r.active_after[0] < 10 and r.rounds == 4
    assert pc.model("few_9")[1].rounds == 1 and pc.model("none_left_12")[1].active_after[0] == 0


def test_recorded_spreads_are_what_the_model_shows():
    """T and M come from the model under permuted edge orders.  The full measurement is the one DESIGN.md section 4 records; here a
    part of it is repeated, and has to stay within the recorded spreads."""
    pose, chi, flips = pc.measure_spread(["plain_64", "shift_100_3", "thin_12", "plain_1000", "gross_40"], orders=4)
    print("pose spread %.3e (recorded %.1e), chi2 spread %.3e (recorded %.1e), mask changes %d" % (pose, pc.POSE_SPREAD, chi, pc.CHI2_SPREAD, flips))
    assert pose <= pc.POSE_SPREAD and chi <= pc.CHI2_SPREAD and flips == 0
    assert pc.T_POSE == 4 * pc.POSE_SPREAD and pc.M_CHI2 == 4 * pc.CHI2_SPREAD


# ---- layers 1 to 3 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["plain_64", "shift_100_2", "gross_257", "few_5"])
def test_layer1_edges(emu, name):
    print(name, "worst Jacobian difference / bound: %.3g" % pc.check_edges(emu, name))


@pytest.mark.parametrize("name", [n for n in NAMES if n != "plane_exact_50"])
def test_layer2_first_linearisation(emu, name):
    sc, res = pc.model(name)
    p3d, p2d, w, K, Tcw = sc
    sums = emu.linearise(emu.pose_of(Tcw), K, pc.Emu.edges(p3d, p2d, w), np.zeros(len(p3d), np.uint8))
    pc.check_linearisation(name, sums)


def test_layer2_with_inactive_edges(emu):
    """A later round's linearisation: the model's pose and active set, the skipped edges leaving the shape as it is."""
    name = "shift_150_5"
    sc, res = pc.model(name)
    p3d, p2d, w, K, Tcw = sc
    L = [l for l in res.lin if l["round"] == 2][0]
    assert 0 < L["active"].sum() < len(p3d)
    sums = emu.linearise(np.concatenate([L["q"], L["t"]]), K, pc.Emu.edges(p3d, p2d, w), (~L["active"]).astype(np.uint8))
    pc.check_linearisation(name, sums, L)


@pytest.mark.parametrize("name", ["plain_10", "plain_257", "shift_100_3", "gross_600", "few_1"])
def test_layer3_trial(emu, name):
    for trial in (0, 1, 2):
        print(name, trial, "dx bound %.3g, rho bound %.3g" % pc.check_trial(emu, name, trial))


def test_layer3_failed_solve_keeps_the_previous_step(emu):
    K, e, st, qt = (400, 400, 320, 240), np.array([[1, 2, 4, 423, 436, 0.5]], np.float32), np.zeros(1, np.uint8), [0, 0, 0, 1, 0, 0, 0]
    ok, dx, qo, (tmp, scale, rho) = emu.trial(pc.triu(-np.eye(6)), 0.5, np.ones(6), qt, 10.0, K, e, st, dx_prev=np.arange(6) * 1e-3)
    assert not ok and dx.tolist() == (np.arange(6) * 1e-3).tolist() and tmp == pm.DBL_MAX and rho < 0
    ok, dx, qo, (tmp, scale, rho) = emu.trial(pc.triu(np.full((6, 6), np.nan)), 0.5, np.ones(6), qt, 10.0, K, e, st)
    assert not ok and not dx.any() and qo.tolist() == qt and scale == 1e-3 and tmp == pm.DBL_MAX


def test_layer3_a_mutation_of_scale_fails(uvo):
    m = pc.Emu(uvo, "SCALE")
    with pytest.raises(AssertionError):
        pc.check_trial(m, "plain_10", 0)


# ---- layers 4 and 5 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_layers_4_and_5(runs, name):
    k = pc.check_all(name, runs[name], pc.first_sums(runs[name]) if name != "plane_exact_50" else None)
    print(name, "compared prefix", k, "of", len(pc.model(name)[1].trials), "trials; thin" if pc.thin(name) else "trials")


def test_non_finite_values_follow_the_arithmetic(runs):
    run, (sc, res) = runs["plane_exact_50"], pc.model("plane_exact_50")
    assert np.isnan(run.trace.lin["chi2"]).all() and not run.trace.trial["ok"].any() and (run.trace.trial["tmp"] == pm.DBL_MAX).all()
    assert run.outlier[0] == 0 and run.outlier.tobytes() == res.outlier.tobytes()


def test_host_build_repeats_itself(emu, runs):
    for name in ("shift_100_2", "plain_257", "plane_exact_50"):
        again = emu.optimize(pc.model(name)[0])
        assert again.Tcw.tobytes() == runs[name].Tcw.tobytes() and again.trace.trial.tobytes() == runs[name].trace.trial.tobytes()
        assert again.trace.lin.tobytes() == runs[name].trace.lin.tobytes() and again.outlier.tobytes() == runs[name].outlier.tobytes()


# ---- the stand-alone program -----------------------------------------------------------------------------------------------------------
def test_stand_alone_program_runs_the_committed_scene_list(tmp_path):
    """tests/emu/poseopt_emu.cpp with its own main (the form that is run under the sanitizers) over tests/golden/poseopt_scenes.bin:
    the file holds the scene list, and the program's counts are the model's."""
    fixture = os.path.join(pc.ROOT, "tests", "golden", "poseopt_scenes.bin")
    scenes = pm.load(fixture)
    assert [len(s[0]) for s in scenes] == [pm.SCENES[n]["n"] for n in NAMES]
    for name, got in zip(NAMES, scenes):
        want = pc.model(name)[0]
        assert all(np.array_equal(np.asarray(a, np.float32), np.asarray(b, np.float32)) for a, b in zip(got, want)), name
    r = subprocess.run([host_build.build("poseopt_emu_main"), fixture], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rows = re.findall(r"^scene (\d+) n (\d+) inliers (\d+) rounds (\d+)", r.stdout, re.M)
    assert len(rows) == len(NAMES)
    for name, (_, n, inl, rounds) in zip(NAMES, rows):
        res = pc.model(name)[1]
        assert (int(n), int(rounds)) == (len(res.outlier), res.rounds) and (pc.thin(name) or int(inl) == res.n_inliers), (name, n, inl, rounds)


# ---- the seeded mutations ---------------------------------------------------------------------------------------------------------------
def _fails(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("mutation", sorted(pc.MUTATIONS))
def test_seeded_mutations_fail_the_same_checks(uvo, mutation):
    m = pc.Emu(uvo, mutation)
    caught = []
    for name in NAMES:
        sc, res = pc.model(name)
        run = m.optimize(sc)
        if _fails(lambda: pc.check_all(name, run, pc.first_sums(run) if name != "plane_exact_50" else None)):
            caught.append(name)
    print(mutation, "caught on", len(caught), "of", len(NAMES), "scenes:", caught[:8])
    assert caught, mutation
