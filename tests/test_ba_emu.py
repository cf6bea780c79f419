"""The bundle adjustment without a GPU: the host build of csrc/ba_core.hpp (tests/emu/ba_emu.cpp, the source the k_ba_* kernels run,
walking the same reduction shapes and the same launch sequence) against the numpy model written from the reference's sources
(tests/ba_model.py), layer by layer as DESIGN.md section 4 states the contract and tests/ba_checks.py derives the bounds.  Nine seeded
mutations of the host build have to fail these same checks."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import ba_checks as pc
import ba_model as bm
import host_build

NAMES = list(bm.SCENES)


@pytest.fixture(scope="module")
def emu(uvo):
    return pc.Emu(uvo)


@pytest.fixture(scope="module")
def runs(emu):
    return {name: emu.adjust(pc.model(name)[0]) for name in NAMES}


def test_new_symbols_are_declared_and_exported(uvo):
    names = ("uvo_bundle_adjuster_create", "uvo_bundle_adjuster_destroy", "uvo_bundle_adjust", "uvo_bundle_adjuster_trace")
    lib = ctypes.CDLL(uvo.LIB_PATH)
    for n in names:
        assert n in uvo.ABI_SYMBOLS and hasattr(lib, n), n
    assert ctypes.sizeof(uvo.BaProblemC) == 24 + 10 * 8 and ctypes.sizeof(uvo.BaResultC) == 6 * 8 + 24
    assert ctypes.sizeof(uvo.BaTraceLin) == 40 and ctypes.sizeof(uvo.BaTraceC) == 8 + 32 * 40 + 320 * 48
    assert uvo.BA_LIN_DTYPE.itemsize == 40 and hasattr(uvo, "BundleAdjuster")


def test_recorded_spreads_are_what_the_model_shows():
    """T and M come from the model under 4 permuted edge orders x 3 reduced solvers.  The measurement over all scenes
    (`python tests/ba_checks.py`) is NOT repeated by the suite; what is repeated is the same measurement on the scene that sets both
    maxima, so the recorded figures themselves are reproduced here: within the recorded spreads, and not below nine tenths of them."""
    est, chi, unclear = pc.measure_spread(["far_start"])
    print("estimate spread %.3e (recorded %.1e), relative chi2 spread %.3e (recorded %.1e)" % (est, pc.EST_SPREAD, chi, pc.CHI2_REL_SPREAD))
    assert 0.9 * pc.EST_SPREAD <= est <= pc.EST_SPREAD and 0.9 * pc.CHI2_REL_SPREAD <= chi <= pc.CHI2_REL_SPREAD and not unclear
    assert pc.T_EST == 4 * pc.EST_SPREAD and pc.M_REL == 4 * pc.CHI2_REL_SPREAD


def test_start_is_the_models(emu):
    """Converter::toSE3Quat of the float poses and the widened points: a full-mode call whose first trial is all that differs."""
    sc, res = pc.model("kf2_fixed1_p8")
    got = emu.one_trial(sc, res.lin[0]["est"], res.lin[0]["X"], np.zeros(len(sc["edge_kf"]), np.uint8), 1.0)
    fixed = np.flatnonzero(sc["fixed"])
    assert np.array_equal(got["est_try"][fixed], res.lin[0]["est"][fixed])


@pytest.mark.parametrize("name", NAMES)
def test_layers_1_to_3_on_the_models_estimates(emu, name):
    """Per edge, the assembled blocks, one whole trial: at the model's first and last linearisation."""
    for w1, w2, w3 in pc.check_layers(emu, name):
        print("%s: worst difference / bound: edges %.3g, assembly %.3g, trial %.3g" % (name, w1, w2, w3))
        assert w1 <= 1 and w2 <= 1 and w3 <= 1


@pytest.mark.parametrize("name", NAMES)
def test_layers_4_and_5_driver_and_answer(runs, name):
    pc.check_all(name, runs[name])


def test_failed_solve_is_a_rejected_trial_that_moves_nothing(runs):
    r = runs["zero_depth"]
    t = r.trace.trial
    assert not t["ok"][:5].any() and (t["tmp"][:5] == pc.DBL_MAX).all() and not t["accepted"][:5].any() and t["ok"][5:].all()
    assert np.isnan(r.trace.lin["chi2"][0]) and np.isfinite(r.trace.lin["chi2"][5:]).all() and r.removed1[0] == 1


def test_every_scene_has_its_syncs_counted(runs):
    for name, r in runs.items():
        rounds = 1 if pc.model(name)[0].get("mode", 0) == bm.FULL else 2
        assert r.n_syncs == r.n_trials + rounds + 1 and r.n_syncs <= 2 + 150 + 1, (name, r.n_syncs)


# what catches which mutation: ("layers", scene) = layers 1 to 3 on the model's estimates, ("call", scene) = layers 4 and 5 on a whole call
CATCH = {
    "LAMBDA_POSE_ONLY": [("layers", "kf2_fixed1_p8")],
    "DINV_PLAIN": [("layers", "realistic")],
    "FIXED_W": [("layers", "kf2_fixed1_p8")],
    "SCHUR_ADD": [("layers", "kf2_fixed1_p8")],
    "NO_WX": [("layers", "lists")],
    "REEVAL": [("layers", "far_start")],
    "RETURN": [("call", "realistic")],
    "STEP_IDLE": [("call", "lonely_keyframe")],
    "TAU_POSES": [("call", "near_point")],
}


@pytest.mark.parametrize("mutation", list(pc.MUTATIONS))
def test_each_mutation_fails_its_checks(uvo, mutation):
    m = pc.Emu(uvo, mutation)
    for kind, name in CATCH[mutation]:
        with pytest.raises(AssertionError):
            if kind == "layers":
                for w in pc.check_layers(m, name):
                    assert max(w) <= 1
            else:
                pc.check_all(name, m.adjust(pc.model(name)[0]))


def test_standalone_program_runs_the_committed_scenes():
    """tests/emu/ba_emu.cpp with its own main (the form that is run under the sanitizers) over tests/golden/ba_scenes.bin: the counts
    it prints for the committed scenes are the model's."""
    fixture = os.path.join(pc.ROOT, "tests", "golden", "ba_scenes.bin")
    out = subprocess.run([host_build.build("ba_emu_main"), fixture], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-2000:] + out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("scene ")]
    assert len(lines) == len(NAMES)
    for line, name in zip(lines, NAMES):
        res = pc.model(name)[1]
        want = "removed %d %d iterations %d %d trials %d" % (res.n_removed1, res.n_removed2, res.iterations[0], res.iterations[1], len(res.trials))
        assert line.endswith(want), (name, line, want)
