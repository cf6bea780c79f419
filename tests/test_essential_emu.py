"""The essential-graph optimisation without a GPU: the host build of csrc/essential_core.hpp (tests/emu/essential_emu.cpp, the source the
k_essential_* kernels run, walking the same sums, the same envelope solve and the same launch sequence) against the numpy model written
from the reference's sources (tests/essential_model.py), layer by layer as tests/essential_checks.py derives the bounds.  Eight seeded
mutations of the host build have to fail these same checks, each in a named layer."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import essential_checks as pc
import essential_model as em
import host_build

NAMES = list(em.SCENES)


@pytest.fixture(scope="module")
def emu(uvo):
    return pc.Emu(uvo)


@pytest.fixture(scope="module")
def runs(emu):
    return {name: emu.optimize(pc.model(name)[0]) for name in NAMES}


def test_new_symbols_are_declared_and_exported(uvo):
    names = ("uvo_essential_graph_create", "uvo_essential_graph_destroy", "uvo_essential_graph_optimize", "uvo_essential_graph_trace")
    lib = ctypes.CDLL(uvo.LIB_PATH)
    header = open(os.path.join(pc.ROOT, "include", "uvo", "uvo.h")).read()
    for n in names:
        assert n in uvo.ABI_SYMBOLS and hasattr(lib, n) and n + "(" in header, n
    assert ctypes.sizeof(uvo.EssentialProblemC) == 16 + 7 * 8 + 8 and ctypes.sizeof(uvo.EssentialResultC) == 3 * 8 + 16
    assert hasattr(uvo, "EssentialGraph")


def test_layer_0_log_and_acos(emu):
    print("log_: worst error / bound %.3g" % pc.check_log(emu.log))
    pc.check_acos(emu.acos)


def test_layer_1_sim3(emu):
    w = pc.check_sim_ops(emu)
    print("product, inverse, log, update: worst difference / bound %.3g" % w)
    assert w <= 1


@pytest.mark.parametrize("name", NAMES)
def test_layers_2_and_3_on_the_models_estimates(emu, name):
    """One linearisation and one trial at the model's first and last linearisation, and at its first rejected trial's lambda."""
    for w in pc.check_layers(emu, name):
        print("%s: worst difference / bound: against the model %.3g, assembly %.3g, trial %.3g" % ((name,) + w))
        assert max(w) <= 1


@pytest.mark.parametrize("name", NAMES)
def test_layers_3_and_4_driver_trajectory_and_answer(runs, name):
    n, total = pc.check_call(name, runs[name])
    print("%s: trajectory compared over %d of the model's %d trials" % (name, n, total))


def test_the_scene_set_meets_its_conditions():
    """In at most a quarter of the scenes may the trajectory comparison stop before the model's last trial; the model's own solves
    succeed wherever it accepts a step; the paths the scenes were chosen for are taken."""
    early = [n for n in NAMES if pc.clear_prefix(pc.model(n)[1]) < len(pc.model(n)[1].trials)]
    assert 4 * len(early) <= len(NAMES), early
    assert all(t["ok"] for n in NAMES for t in pc.model(n)[1].trials if t["accepted"])
    acc = [t["accepted"] for t in pc.model("rejected")[1].trials]
    assert any(not a and any(acc[k + 1:]) for k, a in enumerate(acc)), "no rejected trial is followed by an accepted one"
    sc = em.make("kf150")
    assert len(sc["edge_i"]) > 512 and len(sc["points"]) > 256 and 7 * (len(sc["Scw"]) - 1) > 1024
    sc = em.make("kf40")
    pairs = list(zip(sc["edge_i"], sc["edge_j"]))
    assert len(set(pairs)) < len(pairs) and np.diff(sc["mnid"]).max() > 1 and 17 not in set(sc["edge_i"]) | set(sc["edge_j"])
    assert sc["Scw"][:, 7].min() < 0.9 or sc["Scw"][:, 7].max() > 1.1
    z = pc.model("zero_error")[1].lin[0]
    assert np.abs(z.e).max() < 1e-5
    big = pc.model("large_rotation")[1].lin[0]
    assert np.abs(big.e[:, :3]).max() > 0.1


def test_envelope_solver_equals_the_dense_one(emu):
    """Random SPD matrices with random envelopes, fill included; one with a negative pivot, where both fail alike."""
    g = np.random.default_rng(3)
    for case in range(24):
        F = int(g.integers(1, 14))
        first = np.array([int(g.integers(0, f + 1)) if g.random() < 0.7 else max(f - 1, 0) for f in range(F)])
        N = 7 * F
        inside = np.zeros((N, N), bool)
        for f in range(F):
            inside[7 * f:7 * f + 7, 7 * first[f]:7 * f + 7] = True
        M = np.where(inside, g.normal(size=(N, N)), 0.0)
        M = np.tril(M) + np.tril(M, -1).T
        A = M + (np.abs(M).sum(1).max() + 1) * np.eye(N)      # diagonally dominant: positive definite
        if case % 6 == 5:
            k = int(g.integers(N))
            A[k, k] = -A[k, k]                                   # an indefinite matrix: a negative pivot, ok is false in both
        ok = pc.check_solver(emu, first, A, g.normal(size=N))
        assert ok == (case % 6 != 5), case


def test_refused_graphs_and_graphs_without_work(emu):
    sc = dict(em.make("ring12"))
    assert emu.optimize(dict(sc, edge_i=np.where(np.arange(len(sc["edge_i"])) == 3, 12, sc["edge_i"]))) == 1
    assert emu.optimize(dict(sc, edge_j=np.where(np.arange(len(sc["edge_i"])) == 3, -1, sc["edge_j"]))) == 1
    assert emu.optimize(dict(sc, fixed=12)) == 1
    assert emu.optimize(dict(sc, edge_j=np.where(np.arange(len(sc["edge_i"])) == 3, sc["edge_i"], sc["edge_j"]))) == 2
    full = emu.optimize(sc)
    assert emu.optimize(sc, max_blocks=full.envelope_blocks - 1) == 3 and not isinstance(emu.optimize(sc, max_blocks=full.envelope_blocks), int)
    # no edge, or a single key frame: the answer is the input's
    for s in (dict(sc, edge_i=sc["edge_i"][:0], edge_j=sc["edge_j"][:0], conn=sc["conn"][:0]),
              dict(sc, Scw=sc["Scw"][:1], Scwn=sc["Scwn"][:1], edge_i=sc["edge_i"][:0], edge_j=sc["edge_j"][:0], conn=sc["conn"][:0], ref=sc["ref"] * 0, fixed=0)):
        r = emu.optimize(s)
        T, pts = em.recover(s, s["Scw"])
        assert r.iterations == 0 and r.n_trials == 0 and r.n_syncs == 1 and pc.same_bits(r.S, s["Scw"])
        assert np.abs(r.Tcw - T).max() <= 2.0 ** -22 * np.abs(T).max() and np.abs(r.points - pts).max() <= 2.0 ** -22 * np.abs(pts).max()


# what catches which mutation: ("layers", scene) = layers 2 and 3 on the model's estimates, ("call", scene) = the driver's rules and the
# answer of a whole call, ("solver", None) = the envelope solve against the dense one
CATCH = {
    "MEASURE_SCW": ("layers", "ring12"),
    "ONESIDED": ("layers", "chain3"),
    "SWAPPED": ("layers", "kf2"),
    "LAMBDA_TAU": ("call", "ring12"),
    "FIXED_KEPT": ("layers", "ring12"),
    "ENVELOPE_SHORT": ("layers", "ring12"),
    "ORDER_REVERSED": ("solver", None),
    "POINTS_UNCORRECTED": ("call", "kf40"),
}


@pytest.mark.parametrize("mutation", list(pc.MUTATIONS))
def test_each_mutation_fails_its_checks(uvo, mutation):
    m = pc.Emu(uvo, mutation)
    kind, name = CATCH[mutation]
    with pytest.raises(AssertionError):
        if kind == "layers":
            for w in pc.check_layers(m, name):
                assert max(w) <= 1
        elif kind == "call":
            pc.check_call(name, m.optimize(pc.model(name)[0]))
        else:
            test_envelope_solver_equals_the_dense_one(m)


def test_standalone_program_runs_the_committed_scenes():
    """tests/emu/essential_emu.cpp with its own main (the form that is run under the sanitizers) over tests/golden/essential_scenes.bin: the
    counts it prints for the committed scenes are the model's where the model's decisions are clear to the end."""
    out = subprocess.run([host_build.compile_artefact(pc.EMU_MAIN), em.FIXTURE], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-2000:] + out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("scene ")]
    assert len(lines) == len(NAMES)
    for line, name in zip(lines, NAMES):
        res = pc.model(name)[1]
        if pc.clear_prefix(res) == len(res.trials):
            want = "iterations %d trials %d" % (res.iterations, len(res.trials))
            assert line.endswith(want), (name, line, want)
