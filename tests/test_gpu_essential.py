"""The essential-graph optimisation on the device (csrc/essential.hip) against the host build of the same source
(tests/emu/essential_emu.cpp), bit for bit -- the similarities, the float poses and points, the counts and every record of the trace
tap -- and against the numpy model through the same checks as the host build (tests/essential_checks.py: the exact replay of the
driver's rules, the trajectory over the clear prefix, the answer within T)."""
import numpy as np
import pytest

import essential_checks as pc
import essential_model as em

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def emu(uvo):
    return pc.Emu(uvo)


@pytest.fixture(scope="module")
def matcher(uvo):
    return uvo.ORBmatcher(0.8)


@pytest.fixture(scope="module")
def graph(uvo, matcher):
    g = uvo.EssentialGraph(matcher, 160, 700, 1200, 320)
    yield g
    g.close()


def device_run(graph, sc):
    res = graph.optimize(sc)
    return pc.of_result(res, graph.trace())


def assert_equal_runs(dev, host, what):
    bad = pc.same_run(dev, host)
    assert not bad, (what, bad)


@pytest.mark.parametrize("name", list(em.SCENES))
def test_scenes_bit_for_bit_and_against_the_model(graph, emu, name):
    """One handle through scenes of changing size: 2 key frames with one free, a chain of 3, a ring of 12 with fill, 40 key frames with two
    loops, duplicates and an isolated key frame, 150 key frames / 607 edges / 300 points (edges, rows and points cross the 256-lane
    chunk), rejected trials, no point, the acos branch, every edge at zero error."""
    sc, _ = pc.model(name)
    dev = device_run(graph, sc)
    assert_equal_runs(dev, emu.optimize(sc), name)
    n, total = pc.check_call(name, dev)
    print("%s: trajectory compared over %d of the model's %d trials" % (name, n, total))


def test_small_call_after_a_large_one_and_the_same_call_twice(graph, emu):
    big, small = pc.model("kf150")[0], pc.model("kf2")[0]
    a = device_run(graph, big)
    b = device_run(graph, big)
    assert_equal_runs(a, b, "the same call twice")
    assert_equal_runs(device_run(graph, small), emu.optimize(small), "a small call after a large one")


def test_graphs_without_work_answer_with_the_inputs(graph, emu):
    sc = dict(pc.model("ring12")[0])
    none = dict(sc, edge_i=sc["edge_i"][:0], edge_j=sc["edge_j"][:0], conn=sc["conn"][:0])
    one = dict(none, Scw=sc["Scw"][:1], Scwn=sc["Scwn"][:1], ref=sc["ref"] * 0, fixed=0)
    for s in (none, one):
        dev = device_run(graph, s)
        assert_equal_runs(dev, emu.optimize(s), "no work")
        assert dev.iterations == 0 and dev.n_trials == 0 and len(dev.trace.lin) == 0 and pc.same_bits(dev.S, s["Scw"])


def test_capacity_and_bad_arguments(uvo, matcher, graph):
    sc = dict(pc.model("ring12")[0])
    blocks = device_run(graph, sc).envelope_blocks
    E = len(sc["edge_i"])
    small = uvo.EssentialGraph(matcher, 12, E, blocks - 1, 20)
    with pytest.raises(uvo.UvoError) as err:
        small.optimize(sc)
    assert err.value.code == -4 and "envelope needs %d blocks" % blocks in uvo.last_error()
    small.close()
    exact = uvo.EssentialGraph(matcher, 12, E, blocks, 20)
    assert_equal_runs(pc.of_result(exact.optimize(sc), exact.trace()), device_run(graph, sc), "a handle of exactly the scene's size")
    for bad in (pc.model("kf40")[0], dict(sc, points=np.zeros((21, 3), np.float32), ref=np.zeros(21, np.int32))):
        with pytest.raises(uvo.UvoError) as err:
            exact.optimize(bad)
        assert err.value.code == -4
    exact.close()
    k = np.arange(E) == 3
    for bad, word in ((dict(sc, edge_i=np.where(k, 12, sc["edge_i"])), "out of range"), (dict(sc, edge_j=np.where(k, -1, sc["edge_j"])), "out of range"),
                      (dict(sc, fixed=-1), "out of range"), (dict(sc, edge_j=np.where(k, sc["edge_i"], sc["edge_j"])), "itself"),
                      (dict(sc, ref=np.where(np.arange(len(sc["ref"])) == 0, 12, sc["ref"])), "reference"), (dict(sc, n_iterations=0), "iterations"),
                      (dict(sc, n_iterations=33), "iterations")):
        with pytest.raises(uvo.UvoError) as err:
            graph.optimize(bad)
        assert err.value.code == -1 and word in uvo.last_error(), (word, uvo.last_error())
    with pytest.raises(uvo.UvoError):
        uvo.EssentialGraph(matcher, 0, 1, 1, 0)
