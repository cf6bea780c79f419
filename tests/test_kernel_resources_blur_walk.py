"""What the compiler makes of the blur's row loops (csrc/gauss_body.hpp: one loop per walk, unrolled by 7 rows), read through
tools/loop_mix.py without a GPU.  The step is bound by vector-instruction issue, and the walk's bookkeeping -- row
counter, loop exit, row addresses, the flush's row tests -- is wave-uniform: it belongs in scalar registers.  These tests hold
  * the loop control of every walk: scalar compares and branches (a value loaded through scratch, or derived from one, is a vector value, and
    the row loop becomes a divergent loop with an EXEC region around every unrolled row -- k_gauss7 up to this test's commit),
  * the vector instructions of a loop body (7 rows; both sides of a scalar branch count, so the edge block's row arithmetic is in it), with
    2 % of slack for the compiler's scheduling: full strips 385, narrow strips 420 (padded plane) and 454 (level 0 in place), the scalar-tail
    walk 506; before: 480 - 530 (padded), 432 - 489 (in place), 516 - 573 (tail) -- profiles/LOG.md has the whole table,
  * the EXEC regions of a body: the direct store of a row (7) and the flush's two tasks per unrolled row (14), nothing else,
  * k_gauss7: no scratch (the by-value plans were copied there), and the register budget of five wavefronts per SIMD on both kernels."""
import importlib.util
import os
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _have_hipcc():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    return os.path.exists(hipcc) or shutil.which(hipcc) is not None


pytestmark = pytest.mark.skipif(not _have_hipcc(), reason="no hipcc: the kernels cannot be compiled here")

# vector instructions of the walks' loop bodies, largest first: (scalar tail,) narrow in place, narrow padded, full in place, full padded
WALKS = {True: [506, 454, 420, 385, 385], False: [454, 420, 385, 385]}
SLACK = 0.02
EXEC_REGIONS = 21


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def mixes():
    lm = _tool("loop_mix")    # the committed defaults, whatever UVO_EXTRA_FLAGS says; the walks are the loops that hold the row pass's dot products
    return {src: lm.loop_mix(src, top=8, extra_flags=[], having="v_dot4") for src in ("gauss.hip", "octree.hip")}


@pytest.mark.parametrize("src,kernel,sse2", [("gauss.hip", "uvo::k_gauss7<true>", True), ("gauss.hip", "uvo::k_gauss7<false>", False),
                                             ("octree.hip", "uvo::k_octree_gauss<true>", True), ("octree.hip", "uvo::k_octree_gauss<false>", False)])
def test_walk_loops(mixes, src, kernel, sse2):
    loops = sorted(mixes[src][kernel], key=lambda r: -r["vector"])
    print(kernel, loops)
    assert len(loops) == len(WALKS[sse2]), "one loop per walk"
    for loop, vector in zip(loops, WALKS[sse2]):
        assert loop["control"] == "scalar", loop
        assert loop["vector"] <= vector * (1 + SLACK), loop
        assert loop["vector"] >= vector * (1 - SLACK), "fewer vector instructions than pinned: lower the pin (%s)" % loop
        assert loop["saveexec"] <= EXEC_REGIONS, loop


def test_registers_and_scratch():
    kr = _tool("kernel_resources")
    for src, kernels in (("gauss.hip", ("uvo::k_gauss7<true>", "uvo::k_gauss7<false>")), ("octree.hip", ("uvo::k_octree_gauss<true>", "uvo::k_octree_gauss<false>"))):
        res = kr.resources(src, extra_flags=[])
        for k in kernels:
            r = res[k]
            print(k, r)
            assert r["scratch"] == 0 and r.get("vgpr_spill", 0) == 0
            assert r["vgprs"] + r.get("agprs", 0) <= 96 and r["occupancy"] == 5
