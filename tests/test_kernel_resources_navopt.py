"""What the compiler makes of k_nav_optimize (csrc/navopt.hip), checked without a GPU through tools/kernel_resources.py: the 28 lane
sums and the edge evaluations must stay in registers -- no scratch, no spills, at most 256 registers a lane -- and navopt::Work (H, the
factor, the stacked Jacobian, the right-hand sides, the states), the per-edge state of up to 2048 edges and the reduction words must
fit the static LDS limit."""
import functools
import importlib.util
import os
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _have_hipcc():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    return os.path.exists(hipcc) or shutil.which(hipcc) is not None


pytestmark = pytest.mark.skipif(not _have_hipcc(), reason="no hipcc: the kernels cannot be compiled here")

KERNEL = "uvo::k_nav_optimize"
LDS_EDGES = 2048               # kNavLdsEdges: a double and a state byte each
RED_BYTES = 2 * 4 * 28 * 8 + 2 * 4 * 4 + 28 * 8   # two buffers of four wavefront words for 28 sums and for the counts, the shared sums
# navopt::Work in doubles: H, A (30 x 30 each), J, WJ (31 x 30 each), X (30 x 15), e, We, b, dx, y, oimu, M15, sing, est and backup, cam, camc
WORK_BYTES = 8 * (2 * 900 + 2 * 930 + 450 + 2 * 31 + 3 * 30 + 81 + 225 + 12 + 4 * 22 + 24 + 3)


@functools.lru_cache(maxsize=None)
def _resources():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.resources("navopt.hip", extra_flags=[])


def test_no_scratch_no_spills():
    r = _resources()[KERNEL]
    print(KERNEL, r)
    # scalar registers that do not fit go to lanes of a vector register, never to memory: scratch == 0 covers them too
    assert r["scratch"] == 0 and r.get("vgpr_spill", 0) == 0
    assert r["vgprs"] + r.get("agprs", 0) <= 256
    assert r["lds"] <= 64 * 1024


def test_work_edge_state_and_reduction_words_live_in_lds():
    assert _resources()[KERNEL]["lds"] >= WORK_BYTES + LDS_EDGES * 9 + RED_BYTES
