"""What the compiler makes of k_pose_optimize (csrc/poseopt.hip), checked without a GPU through tools/kernel_resources.py: the 28 lane
sums, the 2 x 6 Jacobian and the unrolled 6 x 6 LDL^T must all stay in registers -- no scratch, no spills -- and the per-edge state of
up to 2048 edges plus the reduction words must fit the static LDS limit."""
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

KERNEL = "uvo::k_pose_optimize"
LDS_EDGES = 2048               # kPoseLdsEdges: a double and a state byte each
RED_BYTES = 2 * 4 * 28 * 8 + 2 * 4 * 4 + 28 * 8   # two buffers of four wavefront words for 28 sums and for the counts, the shared sums


@functools.lru_cache(maxsize=None)
def _resources():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.resources("poseopt.hip", extra_flags=[])


def test_no_scratch_no_spills():
    r = _resources()[KERNEL]
    print(KERNEL, r)
    # scalar registers that do not fit go to lanes of a vector register, never to memory: scratch == 0 covers them too
    assert r["scratch"] == 0 and r.get("vgpr_spill", 0) == 0
    assert r["vgprs"] + r.get("agprs", 0) <= 256
    assert r["lds"] <= 64 * 1024


def test_edge_state_and_reduction_words_live_in_lds():
    assert _resources()[KERNEL]["lds"] >= LDS_EDGES * 9 + RED_BYTES
