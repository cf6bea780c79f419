"""What the compiler makes of k_sim3_optimize (csrc/sim3opt.hip), checked without a GPU through tools/kernel_resources.py: the lane
sums of a pass, one edge's 2 x 7 numeric Jacobian and the unrolled 7 x 7 LDL^T must all stay in registers -- no scratch, no spills --
and the per-pair state of up to 1024 pairs, the reduction words and the 15 perturbed similarities must fit the static LDS limit."""
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

KERNEL = "uvo::k_sim3_optimize"
LDS_PAIRS = 1024               # kSim3OptLdsPairs: two doubles and a state byte each
RED_BYTES = 2 * 4 * 36 * 8 + 2 * 4 * 4 + 36 * 8   # two buffers of four wavefront words for 36 sums and for the counts, the shared sums
SIM_BYTES = 15 * 24 * 8        # 14 perturbed similarities and the estimate: s R | t forward and inverse


@functools.lru_cache(maxsize=None)
def _resources():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.resources("sim3opt.hip", extra_flags=[])


def test_no_scratch_no_spills():
    r = _resources()[KERNEL]
    print(KERNEL, r)
    # scalar registers that do not fit go to lanes of a vector register, never to memory: scratch == 0 covers them too
    assert r["scratch"] == 0 and r.get("vgpr_spill", 0) == 0
    assert r["vgprs"] + r.get("agprs", 0) <= 256
    assert r["lds"] <= 64 * 1024


def test_pair_state_reduction_words_and_similarities_live_in_lds():
    assert _resources()[KERNEL]["lds"] >= LDS_PAIRS * 17 + RED_BYTES + SIM_BYTES
