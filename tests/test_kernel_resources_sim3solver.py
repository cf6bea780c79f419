"""What the compiler makes of the Sim3Solver kernels (csrc/sim3solver.hip), checked without a GPU through tools/kernel_resources.py: the
4 x 4 Jacobi of computeT indexes its matrices by a run-time pivot, so they live in LDS per lane and no kernel may use scratch."""
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

KERNELS = ("uvo::k_sim3_hypotheses", "uvo::k_sim3_score", "uvo::k_sim3_finish")
LANE_BYTES = (36 + 8) * 4      # A[16], V[16], W[4] as floats, indR[4], indC[4] as ints


@functools.lru_cache(maxsize=None)
def _resources():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.resources("sim3solver.hip", extra_flags=[])


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_scratch(kernel):
    r = _resources()[kernel]
    print(kernel, r)
    assert r["scratch"] == 0 and r.get("vgpr_spill", 0) == 0
    assert r["vgprs"] + r.get("agprs", 0) <= 256
    assert r["lds"] <= 64 * 1024


def test_jacobi_matrices_live_in_lds():
    assert _resources()["uvo::k_sim3_hypotheses"]["lds"] >= 64 * LANE_BYTES
