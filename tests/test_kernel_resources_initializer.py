"""What the compiler makes of the two-view initialisation kernels (csrc/initializer.hip), checked without a GPU through
tools/kernel_resources.py: the one-sided Jacobi picks its rows by pair and by sort position, so they live in LDS per lane and no
kernel may use scratch."""
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

KERNELS = ("uvo::k_init_hypotheses", "uvo::k_init_score", "uvo::k_init_select", "uvo::k_init_check_rt", "uvo::k_init_finish")
LANE_BYTES = 81 * 4 + 8 * 8      # nine rows of nine floats, W[8] as doubles


@functools.lru_cache(maxsize=None)
def _resources():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.resources("initializer.hip", extra_flags=[])


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_scratch(kernel):
    r = _resources()[kernel]
    print(kernel, r)
    assert r["scratch"] == 0 and r.get("vgpr_spill", 0) == 0
    assert r["vgprs"] + r.get("agprs", 0) <= 256
    assert r["lds"] <= 64 * 1024


def test_jacobi_rows_live_in_lds():
    for k in ("uvo::k_init_hypotheses", "uvo::k_init_check_rt"):
        assert _resources()[k]["lds"] >= 64 * LANE_BYTES
