"""What the compiler makes of k_resize_level_rows (csrc/pyramid.hip), read through tools/kernel_resources.py without a GPU: the walk keeps two
filtered source rows, the column weights and the raw dwords of four output rows' source rows in registers -- no scratch, no spills, no LDS,
and few enough registers for eight wavefronts per SIMD, the occupancy it was measured at (profiles/r13_resize_rows_ab.txt: with one
row in flight instead of three the kernel is 4 % slower, so what hides the loads is wavefronts times rows in flight)."""
import importlib.util
import os
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _have_hipcc():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    return os.path.exists(hipcc) or shutil.which(hipcc) is not None


pytestmark = pytest.mark.skipif(not _have_hipcc(), reason="no hipcc: the kernels cannot be compiled here")

ROWS_OCCUPANCY = 8


@pytest.fixture(scope="module")
def pyramid_resources():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.resources("pyramid.hip", extra_flags=[])     # the committed defaults, whatever UVO_EXTRA_FLAGS says


def test_rows_kernel_resources(pyramid_resources):
    r = pyramid_resources["uvo::k_resize_level_rows"]
    print(r)
    assert r["scratch"] == 0 and r.get("vgpr_spill", 0) == 0 and r.get("sgpr_spill", 0) == 0
    assert r["lds"] == 0                                     # (an array indexed by a run-time value would be moved to LDS)
    assert r["vgprs"] + r.get("agprs", 0) <= 64
    assert r["occupancy"] == ROWS_OCCUPANCY


def test_the_old_kernel_is_still_there(pyramid_resources):
    """k_resize_level stays as it was: the byte-gather levels, small batches and read_plane's second implementation use it"""
    assert pyramid_resources["uvo::k_resize_level"]["occupancy"] == 6
