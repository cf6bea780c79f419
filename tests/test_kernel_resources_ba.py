"""What the compiler makes of the bundle adjustment's kernels (csrc/ba.hip), checked without a GPU through tools/kernel_resources.py:
the edge kernels (error, Huber weights, both Jacobians) and the reductions with their 27 and 42 lane sums must stay in registers -- no
scratch, no spills, at most 256 VGPRs + AGPRs -- and the reduction words and the solve's two vectors must fit the static LDS limit."""
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

KERNELS = ["uvo::k_ba_" + k for k in ("init", "begin", "edge_lin", "point_sum", "kf_sum", "lin_ctl", "dinv", "schur", "solve", "step", "edge_err", "trial_ctl",
                                       "check", "finish")]


@functools.lru_cache(maxsize=None)
def _resources():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.resources("ba.hip", extra_flags=[])


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_scratch_no_spills(kernel):
    r = _resources()[kernel]
    print(kernel, r)
    assert r["scratch"] == 0 and r.get("vgpr_spill", 0) == 0
    assert r["vgprs"] + r.get("agprs", 0) <= 256
    assert r["lds"] <= 64 * 1024


def test_solve_keeps_its_two_vectors_in_lds():
    assert _resources()["uvo::k_ba_solve"]["lds"] >= 2 * 6 * 64 * 8
