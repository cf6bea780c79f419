"""What the compiler makes of the essential-graph kernels (csrc/essential.hip), checked without a GPU through tools/kernel_resources.py:
every phase is a kernel of its own; the edge kernels (29 evaluations of log(C S_i S_j^-1) an edge) and the envelope solve's diagonal block
must stay in registers -- no scratch, no spills, at most 256 VGPRs + AGPRs -- and the static LDS must fit its limit."""
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

KERNELS = ["uvo::k_essential_" + k for k in ("init", "measure", "edge_lin", "kf_sum", "pair_sum", "lin_ctl", "copy", "solve", "step", "edge_err", "trial_ctl",
                                              "finish_kf", "finish_pts")]


@functools.lru_cache(maxsize=None)
def _resources():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.resources("essential.hip", extra_flags=[])


def test_every_phase_is_a_kernel():
    assert sorted(k for k in _resources() if "k_essential_" in k) == sorted(KERNELS)


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_scratch_no_spills(kernel):
    r = _resources()[kernel]
    print(kernel, r)
    assert r["scratch"] == 0 and r.get("vgpr_spill", 0) == 0
    assert r["vgprs"] + r.get("agprs", 0) <= 256
    assert r["lds"] <= 64 * 1024


def test_solve_keeps_the_columns_pivots_and_diagonal_block_in_lds():
    assert _resources()["uvo::k_essential_solve"]["lds"] >= 64 * 8
