"""What the compiler makes of the k_navba_* kernels (csrc/navba.hip), checked without a GPU through tools/kernel_resources.py: every
phase stays in registers -- no scratch, no spills, at most 256 registers a lane -- and within the static LDS limit.  The edge phase
carries Rcb, Pbc and a key frame's Rcb Rwb^T per edge on top of what k_ba_edge_lin holds; the inertial phases give an edge a lane and
write its 9 x 30 Jacobian straight to global memory so that no lane indexes a local array."""
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

KERNELS = ["uvo::k_navba_" + n for n in ("init", "begin", "edge_lin", "inert_lin", "point_sum", "kf_sum", "lin_ctl", "dinv", "schur", "inert_add", "solve",
                                         "step", "edge_err", "inert_err", "trial_ctl", "check", "finish")]


@functools.lru_cache(maxsize=None)
def _resources():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.resources("navba.hip", extra_flags=[])


def test_every_phase_is_a_kernel():
    assert sorted(k for k in _resources() if "k_navba_" in k) == sorted(KERNELS)


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_scratch_no_spills(kernel):
    r = _resources()[kernel]
    print(kernel, r)
    assert r["scratch"] == 0 and r.get("vgpr_spill", 0) == 0
    assert r["vgprs"] + r.get("agprs", 0) <= 256
    assert r["lds"] <= 64 * 1024


def test_the_solve_keeps_its_two_vectors_in_lds():
    assert _resources()["uvo::k_navba_solve"]["lds"] >= 2 * 15 * 24 * 8
