"""What the compiler makes of the solvePnPRansac kernels (csrc/pnp.hip), checked without a GPU through tools/kernel_resources.py.

k_pnp_hypotheses keeps the EPnP workspace (589 doubles per hypothesis) in LDS precisely so that no 12 x 12 matrix is held in registers or
indexed dynamically in private memory.  The property pinned here is that: no scratch in any of the four kernels, the workspaces in LDS
within what one workgroup may have, registers within the file.  How the lanes are laid out over the hypotheses is free to change."""
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

KERNELS = ("uvo::k_pnp_prepare", "uvo::k_pnp_hypotheses", "uvo::k_pnp_score", "uvo::k_pnp_finish")
WORKSPACE_BYTES = 589 * 8


@functools.lru_cache(maxsize=None)
def _resources():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.resources("pnp.hip", extra_flags=[])


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_scratch(kernel):
    r = _resources()[kernel]
    print(kernel, r)
    assert r["scratch"] == 0 and r.get("vgpr_spill", 0) == 0      # (scalar registers parked in vector lanes are no scratch)
    assert r["vgprs"] + r.get("agprs", 0) <= 256
    assert r["lds"] <= 64 * 1024


def test_workspaces_live_in_lds():
    r = _resources()
    assert r["uvo::k_pnp_hypotheses"]["lds"] >= WORKSPACE_BYTES and r["uvo::k_pnp_finish"]["lds"] >= WORKSPACE_BYTES
