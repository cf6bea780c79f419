"""What the compiler makes of the PnPsolver kernels (csrc/pnpsolver.hip), checked without a GPU through tools/kernel_resources.py: as for
csrc/pnp.hip, the EPnP workspaces live in LDS, so no kernel may use scratch, and the finishing kernel -- pnps::replay with a cooperative
refit inlined into its loop -- has to stay inside the register file."""
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

KERNELS = ("uvo::k_pnps_hypotheses", "uvo::k_pnps_score", "uvo::k_pnps_finish")
WORKSPACE_BYTES = 589 * 8


@functools.lru_cache(maxsize=None)
def _resources():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.resources("pnpsolver.hip", extra_flags=[])


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_scratch(kernel):
    r = _resources()[kernel]
    print(kernel, r)
    assert r["scratch"] == 0 and r.get("vgpr_spill", 0) == 0
    assert r["vgprs"] + r.get("agprs", 0) <= 256
    assert r["lds"] <= 64 * 1024


def test_workspaces_live_in_lds():
    r = _resources()
    assert r["uvo::k_pnps_hypotheses"]["lds"] >= 8 * WORKSPACE_BYTES and r["uvo::k_pnps_finish"]["lds"] >= WORKSPACE_BYTES
