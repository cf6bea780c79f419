"""What the compiler makes of the keyframe database's kernels (csrc/kfdb.hip), checked without a GPU through tools/kernel_resources.py:
no scratch, no spills, and the LDS each one can ask for -- its static part plus the largest dynamic request its launcher makes --
within 64 KiB."""
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

# kernel -> the largest dynamic LDS its launcher requests (kfdb.hpp: kKfdbMaxWords = 4096 words of 12 bytes + 16; the epilogue's header,
# its 1024-entry reduction array and kKfdbLdsSort = 4096 eight-byte keys)
KERNELS = {"uvo::k_kfdb_words": 4096 * 12 + 16, "uvo::k_kfdb_bow_epilogue": 64 + 1024 * 4 + 4096 * 8, "uvo::k_kfdb_haloc_dist": 0, "uvo::k_kfdb_haloc_top3": 0}


@functools.lru_cache(maxsize=None)
def _resources():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.resources("kfdb.hip", extra_flags=[])


def test_launcher_constants_are_the_ones_assumed_here():
    txt = open(os.path.join(ROOT, "u-vip-slam_amd", "csrc", "kfdb.hpp")).read()
    assert "kKfdbMaxWords = 4096" in txt and "kKfdbLdsSort = 4096" in txt
    hip = open(os.path.join(ROOT, "u-vip-slam_amd", "csrc", "kfdb.hip")).read()
    assert "kEpiThreads = 1024" in hip and "kEpiHdr = 64" in hip and "(size_t)nq * 12 + 16" in hip


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_no_scratch_no_spills_lds_within_64k(kernel):
    r = _resources()[kernel]
    print(kernel, r)
    assert r["scratch"] == 0 and r.get("vgpr_spill", 0) == 0 and r.get("sgpr_spill", 0) == 0
    assert r["vgprs"] + r.get("agprs", 0) <= 128          # the epilogues run 1024 threads: 4 wavefronts per SIMD
    assert r["lds"] + KERNELS[kernel] <= 64 * 1024
