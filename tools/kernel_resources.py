#!/usr/bin/env python3
"""What the compiler made of the step's kernels: VGPRs / scratch / LDS / wavefronts per SIMD, without a GPU.

  python tools/kernel_resources.py                      # the step's kernels, one table
  python tools/kernel_resources.py describe.hip         # every kernel of the given csrc files
  python tools/kernel_resources.py --json [files]       # the same as one JSON object

Each file is compiled for the device alone with the flags of u-vip-slam_amd/build.py (+ UVO_EXTRA_FLAGS, as build.py does) and
-Rpass-analysis=kernel-resource-usage; the workgroup size (for LDS per wavefront) is read from the code object's metadata in the
same compile.  The occupancy printed is the compiler's own figure: the smaller of what the registers and what the LDS of a
workgroup admit.  An occupancy experiment that only changes __launch_bounds__ shows up here as "nothing changed" when LDS binds.
"""
import importlib.util
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_PER_CU = 160 * 1024
SIMDS_PER_CU = 4
MAX_WAVES_PER_SIMD = 8

# the kernels of a configs[2] step: (file, demangled name; without template arguments = every instance)
STEP_KERNELS = [("pyramid.hip", "uvo::k_resize_level"), ("fast.hip", "uvo::k_fast_score"), ("fast.hip", "uvo::k_fast_cells"),
                ("octree.hip", "uvo::k_octree_gauss<true>"), ("describe.hip", "uvo::k_assemble<false>"), ("describe.hip", "uvo::k_describe<false>"),
                ("describe.hip", "uvo::k_describe<true>"), ("hamming.hip", "uvo::k_knn2_mfma")]


def _build_module():
    spec = importlib.util.spec_from_file_location("uvo_build", os.path.join(ROOT, "u-vip-slam_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _demangle(names, hipcc):
    filt = os.path.join(os.path.dirname(os.path.realpath(hipcc)), "..", "llvm", "bin", "llvm-cxxfilt")
    for tool in (filt, "llvm-cxxfilt", "c++filt"):
        try:
            out = subprocess.run([tool], input="\n".join(names) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
            return dict(zip(names, out))
        except (OSError, subprocess.CalledProcessError):
            continue
    return {n: n for n in names}


def short_name(demangled):
    """uvo::k_describe<false>(uvo::LevelGeom const*, ...) -> uvo::k_describe<false>; the return type of a template instance goes too"""
    head = demangled.split("(")[0].strip()
    return head[5:] if head.startswith("void ") else head


def resources(src, extra_flags=None):
    """-> {short kernel name: {vgprs, agprs, sgprs, scratch, lds, occupancy, workgroup, waves_per_workgroup, lds_per_wave, lds_waves_per_simd}}"""
    b = _build_module()
    extra = os.environ.get("UVO_EXTRA_FLAGS", "").split() if extra_flags is None else list(extra_flags)
    cmd = [b.HIPCC] + b.FLAGS + extra + ["--cuda-device-only", "-S", "-o", "-", "-Rpass-analysis=kernel-resource-usage", os.path.join(b.CSRC, src)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("hipcc failed for %s:\n%s\n%s" % (src, " ".join(cmd), r.stderr[-4000:]))
    fields = {"VGPRs": "vgprs", "AGPRs": "agprs", "TotalSGPRs": "sgprs", "ScratchSize [bytes/lane]": "scratch", "Occupancy [waves/SIMD]": "occupancy",
              "LDS Size [bytes/block]": "lds", "VGPRs Spill": "vgpr_spill", "SGPRs Spill": "sgpr_spill"}
    per, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+(.*?): (\S+) \[-Rpass-analysis=kernel-resource-usage\]", line)
        if not m:
            continue
        key, val = m.group(1).strip(), m.group(2)
        if key == "Function Name":
            cur = per.setdefault(val, {})
        elif cur is not None and key in fields:
            cur[fields[key]] = int(val)
    wg = {}
    for m in re.finditer(r"\.max_flat_workgroup_size:\s*(\d+)\s*\n\s*\.name:\s*(\S+)", r.stdout):
        wg[m.group(2)] = int(m.group(1))
    names = _demangle(list(per), b.HIPCC)
    out = {}
    for mangled, rec in per.items():
        if mangled not in wg:   # a device function, not a kernel
            continue
        rec["workgroup"] = wg[mangled]
        rec["waves_per_workgroup"] = (wg[mangled] + 63) // 64
        rec["lds_per_wave"] = rec["lds"] / rec["waves_per_workgroup"]
        # wavefronts per SIMD that the LDS alone admits (whole workgroups per CU; never more than the hardware's eight)
        rec["lds_waves_per_simd"] = min(MAX_WAVES_PER_SIMD, (LDS_PER_CU // rec["lds"]) * rec["waves_per_workgroup"] / SIMDS_PER_CU) if rec["lds"] else MAX_WAVES_PER_SIMD
        out[short_name(names[mangled])] = rec
    return out


def step_table(extra_flags=None):
    cache, rows = {}, []
    for src, prefix in STEP_KERNELS:
        if src not in cache:
            cache[src] = resources(src, extra_flags)
        hits = [k for k in cache[src] if k == prefix or k.startswith(prefix + "<")]
        if not hits:
            raise RuntimeError("no kernel %s in %s (has: %s)" % (prefix, src, ", ".join(sorted(cache[src]))))
        for k in hits:
            rows.append((src, k, cache[src][k]))
    return rows


def _print(rows):
    print("%-18s %-34s %5s %7s %9s %9s %5s %10s" % ("file", "kernel", "VGPR", "scratch", "LDS/block", "LDS/wave", "occ", "LDS admits"))
    for src, k, r in rows:
        adm = "%.1f" % r["lds_waves_per_simd"]
        print("%-18s %-34s %5d %7d %9d %9d %5d %10s" % (src, k, r["vgprs"] + r.get("agprs", 0), r["scratch"], r["lds"], r["lds_per_wave"], r["occupancy"], adm))


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if args:
        rows = [(src, k, r) for src in args for k, r in sorted(resources(os.path.basename(src)).items())]
    else:
        rows = step_table()
    if "--json" in sys.argv:
        print(json.dumps({k: r for _, k, r in rows}, indent=1, sort_keys=True))
    else:
        _print(rows)
