#!/usr/bin/env python3
"""The instruction mix of a kernel's loops, read from the gfx950 assembly without a GPU.

  python tools/loop_mix.py gauss.hip                   # the largest loop body of every kernel of the file
  python tools/loop_mix.py --top 3 gauss.hip           # the three largest loop bodies of every kernel (k_gauss7 has one per walk)
  python tools/loop_mix.py --json --top 3 octree.hip   # the same as one JSON object
  python tools/loop_mix.py --with v_dot4 octree.hip    # only loops whose body holds an instruction with this prefix (the blur's walks)
  python tools/loop_mix.py --asm file.s                # an assembly file made earlier (another commit's, for a comparison)

The file is compiled for the device alone with the flags of u-vip-slam_amd/build.py (+ UVO_EXTRA_FLAGS, as build.py does) and -S.  A
loop is what the compiler's block comments say it is: every block "in Loop: Header=..." (an inner loop belongs to the body of the loop
around it too).  Instructions are classed by the prefix of their mnemonic alone:
  vector  v_...                      LDS     ds_...
  memory  global_ flat_ buffer_ scratch_ and the scalar loads      wait    s_wait...
  branch  s_branch, s_cbranch_...    scalar  every other s_...
"saveexec" counts the scalar instructions that open an EXEC region (they are part of `scalar` too).  `control` is `scalar` when every
branch that decides whether the loop goes on -- to its header or out of it -- tests SCC or a VCC written by the scalar unit, i.e. a
compare of scalar registers, and `vector` when one of them tests EXEC or a VCC written by a per-lane compare: a divergent loop.
"""
import importlib.util
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = ("vector", "scalar", "branch", "lds", "memory", "wait")


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def assembly(src, extra_flags=None):
    b = _load("uvo_build", os.path.join(ROOT, "u-vip-slam_amd", "build.py"))
    extra = os.environ.get("UVO_EXTRA_FLAGS", "").split() if extra_flags is None else list(extra_flags)
    cmd = [b.HIPCC] + b.FLAGS + extra + ["--offload-device-only", "-S", "-o", "-", os.path.join(b.CSRC, os.path.basename(src))]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("hipcc failed for %s:\n%s\n%s" % (src, " ".join(cmd), r.stderr[-4000:]))
    return r.stdout


def classify(mnemonic):
    if mnemonic.startswith("v_"):
        return "vector"
    if mnemonic.startswith("ds_"):
        return "lds"
    if mnemonic.startswith(("global_", "flat_", "buffer_", "scratch_", "s_load", "s_buffer_load")):
        return "memory"
    if mnemonic.startswith("s_wait"):
        return "wait"
    if mnemonic.startswith(("s_branch", "s_cbranch")):
        return "branch"
    if mnemonic.startswith("s_"):
        return "scalar"
    return None


def kernels(asm):
    """-> {mangled kernel name: [lines of its body]}"""
    names = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M))
    out, cur = {}, None
    for line in asm.split("\n"):
        m = re.match(r"^([A-Za-z_$][\w$.]*):", line)
        if m and m.group(1) in names:
            cur = out.setdefault(m.group(1), [])
            continue
        if cur is not None:
            if line.lstrip().startswith(".end_amdhsa_kernel") or re.match(r"^\s*\.Lfunc_end", line):
                cur = None
                continue
            cur.append(line)
    return out


def loops(lines, having=None):
    """the loops of a kernel body as the compiler's own block comments name them ("in Loop: Header=BBn_m", "Parent Loop BBn_m"), if `having`
    is given only those whose body holds an instruction that starts with it
    -> [{label, control, instructions, <classes>, saveexec}], largest first"""
    body, member, chain, prev, vcc_vector = {}, {}, [], None, False
    control = {}                                  # loop -> [(mnemonic, target, vcc written by a vector compare)]
    for line in lines:
        text, _, comment = line.partition(";")
        text = text.strip()
        m = re.match(r"^\.L(BB\d+_\d+):", text) or re.match(r"^\s*; %(bb\.\d+):", line)
        if m:                                     # a block starts: its loops are on this line and on the "Parent Loop" lines that follow
            own = re.search(r"in Loop: Header=(BB\d+_\d+)", line)
            chain = [own.group(1)] if own else ([m.group(1)] if "Loop Header" in line else [])
            member[m.group(1)] = chain
            prev = m.group(1)
            continue
        m = re.match(r"^\s*;\s+Parent Loop (BB\d+_\d+)", line)
        if m and prev is not None:
            member[prev] = chain = member[prev] + [m.group(1)]
            continue
        if not text or text.startswith("."):
            continue
        prev = None
        parts = text.split(None, 1)
        mn, ops = parts[0], (parts[1] if len(parts) > 1 else "")
        if ops.split(",")[0].strip() == "vcc" or (mn.startswith("v_cmp") and mn.endswith("_e32")):
            vcc_vector = mn.startswith("v_")
        for lp in chain:
            body.setdefault(lp, []).append(mn)
            if classify(mn) == "branch":
                control.setdefault(lp, []).append((mn, ops.strip().lstrip(".L"), vcc_vector))
    out = []
    for lp, insts in body.items():
        if having and not any(m_.startswith(having) for m_ in insts):
            continue
        # the branches that decide whether the loop goes on: to its header, or out of it
        kinds = set()
        for mn, target, vec in control.get(lp, []):
            if target != lp and lp in member.get(target, []):
                continue                          # a branch inside the body (around an EXEC region, to a latch block)
            kinds.add("scalar" if mn.startswith("s_cbranch_scc") or mn == "s_branch" or (mn.startswith("s_cbranch_vcc") and not vec) else "vector")
        rec = {"label": lp, "control": "vector" if "vector" in kinds else "scalar", "instructions": len(insts), "saveexec": sum(1 for m_ in insts if "saveexec" in m_)}
        for c in CLASSES:
            rec[c] = sum(1 for m_ in insts if classify(m_) == c)
        out.append(rec)
    out.sort(key=lambda r: -r["instructions"])
    return out


def loop_mix(src=None, top=1, extra_flags=None, asm=None, having=None):
    """-> {short kernel name: the `top` largest loop bodies}"""
    kr = _load("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    b = _load("uvo_build", os.path.join(ROOT, "u-vip-slam_amd", "build.py"))
    text = assembly(src, extra_flags) if asm is None else asm
    per = kernels(text)
    names = kr._demangle(list(per), b.HIPCC)
    return {kr.short_name(names[k]): loops(v, having)[:top] for k, v in per.items()}


def _print(mix):
    print("%-28s %-10s %6s %6s %6s %6s %5s %6s %5s %8s  %s" % ("kernel", "loop", "insts", "vector", "scalar", "branch", "LDS", "memory", "wait", "saveexec", "control"))
    for k in sorted(mix):
        for r in mix[k]:
            print("%-28s %-10s %6d %6d %6d %6d %5d %6d %5d %8d  %s" % (k, r["label"], r["instructions"], r["vector"], r["scalar"], r["branch"], r["lds"], r["memory"],
                                                                   r["wait"], r["saveexec"], r["control"]))


if __name__ == "__main__":
    argv = sys.argv[1:]
    top, as_json, from_asm, having, files = 1, False, False, None, []
    while argv:
        a = argv.pop(0)
        if a == "--top":
            top = int(argv.pop(0))
        elif a == "--with":
            having = argv.pop(0)
        elif a == "--json":
            as_json = True
        elif a == "--asm":
            from_asm = True
        else:
            files.append(a)
    if not files:
        sys.exit(__doc__)
    mix = {}
    for f in files:
        mix.update(loop_mix(top=top, asm=open(f).read(), having=having) if from_asm else loop_mix(f, top=top, having=having))
    if as_json:
        print(json.dumps(mix, indent=1, sort_keys=True))
    else:
        _print(mix)
