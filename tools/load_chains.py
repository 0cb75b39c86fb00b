#!/usr/bin/env python3
"""Where do the single-arm rollout kernels wait for model loads?  (static, no GPU)

    python tools/load_chains.py [TREE] [--kernel SUBSTR] [-D...]

Compiles TREE's (default: this tree's) rollout_narrow.hip to device assembly
with build.py's flags for the unit, twice:

* with -DMPCR_PROFILE, and cuts each rollout_kernel's listing at the
  s_memtime stamps (segments in listing order, which is the source order of
  the STAMP()s as far as the compiler keeps the blocks in it); per segment:
  instructions, VALU, global loads, s_waitcnt vmcnt, and loads whose wait is
  the very next instruction;
* as shipped, and prints the same as one total per kernel.

A wait right behind its load is a full memory latency with nothing under it;
several in a row are a dependent chain.  The numbers are static: a segment
with loops is counted once.  Extra -D flags go to both compiles
(-DMPCR_STEP_TABLE=7: the build without the load records).
"""
import importlib.util
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_build(tree):
    path = os.path.join(tree, "manipulator_mujoco_amd", "build.py")
    spec = importlib.util.spec_from_file_location("build_lc", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def listing(b, extra):
    """Device assembly of the narrow unit: {kernel name: [instruction, ...]}."""
    src, flags = next((u[0], u[1]) for u in b.UNITS if u[0].endswith("rollout_narrow.hip"))
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "narrow.s")
        subprocess.run([b.hipcc(), f"--offload-arch={b.ARCH}", "--cuda-device-only", "-S"] + b.FLAGS + flags + extra +
                       ["-o", out, src], check=True)
        with open(out) as f:
            lines = f.read().split("\n")
    kernels, cur = {}, None
    for ln in lines:
        m = re.match(r"^(_Z[\w$.]+):", ln)
        if m:
            cur = kernels.setdefault(m.group(1), []) if "rollout_kernel" in m.group(1) else None
            continue
        if cur is None:
            continue
        if ln.startswith("\t.end_amdhsa_kernel") or ln.startswith(".Lfunc_end"):
            cur = None
            continue
        t = ln.split(";")[0].strip()
        if t and not t.startswith(".") and not t.endswith(":"):
            cur.append(t)
    return kernels


def counts(ins):
    loads = [i for i, t in enumerate(ins) if t.startswith("global_load")]
    at_once = sum(1 for i in loads if i + 1 < len(ins) and re.match(r"s_waitcnt\b.*vmcnt", ins[i + 1]))
    return {"instructions": len(ins), "valu": sum(t.startswith("v_") for t in ins), "global_loads": len(loads),
            "vmcnt_waits": sum(bool(re.match(r"s_waitcnt\b.*vmcnt", t)) for t in ins), "load_then_wait": at_once}


def segments(ins):
    cuts = [i for i, t in enumerate(ins) if t.startswith("s_memtime")]
    return [ins[a:b] for a, b in zip([0] + cuts, cuts + [len(ins)])]


def short(name):
    m = re.search(r"rollout_kernelILi(\d+)ELi(\d+)ELi(\d+)ELb(\d)ELi(\d)ELb(\d)ELb(\d)", name)
    return "rollout_kernel<%s,%s,%s,%s,%s,%s,%s>" % m.groups() if m else name


ROW = "{:>5} {:>7} {:>6} {:>6} {:>6} {:>10}"


def main():
    args = sys.argv[1:]
    extra = [a for a in args if a.startswith("-D")]
    only = args[args.index("--kernel") + 1] if "--kernel" in args else None
    pos = [a for i, a in enumerate(args) if not a.startswith("-") and (i == 0 or args[i - 1] != "--kernel")]
    tree = os.path.abspath(pos[0]) if pos else ROOT
    b = load_build(tree)
    prof, ship = listing(b, extra + ["-DMPCR_PROFILE"]), listing(b, extra)
    print(f"tree {tree}  source {b.source_hash()}  flags {' '.join(extra) or '(shipped)'}")
    for name, ins in ship.items():
        if only and only not in short(name):
            continue
        print(f"\n{short(name)}")
        print(ROW.format("seg", "instr", "VALU", "loads", "waits", "load+wait"))
        for k, seg in enumerate(segments(prof.get(name, []))):
            c = counts(seg)
            print(ROW.format(k, c["instructions"], c["valu"], c["global_loads"], c["vmcnt_waits"], c["load_then_wait"]))
        c = counts(ins)
        print(ROW.format("ship", c["instructions"], c["valu"], c["global_loads"], c["vmcnt_waits"], c["load_then_wait"]))


if __name__ == "__main__":
    main()
