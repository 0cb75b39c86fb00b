#!/usr/bin/env python3
"""Is the device code of two source trees the same?  A plain text diff.

    python tools/isa_identity.py OLD_TREE NEW_TREE [--keep DIR] [-j N] [--functions] [--strip-new TEXT]

For each unit of build.UNITS (paired by position: engine, rollout, the
dual-arm rollout) both trees' source is compiled to device-only assembly with
that tree's own flags for the unit (hipcc --cuda-device-only -S), the lines
naming __hip_cuid_ are dropped (the symbol hashes the source path: the only
thing two builds of the same text differ in) and the rest is compared line by
line.  Prints, per unit, `identical` or the first differing function and how
many lines differ; exit status 1 on any difference.  With --functions a unit
that differs is also broken down by function: which ones differ, and whether
in integer literals alone (a changed struct size or field offset folded into
an instruction) or in their instructions.  --strip-new TEXT drops TEXT from
every line of the new tree's listings first: where the new tree lengthens a
kernel's argument list, its mangled names gain a suffix (an argument of type
mpcr::StepWArgs adds NS_9StepWArgsE) and the functions pair up again without
it.  No GPU needed.
"""
import argparse
import importlib.util
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor


def load_build(tree):
    path = os.path.join(tree, "manipulator_mujoco_amd", "build.py")
    spec = importlib.util.spec_from_file_location("build_" + str(abs(hash(path))), path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def unit_cmds(b):
    """One hipcc -S command (without -o) per unit of a tree's build.py."""
    cmds = []
    for src, flags, *rest in b.UNITS:
        # trees before the (src, flags, precise) units marked a precise unit by "PRECISE" in its flags
        precise = rest[0] if rest else "PRECISE" in flags
        fl = b.FLAGS + [f for f in flags if f != "PRECISE"]
        if precise:
            fl = b._drop_fast(fl)
        cmds.append((src, [b.hipcc(), f"--offload-arch={b.ARCH}", "--cuda-device-only", "-S"] + fl + [src]))
    return cmds


def assembly(cmd, out, strip=None):
    """Compile, drop the __hip_cuid_ lines (and every occurrence of `strip`) in place, return the lines."""
    subprocess.run(cmd + ["-o", out], check=True)
    with open(out) as f:
        lines = [ln.replace(strip, "") if strip else ln for ln in f if "__hip_cuid_" not in ln]
    with open(out, "w") as f:
        f.writelines(lines)
    return lines


def first_function(old, new, old_path, new_path):
    """The function label above the first differing line, and diff's count of differing lines."""
    first = next((i for i, (x, y) in enumerate(zip(old, new)) if x != y), min(len(old), len(new)))
    label = None
    for ln in reversed(old[:first + 1]):
        m = re.match(r"^([A-Za-z_.$][\w.$]*):", ln)
        if m and not m.group(1).startswith(".L"):
            label = m.group(1)
            break
    out = subprocess.run(["diff", old_path, new_path], capture_output=True, text=True).stdout
    return label, sum(ln[:1] in "<>" for ln in out.splitlines())


_LABEL = re.compile(r"^([A-Za-z_$][\w.$]*):")
_NUM = re.compile(r"(?<![\w.])(0x[0-9a-fA-F]+|\d+)(?![\w.])")


def functions(lines):
    """{label: its lines} for every global label of an assembly listing (local .L labels stay inside)."""
    out, cur = {}, None
    for ln in lines:
        m = _LABEL.match(ln)
        if m:
            cur = m.group(1)
            out[cur] = []
        elif cur is not None:
            out[cur].append(ln)
    return out


def per_function(old, new):
    """Per function present in both listings and not line-for-line equal:
    `literals` when the two differ in integer literals alone (same opcodes,
    registers and order; the (old, new) literal pairs are listed), else
    `DIFFERENT`.  Functions in only one listing are named."""
    fo, fn = functions(old), functions(new)
    rows = []
    for name in fo:
        if name not in fn:
            rows.append((name, "only in old", ""))
            continue
        a, b = fo[name], fn[name]
        if a == b:
            continue
        pairs = set()
        same = len(a) == len(b)
        for x, y in zip(a, b) if same else ():
            if x == y:
                continue
            if _NUM.sub("#", x) != _NUM.sub("#", y):
                same = False
                break
            pairs.update((p, q) for p, q in zip(_NUM.findall(x), _NUM.findall(y)) if p != q)
        if same:
            nd = sum(x != y for x, y in zip(a, b))
            rows.append((name, "literals", f"{nd} of {len(a)} lines: " + ", ".join(f"{p}->{q}" for p, q in sorted(pairs))))
        else:
            rows.append((name, "DIFFERENT", f"{len(a)} vs {len(b)} lines"))
    rows += [(name, "only in new", "") for name in fn if name not in fo]
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--keep", help="write the assembly files here instead of a temporary directory")
    ap.add_argument("-j", type=int, default=3, help="compiles in flight")
    ap.add_argument("--functions", action="store_true",
                    help="for a unit that differs, also say per function how: integer literals alone, or more")
    ap.add_argument("--strip-new", metavar="TEXT",
                    help="drop TEXT from the new tree's listings before comparing (a mangled-name suffix)")
    a = ap.parse_args()
    old, new = unit_cmds(load_build(a.old)), unit_cmds(load_build(a.new))
    if len(old) != len(new):
        sys.exit(f"{len(old)} units in {a.old}, {len(new)} in {a.new}")
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(a.j) as pool:
        d = a.keep or tmp
        os.makedirs(d, exist_ok=True)
        jobs = [(pool.submit(assembly, o[1], os.path.join(d, f"old{i}.s")),
                 pool.submit(assembly, n[1], os.path.join(d, f"new{i}.s"), a.strip_new)) for i, (o, n) in enumerate(zip(old, new))]
        bad = 0
        for i, ((o, n), (fo, fn)) in enumerate(zip(zip(old, new), jobs)):
            so, sn = fo.result(), fn.result()
            names = f"{os.path.basename(o[0])} -> {os.path.basename(n[0])}"
            if so == sn:
                print(f"{names}: identical ({len(so)} lines)")
            else:
                label, ndiff = first_function(so, sn, os.path.join(d, f"old{i}.s"), os.path.join(d, f"new{i}.s"))
                print(f"{names}: DIFFERENT, first in {label}, {ndiff} lines differ ({len(so)} vs {len(sn)} lines)")
                bad = 1
                if a.functions:
                    rows = per_function(so, sn)
                    for name, kind, detail in rows:
                        print(f"  {name}: {kind}" + (f" ({detail})" if detail else ""))
                    print(f"  every other function of the unit: identical")
    return bad


if __name__ == "__main__":
    sys.exit(main())
