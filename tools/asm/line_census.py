"""Static instruction census of rollout_kernel by source region (diagnostic).

Compile the device code with line tables, e.g.
    hipcc --offload-arch=gfx950 --cuda-device-only -S -O3 -gline-tables-only <FLAGS> -o ship.s csrc/rollout_narrow.hip
    python tools/asm/line_census.py ship.s [narrow|wide]
(csrc/rollout_wide.hip for the wide kernels.)
Each instruction is charged to the last line of rollout.hip or of one of the
csrc/ headers it includes (.loc, by its .file number) seen before it; lines
are grouped into the enclosing __device__ helper of that file, or, inside the
kernel body, into the phase between two STAMP(k) markers.  Loop bodies
count once (static), so multiply by trip counts when reading.
"""
import collections
import os
import re
import sys

path = sys.argv[1]
which = sys.argv[2] if len(sys.argv) > 2 else "narrow"
tag = "ILi16ELi16ELi24ELb0E" if which == "narrow" else "ILi32ELi32ELi72ELb1E"
CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "manipulator_mujoco_amd", "csrc")


def file_regions(name):
    """(start_line, name) of a source file: helper functions (by signature line) and kernel phases (by STAMP)."""
    regions = []
    kern = None
    for i, l in enumerate(open(os.path.join(CSRC, name)).read().splitlines(), 1):
        m = re.match(r"^(?:template <[^>]*>\s*)?__(?:device|global)__[^(]*?\b(\w+)\s*\(",
                     re.sub(r"__attribute__\(\(.*?\)\)\)?", "", l))  # (an address-space return type is not the name)
        if m:
            regions.append((i, m.group(1)))
            if "__global__" in l:
                kern = i
        m = re.search(r"STAMP\((\d+)\);", l)
        if m and kern and i > kern:
            regions.append((i, f"kernel@after-STAMP{m.group(1)}"))
    return sorted(regions)


def region(regions, line):
    name = "?"
    for s, n in regions:
        if s <= line:
            name = n
        else:
            break
    return name


lines = open(path).read().splitlines()
# .file number -> regions, for rollout.hip and the csrc/ headers (the kernel's device functions)
kfiles = {}
for l in lines:
    f = l.split()
    if len(f) > 2 and f[0] == ".file" and f[1].isdigit():
        name = os.path.basename(re.findall(r'"([^"]*)"', l)[-1])
        if name == "rollout.hip" or (name.endswith(".h") and os.path.exists(os.path.join(CSRC, name))):
            kfiles[f[1]] = file_regions(name)
start = next(i for i, l in enumerate(lines) if l.startswith("_ZN4mpcr14rollout_kernel" + tag) and ":" in l)
end = next(i for i in range(start, len(lines)) if lines[i].strip().startswith(".Lfunc_end"))
cur = "?"
per = collections.defaultdict(collections.Counter)
for l in lines[start:end]:
    s = l.strip()
    if s.startswith(".loc"):
        f = s.split()
        if f[1] in kfiles:
            cur = region(kfiles[f[1]], int(f[2]))
        continue
    if not s or s.startswith(";") or s.startswith(".") or s.endswith(":"):
        continue
    op = s.split()[0]
    cls = ("valu" if op.startswith("v_") else "lds" if op.startswith("ds_") else
           "vmem" if op.startswith(("global_", "buffer_", "flat_")) else "smem" if op.startswith("s_load") else
           "ctl" if op.startswith(("s_waitcnt", "s_cbranch", "s_branch", "s_barrier", "s_nop")) else "salu")
    r = cur
    per[r][cls] += 1
    per[r]["all"] += 1
tot = collections.Counter()
for r, c in sorted(per.items(), key=lambda kv: -kv[1]["all"]):
    tot.update(c)
    print(f"{r:34s} " + " ".join(f"{k}={c[k]:5d}" for k in ("all", "valu", "salu", "lds", "vmem", "smem", "ctl")))
print(f"{'TOTAL':34s} " + " ".join(f"{k}={tot[k]:5d}" for k in ("all", "valu", "salu", "lds", "vmem", "smem", "ctl")))
