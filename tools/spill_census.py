#!/usr/bin/env python3
"""Scalar-register spills of the single-arm rollout kernels, from the assembly.

    python tools/spill_census.py [TREE] [--json] [--keep FILE]

Compiles TREE's (default: this checkout's) rollout_narrow.hip to device-only
assembly with that tree's build.py flags for the unit and prints, per
rollout_kernel instantiation:

  * .sgpr_count, .sgpr_spill_count, .vgpr_count, .vgpr_spill_count of the
    kernel metadata and codeLenInByte;
  * the spill VGPRs.  The compiler spills scalars to lanes of a VGPR, not to
    scratch, so the resource remarks show nothing.  A spill VGPR is identified
    as a register that the listing only ever writes with v_writelane_b32 and
    only ever reads with v_readlane_b32: no other instruction names it (a
    VGPR the algorithm moves lanes of is also read or written by ordinary
    vector instructions);
  * the spill stores (v_writelane_b32 into a spill VGPR) and reloads
    (v_readlane_b32 out of one), counted outside the horizon loop, at loop
    depth 1 (the horizon loop's own blocks) and deeper, from the loop
    annotations of the listing.  The horizon loop is the depth-1 loop with
    the most instructions;
  * VALU instructions in all (v_* opcodes) and the v_readlane_b32 that are
    not reloads;
  * the ten most reloaded slots (VGPR, lane), how many of the reloads are in
    the horizon loop, and the opcode that first consumes the reloaded SGPR.

No GPU needed.
"""
import argparse
import importlib.util
import json
import os
import re
import subprocess
import sys
import tempfile
from collections import Counter

# (waves per candidate 1 or 2: the scenario instantiations, which add WPCS_SCEN to it, are not part of the census)
KERNEL = re.compile(r"^(_ZN4mpcr14rollout_kernelILi(\d+)ELi(\d+)ELi(\d+)ELb([01])ELi([12])ELb([01])ELb([01])E\w+):")
_BLOCK = re.compile(r"^(?:\.L(BB\d+_\d+):|; %bb\.(\d+):)(.*)$")
_INSN = re.compile(r"^\t([a-z][a-z0-9_]+)(?:\s+(.*))?$")
_VREG = re.compile(r"\bv(\d+)\b|\bv\[(\d+):(\d+)\]")
_SREG = re.compile(r"\bs(\d+)\b|\bs\[(\d+):(\d+)\]")


def load_build(tree):
    path = os.path.join(tree, "manipulator_mujoco_amd", "build.py")
    spec = importlib.util.spec_from_file_location("build_" + str(abs(hash(path))), path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def narrow_asm(tree, out):
    """Compile the tree's rollout_narrow.hip to device assembly at `out`."""
    b = load_build(tree)
    for src, flags, *rest in b.UNITS:
        if os.path.basename(src) == "rollout_narrow.hip":
            fl = b.FLAGS + list(flags)
            if rest and rest[0]:
                fl = b._drop_fast(fl)
            cmd = [b.hipcc(), f"--offload-arch={b.ARCH}", "--cuda-device-only", "-S"] + fl + ["-o", out, src]
            r = subprocess.run(cmd, stderr=subprocess.PIPE, text=True)
            if r.returncode != 0:
                sys.exit(f"{' '.join(cmd)}\n{r.stderr}\nhipcc failed on {src}")
            return
    sys.exit(f"{tree}: no rollout_narrow.hip among build.UNITS")


def short_name(m):
    nvw, nbw, ngw, wide, wpc, multi, state = m.groups()[1:]
    return f"rollout_kernel<{nvw},{nbw},{ngw},{'true' if wide == '1' else 'false'},{wpc}," \
           f"{'true' if multi == '1' else 'false'},{'true' if state == '1' else 'false'}>"


def _regs(rx, text):
    out = set()
    for a, lo, hi in rx.findall(text):
        if a:
            out.add(int(a))
        else:
            out.update(range(int(lo), int(hi) + 1))
    return out


def metadata(lines):
    """{mangled name: {field: int}} from the amdhsa.kernels notes."""
    out, cur = {}, None
    for ln in lines:
        if re.match(r"  - \.", ln):  # a kernel's entry opens (its fields are sorted by name)
            cur = {}
        if cur is None:
            continue
        m = re.match(r"    \.name:\s+(\S+)", ln)
        if m:
            out[m.group(1)] = cur
            continue
        m = re.match(r"(?:    |  - )\.(sgpr_count|sgpr_spill_count|vgpr_count|vgpr_spill_count|"
                     r"group_segment_fixed_size|private_segment_fixed_size):\s+(\d+)", ln)
        if m:
            cur[m.group(1)] = int(m.group(2))
    return out


def census(body):
    """The counts of one kernel's listing (its lines between label and End function)."""
    # pass 1: instructions with their block, each block's innermost loop header and depth
    insns = []      # (opcode, operands, block index)
    blocks = []     # (innermost header or None, depth)
    parents = {}    # header -> its parent headers, outermost first
    cur_header, cur_depth, pending = None, 0, None
    for ln in body:
        mb = _BLOCK.match(ln)
        if mb:
            label, rest = mb.group(1), mb.group(3)
            mi = re.search(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)", rest)
            mh = re.search(r"Loop Header: Depth=(\d+)", rest)
            if mi:
                blocks.append((mi.group(1), int(mi.group(2))))
                pending = None
            elif mh:
                blocks.append((label, int(mh.group(1))))
                parents.setdefault(label, [])
                pending = None
            else:
                blocks.append((None, 0))
                # a header inside another loop lists its parents first, then "=> This ... Loop Header"
                pending = label
                mp = re.search(r"Parent Loop (BB\d+_\d+) Depth=(\d+)", rest)
                if mp and label:
                    parents.setdefault(label, []).append(mp.group(1))
            continue
        if pending is not None and ln.lstrip().startswith(";"):
            mp = re.search(r"Parent Loop (BB\d+_\d+) Depth=(\d+)", ln)
            mh = re.search(r"Loop Header: Depth=(\d+)", ln)
            if mp:
                parents.setdefault(pending, []).append(mp.group(1))
                continue
            if mh:
                blocks[-1] = (pending, int(mh.group(1)))
                parents.setdefault(pending, [])
                pending = None
                continue
            if "Child Loop" in ln:
                continue
        mi = _INSN.match(ln)
        if mi and not ln.startswith("\t."):
            pending = None
            if not blocks:
                blocks.append((None, 0))
            insns.append((mi.group(1), (mi.group(2) or "").split(";")[0], len(blocks) - 1))

    def outermost(h):
        return parents[h][0] if parents.get(h) else h

    # the horizon loop: the depth-1 loop holding the most instructions
    size = Counter()
    for _, _, bi in insns:
        h = blocks[bi][0]
        if h is not None:
            size[outermost(h)] += 1
    horizon = size.most_common(1)[0][0] if size else None

    def where(bi):
        h, d = blocks[bi]
        if h is None or outermost(h) != horizon:
            return "outside"
        return "depth1" if d == 1 else "deeper"

    # pass 2: the spill VGPRs
    lane_w, lane_r, other = Counter(), Counter(), set()
    for op, args, _ in insns:
        if op == "v_writelane_b32":
            lane_w.update(_regs(_VREG, args.split(",")[0]))
            other.update(_regs(_VREG, ",".join(args.split(",")[1:])))
        elif op == "v_readlane_b32":
            lane_r.update(_regs(_VREG, args.split(",")[1]))
            other.update(_regs(_VREG, ",".join(args.split(",")[2:])))
        else:
            other.update(_regs(_VREG, args))
    spill = sorted(v for v in lane_w if v not in other)

    # pass 3: stores, reloads, consumers
    stores, reloads = Counter(), Counter()
    slot_all, slot_loop, slot_use = Counter(), Counter(), {}
    valu = other_readlane = 0
    for i, (op, args, bi) in enumerate(insns):
        if op.startswith("v_"):
            valu += 1
        if op == "v_writelane_b32":
            a = [x.strip() for x in args.split(",")]
            if _regs(_VREG, a[0]) & set(spill):
                stores[where(bi)] += 1
        elif op == "v_readlane_b32":
            a = [x.strip() for x in args.split(",")]
            src = _regs(_VREG, a[1])
            if not (src & set(spill)):
                other_readlane += 1
                continue
            w = where(bi)
            reloads[w] += 1
            slot = (f"v{min(src)}", a[2])
            slot_all[slot] += 1
            if w != "outside":
                slot_loop[slot] += 1
            dst = _regs(_SREG, a[0])
            for op2, args2, _ in insns[i + 1:i + 60]:
                ops2 = args2.split(",")
                srcs = ",".join(ops2[1:]) if len(ops2) > 1 and not op2.startswith(("s_cmp", "s_bitcmp", "s_cbranch",
                                                                                   "global_store", "flat_store",
                                                                                   "ds_write", "v_cmpx")) else args2
                if op2 in ("v_readlane_b32",):
                    continue
                if _regs(_SREG, srcs) & dst:
                    slot_use.setdefault(slot, Counter())[op2] += 1
                    break
    top = [{"slot": f"{v} lane {l}", "reloads": n, "in_loop": slot_loop[(v, l)],
            "consumers": dict(slot_use.get((v, l), Counter()).most_common(3))}
           for (v, l), n in slot_all.most_common(10)]
    return {"spill_vgprs": [f"v{v}" for v in spill], "horizon_loop": horizon, "valu_static": valu,
            "readlane_algorithm": other_readlane,
            "stores": {k: stores[k] for k in ("outside", "depth1", "deeper")},
            "reloads": {k: reloads[k] for k in ("outside", "depth1", "deeper")},
            "top_slots": top}


def run(tree, keep=None):
    with tempfile.TemporaryDirectory() as tmp:
        path = keep or os.path.join(tmp, "rollout_narrow.s")
        narrow_asm(tree, path)
        with open(path) as f:
            lines = f.read().split("\n")
    meta = metadata(lines)
    out, i = [], 0
    while i < len(lines):
        m = KERNEL.match(lines[i])
        if not m:
            i += 1
            continue
        j = next(k for k in range(i, len(lines)) if "-- End function" in lines[k])
        code = next((int(re.search(r"codeLenInByte = (\d+)", lines[k]).group(1)) for k in range(j, min(j + 40, len(lines)))
                     if "codeLenInByte" in lines[k]), None)
        row = {"kernel": short_name(m), "mangled": m.group(1), "codeLenInByte": code}
        row.update(meta.get(m.group(1), {}))
        row.update(census(lines[i + 1:j]))
        out.append(row)
        i = j + 1
    return out


def report(rows):
    for r in rows:
        st, rl = r["stores"], r["reloads"]
        print(r["kernel"])
        print(f"  sgpr_count {r.get('sgpr_count')}  sgpr_spill_count {r.get('sgpr_spill_count')}  "
              f"vgpr_count {r.get('vgpr_count')}  vgpr_spill_count {r.get('vgpr_spill_count')}  "
              f"codeLenInByte {r['codeLenInByte']}  LDS {r.get('group_segment_fixed_size')}  "
              f"scratch {r.get('private_segment_fixed_size')}")
        print(f"  spill VGPRs (written only by v_writelane_b32, read only by v_readlane_b32): "
              f"{', '.join(r['spill_vgprs']) or 'none'}")
        print(f"  horizon loop {r['horizon_loop']}; static VALU {r['valu_static']}; "
              f"v_readlane_b32 of the algorithm {r['readlane_algorithm']}")
        print(f"  spill stores   outside {st['outside']:4d}  depth 1 {st['depth1']:4d}  deeper {st['deeper']:4d}"
              f"  (in loop {st['depth1'] + st['deeper']})")
        print(f"  spill reloads  outside {rl['outside']:4d}  depth 1 {rl['depth1']:4d}  deeper {rl['deeper']:4d}"
              f"  (in loop {rl['depth1'] + rl['deeper']})")
        for t in r["top_slots"]:
            use = ", ".join(f"{k} x{v}" for k, v in t["consumers"].items())
            print(f"    {t['slot']:14s} reloads {t['reloads']:3d} (in loop {t['in_loop']:3d})  -> {use}")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("tree", nargs="?", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    ap.add_argument("--json", action="store_true", help="one JSON list instead of the text report")
    ap.add_argument("--keep", help="write the assembly to this file")
    a = ap.parse_args()
    rows = run(os.path.abspath(a.tree), a.keep)
    if a.json:
        print(json.dumps(rows, indent=1))
    else:
        report(rows)
    return 0


if __name__ == "__main__":
    sys.exit(main())
