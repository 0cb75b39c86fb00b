"""The load records (csrc/step_table.h: quad 3 of the pair rows, the pair
set-up records, the equality records) on the CPU: a stand-alone program built
with the address / undefined-behaviour sanitizers turns every bundled model's
packed blob, and two models edited here (an equality without a second joint,
a condim-1 pair), into the records; every field is compared with the chained
lookup in the model arrays that the kernels made before -- integers exact,
floats bit for bit.  Nothing is loaded into Python."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from manipulator_mujoco_amd import models
from model_ref import NEQ, NP, TABLE, f4, frames, i4

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = tuple(dict.fromkeys(models.PLANNER_SCENES + ("hande_scene", "dual_arm")))
CASES = [(n, 0.05) for n in NAMES] + [("scene_mjx", 0.02), ("eq_one_joint", 0.05), ("condim1", 0.05)]
u4 = np.uint32

PAIRJ = np.dtype([("mask1", u4), ("mask2", u4), ("trees", i4), ("mu", f4)])
SETUP = np.dtype([("func", i4), ("slotadr", i4), ("g1", i4), ("g2", i4), ("types", i4), ("rbound1", f4),
                  ("rbound2", f4), ("margin", f4), ("size1", f4, 3), ("pad0", f4), ("size2", f4, 3), ("pad1", f4)])
EQ = np.dtype([("qadr1", i4), ("dadr1", i4), ("qadr2", i4), ("dadr2", i4), ("qpos0_1", f4), ("qpos0_2", f4),
               ("c0", f4), ("c1", f4), ("c2", f4), ("c3", f4), ("c4", f4), ("pad", f4)])
RECORDS = np.dtype([("pair", SETUP, NP), ("eq", EQ, NEQ)])
CONDIM1_PAIR = 58  # the pair made frictionless in the "condim1" model: the box on the table, four live contacts


def edited(name):
    """The two edited models (also tests/test_gpu_step_records.py)."""
    m = models.load("scene_mjx", 0.05)
    if name == "eq_one_joint":
        m.eq_obj2 = np.array(m.eq_obj2)
        m.eq_obj2[0] = -1
    else:
        m.pair_condim = np.array(m.pair_condim)
        m.pair_condim[CONDIM1_PAIR] = 1
    return m


def load(name, dt):
    return edited(name) if name in ("eq_one_joint", "condim1") else models.load(name, dt)


@pytest.fixture(scope="module")
def records(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("step_records")
    exe = str(d / "step_records_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-static-libasan", "-static-libubsan", "-o", exe,
                    os.path.join(ROOT, "tests", "c_host", "step_records_host.cpp")], check=True)
    blobs, ms = [], {}
    for name, dt in CASES:
        m = load(name, dt)
        path = str(d / f"{name}_{dt}.mpcrm")
        m.save(path)
        blobs.append(path)
        ms[(name, dt)] = (m, path)
    r = subprocess.run([exe] + blobs, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
    out = {}
    for key, (m, path) in ms.items():
        raw = np.fromfile(path + ".rec", dtype=np.uint8)
        assert list(raw[:16].view(np.int32)) == [RECORDS.itemsize, SETUP.itemsize, EQ.itemsize, PAIRJ.itemsize]
        assert raw.size == 16 + TABLE.itemsize + RECORDS.itemsize
        table = raw[16:16 + TABLE.itemsize].view(TABLE)[0]
        out[key] = (m, table, raw[16 + TABLE.itemsize:].view(RECORDS)[0])
    return out


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def same_bits(got, ref, what):
    """got (fp32 of the record) is the model's float64 value rounded once to fp32."""
    assert np.array_equal(bits(got), bits(np.asarray(ref, np.float64).astype(np.float32))), what


def geom_map(m):
    """Collision geoms in order of first appearance over the pairs (the device model's numbering)."""
    g = {}
    for p in range(int(m.npair)):
        for k in (int(m.pair_geom1[p]), int(m.pair_geom2[p])):
            g.setdefault(k, len(g))
    return g


@pytest.mark.parametrize("case", CASES, ids=[f"{n}-{dt}" for n, dt in CASES])
def test_pair_records(records, case):
    m, t, r = records[case]
    _, dmap, _, _, tree = frames(m)
    gmap = geom_map(m)
    for p in range(int(m.npair)):
        g1, g2 = int(m.pair_geom1[p]), int(m.pair_geom2[p])
        b1, b2 = int(m.geom_bodyid[g1]), int(m.geom_bodyid[g2])
        q = np.frombuffer(t["row"][p].tobytes()[48:64], dtype=PAIRJ)[0]  # quad 3
        assert q["mask1"] == (int(m.body_dofmask[b1]) if b1 in dmap else 0), f"pair {p} mask1"
        assert q["mask2"] == (int(m.body_dofmask[b2]) if b2 in dmap else 0), f"pair {p} mask2"
        t1, t2 = (tree[b1] if b1 in dmap else 0), (tree[b2] if b2 in dmap else 0)
        assert q["trees"] == (t1 | t2 << 8 | (1 << 16 if int(m.pair_condim[p]) == 1 else 0)), f"pair {p} trees"
        same_bits(q["mu"], m.pair_friction[p], f"pair {p} mu")
        s = r["pair"][p]
        assert s["func"] == int(m.pair_func[p]) and s["slotadr"] == int(m.pair_slotadr[p]), f"pair {p}"
        assert s["g1"] == gmap[g1] and s["g2"] == gmap[g2], f"pair {p} geoms"
        assert s["types"] == (int(m.geom_type[g1]) | int(m.geom_type[g2]) << 8 | int(m.pair_ncon[p]) << 16), f"pair {p}"
        same_bits(s["rbound1"], m.geom_rbound[g1], f"pair {p} rbound1")
        same_bits(s["rbound2"], m.geom_rbound[g2], f"pair {p} rbound2")
        same_bits(s["margin"], np.float64(m.pair_margin[p]) - np.float64(m.pair_gap[p]), f"pair {p} margin")
        same_bits(s["size1"], m.geom_size[g1], f"pair {p} size1")
        same_bits(s["size2"], m.geom_size[g2], f"pair {p} size2")
    assert not r["pair"][int(m.npair):].tobytes().strip(b"\0"), "records past npair are zero"


@pytest.mark.parametrize("case", CASES, ids=[f"{n}-{dt}" for n, dt in CASES])
def test_equality_records(records, case):
    m, _, r = records[case]
    for e in range(int(m.neq)):
        q = r["eq"][e]
        if int(m.eq_type[e]) != 2:  # connect (dual arm): no record
            assert (q["qadr1"], q["dadr1"], q["qadr2"], q["dadr2"]) == (-1, -1, -1, -1)
            continue
        j1, j2 = int(m.eq_obj1[e]), int(m.eq_obj2[e])
        assert q["qadr1"] == int(m.jnt_qposadr[j1]) and q["dadr1"] == int(m.jnt_dofadr[j1])
        same_bits(q["qpos0_1"], m.qpos0[int(m.jnt_qposadr[j1])], "qpos0_1")
        if j2 >= 0:
            assert q["qadr2"] == int(m.jnt_qposadr[j2]) and q["dadr2"] == int(m.jnt_dofadr[j2])
            same_bits(q["qpos0_2"], m.qpos0[int(m.jnt_qposadr[j2])], "qpos0_2")
        else:
            assert q["qadr2"] == -1 and q["dadr2"] == -1 and bits(q["qpos0_2"]) == 0
        for k in range(5):
            same_bits(q[f"c{k}"], m.eq_data[e][k], f"eq {e} c{k}")


def test_edited_models_take_their_paths(records):
    """The edits are in the blobs: one equality without a second joint, one frictionless pair."""
    m, t, r = records[("eq_one_joint", 0.05)]
    assert int(m.neq) == 1 and r["eq"][0]["qadr2"] == -1 and r["eq"][0]["qadr1"] >= 0
    m, t, r = records[("condim1", 0.05)]
    trees = np.frombuffer(t["row"][:int(m.npair)]["qposadr"].tobytes(), dtype=i4)
    assert [p for p in range(int(m.npair)) if trees[p] >> 16 & 1] == [CONDIM1_PAIR]
