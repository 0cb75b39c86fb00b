"""The step table (csrc/step_table.h) on the CPU: a stand-alone program built
with the address / undefined-behaviour sanitizers turns every bundled model's
packed blob into its table; every derived field is compared with the same
formula evaluated here in numpy float64 from the model arrays (<= 1 fp32 ulp;
integers and flags exact) and every resolved index with the chained lookup.
Nothing is loaded into Python."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from manipulator_mujoco_amd import models
from model_ref import (ANCHOR0, BK_FREE, BK_HINGE, BK_SLIDE, BK_WELD, BODY, CONDIM1, DOF, FREE, HINGE, LIMITED, MAXIMP,
                       MINIMP, MINVAL, NJ, NP, POW1, POW2, ROW, SLIDE, TABLE, close, frames, q2m, qmul)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = tuple(dict.fromkeys(models.PLANNER_SCENES + ("dual_arm",)))
# (model, timestep): the bundles at the planner's step and one at another, since K / B depend on it
CASES = [(n, 0.05) for n in NAMES] + [("scene_mjx", 0.02)]


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("step_table")
    exe = str(d / "step_table_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-static-libasan", "-static-libubsan", "-o", exe,
                    os.path.join(ROOT, "tests", "c_host", "step_table_host.cpp")], check=True)
    blobs, ms = [], {}
    for name, dt in CASES:
        m = models.load(name, dt)
        path = str(d / f"{name}_{dt}.mpcrm")
        m.save(path)
        blobs.append(path)
        ms[(name, dt)] = (m, path)
    r = subprocess.run([exe] + blobs, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
    out = {}
    for key, (m, path) in ms.items():
        raw = np.fromfile(path + ".step", dtype=np.uint8)
        sizes = raw[:16].view(np.int32)
        assert list(sizes) == [TABLE.itemsize, BODY.itemsize, DOF.itemsize, ROW.itemsize]
        out[key] = (m, raw[16:].view(TABLE)[0])
    return out


@pytest.mark.parametrize("case", CASES, ids=[f"{n}-{dt}" for n, dt in CASES])
def test_bodies_dofs(tables, case):
    m, t = tables[case]
    moving, dmap, wpos, wquat, tree = frames(m)
    assert t["nbody"] == len(moving)
    anchor0 = True
    for i, b in enumerate(moving):
        r = t["body"][i]
        p = int(m.body_parentid[b])
        j = int(m.body_jntadr[b]) if m.body_jntnum[b] else -1
        jt = int(m.jnt_type[j]) if j >= 0 else -1
        kind = BK_WELD if j < 0 else {FREE: BK_FREE, HINGE: BK_HINGE, SLIDE: BK_SLIDE}[jt]
        assert r["kind"] == kind
        if p in dmap:
            bp, bq = np.asarray(m.body_pos[b], np.float64), np.asarray(m.body_quat[b], np.float64)
            anc = dmap[p]
        else:
            bp = wpos[p] + q2m(wquat[p]) @ np.asarray(m.body_pos[b], np.float64)
            bq = qmul(wquat[p], np.asarray(m.body_quat[b], np.float64))
            anc = -1
        assert r["anc"] == (-1 if kind == BK_FREE else anc)
        assert r["qposadr"] == (int(m.jnt_qposadr[j]) if j >= 0 else -1)
        if j >= 0:
            close(r["qpos0"], m.qpos0[int(m.jnt_qposadr[j])], "qpos0")
        close(r["bquat"], bq, "bquat")
        close(r["bpos"], bp, "bpos")
        close(r["ipos"], m.body_ipos[b], "ipos")
        R = q2m(bq)
        close(r["R"][:, :3], R, "body R")
        if kind in (BK_HINGE, BK_SLIDE):
            ax = np.asarray(m.jnt_axis[j], np.float64)
            close(r["axis"], ax if kind == BK_HINGE else R @ ax, "axis")
            close(r["jpos"], m.jnt_pos[j], "jpos")
            anchor0 &= not np.any(np.asarray(m.jnt_pos[j], np.float32) != 0)
    assert (t["flags"] & ANCHOR0 != 0) == anchor0
    for i in range(int(m.nv)):
        r = t["dof"][i]
        j = int(m.dof_jntid[i])
        b = int(m.dof_bodyid[i])
        sub = i - int(m.jnt_dofadr[j])
        jt = int(m.jnt_type[j])
        assert r["body"] == dmap[b]
        assert r["kind"] == (0 if jt == HINGE else 1 if jt == SLIDE else (2 if sub < 3 else 3))
        assert r["tree"] == tree[b]
        assert r["sub"] == (sub if sub < 3 else sub - 3)
        close(r["axis"], m.jnt_axis[j], "dof axis")
        close(r["jpos"], m.jnt_pos[j], "dof jpos")


def row_ref(solref, solimp, dt, disableflags):
    """The row constants from solref / solimp / timestep in float64."""
    si = np.asarray(solimp, np.float64)
    dmin, dmax = np.clip(si[0], MINIMP, MAXIMP), np.clip(si[1], MINIMP, MAXIMP)
    width, mid, power = si[2], si[3], si[4]
    d = dmax
    flat = np.float32(dmin) == np.float32(dmax) or np.float32(width) <= MINVAL
    with np.errstate(divide="ignore"):
        iw, imid, i1mid = np.float64(1) / width, np.float64(1) / mid, np.float64(1) / (1 - mid)
    if flat:
        dmin = dmax = 0.5 * (np.float64(np.float32(dmin)) + np.float64(np.float32(dmax)))
        iw, mid, imid, i1mid = 0.0, 0.5, 2.0, 2.0
    tc, dr = np.float64(solref[0]), np.float64(solref[1])
    with np.errstate(divide="ignore"):
        if np.float32(tc) > 0:
            if not (disableflags & 2):
                tc = max(tc, 2 * dt)
            K, B = 1 / (d * d * tc * tc * dr * dr), 2 / (d * tc)
        else:
            K, B = -tc / (d * d), -dr / d
    fl = POW1 if flat else (POW2 if np.float32(power) == 2 else POW1 if np.float32(power) == 1 else 0)
    return dict(dmin=dmin, dmax=dmax, iwidth=iw, mid=mid, imid=imid, i1mid=i1mid, K=K, B=B, power=power), fl


def check_row(r, ref, fl, what):
    for k, v in ref.items():
        close(r[k], v, f"{what} {k}")
    assert (r["flags"] & (POW1 | POW2)) == fl, what


@pytest.mark.parametrize("case", CASES, ids=[f"{n}-{dt}" for n, dt in CASES])
def test_rows(tables, case):
    m, t = tables[case]
    dt, dis = float(m.timestep), int(m.disableflags)
    assert dt == case[1]
    for p in range(int(m.npair)):
        r = t["row"][p]
        ref, fl = row_ref(m.pair_solref[p], m.pair_solimp[p], dt, dis)
        check_row(r, ref, fl, f"pair {p}")
        mu = np.float64(m.pair_friction[p])
        invw = (np.float64(m.body_invweight0[int(m.geom_bodyid[int(m.pair_geom1[p])])][0]) +
                np.float64(m.body_invweight0[int(m.geom_bodyid[int(m.pair_geom2[p])])][0]))
        c1 = int(m.pair_condim[p]) == 1
        close(r["diag"], invw if c1 else invw * (1 + mu * mu), "pair diag")
        close(r["margin"], np.float64(m.pair_margin[p]) - np.float64(m.pair_gap[p]), "pair margin")
        assert bool(r["flags"] & CONDIM1) == c1
    for j in range(int(m.njnt)):
        r = t["row"][NP + j]
        ref, fl = row_ref(m.jnt_solref[j], m.jnt_solimp[j], dt, dis)
        check_row(r, ref, fl, f"joint {j}")
        close(r["margin"], m.jnt_margin[j], "jnt margin")
        close(r["diag"], m.dof_invweight0[int(m.jnt_dofadr[j])], "jnt diag")
        close(r["range"], m.jnt_range[j], "jnt range")
        assert r["qposadr"] == int(m.jnt_qposadr[j]) and r["dofadr"] == int(m.jnt_dofadr[j])
        assert bool(r["flags"] & LIMITED) == bool(m.jnt_limited[j] and int(m.jnt_type[j]) in (SLIDE, HINGE))
    for e in range(int(m.neq)):
        r = t["row"][NP + NJ + e]
        ref, fl = row_ref(m.eq_solref[e], m.eq_solimp[e], dt, dis)
        check_row(r, ref, fl, f"eq {e}")
        if int(m.eq_type[e]) == 2:
            diag = np.float64(m.dof_invweight0[int(m.jnt_dofadr[int(m.eq_obj1[e])])])
            if int(m.eq_obj2[e]) >= 0:
                diag += np.float64(m.dof_invweight0[int(m.jnt_dofadr[int(m.eq_obj2[e])])])
        else:
            diag = (np.float64(m.body_invweight0[int(m.eq_obj1[e])][0]) +
                    np.float64(m.body_invweight0[int(m.eq_obj2[e])][0]))
        close(r["diag"], diag, "eq diag")


def test_timestep_moves_stiffness(tables):
    """K / B follow the engine's timestep (the max(tc, 2 dt) rule), the rest does not."""
    a, b = tables[("scene_mjx", 0.05)][1], tables[("scene_mjx", 0.02)][1]
    m = tables[("scene_mjx", 0.05)][0]
    n = int(m.npair)
    floor = np.asarray(m.pair_solref, np.float64)[:n, 0] < 2 * 0.05
    assert floor.any()
    assert (a["row"]["K"][:n][floor] != b["row"]["K"][:n][floor]).all()
    for k in ("dmin", "dmax", "iwidth", "mid", "imid", "i1mid", "diag", "margin"):
        assert np.array_equal(a["row"][k], b["row"][k])
    assert a["body"].tobytes() == b["body"].tobytes() and a["dof"].tobytes() == b["dof"].tobytes()
