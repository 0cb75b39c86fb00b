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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NB, NV, NP, NJ, NEQ = 32, 32, 768, 32, 8
MINVAL, MINIMP, MAXIMP = np.float32(1e-15), np.float32(0.0001), np.float32(0.9999)
ANCHOR0, POW2, POW1, LIMITED, CONDIM1 = 1, 1, 2, 4, 8
FREE, BALL, SLIDE, HINGE = 0, 1, 2, 3
BK_FREE, BK_HINGE, BK_SLIDE, BK_WELD = 1, 2, 3, 4
f4, i4 = np.float32, np.int32

BODY = np.dtype([("kind", i4), ("anc", i4), ("qposadr", i4), ("qpos0", f4), ("bquat", f4, 4), ("bpos", f4, 3),
                 ("pad0", f4), ("axis", f4, 3), ("pad1", f4), ("ipos", f4, 3), ("pad2", f4), ("jpos", f4, 3),
                 ("pad3", f4), ("R", f4, (3, 4))])
DOF = np.dtype([("body", i4), ("kind", i4), ("tree", i4), ("sub", i4), ("axis", f4, 3), ("pad0", f4), ("jpos", f4, 3),
                ("pad1", f4)])
ROW = np.dtype([("dmin", f4), ("dmax", f4), ("iwidth", f4), ("mid", f4), ("imid", f4), ("i1mid", f4), ("K", f4),
                ("B", f4), ("margin", f4), ("diag", f4), ("flags", i4), ("power", f4), ("range", f4, 2),
                ("qposadr", i4), ("dofadr", i4)])
TABLE = np.dtype([("flags", i4), ("nbody", i4), ("pad", i4, 2), ("body", BODY, NB), ("dof", DOF, NV),
                  ("row", ROW, NP + NJ + NEQ)])

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


def close(got, ref, what):
    """got (fp32) within 1 fp32 ulp of ref (float64 formula)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    fin = np.isfinite(ref)
    assert np.array_equal(got[~fin], ref[~fin]), what
    with np.errstate(over="ignore"):
        ulp = np.spacing(np.abs(ref[fin]).astype(np.float32)).astype(np.float64)
    ulp = np.where(np.isfinite(ulp), ulp, np.inf)
    err = np.abs(got[fin] - ref[fin])
    assert (err <= ulp).all(), (what, float((err / ulp).max()))


def qmul(a, b):
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3],
                     a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1],
                     a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]])


def q2m(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def frames(m):
    """Moving-body indices, static world poses, tree indices: the chained lookups."""
    nb = int(m.nbody)
    moving = [b for b in range(1, nb) if m.body_weldid[b] != 0]
    dmap = {b: i for i, b in enumerate(moving)}
    wpos, wquat = np.zeros((nb, 3)), np.zeros((nb, 4))
    wquat[0, 0] = 1
    for b in range(1, nb):
        if b in dmap:
            continue
        p = int(m.body_parentid[b])
        wpos[b] = wpos[p] + q2m(wquat[p]) @ np.asarray(m.body_pos[b], np.float64)
        q = qmul(wquat[p], np.asarray(m.body_quat[b], np.float64))
        wquat[b] = q / np.sqrt((q * q).sum())
    roots = []
    tree = {}
    for b in moving:
        r = int(m.body_rootid[b])
        if r not in roots:
            roots.append(r)
        tree[b] = roots.index(r)
    return moving, dmap, wpos, wquat, tree


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
