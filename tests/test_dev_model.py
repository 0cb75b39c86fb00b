"""The device-model compiler (csrc/dev_model.h with csrc/model_frames.h) on the
CPU: a stand-alone program built with the address / undefined-behaviour
sanitizers compiles every bundled model's packed blob into its DevModel and
tables (nothing is launched, no GPU is opened, nothing is loaded into Python).
Resolved indices are compared exactly with the chained lookups, derived floats
with the same formula in numpy float64 (<= 1 fp32 ulp, model_ref.close), the
values the step table holds too with the step table's dump of the same blob,
and the tables by their properties."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from manipulator_mujoco_amd import models
from model_ref import (BK_FREE, BK_HINGE, BK_SLIDE, BK_WELD, CONDIM1, FREE, HINGE, LIMITED, NJ, NP, SLIDE, TABLE,
                       close, frames, q2m, qmul)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
NTREE, MCW, NVW, MC_ROWS = 4, 16, 32, 24  # DX_NTREE; SmemW::MCW, NVW, MPCR_W_MC_ROWS
LUT_R, CONE_R, CONE_COS = 128, 8, 0.94
EQ_CONNECT, EQ_JOINT, COL_CONVEX = 0, 2, 9

NAMES = tuple(dict.fromkeys(models.PLANNER_SCENES + ("dual_arm",)))
CASES = [(n, 0.05) for n in NAMES] + [("scene_mjx", 0.02), ("scene_mjx_anchored", 0.05)]
TABLES = (("hull_vert", 16), ("hull_info", 8), ("hull_adjv", 16), ("hull_head", 16), ("hull_lut", 16),
          ("face_plane", 16), ("face_vinfo", 8), ("vert_finfo", 8), ("cone_cell", 8), ("cone_face", 4))


def load(name, dt):
    if name != "scene_mjx_anchored":
        return models.load(name, dt)
    m = models.load("scene_mjx", dt)  # tests/test_gpu_step_table.py::test_joint_anchors_match_oracle
    m.jnt_pos = np.array(m.jnt_pos, dtype=np.float64)
    m.jnt_pos[1] = (0.01, -0.02, 0.015)
    m.jnt_pos[3] = (-0.015, 0.01, 0.02)
    return m


def error_code(name):
    with open(os.path.join(ROOT, "include", "mpcr.h")) as f:
        for ln in f:
            w = ln.replace(",", " ").replace("=", " ").split()
            if name in w:
                return int(w[w.index(name) + 1])
    raise KeyError(name)


def refusals(d):
    """(what, blob path, expected code): models the compiler refuses."""
    out = []

    def blob(what, s):
        path = str(d / f"refuse_{what}.mpcrm")
        with open(path, "wb") as f:
            f.write(bytes(s))
        out.append((what, path, error_code("MPCR_EMODEL")))

    s = models.load("scene_mjx", 0.05).to_struct()  # 33 moving bodies: welded children of the last body
    last = s.nbody - 1
    assert s.body_weldid[last] != 0
    for b in range(s.nbody, 34 + sum(1 for k in range(1, s.nbody) if s.body_weldid[k] == 0)):
        s.body_parentid[b], s.body_rootid[b], s.body_weldid[b] = last, s.body_rootid[last], s.body_weldid[last]
        s.body_jntnum[b], s.body_jntadr[b] = 0, -1
        s.body_quat[b][0] = s.body_iquat[b][0] = 1.0
        s.nbody = b + 1
    blob("33_moving_bodies", s)
    s = models.load("scene_mjx", 0.05).to_struct()
    s.jnt_type[1] = 1  # MPCR_JNT_BALL
    blob("ball_joint", s)
    s = models.load("scene_mjx", 0.05).to_struct()
    s.pair_condim[0] = 4
    blob("condim4", s)
    s = models.load("dual_arm", 0.05).to_struct()
    assert s.pair_func[s.npair - 1] >= COL_CONVEX and s.pair_func[0] < COL_CONVEX
    s.pair_func[s.npair - 1] = s.pair_func[0]
    blob("convex_not_last", s)
    return out


class Dev:
    def __init__(self, path, layout):
        raw = np.fromfile(path, dtype=np.uint8)
        size, self.wide = (int(x) for x in raw[:8].view(np.int32))
        self.raw = raw[8:8 + size]
        self.layout = layout
        off = 8 + size
        for name, item in TABLES:
            n = int(raw[off:off + 8].view(np.int64)[0])
            setattr(self, name, raw[off + 8:off + 8 + n * item].view(np.int32).reshape(n, item // 4))
            off += 8 + n * item
        assert off == raw.size

    def __getitem__(self, name):
        off, size, kind = self.layout[name]
        v = self.raw[off:off + size].view({"i": np.int32, "u": np.uint32, "f": np.float32}[kind])
        return v[0] if size == 4 else v


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    d = tmp_path_factory.mktemp("dev_model")
    exe = str(d / "dev_model_host")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(ROOT, "tests", "c_host", "dev_model_host.cpp")], check=True)
    cxx = shutil.which("g++") or shutil.which("c++")
    step_exe = str(d / "step_table_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-o", step_exe, os.path.join(ROOT, "tests", "c_host", "step_table_host.cpp")],
                   check=True)
    r = subprocess.run([exe, "--layout"], capture_output=True, text=True, check=True)
    layout = {w[0]: (int(w[1]), int(w[2]), w[3]) for w in (ln.split() for ln in r.stdout.splitlines())}
    ms = {}
    for name, dt in CASES:
        m = load(name, dt)
        path = str(d / f"{name}_{dt}.mpcrm")
        m.save(path)
        ms[(name, dt)] = (m, path)
    ref = refusals(d)
    r = subprocess.run([exe] + [p for _, p in ms.values()] + [p for _, p, _ in ref], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    subprocess.run([step_exe] + [p for _, p in ms.values()], check=True, capture_output=True)
    out = {}
    for key, (m, path) in ms.items():
        step = np.fromfile(path + ".step", dtype=np.uint8)[16:].view(TABLE)[0]
        out[key] = (m, Dev(path + ".dev", layout), step)
    return dict(models=out, stdout=r.stdout, stderr=r.stderr, refusals=ref)


IDS = [f"{n}-{dt}" for n, dt in CASES]
f8 = lambda x: np.asarray(x, np.float64)


def test_sanitizers_silent(built):
    assert built["stderr"] == ""


def test_refusals(built):
    lines = [ln.split(" ", 3) for ln in built["stdout"].splitlines() if ln.startswith("REFUSED ")]
    got = {w[1]: (int(w[2]), w[3].strip() if len(w) > 3 else "") for w in lines}
    assert len(got) == len(built["refusals"]) == 4
    for what, path, code in built["refusals"]:
        assert path in got, what
        assert got[path][0] == code and got[path][1], (what, got[path])
        assert not os.path.exists(path + ".dev")


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_bodies_dofs(built, case):
    m, d, _ = built["models"][case]
    moving, dmap, wpos, wquat, tree = frames(m)
    assert d["nbody"] == len(moving) and d["ntree"] == len(set(tree.values())) and d["nv"] == m.nv
    depth = {}
    for i, b in enumerate(moving):
        p = int(m.body_parentid[b])
        j = int(m.body_jntadr[b]) if m.body_jntnum[b] else -1
        kind = BK_WELD if j < 0 else {FREE: BK_FREE, HINGE: BK_HINGE, SLIDE: BK_SLIDE}[int(m.jnt_type[j])]
        if p in dmap:
            bp, bq, anc = f8(m.body_pos[b]), f8(m.body_quat[b]), dmap[p]
        else:
            bp, bq, anc = wpos[p] + q2m(wquat[p]) @ f8(m.body_pos[b]), qmul(wquat[p], f8(m.body_quat[b])), -1
        anc = -1 if kind == BK_FREE else anc
        depth[i] = 1 if anc < 0 else depth[anc] + 1
        assert (d["body_kind"][i], d["body_anc"][i], d["body_jnt"][i], d["body_tree"][i]) == (kind, anc, j, tree[b])
        close(d["body_bpos"].reshape(-1, 4)[i, :3], bp, "bpos")
        close(d["body_bquat"].reshape(-1, 4)[i], bq, "bquat")
        close(d["body_ipos"].reshape(-1, 4)[i, :3], m.body_ipos[b], "ipos")
        close(d["body_mass"][i], m.body_mass[b], "mass")
        assert d["body_dofmask"][i] == np.uint32(m.body_dofmask[b])
        sub = 0
        for c in moving:  # the moving bodies whose parent chain passes through b
            a = c
            while a > 0 and a != b:
                a = int(m.body_parentid[a])
            sub |= (1 << dmap[c]) if a == b else 0
        assert d["body_submask"][i] == sub
    assert (1 << int(d["jump_rounds"])) >= max(depth.values()) > (1 << int(d["jump_rounds"])) // 2
    for i in range(int(m.nv)):
        j, b = int(m.dof_jntid[i]), int(m.dof_bodyid[i])
        sub, jt = i - int(m.jnt_dofadr[j]), int(m.jnt_type[j])
        assert d["dof_body"][i] == dmap[b] and d["dof_jnt"][i] == j
        assert d["dof_kind"][i] == (0 if jt == HINGE else 1 if jt == SLIDE else (2 if sub < 3 else 3))
        assert d["dof_sub"][i] == (sub if sub < 3 else sub - 3)
        cm, a = 0, i
        while a >= 0:
            cm |= 1 << a
            a = int(m.dof_parentid[a])
        assert d["dof_chainmask"][i] == cm
        assert d["dof_submask"][i] == d["body_submask"][dmap[b]]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_compact_mass_matrix(built, case):
    m, d, _ = built["models"][case]
    nv = int(m.nv)
    dof_tree = [int(d["body_tree"][d["dof_body"][i]]) for i in range(nv)]
    lanes = d["blane_dof"]
    assert sorted(int(x) for x in lanes if x >= 0) == list(range(nv))  # a bijection onto the dofs
    for t in range(NTREE):  # tree t's dofs, ascending, packed from lane 16 t
        mine = [i for i in range(nv) if dof_tree[i] == t]
        assert list(lanes[16 * t:16 * t + 16]) == mine + [-1] * (16 - len(mine))
    per_tree = max(dof_tree.count(t) for t in range(NTREE))
    assert d["blk_n"] == (8 if per_tree <= 8 else 16)
    # the compact image keeps every row or none; row i's window of MCW columns starts at a multiple of 4, stays
    # inside the NVW columns and covers its tree's dofs
    fits = nv <= MC_ROWS
    for i in range(nv):
        mine = [k for k in range(nv) if dof_tree[k] == dof_tree[i]]
        c0 = int(d["mc_c0"][i])
        assert mine == list(range(mine[0], mine[-1] + 1))  # contiguous in every bundled model
        assert c0 % 4 == 0 and 0 <= c0 <= NVW - MCW and c0 == min(mine[0] & ~3, NVW - MCW)
        fits &= c0 <= mine[0] and mine[-1] < c0 + MCW
    assert d["mc_n"] == (nv if fits else 0)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_geoms_pairs(built, case):
    m, d, _ = built["models"][case]
    moving, dmap, wpos, wquat, tree = frames(m)
    npair = int(m.npair)
    gmap = {}
    for p in range(npair):  # the remap: first use over the pairs
        for g in (int(m.pair_geom1[p]), int(m.pair_geom2[p])):
            gmap.setdefault(g, len(gmap))
    assert d["ngeom"] == len(gmap) and d["npair"] == npair
    gpos, gquat = d["geom_pos"].reshape(-1, 4), d["geom_quat"].reshape(-1, 4)
    for g, i in gmap.items():
        b = int(m.geom_bodyid[g])
        assert d["geom_type"][i] == m.geom_type[g]
        if b in dmap:
            assert d["geom_body"][i] == dmap[b]
            close(gpos[i, :3], m.geom_pos[g], "geom pos")
            close(gquat[i], m.geom_quat[g], "geom quat")
        else:  # static: the world pose
            assert d["geom_body"][i] == -1
            close(gpos[i, :3], wpos[b] + q2m(wquat[b]) @ f8(m.geom_pos[g]), "static geom pos")
            close(gquat[i], qmul(wquat[b], f8(m.geom_quat[g])), "static geom quat")
    impratio = float(m.impratio) if m.impratio > 0 else 1.0
    jinfo = d["pair_jinfo"].reshape(-1, 4)
    for p in range(npair):
        g1, g2 = int(m.pair_geom1[p]), int(m.pair_geom2[p])
        assert (d["pair_g1"][p], d["pair_g2"][p]) == (gmap[g1], gmap[g2])
        close(d["pair_margin"][p], np.float64(m.pair_margin[p]) - np.float64(m.pair_gap[p]), "pair margin")
        close(d["pair_diag"][p], np.float64(m.body_invweight0[int(m.geom_bodyid[g1])][0]) +
              np.float64(m.body_invweight0[int(m.geom_bodyid[g2])][0]), "pair diag")
        close(d["pair_cmu"][p], np.float64(m.pair_friction[p]) / np.sqrt(impratio), "pair cmu")
        b = [int(m.geom_bodyid[g]) for g in (g1, g2)]
        ref = [int(np.uint32(m.body_dofmask[x]).view(np.int32)) if x in dmap else 0 for x in b] + \
              [tree[x] if x in dmap else 0 for x in b]
        assert list(jinfo[p]) == ref


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_equalities(built, case):
    m, d, _ = built["models"][case]
    moving, dmap, wpos, wquat, tree = frames(m)
    rows = []
    data = d["eq_data"].reshape(-1, 8)
    for e in range(int(m.neq)):
        o1, o2 = int(m.eq_obj1[e]), int(m.eq_obj2[e])
        assert d["eq_type"][e] == m.eq_type[e]
        if int(m.eq_type[e]) == EQ_JOINT:
            assert (d["eq_j1"][e], d["eq_j2"][e]) == (o1, o2)
            close(data[e, :5], f8(m.eq_data[e])[:5], "polycoef")
            diag = np.float64(m.dof_invweight0[int(m.jnt_dofadr[o1])])
            if o2 >= 0:
                diag += np.float64(m.dof_invweight0[int(m.jnt_dofadr[o2])])
            rows += [(e, 0)]
        else:
            assert int(m.eq_type[e]) == EQ_CONNECT
            for side, b in enumerate((o1, o2)):
                a = f8(m.eq_data[e])[3 * side:3 * side + 3]
                db = dmap.get(b, -1) if b > 0 else -1
                assert d["eq_b2" if side else "eq_b1"][e] == db
                close(data[e, 4 * side:4 * side + 3], a if db >= 0 else wpos[b] + q2m(wquat[b]) @ a, "anchor")
            diag = np.float64(m.body_invweight0[o1][0]) + np.float64(m.body_invweight0[o2][0])
            rows += [(e, 1), (e, 2), (e, 3)]
        close(d["eq_diag"][e], diag, "eq diag")
    assert d["neqrow"] == len(rows)
    assert list(zip(d["eqrow_eq"][:len(rows)], d["eqrow_k"][:len(rows)])) == rows


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_step_table_agrees(built, case):
    """The values the step table and the device model both hold are the same bits."""
    m, d, t = built["models"][case]
    same = lambda a, b: np.asarray(a, np.float32).tobytes() == np.asarray(b, np.float32).tobytes()
    assert t["nbody"] == d["nbody"]
    jpos, jaxis = d["jnt_pos"].reshape(-1, 4), d["jnt_axis"].reshape(-1, 4)
    for i in range(int(d["nbody"])):
        r, j = t["body"][i], int(d["body_jnt"][i])
        assert (r["kind"], r["anc"]) == (d["body_kind"][i], d["body_anc"][i])
        assert r["qposadr"] == (d["jnt_qposadr"][j] if j >= 0 else -1)
        assert same(r["bquat"], d["body_bquat"].reshape(-1, 4)[i]) and same(r["bpos"], d["body_bpos"].reshape(-1, 4)[i, :3])
        assert same(r["ipos"], d["body_ipos"].reshape(-1, 4)[i, :3])
        assert j < 0 or same(r["qpos0"], d["jnt_qpos0"][j])
        if r["kind"] == BK_HINGE:
            assert same(r["axis"], jaxis[j, :3]) and same(r["jpos"], jpos[j, :3])
    for i in range(int(d["nv"])):
        r, j = t["dof"][i], int(d["dof_jnt"][i])
        assert (r["body"], r["kind"], r["sub"]) == (d["dof_body"][i], d["dof_kind"][i], d["dof_sub"][i])
        assert r["tree"] == (d["body_tree"][r["body"]] if r["body"] >= 0 else -1)
        assert same(r["axis"], jaxis[j, :3]) and same(r["jpos"], jpos[j, :3])
    for p in range(int(d["npair"])):
        r = t["row"][p]
        assert same(r["margin"], d["pair_margin"][p]) and bool(r["flags"] & CONDIM1) == (d["pair_condim"][p] == 1)
    for j in range(int(d["njnt"])):
        r = t["row"][NP + j]
        lim = bool(d["jnt_limited"][j]) and int(d["jnt_type"][j]) in (SLIDE, HINGE)
        assert (r["qposadr"], r["dofadr"]) == (d["jnt_qposadr"][j], d["jnt_dofadr"][j])
        assert bool(r["flags"] & LIMITED) == lim and same(r["margin"], d["jnt_margin"][j])
        assert same(r["diag"], d["dof_invweight0"][d["jnt_dofadr"][j]])
        assert same(r["range"], d["jnt_range"].reshape(-1, 2)[j])
    for e in range(int(d["neq"])):
        assert same(t["row"][NP + NJ + e]["diag"], d["eq_diag"][e])


def test_wide_class(built):
    assert {k[0]: v[1].wide for k, v in built["models"].items() if k[1] == 0.05} == {
        "planner_scene": 0, "ur5e_hande_mjx": 0, "scene_mjx": 0, "dual_arm": 1, "scene_mjx_anchored": 0}


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_hull_tables(built, case):
    m, d, _ = built["models"][case]
    nv = int(m.nhullv)
    assert len(d.hull_vert) == len(d.hull_info) == nv and len(d.hull_head) == 8 * nv and len(d.hull_adjv) == int(m.nhulla)
    if nv == 0:
        assert len(d.hull_lut) == 0 and (d["geom_lutadr"][:int(d["ngeom"])] == -1).all()
        return
    adr, num = d.hull_info[:, 0], d.hull_info[:, 1]
    assert np.array_equal(adr, np.asarray(m.hull_adjadr[:nv])) and np.array_equal(num, np.asarray(m.hull_adjnum[:nv]))
    assert np.array_equal(d.hull_vert[:, :3].view(np.float32), np.asarray(m.hull_vert[:nv], np.float32))
    assert np.array_equal(d.hull_vert[:, 3], num)
    # neighbour records: xyz | index | degree << 16 of the vertex the adjacency names
    u = np.asarray(m.hull_adj[:int(m.nhulla)])
    assert np.array_equal(d.hull_adjv[:, :3], d.hull_vert[u, :3]) and np.array_equal(d.hull_adjv[:, 3], u | (num[u] << 16))
    # every head record is the neighbour record it names; the pads are NaN with index -1
    head = d.hull_head.reshape(nv, 8, 4)
    k = np.arange(8)[None, :]
    live = k < num[:, None]
    assert np.array_equal(head[live], d.hull_adjv[(adr[:, None] + k)[live]])
    assert np.isnan(head[~live][:, :3].view(np.float32)).all() and (head[~live][:, 3] == -1).all()
    # every start cell's vertex lies in its hull, and carries that vertex's record
    ncell = 6 * LUT_R * LUT_R
    seen = 0
    for i in range(int(d["ngeom"])):
        la = int(d["geom_lutadr"][i])
        if la < 0:
            continue
        cells = d.hull_lut[la:la + ncell]
        v = cells[:, 3] & 0x7fff
        a, n = int(d["geom_hulladr"][i]), int(d["geom_hullnum"][i])
        assert len(cells) == ncell and ((v >= a) & (v < a + n)).all()
        assert np.array_equal(cells[:, :3], d.hull_vert[v, :3]) and np.array_equal(cells[:, 3] >> 16, num[v])
        seen += 1
    assert seen > 0


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_cone_table(built, case):
    m, d, _ = built["models"][case]
    if int(m.nface) == 0:
        assert len(d.cone_cell) == 0 and len(d.face_plane) == 0
        return
    nf = int(m.nface)
    assert np.array_equal(d.face_plane.view(np.float32), np.asarray(m.face_plane[:nf], np.float32))
    assert np.array_equal(d.face_vinfo, np.stack([m.face_vadr[:nf], m.face_vnum[:nf]], 1))
    assert np.array_equal(d.vert_finfo, np.stack([m.vert_faceadr[:int(m.nhullv)], m.vert_facenum[:int(m.nhullv)]], 1))
    normals = f8(m.face_plane[:nf])[:, :3]
    normals /= np.linalg.norm(normals, axis=1, keepdims=True)
    rng = np.random.default_rng(7)
    seen = 0
    for i in range(int(d["ngeom"])):
        ca = int(d["geom_coneadr"][i])
        fa, fnum = int(d["geom_faceadr"][i]), int(d["geom_facenum"][i])
        if fa < 0 or fnum <= 0:
            assert ca == -1
            continue
        assert ca >= 0 and ca % (6 * CONE_R * CONE_R) == 0
        dirs = rng.normal(size=(200, 3))
        dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
        ax = np.argmax(np.abs(dirs), axis=1)
        rows = np.arange(len(dirs))
        la = dirs[rows, ax]
        iu = np.clip(np.floor((dirs[rows, (ax + 1) % 3] / np.abs(la) + 1) * 0.5 * CONE_R).astype(int), 0, CONE_R - 1)
        iv = np.clip(np.floor((dirs[rows, (ax + 2) % 3] / np.abs(la) + 1) * 0.5 * CONE_R).astype(int), 0, CONE_R - 1)
        cell = (2 * ax + (la < 0)) * CONE_R * CONE_R + iu * CONE_R + iv
        for k in range(len(dirs)):
            start, cnt = d.cone_cell[ca + cell[k]]
            lst = d.cone_face[start:start + cnt, 0]
            assert (np.diff(lst) > 0).all() and (lst >= fa).all() and (lst < fa + fnum).all()
            want = fa + np.nonzero(normals[fa:fa + fnum] @ dirs[k] >= CONE_COS)[0]
            assert np.isin(want, lst).all()
        seen += 1
    assert seen > 0
