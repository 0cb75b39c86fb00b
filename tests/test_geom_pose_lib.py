"""Static geom poses as a call input, the parts that need no GPU: the three C
entry points are exported and bound, ``mpcr_model_geom_poses`` reports the
device model's geom order and the model's own block, ``Model.geom_row`` /
``pose_rows`` address it, and a stand-alone program built with the address /
undefined-behaviour sanitizers (tests/c_host/geom_pose_host.cpp; nothing is
loaded into Python) checks the block against ``build_dev_model`` bit for bit,
an edited model's block, the ``StateArgs`` size and that no ``DevModel`` field
moved."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from manipulator_mujoco_amd import _lib, models
from manipulator_mujoco_amd.engine import Model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
WORLD = ("mpcr_rollout_cost_world", "mpcr_plant_set_geom_poses", "mpcr_model_geom_poses")
F = _lib.MPCR_F_DEVICE_PTRS
BUNDLED = tuple(dict.fromkeys(models.PLANNER_SCENES + ("dual_arm", "hande_scene", "scene_mjx")))
MOVE, YAW = (0.05, -0.04, 0.02), 0.3

# "name offset bytes" of the DevModel fields tests/test_ctrl_lib.py pins, with
# act_ctrlrange and the size as that feature left them, and the two arrays the
# plant's poses are written into: this feature moves and adds nothing
BEFORE = """nbody 0 4;nu 68 4;integrator 76 4;timestep 100 4;body_kind 148 128;body_mass 3476 128;jnt_type 3876 128;
jnt_qpos0 6820 128;dof_body 6948 128;mc_c0 8116 128;dof_invweight0 8500 128;qpos_init 8628 128;geom_body 8884 288;
geom_rbound 12916 288;pair_g1 13204 3072;pair_jinfo 25504 12288;pair_diag 71584 3072;eq_type 74656 32;
eqrow_k 75424 96;dof_stiffness 75520 128;dof_actfrc 76544 256;act_ntrn 76800 64;act_moment 77248 128;
act_gain 77376 256;act_bias 77632 256;act_frc 77888 128;impl_D 78016 4096;geom_hulladr 82112 288;hull_vert 82976 8;
hull_head 83016 8;geom_faceadr 83024 288;face_plane 83888 8;cone_face 84224 8;ctrl_qposadr 84232 32;cone 84296 4;
pair_cmu 84308 3072;body_visc 87380 256;ten_body 87636 16;ten_pos 87660 64;ten_invw 87804 8"""


def _qmul(a, b):
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3],
                     a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1],
                     a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]])


def _qrot(q, v):
    return _qmul(_qmul(q, np.concatenate([[0.0], v])), q * [1, -1, -1, -1])[1:]


def move_geom(m, name, dpos=MOVE, yaw=YAW):
    """``m`` with static geom ``name`` moved by dpos and turned by yaw about z,
    both in the world: the new world pose taken back into the frame of the
    geom's (static) body, in fp64."""
    g = list(m.names["geom"]).index(name)
    chain, b = [], int(m.geom_bodyid[g])
    while b > 0:
        assert int(m.body_jntnum[b]) == 0, "a static geom"
        chain.append(b)
        b = int(m.body_parentid[b])
    bp, bq = np.zeros(3), np.array([1.0, 0.0, 0.0, 0.0])  # the body's world frame
    for b in reversed(chain):
        bp = bp + _qrot(bq, np.asarray(m.body_pos[b], dtype=np.float64))
        bq = _qmul(bq, np.asarray(m.body_quat[b], dtype=np.float64))
        bq /= np.sqrt(bq @ bq)
    m.geom_pos = np.array(m.geom_pos, dtype=np.float64)
    m.geom_quat = np.array(m.geom_quat, dtype=np.float64)
    wp = bp + _qrot(bq, m.geom_pos[g]) + np.asarray(dpos, dtype=np.float64)
    wq = _qmul([np.cos(0.5 * yaw), 0.0, 0.0, np.sin(0.5 * yaw)], _qmul(bq, m.geom_quat[g]))
    inv = bq * [1, -1, -1, -1]
    m.geom_pos[g] = _qrot(inv, wp - bp)
    m.geom_quat[g] = _qmul(inv, wq)
    return m


def test_world_symbols_are_exported_and_bound():
    lib = _lib.load()
    for name in WORLD:
        assert name in _lib.EXPORTS
        fn = getattr(lib, name)
        assert fn.argtypes is not None and fn.restype is ctypes.c_int, name
    assert lib.mpcr_abi_version() == 4  # backward-compatible additions: the version stays


def test_null_handles_are_einval_with_a_message():
    lib = _lib.load()
    calls = (lambda: lib.mpcr_rollout_cost_world(None, None, 0, 2, 4, None, None, 0, None, None, 0, 0, None, 0, 0, None,
                                                 None, None, None, 0, None, F, None),
             lambda: lib.mpcr_plant_set_geom_poses(None, None),
             lambda: lib.mpcr_model_geom_poses(None, None, None, None, None))
    for call in calls:
        assert lib.mpcr_model_from_blob(b"\0" * 16, 16, ctypes.byref(ctypes.c_void_p())) == -2
        before = lib.mpcr_last_error()
        assert call() == -1
        msg = lib.mpcr_last_error()
        assert msg and msg != before


@pytest.mark.parametrize("name", BUNDLED)
def test_geom_poses_order_and_static_flags(name):
    m = models.load(name, 0.05)
    block, ids, fixed = Model(m).geom_poses()
    # the device model's geom order: first appearance over the pairs
    order = list(dict.fromkeys(int(g) for p in range(int(m.npair)) for g in (m.pair_geom1[p], m.pair_geom2[p])))
    assert ids.tolist() == order and block.shape == (len(order), 8) and block.dtype == np.float32
    # static: no joint on the geom's body or on any body above it
    for r, g in enumerate(ids):
        b, joints = int(m.geom_bodyid[g]), 0
        while b > 0:
            joints += int(m.body_jntnum[b])
            b = int(m.body_parentid[b])
        assert bool(fixed[r]) == (joints == 0), (name, r, g)
    assert fixed.any() and not fixed.all()
    np.testing.assert_array_equal(block[~fixed], np.tile(np.float32([0, 0, 0, 0, 1, 0, 0, 0]), ((~fixed).sum(), 1)))
    np.testing.assert_array_equal(block[fixed, 3], 0.0)
    np.testing.assert_allclose(np.linalg.norm(block[fixed, 4:].astype(np.float64), axis=1), 1.0, atol=1e-6)


def test_geom_row_and_pose_rows():
    m = models.load("planner_scene", 0.05)
    mod = Model(m)
    block, ids, fixed = mod.geom_poses()
    names = list(m.names["geom"])
    r = mod.geom_row("obstacle_1")
    assert ids[r] == names.index("obstacle_1") and fixed[r] and mod.geom_row(int(ids[r])) == r
    with pytest.raises(KeyError):
        mod.geom_row("no_such_geom")
    # a row written by pose_rows: fp64 normalisation, one rounding, every other row untouched
    q = np.array([2.0, 0.0, 0.0, 0.6])
    out = mod.pose_rows(block, {"obstacle_1": ((0.1, 0.2, 0.3), q)})
    want = np.concatenate([[0.1, 0.2, 0.3, 0.0], q / np.sqrt(q @ q)]).astype(np.float32)
    np.testing.assert_array_equal(out[r], want)
    keep = np.arange(len(block)) != r
    np.testing.assert_array_equal(out[keep], block[keep])
    assert out is not block and block[r].tolist() != out[r].tolist()
    # a schedule: the row of every leading index
    sched = mod.pose_rows(np.broadcast_to(block, (3,) + block.shape), {r_id: ((0, 0, 1), (1, 0, 0, 0)) for r_id in [int(ids[r])]})
    np.testing.assert_array_equal(sched[:, r], np.tile(np.float32([0, 0, 1, 0, 1, 0, 0, 0]), (3, 1)))
    moving = int(ids[np.nonzero(~fixed)[0][0]])
    with pytest.raises(ValueError):
        mod.pose_rows(block, {moving: ((0, 0, 0), (1, 0, 0, 0))})


@pytest.mark.parametrize("name,geom", [("scene_mjx", "table_geom_1"), ("planner_scene", "obstacle_1"),
                                        ("dual_arm", "table_geom_2")])
def test_edited_model_gives_an_edited_row(name, geom):
    m = models.load(name, 0.05)
    mod = Model(m)
    block, ids, fixed = mod.geom_poses()
    mb = move_geom(models.load(name, 0.05), geom)
    block_b, ids_b, fixed_b = Model(mb).geom_poses()
    r = mod.geom_row(geom)
    np.testing.assert_array_equal(ids_b, ids)
    np.testing.assert_array_equal(fixed_b, fixed)
    keep = np.arange(len(block)) != r
    np.testing.assert_array_equal(block_b[keep], block[keep])
    # the move in the world, to fp32 rounding of the composed pose
    np.testing.assert_allclose(block_b[r, :3].astype(np.float64) - block[r, :3], MOVE, atol=2e-7)
    w, x, y, z = block[r, 4:].astype(np.float64)
    c, s = np.cos(0.5 * YAW), np.sin(0.5 * YAW)
    np.testing.assert_allclose(block_b[r, 4:], [c * w - s * z, c * x - s * y, c * y + s * x, c * z + s * w], atol=2e-7)
    # and pose_rows on the own block reproduces the edited model's row to one rounding
    again = mod.pose_rows(block, {geom: (block_b[r, :3], block_b[r, 4:])})
    np.testing.assert_allclose(again, block_b, atol=1e-7, rtol=0)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("geom_pose_host")
    exe = str(d / "geom_pose_host")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(ROOT, "tests", "c_host", "geom_pose_host.cpp")], check=True)
    return d, exe


def test_devmodel_layout_and_stateargs_size(host):
    _, exe = host
    r = subprocess.run([exe, "--layout"], capture_output=True, text=True, check=True)
    now = {w[0]: (int(w[1]), int(w[2])) for w in (ln.split() for ln in r.stdout.splitlines())}
    before = {w[0]: (int(w[1]), int(w[2])) for w in (e.split() for e in BEFORE.replace("\n", "").split(";"))}
    assert now.pop("stateargs")[0] == 56
    size = now.pop("sizeof")[0]
    off, nbytes = now.pop("act_ctrlrange")
    gp, gq = now.pop("geom_pos"), now.pop("geom_quat")
    assert now == before
    # act_ctrlrange is still the last field, and the struct as large as the control input left it
    assert nbytes == 16 * 2 * 4 and off >= max(o + n for o, n in before.values()) and 0 <= size - (off + nbytes) < 16
    assert size == 87952
    # geom_pos | geom_quat adjacent: the plant writes its poses with one copy
    assert gp[1] == gq[1] and gq[0] == gp[0] + gp[1]


def test_block_is_the_device_models_bits_under_sanitizers(host):
    d, exe = host
    paths = []
    for name in BUNDLED:
        path = str(d / f"{name}.mpcrm")
        models.load(name, 0.05).save(path)
        paths.append(path)
    r = subprocess.run([exe] + paths, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    ok = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("OK ")]
    assert [w[1] for w in ok] == paths
    seen = {os.path.basename(w[1])[:-6]: (w[2], w[3]) for w in ok}
    for name in BUNDLED:
        block, _, fixed = Model(models.load(name, 0.05)).geom_poses()
        assert seen[name] == (f"ngeom={len(block)}", f"nstatic={int(fixed.sum())}")
    assert int(seen["planner_scene"][1].split("=")[1]) >= 5  # floor, table, three obstacles at least


def test_the_library_and_the_header_agree(host, tmp_path):
    """The library's entry is the header's function: the block of an edited
    model saved to a blob and read by the stand-alone program passed above;
    here the library's block for the same edit equals Model's for that blob."""
    m = move_geom(models.load("scene_mjx", 0.05), "table_geom_1")
    path = str(tmp_path / "edited.mpcrm")
    m.save(path)
    _, exe = host
    r = subprocess.run([exe, path], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    block, _, fixed = Model(m).geom_poses()
    assert f"ngeom={len(block)} nstatic={int(fixed.sum())}" in r.stdout
