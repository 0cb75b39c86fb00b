"""Target poses as a call input, the parts that need no GPU: the two C entry
points are exported and bound, a stand-alone program built with the address /
undefined-behaviour sanitizers (tests/c_host/target_host.cpp; nothing is
loaded into Python) checks where the arguments live in the launch's parameter
bytes and which kernels they select, ``Engine.target_rows`` lays rows out,
``moving_target`` predicts, and the reference the GPU tests hold the kernels
to -- ``schedule_cost4``, the oracle's cost with the pose terms recomputed from
its end-effector trace against a schedule -- is the oracle's own cost at the
constant target."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle
import parity_util as pu
from manipulator_mujoco_amd import _lib, models
from manipulator_mujoco_amd.engine import Engine
from manipulator_mujoco_amd.mpc_planner import moving_target

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
TARGET = ("mpcr_rollout_cost_target", "mpcr_rollout_cost_scenarios_target")

# the test schedule S12 (H = 12, dt = 0.05): the target translates at VEL and
# yaws at YAW_RATE about the world's z from pu.PT / pu.QT
H12, DT, VEL, YAW_RATE = 12, 0.05, np.array([0.2, -0.1, 0.1]), 1.0
QUAT_SCALE = 1.7  # what the staged quaternions are scaled by (the kernel normalises)


def qmul(a, b):
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3],
                     a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1],
                     a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]])


def s12(vel=VEL, yaw_rate=YAW_RATE, H=H12, dt=DT, pt=pu.PT, qt=pu.QT):
    """(pos (H, 3), rot (H, 4)) of the schedule, fp64, unit quaternions."""
    t = np.arange(H) * dt
    pos = np.asarray(pt, dtype=np.float64) + t[:, None] * np.asarray(vel, dtype=np.float64)
    rot = np.stack([qmul([np.cos(0.5 * yaw_rate * a), 0.0, 0.0, np.sin(0.5 * yaw_rate * a)], qt) for a in t])
    return pos, rot


def s12_rows(**kw):
    """The schedule as staged: float32 target rows with the quaternions scaled."""
    pos, rot = s12(**kw)
    return Engine.target_rows(pos, QUAT_SCALE * rot)


def schedule_cost4(o, pos, rot, W):
    """The oracle's cost4 with the pose terms priced against a schedule: from
    result ``o`` of ``oracle.rollout(..., want_eef=True)``, cost_g = sum_t |p_t
    - pos_t|, cost_r = sum_t 2 acos(clip(|q_t . rot_t| / |q_t|)) over its trace
    (p_t | q_t), cost_c the oracle's own (the target does not touch the
    dynamics), the total w_pos cost_g + w_rot cost_r + w_col cost_c.  ``pos``
    (H, 3) and ``rot`` (H, 4) (unit), or with a leading candidate axis."""
    e = o["eef"]
    pos, rot = np.asarray(pos, dtype=np.float64), np.asarray(rot, dtype=np.float64)
    p, q = e[:, :, :3], e[:, :, 3:]
    g = np.linalg.norm(p - pos, axis=2).sum(axis=1)
    d = np.abs((q * rot).sum(axis=2)) / np.linalg.norm(q, axis=2)
    r = (2.0 * np.arccos(np.clip(d, -1.0, 1.0))).sum(axis=1)
    c = o["cost4"][:, 3]
    return np.stack([W[0] * g + W[1] * r + W[2] * c, g, r, c], axis=1)


def schedule_conditioning(m, td, pos, rot, seed=1):
    """``pu.conditioning``'s record for costs priced against the schedule:
    every probe's cost4 recomputed by ``schedule_cost4`` from that probe's own
    end-effector trace (probe A: noise 1e-7 / 1e-6 with seeds 1000 seed + 1,
    + 1, + 2; probe B: 1e-6, + 3).  No probe_f4: the fp32 restatement prices
    the constant target."""
    def run(noise=0.0, sd=0, slots=False):
        o = oracle.rollout(m, td, pu.Q0, pu.W, pu.PT, pu.QT, want_theta=False, want_slots=slots, want_eef=True,
                           workers=pu.WORKERS, noise=noise, seed=1000 * seed + sd)
        o["cost4"] = schedule_cost4(o, pos, rot, pu.W)
        return o

    o = run(slots=m.nslot > 0)
    a = o["cost4"]
    unstable = np.zeros(len(a), bool)

    def probe(eps, sd):
        r = run(eps, sd)
        unstable[:] |= r["nneg"] != o["nneg"]
        return pu._rel(a, r["cost4"])

    s4 = np.maximum.reduce([probe(1e-7, 1), probe(1e-6, 1), probe(1e-6, 2)])
    o["sens4"] = s4
    o["probe_b4"] = probe(1e-6, 3)
    o["probe_b"] = o["probe_b4"][:, 0]
    o["nneg_unstable"] = unstable
    return o, s4[:, 0]


def test_target_symbols_are_exported_and_bound():
    lib = _lib.load()
    for name in TARGET:
        assert name in _lib.EXPORTS
        fn = getattr(lib, name)
        assert fn.argtypes is not None and fn.restype is ctypes.c_int, name
    # the arguments of the world / scenarios entries plus a pointer and two strides
    assert len(lib.mpcr_rollout_cost_target.argtypes) == len(lib.mpcr_rollout_cost_world.argtypes) + 3
    assert len(lib.mpcr_rollout_cost_scenarios_target.argtypes) == len(lib.mpcr_rollout_cost_scenarios.argtypes) + 3
    assert lib.mpcr_abi_version() == 4  # backward-compatible additions: the version stays


def test_null_handles_are_einval_with_a_message():
    lib = _lib.load()
    F = _lib.MPCR_F_DEVICE_PTRS
    calls = (lambda: lib.mpcr_rollout_cost_target(None, None, 0, 2, 4, None, None, 0, None, None, 0, 0, None, 0, 0,
                                                  None, 0, 0, None, None, None, None, 0, None, F, None),
             lambda: lib.mpcr_rollout_cost_scenarios_target(None, None, 0, 2, 2, 2, 4, None, None, 0, None, None, 0, 0,
                                                            None, 0, 0, None, 0, 0, None, None, None, None, None, 0,
                                                            None, F, None))
    for call in calls:
        assert lib.mpcr_model_from_blob(b"\0" * 16, 16, ctypes.byref(ctypes.c_void_p())) == -2
        before = lib.mpcr_last_error()
        assert call() == -1
        msg = lib.mpcr_last_error()
        assert msg and msg != before


def test_argument_bytes_and_kernel_choice_under_sanitizers(tmp_path):
    exe = str(tmp_path / "target_host")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(ROOT, "tests", "c_host", "target_host.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "OK target_host"


def test_target_rows_layout():
    pos, rot = np.array([0.1, -0.2, 0.3]), np.array([0.0, 3.0, 0.0, 4.0])
    row = Engine.target_rows(pos, rot)
    assert row.shape == (8,) and row.dtype == np.float32
    np.testing.assert_array_equal(row, np.float32([0.1, -0.2, 0.3, 0.0, 0.0, 3.0, 0.0, 4.0]))  # not normalised
    # floats 12..19 of a parameter block
    np.testing.assert_array_equal(Engine.params(pu.Q0, pu.W, pos, rot)[12:20], row)
    # a schedule, and broadcasting of one orientation over it
    P = np.arange(15, dtype=np.float64).reshape(5, 3)
    rows = Engine.target_rows(P, rot)
    assert rows.shape == (5, 8)
    np.testing.assert_array_equal(rows[:, :3], P.astype(np.float32))
    np.testing.assert_array_equal(rows[:, 3], 0.0)
    np.testing.assert_array_equal(rows[:, 4:], np.tile(np.float32(rot), (5, 1)))
    assert Engine.target_rows(np.zeros((2, 1, 3)), np.ones((4, 4))).shape == (2, 4, 8)
    for bad in ((np.zeros(4), rot), (pos, np.zeros(3))):
        with pytest.raises(ValueError, match="target_rows"):
            Engine.target_rows(*bad)


def test_moving_target_two_ticks():
    v, H, dt = (0.05, -0.02, 0.1), 4, 0.05
    mt = moving_target(v, H, dt)
    p0, q0 = np.array([0.3, 0.2, 0.5]), np.array([0.0, 1.0, 0.0, 0.0])
    for tick in (0, 1):
        now, (pos, rot) = mt(tick, p0, q0)
        np.testing.assert_allclose(now, p0 + tick * dt * np.asarray(v), rtol=0, atol=1e-15)
        assert pos.shape == (H, 3) and rot.shape == (H, 4)
        for k in range(H):
            np.testing.assert_allclose(pos[k], p0 + (tick + k) * dt * np.asarray(v), rtol=0, atol=1e-15)
        np.testing.assert_array_equal(rot, np.tile(q0, (H, 1)))
        np.testing.assert_array_equal(pos[0], now)  # step 0 is the tick's own time
    # tick 1's horizon is tick 0's, one step on
    np.testing.assert_allclose(mt(1, p0, q0)[1][0][:-1], mt(0, p0, q0)[1][0][1:], rtol=0, atol=1e-15)
    np.testing.assert_array_equal(moving_target((0, 0, 0), H, dt)(7, p0, q0)[0], p0)


def test_s12_is_the_issues_schedule():
    pos, rot = s12()
    np.testing.assert_array_equal(pos[0], pu.PT)
    np.testing.assert_allclose(pos[11], pu.PT + 0.55 * VEL, atol=1e-15)
    np.testing.assert_allclose(np.linalg.norm(rot, axis=1), 1.0, atol=1e-15)
    np.testing.assert_allclose(rot[0], pu.QT, atol=0)
    # qz(a) (x) (0, 1, 0, 0) = (0, cos a/2, sin a/2, 0)
    np.testing.assert_allclose(rot[4], [0.0, np.cos(0.1), np.sin(0.1), 0.0], atol=1e-15)
    rows = s12_rows()
    np.testing.assert_allclose(np.linalg.norm(rows[:, 4:].astype(np.float64), axis=1), QUAT_SCALE, rtol=1e-6)


@pytest.mark.parametrize("name,n", [("scene_mjx", 64), ("dual_arm", 32)])
def test_schedule_cost4_at_the_constant_target_is_the_oracles(name, n):
    m = models.load(name, 0.05)
    td = np.random.default_rng(1).uniform(-0.6, 0.6, (n, 6 * H12))
    o = oracle.rollout(m, td, pu.Q0, pu.W, pu.PT, pu.QT, want_theta=False, want_eef=True, workers=pu.WORKERS)
    own = o["cost4"].copy()
    got = schedule_cost4(o, np.tile(pu.PT, (H12, 1)), np.tile(pu.QT, (H12, 1)), pu.W)
    rel = np.abs(got - own) / np.maximum(np.abs(own), 1e-12)
    print(f"{name} {n}x{H12}: schedule_cost4 against the oracle's cost4 at the constant target, max rel {rel.max():.1e}")
    assert rel.max() < 1e-12  # (7e-15 measured)
    np.testing.assert_array_equal(got[:, 3], own[:, 3])
    # and S12 moves every total (what the GPU parity test requires of the kernels)
    moved = schedule_cost4(o, *s12(), pu.W)
    rel = np.abs(moved[:, 0] - own[:, 0]) / np.abs(own[:, 0])
    print(f"{name}: S12 against the constant target, totals move by {rel.min():.2e} .. {rel.max():.2e}")
    assert rel.min() > (5e-3 if name == "scene_mjx" else 2e-2)
