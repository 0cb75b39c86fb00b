"""The load records (csrc/step_table.h StepRecords, quad 3 of the pair rows)
on the GPU: the single-arm kernels that read them against the fp64 oracle at
the parity bar of tests/parity_util.py, on every bundled single-arm scene, on
two models edited here (an equality without a second joint, a frictionless
pair), pressed into the table and a joint limit (rows past the 40 the
one-wave image keeps in LDS), and through the multi-problem and from-state
entry points."""
import numpy as np
import pytest

import oracle
import parity_util as pu
from manipulator_mujoco_amd import _lib, basis, models
from manipulator_mujoco_amd.engine import MPCR_LAYOUT_THETADOT, Engine
from test_gpu_step_table import run, sine_thetadot
from test_step_records import edited

pytestmark = pytest.mark.gpu

Q0, W, PT, QT = pu.Q0, pu.W, pu.PT, pu.QT
N, H, DT = 64, 20, 0.05


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def max_rows(status):
    return (status >> 2) & 0xFF


def row_sum(status):
    return status >> 11


def test_hande_scene_plant_matches_oracle_step(torch_cuda):
    """hande_scene has no planner-controlled arm (nctrl = 0: neither the
    oracle's rollout nor pu.check apply to it), so it runs as a plant: 10
    steps from qpos0, re-synced to the oracle every step, at the bars of
    tests/test_gpu_plant.py::test_plant_hande_scene_matches_oracle_step.  It
    runs the dual-arm class of kernels, which read no records: what it checks
    of this change is only that such an engine's allocation and upload, now
    sized for the records too, leave that class as it was."""
    from manipulator_mujoco_amd.engine import Plant
    m = models.load("hande_scene")
    plant = Plant(m)
    qpos, qvel, ws = m.qpos0[:m.nq].copy(), np.zeros(m.nv), np.zeros(m.nv)
    for _ in range(10):
        plant.set_state(qpos=qpos, qvel=qvel, qacc_warmstart=ws)
        o = oracle.step(m, qpos, qvel, ws)
        plant.step()
        scale = max(1.0, np.abs(o["qacc"]).max())
        np.testing.assert_allclose(plant.qacc, o["qacc"], atol=2e-3 * scale, rtol=2e-3)
        qpos, qvel, ws = o["qpos"], o["qvel"], o["qacc_warmstart"]
        np.testing.assert_allclose(plant.qpos, qpos, atol=1e-5)
        np.testing.assert_allclose(plant.qvel, qvel, atol=1e-4, rtol=1e-3)


@pytest.mark.parametrize("name", ["scene_mjx", "ur5e_hande_mjx", "planner_scene"])
def test_parity(torch_cuda, name):
    """64 x 20 smooth drives against the oracle (pu.check)."""
    m = models.load(name, DT)
    _, _, Pd, _ = basis.planner_basis(H, DT)
    td = sine_thetadot(N, H, DT, 53)
    c4, _, st = run(Engine(m, H, N, Pd), td)
    o, sens = pu.conditioning(m, td.astype(np.float64))
    stats = pu.check(m, c4[:, 0], o, sens, f"step records {name}")
    print(f"{name}: {stats}, most rows {max_rows(st).max()}")


@pytest.mark.parametrize("which", ["eq_one_joint", "condim1"])
def test_edited_models_match_oracle(torch_cuda, which):
    """An equality without a second joint (the record's qadr2 = -1) and a
    frictionless pair (one row per contact), as
    tests/test_gpu_step_table.py::test_joint_anchors_match_oracle."""
    m = edited(which)
    _, _, Pd, _ = basis.planner_basis(H, DT)
    td = sine_thetadot(N, H, DT, 29)
    e = Engine(m, H, N, Pd)
    g = e.trace(td, MPCR_LAYOUT_THETADOT, Q0, W, PT, QT)
    o = oracle.rollout(m, td.astype(np.float64), Q0, W, PT, QT, want_slots=True, want_eef=True)
    # the edit is live in these rollouts (CPU, the oracle on the unedited model) ...
    ob = oracle.rollout(models.load("scene_mjx", DT), td.astype(np.float64), Q0, W, PT, QT)
    if which == "eq_one_joint":
        # ... the follower finger is free of the driver: the fingers' state moves
        # the arm by far more than the 1e-3 the kernel is held to below
        assert (ob["cost4"][:, 0] != o["cost4"][:, 0]).all()
        assert np.abs(ob["theta"] - o["theta"]).max() > 1e-2
    else:
        # ... the box rests on the table with four contacts of the frictionless
        # pair: one row each where the pyramid has four, 12 rows fewer in the
        # busiest step of every candidate -- and the kernel counts the same
        # rows (a kernel that missed the record's condim-1 bit would count the
        # unedited model's)
        assert (o["maxcon"] >= 4).all() and (ob["maxrows"] - o["maxrows"] == 12).all()
        _, _, st = run(e, td)
        print(f"condim1: rows in the busiest step, kernel {max_rows(st)[:8]}, oracle {o['maxrows'][:8]}")
        np.testing.assert_array_equal(max_rows(st), o["maxrows"])
    oc = o["cost4"][:, 0]
    rel = np.abs(g["cost4"][:, 0].astype(np.float64) - oc) / np.maximum(np.abs(oc), 1e-6)
    graze = (np.abs(o["slots"]) < 1e-5).any(axis=(1, 2)) if m.nslot else np.zeros(N, bool)
    print(f"{which}: max rel {rel[~graze].max():.2e}, grazing {int(graze.sum())}")
    assert rel[~graze].max() < pu.TOL, rel.max()
    assert graze.mean() < 0.1
    assert np.abs(g["theta"] - o["theta"]).max() < 1e-3
    assert np.abs(g["eef"][..., :3] - o["eef"][..., :3]).max() < 1e-3


def pressed_drive():
    """scene_mjx: the drives of tests/test_gpu_newton_reuse.py (the arm reaches
    the table and the box) with the elbow's velocity replaced, in every second
    candidate, by a constant 2.2 rad/s that folds the forearm onto the upper
    arm."""
    td = sine_thetadot(N, H, DT, 41).reshape(N, 6, H)
    td[::2, 2, :] = 2.2
    return td.reshape(N, 6 * H)


def test_pressed_rows_past_lds(torch_cuda):
    """The arm pressed into the table and onto itself, on the one-wave kernel:
    more than 40 rows in a step (J rows in the HBM slab), a joint-limit row
    and the equality row active -- read from status -- and the costs at the
    oracle's bar."""
    m = models.load("scene_mjx", DT)
    assert int(m.neq) == 1 and set(np.asarray(m.pair_condim[:m.npair]).tolist()) == {3}
    _, _, Pd, _ = basis.planner_basis(H, DT)
    td = pressed_drive()
    # the inputs are chosen on the CPU: the oracle's elbow folds past 2.85 rad in
    # the driven candidates (forearm against upper arm and table: contacts)
    o, sens = pu.conditioning(m, td.astype(np.float64))
    th = oracle.rollout(m, td.astype(np.float64), Q0, W, PT, QT)["theta"].reshape(N, 6, H)
    assert (th[::2, 2].max(axis=1) > 2.85).all()
    lib = _lib.load()
    prev = lib.mpcr_set_two_wave_max_n(-1)
    try:
        lib.mpcr_set_two_wave_max_n(0)
        c4, _, st = run(Engine(m, H, N, Pd), td)
    finally:
        lib.mpcr_set_two_wave_max_n(prev)
    print(f"most rows {max_rows(st).max()}, row sums {row_sum(st).min()}..{row_sum(st).max()}")
    assert not (st & 3).any(), "truncated or non-finite"
    assert max_rows(st).max() > 40, max_rows(st).max()
    # rows of a step = 1 equality + limits + 4 per contact (every pair condim 3).
    # The equality's row is in every step by construction (neq = 1, not
    # disabled), so status cannot say more about it than the oracle's count
    # does (CPU); that the kernel's equality path computes what the record
    # says is test_edited_models_match_oracle[eq_one_joint].  A limit row was
    # active wherever the sum over the steps is not H + a multiple of 4
    assert (o["maxrows"] - 4 * o["maxcon"] >= 1).all()
    assert ((row_sum(st) - H) % 4 != 0).any(), "no joint-limit row seen"
    pu.check(m, c4[:, 0], o, sens, "step records pressed")


def test_multi_and_state_entry_points(torch_cuda):
    """The MULTI and STATE instantiations read the same records: one problem
    through rollout_cost_multi and rollout_cost_state is bitwise rollout_cost."""
    torch = torch_cuda
    m = models.load("scene_mjx", DT)
    _, _, Pd, _ = basis.planner_basis(H, DT)
    e = Engine(m, H, N, Pd)
    td = sine_thetadot(N, H, DT, 41)
    c4, theta, st = run(e, td)
    td_d = torch.as_tensor(td).cuda()
    par = torch.as_tensor(np.stack([Engine.params(Q0, W, PT, QT)])).cuda()
    new = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device="cuda:0")  # noqa: E731
    for call in ("multi", "state"):
        c, th, s = new(N, 4), new(N, 6 * H), new(N, dt=torch.int32)
        if call == "multi":
            e.rollout_cost_multi(td_d, MPCR_LAYOUT_THETADOT, par, 1, c, theta=th, status=s)
        else:
            fin = new(N, e.state_layout()["size"])
            e.rollout_cost_state(td_d, MPCR_LAYOUT_THETADOT, par, 1, c, final_state=fin, theta=th, status=s)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(c.cpu().numpy().view(np.int32), c4.view(np.int32), call)
        np.testing.assert_array_equal(th.cpu().numpy(), theta, call)
        np.testing.assert_array_equal(s.cpu().numpy(), st, call)
    assert max_rows(st).max() > 40
