"""Static geom poses as an input of the call (``mpcr_rollout_cost_world``,
``Engine.rollout_cost_state(geom_pose=)``, ``Plant.set_geom_poses``,
``cem_planner(geom_poses=)``).

* a block holding the model's own poses gives bit for bit the call without,
  as one block, one per problem and a schedule of H equal blocks;
* engine A given the block of an edited model B is engine B, bit for bit:
  ``obstacle_1`` moved on the planner scene (the costs move), ``table_geom_2``
  raised on the dual arm (theta or the final state moves);
* with ``table_geom_1`` moved on ``scene_mjx`` the costs meet the parity bar of
  tests/parity_util.py against the fp64 oracle of the edited model -- and every
  cost is off the call without a block, which is why this fails on a build that
  ignores the input;
* a table rising 2 mm per step: the scheduled rollout is what a plant does when
  ``set_geom_poses`` is called before each step, the plant follows the oracle
  of the model edited for each step, the object ends higher, and
  ``set_geom_poses(None)`` restores the untouched plant;
* horizon segments over candidate groups and per-problem blocks equal the
  one-problem, one-launch calls on the slices;
* the planner: graph replay equals eager and reads a block staged since
  capture, the own block staged equals a planner without the flag, two problems
  with two blocks equal two planners; argument errors."""
import ctypes

import numpy as np
import pytest

import oracle
import parity_util as pu
from manipulator_mujoco_amd import _lib, basis, models
from manipulator_mujoco_amd.engine import MPCR_LAYOUT_THETADOT, MPCR_LAYOUT_XI, Engine, Model, Plant, unpack_state
from test_geom_pose_lib import MOVE, YAW, move_geom
from test_gpu_state import PARTS, _engine, _Out, _par_blocks, _same, _two_wave, _xi

pytestmark = pytest.mark.gpu

Q0 = pu.Q0
BAD_STATUS = 1 | 2 | (1 << 10)  # sync, non-finite, truncated (tests/test_gpu_state.py)
RISE = 0.002  # the rising table: metres per step


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def dev(torch, a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def clean(torch, *outs):
    for o in outs:
        assert int((o.st & BAD_STATUS).sum()) == 0
        assert torch.isfinite(o.c).all()


def bits_equal(torch, a, b):
    """Every output of two calls, bit for bit (NaN-proof: floats as int32)."""
    i32 = lambda t: t.view(torch.int32)  # noqa: E731
    return (all(torch.equal(i32(x), i32(y)) for x, y in ((a.c, b.c), (a.th, b.th), (a.td, b.td), (a.fin, b.fin)))
            and torch.equal(a.st, b.st) and torch.equal(a.keys, b.keys))


def usable(torch, *outs):
    """No lost two-wave handshake (which voids a rollout); the truncated and
    non-finite counts are printed.  For the dual arm with its second table
    raised: the table pressed into the arm's base makes more constraint rows
    than the kernels keep for some candidates (the oracle counts 64 rows at
    1 cm and 317 at 3 cm against the kernels' 200), which the engine of the
    edited model truncates in the same way."""
    for o in outs:
        assert int((o.st & (1 << 10)).sum()) == 0
        print(f"truncated {int((o.st & 1).sum())}, non-finite {int(((o.st >> 1) & 1).sum())} of {o.st.numel()}")


def edited(name, geom, dpos=MOVE, yaw=YAW):
    """The bundled model with a static geom moved in the world, and its block."""
    mb = move_geom(models.load(name, 0.05), geom, dpos, yaw)
    return mb, Model(mb).geom_poses()[0]


# ---------------------------------------------------------------------------
# 1. a block holding the model's own poses is the existing call


@pytest.mark.parametrize("name", ["planner_scene", "dual_arm"])
@pytest.mark.parametrize("two_wave", [True, False])
def test_own_block_equals_the_call_without(torch_cuda, name, two_wave):
    torch = torch_cuda
    B, n_per, H = 2, 24, 12
    n = B * n_per
    m, e = _engine(name, H, n)
    blk = e.state_layout()["size"]
    xi, par = _xi(torch, n), _par_blocks(torch, B)
    block, _, fixed = e.model.geom_poses()
    assert fixed.any() and e.ngeom == len(block)
    own = dev(torch, block)
    with _two_wave(two_wave):
        ref, one, per, sched = (_Out(torch, n, H, B, blk) for _ in range(4))
        e.rollout_cost_state(xi, MPCR_LAYOUT_XI, par, B, ref.c, **ref.kw())
        e.rollout_cost_state(xi, MPCR_LAYOUT_XI, par, B, one.c, geom_pose=own, **one.kw())
        e.rollout_cost_state(xi, MPCR_LAYOUT_XI, par, B, per.c, geom_pose=own.repeat(B, 1, 1).contiguous(), **per.kw())
        e.rollout_cost_state(xi, MPCR_LAYOUT_XI, par, B, sched.c, geom_pose=own.repeat(B, H, 1, 1).contiguous(),
                             geom_pose_per_step=True, **sched.kw())
        torch.cuda.synchronize()
    clean(torch, ref, one, per, sched)
    for o in (one, per, sched):
        ref.assert_equal(torch, o)


# ---------------------------------------------------------------------------
# 2. the block of an edited model is an engine of that model


@pytest.mark.parametrize("name,geom,dpos,yaw", [("planner_scene", "obstacle_1", MOVE, YAW),
                                                ("dual_arm", "table_geom_2", (0.0, 0.0, 0.03), 0.0)])
@pytest.mark.parametrize("two_wave", [True, False])
def test_block_of_an_edited_model_is_its_engine_bitwise(torch_cuda, name, geom, dpos, yaw, two_wave):
    torch = torch_cuda
    B, n_per, H = 2, 24, 12
    n = B * n_per
    m, ea = _engine(name, H, n)
    mb, block_b = edited(name, geom, dpos, yaw)
    _, _, Pd, _ = basis.planner_basis(H, 0.05)
    eb = Engine(mb, H, n, Pd)
    blk = ea.state_layout()["size"]
    xi, par = _xi(torch, n), _par_blocks(torch, B)
    with _two_wave(two_wave):
        got, want, base = (_Out(torch, n, H, B, blk) for _ in range(3))
        ea.rollout_cost_state(xi, MPCR_LAYOUT_XI, par, B, got.c, geom_pose=dev(torch, block_b), **got.kw())
        eb.rollout_cost_state(xi, MPCR_LAYOUT_XI, par, B, want.c, **want.kw())
        ea.rollout_cost_state(xi, MPCR_LAYOUT_XI, par, B, base.c, **base.kw())
        torch.cuda.synchronize()
    clean(torch, base)
    assert bits_equal(torch, want, got)
    bad = [int((o.st & BAD_STATUS != 0).sum()) for o in (got, want)]
    print(f"{name}: candidates with a truncated / non-finite / sync status: block {bad[0]}, edited engine {bad[1]} of {n}")
    if name == "planner_scene":
        clean(torch, got, want)
        want.assert_equal(torch, got)
        moved = (got.c[:, 0] != base.c[:, 0]).sum().item()
        print(f"{name}: {moved} of {n} costs differ from the unmoved call")
        assert moved > n // 2  # (oracle: 52 of 64 by more than 1e-3)
    else:
        # nslot = 0: the costs do not see the tables; the dynamics do (oracle: theta moves by 4e-5).  The table
        # raised 3 cm into the arm's base makes 317 constraint rows on the oracle, past the 200 the kernels keep:
        # both engines truncate them (status bit 0) alike, so the statuses are compared and not required clean
        i32 = lambda t: t.view(torch.int32)  # noqa: E731
        assert not torch.equal(i32(got.th), i32(base.th)) or not torch.equal(i32(got.fin), i32(base.fin))


# ---------------------------------------------------------------------------
# 3. oracle parity with the table moved


@pytest.fixture(scope="module")
def table_case():
    """scene_mjx, 64 x 12 uniform joint velocities, table_geom_1 moved, and the
    oracle's costs and conditioning on the edited model (computed once)."""
    m = models.load("scene_mjx", 0.05)
    n, H = 64, 12
    td = np.random.default_rng(1).uniform(-0.6, 0.6, (n, 6 * H))
    mb, block_b = edited("scene_mjx", "table_geom_1")
    o, sens = pu.conditioning(mb, td, seed=1)
    return dict(m=m, mb=mb, block=block_b, n=n, H=H, td=td, o=o, sens=sens)


@pytest.mark.parametrize("two_wave", [True, False])
def test_moved_table_costs_meet_the_parity_bar(torch_cuda, table_case, two_wave):
    torch = torch_cuda
    c = table_case
    n, H, m = c["n"], c["H"], c["m"]
    _, _, Pd, _ = basis.planner_basis(H, 0.05)
    e = Engine(m, H, n, Pd)
    td = dev(torch, c["td"])
    par = dev(torch, Engine.params(pu.Q0, pu.W, pu.PT, pu.QT))
    cost, base = torch.zeros((n, 4), device="cuda"), torch.zeros((n, 4), device="cuda")
    status, status0 = (torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(2))
    with _two_wave(two_wave):
        e.rollout_cost_state(td, MPCR_LAYOUT_THETADOT, par, 1, cost, geom_pose=dev(torch, c["block"]), status=status)
        e.rollout_cost_state(td, MPCR_LAYOUT_THETADOT, par, 1, base, status=status0)
        torch.cuda.synchronize()
    assert int((status & BAD_STATUS).sum()) == 0 and int((status0 & BAD_STATUS).sum()) == 0
    g4, b4 = cost.cpu().numpy().astype(np.float64), base.cpu().numpy().astype(np.float64)
    moved = np.abs(g4[:, 0] - b4[:, 0]) / np.abs(b4[:, 0])
    print(f"table moved vs no block: relative cost change min {moved.min():.2e} median {np.median(moved):.2e} "
          f"max {moved.max():.2e}")
    label = f"geom_pose table_geom_1 scene_mjx {n}x{H} two_wave={two_wave}"
    stats = pu.check(c["mb"], g4[:, 0], c["o"], c["sens"], label=label)
    pu.check_components(c["mb"], g4, c["o"], label=label)
    print(label, stats)
    assert stats["well"] >= 44  # (48 of 64 on the oracle)
    assert (moved > 5e-3).all()  # (oracle: minimum 1.27e-2)


# ---------------------------------------------------------------------------
# 4. a moving obstacle: the plant, the schedule and the oracle


def rising(t):
    """scene_mjx with table_geom_1 where step t finds it, and its block."""
    return edited("scene_mjx", "table_geom_1", (0.0, 0.0, RISE * (t + 1)), 0.0)


def test_scheduled_rollout_equals_plant_steps_with_set_geom_poses_bitwise(torch_cuda):
    torch = torch_cuda
    H = 10
    m, e = _engine("scene_mjx", H, 1)
    blk = e.state_layout()["size"]
    qa = np.asarray(m.ctrl_qposadr[:6])
    own = e.model.geom_poses()[0]
    sched = np.stack([rising(t)[1] for t in range(H)])
    r = e.model.geom_row("table_geom_1")
    np.testing.assert_allclose(sched[:, r, 2] - own[r, 2], RISE * np.arange(1, H + 1), atol=1e-7)
    plant, untouched = Plant(m), Plant(m)
    np.testing.assert_array_equal(plant.geom_poses, own)
    plant.step(np.array([0.2, -0.3, 0.25, 0.1, -0.2, 0.3]))  # one step: a warm start that is not zero
    start = plant.copy_state(torch.zeros(blk, device="cuda"))
    torch.cuda.synchronize()
    S = unpack_state(m, start)
    td = np.random.default_rng(3).uniform(-0.3, 0.3, (1, 6 * H)).astype(np.float32)
    par = dev(torch, Engine.params(S["qpos"][qa], pu.W, pu.PT, pu.QT))
    outs = []
    for two_wave in (True, False):
        with _two_wave(two_wave):
            o, flat = _Out(torch, 1, H, 1, blk), _Out(torch, 1, H, 1, blk)
            e.rollout_cost_state(dev(torch, td), MPCR_LAYOUT_THETADOT, par, 1, o.c, start=start,
                                 geom_pose=dev(torch, sched[None]), geom_pose_per_step=True, **o.kw())
            e.rollout_cost_state(dev(torch, td), MPCR_LAYOUT_THETADOT, par, 1, flat.c, start=start, **flat.kw())
            torch.cuda.synchronize()
        outs.append(o)
    clean(torch, *outs, flat)
    outs[0].assert_equal(torch, outs[1], msg="one wave against two")
    theta, fin = outs[0].th.cpu().numpy(), unpack_state(m, outs[0].fin)
    v = td[0].reshape(6, H)
    for t in range(H):
        plant.set_geom_poses(sched[t])
        np.testing.assert_array_equal(plant.geom_poses, sched[t])
        plant.step(v[:, t].astype(np.float64))
        np.testing.assert_array_equal(plant.qpos[qa].astype(np.float32), theta[0].reshape(6, H)[:, t])
    end = unpack_state(m, plant.copy_state(torch.zeros(blk, device="cuda")))
    for k in PARTS:
        np.testing.assert_array_equal(fin[k][0].view(np.int32), end[k].view(np.int32), err_msg=k)
    # the table carries the object (its free joint's z is qpos 10) up
    lift = float(fin["qpos"][0, 10] - unpack_state(m, flat.fin)["qpos"][0, 10])
    print(f"object z after {H} steps, rising table against the static one: +{lift:.3e}")
    assert lift > 1e-2  # (oracle: 1.46e-2)
    # the model's own poses again: the untouched plant, bit for bit
    plant.set_geom_poses(None)
    np.testing.assert_array_equal(plant.geom_poses, own)
    tpl = (np.array(m.qpos_init[:m.nq], dtype=np.float64), np.array(m.qvel_init[:m.nv], dtype=np.float64), np.zeros(m.nv))
    plant.set_state(*tpl)
    untouched.set_state(*tpl)
    for _ in range(5):
        plant.step()
        untouched.step()
        for a, b in ((plant.qpos, untouched.qpos), (plant.qvel, untouched.qvel), (plant.qacc, untouched.qacc)):
            np.testing.assert_array_equal(a, b)


def test_plant_under_a_rising_table_follows_the_oracle(torch_cuda):
    """The per-step loop of
    tests/test_gpu_step_records.py::test_hande_scene_plant_matches_oracle_step
    on scene_mjx, with the oracle stepping the model edited for step t and the
    plant given that model's block before the step; that test's tolerances."""
    m = models.load("scene_mjx", 0.05)
    plant = Plant(m)
    qpos = np.array(m.qpos_init[:m.nq], dtype=np.float64)
    qvel, ws = np.array(m.qvel_init[:m.nv], dtype=np.float64), np.zeros(m.nv)
    z0 = qpos[10]
    static = (qpos.copy(), qvel.copy(), ws.copy())
    for t in range(10):
        mb_t, block_t = rising(t)
        plant.set_geom_poses(block_t)
        plant.set_state(qpos=qpos, qvel=qvel, qacc_warmstart=ws)
        o = oracle.step(mb_t, qpos, qvel, ws)
        plant.step()
        scale = max(1.0, np.abs(o["qacc"]).max())
        np.testing.assert_allclose(plant.qacc, o["qacc"], atol=2e-3 * scale, rtol=2e-3, err_msg=f"step {t}")
        qpos, qvel, ws = o["qpos"], o["qvel"], o["qacc_warmstart"]
        np.testing.assert_allclose(plant.qpos, qpos, atol=1e-5, err_msg=f"step {t}")
        np.testing.assert_allclose(plant.qvel, qvel, atol=1e-4, rtol=1e-3, err_msg=f"step {t}")
        s = oracle.step(m, *static)
        static = (s["qpos"], s["qvel"], s["qacc_warmstart"])
    lift = qpos[10] - static[0][10]
    print(f"oracle: object z {z0:.4f} -> {qpos[10]:.4f}, above the static table's by {lift:.3e}; plant {plant.qpos[10]:.4f}")
    assert lift > 1e-2 and plant.qpos[10] - static[0][10] > 1e-2  # (1.46e-2)


# ---------------------------------------------------------------------------
# 5. horizon segments over candidate groups, per problem


def switched_schedule(m, H, at, dz):
    """The dual arm's own block up to step `at`; from there table_geom_2 raised by dz."""
    own = Model(m).geom_poses()[0]
    s = np.tile(own, (H, 1, 1))
    s[at:] = edited("dual_arm", "table_geom_2", (0.0, 0.0, dz), 0.0)[1]  # (1 cm: 64 rows on the oracle, 3 cm: 317)
    return s


def _geom_multi_equals_slices(torch, e, B, n_per, H, gp, per_step):
    """The call over B problems reading gp[p] against B one-problem calls on the slices."""
    blk, n = e.state_layout()["size"], B * n_per
    xi, par = _xi(torch, n), _par_blocks(torch, B)
    got = _Out(torch, n, H, B, blk)
    e.rollout_cost_state(xi, MPCR_LAYOUT_XI, par, B, got.c, geom_pose=gp, geom_pose_per_step=per_step, **got.kw())
    torch.cuda.synchronize()
    (clean if e.nu == 0 else usable)(torch, got)
    i32 = lambda t: t.view(torch.int32)  # noqa: E731
    for p in range(B):
        sl = slice(p * n_per, (p + 1) * n_per)
        one = _Out(torch, n_per, H, 1, blk)
        e.rollout_cost_state(xi[sl].contiguous(), MPCR_LAYOUT_XI, par[p].contiguous(), 1, one.c,
                             geom_pose=gp[p:p + 1].contiguous(), geom_pose_per_step=per_step, **one.kw())
        torch.cuda.synchronize()
        # every output, bit for bit (floats as int32: a truncated rollout may hold a NaN)
        for a, b in ((got.c, one.c), (got.th, one.th), (got.td, one.td), (got.fin, one.fin), (got.st, one.st)):
            assert torch.equal(i32(a[sl]), i32(b)), f"problem {p}"
        assert torch.equal(got.keys[p:p + 1], one.keys), f"problem {p}"
    return got, xi, par


def test_segmented_groups_read_the_schedule_by_absolute_step(torch_cuda, monkeypatch):
    """The segmented / grouped dual-arm launch found as
    tests/test_gpu_ctrl.py::test_segmented_groups_read_the_schedule_by_absolute_step
    finds it, with H = 12: segments of 7 and 5 steps over 2 candidate groups,
    the schedules switching pose at step 9, inside the second segment, and a
    group boundary inside a problem.  Each one-problem slice is a batch small
    enough to run as one launch."""
    torch = torch_cuda
    B, H = 3, 12
    monkeypatch.setenv("MPCR_SEG_STEPS", "7")
    monkeypatch.setenv("MPCR_SEG_GROUPS", "2")
    m = models.load("dual_arm", 0.05)
    _, _, Pd, _ = basis.planner_basis(H, 0.05)
    probe = Engine(m, H, B * 1024, Pd)
    lo, hi = 1, 1024
    assert probe.dispatches(B * lo) == 1 and probe.dispatches(B * hi) > 1
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if probe.dispatches(B * mid) > 1 else (mid, hi)
    n_per = hi

    def straddles(n_per):
        d = probe.dispatches(B * n_per)
        G = d // 2  # two segments of H = 12
        per = (B * n_per + G - 1) // G
        return d > 1 and d % 2 == 0 and all((g * per) % n_per for g in range(1, G))

    while not straddles(n_per) or probe.dispatches(B * n_per) < 4:
        n_per += 1
        assert n_per <= 1024
    assert probe.dispatches(B * n_per) >= 4 and straddles(n_per) and probe.dispatches(n_per) == 1
    del probe
    e = Engine(m, H, B * n_per, Pd)
    gp = dev(torch, np.stack([switched_schedule(m, H, 9, 0.005 + 0.001 * p) for p in range(B)]))
    got, xi, par = _geom_multi_equals_slices(torch, e, B, n_per, H, gp, True)
    # the step index is the horizon's: a table raised from step 0 on ends elsewhere
    early = _Out(torch, B * n_per, H, B, e.state_layout()["size"])
    e.rollout_cost_state(xi, MPCR_LAYOUT_XI, par, B, early.c, geom_pose=gp[:, H - 1].contiguous(), **early.kw())
    torch.cuda.synchronize()
    usable(torch, early)
    assert not torch.equal(got.fin.view(torch.int32), early.fin.view(torch.int32))


@pytest.mark.parametrize("name,geom,two_wave", [("planner_scene", "obstacle_1", True),
                                                ("planner_scene", "obstacle_1", False), ("dual_arm", "table_geom_2", True)])
def test_per_problem_blocks_equal_single_calls(torch_cuda, name, geom, two_wave):
    torch = torch_cuda
    B, n_per, H = 2, 24, 8
    m, e = _engine(name, H, B * n_per)
    blk = e.state_layout()["size"]
    moves = (((0.0, 0.0, 0.03), 0.0), (MOVE, YAW)) if name == "planner_scene" else (
        ((0.0, 0.0, 0.005), 0.0), ((0.01, -0.01, 0.007), 0.05))
    gp = dev(torch, np.stack([edited(name, geom, *mv)[1] for mv in moves]))
    with _two_wave(two_wave):
        got, xi, par = _geom_multi_equals_slices(torch, e, B, n_per, H, gp, False)
        # stride 0: one block for every problem is that block repeated
        shared, twice = _Out(torch, B * n_per, H, B, blk), _Out(torch, B * n_per, H, B, blk)
        e.rollout_cost_state(xi, MPCR_LAYOUT_XI, par, B, shared.c, geom_pose=gp[1].contiguous(), **shared.kw())
        e.rollout_cost_state(xi, MPCR_LAYOUT_XI, par, B, twice.c, geom_pose=gp[1].repeat(B, 1, 1).contiguous(),
                             **twice.kw())
        torch.cuda.synchronize()
    (clean if e.nu == 0 else usable)(torch, shared, twice)
    assert bits_equal(torch, shared, twice)
    same = lambda a, b: torch.equal(a.view(torch.int32), b.view(torch.int32))  # noqa: E731
    assert same(shared.fin[n_per:], got.fin[n_per:]) and same(shared.c[n_per:], got.c[n_per:])
    # problem 0 read its own block
    assert not (same(shared.fin[:n_per], got.fin[:n_per]) and same(shared.c[:n_per], got.c[:n_per]))


# ---------------------------------------------------------------------------
# 6. the planner


def _planner(**kw):
    from manipulator_mujoco_amd.planner import cem_planner
    args = dict(num_dof=6, num_batch=64, num_steps=12, timestep=0.05, maxiter_cem=2, num_elite=0.05, w_pos=20.0,
                w_rot=3.0, w_col=80.0, maxiter_projection=10, verbose=False, model_path="planner_scene")
    args.update(kw)
    return cem_planner(**args)


def test_planner_rolls_out_under_the_staged_poses(torch_cuda):
    graphed, eager = _planner(graph=True, geom_poses=True), _planner(geom_poses=True)
    plain = _planner()
    _, block_b = edited("planner_scene", "obstacle_1")
    rng = np.random.default_rng(2)
    tick = (rng.normal(0, 0.2, 66), Q0, np.zeros(6), np.zeros(6), pu.PT, pu.QT)
    # the model's own block staged (nothing passed yet): the planner without the flag
    first = graphed.compute_cem(*tick)
    costs_first = graphed._costs.clone()
    _same(first, plain.compute_cem(*tick))
    _same(first, eager.compute_cem(*tick))
    assert graphed._graphs is not None and len(graphed._graphs) == 1
    captured = graphed._graphs[0]
    # the moved obstacle staged after capture: a replay of the same graph reads it
    second = graphed.compute_cem(*tick, geom_pose=block_b)
    assert graphed._graphs[0] is captured
    # (the candidates' costs: the tick's best candidate passes clear of obstacle_1 either way)
    moved = int((graphed._costs[..., 0] != costs_first[..., 0]).sum())
    print(f"candidate costs moved by the staged block: {moved} of {costs_first[..., 0].numel()}")
    assert moved > 0  # (any: a replay that ignored the staged block would move none)
    _same(second, eager.compute_cem(*tick, geom_pose=block_b))
    _same(second, graphed.compute_cem(*tick))  # None keeps what is staged
    # a fresh planner given that block, and a per-step planner holding it over the horizon
    _same(second, _planner(geom_poses=True).compute_cem(*tick, geom_pose=block_b))
    _same(second, _planner(geom_poses="per_step", graph=True).compute_cem(*tick, geom_pose=block_b))
    with pytest.raises(ValueError, match="geom_poses"):
        plain.compute_cem(*tick, geom_pose=block_b)
    with pytest.raises(ValueError, match="geom-pose block"):
        graphed.compute_cem(*tick, geom_pose=block_b[:-1])
    with pytest.raises(ValueError, match="geom-pose block"):
        graphed.compute_cem(*tick, geom_pose=np.tile(block_b, (12, 1, 1)))  # a schedule needs "per_step"


def test_planner_batch_with_two_blocks_equals_two_planners(torch_cuda):
    B = 2
    batch = _planner(graph=True, geom_poses=True, num_problems=B, seed_step=1, seed=5)
    singles = [_planner(geom_poses=True, seed=5 + p) for p in range(B)]
    rng = np.random.default_rng(7)
    blocks = [edited("planner_scene", "obstacle_1")[1], edited("planner_scene", "obstacle_2", (0.0, 0.05, 0.0), -0.2)[1]]
    tick = dict(xi_mean=rng.normal(0, 0.2, (B, 66)), init_pos=Q0 + rng.uniform(-0.05, 0.05, (B, 6)),
                target_pos=pu.PT + rng.uniform(-0.1, 0.1, (B, 3)),
                target_rot=np.array([[0.0, 1.0, 0.0, 0.0], [0.7071, 0.7071, 0.0, 0.0]]))
    for gps in (blocks, None):  # (None: both blocks stay staged)
        out = batch.compute_cem_batch(**tick, geom_poses=gps)
        for p in range(B):
            ref = singles[p].compute_cem(tick["xi_mean"][p], tick["init_pos"][p], None, None, tick["target_pos"][p],
                                         tick["target_rot"][p], geom_pose=None if gps is None else blocks[p])
            for j in range(9):
                np.testing.assert_array_equal(np.asarray(out[j][p]), np.asarray(ref[j]), err_msg=f"entry {j} problem {p}")
    with pytest.raises(ValueError, match="geom-pose blocks"):
        batch.compute_cem_batch(**tick, geom_poses=blocks[:1])


# ---------------------------------------------------------------------------
# 7. argument errors


def test_world_calls_validate_their_arguments(torch_cuda):
    torch = torch_cuda
    H, n = 8, 16
    m, e = _engine("planner_scene", H, n)
    ng = e.ngeom
    blk8 = 8 * ng
    lib = _lib.load()
    z = lambda *s: torch.zeros(s, device="cuda")  # noqa: E731
    xi, par, c = z(n, 66), z(2, 20), z(n, 4)
    gp = dev(torch, np.tile(e.model.geom_poses()[0], (2, H + 1, 1, 1)))  # (room for the odd strides below)
    par[:] = dev(torch, Engine.params(Q0, pu.W, pu.PT, pu.QT))
    ptr = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)  # noqa: E731
    F = _lib.MPCR_F_DEVICE_PTRS

    def call(stride, step, eng=e, gpp=None, flags=F):
        return lib.mpcr_rollout_cost_world(eng.handle, ptr(xi), MPCR_LAYOUT_XI, 2, n // 2, ptr(par), None, 0, None,
                                           None, 0, 0, ptr(gp) if gpp is None else gpp, stride, step, ptr(c), None,
                                           None, None, 0, None, flags, None)

    EINVAL = -1
    assert call(0, 0) == 0 and call(blk8, 0) == 0 and call(H * blk8, blk8) == 0 and call(0, blk8) == 0
    assert call((H + 1) * blk8, blk8 + 4) == 0  # padded rows
    torch.cuda.synchronize()
    # a step stride below a block
    for bad in (4, blk8 - 4, -blk8):
        assert call(0, bad) == EINVAL and b"geom_step_stride" in lib.mpcr_last_error()
    # a problem stride below what a problem reads: a block, or the H blocks of its schedule
    for bad in (4, blk8 - 4, -blk8):
        assert call(bad, 0) == EINVAL and b"geom_stride" in lib.mpcr_last_error()
    for bad in (blk8, (H - 1) * blk8 + blk8 - 4):
        assert call(bad, blk8) == EINVAL and b"geom_stride" in lib.mpcr_last_error()
    # a misaligned pointer or stride
    assert call(0, 0, gpp=ptr(gp, 4)) == EINVAL and b"16-byte aligned" in lib.mpcr_last_error()
    assert call(0, 0, gpp=ptr(gp, 8)) == EINVAL and b"16-byte aligned" in lib.mpcr_last_error()
    for s, st in ((blk8 + 2, 0), (H * blk8 + 1, blk8), ((H + 1) * blk8, blk8 + 2)):
        assert call(s, st) == EINVAL and b"16-byte aligned" in lib.mpcr_last_error()
    host = np.zeros(2 * H * blk8 + 4, dtype=np.float32)
    hp = host.ctypes.data + (-host.ctypes.data) % 16
    assert call(0, 0, gpp=ctypes.c_void_p(hp)) == EINVAL and b"device memory" in lib.mpcr_last_error()
    assert call(0, 0, flags=0) == EINVAL and b"device pointers" in lib.mpcr_last_error()
    torch.cuda.synchronize()
    # shapes
    for bad, kw in ((z(ng - 1, 8), {}), (z(3, ng, 8), {}), (z(2, H, ng, 8), {}), (z(2, ng, 8), dict(geom_pose_per_step=True)),
                    (z(2, H - 1, ng, 8), dict(geom_pose_per_step=True)), (np.zeros((ng, 8), np.float32), {}),
                    (torch.zeros(ng, 8), {}), (z(ng, 8).double(), {}), (z(ng, 7), {})):
        with pytest.raises(ValueError, match="geom_pose"):
            e.rollout_cost_state(xi, MPCR_LAYOUT_XI, par, 2, c, geom_pose=bad, **kw)
    with pytest.raises(ValueError, match="block must be"):
        Plant(m).set_geom_poses(np.zeros((ng + 1, 8)))
    with pytest.raises(ValueError, match="geom_poses"):
        _planner(geom_poses="every_step")
    torch.cuda.synchronize()


def test_a_model_without_static_collision_geoms_is_refused(torch_cuda):
    """hande_scene's only static collision geom is the floor; a copy with the
    floor hung on the (free) gripper base has none."""
    torch = torch_cuda
    m = models.load("hande_scene")
    _, ids, fixed = Model(m).geom_poses()
    assert fixed.sum() == 1
    g = int(ids[np.nonzero(fixed)[0][0]])
    moving_body = int(m.geom_bodyid[int(ids[np.nonzero(~fixed)[0][0]])])
    m.geom_bodyid = np.array(m.geom_bodyid)
    m.geom_bodyid[g] = moving_body
    block, _, fixed = Model(m).geom_poses()
    assert not fixed.any()
    H, n = 4, 4
    try:
        e = Engine(m, H, n, np.zeros((H, 11), dtype=np.float32))
    except _lib.MpcrError as err:
        pytest.skip(f"no engine for a model without static collision geoms could be made cheaply: {err}")
    lib = _lib.load()
    gp, xi, par, c = dev(torch, block), torch.zeros((n, 11 * max(e.nctrl, 1)), device="cuda"), \
        torch.zeros(20, device="cuda"), torch.zeros((n, 4), device="cuda")
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    rc = lib.mpcr_rollout_cost_world(e.handle, ptr(xi), MPCR_LAYOUT_XI, 1, n, ptr(par), None, 0, None, None, 0, 0,
                                     ptr(gp), 0, 0, ptr(c), None, None, None, 0, None, _lib.MPCR_F_DEVICE_PTRS, None)
    assert rc == -1 and b"no static collision geom" in lib.mpcr_last_error()
    with pytest.raises(_lib.MpcrError, match="no static collision geom"):
        Plant(m).set_geom_poses(block)
    torch.cuda.synchronize()
