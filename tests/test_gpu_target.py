"""Target poses as an input of the call (``mpcr_rollout_cost_target``,
``Engine.rollout_cost_state(target=)``, ``cem_planner(target_schedule=)``,
``run_cem_planner(target_velocity=)``).

* a schedule repeating the parameter block's target gives bit for bit the call
  without one: one row shared, one row per problem, a schedule of H equal rows;
* any schedule leaves cost_c, theta, thetadot, final_state and status bit for
  bit what they were, and moves cost_g and cost_r of every candidate;
* with the test schedule S12 (tests/test_target_lib.py: the target translating
  and yawing, its quaternions staged at norm 1.7) the costs meet the parity
  bar of tests/parity_util.py against the fp64 oracle's trace priced by
  ``schedule_cost4`` -- and every total is off the call without a schedule,
  which is why this fails on a build that ignores the input;
* horizon segments over candidate groups read the row of the absolute step;
* scenarios: each scenario its own schedule, bit for bit the replicated call;
* the planner: the flag without a trajectory is the planner without the flag,
  a graph replay reads a trajectory staged since capture, two problems with
  two trajectories equal two planners; the closed loop; argument errors.
"""
import ctypes

import numpy as np
import pytest

import parity_util as pu
from manipulator_mujoco_amd import _lib, basis, models
from manipulator_mujoco_amd.engine import MPCR_LAYOUT_THETADOT, MPCR_LAYOUT_XI, Engine
from test_gpu_scenarios import scenarios_equal_replicated
from test_gpu_state import _engine, _Out, _par_blocks, _same, _two_wave, _xi
from test_target_lib import DT, H12, QUAT_SCALE, VEL, s12, s12_rows, schedule_conditioning

pytestmark = pytest.mark.gpu

Q0 = pu.Q0
BAD_STATUS = 1 | 2 | (1 << 10)  # sync, non-finite, truncated (tests/test_gpu_state.py)


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


def i32(torch, t):
    return t.view(torch.int32)


def dynamics_equal(torch, a, b):
    """What the target may not touch, bit for bit."""
    return (all(torch.equal(i32(torch, x), i32(torch, y)) for x, y in ((a.c[:, 3], b.c[:, 3]), (a.th, b.th),
                                                                      (a.td, b.td), (a.fin, b.fin)))
            and torch.equal(a.st, b.st))


# ---------------------------------------------------------------------------
# 1. a constant schedule is the call without


@pytest.mark.parametrize("name", ["planner_scene", "dual_arm"])
@pytest.mark.parametrize("two_wave", [True, False])
def test_constant_schedule_equals_the_call_without(torch_cuda, name, two_wave):
    torch = torch_cuda
    B, n_per, H = 2, 24, 12
    n = B * n_per
    m, e = _engine(name, H, n)
    blk = e.state_layout()["size"]
    xi, par = _xi(torch, n), _par_blocks(torch, B)
    rows = par[:, 12:20].contiguous()  # each problem's own target: they differ, quaternions not unit
    qn = torch.linalg.norm(rows[:, 4:], dim=1)
    assert not torch.equal(rows[0], rows[1]) and float((qn - 1).abs().min()) > 1e-3
    # for the one shared row: both problems given problem 0's target
    par_eq = par.clone()
    par_eq[1, 12:20] = par[0, 12:20]
    with _two_wave(two_wave):
        ref, per, sched, ref_eq, one = (_Out(torch, n, H, B, blk) for _ in range(5))
        e.rollout_cost_state(xi, MPCR_LAYOUT_XI, par, B, ref.c, **ref.kw())
        e.rollout_cost_state(xi, MPCR_LAYOUT_XI, par, B, per.c, target=rows, **per.kw())
        e.rollout_cost_state(xi, MPCR_LAYOUT_XI, par, B, sched.c, target=rows[:, None].repeat(1, H, 1).contiguous(),
                             target_per_step=True, **sched.kw())
        e.rollout_cost_state(xi, MPCR_LAYOUT_XI, par_eq, B, ref_eq.c, **ref_eq.kw())
        e.rollout_cost_state(xi, MPCR_LAYOUT_XI, par_eq, B, one.c, target=rows[0].contiguous(), **one.kw())
        torch.cuda.synchronize()
    clean(torch, ref, per, sched, ref_eq, one)
    for o in (per, sched):
        ref.assert_equal(torch, o)
    ref_eq.assert_equal(torch, one)
    # with a schedule the parameter block's own target is not used: another one in the block, the same outputs
    par_x = par.clone()
    par_x[:, 12:15] += 0.3
    par_x[:, 16:20] = torch.as_tensor([0.3, -0.2, 0.9, 0.1]).cuda()
    other = _Out(torch, n, H, B, blk)
    with _two_wave(two_wave):
        e.rollout_cost_state(xi, MPCR_LAYOUT_XI, par_x, B, other.c, target=rows, **other.kw())
        torch.cuda.synchronize()
    ref.assert_equal(torch, other)


# ---------------------------------------------------------------------------
# 2. the target does not touch the dynamics


def two_schedules(torch, par=None):
    """S12 for problem 0, S12 with the velocity negated for problem 1."""
    return dev(torch, np.stack([s12_rows(), s12_rows(vel=-VEL)]))


@pytest.mark.parametrize("name", ["planner_scene", "dual_arm"])
@pytest.mark.parametrize("two_wave", [True, False])
def test_schedule_moves_the_pose_costs_and_nothing_else(torch_cuda, name, two_wave):
    torch = torch_cuda
    B, n_per, H = 2, 24, H12
    n = B * n_per
    m, e = _engine(name, H, n)
    blk = e.state_layout()["size"]
    xi, par = _xi(torch, n), _par_blocks(torch, B)
    with _two_wave(two_wave):
        ref, got = _Out(torch, n, H, B, blk), _Out(torch, n, H, B, blk)
        e.rollout_cost_state(xi, MPCR_LAYOUT_XI, par, B, ref.c, **ref.kw())
        e.rollout_cost_state(xi, MPCR_LAYOUT_XI, par, B, got.c, target=two_schedules(torch), target_per_step=True,
                             **got.kw())
        torch.cuda.synchronize()
    clean(torch, ref, got)
    assert dynamics_equal(torch, ref, got)
    for k, what in ((1, "cost_g"), (2, "cost_r")):
        moved = int((got.c[:, k] != ref.c[:, k]).sum())
        print(f"{name} two_wave={two_wave}: {what} differs on {moved} of {n} candidates")
        assert moved == n


# ---------------------------------------------------------------------------
# 3. oracle parity under S12


@pytest.fixture(scope="module", params=["scene_mjx", "dual_arm"])
def s12_case(request):
    """The batch, and the oracle's record priced against S12 (computed once)."""
    name = request.param
    n = 64 if name == "scene_mjx" else 32
    m = models.load(name, 0.05)
    td = np.random.default_rng(1).uniform(-0.6, 0.6, (n, 6 * H12))
    pos, rot = s12()
    o, sens = schedule_conditioning(m, td, pos, rot, seed=1)
    assert set(("cost4", "sens4", "probe_b4", "probe_b", "nneg", "nneg_unstable")) <= set(o) and "probe_f4" not in o
    assert (m.nslot == 0) or "slots" in o
    # the conditions of this case, on the oracle alone
    assert o["status"] == 0
    print(f"{name}: oracle busiest step {int(o['maxrows'].max())} rows")
    assert int(o["maxrows"].max()) == (19 if name == "scene_mjx" else 60)  # within what the kernels keep
    if name == "scene_mjx":
        for k in (1, 2):
            assert (o["sens4"][:, k] < pu.TOL / 10).all()  # cost_g, cost_r well-conditioned on all 64
    return dict(name=name, m=m, n=n, td=td, o=o, sens=sens)


@pytest.mark.parametrize("two_wave", [True, False])
def test_s12_costs_meet_the_parity_bar(torch_cuda, s12_case, two_wave):
    torch = torch_cuda
    c = s12_case
    n, H, m, name = c["n"], H12, c["m"], c["name"]
    _, _, Pd, _ = basis.planner_basis(H, DT)
    e = Engine(m, H, n, Pd)
    td = dev(torch, c["td"])
    par = dev(torch, Engine.params(pu.Q0, pu.W, pu.PT, pu.QT))
    sched = dev(torch, s12_rows()[None])
    assert abs(float(torch.linalg.norm(sched[0, 3, 4:])) - QUAT_SCALE) < 1e-5
    cost, base = torch.zeros((n, 4), device="cuda"), torch.zeros((n, 4), device="cuda")
    status, status0 = (torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(2))
    with _two_wave(two_wave):
        e.rollout_cost_state(td, MPCR_LAYOUT_THETADOT, par, 1, cost, target=sched, target_per_step=True, status=status)
        e.rollout_cost_state(td, MPCR_LAYOUT_THETADOT, par, 1, base, status=status0)
        torch.cuda.synchronize()
    assert int((status & BAD_STATUS).sum()) == 0 and int((status0 & BAD_STATUS).sum()) == 0
    g4, b4 = cost.cpu().numpy().astype(np.float64), base.cpu().numpy().astype(np.float64)
    moved = np.abs(g4[:, 0] - b4[:, 0]) / np.abs(b4[:, 0])
    print(f"{name} S12 vs no schedule: relative cost change min {moved.min():.2e} median {np.median(moved):.2e} "
          f"max {moved.max():.2e}")
    label = f"target S12 {name} {n}x{H} two_wave={two_wave}"
    stats = pu.check(m, g4[:, 0], c["o"], c["sens"], label=label)
    comp = pu.check_components(m, g4, c["o"], label=label)
    print(label, stats, comp)
    if name == "scene_mjx":
        assert stats["well"] >= 44  # (47 of 64 on the oracle)
        assert (moved > 5e-3).all()  # (oracle: minimum 1.99e-2)
    else:
        assert stats["well"] >= 30  # (32 of 32 on the oracle)
        assert (moved > 2e-2).all()  # (oracle: minimum 8.8e-2)


# ---------------------------------------------------------------------------
# 4. horizon segments over candidate groups


def switched_rows(p, H, at):
    """Problem p's schedule: its own constant target up to step `at`, another from there."""
    a = Engine.target_rows(pu.PT + 0.02 * p, QUAT_SCALE * pu.QT)
    b = Engine.target_rows(pu.PT + (0.15, -0.1 - 0.03 * p, 0.1), s12()[1][6 + p])
    return np.stack([a] * at + [b] * (H - at))


def test_segmented_groups_read_the_schedule_by_absolute_step(torch_cuda, monkeypatch):
    """The segmented / grouped dual-arm launch found as
    tests/test_gpu_geom_pose.py::test_segmented_groups_read_the_schedule_by_absolute_step
    finds it: segments of 7 and 5 steps over 2 candidate groups, a group
    boundary inside a problem, the schedules switching target at step 9,
    inside the second segment."""
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
    blk, n = e.state_layout()["size"], B * n_per
    tg = dev(torch, np.stack([switched_rows(p, H, 9) for p in range(B)]))
    xi, par = _xi(torch, n), _par_blocks(torch, B)
    got = _Out(torch, n, H, B, blk)
    e.rollout_cost_state(xi, MPCR_LAYOUT_XI, par, B, got.c, target=tg, target_per_step=True, **got.kw())
    torch.cuda.synchronize()
    assert int((got.st & (1 << 10)).sum()) == 0
    for p in range(B):
        sl = slice(p * n_per, (p + 1) * n_per)
        one = _Out(torch, n_per, H, 1, blk)
        e.rollout_cost_state(xi[sl].contiguous(), MPCR_LAYOUT_XI, par[p].contiguous(), 1, one.c,
                             target=tg[p:p + 1].contiguous(), target_per_step=True, **one.kw())
        torch.cuda.synchronize()
        for a, b in ((got.c, one.c), (got.th, one.th), (got.td, one.td), (got.fin, one.fin), (got.st, one.st)):
            assert torch.equal(i32(torch, a[sl]), i32(torch, b)), f"problem {p}"
        assert torch.equal(got.keys[p:p + 1], one.keys), f"problem {p}"
    # the step index is the horizon's: the step-11 row held from step 0 costs something else
    early = _Out(torch, n, H, B, blk)
    e.rollout_cost_state(xi, MPCR_LAYOUT_XI, par, B, early.c, target=tg[:, H - 1].contiguous(), **early.kw())
    torch.cuda.synchronize()
    assert dynamics_equal(torch, got, early)
    assert int((got.c[:, 1] != early.c[:, 1]).sum()) == n and int((got.c[:, 2] != early.c[:, 2]).sum()) == n


# ---------------------------------------------------------------------------
# 5. scenarios


@pytest.mark.parametrize("two_wave", [True, False])
def test_scenarios_each_with_its_own_schedule(torch_cuda, two_wave):
    torch = torch_cuda
    B, S, n_per, H = 2, 3, 16, H12
    m, e = _engine("planner_scene", H, B * S * n_per)
    vels = [VEL * f for f in (1.0, -1.0, 0.4)]
    tg = dev(torch, np.stack([s12_rows(vel=vels[s] * (1.0 + 0.25 * p)) for p in range(B) for s in range(S)]))
    with _two_wave(two_wave):
        # (cost4_scen, final_state, status against rollout_cost_state(target=) over the B S problems;
        #  the fold against the numpy scenario_reduce of those rows; theta / thetadot scenario 0's)
        got, ref = scenarios_equal_replicated(torch, e, B, S, n_per, H, 2, target=tg, target_per_step=True)
        # each scenario's slice alone, as one problem reading that scenario's schedule
        blk = e.state_layout()["size"]
        xi, par = _xi(torch, B * n_per), _par_blocks(torch, B)
        for p in range(B):
            for s in range(S):
                r = p * S + s
                one = _Out(torch, n_per, H, 1, blk)
                e.rollout_cost_state(xi[p * n_per:(p + 1) * n_per].contiguous(), MPCR_LAYOUT_XI, par[p].contiguous(), 1,
                                     one.c, target=tg[r:r + 1].contiguous(), target_per_step=True, **one.kw())
                torch.cuda.synchronize()
                assert torch.equal(i32(torch, got.cs[r * n_per:(r + 1) * n_per]), i32(torch, one.c)), (p, s)
    assert int((ref.st & BAD_STATUS).sum()) == 0 and torch.isfinite(ref.c).all()
    tot = got.cs.view(B, S, n_per, 4)[..., 0]
    for p in range(B):
        for s, t in ((0, 1), (0, 2), (1, 2)):
            assert int((tot[p, s] != tot[p, t]).sum()) == n_per  # every candidate priced per scenario


@pytest.mark.parametrize("name", ["planner_scene", "dual_arm"])
def test_one_scenario_with_a_schedule_is_rollout_cost_state(torch_cuda, name):
    from test_gpu_scenarios import _ScenOut
    torch = torch_cuda
    B, n_per, H = 2, 16, H12
    m, e = _engine(name, H, B * n_per)
    blk = e.state_layout()["size"]
    xi, par = _xi(torch, B * n_per), _par_blocks(torch, B)
    kw = dict(target=two_schedules(torch), target_per_step=True)
    got, ref = _ScenOut(torch, B, 1, n_per, H, blk), _Out(torch, B * n_per, H, B, blk)
    e.rollout_cost_scenarios(xi, MPCR_LAYOUT_XI, par, B, 1, got.cs, **kw, **got.kw())
    e.rollout_cost_state(xi, MPCR_LAYOUT_XI, par, B, ref.c, **kw, **ref.kw())
    torch.cuda.synchronize()
    for a, b in ((got.cs, ref.c), (got.c, ref.c), (got.th, ref.th), (got.td, ref.td), (got.fin, ref.fin)):
        assert torch.equal(i32(torch, a), i32(torch, b))
    assert torch.equal(got.st, ref.st) and torch.equal(got.keys, ref.keys)
    assert torch.isfinite(ref.c).all()


# ---------------------------------------------------------------------------
# 6. the planner


def _planner(**kw):
    from manipulator_mujoco_amd.planner import cem_planner
    args = dict(num_dof=6, num_batch=64, num_steps=12, timestep=0.05, maxiter_cem=2, num_elite=0.05, w_pos=20.0,
                w_rot=3.0, w_col=80.0, maxiter_projection=10, verbose=False, model_path="planner_scene")
    args.update(kw)
    return cem_planner(**args)


def test_planner_prices_the_staged_trajectory(torch_cuda):
    graphed, eager = _planner(graph=True, target_schedule=True), _planner(target_schedule=True)
    plain, plain_graphed = _planner(), _planner(graph=True)
    rng = np.random.default_rng(2)
    tick = (rng.normal(0, 0.2, 66), Q0, np.zeros(6), np.zeros(6), pu.PT, pu.QT)
    # no trajectory: target_pos / target_rot held over the horizon, the planner without the flag
    first = graphed.compute_cem(*tick)
    costs_first = graphed._costs.clone()
    _same(first, plain.compute_cem(*tick))
    _same(first, plain_graphed.compute_cem(*tick))
    _same(first, eager.compute_cem(*tick))
    assert graphed._graphs is not None and len(graphed._graphs) == 1
    assert len(plain_graphed._graphs) == 1  # the captured graph count is what it is without the flag
    captured = graphed._graphs[0]
    # a trajectory staged after capture: a replay of the same graph reads it
    pos, rot = s12()
    second = graphed.compute_cem(*tick, target_traj=(pos, QUAT_SCALE * rot))
    assert graphed._graphs[0] is captured
    moved = int((graphed._costs[..., 0] != costs_first[..., 0]).sum())
    print(f"candidate costs moved by the staged trajectory: {moved} of {costs_first[..., 0].numel()}")
    assert moved > costs_first[..., 0].numel() // 2  # (a replay that ignored the staged rows would move none)
    _same(second, eager.compute_cem(*tick, target_traj=(pos, QUAT_SCALE * rot)))
    _same(second, eager.compute_cem(*tick, target_traj=Engine.target_rows(pos, QUAT_SCALE * rot)))  # rows or a pair
    assert any(not np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(first, second))
    # None does not keep what was staged: the tick's target again
    _same(first, graphed.compute_cem(*tick))
    with pytest.raises(ValueError, match="target_schedule"):
        plain.compute_cem(*tick, target_traj=(pos, rot))
    for bad in (Engine.target_rows(pos, rot)[:-1], (pos[:-1], rot), (pos, rot[:, :3]), np.zeros((12, 7)),
                np.zeros((2, 12, 8))):
        with pytest.raises(ValueError, match="target trajectory"):
            graphed.compute_cem(*tick, target_traj=bad)


def test_planner_batch_with_two_trajectories_equals_two_planners(torch_cuda):
    B = 2
    batch = _planner(graph=True, target_schedule=True, num_problems=B, seed_step=1, seed=5)
    singles = [_planner(target_schedule=True, seed=5 + p) for p in range(B)]
    rng = np.random.default_rng(7)
    tick = dict(xi_mean=rng.normal(0, 0.2, (B, 66)), init_pos=Q0 + rng.uniform(-0.05, 0.05, (B, 6)),
                target_pos=pu.PT + rng.uniform(-0.1, 0.1, (B, 3)),
                target_rot=np.array([[0.0, 1.0, 0.0, 0.0], [0.7071, 0.7071, 0.0, 0.0]]))
    trajs = [s12(), s12(vel=-VEL, yaw_rate=-0.5)]
    for tr in (trajs, [trajs[0], None], None):  # (a None entry, or none at all: that problem's target held)
        out = batch.compute_cem_batch(**tick, target_trajs=tr)
        for p in range(B):
            ref = singles[p].compute_cem(tick["xi_mean"][p], tick["init_pos"][p], None, None, tick["target_pos"][p],
                                         tick["target_rot"][p], target_traj=None if tr is None else tr[p])
            for j in range(9):
                np.testing.assert_array_equal(np.asarray(out[j][p]), np.asarray(ref[j]), err_msg=f"entry {j} problem {p}")
    with pytest.raises(ValueError, match="target trajectories"):
        batch.compute_cem_batch(**tick, target_trajs=trajs[:1])


def test_planner_scenarios_take_one_schedule_each(torch_cuda):
    S = 2
    scen = _planner(target_schedule=True, num_scenarios=S)
    rng = np.random.default_rng(3)
    tick = (rng.normal(0, 0.2, 66), Q0, np.zeros(6), np.zeros(6), pu.PT, pu.QT)
    both = np.stack([Engine.target_rows(*s12()), Engine.target_rows(*s12(vel=-VEL))])
    scen.compute_cem(*tick, target_traj=both)
    sc = scen.scenario_costs[:, 0].cpu().numpy()  # (it, S, n, 4)
    assert (sc[:, 0, :, 1] != sc[:, 1, :, 1]).all()
    # one schedule goes to every scenario: the scenarios then agree
    scen.compute_cem(*tick, target_traj=both[0])
    sc = scen.scenario_costs[:, 0].cpu().numpy()
    np.testing.assert_array_equal(sc[:, 0], sc[:, 1])


# ---------------------------------------------------------------------------
# 7. argument errors


def test_target_calls_validate_their_arguments(torch_cuda):
    torch = torch_cuda
    H, n = 8, 16
    m, e = _engine("planner_scene", H, n)
    lib = _lib.load()
    z = lambda *s: torch.zeros(s, device="cuda")  # noqa: E731
    xi, par, c = z(n, 66), z(2, 20), z(n, 4)
    tg = dev(torch, np.tile(Engine.target_rows(pu.PT, pu.QT), (2, H + 2, 2, 1)))  # (room for the odd strides below)
    par[:] = dev(torch, Engine.params(Q0, pu.W, pu.PT, pu.QT))
    ptr = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)  # noqa: E731
    F = _lib.MPCR_F_DEVICE_PTRS

    def call(stride, step, tgp=None, flags=F, params=True):
        return lib.mpcr_rollout_cost_target(e.handle, ptr(xi), MPCR_LAYOUT_XI, 2, n // 2, ptr(par) if params else None,
                                            None, 0, None, None, 0, 0, None, 0, 0, ptr(tg) if tgp is None else tgp,
                                            stride, step, ptr(c), None, None, None, 0, None, flags, None)

    def call_scen(stride, step):
        cs = z(n, 4)
        return lib.mpcr_rollout_cost_scenarios_target(e.handle, ptr(xi), MPCR_LAYOUT_XI, 1, 2, 2, n // 2, ptr(par),
                                                      None, 0, None, None, 0, 0, None, 0, 0, ptr(tg), stride, step,
                                                      ptr(cs), None, None, None, None, 0, None, F, None)

    EINVAL = -1
    assert call(0, 0) == 0 and call(8, 0) == 0 and call(H * 8, 8) == 0 and call(0, 8) == 0
    assert call((H + 1) * 12, 12) == 0  # padded rows
    assert call_scen(H * 8, 8) == 0
    torch.cuda.synchronize()
    for bad in (4, -8):  # a step stride below a row
        assert call(0, bad) == EINVAL and b"target_step_stride" in lib.mpcr_last_error()
        assert call_scen(0, bad) == EINVAL and b"target_step_stride" in lib.mpcr_last_error()
    for bad in (4, -8):  # a problem stride below a row
        assert call(bad, 0) == EINVAL and b"target_stride" in lib.mpcr_last_error()
    for bad in (8, (H - 1) * 8 + 4):  # ... or below the schedule
        assert call(bad, 8) == EINVAL and b"target_stride" in lib.mpcr_last_error()
    assert b"a target row" in lib.mpcr_last_error()
    # a misaligned pointer or stride
    for off in (4, 8):
        assert call(0, 0, tgp=ptr(tg, off)) == EINVAL and b"16-byte aligned" in lib.mpcr_last_error()
    for s, st in ((10, 0), (H * 8 + 1, 8), ((H + 1) * 10, 10)):
        assert call(s, st) == EINVAL and b"16-byte aligned" in lib.mpcr_last_error()
    host = np.zeros(2 * H * 8 + 4, dtype=np.float32)
    hp = host.ctypes.data + (-host.ctypes.data) % 16
    assert call(0, 0, tgp=ctypes.c_void_p(hp)) == EINVAL and b"device memory" in lib.mpcr_last_error()
    assert call(0, 0, flags=0) == EINVAL and b"device pointers" in lib.mpcr_last_error()
    assert call(0, 0, params=False) == EINVAL  # no device parameter block
    # a problem's offset past what the kernel's parked 32-bit count of 4-float quads holds (refused before any launch)
    far = lib.mpcr_rollout_cost_target(e.handle, ptr(xi), MPCR_LAYOUT_XI, n, 1, ptr(z(n, 20)), None, 0, None, None, 0,
                                       0, None, 0, 0, ptr(tg), 2**31 - 4, 0, ptr(c), None, None, None, 0, None, F, None)
    assert far == EINVAL and b"2^34 floats" in lib.mpcr_last_error()
    torch.cuda.synchronize()
    # shapes
    for bad, kw in ((z(7), {}), (z(3, 8), {}), (z(2, H, 8), {}), (z(2, 8), dict(target_per_step=True)),
                    (z(2, H - 1, 8), dict(target_per_step=True)), (np.zeros(8, np.float32), {}), (torch.zeros(8), {}),
                    (z(8).double(), {})):
        with pytest.raises(ValueError, match="target"):
            e.rollout_cost_state(xi, MPCR_LAYOUT_XI, par, 2, c, target=bad, **kw)
        with pytest.raises(ValueError, match="target"):
            e.rollout_cost_scenarios(xi[:n // 2], MPCR_LAYOUT_XI, par, 1, 2, z(n, 4), target=bad, **kw)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------
# 8. the closed loop


def _loop(**kw):
    from manipulator_mujoco_amd.mpc_planner import run_cem_planner
    args = dict(num_dof=6, num_batch=64, num_steps=12, maxiter_cem=2, maxiter_projection=10, w_pos=20.0, w_rot=3.0,
                w_col=80.0, num_elite=0.05, timestep=0.05, initial_qpos=list(Q0), show_viewer=False, save_data=False,
                max_ticks=6, verbose=False, model_path="planner_scene")
    args.update(kw)
    return run_cem_planner(**args)


def _same_run(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if k != "step_ms":
            np.testing.assert_array_equal(np.asarray(a[k]), np.asarray(b[k]), err_msg=k)


def test_closed_loop_tracks_a_moving_target(torch_cuda, monkeypatch):
    v = (0.05, 0.0, 0.0)
    graphed, eager = _loop(target_velocity=v, graph=True), _loop(target_velocity=v, graph=False)
    _same_run(graphed, eager)
    assert len(graphed["cost"]) == 6 and np.isfinite(np.asarray(graphed["theta"])).all()
    assert np.isfinite(np.asarray(graphed["eef_dist"])).all()
    # without the option: the call as it was, and a planner with the flag on and no trajectory is that call
    plain = _loop()
    _same_run(plain, _loop(graph=False))
    _same_run(plain, _loop(planner_kwargs={"target_schedule": True}))
    _same_run(plain, _loop(target_velocity=(0.0, 0.0, 0.0)))  # a target at rest: the held pose, staged as a schedule
    assert any(not np.array_equal(np.asarray(plain[k]), np.asarray(graphed[k])) for k in ("theta", "cost_g"))
    # (reported, not asserted: whether planning against the predicted poses ends closer to the moving target
    #  than aiming at where it is now -- eef_dist is measured to the target's pose at each tick's time)
    from manipulator_mujoco_amd import mpc_planner
    predicted = mpc_planner.moving_target

    def held_target(velocity, num_steps, timestep):
        """``moving_target`` with the pose at the tick's time held over the horizon."""
        mt = predicted(velocity, num_steps, timestep)

        def at(tick, pos, rot):
            now, (_, rots) = mt(tick, pos, rot)
            return now, (np.tile(now, (num_steps, 1)), rots)
        return at

    monkeypatch.setattr(mpc_planner, "moving_target", held_target)
    held = _loop(target_velocity=v)
    print(f"end distance to the moving target after 6 ticks: planning against its predicted poses "
          f"{graphed['eef_dist'][-1]:.4f} m, aiming at its current pose {held['eef_dist'][-1]:.4f} m "
          f"(standing target: {plain['eef_dist'][-1]:.4f} m)")
