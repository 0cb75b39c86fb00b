"""Cost weights per step as an input of the call
(``mpcr_rollout_cost_stepw``, ``Engine.rollout_cost_state(step_w=)``,
``cem_planner(cost_schedule=)``, ``run_cem_planner(terminal_weight=,
discount=)``).

* a schedule of ones gives bit for bit the call without one, in every output:
  shared, per problem, beside ones slot weights and a constant target schedule;
* the parity schedule D (tests/test_stepw_lib.py: 0.85**t, the last step's
  pose terms times 4) leaves theta, thetadot, the final states and the
  statuses bit for bit; a schedule that is D in one column and 1 elsewhere
  leaves the other two cost columns bit for bit;
* a one-hot sweep over the steps sums to the unscheduled columns, and each
  one-hot call's cost_g / cost_r is the oracle's own term of that step -- a
  lane-to-step slip cannot pass;
* D meets the parity bar of tests/parity_util.py against the fp64 oracle's
  record repriced by ``scheduled_cost4`` on the four batches the CPU tests
  hold to the conditioning cap;
* two problems with two schedules equal two one-problem calls; horizon
  segments read the row of the absolute step; scenarios each with their own;
* the planner: the flag without a schedule is the planner without the flag, a
  graph replay reads a schedule staged since capture, two problems with two
  schedules equal two planners; the closed loop; argument errors.
"""
import ctypes

import numpy as np
import pytest

import parity_util as pu
from manipulator_mujoco_amd import _lib, basis, models
from manipulator_mujoco_amd.engine import MPCR_LAYOUT_THETADOT, MPCR_LAYOUT_XI, Engine
from test_gpu_scenarios import _ScenOut, scenarios_equal_replicated
from test_gpu_state import _engine, _Out, _par_blocks, _same, _two_wave, _xi
from test_slotw_lib import BATCH, H12
from test_stepw_lib import PARITY_CASES, parity_case, pose_terms, schedule_d, stepw_conditioning

pytestmark = pytest.mark.gpu

Q0 = pu.Q0
BAD_STATUS = 1 | 2 | (1 << 10)  # sync, non-finite, truncated (tests/test_gpu_state.py)
N_OF = dict(BATCH, dual_arm=32)


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
    """What a schedule may never touch, bit for bit."""
    return (all(torch.equal(i32(torch, x), i32(torch, y)) for x, y in ((a.th, b.th), (a.td, b.td), (a.fin, b.fin)))
            and torch.equal(a.st, b.st))


def col_equal(torch, a, b, k):
    return torch.equal(i32(torch, a.c[:, k]), i32(torch, b.c[:, k]))


def ones_sched(torch, *lead, H=H12):
    """Ones in the three columns that are read, junk in the reserved one."""
    a = torch.ones(lead + (H, 4), device="cuda")
    a[..., 3] = float("nan")
    return a


# ---------------------------------------------------------------------------
# 1. ones are the call without a schedule


@pytest.mark.parametrize("name", ["planner_scene", "scene_mjx", "dual_arm"])
@pytest.mark.parametrize("two_wave", [True, False])
def test_ones_equal_the_call_without(torch_cuda, name, two_wave):
    torch = torch_cuda
    B, H = 2, H12
    n = N_OF[name]
    m, e = _engine(name, H, n)
    blk, ns = e.state_layout()["size"], m.nslot
    xi, par = _xi(torch, n), _par_blocks(torch, B)
    # a constant target schedule: problem p's own parameter-block target at every step
    tg = par[:, 12:20].clone().view(B, 1, 8).expand(B, H, 8).contiguous()
    slot = dict(slot_w=torch.ones(ns, device="cuda")) if ns else {}
    with _two_wave(two_wave):
        ref, one, per, sw, tgt = (_Out(torch, n, H, B, blk) for _ in range(5))
        e.rollout_cost_state(xi, MPCR_LAYOUT_XI, par, B, ref.c, **ref.kw())
        e.rollout_cost_state(xi, MPCR_LAYOUT_XI, par, B, one.c, step_w=ones_sched(torch), **one.kw())
        e.rollout_cost_state(xi, MPCR_LAYOUT_XI, par, B, per.c, step_w=ones_sched(torch, B), **per.kw())
        e.rollout_cost_state(xi, MPCR_LAYOUT_XI, par, B, sw.c, step_w=ones_sched(torch, B), **slot, **sw.kw())
        e.rollout_cost_state(xi, MPCR_LAYOUT_XI, par, B, tgt.c, step_w=ones_sched(torch), target=tg,
                             target_per_step=True, **slot, **tgt.kw())
        torch.cuda.synchronize()
    clean(torch, ref, one, per, sw, tgt)
    if ns:
        assert float(ref.c[:, 3].max()) > 0  # the batch has collision cost to price
    assert float(ref.c[:, 1].min()) > 0 and float(ref.c[:, 2].min()) > 0
    for o in (one, per, sw, tgt):
        ref.assert_equal(torch, o)


# ---------------------------------------------------------------------------
# 2. D moves the costs alone, a column at a time


@pytest.mark.parametrize("name", ["planner_scene", "scene_mjx", "dual_arm"])
@pytest.mark.parametrize("two_wave", [True, False])
def test_d_moves_the_costs_alone_and_a_column_at_a_time(torch_cuda, name, two_wave):
    torch = torch_cuda
    B, H = 2, H12
    n = N_OF[name]
    m, e = _engine(name, H, n)
    blk = e.state_layout()["size"]
    xi, par = _xi(torch, n), _par_blocks(torch, B)
    D = schedule_d()
    with _two_wave(two_wave):
        base, full = _Out(torch, n, H, B, blk), _Out(torch, n, H, B, blk)
        e.rollout_cost_state(xi, MPCR_LAYOUT_XI, par, B, base.c, **base.kw())
        e.rollout_cost_state(xi, MPCR_LAYOUT_XI, par, B, full.c, step_w=dev(torch, D), **full.kw())
        cols = []
        for k in range(3):
            a = np.ones((H, 4), np.float32)
            a[:, k] = D[:, k]
            o = _Out(torch, n, H, B, blk)
            e.rollout_cost_state(xi, MPCR_LAYOUT_XI, par, B, o.c, step_w=dev(torch, a), **o.kw())
            cols.append(o)
        torch.cuda.synchronize()
    clean(torch, base, full, *cols)
    assert dynamics_equal(torch, base, full)
    moved = [int((full.c[:, k] != base.c[:, k]).sum()) for k in range(4)]
    print(f"{name} two_wave={two_wave}: D moves total / cost_g / cost_r / cost_c on {moved} of {n}")
    assert moved[0] == n and moved[1] == n and moved[2] == n
    if m.nslot:
        assert moved[3] > 0
    for k, o in enumerate(cols):
        assert dynamics_equal(torch, base, o)
        for j in range(3):
            if j == k:
                assert col_equal(torch, o, full, 1 + j), (k, j)  # the column under D alone is D's
            else:
                assert col_equal(torch, o, base, 1 + j), (k, j)  # the other two never move


# ---------------------------------------------------------------------------
# 3. step indexing: a one-hot sweep


def test_one_hot_sweep_prices_each_step_by_its_own_row(torch_cuda):
    torch = torch_cuda
    name, H = "planner_scene", H12
    c = parity_case(name, True)  # (the batch and its oracle record; the slot weights are not used here)
    m, n, o = c["m"], c["n"], c["o"]
    _, _, Pd, _ = basis.planner_basis(H, 0.05)
    e = Engine(m, H, n, Pd)
    blk = e.state_layout()["size"]
    td = dev(torch, c["td"])
    par = dev(torch, Engine.params(pu.Q0, pu.W, pu.PT, pu.QT))
    og, orr = pose_terms(o)  # (n, H): the oracle's own terms of each step
    # candidates whose unscheduled cost_g / cost_r are well-conditioned on the oracle
    o1, _ = stepw_conditioning(m, c["td"], np.ones((H, 4)), None, seed=1)
    well_g, well_r = o1["sens4"][:, 1] < pu.TOL / 10, o1["sens4"][:, 2] < pu.TOL / 10
    assert well_g.sum() * 2 >= n and well_r.sum() * 2 >= n
    for two_wave in (True, False):
        with _two_wave(two_wave):
            base = _Out(torch, n, H, 1, blk)
            e.rollout_cost_state(td, MPCR_LAYOUT_THETADOT, par, 1, base.c, **base.kw())
            torch.cuda.synchronize()
            total = np.zeros((n, 4))
            worst_g = worst_r = 0.0
            for k in range(H):
                a = np.zeros((H, 4), np.float32)
                a[k, :3] = 1
                hot = _Out(torch, n, H, 1, blk)
                e.rollout_cost_state(td, MPCR_LAYOUT_THETADOT, par, 1, hot.c, step_w=dev(torch, a), **hot.kw())
                torch.cuda.synchronize()
                assert dynamics_equal(torch, base, hot)
                h4 = hot.c.cpu().numpy().astype(np.float64)
                total += h4
                rg = np.abs(h4[:, 1] - og[:, k]) / np.maximum(np.abs(og[:, k]), 1e-12)
                rr = np.abs(h4[:, 2] - orr[:, k]) / np.maximum(np.abs(orr[:, k]), 1e-12)
                worst_g, worst_r = max(worst_g, rg[well_g].max()), max(worst_r, rr[well_r].max())
                assert rg[well_g].max() < pu.TOL, (two_wave, k, "cost_g", float(rg[well_g].max()))
                assert rr[well_r].max() < pu.TOL, (two_wave, k, "cost_r", float(rr[well_r].max()))
        clean(torch, base)
        b4 = base.c.cpu().numpy().astype(np.float64)
        for j in (1, 2, 3):
            err = np.abs(total[:, j] - b4[:, j]) / np.maximum(np.abs(b4[:, j]), 1e-30)
            err = np.where(b4[:, j] == total[:, j], 0.0, err)
            print(f"{name} two_wave={two_wave} column {j}: one-hot sum against the unscheduled call, worst rel "
                  f"{err.max():.2e}")
            np.testing.assert_allclose(total[:, j], b4[:, j], rtol=2e-5, atol=0)
        print(f"{name} two_wave={two_wave}: one-hot terms against the oracle's, worst rel cost_g {worst_g:.2e} cost_r "
              f"{worst_r:.2e} ({int(well_g.sum())} / {int(well_r.sum())} of {n} well-conditioned)")


# ---------------------------------------------------------------------------
# 4. parity under D


@pytest.mark.parametrize("name,with_w", PARITY_CASES)
@pytest.mark.parametrize("two_wave", [True, False])
def test_d_meets_the_parity_bar(torch_cuda, name, with_w, two_wave):
    torch = torch_cuda
    c = parity_case(name, with_w)
    n, H, m, o = c["n"], H12, c["m"], c["o"]
    assert set(("cost4", "sens4", "probe_b4", "probe_b", "nneg", "nneg_unstable")) <= set(o)
    assert "probe_f4" not in o and o["status"] == 0
    _, _, Pd, _ = basis.planner_basis(H, 0.05)
    e = Engine(m, H, n, Pd)
    blk = e.state_layout()["size"]
    td = dev(torch, c["td"])
    par = dev(torch, Engine.params(pu.Q0, pu.W, pu.PT, pu.QT))
    kw = dict(step_w=dev(torch, c["a"]))
    if with_w:
        kw["slot_w"] = dev(torch, c["w"])
    with _two_wave(two_wave):
        got = _Out(torch, n, H, 1, blk)
        e.rollout_cost_state(td, MPCR_LAYOUT_THETADOT, par, 1, got.c, **kw, **got.kw())
        torch.cuda.synchronize()
    clean(torch, got)
    g4 = got.c.cpu().numpy().astype(np.float64)
    label = f"step weights D {name} {n}x{H} slot weights {'parity' if with_w else 'none'} two_wave={two_wave}"
    oc = o["cost4"][:, 0]
    rel = np.abs(g4[:, 0] - oc) / np.abs(oc)
    print(f"{label}: relative error median {np.median(rel):.2e} worst {rel.max():.2e}")
    stats = pu.check(m, g4[:, 0], o, c["sens"], label=label)
    comp = pu.check_components(m, g4, o, label=label)
    print(label, stats, comp)
    print(f"{label}: well-conditioned {stats['well']} of {n}, worst of them {stats['max_rel_well']:.2e}")
    assert stats["well"] * 2 >= n


# ---------------------------------------------------------------------------
# 5. problems


@pytest.mark.parametrize("two_wave", [True, False])
def test_two_problems_with_two_schedules_equal_two_calls(torch_cuda, two_wave):
    torch = torch_cuda
    name, B, H = "planner_scene", 2, H12
    n = BATCH[name]
    n_per = n // B
    m, e = _engine(name, H, n)
    blk = e.state_layout()["size"]
    xi, par = _xi(torch, n), _par_blocks(torch, B)
    D = schedule_d()
    a = dev(torch, np.stack([D, D[::-1]]))  # D and its time reverse
    with _two_wave(two_wave):
        got, same = _Out(torch, n, H, B, blk), _Out(torch, n, H, B, blk)
        e.rollout_cost_state(xi, MPCR_LAYOUT_XI, par, B, got.c, step_w=a, **got.kw())
        e.rollout_cost_state(xi, MPCR_LAYOUT_XI, par, B, same.c, step_w=a[0].contiguous(), **same.kw())
        torch.cuda.synchronize()
        for p in range(B):
            sl = slice(p * n_per, (p + 1) * n_per)
            one = _Out(torch, n_per, H, 1, blk)
            e.rollout_cost_state(xi[sl].contiguous(), MPCR_LAYOUT_XI, par[p].contiguous(), 1, one.c,
                                 step_w=a[p].contiguous(), **one.kw())
            torch.cuda.synchronize()
            got.assert_equal(torch, one, sl=sl, p=slice(p, p + 1), msg=f"problem {p}")
    clean(torch, got, same)
    # problem 1 reads its own schedule: the shared one prices it differently
    assert torch.equal(i32(torch, got.c[:n_per]), i32(torch, same.c[:n_per]))
    assert int((got.c[n_per:, 1] != same.c[n_per:, 1]).sum()) == n_per


# ---------------------------------------------------------------------------
# 6. horizon segments


def switched(p, H, at):
    """Ones up to step ``at``, then 3 (problem p: 3 + p / 2)."""
    a = np.ones((H, 4), np.float32)
    a[at:, :3] = 3.0 + 0.5 * p
    a[:, 3] = 0
    return a


def test_segmented_groups_read_the_schedule_by_absolute_step(torch_cuda, monkeypatch):
    """The segmented / grouped dual-arm launch found as
    tests/test_gpu_target.py::test_segmented_groups_read_the_schedule_by_absolute_step
    finds it: segments of 7 and 5 steps over 2 candidate groups, a group
    boundary inside a problem, the schedules switching at step 9, inside the
    second segment."""
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
    a9 = dev(torch, np.stack([switched(p, H, 9) for p in range(B)]))
    a8 = dev(torch, np.stack([switched(p, H, 8) for p in range(B)]))
    xi, par = _xi(torch, n), _par_blocks(torch, B)
    got = _Out(torch, n, H, B, blk)
    e.rollout_cost_state(xi, MPCR_LAYOUT_XI, par, B, got.c, step_w=a9, **got.kw())
    torch.cuda.synchronize()
    assert int((got.st & (1 << 10)).sum()) == 0
    for p in range(B):
        sl = slice(p * n_per, (p + 1) * n_per)
        one = _Out(torch, n_per, H, 1, blk)
        e.rollout_cost_state(xi[sl].contiguous(), MPCR_LAYOUT_XI, par[p].contiguous(), 1, one.c,
                             step_w=a9[p:p + 1].contiguous(), **one.kw())
        torch.cuda.synchronize()
        for x, y in ((got.c, one.c), (got.th, one.th), (got.td, one.td), (got.fin, one.fin), (got.st, one.st)):
            assert torch.equal(i32(torch, x[sl]), i32(torch, y)), f"problem {p}"
        assert torch.equal(got.keys[p:p + 1], one.keys), f"problem {p}"
    # the step index is the horizon's: the same schedule switching a step earlier costs something else
    early = _Out(torch, n, H, B, blk)
    e.rollout_cost_state(xi, MPCR_LAYOUT_XI, par, B, early.c, step_w=a8, **early.kw())
    torch.cuda.synchronize()
    assert dynamics_equal(torch, got, early)
    assert int((got.c[:, 1] != early.c[:, 1]).sum()) == n and int((got.c[:, 2] != early.c[:, 2]).sum()) == n


# ---------------------------------------------------------------------------
# 7. scenarios


@pytest.mark.parametrize("two_wave", [True, False])
def test_scenarios_each_with_its_own_schedule(torch_cuda, two_wave):
    torch = torch_cuda
    B, S, n_per, H = 2, 3, 16, H12
    m, e = _engine("planner_scene", H, B * S * n_per)
    D = schedule_d()
    scheds = [D, D[::-1].copy(), Engine.step_weights(H, running=(0, 0, 1), terminal=1.0)]
    scheds[2][H - 1, :2] = 5.0  # the pose terms on arrival only
    a = dev(torch, np.stack([scheds[s] * np.float32(1.0 + 0.5 * p) for p in range(B) for s in range(S)]))  # (B S, H, 4)
    with _two_wave(two_wave):
        # (cost4_scen, final_state, status against rollout_cost_state(step_w=) over the B S problems;
        #  the fold against the numpy scenario_reduce of those rows; theta / thetadot scenario 0's)
        got, ref = scenarios_equal_replicated(torch, e, B, S, n_per, H, 2, step_w=a)
        # (B, S, H, 4) is the same call
        blk = e.state_layout()["size"]
        xi, par = _xi(torch, B * n_per), _par_blocks(torch, B)
        pr = par.view(B, 1, 20).expand(B, S, 20).reshape(B * S, 20).contiguous()
        again = _ScenOut(torch, B, S, n_per, H, blk)
        e.rollout_cost_scenarios(xi, MPCR_LAYOUT_XI, pr, B, S, again.cs, worst=2, index_base=7,
                                 step_w=a.view(B, S, H, 4), **again.kw())
        torch.cuda.synchronize()
    for x, y in ((again.cs, got.cs), (again.c, got.c), (again.fin, got.fin)):
        assert torch.equal(i32(torch, x), i32(torch, y))
    assert int((ref.st & BAD_STATUS).sum()) == 0 and torch.isfinite(ref.c).all()
    cg = got.cs.view(B, S, n_per, 4)[..., 1]
    for p in range(B):
        for s, t in ((0, 1), (0, 2), (1, 2)):
            assert int((cg[p, s] != cg[p, t]).sum()) == n_per  # priced per scenario


# ---------------------------------------------------------------------------
# 8. the planner, the closed loop, argument errors


def _planner(**kw):
    from manipulator_mujoco_amd.planner import cem_planner
    args = dict(num_dof=6, num_batch=64, num_steps=12, timestep=0.05, maxiter_cem=2, num_elite=0.05, w_pos=20.0,
                w_rot=3.0, w_col=80.0, maxiter_projection=10, verbose=False, model_path="planner_scene")
    args.update(kw)
    return cem_planner(**args)


def test_planner_prices_the_staged_schedule(torch_cuda):
    graphed, eager = _planner(graph=True, cost_schedule=True), _planner(cost_schedule=True)
    plain, plain_graphed = _planner(), _planner(graph=True)
    rng = np.random.default_rng(2)
    tick = (rng.normal(0, 0.2, 66), Q0, np.zeros(6), np.zeros(6), pu.PT, pu.QT)
    # nothing staged: ones, the planner without the flag
    first = graphed.compute_cem(*tick)
    costs_first = graphed._costs.clone()
    _same(first, plain.compute_cem(*tick))
    _same(first, plain_graphed.compute_cem(*tick))
    _same(first, eager.compute_cem(*tick))
    assert graphed._graphs is not None and len(graphed._graphs) == 1
    assert len(plain_graphed._graphs) == 1  # the captured graph count is what it is without the flag
    captured = graphed._graphs[0]
    # a schedule staged after capture: a replay of the same graph reads it
    D = schedule_d()
    second = graphed.compute_cem(*tick, step_w=D)
    assert graphed._graphs[0] is captured
    moved = int((graphed._costs[..., 1] != costs_first[..., 1]).sum())
    print(f"candidate position costs moved by the staged schedule: {moved} of {costs_first[..., 1].numel()}")
    assert moved > costs_first[..., 1].numel() // 2  # (a replay that ignored the staged schedule would move none)
    _same(second, eager.compute_cem(*tick, step_w=D))
    # None keeps what was staged; ones restore the first plan
    _same(second, graphed.compute_cem(*tick))
    _same(first, graphed.compute_cem(*tick, step_w=Engine.step_weights(12)))
    with pytest.raises(ValueError, match="cost_schedule"):
        plain.compute_cem(*tick, step_w=D)
    for bad in (D[:-1], np.ones((12, 3)), np.ones((2, 12, 4))):
        with pytest.raises(ValueError, match="step-weight schedule"):
            graphed.compute_cem(*tick, step_w=bad)


def test_planner_batch_with_two_schedules_equals_two_planners(torch_cuda):
    B = 2
    batch = _planner(graph=True, cost_schedule=True, num_problems=B, seed_step=1, seed=5)
    singles = [_planner(cost_schedule=True, seed=5 + p) for p in range(B)]
    rng = np.random.default_rng(7)
    tick = dict(xi_mean=rng.normal(0, 0.2, (B, 66)), init_pos=Q0 + rng.uniform(-0.05, 0.05, (B, 6)),
                target_pos=pu.PT + rng.uniform(-0.1, 0.1, (B, 3)),
                target_rot=np.array([[0.0, 1.0, 0.0, 0.0], [0.7071, 0.7071, 0.0, 0.0]]))
    D = schedule_d()
    scheds = [D, D[::-1].copy()]
    for blocks in (scheds, [None, scheds[0]], None):  # (a None entry, or none at all: that problem's schedule stays)
        out = batch.compute_cem_batch(**tick, step_ws=blocks)
        for p in range(B):
            ref = singles[p].compute_cem(tick["xi_mean"][p], tick["init_pos"][p], None, None, tick["target_pos"][p],
                                         tick["target_rot"][p], step_w=None if blocks is None else blocks[p])
            for j in range(9):
                np.testing.assert_array_equal(np.asarray(out[j][p]), np.asarray(ref[j]), err_msg=f"entry {j} problem {p}")
    with pytest.raises(ValueError, match="step-weight schedules"):
        batch.compute_cem_batch(**tick, step_ws=scheds[:1])


def test_closed_loop_with_a_terminal_weight_and_a_discount(torch_cuda):
    from manipulator_mujoco_amd.mpc_planner import run_cem_planner
    args = dict(num_dof=6, num_batch=64, num_steps=12, maxiter_cem=2, maxiter_projection=10, w_pos=20.0, w_rot=3.0,
                w_col=80.0, num_elite=0.05, timestep=0.05, initial_qpos=list(Q0), show_viewer=False, save_data=False,
                max_ticks=3, verbose=False, model_path="planner_scene")
    got = run_cem_planner(terminal_weight=4, discount=0.85, **args)
    assert len(got["cost"]) == 3
    for k in ("cost", "cost_g", "cost_r", "cost_c", "theta"):
        assert np.isfinite(np.asarray(got[k], dtype=np.float64)).all(), k
    plain = run_cem_planner(**args)
    assert any(not np.array_equal(np.asarray(plain[k]), np.asarray(got[k])) for k in ("theta", "cost_g"))


def test_stepw_calls_validate_their_arguments(torch_cuda):
    torch = torch_cuda
    H, n = 8, 16
    m, e = _engine("planner_scene", H, n)
    lib = _lib.load()
    z = lambda *s: torch.zeros(s, device="cuda")  # noqa: E731
    xi, par, c = z(n, 66), z(2, 20), z(n, 4)
    a = torch.ones(2 * 4 * H + 16, device="cuda")
    par[:] = dev(torch, Engine.params(Q0, pu.W, pu.PT, pu.QT))
    ptr = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)  # noqa: E731
    F = _lib.MPCR_F_DEVICE_PTRS

    def call(stride, ap=None, flags=F, params=True, eng=e):
        return lib.mpcr_rollout_cost_stepw(eng.handle, ptr(xi), MPCR_LAYOUT_XI, 2, n // 2, ptr(par) if params else None,
                                           None, 0, None, None, 0, 0, None, 0, 0, None, 0, 0, None, 0,
                                           ptr(a) if ap is None else ap, stride, ptr(c), None, None, None, 0, None,
                                           flags, None)

    def call_scen(stride):
        cs = z(n, 4)
        return lib.mpcr_rollout_cost_scenarios_stepw(e.handle, ptr(xi), MPCR_LAYOUT_XI, 1, 2, 2, n // 2, ptr(par), None,
                                                     0, None, None, 0, 0, None, 0, 0, None, 0, 0, None, 0, ptr(a),
                                                     stride, ptr(cs), None, None, None, None, 0, None, F, None)

    EINVAL = -1
    assert call(0) == 0 and call(4 * H) == 0 and call(4 * H + 4) == 0 and call_scen(4 * H) == 0 and call_scen(0) == 0
    torch.cuda.synchronize()
    for bad in (6, 4 * H + 2, 4 * H - 1):  # a stride that is no multiple of 4
        assert call(bad) == EINVAL and b"16-byte aligned" in lib.mpcr_last_error()
        assert call_scen(bad) == EINVAL and b"16-byte aligned" in lib.mpcr_last_error()
    for bad in (4, 4 * H - 4, -4 * H):  # a stride in (0, 4 H), or negative
        assert call(bad) == EINVAL and b"step_w_stride" in lib.mpcr_last_error()
        assert call_scen(bad) == EINVAL and b"step_w_stride" in lib.mpcr_last_error()
    for off in (4, 8):  # a misaligned pointer
        assert call(0, ap=ptr(a, off)) == EINVAL and b"16-byte aligned" in lib.mpcr_last_error()
    host = np.ones(2 * 4 * H + 4, dtype=np.float32)
    hp = host.ctypes.data + (-host.ctypes.data) % 16
    assert call(0, ap=ctypes.c_void_p(hp)) == EINVAL and b"device memory" in lib.mpcr_last_error()
    assert call(0, flags=0) == EINVAL and b"device pointers" in lib.mpcr_last_error()  # a host-parameter call
    assert call(0, params=False) == EINVAL  # no device parameter block
    # a model without slots takes a schedule: the pose columns
    md, ed = _engine("dual_arm", H, n)
    assert md.nslot == 0
    assert call(0, eng=ed) == 0
    torch.cuda.synchronize()
    # shapes
    for bad in (z(H), z(H, 3), z(3, H, 4), z(2, H - 1, 4), z(2, 2, H, 4), np.ones((H, 4), np.float32), torch.ones(H, 4),
                z(H, 4).double()):
        with pytest.raises(ValueError, match="step_w"):
            e.rollout_cost_state(xi, MPCR_LAYOUT_XI, par, 2, c, step_w=bad)
    for bad in (z(H), z(H, 3), z(3, H, 4), np.ones((H, 4), np.float32)):
        with pytest.raises(ValueError, match="step_w"):
            e.rollout_cost_scenarios(xi[:n // 2], MPCR_LAYOUT_XI, par, 1, 2, z(n, 4), step_w=bad)
    torch.cuda.synchronize()
