"""Rollouts from a given full state, and their final states
(``mpcr_rollout_cost_state``, ``Engine.rollout_cost_state``,
``cem_planner(plan_from_state=True)``).

* a block holding the template state gives bit for bit what
  ``rollout_cost_multi`` gives;
* from a state with the object moved, turned and moving (S1) the costs meet the
  parity bar of tests/parity_util.py against the fp64 oracle started there (the
  model copied with the state written into qpos_init / qvel_init);
* the rollout is what a plant does: ``set_state`` and H plant steps with a
  candidate's joint velocities give its theta row and its final state block bit
  for bit, on the single-arm scene (S1) and the dual arm (D1);
* one block per problem, one block for all, horizon segments over candidate
  groups: bitwise the one-problem calls on the slices;
* the planner: graph replay equals eager, a replay reads the state staged since,
  the template staged equals a planner without the flag, the selected candidate
  costs what the oracle says from S1, two problems from two plants equal two
  planners; argument errors; the closed-loop driver.
"""
import contextlib
import copy
import ctypes

import numpy as np
import pytest

import parity_util as pu
from manipulator_mujoco_amd import _lib, basis, models
from manipulator_mujoco_amd.engine import MPCR_LAYOUT_THETADOT, MPCR_LAYOUT_XI, Engine, Plant, unpack_state

pytestmark = pytest.mark.gpu

Q0 = pu.Q0
PARTS = ("qpos", "qvel", "qacc_warmstart", "qacc", "eef")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@contextlib.contextmanager
def _two_wave(on):
    """The default variant choice (small batches run two waves per candidate)
    or, on=False, one wave per candidate throughout."""
    lib = _lib.load()
    prev = lib.mpcr_set_two_wave_max_n(-1)
    try:
        if not on:
            lib.mpcr_set_two_wave_max_n(0)
        yield
    finally:
        lib.mpcr_set_two_wave_max_n(prev)


def _template(m):
    return np.array(m.qpos_init[:m.nq], dtype=np.float64), np.array(m.qvel_init[:m.nv], dtype=np.float64)


def s1_state(m):
    """S1 (scene_mjx): the object -- its free joint at qpos 8 / dof 8 -- moved
    5 cm / -4 cm, yawed 0.3 rad and given 0.1 / -0.05 m/s."""
    qpos, qvel = _template(m)
    qpos[8:11] += (0.05, -0.04, 0.0)
    qpos[11:15] = (np.cos(0.15), 0.0, 0.0, np.sin(0.15))
    qvel[8:11] = (0.1, -0.05, 0.0)
    return qpos, qvel


def d1_state(m, shift=0.0):
    """D1 (dual_arm): arm 1's fingers at 0.01, arm 2 posed and moving."""
    qpos, qvel = _template(m)
    qpos[6:8] = 0.01
    qpos[8:14] = np.array([0.3, -0.4, 0.5, -0.2, 0.1, 0.2]) + shift
    qvel[8:14] = (0.2, -0.1, 0.1, 0.0, 0.0, 0.0)
    return qpos, qvel


def _baked(m, qpos, qvel):
    """The model whose template state is (qpos, qvel): what the oracle starts from."""
    mb = copy.deepcopy(m)
    mb.qpos_init = np.array(mb.qpos_init, dtype=np.float64)
    mb.qvel_init = np.array(mb.qvel_init, dtype=np.float64)
    mb.qpos_init[:m.nq] = qpos
    mb.qvel_init[:m.nv] = qvel
    return mb


def _engine(name, H, n):
    m = models.load(name, 0.05)
    _, _, Pd, _ = basis.planner_basis(H, 0.05)
    return m, Engine(m, H, n, Pd)


class _Out:
    """Every output of one call, zero-initialised."""

    def __init__(self, torch, n, H, B, blk, dev="cuda:0"):
        new = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=dev)  # noqa: E731
        self.c, self.th, self.td = new(n, 4), new(n, 6 * H), new(n, 6 * H)
        self.st, self.keys, self.fin = new(n, dt=torch.int32), new(B, dt=torch.int64), new(n, blk)

    def kw(self, final=True):
        return dict(theta=self.th, thetadot=self.td, best_keys=self.keys, status=self.st,
                    **({"final_state": self.fin} if final else {}))

    def assert_equal(self, torch, other, sl=slice(None), p=slice(None), final=True, msg=""):
        assert torch.equal(self.c[sl].view(torch.int32), other.c.view(torch.int32)), msg
        assert torch.equal(self.th[sl], other.th) and torch.equal(self.td[sl], other.td), msg
        assert torch.equal(self.st[sl], other.st), msg
        assert torch.equal(self.keys[p], other.keys), msg
        if final:
            assert torch.equal(self.fin[sl].view(torch.int32), other.fin.view(torch.int32)), msg


def _par_blocks(torch, B, dev="cuda:0"):
    rng = np.random.default_rng(11)
    blocks = [Engine.params(Q0 + rng.uniform(-0.1, 0.1, 6), (20.0 + 3 * p, 3.0 - 0.5 * p, 80.0 + 10 * p),
                            pu.PT + rng.uniform(-0.1, 0.1, 3), pu.QT + rng.uniform(-0.3, 0.3, 4)) for p in range(B)]
    return torch.as_tensor(np.stack(blocks)).to(dev)


def _xi(torch, n, dev="cuda:0"):
    g = torch.Generator(device="cpu").manual_seed(5)
    return (0.3 * torch.randn((n, 66), generator=g)).to(dev)


# ---------------------------------------------------------------------------
# 1. a template block is the existing call


@pytest.mark.parametrize("name,B,n_per,two_wave", [("planner_scene", 3, 40, True), ("planner_scene", 3, 40, False),
                                                   ("dual_arm", 2, 24, True)])
def test_template_block_equals_rollout_cost_multi(torch_cuda, name, B, n_per, two_wave):
    torch = torch_cuda
    H, n = 8, B * n_per
    m, e = _engine(name, H, n)
    blk = e.state_layout()["size"]
    xi, par = _xi(torch, n), _par_blocks(torch, B)
    tpl = torch.as_tensor(e.pack_state()).cuda()
    with _two_wave(two_wave):
        ref, got, per = _Out(torch, n, H, B, blk), _Out(torch, n, H, B, blk), _Out(torch, n, H, B, blk)
        e.rollout_cost_multi(xi, MPCR_LAYOUT_XI, par, B, ref.c, **ref.kw(final=False))
        e.rollout_cost_state(xi, MPCR_LAYOUT_XI, par, B, got.c, start=tpl, **got.kw())
        e.rollout_cost_state(xi, MPCR_LAYOUT_XI, par, B, per.c, start=tpl.repeat(B, 1).contiguous(), **per.kw())
        none = _Out(torch, n, H, B, blk)
        e.rollout_cost_state(xi, MPCR_LAYOUT_XI, par, B, none.c, **none.kw())  # no start: the template itself
        torch.cuda.synchronize()
    for o in (got, per, none):
        ref.assert_equal(torch, o, final=False, msg=name)
    assert torch.isfinite(ref.c).all()
    assert torch.equal(got.fin, per.fin) and torch.equal(got.fin, none.fin)
    fin = unpack_state(m, got.fin)
    assert all(np.isfinite(fin[k]).all() for k in PARTS) and np.abs(fin["qvel"]).max() > 0


# ---------------------------------------------------------------------------
# 2. oracle parity from S1


@pytest.fixture(scope="module")
def s1_case():
    """scene_mjx, 64 x 12 uniform joint velocities, and the oracle's costs and
    conditioning from S1 (computed once)."""
    m = models.load("scene_mjx", 0.05)
    n, H = 64, 12
    td = np.random.default_rng(1).uniform(-0.6, 0.6, (n, 6 * H))
    qpos, qvel = s1_state(m)
    mb = _baked(m, qpos, qvel)
    o, sens = pu.conditioning(mb, td, seed=1)
    assert o["status"] == 0
    return dict(m=m, mb=mb, n=n, H=H, td=td, qpos=qpos, qvel=qvel, o=o, sens=sens)


@pytest.mark.parametrize("two_wave", [True, False])
def test_s1_costs_meet_the_parity_bar(torch_cuda, s1_case, two_wave):
    torch = torch_cuda
    c = s1_case
    n, H, m = c["n"], c["H"], c["m"]
    _, _, Pd, _ = basis.planner_basis(H, 0.05)
    e = Engine(m, H, n, Pd)
    td = torch.as_tensor(c["td"].astype(np.float32)).cuda()
    par = torch.as_tensor(Engine.params(pu.Q0, pu.W, pu.PT, pu.QT)).cuda()
    start = torch.as_tensor(e.pack_state(c["qpos"], c["qvel"])).cuda()
    cost, base = torch.zeros((n, 4), device="cuda"), torch.zeros((n, 4), device="cuda")
    status = torch.zeros(n, dtype=torch.int32, device="cuda")
    with _two_wave(two_wave):
        e.rollout_cost_state(td, MPCR_LAYOUT_THETADOT, par, 1, cost, start=start, status=status)
        e.rollout_cost_multi(td, MPCR_LAYOUT_THETADOT, par, 1, base)
        torch.cuda.synchronize()
    assert int((status & (1 | 2 | (1 << 10))).sum()) == 0
    g4, b4 = cost.cpu().numpy().astype(np.float64), base.cpu().numpy().astype(np.float64)
    # the state matters: every candidate's cost is off the template start's by more than 1e-3
    moved = np.abs(g4[:, 0] - b4[:, 0]) / np.abs(b4[:, 0])
    print(f"S1 vs template start: relative cost change min {moved.min():.2e} median {np.median(moved):.2e}")
    assert (moved > 1e-3).all()
    label = f"state S1 scene_mjx {n}x{H} two_wave={two_wave}"
    stats = pu.check(m, g4[:, 0], c["o"], c["sens"], label=label)
    pu.check_components(m, g4, c["o"], label=label)
    print(label, stats)
    assert stats["well"] >= 40  # (50-51 of 64 on the oracle: the bar is about something)


# ---------------------------------------------------------------------------
# 3. the rollout is what a plant does


@pytest.mark.parametrize("name", ["scene_mjx", "dual_arm"])
def test_rollout_from_state_equals_plant_steps_bitwise(torch_cuda, name):
    torch = torch_cuda
    n, H, picks = 8, 10, (0, 3, 7)
    m, e = _engine(name, H, n)
    lay = e.state_layout()
    blk = lay["size"]
    qa = np.asarray(m.ctrl_qposadr[:6])
    qpos, qvel = s1_state(m) if name == "scene_mjx" else d1_state(m)
    qpos[qa] = Q0
    plant = Plant(m)
    plant.set_state(qpos=qpos, qvel=qvel)
    plant.step(np.array([0.2, -0.3, 0.25, 0.1, -0.2, 0.3]))  # one step: a warm start that is not zero
    start = plant.copy_state(torch.zeros(blk, device="cuda"))
    torch.cuda.synchronize()
    S = unpack_state(m, start)
    np.testing.assert_array_equal(S["qpos"], plant.qpos.astype(np.float32))
    np.testing.assert_array_equal(S["qvel"], plant.qvel.astype(np.float32))
    assert np.abs(S["qacc_warmstart"]).max() > 0

    td = np.random.default_rng(3).uniform(-0.6, 0.6, (n, 6 * H)).astype(np.float32)
    td_d = torch.as_tensor(td).cuda()
    par = torch.as_tensor(Engine.params(S["qpos"][qa], pu.W, pu.PT, pu.QT)).cuda()
    outs = []
    for two_wave in (True, False):
        with _two_wave(two_wave):
            o = _Out(torch, n, H, 1, blk)
            e.rollout_cost_state(td_d, MPCR_LAYOUT_THETADOT, par, 1, o.c, start=start, **o.kw())
            torch.cuda.synchronize()
        outs.append(o)
    outs[0].assert_equal(torch, outs[1], msg="one wave against two")
    assert torch.equal(start, plant.copy_state(torch.zeros(blk, device="cuda")))  # the start block is only read
    theta, fin = outs[0].th.cpu().numpy(), unpack_state(m, outs[0].fin)
    for i in picks:
        plant.set_state(qpos=S["qpos"], qvel=S["qvel"], qacc_warmstart=S["qacc_warmstart"])
        v = td[i].reshape(6, H)
        for t in range(H):
            plant.step(v[:, t].astype(np.float64))
            np.testing.assert_array_equal(plant.qpos[qa].astype(np.float32), theta[i].reshape(6, H)[:, t])
        end = unpack_state(m, plant.copy_state(torch.zeros(blk, device="cuda")))
        for k in PARTS:
            np.testing.assert_array_equal(fin[k][i].view(np.int32), end[k].view(np.int32), err_msg=f"{name} {i} {k}")
    # a test that cannot see the state shows nothing: from the template start
    # (same arm joints) every candidate ends somewhere else
    t0 = _Out(torch, n, H, 1, blk)
    e.rollout_cost_state(td_d, MPCR_LAYOUT_THETADOT, par, 1, t0.c, **t0.kw())
    torch.cuda.synchronize()
    fin0 = unpack_state(m, t0.fin)
    assert (np.abs(fin["qpos"] - fin0["qpos"]).max(axis=1) > 1e-3).all()
    assert not np.array_equal(fin["qvel"], fin0["qvel"]) and not np.array_equal(fin["qacc"], fin0["qacc"])


# ---------------------------------------------------------------------------
# 4. one block per problem, one block for all


def _multi_equals_slices(torch, e, m, B, n_per, H, blocks):
    """The call over B problems starting from blocks[p] against B one-problem
    calls on the slices, every output and the final states."""
    blk, n = e.state_layout()["size"], B * n_per
    xi, par = _xi(torch, n), _par_blocks(torch, B)
    start = torch.as_tensor(np.stack(blocks)).cuda()
    got = _Out(torch, n, H, B, blk)
    e.rollout_cost_state(xi, MPCR_LAYOUT_XI, par, B, got.c, start=start, **got.kw())
    torch.cuda.synchronize()
    for p in range(B):
        sl = slice(p * n_per, (p + 1) * n_per)
        one = _Out(torch, n_per, H, 1, blk)
        e.rollout_cost_state(xi[sl].contiguous(), MPCR_LAYOUT_XI, par[p].contiguous(), 1, one.c,
                             start=start[p].contiguous(), **one.kw())
        torch.cuda.synchronize()
        got.assert_equal(torch, one, sl=sl, p=slice(p, p + 1), msg=f"problem {p}")
    assert torch.isfinite(got.c).all()
    return got, xi, par


@pytest.mark.parametrize("two_wave", [True, False])
def test_per_problem_blocks_equal_single_calls(torch_cuda, two_wave):
    torch = torch_cuda
    B, n_per, H = 3, 40, 8
    m, e = _engine("scene_mjx", H, B * n_per)
    blk = e.state_layout()["size"]
    s1 = s1_state(m)
    other = (s1[0].copy(), -2.0 * s1[1])
    other[0][8:11] += (-0.1, 0.08, 0.0)
    blocks = [e.pack_state(), e.pack_state(*s1), e.pack_state(*other, qacc_warmstart=np.full(m.nv, 0.05))]
    with _two_wave(two_wave):
        got, xi, par = _multi_equals_slices(torch, e, m, B, n_per, H, blocks)
        # the problems start differently
        f = unpack_state(m, got.fin)["qpos"].reshape(B, n_per, m.nq)
        assert np.abs(f[0, :, 8:11] - f[1, :, 8:11]).max() > 1e-2
        # stride 0: one block for every problem is that block three times
        shared, thrice = _Out(torch, B * n_per, H, B, blk), _Out(torch, B * n_per, H, B, blk)
        one = torch.as_tensor(blocks[1]).cuda()
        e.rollout_cost_state(xi, MPCR_LAYOUT_XI, par, B, shared.c, start=one, **shared.kw())
        e.rollout_cost_state(xi, MPCR_LAYOUT_XI, par, B, thrice.c, start=one.repeat(B, 1).contiguous(), **thrice.kw())
        torch.cuda.synchronize()
    shared.assert_equal(torch, thrice)
    assert not torch.equal(shared.c, got.c)


# ---------------------------------------------------------------------------
# 5. horizon segments over candidate groups


def test_segmented_groups_read_the_start_once_and_write_the_final_state(torch_cuda):
    """The smallest dual-arm batch that runs as horizon segments over candidate
    groups whose boundaries fall inside problems (as tests/test_gpu_multi.py
    finds it): the first segment alone reads the start block, a group does not
    advance the per-problem start pointer, the last segment writes the final
    states."""
    torch = torch_cuda
    B, H = 3, 8
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
        G = d // 2  # two segments of H = 8
        per = (B * n_per + G - 1) // G
        return d > 1 and d % 2 == 0 and all((g * per) % n_per for g in range(1, G))

    while not straddles(n_per) or probe.dispatches(B * n_per) < 4:
        n_per += 1
        assert n_per <= 1024
    assert probe.dispatches(B * n_per) >= 4 and straddles(n_per)
    del probe
    e = Engine(m, H, B * n_per, Pd)
    blocks = [e.pack_state(*d1_state(m, shift=0.05 * p)) for p in range(B)]
    got, _, _ = _multi_equals_slices(torch, e, m, B, n_per, H, blocks)
    f = unpack_state(m, got.fin)["qpos"].reshape(B, n_per, m.nq)
    assert np.abs(f[0, :, 8:14] - f[2, :, 8:14]).max() > 1e-2  # arm 2 ends where its problem's start put it


# ---------------------------------------------------------------------------
# 6. the planner


def _planner(**kw):
    from manipulator_mujoco_amd.planner import cem_planner
    args = dict(num_dof=6, num_batch=256, num_steps=12, timestep=0.05, maxiter_cem=2, num_elite=0.05, w_pos=20.0,
                w_rot=3.0, w_col=80.0, maxiter_projection=10, verbose=False, model_path="scene_mjx")
    args.update(kw)
    return cem_planner(**args)


def _same(a, b):
    for j, (x, y) in enumerate(zip(a, b)):
        np.testing.assert_array_equal(np.asarray(x), np.asarray(y), err_msg=f"entry {j}")


def _selected_matches_oracle(mb, out, q0, H):
    """The selected-candidate rule of tests/test_gpu_planner.py, per component:
    best_vels rolled out by the fp64 oracle from the tick's start costs what the
    planner reported (total, g, r, c), to 1e-4 or twice the largest spread of 8
    fp32-sized per-step noise draws."""
    td = np.asarray(out[4], dtype=np.float64).T.reshape(1, 6 * H)
    a = pu.oracle.rollout(mb, td, q0, pu.W, pu.PT, pu.QT, want_theta=False)["cost4"][0]
    sens = np.zeros(4)
    for sd in range(1, 9):
        b = pu.oracle.rollout(mb, td, q0, pu.W, pu.PT, pu.QT, want_theta=False, noise=1e-6, seed=sd)["cost4"][0]
        sens = np.maximum(sens, np.abs(a - b) / np.maximum(np.abs(a), 1e-12))
    got = np.array([float(out[0][-1]), float(out[1]), float(out[2]), float(out[3])])
    rel = np.where((a == 0) & (got == 0), 0.0, np.abs(got - a) / np.maximum(np.abs(a), 1e-12))
    print(f"selected candidate vs oracle (cost, g, r, c): rel {rel}, conditioning {sens}")
    assert (rel < np.maximum(pu.TOL, 2 * sens)).all(), (rel, sens, got, a)


def test_planner_plans_from_the_staged_state(torch_cuda):
    H = 12
    graphed, eager = _planner(graph=True, plan_from_state=True), _planner(plan_from_state=True)
    plain = _planner()
    m = graphed.model
    qa = np.asarray(m.ctrl_qposadr[:6])
    rng = np.random.default_rng(2)
    tick = (rng.normal(0, 0.2, 66), Q0, np.zeros(6), np.zeros(6), pu.PT, pu.QT)
    # the template staged (nothing passed yet): the planner without the flag
    first = graphed.compute_cem(*tick)
    _same(first, plain.compute_cem(*tick))
    _same(first, eager.compute_cem(*tick))
    assert graphed._graphs is not None and len(graphed._graphs) == 1
    captured = graphed._graphs[0]
    # the plant moves to S1: a replay of the same graph reads it
    qpos, qvel = s1_state(m)
    qpos[qa] = Q0
    plant = Plant(m)
    plant.set_state(qpos=qpos, qvel=qvel)
    second = graphed.compute_cem(*tick, state=plant)
    assert graphed._graphs[0] is captured
    assert not np.array_equal(second[0], first[0]) and not np.array_equal(second[4], first[4])
    _same(second, eager.compute_cem(*tick, state=(qpos, qvel)))  # the arrays, eagerly
    _same(second, graphed.compute_cem(*tick))  # None keeps what is staged
    _selected_matches_oracle(_baked(m, qpos, qvel), second, Q0, H)
    with pytest.raises(ValueError, match="plan_from_state"):
        plain.compute_cem(*tick, state=plant)


def test_planner_batch_from_two_plants_equals_two_planners(torch_cuda):
    B = 2
    batch = _planner(graph=True, plan_from_state=True, num_problems=B, seed_step=1, seed=5)
    singles = [_planner(plan_from_state=True, seed=5 + p) for p in range(B)]
    m = batch.model
    qa = np.asarray(m.ctrl_qposadr[:6])
    rng = np.random.default_rng(7)
    init = Q0 + rng.uniform(-0.05, 0.05, (B, 6))
    plants = []
    for p, (qpos, qvel) in enumerate((_template(m), s1_state(m))):
        qpos[qa] = init[p]
        plants.append(Plant(m))
        plants[p].set_state(qpos=qpos, qvel=qvel)
        plants[p].step(rng.uniform(-0.3, 0.3, 6))  # (a warm start each, and the arm where the step left it)
        init[p] = plants[p].qpos[qa]
    tick = dict(xi_mean=rng.normal(0, 0.2, (B, 66)), init_pos=init, target_pos=pu.PT + rng.uniform(-0.1, 0.1, (B, 3)),
                target_rot=np.array([[0.0, 1.0, 0.0, 0.0], [0.7071, 0.7071, 0.0, 0.0]]))
    for states in (plants, None):  # (None: both blocks stay staged)
        out = batch.compute_cem_batch(**tick, states=states)
        for p in range(B):
            ref = singles[p].compute_cem(tick["xi_mean"][p], tick["init_pos"][p], None, None, tick["target_pos"][p],
                                         tick["target_rot"][p], state=None if states is None else plants[p])
            for j in range(9):
                np.testing.assert_array_equal(np.asarray(out[j][p]), np.asarray(ref[j]), err_msg=f"entry {j} problem {p}")
    with pytest.raises(ValueError, match="start states"):
        batch.compute_cem_batch(**tick, states=plants[:1])


# ---------------------------------------------------------------------------
# 7. argument errors, 8. the driver


def test_state_calls_validate_their_arguments(torch_cuda):
    torch = torch_cuda
    H, n = 8, 16
    m, e = _engine("planner_scene", H, n)
    lib = _lib.load()
    blk = e.state_layout()["size"]
    z = lambda *s: torch.zeros(s, device="cuda")  # noqa: E731
    xi, par, c, start, fin = z(n, 66), z(2, 20), z(n, 4), z(2, blk), z(n, blk)
    start[:] = torch.as_tensor(e.pack_state()).cuda()
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    F = _lib.MPCR_F_DEVICE_PTRS

    def call(stride, flags=F, nprob=2, n_per=n // 2):
        return lib.mpcr_rollout_cost_state(e.handle, ptr(xi), MPCR_LAYOUT_XI, nprob, n_per, ptr(par), ptr(start), stride,
                                           ptr(fin), ptr(c), None, None, None, 0, None, flags, None)

    assert call(blk) == 0 and call(0) == 0
    # the raw entry is the Engine's call: per-problem start blocks (problem 1's
    # free dofs moving), bit for bit on the costs and the final states
    xi[:], par[:] = _xi(torch, n), _par_blocks(torch, 2)
    start[1, e.state_layout()["qvel"] + 6:e.state_layout()["qvel"] + m.nv] = 0.05
    assert call(blk) == 0
    torch.cuda.synchronize()
    c_ref, fin_ref = z(n, 4), z(n, blk)
    e.rollout_cost_state(xi, MPCR_LAYOUT_XI, par, 2, c_ref, start=start, final_state=fin_ref)
    torch.cuda.synchronize()
    assert torch.equal(c.view(torch.int32), c_ref.view(torch.int32))
    assert torch.equal(fin.view(torch.int32), fin_ref.view(torch.int32))
    for bad in (1, blk - 1, -blk):
        assert call(bad) == -1 and b"start_stride" in lib.mpcr_last_error()
    assert call(blk, flags=0) == -1 and b"device pointers" in lib.mpcr_last_error()  # host-pointer mode: none
    assert call(blk, nprob=3) == -1 and b"max_n" in lib.mpcr_last_error()
    torch.cuda.synchronize()
    host = e.pack_state()
    with pytest.raises(ValueError, match="start"):
        e.rollout_cost_state(xi, MPCR_LAYOUT_XI, par, 2, c, start=host)
    with pytest.raises(ValueError, match="final_state"):
        e.rollout_cost_state(xi, MPCR_LAYOUT_XI, par, 2, c, final_state=np.zeros((n, blk), np.float32))
    with pytest.raises(ValueError, match="start"):
        e.rollout_cost_state(xi, MPCR_LAYOUT_XI, par, 2, c, start=z(3, blk))
    with pytest.raises(ValueError, match="final_state"):
        e.rollout_cost_state(xi, MPCR_LAYOUT_XI, par, 2, c, final_state=z(n - 1, blk))
    plant = Plant(m)
    with pytest.raises(ValueError, match="tensor"):
        plant.copy_state(z(blk - 1))
    host_blk = np.zeros(blk, dtype=np.float32)  # the destination must be device memory on the plant's device
    assert lib.mpcr_plant_copy_state(plant.handle, host_blk.ctypes.data_as(ctypes.c_void_p), None) == -1
    assert b"plant's device" in lib.mpcr_last_error()
    plant.copy_state(z(blk))
    torch.cuda.synchronize()


def test_headless_closed_loop_plans_from_the_plant(torch_cuda):
    from manipulator_mujoco_amd.mpc_planner import run_cem_planner
    out = run_cem_planner(num_dof=6, num_batch=256, num_steps=12, maxiter_cem=2, maxiter_projection=10, w_pos=20.0,
                          w_rot=3.0, w_col=80.0, num_elite=0.05, timestep=0.05, initial_qpos=list(Q0),
                          target_names=["target_0", "home"], show_viewer=False, save_data=False, max_ticks=3,
                          verbose=False, plan_from_state=True)
    assert len(out["cost"]) == 3 and len(out["theta"]) == 3
    assert np.isfinite(np.asarray(out["theta"])).all() and np.isfinite(np.asarray(out["eef_dist"])).all()
    assert np.isfinite(np.asarray(out["cost"], dtype=np.float64)).all()
