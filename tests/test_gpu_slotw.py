"""Collision-cost weights per contact slot as an input of the call
(``mpcr_rollout_cost_slotw``, ``Engine.rollout_cost_state(slot_w=)``,
``cem_planner(collision_weights=)``, ``run_cem_planner(touch_target=)``).

* a block of ones gives bit for bit the call without one, in every output: one
  block shared, one per problem, rows padded with junk beyond nslot;
* the weight set X (tests/test_slotw_lib.py: zero on one body's slots, 0.25 on
  one obstacle, 2.0 on the table) leaves cost_g, cost_r, theta, thetadot, the
  final states and the statuses bit for bit, moves cost_c and the total of
  every candidate whose oracle slot distances say it should, and meets the
  parity bar of tests/parity_util.py against the fp64 oracle's slot distances
  priced by ``weighted_cost4`` -- which is why this fails on a build that
  ignores the input;
* two problems with different blocks equal two one-problem calls;
* scenarios: each its own block, bit for bit the replicated call and the fold;
* the planner: the flag without weights is the planner without the flag, a
  graph replay reads weights staged since capture, two problems with two
  blocks equal two planners; the closed loop; argument errors.

No shipped model has a robot-masked pair at index 128 or above
(tests/test_slotw_lib.py asserts it), so the slab path of the single-arm
kernels' slot history is not reached by any of them, with or without weights.
"""
import ctypes

import numpy as np
import pytest

import parity_util as pu
from manipulator_mujoco_amd import _lib, basis, models
from manipulator_mujoco_amd.engine import MPCR_LAYOUT_THETADOT, MPCR_LAYOUT_XI, Engine, Model
from test_gpu_scenarios import _ScenOut, scenarios_equal_replicated
from test_gpu_state import _engine, _Out, _par_blocks, _same, _two_wave, _xi
from test_slotw_lib import (BATCH, H12, PARITY_SCALE, batch_td, parity_weights, slotw_conditioning, weighted_cost4,
                            x_weights)

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


def rest_equal(torch, a, b):
    """What the weights may not touch, bit for bit."""
    return (all(torch.equal(i32(torch, x), i32(torch, y)) for x, y in ((a.c[:, 1], b.c[:, 1]), (a.c[:, 2], b.c[:, 2]),
                                                                      (a.th, b.th), (a.td, b.td), (a.fin, b.fin)))
            and torch.equal(a.st, b.st))


def two_blocks(torch, name, m):
    """X for problem 0, another block for problem 1 (the table free, the robot's wrist geoms at 3)."""
    other = Model(m).slot_weights(geoms={"table_geom_1": 0.0, "robot_0": 3.0, "robot_9": 3.0})
    return dev(torch, np.stack([x_weights(name, m), other]))


# ---------------------------------------------------------------------------
# 1. ones are the call without a block


@pytest.mark.parametrize("name", ["planner_scene", "scene_mjx"])
@pytest.mark.parametrize("two_wave", [True, False])
def test_ones_equal_the_call_without(torch_cuda, name, two_wave):
    torch = torch_cuda
    B, H = 2, H12
    n = BATCH[name]
    m, e = _engine(name, H, n)
    blk, ns = e.state_layout()["size"], m.nslot
    ns4 = (ns + 3) & ~3
    assert ns4 > ns  # both scenes leave room for junk behind a row
    xi, par = _xi(torch, n), _par_blocks(torch, B)
    junk = torch.ones((B, ns4), device="cuda")
    junk[:, ns:] = torch.as_tensor([float("nan"), -7.5, 1e30])[: ns4 - ns].cuda()
    with _two_wave(two_wave):
        ref, one, per, pad = (_Out(torch, n, H, B, blk) for _ in range(4))
        e.rollout_cost_state(xi, MPCR_LAYOUT_XI, par, B, ref.c, **ref.kw())
        e.rollout_cost_state(xi, MPCR_LAYOUT_XI, par, B, one.c, slot_w=torch.ones(ns, device="cuda"), **one.kw())
        e.rollout_cost_state(xi, MPCR_LAYOUT_XI, par, B, per.c, slot_w=torch.ones((B, ns), device="cuda"), **per.kw())
        e.rollout_cost_state(xi, MPCR_LAYOUT_XI, par, B, pad.c, slot_w=junk, **pad.kw())
        torch.cuda.synchronize()
    clean(torch, ref, one, per, pad)
    assert float(ref.c[:, 3].max()) > 0  # the batch has collision cost to price
    for o in (one, per, pad):
        ref.assert_equal(torch, o)


# ---------------------------------------------------------------------------
# 2. X moves cost_c alone, and meets the parity bar


@pytest.fixture(scope="module", params=["planner_scene", "scene_mjx"])
def x_case(request):
    """The batch, and the oracle's record priced by the batch's parity weights
    (X on scene_mjx, X / 4 on planner_scene: tests/test_slotw_lib.py, PARITY_SCALE; computed once)."""
    name = request.param
    m = models.load(name, 0.05)
    td, w = batch_td(name), parity_weights(name, m)
    o, sens = slotw_conditioning(m, td, w, seed=1)
    assert set(("cost4", "sens4", "probe_b4", "probe_b", "nneg", "nneg_unstable", "slots")) <= set(o)
    assert "probe_f4" not in o and o["status"] == 0
    return dict(name=name, m=m, n=len(td), td=td, w=w, o=o, sens=sens)


@pytest.mark.parametrize("two_wave", [True, False])
def test_x_moves_cost_c_alone_and_meets_the_parity_bar(torch_cuda, x_case, two_wave):
    torch = torch_cuda
    c = x_case
    n, H, m, name = c["n"], H12, c["m"], c["name"]
    _, _, Pd, _ = basis.planner_basis(H, 0.05)
    e = Engine(m, H, n, Pd)
    blk = e.state_layout()["size"]
    td = dev(torch, c["td"])
    par = dev(torch, Engine.params(pu.Q0, pu.W, pu.PT, pu.QT))
    par2 = dev(torch, Engine.params(pu.Q0, pu.W * (1, 1, 2), pu.PT, pu.QT))
    w = dev(torch, c["w"])
    wx = dev(torch, x_weights(name, m))
    with _two_wave(two_wave):
        base, got, dbl, wcol2, gotx = (_Out(torch, n, H, 1, blk) for _ in range(5))
        e.rollout_cost_state(td, MPCR_LAYOUT_THETADOT, par, 1, base.c, **base.kw())
        e.rollout_cost_state(td, MPCR_LAYOUT_THETADOT, par, 1, got.c, slot_w=w, **got.kw())
        e.rollout_cost_state(td, MPCR_LAYOUT_THETADOT, par, 1, dbl.c, slot_w=(2 * w).contiguous(), **dbl.kw())
        e.rollout_cost_state(td, MPCR_LAYOUT_THETADOT, par2, 1, wcol2.c, slot_w=w, **wcol2.kw())
        e.rollout_cost_state(td, MPCR_LAYOUT_THETADOT, par, 1, gotx.c, slot_w=wx, **gotx.kw())
        torch.cuda.synchronize()
    clean(torch, base, got, dbl, wcol2, gotx)
    assert rest_equal(torch, base, got) and rest_equal(torch, base, dbl) and rest_equal(torch, base, gotx)
    g4, b4 = got.c.cpu().numpy().astype(np.float64), base.c.cpu().numpy().astype(np.float64)
    x4 = gotx.c.cpu().numpy().astype(np.float64)
    # every candidate whose oracle slot distances move cost_c by more than fp32 noise moves on the GPU: under
    # the parity weights and under X itself
    o = c["o"]
    ones = weighted_cost4(o, np.ones(m.nslot), pu.W)
    for tag, ow, gw in ((f"X x {PARITY_SCALE[name]}", o["cost4"], g4), ("X", weighted_cost4(o, x_weights(name, m), pu.W), x4)):
        should = np.abs(ow[:, 3] - ones[:, 3]) > 1e-3 * np.maximum(ones[:, 3], 1.0)
        moved_c, moved_t = gw[:, 3] != b4[:, 3], gw[:, 0] != b4[:, 0]
        print(f"{name} two_wave={two_wave} {tag}: the oracle moves cost_c on {int(should.sum())} of {n}, the GPU on "
              f"{int(moved_c.sum())} (total: {int(moved_t.sum())})")
        assert should.sum() * 2 >= n and moved_c[should].all() and moved_t[should].all()
        # and by what the oracle says, to the parity tolerance where cost_c is well-conditioned
        okc = o["sens4"][:, 3] < pu.TOL / 10
        relc = np.abs(gw[:, 3] - ow[:, 3]) / np.maximum(np.abs(ow[:, 3]), 1e-12)
        print(f"  cost_c against the oracle's: median rel {np.median(relc):.2e}, worst {relc.max():.2e}, worst of "
              f"{int(okc.sum())} with cost_c well-conditioned {relc[okc].max() if okc.any() else 0.0:.2e}")
    # doubling every weight and doubling w_col scale cost_c alike, to fp32 rounding
    d4, w4 = dbl.c.cpu().numpy().astype(np.float64), wcol2.c.cpu().numpy().astype(np.float64)
    np.testing.assert_allclose(d4[:, 3], 2 * g4[:, 3], rtol=1e-5, atol=1e-6)
    np.testing.assert_array_equal(w4[:, 3], g4[:, 3])
    np.testing.assert_allclose(d4[:, 0], w4[:, 0], rtol=1e-5)
    label = f"slot weights X {name} {n}x{H} two_wave={two_wave}"
    stats = pu.check(m, g4[:, 0], o, c["sens"], label=label)
    comp = pu.check_components(m, g4, o, label=label)
    oc = o["cost4"][:, 0]
    rel = np.abs(g4[:, 0] - oc) / np.abs(oc)
    print(label, stats, comp)
    print(f"{label}: well-conditioned {stats['well']} of {n}, relative error median {np.median(rel):.2e} worst "
          f"{rel.max():.2e}")
    assert stats["well"] * 2 >= n


# ---------------------------------------------------------------------------
# 3. problems


@pytest.mark.parametrize("two_wave", [True, False])
def test_two_problems_with_two_blocks_equal_two_calls(torch_cuda, two_wave):
    torch = torch_cuda
    name, B, H = "planner_scene", 2, H12
    n = BATCH[name]
    n_per = n // B
    m, e = _engine(name, H, n)
    blk = e.state_layout()["size"]
    xi, par = _xi(torch, n), _par_blocks(torch, B)
    w = two_blocks(torch, name, m)
    with _two_wave(two_wave):
        got, same = _Out(torch, n, H, B, blk), _Out(torch, n, H, B, blk)
        e.rollout_cost_state(xi, MPCR_LAYOUT_XI, par, B, got.c, slot_w=w, **got.kw())
        e.rollout_cost_state(xi, MPCR_LAYOUT_XI, par, B, same.c, slot_w=w[0].contiguous(), **same.kw())
        torch.cuda.synchronize()
        for p in range(B):
            sl = slice(p * n_per, (p + 1) * n_per)
            one = _Out(torch, n_per, H, 1, blk)
            e.rollout_cost_state(xi[sl].contiguous(), MPCR_LAYOUT_XI, par[p].contiguous(), 1, one.c,
                                 slot_w=w[p].contiguous(), **one.kw())
            torch.cuda.synchronize()
            got.assert_equal(torch, one, sl=sl, p=slice(p, p + 1), msg=f"problem {p}")
    clean(torch, got, same)
    # problem 1 reads its own block: the shared one prices it differently
    assert torch.equal(i32(torch, got.c[:n_per]), i32(torch, same.c[:n_per]))
    assert int((got.c[n_per:, 3] != same.c[n_per:, 3]).sum()) > n_per // 2


# ---------------------------------------------------------------------------
# 4. scenarios


@pytest.mark.parametrize("two_wave", [True, False])
def test_scenarios_each_with_its_own_block(torch_cuda, two_wave):
    torch = torch_cuda
    B, S, n_per, H = 2, 3, 16, H12
    m, e = _engine("planner_scene", H, B * S * n_per)
    M = Model(m)
    blocks = [x_weights("planner_scene", m), M.slot_weights(geoms={"table_geom_1": 0.0}), M.slot_weights(default=1.5)]
    w = dev(torch, np.stack([blocks[s] * (1.0 + 0.5 * p) for p in range(B) for s in range(S)]))  # (B S, nslot)
    with _two_wave(two_wave):
        # (cost4_scen, final_state, status against rollout_cost_state(slot_w=) over the B S problems;
        #  the fold against the numpy scenario_reduce of those rows; theta / thetadot scenario 0's)
        got, ref = scenarios_equal_replicated(torch, e, B, S, n_per, H, 2, slot_w=w)
        # (B, S, nslot) is the same call
        blk = e.state_layout()["size"]
        xi, par = _xi(torch, B * n_per), _par_blocks(torch, B)
        pr = par.view(B, 1, 20).expand(B, S, 20).reshape(B * S, 20).contiguous()
        again = _ScenOut(torch, B, S, n_per, H, blk)
        e.rollout_cost_scenarios(xi, MPCR_LAYOUT_XI, pr, B, S, again.cs, worst=2, index_base=7,
                                 slot_w=w.view(B, S, -1), **again.kw())
        torch.cuda.synchronize()
    for a, b in ((again.cs, got.cs), (again.c, got.c), (again.fin, got.fin)):
        assert torch.equal(i32(torch, a), i32(torch, b))
    assert int((ref.st & BAD_STATUS).sum()) == 0 and torch.isfinite(ref.c).all()
    cc = got.cs.view(B, S, n_per, 4)[..., 3]
    for p in range(B):
        for s, t in ((0, 1), (0, 2), (1, 2)):
            assert int((cc[p, s] != cc[p, t]).sum()) > n_per // 2  # priced per scenario


def test_one_scenario_with_a_block_is_rollout_cost_state(torch_cuda):
    torch = torch_cuda
    name, B, n_per, H = "planner_scene", 2, 16, H12
    m, e = _engine(name, H, B * n_per)
    blk = e.state_layout()["size"]
    xi, par = _xi(torch, B * n_per), _par_blocks(torch, B)
    kw = dict(slot_w=two_blocks(torch, name, m))
    got, ref = _ScenOut(torch, B, 1, n_per, H, blk), _Out(torch, B * n_per, H, B, blk)
    e.rollout_cost_scenarios(xi, MPCR_LAYOUT_XI, par, B, 1, got.cs, **kw, **got.kw())
    e.rollout_cost_state(xi, MPCR_LAYOUT_XI, par, B, ref.c, **kw, **ref.kw())
    torch.cuda.synchronize()
    for a, b in ((got.cs, ref.c), (got.c, ref.c), (got.th, ref.th), (got.td, ref.td), (got.fin, ref.fin)):
        assert torch.equal(i32(torch, a), i32(torch, b))
    assert torch.equal(got.st, ref.st) and torch.equal(got.keys, ref.keys)
    assert torch.isfinite(ref.c).all()


# ---------------------------------------------------------------------------
# 5. the planner


def _planner(**kw):
    from manipulator_mujoco_amd.planner import cem_planner
    args = dict(num_dof=6, num_batch=64, num_steps=12, timestep=0.05, maxiter_cem=2, num_elite=0.05, w_pos=20.0,
                w_rot=3.0, w_col=80.0, maxiter_projection=10, verbose=False, model_path="planner_scene")
    args.update(kw)
    return cem_planner(**args)


def test_planner_prices_the_staged_weights(torch_cuda):
    graphed, eager = _planner(graph=True, collision_weights=True), _planner(collision_weights=True)
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
    # weights staged after capture: a replay of the same graph reads them
    w = Model(graphed.model).slot_weights(default=1.5)
    second = graphed.compute_cem(*tick, slot_w=w)
    assert graphed._graphs[0] is captured
    moved = int((graphed._costs[..., 3] != costs_first[..., 3]).sum())
    print(f"candidate collision costs moved by the staged weights: {moved} of {costs_first[..., 3].numel()}")
    assert moved > costs_first[..., 3].numel() // 2  # (a replay that ignored the staged block would move none)
    _same(second, eager.compute_cem(*tick, slot_w=w))
    # None keeps what was staged; ones restore the first plan
    _same(second, graphed.compute_cem(*tick))
    _same(first, graphed.compute_cem(*tick, slot_w=np.ones(187, np.float32)))
    with pytest.raises(ValueError, match="collision_weights"):
        plain.compute_cem(*tick, slot_w=w)
    for bad in (w[:-1], np.ones(188), np.ones((2, 187))):
        with pytest.raises(ValueError, match="slot-weight block"):
            graphed.compute_cem(*tick, slot_w=bad)
    with pytest.raises(ValueError, match="collision_weights"):
        _planner(collision_weights=True, model_path="dual_arm", num_batch=8)


def test_planner_batch_with_two_blocks_equals_two_planners(torch_cuda):
    B = 2
    batch = _planner(graph=True, collision_weights=True, num_problems=B, seed_step=1, seed=5)
    singles = [_planner(collision_weights=True, seed=5 + p) for p in range(B)]
    rng = np.random.default_rng(7)
    tick = dict(xi_mean=rng.normal(0, 0.2, (B, 66)), init_pos=Q0 + rng.uniform(-0.05, 0.05, (B, 6)),
                target_pos=pu.PT + rng.uniform(-0.1, 0.1, (B, 3)),
                target_rot=np.array([[0.0, 1.0, 0.0, 0.0], [0.7071, 0.7071, 0.0, 0.0]]))
    M = Model(batch.model)
    ws = [x_weights("planner_scene", batch.model), M.slot_weights(geoms={"table_geom_1": 0.0}, default=1.5)]
    for blocks in (ws, [None, ws[0]], None):  # (a None entry, or none at all: that problem's block stays)
        out = batch.compute_cem_batch(**tick, slot_ws=blocks)
        for p in range(B):
            ref = singles[p].compute_cem(tick["xi_mean"][p], tick["init_pos"][p], None, None, tick["target_pos"][p],
                                         tick["target_rot"][p], slot_w=None if blocks is None else blocks[p])
            for j in range(9):
                np.testing.assert_array_equal(np.asarray(out[j][p]), np.asarray(ref[j]), err_msg=f"entry {j} problem {p}")
    with pytest.raises(ValueError, match="slot-weight blocks"):
        batch.compute_cem_batch(**tick, slot_ws=ws[:1])


def test_planner_scenarios_take_one_block_each(torch_cuda):
    S = 2
    scen = _planner(collision_weights=True, num_scenarios=S)
    rng = np.random.default_rng(3)
    tick = (rng.normal(0, 0.2, 66), Q0, np.zeros(6), np.zeros(6), pu.PT, pu.QT)
    M = Model(scen.model)
    both = np.stack([M.slot_weights(), M.slot_weights(default=1.5)])
    scen.compute_cem(*tick, slot_w=both)
    sc = scen.scenario_costs[:, 0].cpu().numpy()  # (it, S, n, 4)
    assert (sc[:, 0, :, 3] != sc[:, 1, :, 3]).mean() > 0.5
    np.testing.assert_allclose(sc[:, 1, :, 3], 2.25 * sc[:, 0, :, 3], rtol=1e-5)  # both geoms of a slot at 1.5
    np.testing.assert_array_equal(sc[:, 0, :, 1:3], sc[:, 1, :, 1:3])
    # one block goes to every scenario: the scenarios then agree
    scen.compute_cem(*tick, slot_w=both[1])
    sc = scen.scenario_costs[:, 0].cpu().numpy()
    np.testing.assert_array_equal(sc[:, 0], sc[:, 1])


# ---------------------------------------------------------------------------
# 6. argument errors


def test_slotw_calls_validate_their_arguments(torch_cuda):
    torch = torch_cuda
    H, n = 8, 16
    m, e = _engine("planner_scene", H, n)
    ns = m.nslot  # 187: rows of 188
    lib = _lib.load()
    z = lambda *s: torch.zeros(s, device="cuda")  # noqa: E731
    xi, par, c = z(n, 66), z(2, 20), z(n, 4)
    w = torch.ones(2 * 192 + 8, device="cuda")
    par[:] = dev(torch, Engine.params(Q0, pu.W, pu.PT, pu.QT))
    ptr = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)  # noqa: E731
    F = _lib.MPCR_F_DEVICE_PTRS

    def call(stride, wp=None, flags=F, params=True, eng=e):
        return lib.mpcr_rollout_cost_slotw(eng.handle, ptr(xi), MPCR_LAYOUT_XI, 2, n // 2, ptr(par) if params else None,
                                           None, 0, None, None, 0, 0, None, 0, 0, None, 0, 0,
                                           ptr(w) if wp is None else wp, stride, ptr(c), None, None, None, 0, None, flags,
                                           None)

    def call_scen(stride):
        cs = z(n, 4)
        return lib.mpcr_rollout_cost_scenarios_slotw(e.handle, ptr(xi), MPCR_LAYOUT_XI, 1, 2, 2, n // 2, ptr(par), None,
                                                     0, None, None, 0, 0, None, 0, 0, None, 0, 0, ptr(w), stride,
                                                     ptr(cs), None, None, None, None, 0, None, F, None)

    EINVAL = -1
    assert call(0) == 0 and call(188) == 0 and call(192) == 0 and call_scen(188) == 0 and call_scen(0) == 0
    torch.cuda.synchronize()
    for bad in (6, 190, 187):  # a stride that is no multiple of 4
        assert call(bad) == EINVAL and b"16-byte aligned" in lib.mpcr_last_error()
        assert call_scen(bad) == EINVAL and b"16-byte aligned" in lib.mpcr_last_error()
    for bad in (4, 184, -188):  # a stride below nslot
        assert call(bad) == EINVAL and b"slot_w_stride" in lib.mpcr_last_error()
    for off in (4, 8):  # a misaligned pointer
        assert call(0, wp=ptr(w, off)) == EINVAL and b"16-byte aligned" in lib.mpcr_last_error()
    host = np.ones(2 * 192 + 4, dtype=np.float32)
    hp = host.ctypes.data + (-host.ctypes.data) % 16
    assert call(0, wp=ctypes.c_void_p(hp)) == EINVAL and b"device memory" in lib.mpcr_last_error()
    assert call(0, flags=0) == EINVAL and b"device pointers" in lib.mpcr_last_error()  # a host-parameter call
    assert call(0, params=False) == EINVAL  # no device parameter block
    # a model without slots
    md, ed = _engine("dual_arm", H, n)
    assert md.nslot == 0
    assert call(0, eng=ed) == EINVAL and b"nslot = 0" in lib.mpcr_last_error()
    torch.cuda.synchronize()
    # shapes
    for bad in (z(7), z(3, ns), z(2, ns - 1), z(2, 2, ns), np.ones(ns, np.float32), torch.ones(ns), z(ns).double()):
        with pytest.raises(ValueError, match="slot_w"):
            e.rollout_cost_state(xi, MPCR_LAYOUT_XI, par, 2, c, slot_w=bad)
        with pytest.raises(ValueError, match="slot_w"):
            e.rollout_cost_scenarios(xi[:n // 2], MPCR_LAYOUT_XI, par, 1, 2, z(n, 4), slot_w=bad)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------
# 7. the closed loop


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


def test_closed_loop_may_touch_its_target(torch_cuda):
    graphed, eager = _loop(touch_target=True, graph=True), _loop(touch_target=True, graph=False)
    _same_run(graphed, eager)
    assert len(graphed["cost"]) == 6 and np.isfinite(np.asarray(graphed["theta"])).all()
    # without the option: the calls as they were, and a planner with the flag on and nothing staged is that loop
    plain = _loop()
    _same_run(plain, _loop(graph=False))
    _same_run(plain, _loop(planner_kwargs={"collision_weights": True}))
    _same_run(_loop(target_names=["home"]), _loop(touch_target=True, target_names=["home"]))  # "home" exempts nothing
    assert any(not np.array_equal(np.asarray(plain[k]), np.asarray(graphed[k])) for k in ("theta", "cost_c"))
    # (reported, not asserted: six ticks decide nothing)
    print(f"end distance to target_0 after 6 ticks: contacts with it free {graphed['eef_dist'][-1]:.4f} m, charged "
          f"{plain['eef_dist'][-1]:.4f} m; last tick's cost_c {float(graphed['cost_c'][-1]):.3f} against "
          f"{float(plain['cost_c'][-1]):.3f}")
