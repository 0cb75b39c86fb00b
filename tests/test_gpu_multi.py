"""Several independent MPC problems in one batched CEM tick.

The acceptance bar is exact: every multi-problem call is bit for bit the
single-problem calls on its slices (the kernels are independent of batch size
and launch shape), so every comparison here is ``torch.equal`` /
``assert_array_equal`` against the existing single-problem path on the same
inputs -- the rollout (narrow and dual-arm kernels, the segmented / grouped
launch included), the distribution kernels, and whole planner ticks, eager
and graph-replayed.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BOUNDS = (0.8, 1.8, np.pi)
Q0 = np.array([1.5, -1.8, 1.75, -1.25, -1.6, 0.0])


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _param_blocks(B):
    """B different parameter blocks: init_pos, weights, target position and a
    target quaternion that is not normalised."""
    from manipulator_mujoco_amd.engine import Engine
    rng = np.random.default_rng(11)
    blocks = []
    for p in range(B):
        q0 = Q0 + rng.uniform(-0.1, 0.1, 6)
        w = (20.0 + 3 * p, 3.0 - 0.5 * p, 80.0 + 10 * p)
        pt = np.array([-0.3, -0.3, 0.5]) + rng.uniform(-0.1, 0.1, 3)
        qt = np.array([0.0, 1.0, 0.0, 0.0]) + rng.uniform(-0.3, 0.3, 4)
        qt *= 1.0 + 0.5 * (p + 1)  # any norm: the kernel normalises
        blocks.append(Engine.params(q0, w, pt, qt))
    return np.stack(blocks)


def _rollout_multi_equals_slices(torch, model_name, B, n_per, H, index_bases=(0,)):
    from manipulator_mujoco_amd import basis, models
    from manipulator_mujoco_amd.engine import MPCR_LAYOUT_XI, Engine
    dev = torch.device("cuda:0")
    _, _, Pd, _ = basis.planner_basis(H, 0.05)
    e = Engine(models.load(model_name, 0.05), H, B * n_per, Pd)
    g = torch.Generator(device="cpu").manual_seed(5)
    xi = (0.3 * torch.randn((B * n_per, 66), generator=g)).to(dev)
    par = torch.as_tensor(_param_blocks(B)).to(dev)
    new = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=dev)  # noqa: E731
    for ib in index_bases:
        c, th, td = new(B * n_per, 4), new(B * n_per, 6 * H), new(B * n_per, 6 * H)
        st, keys = new(B * n_per, dt=torch.int32), new(B, dt=torch.int64)
        e.rollout_cost_multi(xi, MPCR_LAYOUT_XI, par, B, c, theta=th, thetadot=td, best_keys=keys, index_base=ib,
                             status=st)
        torch.cuda.synchronize()
        for p in range(B):
            sl = slice(p * n_per, (p + 1) * n_per)
            c1, th1, td1 = new(n_per, 4), new(n_per, 6 * H), new(n_per, 6 * H)
            st1, k1 = new(n_per, dt=torch.int32), new(1, dt=torch.int64)
            e.rollout_cost_dp(xi[sl].contiguous(), MPCR_LAYOUT_XI, par[p].contiguous(), c1, theta=th1, thetadot=td1,
                              best_key=k1, index_base=ib, status=st1)
            torch.cuda.synchronize()
            assert torch.equal(c[sl].view(torch.int32), c1.view(torch.int32)), (model_name, p)
            assert torch.equal(th[sl], th1) and torch.equal(td[sl], td1), (model_name, p)
            assert torch.equal(st[sl], st1), (model_name, p)
            assert torch.equal(keys[p:p + 1], k1), (model_name, p, ib)
        assert torch.isfinite(c).all()
    return e


def test_rollout_narrow_equals_single_calls(torch_cuda):
    _rollout_multi_equals_slices(torch_cuda, "planner_scene", B=3, n_per=40, H=8, index_bases=(0, 1000))


def test_rollout_dual_arm_equals_single_calls(torch_cuda):
    _rollout_multi_equals_slices(torch_cuda, "dual_arm", B=2, n_per=24, H=8)


def test_rollout_dual_arm_segmented_groups_straddle_problems(torch_cuda):
    """The smallest batch the dual-arm engine runs as horizon segments over
    candidate groups (H = 8 is above the 7-step segment), with no group
    boundary on a problem boundary: a group's launch starts inside a problem."""
    from manipulator_mujoco_amd import basis, models
    from manipulator_mujoco_amd.engine import Engine
    B, H = 3, 8
    _, _, Pd, _ = basis.planner_basis(H, 0.05)
    probe = Engine(models.load("dual_arm", 0.05), H, B * 1024, Pd)  # (above the resident blocks: 8 per CU)
    lo, hi = 1, 1024
    assert probe.dispatches(B * lo) == 1 and probe.dispatches(B * hi) > 1
    while hi - lo > 1:  # (dispatches grow with the batch: one launch, then segments, then groups)
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
    assert probe.dispatches(B * n_per) >= 4 and straddles(n_per)  # >= 2 groups x 2 segments
    del probe
    _rollout_multi_equals_slices(torch_cuda, "dual_arm", B=B, n_per=n_per, H=H)


def _spd(torch, B, nv, dev):
    g = torch.Generator(device="cpu").manual_seed(3)
    a = torch.randn((B, nv, nv), generator=g)
    scale = torch.tensor([0.5, 2.0, 8.0])[:B].view(B, 1, 1)
    return ((a @ a.transpose(1, 2)) / nv * scale + scale * torch.eye(nv)).to(dev).contiguous()


@pytest.mark.parametrize("seed_step", [1, 0])
def test_factor_sample_project_equal_single_calls(torch_cuda, seed_step):
    torch = torch_cuda
    from manipulator_mujoco_amd import basis
    from manipulator_mujoco_amd.cem import CemContext
    dev = torch.device("cuda:0")
    B, n, H, nv, seed, counter = 3, 40, 16, 66, 77, 2
    _, P, Pd, Pdd = basis.planner_basis(H, 0.05)
    multi = CemContext(P, Pd, Pdd, 6, B * n, num_problems=B)
    single = CemContext(P, Pd, Pdd, 6, n)
    cov = _spd(torch, B, nv, dev)
    g = torch.Generator(device="cpu").manual_seed(4)
    mean = (0.2 * torch.randn((B, nv), generator=g)).to(dev)
    beq = torch.zeros((B, 6, 5))
    beq[:, :, 0] = torch.as_tensor(Q0, dtype=torch.float32) + 0.05 * torch.randn((B, 6), generator=g)
    beq[:, :, 1] = 0.1 * torch.randn((B, 6), generator=g)
    beq = beq.reshape(B, 30).to(dev).contiguous()
    xs, xf = torch.zeros((B, n, nv), device=dev), torch.zeros((B, n, nv), device=dev)
    multi.factor_multi(cov, 0.003)
    multi.sample_project_multi(B, n, mean, seed, counter, beq, 10, BOUNDS, seed_step=seed_step, xi_samples=xs, out=xf)
    torch.cuda.synchronize()
    for p in range(B):
        s1, f1 = torch.zeros((n, nv), device=dev), torch.zeros((n, nv), device=dev)
        single.factor(cov[p].contiguous(), 0.003)
        single.sample_project(n, mean[p].contiguous(), seed + p * seed_step, counter, beq[p].contiguous(), 10, BOUNDS,
                              xi_samples=s1, out=f1)
        torch.cuda.synchronize()
        assert torch.equal(xs[p], s1) and torch.equal(xf[p], f1), p
    assert torch.isfinite(xf).all()
    if seed_step == 0:  # shared draws: z is the same, mean and factor differ
        assert not torch.equal(xs[0], xs[1])


def _cost_cases(torch, B, n):
    """Costs with ties, +0 / -0, NaN and -inf, placed differently per problem."""
    g = torch.Generator(device="cpu").manual_seed(9)
    c = torch.randn((B, n), generator=g)
    for p in range(B):
        c[p, (p + 1) % n] = c[p, (p + 4) % n]          # a tie between two indices
        c[p, (2 * p + 2) % n] = 0.0
        c[p, (2 * p + 5) % n] = -0.0
        c[p, (3 * p) % n] = float("nan")
        c[p, (n - 1 - p) % n] = float("-inf")
        if n > 100:
            c[p, 100 + 7 * p:100 + 7 * p + 40] = -1.5  # a run of ties across the k-th place
    return c


@pytest.mark.parametrize("n,k", [(7, 3), (1000, 50)])
def test_topk_and_update_equal_single_calls(torch_cuda, n, k):
    torch = torch_cuda
    from manipulator_mujoco_amd import basis, models
    from manipulator_mujoco_amd.cem import CemContext, topk, topk_multi
    from manipulator_mujoco_amd.engine import Engine
    dev = torch.device("cuda:0")
    B, H, nv = 3, 8, 66
    _, P, Pd, Pdd = basis.planner_basis(H, 0.05)
    e = Engine(models.load("planner_scene", 0.05), H, B * n, Pd)
    ctx = CemContext(P, Pd, Pdd, 6, B * n, num_problems=B)
    c1 = _cost_cases(torch, B, n).to(dev).contiguous()
    c4 = torch.zeros((B, n, 4), device=dev)
    c4[:, :, 0] = c1
    g = torch.Generator(device="cpu").manual_seed(10)
    xi = torch.randn((B, n, nv), generator=g).to(dev)
    for cost, stride in ((c1, 1), (c4, 4)):
        idx = topk_multi(e, cost, B, k, stride=stride)
        torch.cuda.synchronize()
        assert idx.shape == (B, k)
        for p in range(B):
            ref = topk(e, cost[p].contiguous(), k, stride=stride)
            assert torch.equal(idx[p], ref), (p, stride)
            assert int(idx[p].max()) < n
        # update: those elites, distinct prior mean / cov per problem; a NaN
        # elite cost (n = 7 selects none, k < the finite count) stays out
        mean = (0.1 * torch.randn((B, nv), generator=g)).to(dev)
        cov = _spd(torch, B, nv, dev)
        m1, v1 = mean.clone(), cov.clone()
        ctx.update_multi(xi, cost, stride, idx, 10.0, 0.6, 0.6, mean, cov, reg=1e-4)
        torch.cuda.synchronize()
        for p in range(B):
            mp, vp = m1[p].clone(), v1[p].clone()
            ctx.update(xi[p].contiguous(), cost[p].contiguous(), stride, idx[p].contiguous(), 10.0, 0.6, 0.6, mp, vp,
                       reg=1e-4)
            torch.cuda.synchronize()
            assert torch.equal(mean[p].view(torch.int32), mp.view(torch.int32)), (p, stride)
            assert torch.equal(cov[p].view(torch.int32), vp.view(torch.int32)), (p, stride)


def test_multi_calls_validate_their_arguments(torch_cuda):
    torch = torch_cuda
    from manipulator_mujoco_amd import _lib, basis, models
    from manipulator_mujoco_amd.cem import CemContext, topk_multi
    from manipulator_mujoco_amd.engine import MPCR_LAYOUT_XI, Engine
    dev = torch.device("cuda:0")
    H = 8
    _, P, Pd, Pdd = basis.planner_basis(H, 0.05)
    e = Engine(models.load("planner_scene", 0.05), H, 16, Pd)
    z = lambda *s: torch.zeros(s, device=dev)  # noqa: E731
    with pytest.raises(_lib.MpcrError, match="max_n"):
        e.rollout_cost_multi(z(24, 66), MPCR_LAYOUT_XI, z(3, 20), 3, z(24, 4))
    with pytest.raises(_lib.MpcrError, match="k="):
        topk_multi(e, z(2, 8), 2, 9)
    ctx = CemContext(P, Pd, Pdd, 6, 16, num_problems=2)
    with pytest.raises(_lib.MpcrError, match="factor"):  # no factor call yet
        ctx.sample_project_multi(2, 8, z(2, 66), 1, 0, z(2, 30), 2, BOUNDS)
    ctx.factor(10.0 * torch.eye(66, device=dev), 0.003)  # covers one problem only
    with pytest.raises(_lib.MpcrError, match="factor"):
        ctx.sample_project_multi(2, 8, z(2, 66), 1, 0, z(2, 30), 2, BOUNDS)
    with pytest.raises(_lib.MpcrError, match="nprob"):
        ctx.factor_multi(z(3, 66, 66))
    with pytest.raises(_lib.MpcrError, match="k="):
        ctx.update_multi(z(2, 8, 66), z(2, 8), 1, torch.zeros((2, 9), dtype=torch.int32, device=dev), 10.0, 0.6, 0.6,
                         z(2, 66), z(2, 66, 66))


# ---------------------------------------------------------------------------
# whole planner ticks


def _planner(**kw):
    from manipulator_mujoco_amd.planner import cem_planner
    args = dict(num_dof=6, num_batch=64, num_steps=16, timestep=0.05, maxiter_cem=3, num_elite=0.05, w_pos=20.0,
                w_rot=3.0, w_col=80.0, maxiter_projection=10, verbose=False)
    args.update(kw)
    return cem_planner(**args)


def _batch_ticks(B):
    """Three ticks whose means, states, targets and weights change per problem."""
    rng = np.random.default_rng(2)
    for t in range(3):
        yield dict(xi_mean=rng.normal(0, 0.3 if t else 0.0, (B, 66)),
                   init_pos=Q0 + rng.uniform(-0.05, 0.05, (B, 6)),
                   init_vel=rng.uniform(-0.1, 0.1, (B, 6)) * (t > 0),
                   init_acc=rng.uniform(-0.1, 0.1, (B, 6)) * (t > 1),
                   target_pos=np.array([-0.3, -0.3, 0.5]) + rng.uniform(-0.1, 0.1, (B, 3)),
                   target_rot=np.array([[0.0, 1.0, 0.0, 0.0], [0.7071, 0.7071, 0.0, 0.0], [0.5, 0.5, 0.5, 0.5]])[:B],
                   weights=np.array([20.0, 3.0, 80.0]) + rng.uniform(0.0, 2.0, (B, 3)))


def _batch_equals_ordinary_planners(model_path, graph, seed=5):
    B = 3
    batch = _planner(model_path=model_path, num_problems=B, seed_step=1, seed=seed, graph=graph)
    singles = []
    for p in range(B):
        singles.append(_planner(model_path=model_path, seed=seed + p))
    for tick in _batch_ticks(B):
        out = batch.compute_cem_batch(**tick)
        assert len(out) == 9
        for p in range(B):
            sp = singles[p]
            w = tick["weights"][p].astype(np.float32)
            sp.cost_weights = {"w_pos": w[0], "w_rot": w[1], "w_col": w[2]}
            ref = sp.compute_cem(tick["xi_mean"][p], tick["init_pos"][p], tick["init_vel"][p], tick["init_acc"][p],
                                 tick["target_pos"][p], tick["target_rot"][p])
            for j in range(9):
                np.testing.assert_array_equal(np.asarray(out[j][p]), np.asarray(ref[j]), err_msg=f"entry {j} problem {p}")
    return batch


@pytest.mark.parametrize("graph", [False, True])
def test_planner_batch_equals_ordinary_planners(torch_cuda, graph):
    batch = _batch_equals_ordinary_planners(None, graph)
    if graph:
        assert batch._graphs is not None and len(batch._graphs) == 1  # one captured graph per tick
    with pytest.raises(ValueError, match="compute_cem_batch"):
        batch.compute_cem(np.zeros(66))


def test_planner_batch_dual_arm(torch_cuda):
    batch = _batch_equals_ordinary_planners("dual_arm", graph=True)
    assert batch._graphs is not None


def test_planner_batch_without_rollouts_and_one_problem(torch_cuda):
    """``return_rollouts=False`` leaves the two rollout entries None, and a
    planner of one problem serves both calls, replaying the one tick the
    first of them captured."""
    p = _planner(graph=True, return_rollouts=False, seed=3)
    tick = next(iter(_batch_ticks(1)))
    tick.pop("weights")
    out = p.compute_cem_batch(**tick)
    assert p._graphs is not None and len(p._graphs) == 1
    captured = p._graphs[0]
    ref = p.compute_cem(tick["xi_mean"][0], tick["init_pos"][0], tick["init_vel"][0], tick["init_acc"][0],
                        tick["target_pos"][0], tick["target_rot"][0])
    assert out[7] is None and out[8] is None and ref[7] is None
    for j in range(7):
        np.testing.assert_array_equal(np.asarray(out[j][0]), np.asarray(ref[j]))
    assert len(p._graphs) == 1 and p._graphs[0] is captured


# ---------------------------------------------------------------------------
# one problem through the multi-problem calls: nprob = 1 is the one-problem call


@pytest.mark.parametrize("model_name,n,index_bases", [("planner_scene", 40, (0, 1000)), ("dual_arm", 24, (0,))])
def test_rollout_one_problem_equals_the_one_problem_call(torch_cuda, model_name, n, index_bases):
    """``rollout_cost_multi(nprob=1)`` against ``rollout_cost_dp``: cost4 as
    bits, theta, thetadot, status and the key."""
    _rollout_multi_equals_slices(torch_cuda, model_name, B=1, n_per=n, H=8, index_bases=index_bases)


def test_distribution_stages_one_problem_equal_the_one_problem_calls(torch_cuda):
    """factor + sample_project, then topk + update, through the ``_multi``
    calls with nprob = 1 against the one-problem calls.  ``seed_step`` does
    not reach problem 0 and ``index_base`` offsets both alike."""
    torch = torch_cuda
    from manipulator_mujoco_amd import basis, models
    from manipulator_mujoco_amd.cem import CemContext, topk, topk_multi
    from manipulator_mujoco_amd.engine import Engine
    dev = torch.device("cuda:0")
    n, k, H, nv, seed, counter = 7, 3, 8, 66, 77, 2
    _, P, Pd, Pdd = basis.planner_basis(H, 0.05)
    e = Engine(models.load("planner_scene", 0.05), H, n, Pd)
    multi, single = CemContext(P, Pd, Pdd, 6, n), CemContext(P, Pd, Pdd, 6, n)
    cov = _spd(torch, 1, nv, dev)
    g = torch.Generator(device="cpu").manual_seed(4)
    mean = (0.2 * torch.randn((1, nv), generator=g)).to(dev)
    beq = torch.zeros((1, 6, 5))
    beq[:, :, 0] = torch.as_tensor(Q0, dtype=torch.float32) + 0.05 * torch.randn((1, 6), generator=g)
    beq[:, :, 1] = 0.1 * torch.randn((1, 6), generator=g)
    beq = beq.reshape(1, 30).to(dev).contiguous()
    xs, xf = torch.zeros((1, n, nv), device=dev), torch.zeros((1, n, nv), device=dev)
    s1, f1 = torch.zeros((n, nv), device=dev), torch.zeros((n, nv), device=dev)
    multi.factor_multi(cov, 0.003)
    multi.sample_project_multi(1, n, mean, seed, counter, beq, 10, BOUNDS, seed_step=5, xi_samples=xs, out=xf,
                               index_base=1000)
    single.factor(cov[0], 0.003)
    single.sample_project(n, mean[0], seed, counter, beq[0], 10, BOUNDS, xi_samples=s1, out=f1, index_base=1000)
    torch.cuda.synchronize()
    assert torch.equal(xs[0], s1) and torch.equal(xf[0], f1)
    assert torch.isfinite(xf).all()

    c1 = _cost_cases(torch, 1, n).to(dev).contiguous()
    c4 = torch.zeros((1, n, 4), device=dev)
    c4[:, :, 0] = c1
    for cost, stride in ((c1, 1), (c4, 4)):
        idx = topk_multi(e, cost, 1, k, stride=stride)
        ref = topk(e, cost[0], k, stride=stride)
        torch.cuda.synchronize()
        assert idx.shape == (1, k) and torch.equal(idx[0], ref), stride
        m, v = mean.clone(), cov.clone()
        m1, v1 = mean[0].clone(), cov[0].clone()
        multi.update_multi(xs, cost, stride, idx, 10.0, 0.6, 0.6, m, v, reg=1e-4)
        single.update(s1, cost[0], stride, ref, 10.0, 0.6, 0.6, m1, v1, reg=1e-4)
        torch.cuda.synchronize()
        assert torch.equal(m[0].view(torch.int32), m1.view(torch.int32)), stride
        assert torch.equal(v[0].view(torch.int32), v1.view(torch.int32)), stride
        assert not torch.equal(m, mean)


def test_planner_one_problem_shard_draws_from_index_base(torch_cuda):
    """A one-problem planner is its rank's shard of the batch: with a non-zero
    ``index_base`` (set as a second rank would have it) the tick's first
    samples are those the one-problem calls draw from that base, not the
    draws of a planner at base 0."""
    torch = torch_cuda
    base = 1000
    from manipulator_mujoco_amd.engine import MPCR_LAYOUT_XI
    # (one iteration: the buffers keep the samples drawn around the tick's input mean)
    shard, whole = _planner(seed=3, maxiter_cem=1), _planner(seed=3, maxiter_cem=1)
    shard.index_base = base
    tick = next(iter(_batch_ticks(1)))
    args = (tick["xi_mean"][0], tick["init_pos"][0], tick["init_vel"][0], tick["init_acc"][0], tick["target_pos"][0],
            tick["target_rot"][0])
    out = shard.compute_cem(*args)
    whole.compute_cem(*args)
    n, nv = whole.n_local, whole.nvar
    xs, xf = torch.zeros((n, nv), device=whole.device), torch.zeros((n, nv), device=whole.device)
    whole.cem.factor(whole._eye10, 0.003)
    whole.cem.sample_project(n, whole._mean_in, whole.seed, 0, whole._beq, whole.maxiter_projection, BOUNDS,
                             xi_samples=xs, out=xf, index_base=base)
    c4, key = torch.zeros((n, 4), device=whole.device), torch.zeros(1, dtype=torch.int64, device=whole.device)
    whole.engine.rollout_cost_dp(xf, MPCR_LAYOUT_XI, whole._par, c4, best_key=key, index_base=base)
    torch.cuda.synchronize()
    assert torch.equal(shard._xs, xs) and torch.equal(shard._xf, xf)
    assert not torch.equal(shard._xs, whole._xs)
    assert torch.equal(shard._costs[0].view(torch.int32), c4.view(torch.int32))
    assert torch.equal(shard._key, key) and (int(key.item()) & 0xFFFFFFFF) >= base
    assert np.isfinite(out[0]).all()
