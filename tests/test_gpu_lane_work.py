"""The single-arm step's lane work (csrc/rollout.hip, MPCR_LANE_WORK): the pose
cost's transcendental tail deferred and spread over lanes, the trees' centres
of mass in one reduction, Newton's first rows from the warm-start choice and
the line search's q0 at alpha = 0 from Newton's cost.  An engine created with MPCR_LANE_WORK=0 runs the former step; both must
give the same bits -- costs, theta, thetadot, status and final states -- on
every single-arm scene and kernel variant.

The candidates are rows of the bench's draw (bench.synthetic_xi(4096, H, seed
20250632)), chosen on the CPU with the fp64 oracle (oracle.rollout's slot
distances and maxrows).  At H = 70 (past the 64-step flush of the pose cost)
each batch of 64 holds steps in which a robot pair emits a contact and steps in
which none does, and candidates whose busiest step has at most 32 constraint
rows and candidates with more; the tests assert that on the engine's own
outputs.  At H = 8 the arm reaches nothing from the bench's start pose: no
bundled single-arm scene has a contact or more than 18 rows there (the oracle:
18 / 16 / 2 rows in every step); the tests assert that too.

scene_mjx and planner_scene have two kinematic trees, ur5e_hande_mjx one (the
centres of mass); more than four trees take the former loop (a static check)."""
import os
import re

import numpy as np
import pytest

import parity_util as pu
from manipulator_mujoco_amd import _lib, basis, models
from manipulator_mujoco_amd.engine import MPCR_LAYOUT_XI, Engine, pack_state
from test_gpu_narrow_on_demand import slot_margins

pytestmark = pytest.mark.gpu

Q0, W, PT, QT = pu.Q0, pu.W, pu.PT, pu.QT
N = 64
# rows of the draw at H = 70 (H = 8: the first 64)
ROWS70 = {
    "scene_mjx": np.concatenate([np.arange(46), [96, 146, 155, 291, 403, 473, 501, 530, 634, 668, 696, 724, 733, 798,
                                                 815, 817, 876, 928]]),
    "planner_scene": np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24,
                               25, 26, 29, 32, 38, 39, 46, 50, 55, 56, 57, 58, 59, 61, 62, 64, 65, 66, 72, 75, 80, 83, 84,
                               86, 92, 93, 94, 100, 106, 108, 109, 115, 129, 138, 141, 146, 148, 155, 156]),
    "ur5e_hande_mjx": np.arange(64),
}
NAMES = sorted(ROWS70)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def draws():
    """H -> the bench's 4096 x 66 draw, once."""
    import bench
    return {H: bench.synthetic_xi(4096, H, 20250629 + 3).numpy() for H in (8, 70)}


def batch(draws, name, H):
    rows = ROWS70[name] if H == 70 else np.arange(N)
    assert rows.size == N and np.unique(rows).size == N
    return np.ascontiguousarray(draws[H][rows], dtype=np.float32)


def engine(m, H, n, lane_work):
    """An engine with the lane work (the default) or the former step; the
    variable is read when the engine is created."""
    _, _, Pd, _ = basis.planner_basis(H, 0.05)
    prev = os.environ.pop("MPCR_LANE_WORK", None)
    try:
        if not lane_work:
            os.environ["MPCR_LANE_WORK"] = "0"
        return Engine(m, H, n, Pd)
    finally:
        os.environ.pop("MPCR_LANE_WORK", None)
        if prev is not None:
            os.environ["MPCR_LANE_WORK"] = prev


def run(torch, e, inp, nprob=1, start=None, final=False, params=None):
    n, H = inp.shape[0], e.H
    c4 = torch.zeros((n, 4), device="cuda")
    theta, thetadot = torch.zeros((n, 6 * H), device="cuda"), torch.zeros((n, 6 * H), device="cuda")
    status = torch.zeros(n, dtype=torch.int32, device="cuda")
    fin = torch.zeros((n, e.state_layout()["size"]), device="cuda") if final else None
    if params is None:
        params = np.tile(Engine.params(Q0, W, PT, QT), (nprob, 1))
    par = torch.as_tensor(np.ascontiguousarray(params, dtype=np.float32)).cuda()
    x = torch.as_tensor(inp).cuda()
    if start is None and not final:
        e.rollout_cost_multi(x, MPCR_LAYOUT_XI, par, nprob, c4, theta=theta, thetadot=thetadot, status=status)
    else:
        e.rollout_cost_state(x, MPCR_LAYOUT_XI, par, nprob, c4, start=start, final_state=fin, theta=theta,
                             thetadot=thetadot, status=status)
    torch.cuda.synchronize()
    out = {"cost4": c4.cpu().numpy(), "theta": theta.cpu().numpy(), "thetadot": thetadot.cpu().numpy(),
           "status": status.cpu().numpy()}
    if final:
        out["final_state"] = fin.cpu().numpy()
    return out


def same_bits(a, b):
    assert a.keys() == b.keys()
    for k in a:
        np.testing.assert_array_equal(a[k].view(np.int32), b[k].view(np.int32), err_msg=k)
    assert np.isfinite(a["cost4"]).all()


def both(torch, m, inp, H, two_wave, **kw):
    lib = _lib.load()
    prev = lib.mpcr_set_two_wave_max_n(-1)
    try:
        lib.mpcr_set_two_wave_max_n(2048 if two_wave else 0)
        on_e = engine(m, H, inp.shape[0], True)
        on = run(torch, on_e, inp, **kw)
        off = run(torch, engine(m, H, inp.shape[0], False), inp, **kw)
    finally:
        lib.mpcr_set_two_wave_max_n(prev)
    same_bits(on, off)
    return on, on_e


def max_rows(status):
    return (status >> 2) & 0xFF


@pytest.mark.parametrize("two_wave", [False, True], ids=["one_wave", "two_wave"])
@pytest.mark.parametrize("H", [8, 70])
@pytest.mark.parametrize("name", NAMES)
def test_lane_work_is_bitwise(torch_cuda, draws, name, H, two_wave):
    m = models.load(name, 0.05)
    inp = batch(draws, name, H)
    on, e = both(torch_cuda, m, inp, H, two_wave)
    mr = max_rows(on["status"])
    assert (mr > 0).all()  # every candidate runs the Newton solve
    slots = e.trace(inp, MPCR_LAYOUT_XI, Q0, W, PT, QT)["slots"]
    emits = (slots < slot_margins(m)).any(axis=2)  # (candidate, step): some robot pair emits a contact
    if H == 8:  # the arm reaches nothing yet: no contact, the rows of the resting scene
        assert not emits.any(), int(emits.sum())
        assert (mr <= 32).all(), mr.max()
        return
    print(f"{name} H={H}: {int(emits.sum())} of {emits.size} candidate-steps emit a robot contact; busiest step's rows "
          f"min {mr.min()} max {mr.max()}, {int((mr <= 32).sum())} candidates <= 32, {int((mr > 32).sum())} above")
    # both classes of step, and solves with few and with many rows
    assert emits.any() and not emits.all(), (int(emits.sum()), emits.size)
    assert (mr <= 32).any() and (mr > 32).any(), (mr.min(), mr.max())


def test_final_states_are_bitwise(torch_cuda, draws):
    """rollout_cost_state without a start block: the final states too."""
    on, _ = both(torch_cuda, models.load("scene_mjx", 0.05), batch(draws, "scene_mjx", 70), 70, False, final=True)
    assert np.abs(on["final_state"]).max() > 0


def test_multi_call_is_bitwise(torch_cuda, draws):
    """One MULTI call, 2 problems x 32 with their own targets."""
    par = np.stack([Engine.params(Q0, W, PT, QT), Engine.params(Q0, W, (-0.2, 0.35, 0.45), QT)])
    on, _ = both(torch_cuda, models.load("scene_mjx", 0.05), batch(draws, "scene_mjx", 70), 70, False, nprob=2,
                 params=par)
    assert not np.array_equal(on["cost4"][:32, 1], on["cost4"][32:, 1])


@pytest.mark.parametrize("two_wave", [False, True], ids=["one_wave", "two_wave"])
def test_state_call_is_bitwise(torch_cuda, draws, two_wave):
    """One STATE call: a start block (the template state with the object moved
    3 cm and a warm start given) and the final states."""
    m = models.load("planner_scene", 0.05)
    inp = batch(draws, "planner_scene", 70)
    arm = set(int(a) for a in m.ctrl_qposadr[:6])
    obj = [i for i in range(int(m.nq)) if i not in arm][:3]  # the free joint's position
    qpos = np.array(m.qpos_init[:int(m.nq)], dtype=np.float64)
    qpos[obj[0]] += 0.03
    start = torch_cuda.as_tensor(pack_state(m, qpos=qpos, qacc_warmstart=0.5 * np.ones(int(m.nv)))).cuda()
    on, _ = both(torch_cuda, m, inp, 70, two_wave, start=start, final=True)
    plain, _ = both(torch_cuda, m, inp, 70, two_wave, final=True)
    assert not np.array_equal(on["final_state"], plain["final_state"])  # the start block was used


def test_more_than_four_trees_keep_the_loop():
    """The one-reduction centres of mass hold a tree per 16-lane row: the
    kernel takes them only for ntree <= WAVE / 16 and NBW == 16 (source check;
    no bundled model has five trees)."""
    src = open(os.path.join(os.path.dirname(_lib.__file__), "csrc", "rollout.hip")).read()
    cond = re.search(r"if constexpr \(LW_COM && NBW == 16\)\s*\n\s*com_rows = (.*);", src)
    assert cond, "the centre-of-mass condition moved"
    assert "m->ntree <= WAVE / 16" in cond.group(1) and "DEV_NO_LANE_WORK" in cond.group(1)
    assert re.search(r"for \(int tr = 0; tr < m->ntree; tr\+\+\) \{.*?if \(com_rows\) break;", src, re.S)
    for name in NAMES:
        assert int(models.load(name, 0.05).ntree) in (1, 2)
    assert {int(models.load(n, 0.05).ntree) for n in NAMES} == {1, 2}
