"""The single-arm kernels read their launch arguments where they use them
(csrc/kernarg.h, KA / KSA: the kernarg segment, not registers held
across the horizon loop).  Such a read can go wrong only where an argument is
optional or offset, so every optional output is left out in turn, the best
key's index base is moved, and the same trajectories go in through the other
input layout -- on both single-arm models, at 5 candidates x 6 steps (per
problem), through three entries, with one wave per candidate forced and with
the default two waves (the threshold the MPCR_WPC2_MAX_N environment variable
initialises when the library loads, set here through mpcr_set_two_wave_max_n
as the other suites do: 0 forces one wave).

The instantiations these sizes select (rollout_kernel<16, 16, 24, false, WPC,
MULTI, STATE>):

  entry                                   one wave          two waves
  rollout_cost (parameters by value)      <1, false, false> <2, false, false>
  rollout_cost_state, start + final       <1, true, true>   <2, true, true>
  rollout_cost_multi, two problems        <1, true, false>  <2, true, false>

Everything is compared bit for bit against one call of the same entry with
every optional output requested.
"""
import contextlib

import numpy as np
import pytest

from manipulator_mujoco_amd import _lib, basis, models
from manipulator_mujoco_amd.engine import MPCR_LAYOUT_THETADOT, MPCR_LAYOUT_XI, Engine

pytestmark = pytest.mark.gpu

H, N_PER = 6, 5
Q0 = np.array([1.5, -1.8, 1.75, -1.25, -1.6, 0.0])
W = (20.0, 3.0, 80.0)
PT = (-0.3, -0.3, 0.5)
QT = (0.0, 1.0, 0.0, 0.0)
BASE = 1000
ENTRIES = ("cost", "state", "multi")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@contextlib.contextmanager
def _two_wave(on):
    lib = _lib.load()
    prev = lib.mpcr_set_two_wave_max_n(-1)
    try:
        lib.mpcr_set_two_wave_max_n(2048 if on else 0)
        yield
    finally:
        lib.mpcr_set_two_wave_max_n(prev)


_ENGINES = {}


def _engine(name):
    if name not in _ENGINES:
        m = models.load(name, 0.05)
        _, _, Pd, _ = basis.planner_basis(H, 0.05)
        _ENGINES[name] = Engine(m, H, 2 * N_PER, Pd)
    return _ENGINES[name]


class _Call:
    """One entry on one engine: run(**which outputs) -> dict of host arrays."""

    def __init__(self, torch, e, entry):
        self.torch, self.e, self.entry = torch, e, entry
        self.B = 2 if entry == "multi" else 1
        self.n = self.B * N_PER
        g = torch.Generator(device="cpu").manual_seed(5)
        self.xi = (0.3 * torch.randn((self.n, 66), generator=g)).cuda()
        rng = np.random.default_rng(11)
        blocks = [Engine.params(Q0 + rng.uniform(-0.1, 0.1, 6), (20.0 + 3 * p, 3.0 - 0.5 * p, 80.0 + 10 * p),
                                np.array(PT) + rng.uniform(-0.1, 0.1, 3), np.array(QT) + rng.uniform(-0.3, 0.3, 4))
                  for p in range(self.B)]
        self.par = torch.as_tensor(np.stack(blocks)).cuda()
        self.blk = e.state_layout()["size"]
        if entry == "state":
            # a start block off the template: every dof moving a little (the arm's are the controls' anyway)
            mc = e.model.compiled
            qvel = np.array(mc.qvel_init[:mc.nv], dtype=np.float64) + 0.01
            self.start = torch.as_tensor(e.pack_state(qvel=qvel)).cuda()

    def run(self, inp=None, layout=MPCR_LAYOUT_XI, theta=True, thetadot=True, status=True, index_base=0):
        torch, n = self.torch, self.n
        new = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device="cuda")  # noqa: E731
        out = {"cost4": new(n, 4), "keys": new(self.B, dt=torch.int64)}
        if theta:
            out["theta"] = new(n, 6 * H)
        if thetadot:
            out["thetadot"] = new(n, 6 * H)
        if status:
            out["status"] = new(n, dt=torch.int32)
        inp = self.xi if inp is None else inp
        kw = dict(theta=out.get("theta"), thetadot=out.get("thetadot"), status=out.get("status"), index_base=index_base)
        if self.entry == "cost":
            self.e.rollout_cost(inp, layout, Q0, W, PT, QT, cost4=out["cost4"], best_key=out["keys"], **kw)
        elif self.entry == "multi":
            self.e.rollout_cost_multi(inp, layout, self.par, self.B, out["cost4"], best_keys=out["keys"], **kw)
        else:
            out["final"] = new(n, self.blk)
            self.e.rollout_cost_state(inp, layout, self.par, 1, out["cost4"], start=self.start,
                                      final_state=out["final"], best_keys=out["keys"], **kw)
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in out.items()}


def _bits(a):
    return a.view(np.int32) if a.dtype == np.float32 else a


def _assert_same(full, other, what, skip=()):
    for k, v in other.items():
        if k in skip:
            continue
        assert np.array_equal(_bits(full[k]), _bits(v)), f"{what}: {k} differs"


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("two_wave", [False, True], ids=["one_wave", "two_wave"])
@pytest.mark.parametrize("name", ["scene_mjx", "ur5e_hande_mjx"])
def test_optional_and_offset_arguments(torch_cuda, name, two_wave, entry):
    c = _Call(torch_cuda, _engine(name), entry)
    with _two_wave(two_wave):
        full = c.run()
        assert np.isfinite(full["cost4"]).all() and (full["cost4"][:, 0] > 0).all()
        assert np.abs(full["theta"]).max() > 0 and np.abs(full["thetadot"]).max() > 0
        # each optional output left out in turn: the others are what they were
        for leave in ("theta", "thetadot", "status"):
            o = c.run(**{leave: False})
            assert leave not in o
            _assert_same(full, o, f"without {leave}")
        # a non-zero index base: the key's low word moves by it, nothing else does
        o = c.run(index_base=BASE)
        _assert_same(full, o, "index_base", skip=("keys",))
        kf, kb = full["keys"].astype(np.uint64), o["keys"].astype(np.uint64)
        assert np.array_equal(kf >> np.uint64(32), kb >> np.uint64(32)), "index_base: the key's cost word moved"
        lo_f, lo_b = kf & np.uint64(0xFFFFFFFF), kb & np.uint64(0xFFFFFFFF)
        assert np.array_equal(lo_f + np.uint64(BASE), lo_b), "index_base: the key's index word"
        assert (lo_f < np.uint64(N_PER)).all(), "the key's index is the index within the problem"
        # the same trajectories through the theta-dot layout (thetadot is then an output copy of the input)
        td = torch_cuda.as_tensor(full["thetadot"]).cuda()
        o = c.run(inp=td, layout=MPCR_LAYOUT_THETADOT)
        _assert_same(full, o, "theta-dot layout")
        o = c.run(inp=td, layout=MPCR_LAYOUT_THETADOT, thetadot=False)
        _assert_same(full, o, "theta-dot layout without thetadot")
