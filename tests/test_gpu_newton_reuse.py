"""Newton's first iteration takes M qacc, the Gauss term and the cost from the
warm-start choice that just computed them (csrc/rollout.hip).  An engine
created with MPCR_NEWTON_REUSE=0 recomputes them as before; both must give the
same bits on every single-arm scene and kernel variant."""
import os

import numpy as np
import pytest

from manipulator_mujoco_amd import _lib, basis, models
from manipulator_mujoco_amd.engine import Engine
from test_gpu_step_table import run, sine_thetadot

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def engine(name, H, n, reuse):
    """An engine with the reuse on (the default) or off; the variable is read
    when the engine is created."""
    _, _, Pd, _ = basis.planner_basis(H, 0.05)
    prev = os.environ.pop("MPCR_NEWTON_REUSE", None)
    try:
        if not reuse:
            os.environ["MPCR_NEWTON_REUSE"] = "0"
        return Engine(models.load(name, 0.05), H, n, Pd)
    finally:
        os.environ.pop("MPCR_NEWTON_REUSE", None)
        if prev is not None:
            os.environ["MPCR_NEWTON_REUSE"] = prev


def both(name, n, H, seed):
    td = sine_thetadot(n, H, 0.05, seed)
    off = run(engine(name, H, n, False), td)
    on = run(engine(name, H, n, True), td)
    for a, b in zip(on, off):
        np.testing.assert_array_equal(a, b)
    return on


def max_rows(status):
    return (status >> 2) & 0xFF


@pytest.mark.parametrize("name,n", [("scene_mjx", 64), ("planner_scene", 64), ("ur5e_hande_mjx", 64),
                                    ("hande_scene", 16)])
def test_reuse_is_bitwise(torch_cuda, name, n):
    """Two-wave kernel (the default for these batch sizes).  hande_scene runs
    100 Newton iterations: the reuse is in the first only."""
    c4, theta, st = both(name, n, 20, 41)
    print(f"{name}: most rows in one step {max_rows(st).max()}, fewest {max_rows(st).min()}")
    assert np.isfinite(c4).all()
    if name == "scene_mjx":
        # the drive reaches the table and the box: both warm-start outcomes,
        # and steps with more rows than the one-wave image keeps in LDS
        assert max_rows(st).max() > 40, max_rows(st).max()


@pytest.mark.parametrize("two_wave", [True, False])
def test_reuse_is_bitwise_on_each_kernel(torch_cuda, two_wave):
    """scene_mjx on the two-wave kernel and on the forced one-wave kernel (J
    rows past 40 in the HBM slab)."""
    lib = _lib.load()
    prev = lib.mpcr_set_two_wave_max_n(-1)
    try:
        lib.mpcr_set_two_wave_max_n(2048 if two_wave else 0)
        _, _, st = both("scene_mjx", 64, 20, 41)
    finally:
        lib.mpcr_set_two_wave_max_n(prev)
    assert max_rows(st).max() > 40, max_rows(st).max()


def test_reuse_is_bitwise_on_a_ragged_batch(torch_cuda):
    both("scene_mjx", 65, 3, 47)
