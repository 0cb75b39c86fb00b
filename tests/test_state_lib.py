"""Planning from a state, the parts that need no GPU: the three C entry points
are exported and bound, the state-block layout, a null handle is MPCR_EINVAL
with a message, and ``pack_state`` / ``unpack_state`` round-trip a state and
fill what is left out from the model's template."""
import ctypes

import numpy as np
import pytest

from manipulator_mujoco_amd import _lib, models
from manipulator_mujoco_amd.engine import Engine, pack_state, state_layout, unpack_state

STATE = ("mpcr_state_layout", "mpcr_rollout_cost_state", "mpcr_plant_copy_state")
F = _lib.MPCR_F_DEVICE_PTRS


def test_state_symbols_are_exported_and_bound():
    lib = _lib.load()
    for name in STATE:
        assert name in _lib.EXPORTS
        fn = getattr(lib, name)
        assert fn.argtypes is not None and fn.restype is ctypes.c_int, name
    assert lib.mpcr_abi_version() == 4  # backward-compatible additions: the version stays


def test_state_layout_is_ascending_and_ends_with_eef():
    lib = _lib.load()
    o = [ctypes.c_int(-1) for _ in range(5)]
    size = lib.mpcr_state_layout(*(ctypes.byref(x) for x in o))
    off = [x.value for x in o]
    assert off[0] == 0 and off == sorted(set(off))
    assert size == off[4] + 8
    assert lib.mpcr_state_layout(None, None, None, None, None) == size  # every part is optional
    lay = state_layout()
    assert [lay[k] for k in ("qpos", "qvel", "qacc_warmstart", "qacc", "eef")] == off and lay["size"] == size
    assert Engine.state_layout() == lay
    # room for the largest bundled model
    m = models.load("dual_arm", 0.05)
    assert lay["qvel"] - lay["qpos"] >= m.nq and lay["qacc_warmstart"] - lay["qvel"] >= m.nv


@pytest.mark.parametrize("name", ["mpcr_rollout_cost_state", "mpcr_plant_copy_state"])
def test_null_handle_is_einval_with_a_message(name):
    lib = _lib.load()
    calls = {
        "mpcr_rollout_cost_state": lambda: lib.mpcr_rollout_cost_state(None, None, 0, 2, 4, None, None, 0, None, None,
                                                                       None, None, None, 0, None, F, None),
        "mpcr_plant_copy_state": lambda: lib.mpcr_plant_copy_state(None, None, None),
    }
    # a different failure first, so the message checked below is this call's
    assert lib.mpcr_model_from_blob(b"\0" * 16, 16, ctypes.byref(ctypes.c_void_p())) == -2
    before = lib.mpcr_last_error()
    assert calls[name]() == -1
    msg = lib.mpcr_last_error()
    assert msg and msg != before


@pytest.mark.parametrize("name", ["scene_mjx", "dual_arm"])
def test_pack_state_round_trips_and_fills_from_the_template(name):
    m = models.load(name, 0.05)
    lay = state_layout()
    rng = np.random.default_rng(4)
    qpos, qvel, qws = (rng.uniform(-1, 1, k).astype(np.float32) for k in (m.nq, m.nv, m.nv))
    blk = pack_state(m, qpos, qvel, qws)
    assert blk.dtype == np.float32 and blk.shape == (lay["size"],)
    parts = unpack_state(m, blk)
    np.testing.assert_array_equal(parts["qpos"], qpos)
    np.testing.assert_array_equal(parts["qvel"], qvel)
    np.testing.assert_array_equal(parts["qacc_warmstart"], qws)
    # nothing outside the three parts: padding, qacc and eef stay 0
    used = np.zeros(lay["size"], bool)
    for k, n in (("qpos", m.nq), ("qvel", m.nv), ("qacc_warmstart", m.nv)):
        used[lay[k]:lay[k] + n] = True
    assert not blk[~used].any()
    # parts left out come from the template state: qpos_init, qvel_init, a zero warm start
    tpl = unpack_state(m, pack_state(m))
    np.testing.assert_array_equal(tpl["qpos"], np.asarray(m.qpos_init[:m.nq], dtype=np.float32))
    np.testing.assert_array_equal(tpl["qvel"], np.asarray(m.qvel_init[:m.nv], dtype=np.float32))
    assert not tpl["qacc_warmstart"].any()
    only_v = unpack_state(m, pack_state(m, qvel=qvel))
    np.testing.assert_array_equal(only_v["qpos"], tpl["qpos"])
    np.testing.assert_array_equal(only_v["qvel"], qvel)
    with pytest.raises(ValueError, match="qpos"):
        pack_state(m, qpos=qpos[:-1])
    # stacked blocks unpack along the last axis
    both = unpack_state(m, np.stack([blk, pack_state(m)]))
    assert both["qpos"].shape == (2, m.nq) and both["eef"].shape == (2, 7)
