"""The multi-problem entry points of the C ABI without a GPU: exported,
bound by ``_lib`` and rejecting a null handle with MPCR_EINVAL and a message
(the header / ``EXPORTS`` agreement is tests/test_lib.py's)."""
import ctypes

import pytest

from manipulator_mujoco_amd import _lib

MULTI = ("mpcr_rollout_cost_multi", "mpcr_topk_multi", "mpcr_cem_set_problems", "mpcr_cem_factor_multi",
         "mpcr_cem_sample_project_multi", "mpcr_cem_update_multi")
F = _lib.MPCR_F_DEVICE_PTRS


def test_multi_symbols_are_exported_and_bound():
    lib = _lib.load()
    for name in MULTI:
        assert name in _lib.EXPORTS
        fn = getattr(lib, name)
        assert fn.argtypes is not None and fn.restype is ctypes.c_int, name
    assert lib.mpcr_abi_version() == 4  # backward-compatible additions: the version stays


def _null_handle_calls(lib):
    bounds = (ctypes.c_float * 3)(0.8, 1.8, 3.14)
    u64 = ctypes.c_uint64
    return {
        "mpcr_rollout_cost_multi": lambda: lib.mpcr_rollout_cost_multi(None, None, 0, 2, 4, None, None, None, None,
                                                                       None, 0, None, F, None),
        "mpcr_topk_multi": lambda: lib.mpcr_topk_multi(None, None, 1, 2, 4, 2, None, F, None),
        "mpcr_cem_set_problems": lambda: lib.mpcr_cem_set_problems(None, 2),
        "mpcr_cem_factor_multi": lambda: lib.mpcr_cem_factor_multi(None, None, 2, 0.003, F, None),
        "mpcr_cem_sample_project_multi": lambda: lib.mpcr_cem_sample_project_multi(
            None, 2, 4, None, u64(1), u64(1), u64(0), 0, None, None, None, 10, bounds, 1.0, None, F, None),
        "mpcr_cem_update_multi": lambda: lib.mpcr_cem_update_multi(None, None, 2, 4, None, 1, None, 2, 10.0, 0.6, 0.6,
                                                                   1e-4, None, None, F, None),
    }


@pytest.mark.parametrize("name", MULTI)
def test_null_handle_is_einval_with_a_message(name):
    lib = _lib.load()
    # a different failure first, so the message checked below is this call's
    assert lib.mpcr_model_from_blob(b"\0" * 16, 16, ctypes.byref(ctypes.c_void_p())) == -2
    before = lib.mpcr_last_error()
    assert _null_handle_calls(lib)[name]() == -1
    msg = lib.mpcr_last_error()
    assert msg and msg != before
