"""ctypes binding of libmpcr (include/mpcr.h).

The shared library is built in-tree by ``__graft_entry__.build()`` /
``python -m manipulator_mujoco_amd.build``.  There is deliberately no CPU
fallback: if the library or a gfx950 device is missing, every entry point
raises.
"""

from __future__ import annotations

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MPCR_LIB") or os.path.join(_HERE, "libmpcr.so")  # MPCR_LIB: A/B builds (tools/)

MPCR_LAYOUT_XI = 0
MPCR_LAYOUT_THETADOT = 1
MPCR_F_DEVICE_PTRS = 1
MPCR_F_RESET_BEST = 2
MPCR_F_SYNC = 4

_vp, _i, _d, _f, _u64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_float, ctypes.c_uint64
_P = ctypes.POINTER
# the argument types of every entry bound here, in include/mpcr.h's order
_ARGTYPES = {
    "mpcr_last_error": [],
    "mpcr_abi_version": [],
    "mpcr_device_arch": [_i, ctypes.c_char_p, _i],
    "mpcr_model_from_blob": [_vp, ctypes.c_size_t, _P(_vp)],
    "mpcr_model_load": [ctypes.c_char_p, _d, _P(_vp)],
    "mpcr_model_set_timestep": [_vp, _d],
    "mpcr_model_info": [_vp, _P(_i), _P(_i), _P(_i), _P(_i), _P(_i)],
    "mpcr_model_free": [_vp],
    "mpcr_engine_create": [_vp, _i, _i, _i, _vp, _i, _P(_vp)],
    "mpcr_engine_free": [_vp],
    "mpcr_rollout_cost": [_vp, _vp, _i, _i, _P(_d), _P(_f), _P(_f), _P(_f), _vp, _vp, _vp, _vp, _i, _vp, _i, _vp],
    "mpcr_argmin": [_vp, _vp, _i, _i, _i, _vp, _P(_i), _P(_f), _i, _vp],
    "mpcr_best_key_decode": [_u64, _P(_i), _P(_f)],
    "mpcr_topk": [_vp, _vp, _i, _i, _i, _vp, _i, _vp],
    "mpcr_cem_create": [_i, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _P(_vp)],
    "mpcr_cem_free": [_vp],
    "mpcr_cem_factor": [_vp, _vp, _f, _i, _vp],
    "mpcr_cem_sample_project": [_vp, _i, _vp, _u64, _u64, _i, _vp, _vp, _vp, _i, _i, _P(_f), _f, _vp, _i, _vp],
    "mpcr_project": [_vp, _vp, _vp, _i, _i, _i, _P(_f), _f, _vp, _i, _vp],
    "mpcr_cem_update": [_vp, _vp, _i, _vp, _i, _vp, _i, _f, _f, _f, _f, _vp, _vp, _i, _vp],
    "mpcr_rollout_cost_dp": [_vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _i, _vp],
    "mpcr_plant_create": [_vp, _i, _P(_vp)],
    "mpcr_plant_free": [_vp],
    "mpcr_plant_set_state": [_vp, _P(_d), _P(_d), _P(_d)],
    "mpcr_plant_get_state": [_vp, _P(_d), _P(_d), _P(_d), _P(_d)],
    "mpcr_plant_step": [_vp, _P(_d), _i, _vp],
    "mpcr_rollout_occupancy": [_i, _P(_i)],
    "mpcr_set_two_wave_max_n": [_i],
    "mpcr_engine_dispatches": [_vp, _i, _P(_i)],
    "mpcr_comm_unique_id": [ctypes.c_char_p],
    "mpcr_comm_init": [_i, _i, ctypes.c_char_p, _i, _P(_vp)],
    "mpcr_comm_free": [_vp],
    "mpcr_comm_allreduce_key": [_vp, _vp, _i, _vp],
    "mpcr_comm_allgather": [_vp, _vp, _vp, ctypes.c_size_t, _vp],
    "mpcr_comm_gather_elites": [_vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp],
    "mpcr_model_hull_starts": [_vp, _i, _P(ctypes.c_int32), _P(ctypes.c_int32), _P(ctypes.c_uint8), ctypes.c_int64],
    "mpcr_set_hull_start_scramble": [_u64],
    # several problems in one call
    "mpcr_rollout_cost_multi": [_vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _i, _vp],
    "mpcr_topk_multi": [_vp, _vp, _i, _i, _i, _i, _vp, _i, _vp],
    "mpcr_cem_set_problems": [_vp, _i],
    "mpcr_cem_factor_multi": [_vp, _vp, _i, _f, _i, _vp],
    "mpcr_cem_sample_project_multi": [_vp, _i, _i, _vp, _u64, _u64, _u64, _i, _vp, _vp, _vp, _i, _P(_f), _f, _vp, _i,
                                      _vp],
    "mpcr_cem_update_multi": [_vp, _vp, _i, _i, _vp, _i, _vp, _i, _f, _f, _f, _f, _vp, _vp, _i, _vp],
    # planning from a state
    "mpcr_state_layout": [_P(_i), _P(_i), _P(_i), _P(_i), _P(_i)],
    "mpcr_rollout_cost_state": [_vp, _vp, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _i, _vp],
    "mpcr_plant_copy_state": [_vp, _vp, _vp],
    # actuator controls as a call input
    "mpcr_rollout_cost_ctrl": [_vp, _vp, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _i, _vp, _i,
                               _vp],
    "mpcr_plant_set_ctrl": [_vp, _P(_d)],
    "mpcr_model_actuators": [_vp, _P(_i), _P(_d), _P(_i)],
    # static geom poses as a call input
    "mpcr_rollout_cost_world": [_vp, _vp, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _i, _i, _vp, _i, _i, _vp, _vp, _vp, _vp,
                                _i, _vp, _i, _vp],
    "mpcr_plant_set_geom_poses": [_vp, _P(_f)],
    "mpcr_model_geom_poses": [_vp, _P(_i), _P(_f), _P(_i), _P(_i)],
    # the wave-reduction self-test
    "mpcr_selftest_reduce": [_i, _vp, _i, _vp],
    # scenarios (one set of candidates, several worlds)
    "mpcr_rollout_cost_scenarios": [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _i, _i, _vp, _i, _i, _vp,
                                    _vp, _vp, _vp, _vp, _i, _vp, _i, _vp],
    "mpcr_scenario_reduce": [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _i, _i, _vp],
    # target poses as a call input
    "mpcr_rollout_cost_target": [_vp, _vp, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _i, _i, _vp, _i, _i, _vp, _i, _i, _vp,
                                 _vp, _vp, _vp, _i, _vp, _i, _vp],
    "mpcr_rollout_cost_scenarios_target": [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _i, _i, _vp, _i, _i,
                                           _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _i, _vp],
    # collision-cost weights per contact slot as a call input
    "mpcr_rollout_cost_slotw": [_vp, _vp, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _i, _i, _vp, _i, _i, _vp, _i, _i, _vp,
                                _i, _vp, _vp, _vp, _vp, _i, _vp, _i, _vp],
    "mpcr_rollout_cost_scenarios_slotw": [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _i, _i, _vp, _i, _i,
                                          _vp, _i, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _i, _vp],
    "mpcr_model_slots": [_vp, _P(_i), _P(_i), _P(_i), _P(_i)],
    # cost weights per step as a call input
    "mpcr_rollout_cost_stepw": [_vp, _vp, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _i, _i, _vp, _i, _i, _vp, _i, _i, _vp,
                                _i, _vp, _i, _vp, _vp, _vp, _vp, _i, _vp, _i, _vp],
    "mpcr_rollout_cost_scenarios_stepw": [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _i, _i, _vp, _i, _i,
                                          _vp, _i, _i, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _i, _vp],
}
# every symbol include/mpcr.h declares (tests check the exports)
EXPORTS = tuple(_ARGTYPES)
# debug / parity entries, outside the stable ABI surface
_ARGTYPES.update({
    "mpcr_rollout_trace": [_vp, _vp, _i, _i, _P(_d), _P(_f), _P(_f), _P(_f), _vp, _vp, _vp, _vp],
    "mpcr_plant_step_debug": [_vp, _P(_d), _vp, _i],
    "mpcr_plant_dbg_size": [],
})
# what an entry returns, where it is not the int status
_VOID = ("mpcr_model_free", "mpcr_engine_free", "mpcr_best_key_decode", "mpcr_cem_free", "mpcr_plant_free",
         "mpcr_comm_free")
_RESTYPE = {"mpcr_last_error": ctypes.c_char_p, "mpcr_model_hull_starts": ctypes.c_int64,
            "mpcr_set_hull_start_scramble": _u64, **dict.fromkeys(_VOID)}

_lib = None


class MpcrError(RuntimeError):
    pass


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MpcrError(f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'`")
    # torch's HIP runtime first: torch links an unversioned libamdhip64.so of
    # its own, libmpcr the system's libamdhip64.so.7 (the same SONAME).  Loaded
    # in this order libmpcr binds to torch's copy; the other way round the
    # process holds two HIP runtimes and libmpcr's finds no device.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = ctypes.CDLL(LIB_PATH)
    # an entry this library does not export stays unbound: a library built
    # before it (MPCR_LIB, A/B runs against an older build) still loads, and
    # calling the entry there raises AttributeError
    for name, argtypes in _ARGTYPES.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.argtypes, fn.restype = argtypes, _RESTYPE.get(name, ctypes.c_int)
    _lib = lib
    return lib


def check(rc: int):
    if rc != 0:
        msg = load().mpcr_last_error().decode(errors="replace")
        raise MpcrError(f"libmpcr error {rc}: {msg}")


def decode_key(key: int):
    idx = ctypes.c_int()
    val = ctypes.c_float()
    load().mpcr_best_key_decode(ctypes.c_uint64(key), ctypes.byref(idx), ctypes.byref(val))
    return idx.value, val.value
