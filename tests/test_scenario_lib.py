"""Scenarios (one set of candidates priced in several worlds), the parts that
need no GPU: the two C entry points are exported and bound and refuse a null
handle, ``cem_planner`` checks ``num_scenarios`` / ``scenario_worst`` before it
touches a device, and ``scenario_reduce_np`` -- the numpy statement of
``mpcr_scenario_reduce`` that tests/test_gpu_scenarios.py holds the kernel to,
bit for bit -- has the properties the fold is defined by."""
import ctypes

import numpy as np
import pytest

from manipulator_mujoco_amd import _lib

SCEN = ("mpcr_rollout_cost_scenarios", "mpcr_scenario_reduce")
F = _lib.MPCR_F_DEVICE_PTRS


def scenario_reduce_np(cost4_scen, nprob, nscen, n_per, worst):
    """``mpcr_scenario_reduce`` in numpy: rows (p nscen + s) n_per + i of
    cost4_scen -> (nprob n_per, 4).  Per candidate the ``worst`` rows with the
    largest total are selected (NaN above everything, then descending, -0 ==
    +0, ties to the lower scenario); each column is their fp32 sum, taken in
    ascending scenario order one row after the other from the first, divided
    by float32(worst)."""
    cs = np.asarray(cost4_scen, dtype=np.float32).reshape(nprob, nscen, n_per, 4)
    out = np.empty((nprob, n_per, 4), dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for p in range(nprob):
            for i in range(n_per):
                tot = cs[p, :, i, 0]
                # (-0.0 == 0.0 in the comparison of the keys, so the index breaks that tie)
                order = sorted(range(nscen), key=lambda s: (0, 0.0, s) if np.isnan(tot[s]) else (1, -float(tot[s]), s))
                sel = sorted(order[:worst])
                acc = cs[p, sel[0], i].copy()
                for s in sel[1:]:
                    acc = (acc + cs[p, s, i]).astype(np.float32)
                out[p, i] = acc / np.float32(worst)
    return out.reshape(nprob * n_per, 4)


def pack_key_np(total, index_base=0):
    """The packed argmin key of a float32 column (``mpcr_best_key_decode``'s
    inverse): NaN first, then ascending, the low word the first index."""
    best = 0xFFFFFFFFFFFFFFFF
    for i, c in enumerate(np.asarray(total, dtype=np.float32)):
        u = int(np.float32(c).view(np.uint32))
        k = 0 if np.isnan(c) else ((~u & 0xFFFFFFFF) if u & 0x80000000 else (u | 0x80000000))
        best = min(best, (k << 32) | ((index_base + i) & 0xFFFFFFFF))
    return best


def test_scenario_symbols_are_exported_and_bound():
    lib = _lib.load()
    for name in SCEN:
        assert name in _lib.EXPORTS
        fn = getattr(lib, name)
        assert fn.argtypes is not None and fn.restype is ctypes.c_int, name
    assert len(lib.mpcr_rollout_cost_scenarios.argtypes) == 26 and len(lib.mpcr_scenario_reduce.argtypes) == 11
    assert lib.mpcr_abi_version() == 4  # a backward-compatible addition: the version stays


@pytest.mark.parametrize("name", SCEN)
def test_null_handle_is_einval_with_a_message(name):
    lib = _lib.load()
    calls = {
        "mpcr_rollout_cost_scenarios": lambda: lib.mpcr_rollout_cost_scenarios(
            None, None, 0, 2, 3, 3, 4, None, None, 0, None, None, 0, 0, None, 0, 0, None, None, None, None, None, 0, None,
            F, None),
        "mpcr_scenario_reduce": lambda: lib.mpcr_scenario_reduce(None, None, 2, 3, 4, 3, None, None, 0, F, None),
    }
    # a different failure first, so the message checked below is this call's
    assert lib.mpcr_model_from_blob(b"\0" * 16, 16, ctypes.byref(ctypes.c_void_p())) == -2
    before = lib.mpcr_last_error()
    assert calls[name]() == -1
    msg = lib.mpcr_last_error()
    assert msg and msg != before


@pytest.mark.parametrize("kw,match", [(dict(num_scenarios=0), "num_scenarios"), (dict(num_scenarios=65), "num_scenarios"),
                                      (dict(num_scenarios=3, scenario_worst=0), "scenario_worst"),
                                      (dict(num_scenarios=3, scenario_worst=4), "scenario_worst"),
                                      (dict(scenario_worst=2), "scenario_worst")])
def test_planner_checks_its_scenario_arguments_first(kw, match):
    from manipulator_mujoco_amd.planner import cem_planner
    with pytest.raises(ValueError, match=match):
        cem_planner(num_dof=6, num_batch=64, num_steps=12, timestep=0.05, maxiter_cem=2, num_elite=0.05, w_pos=20.0,
                    w_rot=3.0, w_col=80.0, maxiter_projection=10, verbose=False, **kw)


def _rows(rng, nprob, nscen, n_per):
    return rng.uniform(0.5, 40.0, (nprob * nscen * n_per, 4)).astype(np.float32)


def test_reference_all_scenarios_is_the_sequential_fp32_mean():
    rng = np.random.default_rng(0)
    B, S, n = 2, 5, 7
    cs = _rows(rng, B, S, n)
    got = scenario_reduce_np(cs, B, S, n, S).reshape(B, n, 4)
    c = cs.reshape(B, S, n, 4)
    acc = c[:, 0].copy()
    for s in range(1, S):
        acc = acc + c[:, s]
    assert acc.dtype == np.float32
    np.testing.assert_array_equal(got, acc / np.float32(S))
    # close to, and for some entries other than, the fp64 mean rounded once: the order is part of the definition
    exact = c.astype(np.float64).mean(axis=1)
    np.testing.assert_allclose(got, exact, rtol=4e-7)


def test_reference_one_is_the_worst_row_itself():
    rng = np.random.default_rng(1)
    B, S, n = 3, 4, 9
    cs = _rows(rng, B, S, n)
    got = scenario_reduce_np(cs, B, S, n, 1).reshape(B, n, 4)
    c = cs.reshape(B, S, n, 4)
    w = c[..., 0].argmax(axis=1)  # (first index of the maximum)
    for p in range(B):
        for i in range(n):
            np.testing.assert_array_equal(got[p, i].view(np.int32), c[p, w[p, i], i].view(np.int32))


def test_reference_selects_a_nan_row_first_and_breaks_zero_ties_by_index():
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    # one candidate, four scenarios: totals 3, NaN, +inf, 7
    cs = np.array([[3, 1, 1, 1], [nan, 2, 2, 2], [inf, 3, 3, 3], [7, 4, 4, 4]], dtype=np.float32)
    one = scenario_reduce_np(cs, 1, 4, 1, 1)[0]
    assert np.isnan(one[0]) and tuple(one[1:]) == (2, 2, 2)  # NaN above +inf
    two = scenario_reduce_np(cs, 1, 4, 1, 2)[0]
    assert np.isnan(two[0]) and tuple(two[1:]) == (2.5, 2.5, 2.5)  # then +inf
    three = scenario_reduce_np(cs, 1, 4, 1, 3)[0]
    assert tuple(three[1:]) == (3, 3, 3)  # then 7: rows 1, 2, 3
    # -0 and +0 tie: the lower scenario wins, whichever sign it holds
    z = np.array([[-0.0, 1, 0, 0], [0.0, 2, 0, 0], [-1.0, 3, 0, 0]], dtype=np.float32)
    r = scenario_reduce_np(z, 1, 3, 1, 1)[0]
    assert r[1] == 1 and np.signbit(r[0])  # the row itself, its -0 kept
    r = scenario_reduce_np(z[[1, 0, 2]], 1, 3, 1, 1)[0]
    assert r[1] == 2 and not np.signbit(r[0])
    # equal totals, different components: the lower scenario
    e = np.array([[5, 1, 4, 0], [5, 4, 1, 0], [5, 2, 2, 1]], dtype=np.float32)
    assert tuple(scenario_reduce_np(e, 1, 3, 1, 1)[0]) == (5, 1, 4, 0)
    assert tuple(scenario_reduce_np(e, 1, 3, 1, 2)[0]) == (5, 2.5, 2.5, 0)


def test_reference_key_packing_matches_the_decoder():
    lib = _lib.load()
    tot = np.array([4.0, -2.0, 7.5, -2.0], dtype=np.float32)
    idx, val = _lib.decode_key(pack_key_np(tot, index_base=10))
    assert (idx, val) == (11, -2.0)
    idx, val = _lib.decode_key(pack_key_np(np.array([1.0, np.nan, -np.inf], dtype=np.float32)))
    assert idx == 1 and np.isnan(val)
    assert lib.mpcr_abi_version() == 4
