"""Collision-cost weights per contact slot as a call input, the parts that
need no GPU: the two C entry points and ``mpcr_model_slots`` are exported and
bound, a stand-alone program built with the address / undefined-behaviour
sanitizers (tests/c_host/slotw_host.cpp; nothing is loaded into Python) checks
where the arguments live in the launch's argument bytes and which kernels they
select, ``mpcr_model_slots`` agrees with the compiled models,
``Model.slot_weights`` follows the product rule, and the reference the GPU
tests hold the kernels to -- ``weighted_cost4``, the oracle's cost with cost_c
recomputed from its slot distances under a weight block -- is the oracle's own
cost at all ones, and leaves at least half of each GPU parity batch
well-conditioned under that batch's parity weights (X, or X / 4 on
planner_scene: see PARITY_SCALE)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle
import parity_util as pu
from manipulator_mujoco_amd import _lib, models
from manipulator_mujoco_amd.engine import Model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
SLOTW = ("mpcr_rollout_cost_slotw", "mpcr_rollout_cost_scenarios_slotw")
H12 = 12

# the weight set X of each GPU parity batch: zero on one body's slots, 0.25 on
# one obstacle, 2.0 on the table, 1 elsewhere.  scene_mjx has no obstacle body:
# its floor takes the 0.25.
X = {"planner_scene": dict(bodies={"target_0": 0.0}, geoms={"obstacle_1": 0.25, "table_geom_1": 2.0}),
     "scene_mjx": dict(bodies={"object_0": 0.0}, geoms={"floor": 0.25, "table_geom_1": 2.0})}
BATCH = {"planner_scene": 48, "scene_mjx": 64}


def x_weights(name, m=None):
    return Model(m or models.load(name, 0.05)).slot_weights(**X[name])


# The weights of the GPU parity batches.  scene_mjx 64 x 12: X (48 of 64 candidates well-conditioned on the
# oracle).  planner_scene 48 x 12: X leaves 8 of 48 well-conditioned, and so does any set at that level -- all
# ones leave 9: the batch's cost_c (187 slots' approach terms, differences of nearby distances) moves by 3.7e-5
# relative (median) under probe A whatever the weights, and at weight 1 it is w_col cost_c = 226 of the median
# total 420, which puts the total at 1.8e-5, above the well-conditioned bar of 1e-5.  The set chosen in X's
# place is X / 4 (0 on target_0, 0.0625 on obstacle_1, 0.5 on the table, 0.25 elsewhere): the same pattern at
# the level where cost_c's share of the total is under a quarter (0.25 x 226 of 249), so that the total's
# sensitivity, share x 3.7e-5, falls under the bar -- 39 of 48 well-conditioned (X / 2: 19).  X itself is
# still run on planner_scene for everything but the parity bar.
PARITY_SCALE = {"planner_scene": 0.25, "scene_mjx": 1.0}


def parity_weights(name, m=None):
    return (np.float32(PARITY_SCALE[name]) * x_weights(name, m)).astype(np.float32)


def batch_td(name):
    return np.random.default_rng(1).uniform(-0.6, 0.6, (BATCH[name], 6 * H12))


def weighted_cost4(o, w, W):
    """The oracle's cost4 with the collision term priced by the slot weights
    ``w`` (nslot,): from result ``o`` of ``oracle.rollout(..., want_slots=True)``,
    cost_c = sum_s sum_t w[s] ([d_t,s < 0] + [t > 0] relu(0.995 d_t-1,s - d_t,s))
    over its slot distances d (n, H, nslot), cost_g and cost_r the oracle's own
    (the weights do not touch the dynamics), the total w_pos cost_g + w_rot
    cost_r + w_col cost_c."""
    d = np.asarray(o["slots"], dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    per_slot = (d < 0).sum(axis=1) + np.maximum(0.995 * d[:, :-1] - d[:, 1:], 0.0).sum(axis=1)  # (n, nslot)
    c = per_slot @ w
    g, r = o["cost4"][:, 1], o["cost4"][:, 2]
    return np.stack([W[0] * g + W[1] * r + W[2] * c, g, r, c], axis=1)


def weighted_nneg(o, w):
    """#{d < 0} over the slots whose weight is non-zero."""
    return (np.asarray(o["slots"])[:, :, np.asarray(w) != 0] < 0).sum(axis=(1, 2))


def slotw_conditioning(m, td, w, seed=1):
    """``pu.conditioning``'s record for costs priced by the weights: every
    probe's cost4 recomputed by ``weighted_cost4`` from that probe's own slot
    distances (probe A: noise 1e-7 / 1e-6 with seeds 1000 seed + 1, + 1, + 2;
    probe B: 1e-6, + 3), nneg counted over the slots of non-zero weight.  No
    probe_f4: the fp32 restatement prices every slot at 1."""
    def run(noise=0.0, sd=0):
        o = oracle.rollout(m, td, pu.Q0, pu.W, pu.PT, pu.QT, want_theta=False, want_slots=True, workers=pu.WORKERS,
                           noise=noise, seed=1000 * seed + sd)
        o["cost4"] = weighted_cost4(o, w, pu.W)
        o["nneg"] = weighted_nneg(o, w)
        return o

    o = run()
    a = o["cost4"]
    unstable = np.zeros(len(a), bool)

    def probe(eps, sd):
        r = run(eps, sd)
        unstable[:] |= r["nneg"] != o["nneg"]
        return pu._rel(a, r["cost4"])

    s4 = np.maximum.reduce([probe(1e-7, 1), probe(1e-6, 1), probe(1e-6, 2)])
    o["sens4"] = s4
    o["probe_b4"] = probe(1e-6, 3)
    o["probe_b"] = o["probe_b4"][:, 0]
    o["nneg_unstable"] = unstable
    return o, s4[:, 0]


def test_slotw_symbols_are_exported_and_bound():
    lib = _lib.load()
    for name in SLOTW + ("mpcr_model_slots",):
        assert name in _lib.EXPORTS
        fn = getattr(lib, name)
        assert fn.argtypes is not None and fn.restype is ctypes.c_int, name
    # the arguments of the target entries plus a pointer and a stride
    assert len(lib.mpcr_rollout_cost_slotw.argtypes) == len(lib.mpcr_rollout_cost_target.argtypes) + 2
    assert (len(lib.mpcr_rollout_cost_scenarios_slotw.argtypes)
            == len(lib.mpcr_rollout_cost_scenarios_target.argtypes) + 2)
    assert lib.mpcr_abi_version() == 4  # backward-compatible additions: the version stays


def test_null_handles_are_einval_with_a_message():
    lib = _lib.load()
    F = _lib.MPCR_F_DEVICE_PTRS
    calls = (lambda: lib.mpcr_rollout_cost_slotw(None, None, 0, 2, 4, None, None, 0, None, None, 0, 0, None, 0, 0, None,
                                                 0, 0, None, 0, None, None, None, None, 0, None, F, None),
             lambda: lib.mpcr_rollout_cost_scenarios_slotw(None, None, 0, 2, 2, 2, 4, None, None, 0, None, None, 0, 0,
                                                           None, 0, 0, None, 0, 0, None, 0, None, None, None, None,
                                                           None, 0, None, F, None),
             lambda: lib.mpcr_model_slots(None, None, None, None, None))
    for call in calls:
        assert lib.mpcr_model_from_blob(b"\0" * 16, 16, ctypes.byref(ctypes.c_void_p())) == -2
        before = lib.mpcr_last_error()
        assert call() == -1
        msg = lib.mpcr_last_error()
        assert msg and msg != before


def test_argument_bytes_and_kernel_choice_under_sanitizers(tmp_path):
    exe = str(tmp_path / "slotw_host")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(ROOT, "tests", "c_host", "slotw_host.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "OK slotw_host"


@pytest.mark.parametrize("name,nslot", [("planner_scene", 187), ("ur5e_hande_mjx", 47), ("scene_mjx", 87),
                                        ("dual_arm", 0)])
def test_model_slots_agree_with_the_compiled_model(name, nslot):
    m = models.load(name, 0.05)
    M = Model(m)
    g1, g2, pair = M.slots()
    assert len(g1) == len(g2) == len(pair) == nslot == m.nslot
    # every array argument is nullable: the count alone
    ns = ctypes.c_int(-1)
    assert _lib.load().mpcr_model_slots(M.handle, ctypes.byref(ns), None, None, None) == 0 and ns.value == nslot
    _, ids, _ = M.geom_poses()  # device row -> model geom id
    sa, nc = np.asarray(m.pair_slotadr)[:m.npair], np.asarray(m.pair_ncon)[:m.npair]
    seen = np.zeros(nslot, bool)
    for p in range(m.npair):
        if sa[p] < 0:
            continue
        for c in range(nc[p]):
            s = sa[p] + c
            assert pair[s] == p and ids[g1[s]] == m.pair_geom1[p] and ids[g2[s]] == m.pair_geom2[p]
            seen[s] = True
    assert seen.all()
    if nslot:
        print(f"{name}: largest pair index with a slot {int(pair.max())}")
        assert int(pair.max()) < 128  # no shipped model reaches the slab path of the single-arm kernels


def test_slot_weights_product_rule_bodies_and_errors():
    m = models.load("planner_scene", 0.05)
    M = Model(m)
    g1, g2, _ = M.slots()
    ones = M.slot_weights()
    assert ones.dtype == np.float32 and ones.shape == (187,) and (ones == 1).all()
    assert (M.slot_weights(default=0.5) == 0.25).all()  # both geoms at the default: the product
    row = M.geom_row
    w = M.slot_weights(geoms={"robot_3": 3.0, "obstacle_1": 0.25})
    a, b = row("robot_3"), row("obstacle_1")
    for s in range(187):
        want = (3.0 if a in (g1[s], g2[s]) else 1.0) * (0.25 if b in (g1[s], g2[s]) else 1.0)
        assert w[s] == np.float32(want), s
    assert (w == 0.75).sum() >= 1  # robot_3 against obstacle_1
    # a geom by its model id is the geom by its name
    gid = m.names["geom"].index("obstacle_1")
    np.testing.assert_array_equal(M.slot_weights(geoms={gid: 0.25, "robot_3": 3.0}), w)
    # a body: all its collision geoms
    wb = M.slot_weights(bodies={"target_0": 0.0})
    t0 = row("target_0")
    np.testing.assert_array_equal(wb == 0, (g1 == t0) | (g2 == t0))
    assert (wb == 0).sum() == 20
    np.testing.assert_array_equal(wb, M.slot_weights(geoms={"target_0": 0.0}))
    x = x_weights("planner_scene", m)
    vals, cnt = np.unique(x, return_counts=True)
    assert list(vals) == [0.0, 0.25, 1.0, 2.0] and list(cnt) == [20, 20, 127, 20]
    vals, cnt = np.unique(x_weights("scene_mjx"), return_counts=True)
    assert list(vals) == [0.0, 0.25, 1.0, 2.0] and cnt[0] == 20 and cnt[3] == 20
    for bad in (dict(geoms={"no_such_geom": 1.0}), dict(bodies={"no_such_body": 1.0}), dict(geoms={9999: 1.0}),
                dict(bodies={"world": 2.0})):  # (the world body's floor is in a pair; a body without geoms is refused)
        if bad == dict(bodies={"world": 2.0}):
            assert (M.slot_weights(**bad) != 1).any()
            continue
        with pytest.raises(ValueError):
            M.slot_weights(**bad)
    assert Model(models.load("dual_arm", 0.05)).slot_weights().shape == (0,)


@pytest.fixture(scope="module", params=["planner_scene", "scene_mjx"])
def x_case(request):
    """The GPU parity batch of a scene and the oracle's record priced by its parity weights."""
    name = request.param
    m = models.load(name, 0.05)
    td = batch_td(name)
    w = parity_weights(name, m)
    o, sens = slotw_conditioning(m, td, w, seed=1)
    return dict(name=name, m=m, td=td, w=w, o=o, sens=sens)


@pytest.mark.parametrize("name", ["planner_scene", "scene_mjx"])
def test_weighted_cost4_at_ones_is_the_oracles(name):
    m = models.load(name, 0.05)
    td = batch_td(name)
    o = oracle.rollout(m, td, pu.Q0, pu.W, pu.PT, pu.QT, want_theta=False, want_slots=True, workers=pu.WORKERS)
    own = o["cost4"].copy()
    got = weighted_cost4(o, np.ones(m.nslot), pu.W)
    rel = np.abs(got - own) / np.maximum(np.abs(own), 1e-12)
    print(f"{name} {len(td)}x{H12}: weighted_cost4 at ones against the oracle's cost4, max rel {rel.max():.1e}")
    assert rel.max() < 1e-9
    np.testing.assert_array_equal(weighted_nneg(o, np.ones(m.nslot)), o["nneg"])
    # doubling every weight is doubling w_col
    a = weighted_cost4(o, 2.0 * np.ones(m.nslot), pu.W)
    b = weighted_cost4(o, np.ones(m.nslot), pu.W * (1, 1, 2))
    np.testing.assert_allclose(a[:, 0], b[:, 0], rtol=1e-14)


def test_parity_weights_leave_half_of_each_batch_well_conditioned(x_case):
    c = x_case
    o, sens, m = c["o"], c["sens"], c["m"]
    assert o["status"] == 0
    well = (sens < pu.TOL / 10) & ~pu.grazing(m, o)
    ones = weighted_cost4(o, np.ones(m.nslot), pu.W)
    moved = o["cost4"][:, 3] != ones[:, 3]
    print(f"{c['name']}: X x {PARITY_SCALE[c['name']]} leaves {int(well.sum())} of {len(sens)} candidates well-conditioned; cost_c moves on "
          f"{int(moved.sum())}; busiest step {int(o['maxrows'].max())} rows")
    assert well.sum() * 2 >= len(sens)
    assert moved.sum() * 2 >= len(sens)  # the weights act on the batch
    assert int(well.sum()) == {"planner_scene": 39, "scene_mjx": 48}[c["name"]]  # (the oracle's counts, as recorded)
