"""Actuator controls as a call input, the parts that need no GPU: the three C
entry points are exported and bound, ``mpcr_model_actuators`` reports the
model's ranges, and a stand-alone program built with the address /
undefined-behaviour sanitizers (tests/c_host/ctrl_host.cpp; nothing is loaded
into Python) checks what csrc/dev_model.h holds for them: the appended range
array, that no earlier DevModel field moved, the D derivation on its own
against impl_D, and the predicate that refuses a control input."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from manipulator_mujoco_amd import _lib, models
from manipulator_mujoco_amd.engine import Model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
CTRL = ("mpcr_rollout_cost_ctrl", "mpcr_plant_set_ctrl", "mpcr_model_actuators")
F = _lib.MPCR_F_DEVICE_PTRS
BUNDLED = tuple(dict.fromkeys(models.PLANNER_SCENES + ("dual_arm", "hande_scene", "scene_mjx")))

# "name offset bytes" of DevModel fields across the whole struct, and its
# size, as the struct was before act_ctrlrange was appended (ctrl_host --layout
# of that tree): the kernels that do not read the new array address every
# field where they did
BEFORE = """nbody 0 4;nu 68 4;integrator 76 4;timestep 100 4;body_kind 148 128;body_mass 3476 128;jnt_type 3876 128;
jnt_qpos0 6820 128;dof_body 6948 128;mc_c0 8116 128;dof_invweight0 8500 128;qpos_init 8628 128;geom_body 8884 288;
geom_rbound 12916 288;pair_g1 13204 3072;pair_jinfo 25504 12288;pair_diag 71584 3072;eq_type 74656 32;
eqrow_k 75424 96;dof_stiffness 75520 128;dof_actfrc 76544 256;act_ntrn 76800 64;act_moment 77248 128;
act_gain 77376 256;act_bias 77632 256;act_frc 77888 128;impl_D 78016 4096;geom_hulladr 82112 288;hull_vert 82976 8;
hull_head 83016 8;geom_faceadr 83024 288;face_plane 83888 8;cone_face 84224 8;ctrl_qposadr 84232 32;cone 84296 4;
pair_cmu 84308 3072;body_visc 87380 256;ten_body 87636 16;ten_pos 87660 64;ten_invw 87804 8;sizeof 87824 0"""


def test_ctrl_symbols_are_exported_and_bound():
    lib = _lib.load()
    for name in CTRL:
        assert name in _lib.EXPORTS
        fn = getattr(lib, name)
        assert fn.argtypes is not None and fn.restype is ctypes.c_int, name
    assert lib.mpcr_abi_version() == 4  # backward-compatible additions: the version stays


def test_null_handles_are_einval_with_a_message():
    lib = _lib.load()
    calls = (lambda: lib.mpcr_rollout_cost_ctrl(None, None, 0, 2, 4, None, None, 0, None, None, 0, 0, None, None, None,
                                                None, 0, None, F, None),
             lambda: lib.mpcr_plant_set_ctrl(None, None),
             lambda: lib.mpcr_model_actuators(None, None, None, None))
    for call in calls:
        assert lib.mpcr_model_from_blob(b"\0" * 16, 16, ctypes.byref(ctypes.c_void_p())) == -2
        before = lib.mpcr_last_error()
        assert call() == -1
        msg = lib.mpcr_last_error()
        assert msg and msg != before


@pytest.mark.parametrize("name", ["dual_arm", "hande_scene", "scene_mjx"])
def test_model_actuators_reports_the_models_ranges(name):
    m = models.load(name, 0.05)
    nu, rng, lim = Model(m).actuators()
    assert nu == int(getattr(m, "nu", 0))
    if name == "scene_mjx":
        assert nu == 0
        return
    assert nu == {"dual_arm": 14, "hande_scene": 1}[name]
    np.testing.assert_array_equal(rng, np.asarray(m.act_ctrlrange, dtype=np.float64).reshape(-1, 2)[:nu])
    np.testing.assert_array_equal(lim, np.asarray(m.act_ctrllimited)[:nu] != 0)
    # clamp_ctrl is the library's clamp: inside the range untouched, outside onto it
    mod = Model(m)
    big = np.full(nu, 1e6)
    hi = mod.clamp_ctrl(big)
    np.testing.assert_array_equal(hi[lim], rng[lim, 1])
    np.testing.assert_array_equal(hi[~lim], big[~lim])
    np.testing.assert_array_equal(mod.clamp_ctrl(mod.own_ctrl()), mod.own_ctrl())


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("ctrl_host")
    exe = str(d / "ctrl_host")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(ROOT, "tests", "c_host", "ctrl_host.cpp")], check=True)
    return d, exe


def test_no_earlier_devmodel_field_moved(host):
    _, exe = host
    r = subprocess.run([exe, "--layout"], capture_output=True, text=True, check=True)
    now = {w[0]: (int(w[1]), int(w[2])) for w in (ln.split() for ln in r.stdout.splitlines())}
    before = {w[0]: (int(w[1]), int(w[2])) for w in (e.split() for e in BEFORE.replace("\n", "").split(";"))}
    size_before = before.pop("sizeof")[0]
    size_now = now.pop("sizeof")[0]
    off, nbytes = now.pop("act_ctrlrange")
    assert now == before
    # appended: behind everything the struct held, and nothing behind it but the struct's alignment padding
    assert off >= max(o + n for o, n in before.values()) and off + nbytes <= size_before + nbytes
    assert nbytes == 16 * 2 * 4 and 0 <= size_now - (off + nbytes) < 16


def test_range_array_implicit_d_and_predicate_under_sanitizers(host):
    d, exe = host
    paths = []
    for name in BUNDLED:
        path = str(d / f"{name}.mpcrm")
        models.load(name, 0.05).save(path)
        paths.append(path)
    r = subprocess.run([exe] + paths, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    ok = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("OK ")]
    assert [w[1] for w in ok] == paths
    seen = {os.path.basename(w[1])[:-6]: (w[2], w[3]) for w in ok}
    assert seen["dual_arm"][0] == "nu=14" and seen["hande_scene"][0] == "nu=1"
    # the D check ran: at least one bundled model with actuators integrates implicitly
    assert any(nu != "nu=0" and integ == "integrator=3" for nu, integ in seen.values())
