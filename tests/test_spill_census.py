"""Scalar-register spills of the single-arm rollout kernels (no GPU): the
census of tools/spill_census.py on this checkout, one compile of
rollout_narrow.hip to assembly.

For all six instantiations: no VGPR spills, no scratch, at most 128 VGPRs
(4 waves per SIMD), and the scalar spill count and the spill reloads inside
the horizon loop at most what the build that introduced this test reached.
The ceilings stand beside the parent's (da7eb63) values; the goal, zero
in-loop reloads for the one-wave kernels, is not reached: what remains is the
set of step-local lane masks and model scalars the compiler saves across the
collision phase and a dozen per-step reloads at the step's top
(profiles/sgpr_spills_audit.txt).
"""
import importlib.util
import os
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (WPC, MULTI, STATE): (sgpr_spill_count, in-loop reloads) -- the parent's, then this build's ceiling
PARENT = {
    (2, True, False): (80, 75),
    (2, False, False): (60, 105),
    (1, True, False): (103, 236),
    (1, False, False): (79, 197),
    (2, True, True): (93, 118),
    (1, True, True): (120, 229),
}
CEILING = {
    (2, True, False): (31, 30),
    (2, False, False): (31, 30),
    (1, True, False): (56, 47),
    (1, False, False): (56, 47),
    (2, True, True): (41, 38),
    (1, True, True): (64, 87),
}


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    return None


@pytest.fixture(scope="module")
def census():
    if _hipcc() is None:
        pytest.skip("hipcc not found")
    spec = importlib.util.spec_from_file_location("spill_census", os.path.join(ROOT, "tools", "spill_census.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    rows = mod.run(ROOT)
    out = {}
    for r in rows:
        wpc, multi, state = r["kernel"].rstrip(">").split(",")[4:]
        out[(int(wpc), multi == "true", state == "true")] = r
    return out


def test_six_single_arm_kernels(census):
    assert set(census) == set(CEILING)


@pytest.mark.parametrize("key", sorted(CEILING), ids=lambda k: f"wpc{k[0]}_multi{int(k[1])}_state{int(k[2])}")
def test_spills_within_ceiling(census, key):
    r = census[key]
    in_loop = r["reloads"]["depth1"] + r["reloads"]["deeper"]
    print(f"{r['kernel']}: sgpr_spill_count {r['sgpr_spill_count']} (parent {PARENT[key][0]}, ceiling "
          f"{CEILING[key][0]}), in-loop reloads {in_loop} (parent {PARENT[key][1]}, ceiling {CEILING[key][1]}), "
          f"VGPRs {r['vgpr_count']}, codeLenInByte {r['codeLenInByte']}")
    assert r["vgpr_spill_count"] == 0
    assert r["private_segment_fixed_size"] == 0, "scratch"
    assert r["vgpr_count"] <= 128
    assert r["group_segment_fixed_size"] == (18240 if key[0] == 2 else 9520), "LDS image"
    assert r["sgpr_spill_count"] <= CEILING[key][0]
    assert in_loop <= CEILING[key][1]
    # the census and the metadata agree: one lane written per spilled scalar at least
    assert bool(r["spill_vgprs"]) == (r["sgpr_spill_count"] > 0)


def test_ceilings_below_parent():
    for k, (spills, reloads) in CEILING.items():
        assert spills < PARENT[k][0] and reloads < PARENT[k][1]
