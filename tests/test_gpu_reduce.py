"""The rollout kernels' wave reductions (csrc/wave.h: wsum, wsum2, wsum3,
wsum_lo<16>, wsum_lo<32>) against the reference form they replaced, through
mpcr_selftest_reduce: every production form returns the reference's bits
(NaN included: compared as bit patterns), also at the row boundaries and for
the inputs whose sum a left-out "+ 0" step could change (-0)."""
import ctypes

import numpy as np
import pytest

from manipulator_mujoco_amd import _lib

pytestmark = pytest.mark.gpu

NOUT = 12
# out columns (include/mpcr.h): (production form, its reference, vector offset of the reference)
FORMS = {"wsum": (1, 0, 0), "wsum2.a": (2, 0, 0), "wsum2.b": (3, 0, 1), "wsum3.a": (4, 0, 0), "wsum3.b": (5, 0, 1),
         "wsum3.c": (6, 0, 2), "wsum_lo<16>": (8, 7, 0), "wsum_lo<32>": (10, 9, 0)}


def vectors():
    rng = np.random.default_rng(20250712)
    v = [rng.choice([-1.0, 1.0], (256, 64)) * 10.0 ** rng.uniform(-6, 6, (256, 64))]
    names = ["seeded"] * 256
    for last in (0, 14, 15, 16, 22, 31, 32, 63):  # non-zeros end at this lane
        x = np.zeros((1, 64))
        x[0, :last + 1] = rng.choice([-1.0, 1.0], last + 1) * 10.0 ** rng.uniform(-6, 6, last + 1)
        v.append(x)
        names.append(f"ends at lane {last}")
    v.append(np.zeros((1, 64)))
    names.append("zeros")
    for lane in (3, 40):
        for val, nm in ((np.nan, "NaN"), (np.inf, "+inf")):
            x = rng.normal(0, 10, (1, 64))
            x[0, lane] = val
            v.append(x)
            names.append(f"{nm} at lane {lane}")
    # negative zeros: every lane; the first row / the first two rows only (the
    # rest +0); one -0 among +0; one -0 among values that cancel
    for lanes, nm in ((slice(0, 64), "-0 everywhere"), (slice(0, 16), "-0 in lanes 0-15"),
                      (slice(0, 32), "-0 in lanes 0-31"), (slice(5, 6), "one -0 lane")):
        x = np.zeros((1, 64))
        x[0, lanes] = -0.0
        v.append(x)
        names.append(nm)
    x = np.zeros((1, 64))
    x[0, :4] = (1.5, -0.0, -1.5, -0.0)
    v.append(x)
    names.append("-0 among cancelling values")
    return np.concatenate(v).astype(np.float32), names


@pytest.fixture(scope="module")
def sums():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    lib = _lib.load()
    vin, names = vectors()
    out = np.full((len(vin), NOUT), 7.0, dtype=np.float32)
    _lib.check(lib.mpcr_selftest_reduce(torch.cuda.current_device(), vin.ctypes.data_as(ctypes.c_void_p), len(vin),
                                        out.ctypes.data_as(ctypes.c_void_p)))
    return vin, names, out.view(np.uint32)


def test_reference_is_the_sum(sums):
    """The reference itself: finite inputs sum to the fp64 sum within fp32
    rounding of the six steps, NaN / inf lanes give NaN / inf."""
    vin, names, bits = sums
    ref = bits[:, 0].view(np.float32).astype(np.float64)
    fin = np.isfinite(vin).all(axis=1)
    bound = ((1 + 2.0 ** -24) ** 6 - 1) * np.abs(vin[fin].astype(np.float64)).sum(axis=1)
    assert (np.abs(ref[fin] - vin[fin].astype(np.float64).sum(axis=1)) <= bound).all()
    for k, nm in enumerate(names):
        if nm.startswith("NaN"):
            assert np.isnan(ref[k])
        if nm.startswith("+inf"):
            assert ref[k] == np.inf
    assert (bits[:, 11] == 0).all()


@pytest.mark.parametrize("form", sorted(FORMS))
def test_form_is_bitwise_the_reference(sums, form):
    vin, names, bits = sums
    col, refcol, off = FORMS[form]
    want = np.roll(bits[:, refcol], -off)
    bad = np.nonzero(bits[:, col] != want)[0]
    assert bad.size == 0, [(names[k], hex(bits[k, col]), hex(want[k])) for k in bad[:8]]
