import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs an MI355X (gfx950); run with -m gpu")


@pytest.fixture(scope="session")
def mjcf_scenes(tmp_path_factory):
    """The MJCF scenes the bundles were compiled from (tests/golden/mjcf: the
    .xml files and, xz-compressed, the meshes they load), unpacked into a
    temporary directory with their own layout; returns that directory."""
    import lzma
    import shutil
    src = os.path.join(GOLDEN, "mjcf")
    dst = str(tmp_path_factory.mktemp("mjcf"))
    for d, _, files in os.walk(src):
        out = os.path.join(dst, os.path.relpath(d, src))
        os.makedirs(out, exist_ok=True)
        for f in files:
            with open(os.path.join(d, f), "rb") as fh:
                data = fh.read()
            if f.endswith(".xz"):
                f, data = f[:-3], lzma.decompress(data)
            with open(os.path.join(out, f), "wb") as fh:
                fh.write(data)
    # the planner scene loads the same two Hand-E meshes from a folder of its own: stored once
    hande = os.path.join(dst, "sampling_based_planner", "ur5e_hande_mjx", "assets", "hande")
    os.makedirs(hande)
    for f in ("coupler.stl", "hande.stl"):
        shutil.copy(os.path.join(dst, "universal_robots_ur5e", "assets", "hande", f), hande)
    return dst


@pytest.fixture(scope="session")
def planner_model():
    from manipulator_mujoco_amd import models
    return models.load("planner_scene", 0.05)


@pytest.fixture(scope="session")
def all_models():
    from manipulator_mujoco_amd import models
    return {k: models.load(k, 0.05) for k in models.BUNDLES}
