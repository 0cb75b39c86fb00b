"""The launch planning (csrc/rollout_plan.h: waves per candidate, horizon
segments, candidate groups, the arguments of a group) without a GPU: a
stand-alone program built with the address / undefined-behaviour sanitizers
(tests/c_host/plan_host.cpp; nothing is loaded into Python) holds
``rollout_dispatches``, ``seg_plan`` and ``group_args`` to the rules their
comments state, on hand-filled arguments and thresholds of its own."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
CSRC = os.path.join(ROOT, "manipulator_mujoco_amd", "csrc")


def test_launch_planning_under_sanitizers(tmp_path):
    exe = str(tmp_path / "plan_host")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(ROOT, "tests", "c_host", "plan_host.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "OK plan_host"


def test_the_plan_header_is_host_code_and_the_single_arm_unit_has_no_planning():
    plan = open(os.path.join(CSRC, "rollout_plan.h")).read()
    for word in ("__global__", "__device__", "hipLaunchKernelGGL", "<<<"):
        assert word not in plan, word
    narrow = open(os.path.join(CSRC, "rollout_narrow.hip")).read()
    for word in ("group_args", "seg_plan", "rollout_dispatches", "getenv", "hipStreamWaitEvent"):
        assert word not in narrow, word
