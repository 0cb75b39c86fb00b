"""bench.py's self-launch path: `python bench.py --gpus N`
outside torch.distributed.run starts N fresh rank processes itself (the parent
never imports torch), rank 0's JSON line is the output and the exit code is
the worst rank's.  The plumbing runs here on CPU through the hidden
--launch-selftest hook (gloo group, one all-reduce); tests/test_gpu_bench.py
runs the real bench through the same path on the GPU box."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(args, extra_env=None):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    env.update(extra_env or {})
    return subprocess.run([sys.executable, "bench.py"] + args, cwd=ROOT, env=env, capture_output=True, text=True,
                          timeout=180)


def test_self_launch_two_ranks():
    r = _bench(["--gpus", "2", "--launch-selftest"])
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    rec = json.loads(lines[0])
    assert rec["world"] == 2 and rec["sum_ranks_plus_1"] == 3
    assert rec["env"]["WORLD_SIZE"] == "2" and rec["env"]["RANK"] == "0" and rec["env"]["MASTER_ADDR"] == "127.0.0.1"


def test_self_launch_four_ranks():
    r = _bench(["--gpus", "4", "--launch-selftest"])
    assert r.returncode == 0, r.stderr[-4000:]
    rec = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
    assert rec["world"] == 4 and rec["sum_ranks_plus_1"] == 10


def test_self_launch_failing_rank_fails_the_run():
    # rank 1 exits 3 before joining; rank 0 blocks in the rendezvous and is
    # killed after the grace period: the parent returns the worst code
    r = _bench(["--gpus", "2", "--launch-selftest"], {"MPCR_SELFTEST_FAIL_RANK": "1", "TORCH_DIST_INIT_BARRIER": "0"})
    assert r.returncode != 0
    assert not [ln for ln in r.stdout.splitlines() if ln.startswith("{")]


def test_parent_does_not_import_torch():
    # the launcher returns before the parent imports torch (so it cannot
    # initialise the GPU): bench.py keeps torch imports inside main()'s rank path
    src = open(os.path.join(ROOT, "bench.py")).read()
    head = src.split("def main():")[0]
    assert "\nimport torch" not in head and "\nfrom torch" not in head
    body = src.split("def main():")[1]
    assert body.index("launch_ranks(") < body.index("import torch")


def test_dump_outputs_keeps_types_and_budget(tmp_path, monkeypatch):
    """--dump-outputs: fp32 / fp64 stay, integers become fp64, and a dump over
    the byte budget keeps the same seeded, sorted row sample on every call."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    rng = np.random.default_rng(0)
    arrays = {"a": rng.normal(size=(1000, 8)).astype(np.float32), "s": np.arange(1000, dtype=np.int32),
              "k": np.array([3, 1.5])}
    bench.dump_outputs(str(tmp_path / "all"), arrays)
    got = {f[:-4]: np.load(tmp_path / "all" / f) for f in os.listdir(tmp_path / "all")}
    assert sorted(got) == ["a", "k", "s"]
    assert got["a"].dtype == np.float32 and got["s"].dtype == np.float64 and got["k"].dtype == np.float64
    assert (got["a"] == arrays["a"]).all() and (got["s"] == arrays["s"]).all()
    # the budget bounds the folder: every file of every rank, headers and row numbers included
    monkeypatch.setattr(bench, "DUMP_BUDGET", 8000)
    for d in ("x", "y"):
        for r in (0, 1):
            bench.dump_outputs(str(tmp_path / d), arrays, rank=r, world=2)
    assert sum(os.path.getsize(tmp_path / "x" / f) for f in os.listdir(tmp_path / "x")) <= 8000
    x = {f[:-4]: np.load(tmp_path / "x" / f) for f in os.listdir(tmp_path / "x")}
    y = {f[:-4]: np.load(tmp_path / "y" / f) for f in os.listdir(tmp_path / "y")}
    assert sorted(x) == sorted(f"{n}_rank{r}" for n in ("a", "a_rows", "k", "s", "s_rows") for r in (0, 1))
    assert (x["k_rank1"] == arrays["k"]).all()
    rows = x["a_rows_rank1"].astype(int)
    assert len(rows) > 0 and (np.diff(rows) > 0).all() and (x["a_rank1"] == arrays["a"][rows]).all()
    assert (x["s_rank1"] == arrays["s"][x["s_rows_rank1"].astype(int)]).all()
    assert all((x[k] == y[k]).all() for k in x)
