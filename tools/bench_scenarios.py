"""Time one scenario rollout against the two ways to price the same candidates
in the same worlds with the calls that existed before it.

    python tools/bench_scenarios.py [--model planner_scene] [--S 4] [--n 4096] [--H 50]
                                    [--geom obstacle_1] [--rounds 3] [--reps 5] [--out FILE]

n projected candidates of one problem, S scenarios: scenario s has static geom
``--geom`` displaced by s x (2 cm, -1.5 cm, 1 cm).  Three sides, alternated
``--rounds`` times in one process, each the median of ``--reps`` launches
between HIP events on the launch stream (theta and thetadot requested, as the
planner does):

  scenarios   one ``rollout_cost_scenarios`` call: S n rollouts reading n
              input rows, theta / thetadot written by scenario 0, the fold
  replicated  ``rollout_cost_state`` over S problems with the input copied S
              times (the copy is not timed) plus ``scenario_reduce``
  one_world   S ``rollout_cost_state`` calls of n candidates, one per world,
              plus ``scenario_reduce`` on their costs put side by side

and the fold alone.  Also prints the bytes the shared input and the
nominal-only theta / thetadot rows save.  Prints one JSON line; ``--out`` also
writes it to a file.  Diagnostic only (not the bench.py contract).  Needs a
gfx950 GPU.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

Q0 = np.array([1.5, -1.8, 1.75, -1.25, -1.6, 0.0])
W, PT, QT = (20.0, 3.0, 80.0), (-0.3, -0.3, 0.5), (0.0, 1.0, 0.0, 0.0)
STEP = np.array([0.02, -0.015, 0.01])


def ev_time(fn, reps):
    import torch
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="planner_scene")
    ap.add_argument("--S", type=int, default=4)
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--H", type=int, default=50)
    ap.add_argument("--geom", default="obstacle_1")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    from manipulator_mujoco_amd import basis, models
    from manipulator_mujoco_amd.engine import MPCR_LAYOUT_XI, Engine
    from manipulator_mujoco_amd.projection import ProjectionFilter
    if not torch.cuda.is_available():
        raise SystemExit("bench_scenarios needs a gfx950 GPU")
    S, n, H = a.S, a.n, a.H
    m = models.load(a.model, 0.05)
    _, P, Pd, Pdd = basis.planner_basis(H, 0.05)
    e = Engine(m, H, S * n, Pd)
    proj = ProjectionFilter(P, Pd, Pdd, 6, torch.device("cpu"))
    xi = proj(torch.tensor(np.random.default_rng(20250632).normal(0, np.sqrt(10.003), (n, 66)).astype(np.float32)),
              proj.boundary(Q0, np.zeros(6), np.zeros(6), n), 10).cuda()
    own, ids, fixed = e.model.geom_poses()
    row = e.model.geom_row(a.geom)
    if not fixed[row]:
        raise SystemExit(f"geom {a.geom!r} is not static")
    gp = np.stack([own] * S)
    for s in range(S):
        gp[s, row, :3] += (s * STEP).astype(np.float32)
    gp = torch.as_tensor(gp).cuda()
    par = torch.as_tensor(np.tile(Engine.params(Q0, W, PT, QT), (S, 1))).cuda()
    xr = xi.repeat(S, 1).contiguous()
    f32 = dict(dtype=torch.float32, device="cuda")
    cs, c = torch.empty((S * n, 4), **f32), torch.empty((n, 4), **f32)
    th, td = torch.empty((n, 6 * H), **f32), torch.empty((n, 6 * H), **f32)
    thr, tdr = torch.empty((S * n, 6 * H), **f32), torch.empty((S * n, 6 * H), **f32)
    key, keys = torch.empty(1, dtype=torch.int64, device="cuda"), torch.empty(S, dtype=torch.int64, device="cuda")

    def scenarios():
        e.rollout_cost_scenarios(xi, MPCR_LAYOUT_XI, par, 1, S, cs, cost4=c, geom_pose=gp, theta=th, thetadot=td,
                                 best_keys=key)

    def replicated():
        e.rollout_cost_state(xr, MPCR_LAYOUT_XI, par, S, cs, geom_pose=gp, theta=thr, thetadot=tdr, best_keys=keys)
        e.scenario_reduce(cs, 1, S, S, cost4=c, best_keys=key)

    def one_world():
        for s in range(S):
            e.rollout_cost_state(xi, MPCR_LAYOUT_XI, par[s], 1, cs[s * n:(s + 1) * n], geom_pose=gp[s],
                                 theta=thr[s * n:(s + 1) * n], thetadot=tdr[s * n:(s + 1) * n], best_keys=keys[s:s + 1])
        e.scenario_reduce(cs, 1, S, S, cost4=c, best_keys=key)

    def fold():
        e.scenario_reduce(cs, 1, S, S, cost4=c, best_keys=key)

    sides = dict(scenarios=scenarios, replicated=replicated, one_world=one_world, fold=fold)
    out = {}
    for name, fn in sides.items():  # warm-up; the three ways agree on the fold
        fn()
        torch.cuda.synchronize()
        out[name] = c.clone()
    same = all(torch.equal(out["scenarios"].view(torch.int32), out[k].view(torch.int32)) for k in ("replicated", "one_world"))
    runs = {k: [] for k in sides}
    for _ in range(a.rounds):
        for name, fn in sides.items():
            runs[name].append(ev_time(fn, a.reps))
    row_b = 6 * H * 4
    res = {"model": a.model, "geom": a.geom, "scenarios": S, "candidates": n, "H": H, "rounds": a.rounds, "reps": a.reps,
           "folds_bitwise_equal": bool(same)}
    for k in sides:
        res[f"{k}_ms"] = [round(x, 4) for x in runs[k]]
        res[f"{k}_median_ms"] = round(float(np.median(runs[k])), 4)
    res["input_bytes_shared"], res["input_bytes_replicated"] = n * 66 * 4, S * n * 66 * 4
    res["theta_thetadot_bytes_nominal_only"], res["theta_thetadot_bytes_every_scenario"] = 2 * n * row_b, 2 * S * n * row_b
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
