"""Time one batched multi-problem tick against the same problems planned one
after another.

    python tools/bench_multi.py [--model scene_mjx] [--B 8] [--n 512] [--H 50] [--iters 3]
                                [--rounds 3] [--ticks 9] [--parent-lib PATH] [--out FILE]

Two sides, each in a fresh child process (a process binds one libmpcr),
alternated ``--rounds`` times:

  batch  one ``compute_cem_batch`` tick of a ``num_problems=B`` planner
  seq    B ``compute_cem`` ticks in sequence on a one-problem planner of the
         same ``num_batch`` -- on ``--parent-lib`` (a libmpcr.so built from an
         earlier commit, bound through MPCR_LIB) when given, else this build

Both planners run ``graph=True, return_rollouts=False`` (what the closed loop
uses).  A tick's time is the median over ``--ticks`` ticks of HIP events on the
launch stream around the call (the host copies of the results included, the
call ends with them) and of the wall clock; the batch side also times each
stage of one CEM iteration (factor, sample/project, rollout, top-k, update)
with events.  Prints one JSON line; ``--out`` also writes it to a file.
Diagnostic only (not the bench.py contract).  Needs a gfx950 GPU.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

Q0 = np.array([1.5, -1.8, 1.75, -1.25, -1.6, 0.0])
PT, QT = np.array([-0.3, -0.3, 0.5]), np.array([0.0, 1.0, 0.0, 0.0])


def ev_time(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    ev, wall = [], []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        b.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        ev.append(a.elapsed_time(b))
    return float(np.median(ev)), float(np.median(wall))


def problems(B):
    rng = np.random.default_rng(1)
    return dict(xi_mean=np.zeros((B, 66)), init_pos=Q0 + rng.uniform(-0.05, 0.05, (B, 6)),
                init_vel=np.zeros((B, 6)), init_acc=np.zeros((B, 6)),
                target_pos=PT + rng.uniform(-0.1, 0.1, (B, 3)), target_rot=np.tile(QT, (B, 1)))


def child(args):
    import torch

    from manipulator_mujoco_amd.cem import topk_multi
    from manipulator_mujoco_amd.planner import cem_planner
    if not torch.cuda.is_available():
        raise SystemExit("bench_multi needs a gfx950 GPU")
    B, n = args.B, args.n
    kw = dict(num_dof=6, num_batch=n, num_steps=args.H, timestep=0.05, maxiter_cem=args.iters, num_elite=0.05,
              w_pos=20.0, w_rot=3.0, w_col=80.0, maxiter_projection=10, model_path=args.model, verbose=False,
              graph=True, return_rollouts=False)
    pr = problems(B)
    res = {"side": args.side}
    if args.side == "seq":
        p = cem_planner(**kw)

        def tick():
            for i in range(B):
                p.compute_cem(pr["xi_mean"][i], pr["init_pos"][i], pr["init_vel"][i], pr["init_acc"][i],
                              pr["target_pos"][i], pr["target_rot"][i])
    else:
        p = cem_planner(num_problems=B, seed_step=1, **kw)

        def tick():
            p.compute_cem_batch(**pr)
    tick()  # warm-up and graph capture
    res["tick_event_ms"], res["tick_wall_ms"] = ev_time(tick, args.ticks)
    if args.side == "batch":
        # the stages of one iteration on the buffers the tick left behind
        bounds = (p.v_max, p.a_max, p.p_max)
        nv = p.nvar
        cov = p._cov.view(B, nv, nv)
        st = {}
        st["factor_ms"] = ev_time(lambda: p.cem.factor_multi(cov, 0.003), 20)[0]
        st["sample_project_ms"] = ev_time(lambda: p.cem.sample_project_multi(
            B, n, p._mean, 1, 0, p._beq, 10, bounds, seed_step=1, xi_samples=p._xs, out=p._xf), 20)[0]
        cost = p._costs[0]
        st["rollout_ms"] = ev_time(lambda: p.engine.rollout_cost_multi(
            p._xf.view(B * n, nv), 0, p._par, B, cost, best_keys=p._key), 5)[0]
        idx = p._idx.view(B, p.ellite_num)
        st["topk_ms"] = ev_time(lambda: topk_multi(p.engine, cost, B, p.ellite_num, stride=4, out=idx), 20)[0]
        m0, c0 = p._mean.clone(), p._cov.clone()

        def upd():
            p._mean.copy_(m0)
            p._cov.copy_(c0)
            p.cem.update_multi(p._xs.view(B, n, nv), cost, 4, idx, 10.0, 0.6, 0.6, p._mean, p._cov)
        st["update_ms_incl_2_copies"] = ev_time(upd, 20)[0]
        res["stages"] = st
    print("BENCH_MULTI " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="scene_mjx")
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--n", type=int, default=512, help="candidates per problem")
    ap.add_argument("--H", type=int, default=50)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--ticks", type=int, default=9)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--side", choices=("batch", "seq"), default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.side:
        return child(args)
    base = [sys.executable, os.path.abspath(__file__)]
    for k in ("model", "B", "n", "H", "iters", "ticks"):
        base += [f"--{k}", str(getattr(args, k))]
    runs = {"batch": [], "seq": []}
    for _ in range(args.rounds):
        for side in ("batch", "seq"):
            env = dict(os.environ)
            env.pop("MPCR_LIB", None)
            if side == "seq" and args.parent_lib:
                env["MPCR_LIB"] = os.path.abspath(args.parent_lib)
            r = subprocess.run(base + ["--side", side], env=env, capture_output=True, text=True, timeout=300)
            line = [x for x in r.stdout.splitlines() if x.startswith("BENCH_MULTI ")]
            if r.returncode != 0 or not line:
                sys.stderr.write(r.stdout + r.stderr)
                raise SystemExit(f"{side} side failed (exit {r.returncode})")
            runs[side].append(json.loads(line[-1][len("BENCH_MULTI "):]))
    med = lambda side, k: float(np.median([x[k] for x in runs[side]]))  # noqa: E731
    res = {"model": args.model, "problems": args.B, "candidates_per_problem": args.n, "H": args.H, "iters": args.iters,
           "graph": True, "return_rollouts": False, "ticks_per_run": args.ticks, "rounds": args.rounds,
           "seq_lib": "parent build (MPCR_LIB)" if args.parent_lib else "this build"}
    for side in ("batch", "seq"):
        for k in ("tick_event_ms", "tick_wall_ms"):
            res[f"{side}_{k}"] = [round(x[k], 4) for x in runs[side]]
    res["speedup_event"] = round(med("seq", "tick_event_ms") / med("batch", "tick_event_ms"), 3)
    res["speedup_wall"] = round(med("seq", "tick_wall_ms") / med("batch", "tick_wall_ms"), 3)
    keys = runs["batch"][0]["stages"].keys()
    res["batch_stages_ms"] = {k: round(float(np.median([x["stages"][k] for x in runs["batch"]])), 4) for k in keys}
    out = json.dumps(res)
    print(out)
    if args.out:
        with open(args.out, "w") as f:
            f.write(out + "\n")


if __name__ == "__main__":
    main()
