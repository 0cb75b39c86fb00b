"""Time one libmpcr variant (path in argv[1]) on the C3 bench workload; prints
median kernel ms over R repetitions (HIP events on the launch stream).
MODEL / N / H choose the workload.  ENTRY=state times the device-parameter
state entry (Engine.rollout_cost_state, one problem, no state blocks) instead
of rollout_cost, with CTRL=none (no control block: runs on a library from
before the control input too), const (one block of the model's own controls)
or sched (one row per step), and GEOM=none, const (one block of the model's
own static geom poses) or sched (one block per step); START=1 starts from a
block holding the template state, which alone selects the STATE kernels;
TARGET=none, const (one target row, the parameter block's) or sched (one row
per step, the target translating and yawing over the horizon); SLOTW=none,
ones (one slot-weight block of ones) or mixed (one block of weights 0, 0.25,
1 and 2 in turn); STEPW=none, ones (one step-weight schedule of ones) or mixed
(one schedule discounted by 0.85 a step, the last step's pose terms times 4)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from manipulator_mujoco_amd import _lib  # noqa: E402

_lib.LIB_PATH = os.path.abspath(sys.argv[1])
import torch  # noqa: E402

from manipulator_mujoco_amd import basis, models  # noqa: E402
from manipulator_mujoco_amd.engine import MPCR_LAYOUT_XI, Engine  # noqa: E402
from manipulator_mujoco_amd.projection import ProjectionFilter  # noqa: E402

name = os.environ.get("MODEL", "scene_mjx")
n, H = int(os.environ.get("N", 4096)), int(os.environ.get("H", 50))
m = models.load(name, 0.05)
_, P, Pd, Pdd = basis.planner_basis(H, 0.05)
q0 = np.array([1.5, -1.8, 1.75, -1.25, -1.6, 0.0])
proj = ProjectionFilter(P, Pd, Pdd, 6, torch.device("cpu"))
xi = proj(torch.tensor(np.random.default_rng(20250632).normal(0, np.sqrt(10.003), (n, 66)).astype(np.float32)),
          proj.boundary(q0, np.zeros(6), np.zeros(6), n), 10).cuda()
e = Engine(m, H, n, Pd)
st = torch.zeros(n, dtype=torch.int32, device="cuda")
c4 = torch.empty((n, 4), device="cuda")
th = torch.empty((n, 6 * H), device="cuda")
td = torch.empty((n, 6 * H), device="cuda")
if os.environ.get("THETA", "1") == "0":  # traffic attribution: no theta / thetadot outputs
    th = td = None
key = torch.empty(1, dtype=torch.int64, device="cuda")
args = (xi, MPCR_LAYOUT_XI, q0, (20., 3., 80.), (-0.3, -0.3, 0.5), (0., 1., 0., 0.))
entry, ctrl_mode = os.environ.get("ENTRY", "cost"), os.environ.get("CTRL", "none")
geom_mode, target_mode = os.environ.get("GEOM", "none"), os.environ.get("TARGET", "none")
slotw_mode, stepw_mode = os.environ.get("SLOTW", "none"), os.environ.get("STEPW", "none")
if entry == "state":
    par = torch.as_tensor(Engine.params(*args[2:])).cuda()
    ckw = {}
    if ctrl_mode != "none":
        own = torch.as_tensor(e.model.own_ctrl().astype(np.float32)).cuda()
        ckw = dict(ctrl=own) if ctrl_mode == "const" else dict(ctrl=own.repeat(1, H, 1).contiguous(), ctrl_per_step=True)
    if os.environ.get("START", "0") == "1":
        ckw["start"] = torch.as_tensor(e.pack_state()).cuda()
    if geom_mode != "none":
        own = torch.as_tensor(e.model.geom_poses()[0]).cuda()
        ckw |= (dict(geom_pose=own) if geom_mode == "const"
                else dict(geom_pose=own.repeat(1, H, 1, 1).contiguous(), geom_pose_per_step=True))
    if target_mode != "none":
        t = np.arange(H if target_mode == "sched" else 1) * 0.05
        pos = np.asarray(args[4]) + t[:, None] * np.array([0.2, -0.1, 0.1]) * (12.0 / H)
        rot = np.stack([np.zeros_like(t), np.cos(0.5 * t * (12.0 / H)), np.sin(0.5 * t * (12.0 / H)), np.zeros_like(t)], 1)
        rows = torch.as_tensor(Engine.target_rows(pos, 1.7 * rot)).cuda()
        ckw |= dict(target=rows[0].contiguous()) if target_mode == "const" else dict(target=rows[None].contiguous(),
                                                                                     target_per_step=True)
    if slotw_mode != "none":
        ns4 = (e.nslot + 3) & ~3
        w = np.ones(ns4, np.float32) if slotw_mode == "ones" else np.tile(np.float32([0, 0.25, 1, 2]), ns4 // 4)
        ckw["slot_w"] = torch.as_tensor(w).cuda()
    if stepw_mode != "none":
        a = Engine.step_weights(H) if stepw_mode == "ones" else Engine.step_weights(H, discount=0.85, terminal=4)
        ckw["step_w"] = torch.as_tensor(a).cuda()

    def run(theta=None, thetadot=None, best_key=None, status=None):
        e.rollout_cost_state(xi, MPCR_LAYOUT_XI, par, 1, c4, theta=theta, thetadot=thetadot, best_keys=best_key,
                             status=status, **ckw)
else:
    def run(**kw):
        e.rollout_cost(*args, cost4=c4, **kw)
for _ in range(2):
    run(theta=th, thetadot=td, best_key=key)
torch.cuda.synchronize()
ts = []
for _ in range(int(os.environ.get("R", 10))):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    run(theta=th, thetadot=td, best_key=key)
    b.record()
    torch.cuda.synchronize()
    ts.append(a.elapsed_time(b))
occ = ""
lib = _lib.load()
if hasattr(lib, "mpcr_rollout_occupancy"):
    import ctypes
    info = (ctypes.c_int * 6)()
    lib.mpcr_rollout_occupancy.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    if lib.mpcr_rollout_occupancy(0, info) == 0:
        occ = (f" [narrow {info[0]} blocks/CU, {info[1]} B LDS, {info[2]} VGPR;"
               f" wide {info[3]} blocks/CU, {info[4]} B LDS, {info[5]} VGPR]")
run(theta=th, thetadot=td, best_key=key, status=st)
sv = st.cpu().numpy()
rows = f" rows/step {float((sv >> 11).mean()) / H:.1f} max-rows p50/p90/p99 " + "/".join(
    str(int(np.percentile((sv >> 2) & 255, q))) for q in (50, 90, 99))
tag = (f" {entry}/ctrl={ctrl_mode}/geom={geom_mode}/start={os.environ.get('START', '0')}/target={target_mode}"
       + (f"/slotw={slotw_mode}" if slotw_mode != "none" else "")
       + (f"/stepw={stepw_mode}" if stepw_mode != "none" else "") if entry == "state" else "")
print(f"{os.path.basename(sys.argv[1])}{tag}{occ}{rows} {name} {n}x{H} median {np.median(ts):.3f} ms min {np.min(ts):.3f} "
      f"-> {n / np.median(ts) * 1e3:.0f} rollouts/s  cost0 {float(c4[:, 0].sum()):.6e}")
if os.environ.get("SAVE"):  # outputs of the last launch, for bitwise comparisons between variants
    np.savez(os.environ["SAVE"], c4=c4.cpu().numpy(), th=None if th is None else th.cpu().numpy(), st=sv)
