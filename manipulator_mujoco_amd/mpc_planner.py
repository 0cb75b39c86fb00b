"""Headless closed-loop MPC driver (reference: SBP/mpc_planner.py:14-314).

``run_cem_planner`` keeps the reference's keyword arguments, target-switching
logic, printed status line, CSV names and returned dict.  What differs:

* the plant (``cem.data`` + ``mujoco.mj_step`` on CPU in the reference,
  :109-114,179-180) is ``engine.Plant``: the same model stepped on the GPU by
  the rollout kernel (n = 1, H = 1, fp32 state resident on the device);
* the reference's only implemented branch drives a passive OpenGL viewer
  (:146-233) and its headless branch is a stub (:234-236).  Here the loop is
  headless and runs ``max_ticks`` ticks (the viewer loop ran until the window
  closed); ``show_viewer`` is accepted and ignored.
* target bodies are read from the compiled model (``model.body(name).pos /
  .quat``, :124-125,157-158); the reference's writes to ``target_0``'s body
  pose (:165-166,219-220) go to a host-side override table, since they only
  ever change what later ticks read as the target.
"""

from __future__ import annotations

import argparse
import os
import time

import numpy as np

from .engine import Engine, Plant
from .planner import cem_planner
from .quat_math import quaternion_distance


class _Bodies:
    """``model.body(name).pos / .quat`` with the reference's writes kept host-side."""

    def __init__(self, model):
        self._names = list(model.names["body"])
        self._pos = {n: np.array(model.body_pos[i], dtype=np.float64) for i, n in enumerate(self._names)}
        self._quat = {n: np.array(model.body_quat[i], dtype=np.float64) for i, n in enumerate(self._names)}

    def pos(self, name):
        return self._pos[name].copy()

    def quat(self, name):
        return self._quat[name].copy()

    def set(self, name, pos, quat):
        self._pos[name] = np.array(pos, dtype=np.float64)
        self._quat[name] = np.array(quat, dtype=np.float64)

    def __contains__(self, name):
        return name in self._pos


def hold_ctrl(model, num_dof, hold=True, gripper=None):
    """A ``run_cem_planner(ctrl=...)`` callable for a compiled model.  hold:
    every actuator whose single transmission dof is one of the planner's
    ``num_dof`` controlled dofs gets the plant's current joint position, so a
    position servo holds the pose the plan has reached instead of pulling back
    to its compiled target.  gripper: the control of every actuator with a
    two-dof transmission (the finger pairs).  The rest keep the model's own."""
    nu = int(getattr(model, "nu", 0))
    own = np.asarray(getattr(model, "act_ctrl", np.zeros(nu)), dtype=np.float64).reshape(-1)[:nu]
    ntrn = np.asarray(model.act_ntrn)[:nu]
    dof = np.asarray(model.act_dof).reshape(-1, 2)[:nu]
    qadr = np.asarray(model.act_qadr).reshape(-1, 2)[:nu]
    planned = set(int(v) for v in np.asarray(model.ctrl_dofadr)[:num_dof])
    held = [a for a in range(nu) if ntrn[a] == 1 and int(dof[a, 0]) in planned] if hold else []
    pairs = [a for a in range(nu) if ntrn[a] == 2] if gripper is not None else []

    def ctrl(_tick, plant):
        c = own.copy()
        for a in held:
            c[a] = plant.qpos[qadr[a, 0]]
        for a in pairs:
            c[a] = gripper
        return c

    return ctrl


def moving_obstacle(model, name, velocity, num_steps, timestep):
    """A ``run_cem_planner(geom_poses=...)`` callable for a compiled model:
    static collision geom ``name`` moves at the constant world ``velocity``
    (m/s) from its model pose.  At tick k the plant gets the pose at the tick's
    time, k timestep, and the planner the ``num_steps`` predicted poses of its
    horizon: step j of a rollout, like the plant's step j ticks later, finds
    the geom at (k + j) timestep."""
    from .engine import Model
    mod = Model(model)
    own, ids, fixed = mod.geom_poses()
    row = mod.geom_row(name)
    if not fixed[row]:
        raise ValueError(f"geom {name!r} is not static")
    gid = int(ids[row])
    p0, quat = own[row, :3].astype(np.float64), own[row, 4:].astype(np.float64)
    v = np.asarray(velocity, dtype=np.float64).reshape(3)

    def at(k):
        return mod.pose_rows(own, {gid: (p0 + v * (k * timestep), quat)})

    def poses(tick, _plant):
        return at(tick), np.stack([at(tick + j) for j in range(num_steps)])

    return poses


def moving_target(velocity, num_steps, timestep):
    """A target that translates at the constant world ``velocity`` (m/s), its
    orientation held: a callable ``(tick, pos, rot) -> (pos_now, (pos_traj,
    rot_traj))`` for the pose ``pos`` / ``rot`` the target had when it became
    current, ``tick`` ticks ago.  ``pos_now`` is its position at the tick's
    time, pos + tick timestep velocity; the trajectory holds the ``num_steps``
    predicted poses of the planner's horizon (``compute_cem(target_traj=)``),
    step k at pos + (tick + k) timestep velocity: (num_steps, 3) and
    (num_steps, 4)."""
    v = np.asarray(velocity, dtype=np.float64).reshape(3)

    def at(tick, pos, rot):
        pos, rot = np.asarray(pos, dtype=np.float64).reshape(3), np.asarray(rot, dtype=np.float64).reshape(4)
        k = tick + np.arange(num_steps, dtype=np.float64)
        traj = pos[None, :] + (k * timestep)[:, None] * v[None, :]
        return pos + (tick * timestep) * v, (traj, np.tile(rot, (num_steps, 1)))

    return at


def run_cem_planner(num_dof=None, num_batch=None, num_steps=None, maxiter_cem=None, maxiter_projection=None,
                    w_pos=None, w_rot=None, w_col=None, num_elite=None, timestep=None, initial_qpos=None,
                    target_names=None, show_viewer=None, cam_distance=None, show_contact_points=None,
                    position_threshold=None, rotation_threshold=None, save_data=None, data_dir=None,
                    stop_at_final_target=None, *, max_ticks=100, model_path=None, device=None, graph=True,
                    verbose=True, planner_kwargs=None, plan_from_state=False, ctrl=None, geom_poses=None,
                    hypotheses=None, scenario_worst=None, target_velocity=None, touch_target=False,
                    terminal_weight=None, discount=None):
    """Run the CEM planner in closed loop for ``max_ticks`` ticks (headless).
    plan_from_state: every tick's rollouts start from the plant's full state
    (a device copy of its block) instead of the template state with the arm
    joints set, which is the reference's behaviour and the default.
    ctrl: the actuator controls, nu values in actuator order or a callable
    ``(tick, plant) -> array`` (``hold_ctrl``), given every tick to the plant
    and to the planner's rollouts; None keeps the model's own in both (the
    reference never sets MjData.ctrl).
    geom_poses: the static collision geoms' world poses, a geom-pose block
    (ng, 8) (``Model.geom_poses``, ``Model.pose_rows``) or a callable ``(tick,
    plant) -> block`` (``moving_obstacle``), given every tick to the plant and
    to the planner's rollouts; the callable may return ``(block, schedule)``
    with a per-step schedule (num_steps, ng, 8) for the planner's horizon.
    None keeps the model's poses in both.
    hypotheses: ``[(geom name, (dx, dy, dz)), ...]``, world hypotheses the
    planner prices every candidate in besides the plant's own world (scenario
    0): each adds a scenario in which that static geom is displaced by the
    offset (m, world) from wherever the tick's poses put it
    (``cem_planner(num_scenarios=)``).  scenario_worst: a candidate's cost is
    the mean of its that many largest scenario costs (default: of all).
    target_velocity: from the tick a named target body becomes current, its
    position translates at this constant world velocity (m/s), one timestep
    per tick (``moving_target``): the planner gets the num_steps predicted
    poses of its horizon (``cem_planner(target_schedule=)``), the reached-test
    and the logged cost_g use the pose at the tick's time.  "home" does not
    move.  None: the targets stand still, and nothing changes.
    touch_target: while a named target body is current, the contact slots of
    its collision geoms cost nothing (``cem_planner(collision_weights=)``,
    weight 0): the plan may near and touch the body it is sent to, and every
    other contact costs what it did.  The weights are restored when the target
    switches; "home" exempts nothing.  False: the loop makes the calls it made.
    terminal_weight, discount: the horizon's cost is weighed per step
    (``cem_planner(cost_schedule=)``, ``Engine.step_weights``): step t's terms
    count ``discount**t``, and the last step's position and rotation terms
    ``terminal_weight`` times that.  Staged once, ahead of the first tick.
    Both None: the flat sum, and the loop makes the calls it made."""
    hypotheses = list(hypotheses or [])
    scheduled = terminal_weight is not None or discount is not None
    if initial_qpos is None:
        initial_qpos = [1.5, -1.8, 1.75, -1.25, -1.6, 0]
    if target_names is None:
        target_names = ["target_0", "target_1", "home"]
    if position_threshold is None:
        position_threshold = 0.04
    if rotation_threshold is None:
        rotation_threshold = 0.3
    if stop_at_final_target is None:
        stop_at_final_target = True
    if save_data:
        os.makedirs(data_dir, exist_ok=True)
    log = print if verbose else (lambda *a, **k: None)

    start_time = time.time()
    cem = cem_planner(num_dof=num_dof, num_batch=num_batch, num_steps=num_steps, maxiter_cem=maxiter_cem,
                      w_pos=w_pos, w_rot=w_rot, w_col=w_col, num_elite=num_elite, timestep=timestep,
                      maxiter_projection=maxiter_projection, model_path=model_path, device=device, graph=graph,
                      verbose=verbose, **({"return_rollouts": False} | (planner_kwargs or {})
                                          | ({"plan_from_state": True} if plan_from_state else {})
                                          | ({"actuator_ctrl": True} if ctrl is not None else {})
                                          | ({"geom_poses": "per_step"} if geom_poses is not None or hypotheses
                                             else {})
                                          | ({"num_scenarios": 1 + len(hypotheses), "scenario_worst": scenario_worst}
                                             if hypotheses else {})
                                          | ({"target_schedule": True} if target_velocity is not None else {})
                                          | ({"collision_weights": True} if touch_target else {})
                                          | ({"cost_schedule": True} if scheduled else {})))
    log(f"Initialized CEM Planner: {round(time.time() - start_time, 2)}s")

    model = cem.model
    data = Plant(model, device=cem.device.index)
    cem.data = data
    bodies = _Bodies(model)

    qpos = data.qpos.copy()
    qpos[np.asarray(model.ctrl_qposadr[:num_dof])] = np.asarray(initial_qpos, dtype=np.float64)
    data.set_state(qpos=qpos)
    data.forward()
    ctrl_q = np.asarray(model.ctrl_qposadr[:num_dof])
    ctrl_v = np.asarray(model.ctrl_dofadr[:num_dof])

    xi_mean = np.zeros(cem.nvar)
    init_position = data.site_xpos_tcp
    init_rotation = data.xquat_hande

    # ("home" is no body: the pose the loop started at, as in the loop below --
    # the only target of a model without target bodies, such as the dual arm)
    target_pos = bodies.pos(target_names[0]) if target_names[0] != "home" else init_position
    target_rot = bodies.quat(target_names[0]) if target_names[0] != "home" else init_rotation
    start_time = time.time()
    from_plant = {"state": data} if plan_from_state else {}  # each tick plans from the plant's state

    def apply_ctrl(tick):
        """The tick's controls to the plant; the planner's argument for them."""
        if ctrl is None:
            return {}
        c = np.asarray(ctrl(tick, data) if callable(ctrl) else ctrl, dtype=np.float64).reshape(-1)
        data.set_ctrl(c)
        return {"ctrl": c}

    hyp_rows = []  # (row of the geom-pose block, world offset) per hypothesis
    if hypotheses:
        own_block, _, fixed = data.model.geom_poses()
        for name, d in hypotheses:
            row = data.model.geom_row(name)
            if not fixed[row]:
                raise ValueError(f"hypothesis: geom {name!r} is not static")
            hyp_rows.append((row, np.asarray(d, dtype=np.float32).reshape(3)))

    def apply_geom_poses(tick):
        """The tick's geom poses to the plant; the planner's argument for them
        (with hypotheses: one schedule per scenario, the plant's world first)."""
        if geom_poses is None and not hyp_rows:
            return {}
        sched = None
        if geom_poses is not None:
            g = geom_poses(tick, data) if callable(geom_poses) else geom_poses
            block, sched = g if isinstance(g, tuple) else (g, g)
            data.set_geom_poses(block)
        if not hyp_rows:
            return {"geom_pose": sched}
        base = np.asarray(own_block if sched is None else sched, dtype=np.float32)
        base = np.broadcast_to(base, (num_steps,) + base.shape[-2:])
        scen = np.stack([base] * (1 + len(hyp_rows)))
        for s, (row, d) in enumerate(hyp_rows, start=1):
            scen[s, :, row, :3] += d
        return {"geom_pose": scen}

    def touch_weights(name):
        """The planner's slot weights while ``name`` is the current target: 0
        on the slots of that body's geoms, 1 elsewhere ("home", or a target
        that is no body with collision geoms: all ones)."""
        if not touch_target:
            return {}
        m = cem.engine.model
        try:
            return {"slot_w": m.slot_weights(bodies={name: 0.0}) if name != "home" else m.slot_weights()}
        except ValueError:
            return {"slot_w": m.slot_weights()}

    # the horizon's step weights, staged once: every later tick keeps them
    step_w = ({"step_w": Engine.step_weights(num_steps, discount=1.0 if discount is None else discount,
                                             terminal=1.0 if terminal_weight is None else terminal_weight)}
              if scheduled else {})
    _ = cem.compute_cem(xi_mean, data.qpos[ctrl_q], data.qvel[ctrl_v], data.qacc[ctrl_v], target_pos, target_rot,
                        **from_plant, **apply_ctrl(0), **apply_geom_poses(0), **touch_weights(target_names[0]),
                        **step_w)
    log(f"Compute CEM: {round(time.time() - start_time, 2)}s")

    thetadot = np.zeros(num_dof)
    cost_g_list, cost_list, cost_r_list, cost_c_list, thetadot_list, theta_list = [], [], [], [], [], []
    step_ms, eef_dist = [], []
    target_idx = 0
    current_target = target_names[target_idx]
    target_motion = None if target_velocity is None else moving_target(target_velocity, num_steps, timestep)
    target_since = 0  # the tick the current target became current
    if show_viewer:
        log("No viewer on this build: running the closed loop headless")

    for _tick in range(int(max_ticks)):
        t0 = time.time()
        if current_target != "home":
            target_pos = bodies.pos(current_target)
            target_rot = bodies.quat(current_target)
        else:
            target_pos = init_position
            target_rot = init_rotation
        if current_target == "target_1" and "target_0" in target_names:
            bodies.set("target_0", data.site_xpos_tcp, data.xquat_hande)
        to_target = {}
        if target_motion is not None and current_target != "home":
            target_pos, traj = target_motion(_tick - target_since, target_pos, target_rot)
            to_target = {"target_traj": traj}

        cost, best_cost_g, best_cost_r, best_cost_c, best_vels, best_traj, xi_mean, _, _ = cem.compute_cem(
            xi_mean, data.qpos[ctrl_q], data.qvel[ctrl_v], data.qacc[ctrl_v], target_pos, target_rot, **from_plant,
            **apply_ctrl(_tick), **apply_geom_poses(_tick), **to_target, **touch_weights(current_target))

        thetadot = np.mean(best_vels[1:num_steps - 2], axis=0)
        data.step(thetadot)

        current_cost_g = np.linalg.norm(data.site_xpos_tcp - target_pos)
        current_cost_r = quaternion_distance(data.xquat_hande, target_rot)
        current_cost = np.round(cost, 2)
        step_ms.append((time.time() - t0) * 1000)
        eef_dist.append(float(current_cost_g))
        log(f'Step Time: {"%.0f" % step_ms[-1]}ms | Cost g: {"%.2f" % (float(current_cost_g))}'
            f' | Cost r: {"%.2f" % (float(current_cost_r))} | Cost c: {"%.2f" % (float(best_cost_c))}'
            f' | Cost: {current_cost}')
        log(f"eef_quat: {data.xquat_hande}")
        log(f"target: {current_target}")

        if current_cost_g < position_threshold and current_cost_r < rotation_threshold:
            if target_idx == len(target_names) - 1:
                if stop_at_final_target:
                    log(f"Reached final target: {current_target}. Stopping motion.")
                    thetadot = np.zeros(num_dof)
                    qvel = data.qvel.copy()
                    qvel[ctrl_v] = thetadot
                    data.set_state(qvel=qvel)
                else:
                    target_idx = 0
                    current_target = target_names[target_idx]
                    target_since = _tick + 1
                    log(f"Reached final target. Looping back to first target: {current_target}")
            else:
                target_idx = target_idx + 1
                current_target = target_names[target_idx]
                target_since = _tick + 1
                log(f"Moving to next target: {current_target}")
            if current_target == "home" and "target_0" in target_names:
                bodies.set("target_0", data.site_xpos_tcp, data.xquat_hande)

        cost_g_list.append(best_cost_g)
        cost_r_list.append(best_cost_r)
        cost_c_list.append(best_cost_c)
        thetadot_list.append(thetadot)
        theta_list.append(data.qpos[ctrl_q].copy())
        cost_list.append(current_cost[-1] if isinstance(current_cost, np.ndarray) else current_cost)

    if save_data:
        np.savetxt(f"{data_dir}/costs.csv", cost_list, delimiter=",")
        np.savetxt(f"{data_dir}/thetadot.csv", thetadot_list, delimiter=",")
        np.savetxt(f"{data_dir}/theta.csv", theta_list, delimiter=",")
        np.savetxt(f"{data_dir}/cost_g.csv", cost_g_list, delimiter=",")
        np.savetxt(f"{data_dir}/cost_r.csv", cost_r_list, delimiter=",")
        np.savetxt(f"{data_dir}/cost_c.csv", cost_c_list, delimiter=",")

    return {"cost_g": cost_g_list, "cost_r": cost_r_list, "cost_c": cost_c_list, "cost": cost_list,
            "thetadot": thetadot_list, "theta": theta_list, "step_ms": step_ms, "eef_dist": eef_dist, "target": current_target}


def main(argv=None):  # SBP/mpc_planner.py:256-314
    parser = argparse.ArgumentParser(description="Run CEM planner with configurable parameters (headless)")
    parser.add_argument("--num_dof", type=int, default=6)
    parser.add_argument("--num_batch", type=int, default=1000)
    parser.add_argument("--num_steps", type=int, default=16)
    parser.add_argument("--maxiter_cem", type=int, default=1)
    parser.add_argument("--maxiter_projection", type=int, default=10)
    parser.add_argument("--w_pos", type=float, default=20.0)
    parser.add_argument("--w_rot", type=float, default=3.0)
    parser.add_argument("--w_col", type=float, default=10.0)
    parser.add_argument("--num_elite", type=float, default=0.05)
    parser.add_argument("--timestep", type=float, default=0.05)
    parser.add_argument("--initial_qpos", type=float, nargs="+", default=None)
    parser.add_argument("--no_viewer", action="store_true")
    parser.add_argument("--cam_distance", type=float, default=4)
    parser.add_argument("--no_contact_points", action="store_true")
    parser.add_argument("--position_threshold", type=float, default=0.04)
    parser.add_argument("--rotation_threshold", type=float, default=0.3)
    parser.add_argument("--targets", type=str, nargs="+", default=None)
    parser.add_argument("--save_data", action="store_true")
    parser.add_argument("--data_dir", type=str, default="data")
    parser.add_argument("--continue_after_final", action="store_true")
    parser.add_argument("--max_ticks", type=int, default=100)
    parser.add_argument("--model", type=str, default=None, help="MJCF path or bundled model name")
    parser.add_argument("--no_graph", action="store_true")
    parser.add_argument("--plan_from_state", action="store_true",
                        help="plan each tick from the plant's full state, not the template state")
    parser.add_argument("--ctrl_hold", action="store_true",
                        help="each tick, the servos of the planned joints get the plant's current joint positions")
    parser.add_argument("--gripper", type=float, default=None, metavar="G",
                        help="control of the actuators with a two-dof transmission (the finger pairs)")
    parser.add_argument("--obstacle", nargs=4, default=None, metavar=("NAME", "VX", "VY", "VZ"),
                        help="a named static geom moves at this constant world velocity (m/s): the plant gets its "
                             "pose at each tick's time, the planner the predicted poses of its horizon")
    parser.add_argument("--hypothesis", nargs=4, action="append", default=None, metavar=("NAME", "DX", "DY", "DZ"),
                        help="repeatable: one more world the planner prices every candidate in, with this static geom "
                             "displaced by the offset (m); scenario 0 is the plant's own world")
    parser.add_argument("--scenario_worst", type=int, default=None, metavar="K",
                        help="a candidate's cost is the mean of its K largest scenario costs (default: of all)")
    parser.add_argument("--target_velocity", nargs=3, type=float, default=None, metavar=("VX", "VY", "VZ"),
                        help="a target body, once current, translates at this constant world velocity (m/s): the "
                             "planner gets the predicted poses of its horizon")
    parser.add_argument("--touch_target", action="store_true",
                        help="while a target body is current, contacts with its geoms cost nothing: the plan may touch "
                             "the body it is sent to")
    parser.add_argument("--terminal_weight", type=float, default=None, metavar="K",
                        help="the last step's position and rotation cost count K times (Engine.step_weights)")
    parser.add_argument("--discount", type=float, default=None, metavar="G",
                        help="step t of the horizon counts G**t in every cost term (Engine.step_weights)")
    a = parser.parse_args(argv)
    geom_poses = None
    if a.obstacle is not None:
        from .planner import _resolve_model
        geom_poses = moving_obstacle(_resolve_model(a.model, a.timestep), a.obstacle[0],
                                     [float(x) for x in a.obstacle[1:]], a.num_steps, a.timestep)
    ctrl = None
    if a.ctrl_hold or a.gripper is not None:
        from .planner import _resolve_model
        ctrl = hold_ctrl(_resolve_model(a.model, a.timestep), a.num_dof, hold=a.ctrl_hold, gripper=a.gripper)
    return run_cem_planner(num_dof=a.num_dof, num_batch=a.num_batch, num_steps=a.num_steps,
                           maxiter_cem=a.maxiter_cem, maxiter_projection=a.maxiter_projection, w_pos=a.w_pos,
                           w_rot=a.w_rot, w_col=a.w_col, num_elite=a.num_elite, timestep=a.timestep,
                           initial_qpos=a.initial_qpos, target_names=a.targets, show_viewer=not a.no_viewer,
                           cam_distance=a.cam_distance, show_contact_points=not a.no_contact_points,
                           position_threshold=a.position_threshold, rotation_threshold=a.rotation_threshold,
                           save_data=a.save_data, data_dir=a.data_dir,
                           stop_at_final_target=not a.continue_after_final, max_ticks=a.max_ticks,
                           model_path=a.model, graph=not a.no_graph, plan_from_state=a.plan_from_state,
                           ctrl=ctrl, geom_poses=geom_poses,
                           hypotheses=[(h[0], [float(x) for x in h[1:]]) for h in a.hypothesis or []],
                           scenario_worst=a.scenario_worst, target_velocity=a.target_velocity,
                           touch_target=a.touch_target, terminal_weight=a.terminal_weight, discount=a.discount)


if __name__ == "__main__":
    main()
