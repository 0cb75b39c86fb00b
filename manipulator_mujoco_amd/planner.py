"""Drop-in ``cem_planner`` (reference: SBP/mjx_planner.py:17-406).

Same constructor keywords and the same ``compute_cem`` 9-tuple, so
``run_mpc_planner.py`` / ``mpc_planner.run_cem_planner`` only swap the import.
Per CEM iteration (``cem_iter``, :337-362), every step a HIP kernel of
libmpcr on the current torch stream (no host round trip inside the loop):

  1. L = chol(cov + 0.003 I)                                (:312-316)  mpcr_cem_factor
  2. MVN samples xi = mean + z L^T fused with the ADMM
     projection filter                                      (:180-249)  mpcr_cem_sample_project
  3. thetadot = A_thetadot xi, H physics steps, cost        (:348-354)  mpcr_rollout_cost
  4. elites (stable argsort, NaN last)                      (:305-310)  mpcr_topk
  5. weighted mean/cov update                               (:318-335)  mpcr_cem_update
and finally the best candidate of the last iteration through the packed
argmin key the rollout kernel reduces with an atomic min (:395-402).

With ranks > 1 (``group``), each rank owns num_batch/ranks candidates
(Philox draws keyed by the global candidate index, so the samples are the
single-GPU ones), and steps 4-5 become local top-E -> all-gather of the elite
rows -> the same global top-E and update on every rank (dist.gather_elites);
the best candidate is one 8-byte MIN all-reduce.  With
``graph=True`` the per-iteration kernel sequences are captured in HIP graphs
on the first call (per-tick inputs live in static device buffers).

With ``num_problems=B``, ``compute_cem_batch`` plans B independent problems
(own start state, target, weights, distribution and best key) in one tick:
the same five kernels per iteration, each launched once over all problems,
bitwise what B one-problem planners compute.  There is one tick path: every
planner calls the ``*_multi`` entry points over its B problems, and the
default B = 1 is their ``nprob = 1`` case (the one-problem kernels), which
``compute_cem`` and ``compute_cem_batch`` share, captured graph included.

With ``num_scenarios=S`` each problem makes one plan against S world
hypotheses (scenarios): the samples are drawn and projected once, rolled out
in every scenario's world (its own start state, controls and geom poses) by
one launch, and folded per candidate -- mean, worst case or the mean of the
``scenario_worst`` worst (``Engine.scenario_reduce``) -- into the costs the
elites, the update and the best key see.  The default S = 1 is the path above.

Reference behaviours kept on purpose, each behind a flag:
  * elites are gathered from the *unprojected* samples (``elite_from_filtered=False``)
  * the sampling key is not advanced across calls (fixed ``seed`` per call)
  * ``init_vel`` only enters the boundary vector (the rollout overwrites qvel[:6])
  * a NaN cost wins the final argmin, sorts last among elites.
The MVN draws use Philox4x32-10 keyed by (seed, iteration), not JAX's
threefry, so samples are statistically equivalent but not bit-identical to
the reference's.
"""

from __future__ import annotations

import os
import time

import numpy as np

from . import _lib, basis, models
from .cem import CemContext, topk, topk_multi
from .engine import MPCR_LAYOUT_XI, Engine
from .mjcf import load_model

DEFAULT_MODEL = "planner_scene"  # SBP/ur5e_hande_mjx/scene.xml (:100)


def _resolve_model(model_path, timestep):
    if model_path is None:
        return models.load(DEFAULT_MODEL, timestep)
    if model_path in models.BUNDLES:
        return models.load(model_path, timestep)
    return load_model(model_path, timestep)


class cem_planner:  # noqa: N801 (reference name)
    """Reference constructor keywords plus, keyword-only:

    model_path          MJCF path or bundled model name (default: the
                        planner scene the reference hard-wires, :100)
    device              GPU ordinal (default LOCAL_RANK)
    seed                Philox key of the MVN draws (fixed per call, §0.6)
    elite_from_filtered gather elites from the projected samples instead
    graph               capture each CEM iteration's kernels in HIP graphs on
                        the first call and replay them on later calls
    group               torch.distributed process group: ``num_batch`` is
                        the GLOBAL batch, sharded evenly over the ranks
                        (SURVEY.md §8e); None = single GPU unless an
                        initialised default group has more than one rank
    gather_rollouts     with ranks > 1, all-gather the full thetadot/theta
                        arrays of the 9-tuple (default: this rank's shard)
    return_rollouts     False: the 9-tuple's thetadot/theta (iters x N x 6H,
                        what the closed loop discards) are returned as None
                        instead of being copied to the host every tick
    capture_exchange    with graph=True and an RCCL group, capture the elite
                        all-gathers in the tick's graph (default); False
                        captures each iteration's device segment and runs the
                        exchange eagerly between the replays (as with gloo)
    num_problems        independent problems planned per ``compute_cem_batch``
                        tick (own start state, target, weights, distribution
                        and best key each); ``num_batch`` stays the candidates
                        per problem.  One rank only
    seed_step           problem p draws with the Philox key seed + p seed_step
                        (0: every problem the same draws), i.e. what a
                        planner built with that seed draws
    plan_from_state     rollouts start from a full state per problem (object,
                        fingers, other arm; ``compute_cem(state=...)``) instead
                        of the model's template state with only the arm joints
                        set, which is what the reference does (:105-107) and
                        the default here.  The state lives in a static device
                        buffer, initialised to the template, that the
                        (captured) rollouts read each tick
    actuator_ctrl       the rollouts read the actuator controls per problem
                        from a static device buffer (``compute_cem(ctrl=...)``),
                        initialised to the model's own, instead of the values
                        the model was compiled with.  Independent of
                        plan_from_state; both may be on
    geom_poses          the rollouts read the static collision geoms' world
                        poses per problem from a static device buffer
                        (``compute_cem(geom_pose=...)``), initialised to the
                        model's own (``Model.geom_poses``), instead of the
                        poses the model was compiled with: True, one block
                        (ng, 8) per problem; "per_step", one block per step of
                        the horizon (H, ng, 8), an obstacle that moves during
                        it.  Independent of the two above
    target_schedule     the rollouts price the end effector against a target
                        pose per step of the horizon, read per problem from a
                        static device buffer of target rows (H, 8)
                        (``compute_cem(target_traj=...)``), instead of the one
                        pose of the parameter block.  Every tick stages it: a
                        tick without a trajectory holds ``target_pos`` /
                        ``target_rot`` over the horizon and plans what a
                        planner without the flag plans, bit for bit
    collision_weights   the rollouts price each robot-masked contact slot with
                        a weight read per problem (and scenario) from a static
                        device buffer of slot-weight blocks
                        (``compute_cem(slot_w=...)``, ``Model.slot_weights``),
                        initialised to ones, instead of charging every contact
                        alike: 0 permits a contact, 2 charges it double.  A
                        planner with the flag and nothing staged plans what a
                        planner without it plans, bit for bit
    cost_schedule       the rollouts weigh each step's cost terms with a row
                        a_pos a_rot a_col 0 read per problem (and scenario)
                        from a static device buffer of step-weight schedules
                        (``compute_cem(step_w=...)``, ``Engine.step_weights``),
                        initialised to ones, instead of summing the horizon
                        flat: a terminal weight, a discount, a term that
                        counts only on arrival.  A planner with the flag and
                        nothing staged plans what a planner without it plans,
                        bit for bit
    num_scenarios       world hypotheses per problem (default 1: none).  With
                        S > 1 the state, control and geom-pose buffers hold
                        one block per problem and scenario -- ``compute_cem``'s
                        ``state`` / ``ctrl`` / ``geom_pose`` take a leading (S,
                        ...) axis (``state``: a list of S), an input without
                        it goes to every scenario -- every candidate is rolled
                        out in each, and the CEM step runs once per problem on
                        the folded costs.  ``scenario_costs`` keeps the
                        per-scenario ones; the 9-tuple's trajectories are
                        scenario 0's, the nominal one.  One rank only
    scenario_worst      k: a candidate's cost is the mean of its k largest
                        scenario costs (default S, the mean; 1, the worst case)
    """

    def __init__(self, num_dof=None, num_batch=None, num_steps=None, timestep=None, maxiter_cem=None,
                 num_elite=None, w_pos=None, w_rot=None, w_col=None, maxiter_projection=None, *,
                 model_path=None, device=None, seed=0, elite_from_filtered=False, graph=False, group=None,
                 gather_rollouts=False, return_rollouts=True, capture_exchange=True, verbose=True,
                 num_problems=1, seed_step=0, plan_from_state=False, actuator_ctrl=False, geom_poses=False,
                 num_scenarios=1, scenario_worst=None, target_schedule=False, collision_weights=False,
                 cost_schedule=False):
        import torch
        import torch.distributed as tdist

        self.num_scenarios = int(num_scenarios)
        if not 1 <= self.num_scenarios <= 64:
            raise ValueError(f"num_scenarios={self.num_scenarios} outside [1, 64]")
        self.scenario_worst = self.num_scenarios if scenario_worst is None else int(scenario_worst)
        if not 1 <= self.scenario_worst <= self.num_scenarios:
            raise ValueError(f"scenario_worst={self.scenario_worst} outside [1, num_scenarios={self.num_scenarios}]")
        if not torch.cuda.is_available():
            raise _lib.MpcrError("cem_planner needs a gfx950 GPU (no CPU fallback)")
        self.num_dof = int(num_dof)
        self.num_batch = int(num_batch)
        self.num = int(num_steps)
        self.t = float(timestep)
        self.maxiter_cem = int(maxiter_cem)
        self.maxiter_projection = int(maxiter_projection) if maxiter_projection is not None else 0
        self.num_elite = float(num_elite)
        self.ellite_num = int(self.num_elite * self.num_batch)
        self.cost_weights = {"w_pos": w_pos, "w_rot": w_rot, "w_col": w_col}
        self.seed = int(seed)
        self.elite_from_filtered = bool(elite_from_filtered)
        self.graph = bool(graph)
        self.gather_rollouts = bool(gather_rollouts)
        self.return_rollouts = bool(return_rollouts)
        self.capture_exchange = bool(capture_exchange)
        # CEM constants (:84-97)
        self.v_max, self.a_max, self.p_max = 0.8, 1.8, np.pi
        self.alpha_mean, self.alpha_cov, self.lamda = 0.6, 0.6, 10.0

        # candidate shards
        self.group = group
        if group is None and tdist.is_available() and tdist.is_initialized() and tdist.get_world_size() > 1:
            self.group = tdist.group.WORLD
        self.world = tdist.get_world_size(self.group) if self.group is not None else 1
        self.rank = tdist.get_rank(self.group) if self.group is not None else 0
        if self.num_batch % self.world:
            raise ValueError(f"num_batch={self.num_batch} must split evenly over {self.world} ranks")
        self.n_local = self.num_batch // self.world
        self.num_problems = int(num_problems)
        self.seed_step = int(seed_step)
        if self.num_problems < 1:
            raise ValueError(f"num_problems={self.num_problems} must be at least 1")
        if self.num_problems > 1 and self.world > 1:
            raise ValueError(f"num_problems={self.num_problems} with {self.world} ranks: sharded multi-problem "
                             "planning is not supported")
        if self.num_scenarios > 1 and self.world > 1:
            raise ValueError(f"num_scenarios={self.num_scenarios} with {self.world} ranks: sharded scenario planning "
                             "is not supported")
        self.exchange = self.world > 1  # elites through gather_elites (forced on one rank in tests)
        self.index_base = self.rank * self.n_local

        self.t_fin = self.num * self.t
        self.tot_time, self.P, self.Pdot, self.Pddot = basis.planner_basis(self.num, self.t)
        self.nvar_single = self.P.shape[1]
        self.nvar = self.nvar_single * self.num_dof

        dev = int(device) if device is not None else int(os.environ.get("LOCAL_RANK", 0))
        self.device = torch.device("cuda", dev)
        self.model = _resolve_model(model_path, self.t)
        self.model_path = getattr(self.model, "source", model_path)
        if self.model.nctrl != self.num_dof:
            raise ValueError(f"model controls {self.model.nctrl} dofs, num_dof={self.num_dof}")
        self.data = None  # the closed-loop plant: mpc_planner.run_cem_planner (engine.Plant)
        self.hande_id = self.model.hande_body
        self.tcp_id = self.model.tcp_site
        n = self.n_local
        B = self.num_problems
        S = self.num_scenarios
        self.engine = Engine(self.model, self.num, B * S * n, self.Pdot, device=dev)
        self.cem = CemContext(self.P, self.Pdot, self.Pddot, self.num_dof, B * n, device=dev, num_problems=B)
        f32 = dict(dtype=torch.float32, device=self.device)
        H, it_n = self.num, self.maxiter_cem
        pb = (B,) if B > 1 else ()  # the leading problem axis of every device buffer (none for one problem)
        sb = (S,) if S > 1 else ()  # the scenario axis of the per-world buffers, after the problem's
        self._key = torch.empty(B, dtype=torch.int64, device=self.device)
        self._eye10 = 10.0 * torch.eye(self.nvar, **f32)  # xi_cov (:386)
        self._mean = torch.empty(pb + (self.nvar,), **f32)
        self._cov = torch.empty(pb + (self.nvar, self.nvar), **f32)
        self._xs = torch.empty(pb + (n, self.nvar), **f32)  # xi_samples
        self._xf = torch.empty(pb + (n, self.nvar), **f32)  # xi_filtered
        self._idx = torch.empty(pb + (max(self.ellite_num, 1),), dtype=torch.int32, device=self.device)
        self._beq = torch.empty(pb + (5 * self.num_dof,), **f32)
        self._par = torch.zeros(pb + sb + (20,), **f32)  # init_pos | weights | target (Engine.params)
        self._thetadot = torch.empty((it_n,) + pb + (n, self.num_dof * H), **f32)
        self._theta = torch.empty((it_n,) + pb + (n, self.num_dof * H), **f32)
        self._costs = torch.empty((it_n,) + pb + (n, 4), **f32)
        self._mean_in = torch.empty(pb + (self.nvar,), **f32)
        # every candidate's cost in every scenario; _costs then holds the fold
        self._scen_costs = torch.empty((it_n, B, S, n, 4), **f32) if S > 1 else None
        # one start state block per problem (Engine.pack_state), the template until a tick stages another
        self.plan_from_state = bool(plan_from_state)
        self._state = None
        if self.plan_from_state:
            self._state = torch.as_tensor(self.engine.pack_state()).to(self.device).repeat(B * S, 1).contiguous()
            self._state = self._state.view((B,) + sb + (-1,))
        # one control block per problem (actuator order), the model's own until a tick stages another
        self.actuator_ctrl = bool(actuator_ctrl)
        self._ctrl = None
        if self.actuator_ctrl:
            own = self.engine.model.own_ctrl().astype(np.float32)
            if own.size == 0:
                raise ValueError("actuator_ctrl: the model has no actuators")
            self._ctrl = torch.as_tensor(own).to(self.device).repeat(B * S, 1).contiguous().view((B,) + sb + (-1,))
        # one geom-pose block per problem, or per problem and step: the model's own until a tick stages another
        if geom_poses not in (False, True, "per_step"):
            raise ValueError(f"geom_poses={geom_poses!r}: False, True or 'per_step'")
        self.geom_poses = geom_poses
        self._gpose = None
        if geom_poses:
            own, _, fixed = self.engine.model.geom_poses()
            if not fixed.any():
                raise ValueError("geom_poses: the model has no static collision geom")
            rep = (B * S, H, 1, 1) if geom_poses == "per_step" else (B * S, 1, 1)
            self._gpose = torch.as_tensor(own).to(self.device).repeat(*rep).contiguous()
            self._gpose = self._gpose.view((B,) + sb + tuple(self._gpose.shape[1:]))
        # one target row per problem (and scenario) and step: every tick stages it (_stage_targets)
        self.target_schedule = bool(target_schedule)
        self._target = torch.zeros((B,) + sb + (H, 8), **f32) if self.target_schedule else None
        # one slot-weight block per problem (and scenario), rows padded to a multiple of 4 floats: ones until
        # a tick stages another
        self.collision_weights = bool(collision_weights)
        self._slot_w = None
        if self.collision_weights:
            if self.engine.nslot == 0:
                raise ValueError("collision_weights: the model has no robot-masked contact slot")
            self._slot_w = torch.ones((B,) + sb + ((self.engine.nslot + 3) & ~3,), **f32)
        # one step-weight schedule per problem (and scenario), H rows of 4: ones until a tick stages another
        self.cost_schedule = bool(cost_schedule)
        self._step_w = torch.ones((B,) + sb + (H, 4), **f32) if self.cost_schedule else None
        self._graphs = None
        if verbose and self.rank == 0:
            self.print_info()

    @property
    def scenario_costs(self):
        """(maxiter_cem, num_problems, num_scenarios, n, 4) device tensor:
        every candidate's cost row in every scenario, as the last tick left
        it (the 9-tuple's costs are their fold); None without scenarios."""
        return self._scen_costs

    def print_info(self):
        _lib.load()
        print(f"\n Default backend: gfx950 (libmpcr)\n Model path: {self.model_path}"
              f"\n Timestep: {self.t}\n CEM Iter: {self.maxiter_cem}\n Number of batches: {self.num_batch}"
              f"\n Number of steps per trajectory: {self.num}\n Time per trajectory: {self.t_fin}"
              + (f"\n Ranks: {self.world} x {self.n_local} candidates" if self.world > 1 else ""))

    # ------------------------------------------------------------------
    # one CEM iteration = two device segments around the (multi-rank) elite
    # exchange; each segment is a fixed kernel sequence on the current
    # stream, so it can be captured in a HIP graph and replayed
    def _seg_sample_rollout(self, it):
        """compute_xi_samples + projection + rollout + cost (:345-354)."""
        bounds = (self.v_max, self.a_max, self.p_max)
        if it == 0:
            self._mean.copy_(self._mean_in)
            self._cov.copy_(self._eye10)  # (broadcast over the problems)
        last = it == self.maxiter_cem - 1
        # one workgroup / grid row per problem; one problem (B = 1, this
        # rank's shard of it from index_base on) is the same calls
        B, n = self.num_problems, self.n_local
        self.cem.factor_multi(self._cov.view(B, self.nvar, self.nvar), 0.003)
        self.cem.sample_project_multi(B, n, self._mean, self.seed, it, self._beq, self.maxiter_projection, bounds,
                                      rho=1.0, seed_step=self.seed_step, xi_samples=self._xs, out=self._xf,
                                      index_base=self.index_base)
        out = dict(theta=self._theta[it], thetadot=self._thetadot[it], best_keys=self._key if last else None,
                   index_base=self.index_base)
        S = self.num_scenarios
        if S > 1:
            # every scenario of a problem rolls out the problem's samples in its
            # own world; the fold leaves one cost row per candidate (and the keys)
            flat = lambda t: None if t is None else t.view((B * S,) + tuple(t.shape[2:]))  # noqa: E731
            self.engine.rollout_cost_scenarios(self._xf.view(B * n, self.nvar), MPCR_LAYOUT_XI, self._par, B, S,
                                               self._scen_costs[it], worst=self.scenario_worst, cost4=self._costs[it],
                                               start=flat(self._state), ctrl=flat(self._ctrl),
                                               geom_pose=flat(self._gpose),
                                               geom_pose_per_step=self.geom_poses == "per_step",
                                               target=flat(self._target), target_per_step=self.target_schedule,
                                               slot_w=self._slot_w, step_w=self._step_w, **out)
        else:
            # one launch over the problems, reading each one's start / control /
            # geom-pose block where the planner stages one (None: the model's own)
            self.engine.rollout_cost_state(self._xf.view(B * n, self.nvar), MPCR_LAYOUT_XI, self._par, B,
                                           self._costs[it], start=self._state, ctrl=self._ctrl,
                                           geom_pose=self._gpose, geom_pose_per_step=self.geom_poses == "per_step",
                                           target=self._target, target_per_step=self.target_schedule,
                                           slot_w=self._slot_w, step_w=self._step_w, **out)

    def _seg_local_update(self, it):
        """compute_ellite_samples + compute_mean_cov on one rank (:355-360)."""
        src = self._xf if self.elite_from_filtered else self._xs
        B, n = self.num_problems, self.n_local
        idx = self._idx.view(B, self.ellite_num)
        topk_multi(self.engine, self._costs[it], B, self.ellite_num, stride=4, out=idx)
        self.cem.update_multi(src.view(B, n, self.nvar), self._costs[it], 4, idx, self.lamda, self.alpha_mean,
                              self.alpha_cov, self._mean, self._cov, reg=1e-4)

    def _topk_fn(self, cost, k):
        return topk(self.engine, cost, k, stride=1)

    def _exchange_update(self, it):
        """Sharded elites: all-gather local top-E rows, select, replicated update."""
        from .dist import gather_elites
        src = self._xf if self.elite_from_filtered else self._xs
        g_cost, g_xi, sel = gather_elites(self._costs[it, :, 0].contiguous(), src, self.ellite_num, self._topk_fn,
                                          group=self.group)
        self.cem.update(g_xi, g_cost, 1, sel, self.lamda, self.alpha_mean, self.alpha_cov, self._mean, self._cov,
                        reg=1e-4)

    def _run_iterations(self):
        import torch
        it_n = self.maxiter_cem
        if not self.graph:
            for it in range(it_n):
                self._seg_sample_rollout(it)
                if not self.exchange:
                    self._seg_local_update(it)
                else:
                    self._exchange_update(it)
            return
        if self._graphs is None:
            # warm up on a side stream (allocator / library state), then capture
            s = torch.cuda.Stream(self.device)
            s.wait_stream(torch.cuda.current_stream(self.device))
            with torch.cuda.stream(s):
                self._run_eager_once()
            torch.cuda.current_stream(self.device).wait_stream(s)
            torch.cuda.synchronize(self.device)
            graphs = []
            if not self.exchange or (self.capture_exchange and self._exchange_capturable()):
                # the whole tick in one graph; with an RCCL group the elite
                # all-gathers are captured too (device buffers, stream-ordered)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    for it in range(it_n):
                        self._seg_sample_rollout(it)
                        if not self.exchange:
                            self._seg_local_update(it)
                        else:
                            self._exchange_update(it)
                graphs.append(g)
            else:  # gloo (host-staged) exchange: device segments in graphs, the exchange between them eager
                for it in range(it_n):
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g):
                        self._seg_sample_rollout(it)
                    graphs.append(g)
            self._graphs = graphs
        if len(self._graphs) == 1:
            self._graphs[0].replay()
        else:
            for it in range(it_n):
                self._graphs[it].replay()
                self._exchange_update(it)

    def _exchange_capturable(self):
        """RCCL collectives on device tensors can be captured into the tick's
        graph; host-staged (gloo) ones cannot."""
        import torch.distributed as dist
        return dist.get_backend(self.group) == "nccl"

    def _run_eager_once(self):
        graph, self.graph = self.graph, False
        try:
            self._run_iterations()
        finally:
            self.graph = graph

    def _stage(self, xi_mean, init_pos, init_vel, init_acc, target_pos, target_rot, weights):
        """The tick's inputs, one row per problem, into the static device
        buffers the (captured) kernels read."""
        import torch
        B, d = self.num_problems, self.num_dof
        self._mean_in.copy_(torch.as_tensor(np.ascontiguousarray(xi_mean)).view(self._mean_in.shape))
        z = np.zeros((B, d))
        st = np.stack([init_pos, init_vel, init_acc, z, z], axis=2)  # state_term per problem (:374-384)
        # compute_boundary_vec (:174-178)
        self._beq.copy_(torch.as_tensor(st.reshape(B, 5 * d).astype(np.float32)).view(self._beq.shape))
        par = np.stack([Engine.params(init_pos[p], weights[p], target_pos[p], target_rot[p]) for p in range(B)])
        if self.num_scenarios > 1:  # every scenario of a problem has the problem's parameters
            par = np.repeat(par[:, None], self.num_scenarios, axis=1)
        self._par.copy_(torch.as_tensor(par).view(self._par.shape))

    def _stage_states(self, states):
        """Each problem's start state into its block of the static buffer: a
        ``Plant`` (device-to-device copy of its block), ``(qpos, qvel[,
        qacc_warmstart])`` arrays, or None, which keeps what is staged."""
        import torch
        if states is None:
            return
        if not self.plan_from_state:
            raise ValueError("a start state needs a planner built with plan_from_state=True")
        if len(states) != self.num_problems:
            raise ValueError(f"{len(states)} start states for {self.num_problems} problem(s)")
        S = self.num_scenarios
        for p, st in enumerate(states):
            if st is None:
                continue
            # scenarios: a list holds one start state per scenario, anything else goes to each
            per = st if S > 1 and isinstance(st, list) else [st] * S
            if len(per) != S:
                raise ValueError(f"{len(per)} start states for {S} scenarios")
            for sc, e in enumerate(per):
                if e is None:
                    continue
                dst = self._state[p, sc] if S > 1 else self._state[p]
                if hasattr(e, "copy_state"):
                    e.copy_state(dst)
                else:
                    if not 2 <= len(e) <= 3:
                        raise ValueError("a start state is a Plant or (qpos, qvel[, qacc_warmstart])")
                    dst.copy_(torch.as_tensor(self.engine.pack_state(*e)))

    def _stage_ctrls(self, ctrls):
        """Each problem's actuator controls (nu values, actuator order) into
        its block of the static buffer; None keeps what is staged.  Every rank
        of a sharded planner stages the same block."""
        import torch
        if ctrls is None:
            return
        if not self.actuator_ctrl:
            raise ValueError("actuator controls need a planner built with actuator_ctrl=True")
        if len(ctrls) != self.num_problems:
            raise ValueError(f"{len(ctrls)} control blocks for {self.num_problems} problem(s)")
        nu = self._ctrl.shape[-1]
        full = tuple(self._ctrl.shape[1:])  # (nu,), or (S, nu) with scenarios
        for p, c in enumerate(ctrls):
            if c is None:
                continue
            c = np.asarray(c, dtype=np.float32)
            if c.shape != (nu,) and c.shape != full:
                raise ValueError(f"a control block holds nu={nu} values" + (f" (or {full}, one row per scenario)"
                                                                             if len(full) == 2 else "")
                                 + f", got shape {c.shape}")
            self._ctrl[p].copy_(torch.as_tensor(np.broadcast_to(c, full).copy()))

    def _stage_geom_poses(self, blocks):
        """Each problem's geom-pose block into the static buffer: (ng, 8) or,
        for a planner built with geom_poses="per_step", also (H, ng, 8), one
        block per step (a single block is held over the horizon).  None keeps
        what is staged.  Every rank of a sharded planner stages the same
        block."""
        import torch
        if blocks is None:
            return
        if not self.geom_poses:
            raise ValueError("geom poses need a planner built with geom_poses=True or 'per_step'")
        if len(blocks) != self.num_problems:
            raise ValueError(f"{len(blocks)} geom-pose blocks for {self.num_problems} problem(s)")
        # what one problem holds, and one scenario of it: with scenarios a
        # leading (S, ...) axis, one block (or schedule) per scenario
        whole = tuple(self._gpose.shape[1:])
        full = whole[1:] if self.num_scenarios > 1 else whole
        for p, g in enumerate(blocks):
            if g is None:
                continue
            g = np.asarray(g.cpu() if hasattr(g, "cpu") else g, dtype=np.float32)
            if g.shape != full and g.shape != full[-2:] and g.shape != whole:
                raise ValueError(f"a geom-pose block is {full[-2:]}"
                                 + (f" or {full}" if len(full) == 3 else "")
                                 + (f" or {whole}, one per scenario" if whole != full else "") + f", got {g.shape}")
            self._gpose[p].copy_(torch.as_tensor(np.broadcast_to(g, whole).copy()))

    def _stage_slot_weights(self, blocks):
        """Each problem's slot-weight block into the static buffer: (nslot,)
        (``Model.slot_weights``) or, with scenarios, also (S, nslot), one per
        scenario.  None keeps what is staged (at first ones).  Every rank of a
        sharded planner stages the same block."""
        import torch
        if blocks is None:
            return
        if not self.collision_weights:
            raise ValueError("slot weights need a planner built with collision_weights=True")
        if len(blocks) != self.num_problems:
            raise ValueError(f"{len(blocks)} slot-weight blocks for {self.num_problems} problem(s)")
        ns, S = self.engine.nslot, self.num_scenarios
        for p, w in enumerate(blocks):
            if w is None:
                continue
            w = np.asarray(w.cpu() if hasattr(w, "cpu") else w, dtype=np.float32)
            if w.shape != (ns,) and not (S > 1 and w.shape == (S, ns)):
                raise ValueError(f"a slot-weight block is ({ns},)" + (f" or ({S}, {ns}), one per scenario" if S > 1 else "")
                                 + f"; got {w.shape}")
            self._slot_w[p][..., :ns].copy_(torch.as_tensor(np.broadcast_to(w, tuple(self._slot_w.shape[1:-1]) + (ns,))
                                                            .copy()))

    def _stage_step_weights(self, scheds):
        """Each problem's step-weight schedule into the static buffer: (H, 4)
        (``Engine.step_weights``) or, with scenarios, also (S, H, 4), one per
        scenario.  None keeps what is staged (at first ones).  Every rank of a
        sharded planner stages the same schedule."""
        import torch
        if scheds is None:
            return
        if not self.cost_schedule:
            raise ValueError("step weights need a planner built with cost_schedule=True")
        if len(scheds) != self.num_problems:
            raise ValueError(f"{len(scheds)} step-weight schedules for {self.num_problems} problem(s)")
        H, S = self.num, self.num_scenarios
        for p, a in enumerate(scheds):
            if a is None:
                continue
            a = np.asarray(a.cpu() if hasattr(a, "cpu") else a, dtype=np.float32)
            if a.shape != (H, 4) and not (S > 1 and a.shape == (S, H, 4)):
                raise ValueError(f"a step-weight schedule is ({H}, 4)" + (f" or ({S}, {H}, 4), one per scenario"
                                                                          if S > 1 else "") + f"; got {a.shape}")
            self._step_w[p].copy_(torch.as_tensor(np.broadcast_to(a, tuple(self._step_w.shape[1:])).copy()))

    def _stage_targets(self, trajs, target_pos, target_rot):
        """Each problem's target schedule into the static buffer: (H, 8) target
        rows (``Engine.target_rows``) or a (pos (H, 3), rot (H, 4)) pair; with
        scenarios also a leading (S, ...) axis, one schedule per scenario.
        Unlike the other blocks, None does not keep what is staged: the tick's
        target_pos / target_rot, given every tick, are held over the horizon.
        Every rank of a sharded planner stages the same schedule."""
        import torch
        if not self.target_schedule:
            if trajs is not None and any(t is not None for t in trajs):
                raise ValueError("a target trajectory needs a planner built with target_schedule=True")
            return
        B, S, H = self.num_problems, self.num_scenarios, self.num
        if trajs is None:
            trajs = [None] * B
        if len(trajs) != B:
            raise ValueError(f"{len(trajs)} target trajectories for {B} problem(s)")
        whole = tuple(self._target.shape[1:])  # (H, 8), or (S, H, 8) with scenarios
        out = np.empty((B,) + whole, dtype=np.float32)
        for p, tr in enumerate(trajs):
            if tr is None:
                out[p] = Engine.target_rows(target_pos[p], target_rot[p])
                continue
            if isinstance(tr, (tuple, list)) and len(tr) == 2:
                pos, rot = (np.asarray(x.cpu() if hasattr(x, "cpu") else x, dtype=np.float32) for x in tr)
                if pos.shape[-1:] != (3,) or rot.shape[-1:] != (4,) or pos.shape[:-1] != rot.shape[:-1]:
                    raise ValueError(f"a target trajectory pair is (pos (H, 3), rot (H, 4)); got {pos.shape}, {rot.shape}")
                tr = Engine.target_rows(pos, rot)
            tr = np.asarray(tr.cpu() if hasattr(tr, "cpu") else tr, dtype=np.float32)
            if tr.shape != (H, 8) and tr.shape != whole:
                raise ValueError(f"a target trajectory is ({H}, 8) rows or a (pos ({H}, 3), rot ({H}, 4)) pair"
                                 + (f", or {whole}, one per scenario" if S > 1 else "") + f"; got {tr.shape}")
            out[p] = tr
        self._target.copy_(torch.as_tensor(out))

    def compute_cem(self, xi_mean, init_pos=(1.5, -1.8, 1.75, -1.25, -1.6, 0.0), init_vel=None, init_acc=None,
                    target_pos=None, target_rot=None, state=None, ctrl=None, geom_pose=None, target_traj=None,
                    slot_w=None, step_w=None):
        """One MPC tick of CEM (SBP/mjx_planner.py:364-406). Returns the reference 9-tuple (numpy).
        state (planners built with plan_from_state): the full state the
        rollouts start from, a ``Plant`` or ``(qpos, qvel[, qacc_warmstart])``;
        None keeps the one staged last (at first the template).  init_pos
        still sets the arm joints.  ctrl (planners built with actuator_ctrl):
        the actuator controls of the rollouts, nu values; None keeps the ones
        staged last (at first the model's own).  geom_pose (planners built
        with geom_poses): the static geoms' poses of the rollouts, a
        geom-pose block (ng, 8) or, "per_step", (H, ng, 8); None keeps the
        one staged last (at first the model's own).  target_traj (planners
        built with target_schedule): the target pose of every step of the
        horizon, (H, 8) target rows or a (pos (H, 3), rot (H, 4)) pair, with
        scenarios also (S, H, 8); None holds target_pos / target_rot over
        the horizon.  slot_w (planners built with collision_weights): what
        each contact slot costs, (nslot,) (``Model.slot_weights``) or, with
        scenarios, also (S, nslot); None keeps the block staged last (at
        first ones).  step_w (planners built with cost_schedule): the
        horizon's step weights, (H, 4) (``Engine.step_weights``) or, with
        scenarios, also (S, H, 4); None keeps the schedule staged last (at
        first ones)."""
        import torch

        from . import dist as mdist

        if self.num_problems > 1:
            raise ValueError(f"this planner was built with num_problems={self.num_problems}: "
                             "use compute_cem_batch (compute_cem plans one problem)")
        d = self.num_dof
        H = self.num
        init_pos = np.asarray(init_pos, np.float64)[:d]
        init_vel = np.zeros(d) if init_vel is None else np.asarray(init_vel, np.float64)[:d]
        init_acc = np.zeros(d) if init_acc is None else np.asarray(init_acc, np.float64)[:d]
        target_pos = np.zeros(3) if target_pos is None else np.asarray(target_pos, np.float64)
        target_rot = np.zeros(4) if target_rot is None else np.asarray(target_rot, np.float64)
        w = (self.cost_weights["w_pos"], self.cost_weights["w_rot"], self.cost_weights["w_col"])

        if self.ellite_num < 1:
            raise ValueError("num_elite * num_batch must select at least one elite")
        self._stage(np.asarray(xi_mean, np.float32).reshape(1, self.nvar), init_pos[None], init_vel[None],
                    init_acc[None], target_pos[None], target_rot[None], [w])
        self._stage_states(None if state is None else [state])
        self._stage_ctrls(None if ctrl is None else [ctrl])
        self._stage_geom_poses(None if geom_pose is None else [geom_pose])
        self._stage_targets(None if target_traj is None else [target_traj], target_pos[None], target_rot[None])
        self._stage_slot_weights(None if slot_w is None else [slot_w])
        self._stage_step_weights(None if step_w is None else [step_w])
        self._run_iterations()

        costs, theta, thetadot = self._costs, self._theta, self._thetadot
        cost_min = torch.amin(costs[:, :, 0], dim=1)
        if self.world > 1:
            mdist.allreduce_min_key(self._key, group=self.group)
            cost_min = torch.as_tensor(mdist.allgather_min(cost_min, group=self.group))
        idx, _ = _lib.decode_key(int(self._key.item()) & 0xFFFFFFFFFFFFFFFF)
        owner, li = divmod(idx, self.n_local)
        best = torch.empty(4 + 2 * d * H, dtype=torch.float32, device=self.device)
        if owner == self.rank:
            best[:4] = costs[-1, li]
            best[4:4 + d * H] = thetadot[-1, li]
            best[4 + d * H:] = theta[-1, li]
        if self.world > 1:
            mdist.broadcast(best, owner, group=self.group)
            if self.gather_rollouts and self.return_rollouts:
                theta, thetadot = (self._gather_all(x) for x in (theta, thetadot))
        if not self.return_rollouts:
            theta = thetadot = None
        best_vels = best[4:4 + d * H].reshape(d, H).T
        best_traj = best[4 + d * H:].reshape(d, H).T
        out = (cost_min, best[1], best[2], best[3], best_vels, best_traj, self._mean, thetadot, theta)
        return tuple(o.cpu().numpy() if isinstance(o, torch.Tensor) else o for o in out)

    def compute_cem_batch(self, xi_mean, init_pos, init_vel=None, init_acc=None, target_pos=None, target_rot=None,
                          weights=None, states=None, ctrls=None, geom_poses=None, target_trajs=None,
                          slot_ws=None, step_ws=None):
        """One MPC tick of ``num_problems`` independent CEM problems in one
        batched sequence of launches (each kernel of ``compute_cem`` once,
        over every problem): xi_mean (B, nvar), init_pos / init_vel /
        init_acc (B, num_dof), target_pos (B, 3), target_rot (B, 4), weights
        (B, 3) (w_pos, w_rot, w_col; default the constructor's for every
        problem).  Returns the 9 entries of ``compute_cem``, each stacked
        over the problems on a new leading axis: ``out[j][p]`` is bitwise
        entry j of ``compute_cem`` on a planner with seed ``seed + p
        seed_step`` given problem p's arguments.  states (planners built with
        plan_from_state): one start state per problem, each as ``compute_cem``'s
        ``state`` (a None entry keeps that problem's).  ctrls (planners built
        with actuator_ctrl): one control block per problem, likewise.
        geom_poses (planners built with geom_poses): one geom-pose block per
        problem, likewise.  target_trajs (planners built with
        target_schedule): one target trajectory per problem as
        ``compute_cem``'s ``target_traj``; a None entry holds that problem's
        target_pos / target_rot over the horizon.  slot_ws (planners built
        with collision_weights): one slot-weight block per problem as
        ``compute_cem``'s ``slot_w``; a None entry keeps that problem's.
        step_ws (planners built with cost_schedule): one step-weight schedule
        per problem as ``compute_cem``'s ``step_w``, likewise."""
        import torch

        B, d, H, n, it_n = self.num_problems, self.num_dof, self.num, self.n_local, self.maxiter_cem
        if self.world > 1:
            raise ValueError("compute_cem_batch runs on one rank")
        if self.ellite_num < 1:
            raise ValueError("num_elite * num_batch must select at least one elite")

        def rows(x, cols, name, dtype=np.float64):
            a = np.zeros((B, cols), dtype) if x is None else np.asarray(x, dtype)
            if a.ndim != 2 or a.shape[0] != B or a.shape[1] < cols:
                raise ValueError(f"{name} must be ({B}, {cols}), got {a.shape}")
            return a[:, :cols]

        xi_mean = rows(xi_mean, self.nvar, "xi_mean", np.float32)
        init_pos = rows(init_pos, d, "init_pos")
        init_vel, init_acc = rows(init_vel, d, "init_vel"), rows(init_acc, d, "init_acc")
        target_pos, target_rot = rows(target_pos, 3, "target_pos"), rows(target_rot, 4, "target_rot")
        if weights is None:
            weights = [[self.cost_weights["w_pos"], self.cost_weights["w_rot"], self.cost_weights["w_col"]]] * B
        weights = rows(weights, 3, "weights", np.float32)

        self._stage(xi_mean, init_pos, init_vel, init_acc, target_pos, target_rot, weights)
        self._stage_states(states)
        self._stage_ctrls(ctrls)
        self._stage_geom_poses(geom_poses)
        self._stage_targets(target_trajs, target_pos, target_rot)
        self._stage_slot_weights(slot_ws)
        self._stage_step_weights(step_ws)
        self._run_iterations()

        # each problem's best candidate of the last iteration: the low word of
        # its key is the index within the problem; one gather, one transfer
        costs = self._costs.view(it_n, B, n, 4)
        theta, thetadot = self._theta.view(it_n, B, n, d * H), self._thetadot.view(it_n, B, n, d * H)
        li = self._key & 0xFFFFFFFF
        flat = li + n * torch.arange(B, dtype=torch.int64, device=self.device)
        packed = torch.cat([torch.amin(costs[..., 0], dim=2).T,
                            costs[-1].reshape(B * n, 4).index_select(0, flat),
                            thetadot[-1].reshape(B * n, d * H).index_select(0, flat),
                            theta[-1].reshape(B * n, d * H).index_select(0, flat),
                            self._mean.view(B, self.nvar)], dim=1).cpu().numpy()
        o = it_n
        cost_min, best = packed[:, :o], packed[:, o:o + 4]
        best_vels = packed[:, o + 4:o + 4 + d * H].reshape(B, d, H).transpose(0, 2, 1)
        best_traj = packed[:, o + 4 + d * H:o + 4 + 2 * d * H].reshape(B, d, H).transpose(0, 2, 1)
        mean = packed[:, o + 4 + 2 * d * H:]
        td = th = None
        if self.return_rollouts:
            td, th = (x.permute(1, 0, 2, 3).cpu().numpy() for x in (thetadot, theta))
        return (cost_min, best[:, 1], best[:, 2], best[:, 3], best_vels, best_traj, mean, td, th)

    def _gather_all(self, x):
        from .dist import all_gather
        it_n, n, c = x.shape
        return all_gather(x, self.group).permute(1, 0, 2, 3).reshape(it_n, self.world * n, c)


def main():  # SBP/mjx_planner.py:408-428 (with its unpacking bug fixed)
    t0 = time.time()
    opt = cem_planner(num_dof=6, num_batch=2000, num_steps=50, maxiter_cem=30, w_pos=1, w_rot=0.5, w_col=10,
                      num_elite=0.05, timestep=0.05, maxiter_projection=10)
    t1 = time.time()
    out = opt.compute_cem(np.zeros(opt.nvar))
    print(f"Total time: {round(time.time() - t0, 2)}s")
    print(f"Compute CEM time: {round(time.time() - t1, 2)}s")
    return out


if __name__ == "__main__":
    main()
