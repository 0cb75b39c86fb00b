"""Python handle on a libmpcr engine (one compiled model on one GPU).

``Engine.rollout_cost`` is the fused hot path: Bernstein basis -> H physics
steps -> cost, one wavefront per candidate.
Accepts either torch device tensors (zero-copy, launched on the current
torch stream) or host numpy arrays (staged through the engine's buffers).
"""

from __future__ import annotations

import ctypes
import math

import numpy as np

from . import _lib
from ._lib import MPCR_F_DEVICE_PTRS, MPCR_F_RESET_BEST, MPCR_LAYOUT_THETADOT, MPCR_LAYOUT_XI, check


def _f32p(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _check_tensor(name, t, device=None):
    """What every device-pointer call asks of a tensor it hands to the library."""
    import torch
    if (not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous()
            or (device is not None and t.device != device)):
        raise ValueError(f"{name} must be a contiguous float32 CUDA tensor"
                         + (" on the input's device" if device is not None else ""))


def _stream_arg(t, stream):
    """The stream a call runs on: the current torch stream of ``t``'s device
    unless one is given."""
    import torch
    return ctypes.c_void_p(stream if stream is not None else torch.cuda.current_stream(t.device).cuda_stream)


def _call_tail(t, reset_best, stream):
    """The (flags, stream) that end a device-pointer call."""
    return MPCR_F_DEVICE_PTRS | (MPCR_F_RESET_BEST if reset_best else 0), _stream_arg(t, stream)


class Model:
    """Host model handle (``mpcr_model``) built from a compiled model."""

    def __init__(self, compiled):
        lib = _lib.load()
        self.compiled = compiled
        blob = compiled.to_blob()
        self._blob = ctypes.create_string_buffer(blob, len(blob))
        h = ctypes.c_void_p()
        check(lib.mpcr_model_from_blob(self._blob, len(blob), ctypes.byref(h)))
        self.handle = h

    def hull_starts(self, R: int = 0, exact: bool = False):
        """The support start table engines build for this model
        (mpcr_model_hull_starts; R = 0: the library's MPCR_LUT_R): per-geom
        first cell (-1: no hull), the global hull vertex of every cell and,
        with exact, the cells whose climb the engine skips."""
        lib = _lib.load()
        adr = np.empty(max(1, self.compiled.ngeom), dtype=np.int32)
        i32p, u8p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint8)
        n = lib.mpcr_model_hull_starts(self.handle, R, adr.ctypes.data_as(i32p), None, None, 0)
        check(int(min(n, 0)))
        cells = np.empty(max(1, n), dtype=np.int32)
        ex = np.empty(max(1, n), dtype=np.uint8)
        check(int(min(lib.mpcr_model_hull_starts(self.handle, R, None, cells.ctypes.data_as(i32p),
                                                 ex.ctypes.data_as(u8p) if exact else None, n), 0)))
        out = (adr[:self.compiled.ngeom], cells[:n])
        return out + (ex[:n].astype(bool),) if exact else out

    def actuators(self):
        """``mpcr_model_actuators``: (nu, ctrlrange (nu, 2), limited (nu,) bool)."""
        lib = _lib.load()
        nu = ctypes.c_int()
        check(lib.mpcr_model_actuators(self.handle, ctypes.byref(nu), None, None))
        rng = np.zeros((max(nu.value, 1), 2))
        lim = np.zeros(max(nu.value, 1), dtype=np.int32)
        check(lib.mpcr_model_actuators(self.handle, None, rng.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                       lim.ctypes.data_as(ctypes.POINTER(ctypes.c_int))))
        return nu.value, rng[:nu.value], lim[:nu.value].astype(bool)

    def own_ctrl(self):
        """The model's own controls (act_ctrl), nu values."""
        nu = int(getattr(self.compiled, "nu", 0))
        return np.asarray(getattr(self.compiled, "act_ctrl", np.zeros(nu)), dtype=np.float64).reshape(-1)[:nu].copy()

    def clamp_ctrl(self, ctrl):
        """``ctrl`` clamped to ctrlrange where the model limits it, as the
        library and the kernel clamp it."""
        nu, rng, lim = self.actuators()
        c = np.array(ctrl, dtype=np.float64).reshape(-1)[:nu]
        return np.where(lim, np.clip(c, rng[:, 0], rng[:, 1]), c)

    def geom_poses(self):
        """``mpcr_model_geom_poses``: (block (ng, 8) float32, model_geom_ids
        (ng,), is_static (ng,) bool) -- the model's own geom-pose block in the
        device model's geom order, row ``x y z 0 | qw qx qy qz``, exactly the
        static poses an engine of this model holds."""
        lib = _lib.load()
        ng = ctypes.c_int()
        check(lib.mpcr_model_geom_poses(self.handle, ctypes.byref(ng), None, None, None))
        n = max(ng.value, 1)
        block = np.zeros((n, 8), dtype=np.float32)
        ids, fixed = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
        ip = ctypes.POINTER(ctypes.c_int)
        check(lib.mpcr_model_geom_poses(self.handle, None, _f32p(block), ids.ctypes.data_as(ip),
                                        fixed.ctypes.data_as(ip)))
        return block[:ng.value], ids[:ng.value], fixed[:ng.value].astype(bool)

    def geom_row(self, name_or_id):
        """The geom-pose block's row of a model geom, by name or model geom id."""
        g = name_or_id
        if isinstance(g, str):
            names = self.compiled.names["geom"]
            found = [i for i, n in (names.items() if isinstance(names, dict) else enumerate(names)) if n == g]
            if not found:
                raise KeyError(f"no geom named {g!r}")
            g = int(found[0])
        _, ids, _ = self.geom_poses()
        rows = np.nonzero(ids == int(g))[0]
        if rows.size == 0:
            raise KeyError(f"geom {name_or_id!r} is in no collision pair: it has no row")
        return int(rows[0])

    def pose_rows(self, block, poses):
        """A copy of ``block`` (..., ng, 8) with the rows of ``poses`` = {geom
        name or id: (pos, quat)} replaced: the world position and quaternion
        (w x y z), normalised in fp64 and rounded to fp32 once.  Only static
        geoms have a row that is read."""
        out = np.array(block, dtype=np.float32, copy=True)
        _, _, fixed = self.geom_poses()
        for key, (pos, quat) in poses.items():
            r = self.geom_row(key)
            if not fixed[r]:
                raise ValueError(f"geom {key!r} is not static: its row is not read")
            q = np.asarray(quat, dtype=np.float64).reshape(4)
            out[..., r, 0:3] = np.asarray(pos, dtype=np.float64).reshape(3)
            out[..., r, 3] = 0.0
            out[..., r, 4:8] = q / np.sqrt(np.sum(q * q))
        return out

    def slots(self):
        """``mpcr_model_slots``: (geom1, geom2, pair), each (nslot,) int32 --
        per robot-masked contact slot, in slot order, its two geoms as rows of
        ``geom_poses`` (the device model's geom order) and the collision pair
        that owns it.  Needs the library, no GPU."""
        lib = _lib.load()
        ns = ctypes.c_int()
        check(lib.mpcr_model_slots(self.handle, ctypes.byref(ns), None, None, None))
        out = [np.zeros(max(ns.value, 1), dtype=np.int32) for _ in range(3)]
        ip = ctypes.POINTER(ctypes.c_int)
        check(lib.mpcr_model_slots(self.handle, None, *(a.ctypes.data_as(ip) for a in out)))
        return tuple(a[:ns.value] for a in out)

    def slot_weights(self, geoms=None, bodies=None, default=1.0):
        """A slot-weight block (``Engine.rollout_cost_state(slot_w=)``), float32
        (nslot,): a slot's weight is the product of its two geoms' weights.
        ``geoms`` maps a geom name or model geom id to a weight, ``bodies`` a
        body name to the weight of all its collision geoms (a geom named in
        ``geoms`` keeps that weight); every other geom weighs ``default``.
        Unknown names raise ``ValueError``."""
        g1, g2, _ = self.slots()
        _, ids, _ = self.geom_poses()
        gw = np.full(max(ids.size, 1), float(default), dtype=np.float64)
        names = self.compiled.names["body"]
        names = list(names.values()) if isinstance(names, dict) else list(names)
        bodyid = np.asarray(self.compiled.geom_bodyid).reshape(-1)
        for key, w in (bodies or {}).items():
            if key not in names:
                raise ValueError(f"no body named {key!r}")
            rows = np.nonzero(bodyid[ids] == names.index(key))[0]
            if rows.size == 0:
                raise ValueError(f"body {key!r} has no collision geom")
            gw[rows] = float(w)
        for key, w in (geoms or {}).items():
            try:
                gw[self.geom_row(key)] = float(w)
            except KeyError as e:
                raise ValueError(str(e.args[0])) from None
        return (gw[g1] * gw[g2]).astype(np.float32)

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                _lib.load().mpcr_model_free(self.handle)
        except Exception:  # interpreter shutdown
            pass
        self.handle = None


def state_layout():
    """``mpcr_state_layout``: the offset of each part of a state block (qpos,
    qvel, qacc_warmstart, qacc, eef) and the block's ``size``, in floats.
    Needs the library, no GPU."""
    o = [ctypes.c_int() for _ in range(5)]
    size = _lib.load().mpcr_state_layout(*(ctypes.byref(x) for x in o))
    return dict(zip(("qpos", "qvel", "qacc_warmstart", "qacc", "eef"), (x.value for x in o)), size=size)


def pack_state(compiled_model, qpos=None, qvel=None, qacc_warmstart=None):
    """``Engine.pack_state`` for a compiled model (no GPU needed)."""
    m, lay = compiled_model, state_layout()
    blk = np.zeros(lay["size"], dtype=np.float32)
    for name, x, n, dflt in (("qpos", qpos, int(m.nq), m.qpos_init), ("qvel", qvel, int(m.nv), m.qvel_init),
                             ("qacc_warmstart", qacc_warmstart, int(m.nv), np.zeros(int(m.nv)))):
        a = np.asarray(dflt if x is None else x, dtype=np.float64).reshape(-1)
        if a.size < n:
            raise ValueError(f"{name} needs {n} entries, got {a.size}")
        blk[lay[name]:lay[name] + n] = a[:n]
    return blk


def unpack_state(compiled_model, block):
    """The parts of state blocks (..., size), host array or tensor moved to the
    host: dict of qpos (..., nq), qvel / qacc_warmstart / qacc (..., nv), eef (..., 7)."""
    lay = state_layout()
    b = np.asarray(block.cpu() if hasattr(block, "cpu") else block)
    nq, nv = int(compiled_model.nq), int(compiled_model.nv)
    return {k: b[..., lay[k]:lay[k] + n] for k, n in (("qpos", nq), ("qvel", nv), ("qacc_warmstart", nv),
                                                      ("qacc", nv), ("eef", 7))}


class Engine:
    def __init__(self, compiled_model, num_steps: int, max_n: int, pdot: np.ndarray, device: int = 0):
        lib = _lib.load()
        self.model = Model(compiled_model)
        self.H = int(num_steps)
        self.max_n = int(max_n)
        self.nctrl = int(compiled_model.nctrl)
        self.nslot = int(compiled_model.nslot)
        self.nu = int(getattr(compiled_model, "nu", 0))
        self._ngeom = None
        pdot = np.ascontiguousarray(pdot, dtype=np.float32)
        if pdot.shape[0] != self.H:
            raise ValueError(f"pdot has {pdot.shape[0]} rows, expected num_steps={self.H}")
        self.nbasis = pdot.shape[1]
        self.device = int(device)
        h = ctypes.c_void_p()
        check(lib.mpcr_engine_create(self.model.handle, self.device, self.max_n, self.H, pdot.ctypes.data,
                                     self.nbasis, ctypes.byref(h)))
        self.handle = h

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                _lib.load().mpcr_engine_free(self.handle)
        except Exception:  # interpreter shutdown
            pass
        self.handle = None

    def dispatches(self, n: int) -> int:
        """Kernel dispatches one rollout_cost over n candidates issues
        (mpcr_engine_dispatches: horizon segments x candidate groups for large
        dual-arm batches, else 1) -- per-dispatch profiler counters times this
        are per call."""
        out = ctypes.c_int()
        check(_lib.load().mpcr_engine_dispatches(self.handle, int(n), ctypes.byref(out)))
        return int(out.value)

    @staticmethod
    def _vec(x, n, dtype):
        a = np.zeros(n, dtype=dtype)
        x = np.asarray(x, dtype=dtype).reshape(-1)
        a[: x.size] = x
        return a

    def rollout_cost(self, inp, layout: int, q0, w, ptgt, qtgt, cost4=None, theta=None, thetadot=None,
                     best_key=None, index_base: int = 0, status=None, reset_best: bool = True, stream=None):
        """Run the fused rollout.

        torch path: ``inp``/outputs are CUDA tensors (float32, contiguous);
        ``best_key`` an int64 tensor of one element.  numpy path: host arrays.
        Returns cost4 (and fills the optional outputs in place).
        """
        lib = _lib.load()
        q0 = self._vec(q0, 8, np.float64)
        w = self._vec(w, 3, np.float32)
        pt = self._vec(ptgt, 3, np.float32)
        qt = self._vec(qtgt, 4, np.float32)
        dp = ctypes.POINTER(ctypes.c_double)
        try:
            import torch
            is_torch = isinstance(inp, torch.Tensor)
        except ImportError:  # pragma: no cover
            is_torch = False
        n = int(inp.shape[0])
        if is_torch:
            _check_tensor("input", inp)
            if cost4 is None:
                cost4 = torch.empty((n, 4), dtype=torch.float32, device=inp.device)
            check(lib.mpcr_rollout_cost(self.handle, _ptr(inp), layout, n, q0.ctypes.data_as(dp), _f32p(w),
                                        _f32p(pt), _f32p(qt), _ptr(cost4), _ptr(theta), _ptr(thetadot),
                                        _ptr(best_key), int(index_base), _ptr(status),
                                        *_call_tail(inp, reset_best, stream)))
            return cost4
        inp = np.ascontiguousarray(inp, dtype=np.float32)
        if cost4 is None:
            cost4 = np.zeros((n, 4), dtype=np.float32)
        key = np.zeros(1, dtype=np.uint64) if best_key is not None else None
        hp = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None else None  # noqa: E731
        check(lib.mpcr_rollout_cost(self.handle, hp(inp), layout, n, q0.ctypes.data_as(dp), _f32p(w), _f32p(pt),
                                    _f32p(qt), hp(cost4), hp(theta), hp(thetadot), hp(key), int(index_base),
                                    hp(status), 0, None))
        if best_key is not None:
            best_key[...] = key
        return cost4

    @staticmethod
    def params(q0, w, ptgt, qtgt):
        """The 20-float parameter block ``mpcr_rollout_cost_dp`` reads on the
        device: init_pos[8] | w[3], 0 | ptgt[3], 0 | qtgt[4]."""
        p = np.zeros(20, dtype=np.float32)
        q0 = np.asarray(q0, dtype=np.float64).reshape(-1)
        p[: q0.size] = q0
        p[8:11] = np.asarray(w, dtype=np.float32).reshape(-1)[:3]
        p[12:15] = np.asarray(ptgt, dtype=np.float32).reshape(-1)[:3]
        p[16:20] = np.asarray(qtgt, dtype=np.float32).reshape(-1)[:4]
        return p

    @staticmethod
    def target_rows(pos, rot):
        """Target rows (``mpcr_rollout_cost_target``), float32 ``(..., 8)``: x y
        z 0 | qw qx qy qz from ``pos`` ``(..., 3)`` and ``rot`` ``(..., 4)``,
        broadcast against each other.  Only the layout: the kernel normalises
        the quaternion."""
        pos, rot = np.asarray(pos, dtype=np.float32), np.asarray(rot, dtype=np.float32)
        if pos.shape[-1:] != (3,) or rot.shape[-1:] != (4,):
            raise ValueError(f"target_rows takes (..., 3) and (..., 4); got {pos.shape} and {rot.shape}")
        lead = np.broadcast_shapes(pos.shape[:-1], rot.shape[:-1])
        rows = np.zeros(lead + (8,), dtype=np.float32)
        rows[..., :3] = pos
        rows[..., 4:] = rot
        return rows

    @staticmethod
    def step_weights(H, discount=1.0, terminal=1.0, running=(1.0, 1.0, 1.0)):
        """A step-weight schedule (``Engine.rollout_cost_state(step_w=)``),
        float32 ``(H, 4)``: row t is a_pos a_rot a_col 0 with ``a[t, k] =
        float32(running[k] * discount**t)``, computed in fp64, and the last
        row's a_pos and a_rot multiplied by ``terminal`` -- a terminal weight
        on the pose terms, a discount over the horizon, a running weight per
        term (``running=(0, 0, 1), terminal=...`` with ``discount=1`` would
        zero the pose terms of every row, the last included: give the
        terminal row by hand then).  Column 3 is zero."""
        H = int(H)
        run = np.asarray(running, dtype=np.float64).reshape(-1)
        if H < 1 or run.shape != (3,):
            raise ValueError(f"step_weights takes H >= 1 and three running weights; got H={H}, running={running!r}")
        a = np.zeros((H, 4), dtype=np.float64)
        a[:, :3] = run[None, :] * (float(discount) ** np.arange(H, dtype=np.float64))[:, None]
        a[H - 1, :2] *= float(terminal)
        return a.astype(np.float32)

    @staticmethod
    def state_layout():
        """``mpcr_state_layout``: the offsets of a state block's parts and its
        size in floats (no GPU needed)."""
        return state_layout()

    def pack_state(self, qpos=None, qvel=None, qacc_warmstart=None):
        """A float32 state block (host) holding qpos (nq), qvel (nv) and
        qacc_warmstart (nv); a part left out is the model's template state's
        (qpos_init, qvel_init, a zero warm start), the rest of the block 0."""
        return pack_state(self.model.compiled, qpos, qvel, qacc_warmstart)

    def _rollout_dp(self, nprob, inp, layout, params, cost4, theta, thetadot, best_keys, index_base, status,
                    reset_best, stream, state=None, ctrl=None, ctrl_per_step=False, geom_pose=None,
                    geom_pose_per_step=False, target=None, target_per_step=False, slot_w=None, step_w=None):
        """nprob None: ``rollout_cost_dp`` (its own C entry, which takes an
        empty batch); else ``rollout_cost_multi`` or, with state = (start,
        final_state), ``rollout_cost_state`` (``mpcr_rollout_cost_world``,
        whichever of its blocks are set; with a target schedule
        ``mpcr_rollout_cost_target``)."""
        _check_tensor("input", inp)
        _check_tensor("cost4", cost4)
        n, lib = int(inp.shape[0]), _lib.load()
        fn, shape = lib.mpcr_rollout_cost_dp, (n,)
        if nprob is not None:
            if nprob < 1 or n % nprob:
                raise ValueError(f"input rows ({n}) must split evenly over nprob={nprob} problems")
            if best_keys is not None and best_keys.numel() < nprob:
                raise ValueError("best_keys needs nprob elements")
            fn, shape = lib.mpcr_rollout_cost_multi, (nprob, n // nprob)
        args = (self._params_arg(params, nprob or 1),)
        if state is not None:
            fn = lib.mpcr_rollout_cost_world
            args += self._state_args(nprob, n, inp, *state, ctrl, ctrl_per_step, geom_pose, geom_pose_per_step)
            if target is not None or slot_w is not None or step_w is not None:
                fn = lib.mpcr_rollout_cost_target
                args += self._block_args("target", target, (8,), nprob, inp.device, target_per_step)
            if slot_w is not None or step_w is not None:
                fn = lib.mpcr_rollout_cost_slotw
                slot_w, sw_args = self._slot_w_args(slot_w, nprob, inp.device)
                args += sw_args
            if step_w is not None:
                fn = lib.mpcr_rollout_cost_stepw
                args += self._block_args("step_w", step_w, (self.H, 4), nprob, inp.device)[:2]
        check(fn(self.handle, _ptr(inp), layout, *shape, *args, _ptr(cost4), _ptr(theta), _ptr(thetadot),
                 _ptr(best_keys), int(index_base), _ptr(status), *_call_tail(inp, reset_best, stream)))
        return cost4

    @staticmethod
    def _params_arg(params, nprob):
        _check_tensor("params", params)
        if params.numel() < 20 * nprob:
            raise ValueError("params needs 20 floats per rollout problem")
        return _ptr(params)

    def _state_args(self, nprob, n, inp, start, final_state, ctrl, ctrl_per_step, geom_pose, geom_pose_per_step):
        """What ``mpcr_rollout_cost_world`` and ``mpcr_rollout_cost_scenarios``
        take from ``start`` to the geom-pose strides, validated for ``nprob``
        rollout problems of ``n`` candidates in all."""
        dev = inp.device
        # (a call without state blocks, a plain planner's, does not ask the library for their size)
        blk = self.state_layout()["size"] if start is not None or final_state is not None else 0
        if final_state is not None:
            _check_tensor("final_state", final_state, dev)
            if final_state.numel() != n * blk or final_state.shape[-1] != blk:
                raise ValueError(f"final_state must be ({n}, {blk})")
        start_args = self._block_args("start", start, (blk,), nprob, dev, by_numel=True)[:2]
        return (*start_args, _ptr(final_state),
                *self._block_args("ctrl", ctrl, (self.nu,), nprob, dev, ctrl_per_step),
                *self._block_args("geom_pose", geom_pose, (self.ngeom, 8), nprob, dev, geom_pose_per_step))

    def _block_args(self, name, t, unit, nprob, device, per_step=False, by_numel=False):
        """(pointer, problem stride, step stride) of a block tensor: one unit
        for every problem, ``(nprob,) + unit`` with one per problem or, with
        per_step, ``(nprob, H) + unit`` with one per problem and step.
        by_numel: any shape of that many elements whose last dimension is the
        unit's.  None: no block."""
        if t is None:
            return None, 0, 0
        _check_tensor(name, t, device)
        size = math.prod(unit)
        shapes = [(nprob, self.H) + unit] if per_step else [unit, (nprob,) + unit]
        if by_numel:
            shape_ok = t.numel() in (size, nprob * size) and t.shape[-1] == unit[-1]
        else:
            shape_ok = tuple(t.shape) in shapes or unit == (0,)  # no actuators: the library refuses the call
        if not shape_ok:
            raise ValueError(f"{name} must be " + " or ".join(map(str, shapes))
                             + (f" (with {name}_per_step)" if per_step else "") + f"; got {tuple(t.shape)}")
        if per_step:
            return _ptr(t), self.H * size, size
        return _ptr(t), size if nprob > 1 and t.numel() == nprob * size else 0, 0

    def _slot_w_args(self, t, nprob, device):
        """(the tensor the call reads, (pointer, problem stride)) of a
        slot-weight tensor: ``(nslot,)`` for every rollout problem or ``(nprob,
        nslot)`` with one block each.  Rows of nslot floats are padded (a copy,
        with ones) to the next multiple of 4, the block's alignment; rows
        already that long -- a planner's own buffer -- are passed as they are."""
        import torch
        if t is None:  # (a call that carries only a later block)
            return None, (None, 0)
        _check_tensor("slot_w", t, device)
        ns4 = (self.nslot + 3) & ~3
        if t.dim() not in (1, 2) or t.shape[-1] not in (self.nslot, ns4):
            raise ValueError(f"slot_w must be ({self.nslot},) or ({nprob}, {self.nslot}) (rows may be padded to "
                             f"{ns4}); got {tuple(t.shape)}")
        if t.shape[-1] != ns4:
            t = torch.nn.functional.pad(t, (0, ns4 - t.shape[-1]), value=1.0).contiguous()
        return t, self._block_args("slot_w", t, (ns4,), nprob, device)[:2]

    @property
    def ngeom(self):
        """The device model's collision geoms: the rows of a geom-pose block."""
        if self._ngeom is None:
            self._ngeom = int(self.model.geom_poses()[0].shape[0])
        return self._ngeom

    def rollout_cost_dp(self, inp, layout: int, params, cost4, theta=None, thetadot=None, best_key=None,
                        index_base: int = 0, status=None, reset_best: bool = True, stream=None):
        """``rollout_cost`` with the per-call arguments in a device tensor
        (``params``, 20 float32, see ``Engine.params``): graph-capturable."""
        return self._rollout_dp(None, inp, layout, params, cost4, theta, thetadot, best_key, index_base, status,
                                reset_best, stream)

    def rollout_cost_multi(self, inp, layout: int, params, nprob: int, cost4, theta=None, thetadot=None,
                           best_keys=None, index_base: int = 0, status=None, reset_best: bool = True, stream=None):
        """``nprob`` independent problems in one launch (``mpcr_rollout_cost_multi``):
        ``inp`` holds nprob * n_per rows, problem p owning rows [p n_per,
        (p + 1) n_per); ``params`` is (nprob, 20), one ``Engine.params`` block
        per problem; ``best_keys`` an int64 tensor of nprob elements whose key
        p carries ``index_base`` + the index within problem p.  Bitwise the
        ``rollout_cost_dp`` calls on the slices; one problem runs the very
        kernel ``rollout_cost_dp`` runs.  Graph-capturable."""
        return self._rollout_dp(int(nprob), inp, layout, params, cost4, theta, thetadot, best_keys, index_base,
                                status, reset_best, stream)

    def rollout_cost_state(self, inp, layout: int, params, nprob: int, cost4, start=None, final_state=None,
                           theta=None, thetadot=None, best_keys=None, index_base: int = 0, status=None,
                           reset_best: bool = True, stream=None, ctrl=None, ctrl_per_step: bool = False,
                           geom_pose=None, geom_pose_per_step: bool = False, target=None,
                           target_per_step: bool = False, slot_w=None, step_w=None):
        """``rollout_cost_multi`` from a given full state and / or returning
        the final states (``mpcr_rollout_cost_state``).  ``start``: a device
        tensor of one state block (``pack_state``, ``Plant.copy_state``) shared
        by every problem, or (nprob, block) with one per problem -- its qpos,
        qvel and qacc_warmstart replace the template state, the parameter
        block's init_pos still overrides the arm joints.  ``final_state``: a
        device tensor (nprob * n_per, block) that receives, per candidate,
        what a plant holds after the same steps.  Both None:
        ``rollout_cost_multi``.  Graph-capturable; a replay reads ``start``
        afresh.  ``ctrl`` (``mpcr_rollout_cost_ctrl``): the actuator controls
        as a device tensor in actuator order, (nu,) for every problem or
        (nprob, nu) with one block per problem, or with ``ctrl_per_step``
        (nprob, H, nu), one row per step; clamped to the model's ctrlrange in
        the kernel and read when it runs.  None keeps the model's own.
        ``geom_pose`` (``mpcr_rollout_cost_world``): the static collision
        geoms' world poses as a device tensor of geom-pose blocks
        (``Model.geom_poses``, ``Model.pose_rows``), (ng, 8) for every problem
        or (nprob, ng, 8) with one block per problem, or with
        ``geom_pose_per_step`` (nprob, H, ng, 8), one block per step; used as
        it is and read when the kernel runs.  None keeps the model's poses.
        ``target`` (``mpcr_rollout_cost_target``): the pose the cost's goal and
        rotation terms read, as a device tensor of target rows
        (``Engine.target_rows``), (8,) for every problem or (nprob, 8) with one
        per problem, or with ``target_per_step`` (nprob, H, 8), one row per
        step; the quaternion may have any norm.  It replaces the parameter
        block's ptgt / qtgt and is read when the kernel runs.  None keeps the
        parameter block's target.
        ``slot_w`` (``mpcr_rollout_cost_slotw``): what each robot-masked
        contact slot costs, a device tensor of slot-weight blocks
        (``Model.slot_weights``), (nslot,) for every problem or (nprob, nslot)
        with one per problem: cost_c sums w[slot] times the slot's terms, the
        values used as they are.  Cost only -- every other output is bitwise
        the call without it, and ones are that call exactly -- and read when
        the kernel runs.  None prices every slot at 1.
        ``step_w`` (``mpcr_rollout_cost_stepw``): when the cost's terms
        matter, a device tensor of step-weight schedules
        (``Engine.step_weights``), (H, 4) for every problem or (nprob, H, 4)
        with one per problem; row t is a_pos a_rot a_col 0 and prices step
        t's position, rotation and collision terms, the values used as they
        are.  Cost only -- ones are the call without it exactly, theta,
        thetadot, final states and statuses never move -- and read when the
        kernel runs.  None prices every step at 1."""
        return self._rollout_dp(int(nprob), inp, layout, params, cost4, theta, thetadot, best_keys, index_base,
                                status, reset_best, stream, state=(start, final_state), ctrl=ctrl,
                                ctrl_per_step=ctrl_per_step, geom_pose=geom_pose,
                                geom_pose_per_step=geom_pose_per_step, target=target,
                                target_per_step=target_per_step, slot_w=slot_w, step_w=step_w)

    @staticmethod
    def _cost_rows(name, t, rows, device=None):
        _check_tensor(name, t, device)
        if t.numel() != rows * 4 or t.shape[-1] != 4:
            raise ValueError(f"{name} must hold {rows} rows of 4; got {tuple(t.shape)}")

    def scenario_reduce(self, cost4_scen, nprob: int, nscen: int, worst: int, cost4=None, best_keys=None,
                        index_base: int = 0, reset_best: bool = True, stream=None):
        """Fold per-scenario costs into one row per candidate
        (``mpcr_scenario_reduce``).  ``cost4_scen``: a device tensor of
        nprob * nscen * n_per rows of 4, candidate i of problem p in scenario s
        at row (p nscen + s) n_per + i.  Per candidate the ``worst`` rows with
        the largest total are averaged, column by column: ``worst`` = nscen is
        the mean, 1 the worst scenario's row, between them a CVaR.  Returns
        ``cost4`` (nprob * n_per, 4); ``best_keys`` (int64, nprob elements)
        receives the packed argmin key of the aggregated total per problem.
        Graph-capturable."""
        import torch
        nprob, nscen, worst = int(nprob), int(nscen), int(worst)
        if nprob < 1 or nscen < 1:
            raise ValueError(f"nprob={nprob}, nscen={nscen}: both must be >= 1")
        _check_tensor("cost4_scen", cost4_scen)
        rows = cost4_scen.numel() // 4
        if rows % (nprob * nscen):
            raise ValueError(f"cost4_scen rows ({rows}) must split evenly over nprob={nprob} x nscen={nscen}")
        n_per = rows // (nprob * nscen)
        self._cost_rows("cost4_scen", cost4_scen, rows)
        if cost4 is None:
            cost4 = torch.empty((nprob * n_per, 4), dtype=torch.float32, device=cost4_scen.device)
        self._cost_rows("cost4", cost4, nprob * n_per, cost4_scen.device)
        if best_keys is not None and best_keys.numel() < nprob:
            raise ValueError("best_keys needs nprob elements")
        check(_lib.load().mpcr_scenario_reduce(self.handle, _ptr(cost4_scen), nprob, nscen, n_per, worst, _ptr(cost4),
                                               _ptr(best_keys), int(index_base),
                                               *_call_tail(cost4_scen, reset_best, stream)))
        return cost4

    def rollout_cost_scenarios(self, inp, layout: int, params, nprob: int, nscen: int, cost4_scen, worst=None,
                               cost4=None, start=None, final_state=None, theta=None, thetadot=None, best_keys=None,
                               index_base: int = 0, status=None, reset_best: bool = True, stream=None, ctrl=None,
                               ctrl_per_step: bool = False, geom_pose=None, geom_pose_per_step: bool = False,
                               target=None, target_per_step: bool = False, slot_w=None, step_w=None):
        """One set of candidates priced in ``nscen`` scenarios per problem
        (``mpcr_rollout_cost_scenarios``).  ``inp`` holds nprob * n_per rows;
        rollout problem r = p nscen + s is scenario s of problem p and is
        addressed like a problem of ``rollout_cost_state``: ``params`` is
        (nprob * nscen, 20), and ``start`` / ``ctrl`` / ``geom_pose`` hold one
        block for all or one per rollout problem (leading size nprob * nscen).
        ``cost4_scen``, ``status`` and ``final_state`` have nprob * nscen *
        n_per rows; ``theta`` and ``thetadot`` nprob * n_per, written by
        scenario 0.  ``cost4`` (nprob * n_per, 4; None skips the fold) receives
        ``scenario_reduce`` with ``worst`` (default nscen: the mean), and
        ``best_keys`` (needs ``cost4``) its keys.  Each scenario's slice is
        bitwise the ``rollout_cost_state`` call on that scenario's blocks.
        ``target`` / ``target_per_step`` as there, per rollout problem
        (``mpcr_rollout_cost_scenarios_target``).  ``slot_w``
        (``mpcr_rollout_cost_scenarios_slotw``): (nslot,), (nprob, nslot) -- a
        problem's block for all its scenarios -- or (nprob, nscen, nslot), one
        per hypothesis.  ``step_w`` (``mpcr_rollout_cost_scenarios_stepw``):
        (H, 4), (nprob, H, 4) -- a problem's schedule for all its scenarios --
        or (nprob, nscen, H, 4), one per hypothesis.  A per-problem ``slot_w``
        or ``step_w`` given with scenarios, and a ``slot_w`` whose rows need
        padding, are expanded into a temporary the launch reads: on the
        current stream the allocator keeps it alive for the kernel; a caller
        that passes a ``stream=`` of its own should pass the per-scenario
        (padded) tensor itself and keep it alive until the launch has run.
        Returns ``cost4`` (or ``cost4_scen`` without one).  Graph-capturable."""
        nprob, nscen = int(nprob), int(nscen)
        worst = nscen if worst is None else int(worst)
        _check_tensor("input", inp)
        n = int(inp.shape[0])
        if nprob < 1 or nscen < 1 or n % nprob:
            raise ValueError(f"input rows ({n}) must split evenly over nprob={nprob} problems (nscen={nscen} >= 1)")
        n_per, R = n // nprob, nprob * nscen
        self._cost_rows("cost4_scen", cost4_scen, R * n_per, inp.device)
        if cost4 is not None:
            self._cost_rows("cost4", cost4, n, inp.device)
        if best_keys is not None and (cost4 is None or best_keys.numel() < nprob):
            raise ValueError("best_keys needs nprob elements and cost4 (the keys come from the fold)")
        if status is not None and status.numel() < R * n_per:
            raise ValueError(f"status needs {R * n_per} elements")
        # the R rollout problems' blocks, as rollout_cost_state takes its nprob problems'
        args = self._state_args(R, R * n_per, inp, start, final_state, ctrl, ctrl_per_step, geom_pose,
                                geom_pose_per_step)
        fn = _lib.load().mpcr_rollout_cost_scenarios
        if target is not None or slot_w is not None or step_w is not None:
            fn = _lib.load().mpcr_rollout_cost_scenarios_target
            args += self._block_args("target", target, (8,), R, inp.device, target_per_step)
        if step_w is not None:
            _check_tensor("step_w", step_w, inp.device)
            if step_w.dim() == 3 and nscen > 1 and step_w.shape[0] == nprob:  # a problem's schedule for its scenarios
                step_w = step_w.unsqueeze(1).expand(nprob, nscen, *step_w.shape[1:]).contiguous()
            if step_w.dim() == 4 and tuple(step_w.shape[:2]) == (nprob, nscen):
                step_w = step_w.reshape(R, *step_w.shape[2:])
        if slot_w is not None:
            fn = _lib.load().mpcr_rollout_cost_scenarios_slotw
            _check_tensor("slot_w", slot_w, inp.device)
            if slot_w.dim() == 2 and nscen > 1 and slot_w.shape[0] == nprob:  # a problem's block for its scenarios
                slot_w = slot_w.unsqueeze(1).expand(nprob, nscen, slot_w.shape[-1]).contiguous()
            if slot_w.dim() == 3 and tuple(slot_w.shape[:2]) == (nprob, nscen):
                slot_w = slot_w.reshape(R, slot_w.shape[-1])
            slot_w, sw_args = self._slot_w_args(slot_w, R, inp.device)
            args += sw_args
        if step_w is not None:
            fn = _lib.load().mpcr_rollout_cost_scenarios_stepw
            args += ((None, 0) if slot_w is None else ()) + self._block_args("step_w", step_w, (self.H, 4), R,
                                                                             inp.device)[:2]
        check(fn(
            self.handle, _ptr(inp), layout, nprob, nscen, worst, n_per, self._params_arg(params, R), *args,
            _ptr(cost4_scen), _ptr(cost4), _ptr(theta), _ptr(thetadot), _ptr(best_keys), int(index_base),
            _ptr(status), *_call_tail(inp, reset_best, stream)))
        return cost4 if cost4 is not None else cost4_scen

    def trace(self, inp, layout: int, q0, w, ptgt, qtgt):
        """Debug/parity run (host arrays): cost4, theta, per-step eef pose, masked slot distances."""
        lib = _lib.load()
        inp = np.ascontiguousarray(inp, dtype=np.float32)
        n = inp.shape[0]
        q0 = self._vec(q0, 8, np.float64)
        w = self._vec(w, 3, np.float32)
        pt = self._vec(ptgt, 3, np.float32)
        qt = self._vec(qtgt, 4, np.float32)
        cost4 = np.zeros((n, 4), dtype=np.float32)
        theta = np.zeros((n, self.nctrl * self.H), dtype=np.float32)
        eef = np.zeros((n, self.H, 7), dtype=np.float32)
        slots = np.zeros((n, self.H, max(self.nslot, 1)), dtype=np.float32)
        check(lib.mpcr_rollout_trace(self.handle, inp.ctypes.data_as(ctypes.c_void_p), layout, n,
                                     q0.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), _f32p(w), _f32p(pt),
                                     _f32p(qt), cost4.ctypes.data_as(ctypes.c_void_p),
                                     theta.ctypes.data_as(ctypes.c_void_p), eef.ctypes.data_as(ctypes.c_void_p),
                                     slots.ctypes.data_as(ctypes.c_void_p)))
        return dict(cost4=cost4, theta=theta, eef=eef, slots=slots[:, :, : self.nslot])


class Plant:
    """One environment of a compiled model stepped on the GPU by the rollout
    kernel (``mpcr_plant_*``): the closed-loop plant of
    ``run_cem_planner`` (CPU ``MjData`` + ``mj_step`` in the reference,
    SBP/mpc_planner.py:109-114,179-180).  State is fp32 on the device."""

    def __init__(self, compiled_model, device: int = 0):
        lib = _lib.load()
        self.model = Model(compiled_model)
        self.nq, self.nv = int(compiled_model.nq), int(compiled_model.nv)
        self.nctrl = int(compiled_model.nctrl)
        self.nu = int(getattr(compiled_model, "nu", 0))
        self._ctrl = None  # the controls applied (clamped); None: the model's own
        self._geom_poses = None  # the geom-pose block applied; None: the model's own
        h = ctypes.c_void_p()
        check(lib.mpcr_plant_create(self.model.handle, int(device), ctypes.byref(h)))
        self.handle = h
        self.device = int(device)
        self.qpos = np.zeros(self.nq)
        self.qvel = np.zeros(self.nv)
        self.qacc = np.zeros(self.nv)
        self.eef = np.zeros(7)
        self._pull()

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                _lib.load().mpcr_plant_free(self.handle)
        except Exception:  # interpreter shutdown
            pass
        self.handle = None

    def _pull(self):
        dp = ctypes.POINTER(ctypes.c_double)
        check(_lib.load().mpcr_plant_get_state(self.handle, self.qpos.ctypes.data_as(dp),
                                               self.qvel.ctypes.data_as(dp), self.qacc.ctypes.data_as(dp),
                                               self.eef.ctypes.data_as(dp)))

    def set_state(self, qpos=None, qvel=None, qacc_warmstart=None):
        dp = ctypes.POINTER(ctypes.c_double)
        arr = lambda x, n: None if x is None else np.ascontiguousarray(x, dtype=np.float64).reshape(n)  # noqa: E731
        qp, qv, qw = arr(qpos, self.nq), arr(qvel, self.nv), arr(qacc_warmstart, self.nv)
        check(_lib.load().mpcr_plant_set_state(self.handle, None if qp is None else qp.ctypes.data_as(dp),
                                               None if qv is None else qv.ctypes.data_as(dp),
                                               None if qw is None else qw.ctypes.data_as(dp)))
        self._pull()

    def set_ctrl(self, ctrl):
        """The plant's actuator controls from now on (``mpcr_plant_set_ctrl``):
        nu values in actuator order, clamped to the model's ctrlrange; None
        restores the model's own."""
        c = None
        if ctrl is not None:
            c = np.ascontiguousarray(ctrl, dtype=np.float64).reshape(-1)
            if c.size != self.nu:
                raise ValueError(f"ctrl must hold nu={self.nu} values, got {c.size}")
        check(_lib.load().mpcr_plant_set_ctrl(
            self.handle, None if c is None else c.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))
        self._ctrl = None if c is None else self.model.clamp_ctrl(c)

    @property
    def ctrl(self):
        """The controls the plant applies (clamped), in actuator order."""
        return self.model.clamp_ctrl(self.model.own_ctrl()) if self._ctrl is None else self._ctrl.copy()

    def set_geom_poses(self, block):
        """The plant's static geom poses from now on
        (``mpcr_plant_set_geom_poses``): a host geom-pose block (ng, 8)
        (``Model.geom_poses``, ``Model.pose_rows``) whose static rows are used
        as they are; None restores the model's own."""
        b = None
        if block is not None:
            own = self.model.geom_poses()[0]
            b = np.ascontiguousarray(block.cpu() if hasattr(block, "cpu") else block, dtype=np.float32)
            if b.shape != own.shape:
                raise ValueError(f"block must be {own.shape}, got {b.shape}")
        check(_lib.load().mpcr_plant_set_geom_poses(self.handle, None if b is None else _f32p(b)))
        self._geom_poses = None if b is None else b.copy()

    @property
    def geom_poses(self):
        """The geom-pose block the plant applies, (ng, 8) float32."""
        return self.model.geom_poses()[0] if self._geom_poses is None else self._geom_poses.copy()

    def copy_state(self, tensor, stream=None):
        """The plant's state block into ``tensor`` (float32, CUDA, contiguous,
        at least one block), device to device on the current torch stream
        (``mpcr_plant_copy_state``): a planner's start state."""
        size = Engine.state_layout()["size"]
        _check_tensor("tensor", tensor)
        if tensor.numel() < size or tensor.device.index != self.device:
            raise ValueError(f"tensor must hold at least {size} elements on the plant's device (cuda:{self.device})")
        check(_lib.load().mpcr_plant_copy_state(self.handle, _ptr(tensor), _stream_arg(tensor, stream)))
        return tensor

    def forward(self):
        """mj_forward: qacc and the eef pose at the current state."""
        check(_lib.load().mpcr_plant_step(self.handle, None, 0, None))
        self._pull()

    def step(self, qvel_ctrl=None):
        """qvel[:nctrl] = qvel_ctrl; mj_step.  Afterwards ``eef`` holds the tcp
        position / hande quaternion of the state the step started from (as
        MjData.site_xpos / xquat after mj_step)."""
        dp = ctypes.POINTER(ctypes.c_double)
        v = None
        if qvel_ctrl is not None:
            v = np.ascontiguousarray(qvel_ctrl, dtype=np.float64).reshape(self.nctrl)
        check(_lib.load().mpcr_plant_step(self.handle, None if v is None else v.ctypes.data_as(dp), 1, None))
        self._pull()

    def step_debug(self, qvel_ctrl, mpr_pair=-1):
        """step() that also returns the step's active contacts, constraint-row
        parameters, qacc_smooth and qacc (``parse_step_debug``; parity
        debugging, mpcr_plant_step_debug)."""
        lib = _lib.load()
        buf = np.zeros(lib.mpcr_plant_dbg_size(), dtype=np.float32)
        v = np.ascontiguousarray(qvel_ctrl, dtype=np.float64).reshape(self.nctrl)
        check(lib.mpcr_plant_step_debug(self.handle, v.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                        buf.ctypes.data_as(ctypes.c_void_p), int(mpr_pair)))
        self._pull()
        return parse_step_debug(buf, self.nv)

    @property
    def site_xpos_tcp(self):
        return self.eef[:3].copy()

    @property
    def xquat_hande(self):
        return self.eef[3:7].copy()


__all__ = ["Engine", "Model", "Plant", "MPCR_LAYOUT_XI", "MPCR_LAYOUT_THETADOT"]


DBG_CON, DBG_MAXCON, DBG_MAXROW, DBG_NV = 2, 48, 200, 32  # rollout.h DBG_* layout


def parse_step_debug(buf, nv):
    """DBG_* buffer (kernel or oracle_step_debug) -> dict of numpy arrays."""
    buf = np.asarray(buf, dtype=np.float64)
    ncon, nefc = int(buf[0]), int(buf[1])
    con = buf[DBG_CON:DBG_CON + 8 * DBG_MAXCON].reshape(DBG_MAXCON, 8)[:min(ncon, DBG_MAXCON)]
    r0 = DBG_CON + 8 * DBG_MAXCON
    rows = buf[r0:r0 + 3 * DBG_MAXROW].reshape(DBG_MAXROW, 3)[:min(nefc, DBG_MAXROW)]
    q0 = r0 + 3 * DBG_MAXROW
    return dict(ncon=ncon, nefc=nefc, con_pos=con[:, 0:3], con_dist=con[:, 3], con_pair=con[:, 4].astype(int),
                con_normal=con[:, 5:8], efc_D=rows[:, 0], efc_aref=rows[:, 1], efc_vel=rows[:, 2],
                qacc_smooth=buf[q0:q0 + nv], qacc=buf[q0 + DBG_NV:q0 + DBG_NV + nv],
                info=buf[q0 + 2 * DBG_NV:q0 + 2 * DBG_NV + 8],
                grad=buf[q0 + 2 * DBG_NV + 8:q0 + 2 * DBG_NV + 8 + nv],
                search=buf[q0 + 3 * DBG_NV + 8:q0 + 3 * DBG_NV + 8 + nv],
                mpr=buf[q0 + 4 * DBG_NV + 8:q0 + 4 * DBG_NV + 8 + 112])
