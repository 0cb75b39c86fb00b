"""Device-resident CEM distribution step (libmpcr ``mpcr_cem_*`` / ``mpcr_topk``).

Wraps the HIP kernels of ``csrc/cem.hip`` for torch CUDA tensors, launched on
the current torch stream (so a whole CEM iteration can be captured in a
graph).  Reference functions (SBP/mjx_planner.py):

  ``factor`` + ``sample_project``  compute_xi_samples (:312-316) fused with
                                   compute_projection_filter (:180-249)
  ``project``                      compute_projection_filter alone
  ``topk``                         compute_ellite_samples' argsort (:305-310)
  ``update``                       compute_mean_cov / comp_prod (:318-335)

Every call requires a gfx950 device and the built library; there is no
torch or CPU fallback.
"""

from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from ._lib import MPCR_F_DEVICE_PTRS, check

NBASIS = 11


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _dev(t, dtype, name):
    import torch
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dtype or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous {dtype} CUDA tensor")
    return t


class CemContext:
    """Projection tables (basis rows, KKT inverse) + the Cholesky factor for
    one (num_dof, horizon) planner on one device."""

    def __init__(self, P, Pdot, Pddot, num_dof: int, max_n: int, device: int = 0, qinv=None,
                 num_problems: int = 1):
        lib = _lib.load()
        P, Pdot, Pddot = (np.ascontiguousarray(x, dtype=np.float64) for x in (P, Pdot, Pddot))
        if P.shape[1] != NBASIS:
            raise ValueError(f"the CEM kernels are built for an order-10 basis ({NBASIS} columns)")
        self.num_dof = int(num_dof)
        self.H = int(P.shape[0])
        self.nvar = self.num_dof * NBASIS
        self.max_n = int(max_n)
        self.device = int(device)
        q = None
        if qinv is not None:
            q = np.ascontiguousarray(qinv, dtype=np.float64)
            ne = self.nvar + 5 * self.num_dof
            if q.shape != (ne, ne):
                raise ValueError(f"qinv must be {ne}x{ne}")
        h = ctypes.c_void_p()
        check(lib.mpcr_cem_create(self.device, self.num_dof, self.H, NBASIS, P.ctypes.data, Pdot.ctypes.data,
                                  Pddot.ctypes.data, q.ctypes.data if q is not None else None, self.max_n,
                                  ctypes.byref(h)))
        self.handle = h
        self.num_problems = int(num_problems)
        if self.num_problems != 1:  # room for one Cholesky factor per problem (the *_multi calls)
            check(lib.mpcr_cem_set_problems(self.handle, self.num_problems))

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                _lib.load().mpcr_cem_free(self.handle)
        except Exception:  # interpreter shutdown
            pass
        self.handle = None

    @staticmethod
    def _stream(t, stream):
        import torch
        return ctypes.c_void_p(stream if stream is not None else torch.cuda.current_stream(t.device).cuda_stream)

    # Each stage has one body, which both of its public calls go through.  The
    # one-problem call is the nprob = 1 case without the leading problem axis
    # on its tensors; it keeps its own C entry for what only that entry takes
    # (per-candidate b_eq rows, an empty batch, elites gathered from more
    # candidates than max_n).

    def _factor(self, multi, cov, reg, stream):
        import torch
        _dev(cov, torch.float32, "cov")
        if multi and cov.dim() != 3:
            raise ValueError("cov must be (nprob, nvar, nvar)")
        lib = _lib.load()
        fn, nprob = (lib.mpcr_cem_factor_multi, (int(cov.shape[0]),)) if multi else (lib.mpcr_cem_factor, ())
        check(fn(self.handle, _ptr(cov), *nprob, float(reg), MPCR_F_DEVICE_PTRS, self._stream(cov, stream)))

    def factor(self, cov, reg: float = 0.003, stream=None):
        """L = chol(cov + reg I) for the next ``sample_project``."""
        self._factor(False, cov, reg, stream)

    def factor_multi(self, cov, reg: float = 0.003, stream=None):
        """One Cholesky factor per problem: cov is (nprob, nvar, nvar)."""
        self._factor(True, cov, reg, stream)

    def _sample_project(self, nprob, n, mean, seed, counter, b_eq, maxiter, bounds, rho, xi_samples, out, xi_in,
                        index_base, stream, beq_shared=True, seed_step=0):
        """nprob None: ``sample_project``; else ``sample_project_multi``."""
        import torch
        ref = mean if mean is not None else xi_in
        if ref is None:
            raise ValueError("need mean or xi_in")
        if out is None:
            shape = (n, self.nvar) if nprob is None else (nprob, n, self.nvar)
            out = torch.empty(shape, dtype=torch.float32, device=ref.device)
        for name, t in (("mean", mean), ("xi_in", xi_in), ("xi_samples", xi_samples), ("out", out),
                        ("b_eq", b_eq)):
            if t is not None:
                _dev(t, torch.float32, name)
        bnd = (ctypes.c_float * 3)(*[float(b) for b in bounds])
        u64 = lambda v: ctypes.c_uint64(int(v) & (2**64 - 1))  # noqa: E731
        lib, st = _lib.load(), self._stream(ref, stream)
        if nprob is None:
            check(lib.mpcr_cem_sample_project(
                self.handle, int(n), _ptr(mean), u64(seed), u64(counter), int(index_base), _ptr(xi_in),
                _ptr(xi_samples), _ptr(b_eq), 0 if beq_shared else 5 * self.num_dof, int(maxiter), bnd, float(rho),
                _ptr(out), MPCR_F_DEVICE_PTRS, st))
            return out
        for name, t, numel in (("mean", mean, nprob * self.nvar), ("b_eq", b_eq, nprob * 5 * self.num_dof),
                               ("xi_in", xi_in, nprob * n * self.nvar), ("out", out, nprob * n * self.nvar),
                               ("xi_samples", xi_samples, nprob * n * self.nvar)):
            if t is not None and t.numel() != numel:
                raise ValueError(f"{name} has {t.numel()} elements, expected {numel}")
        check(lib.mpcr_cem_sample_project_multi(
            self.handle, int(nprob), int(n), _ptr(mean), u64(seed), u64(seed_step), u64(counter), int(index_base),
            _ptr(xi_in), _ptr(xi_samples), _ptr(b_eq), int(maxiter), bnd, float(rho), _ptr(out), MPCR_F_DEVICE_PTRS,
            st))
        return out

    def sample_project(self, n, mean, seed, counter, b_eq, maxiter, bounds, rho=1.0, xi_samples=None, out=None,
                       xi_in=None, beq_shared=True, index_base=0, stream=None):
        """xi_samples = mean + z L^T (Philox (seed, counter), candidate i drawn
        as global candidate ``index_base + i``); or ``xi_in`` when mean is
        None; then ``maxiter`` ADMM iterations.  Returns the projected
        (n, nvar) tensor."""
        return self._sample_project(None, n, mean, seed, counter, b_eq, maxiter, bounds, rho, xi_samples, out, xi_in,
                                    index_base, stream, beq_shared=beq_shared)

    def sample_project_multi(self, nprob, n_per, mean, seed, counter, b_eq, maxiter, bounds, rho=1.0, seed_step=0,
                             xi_samples=None, out=None, xi_in=None, index_base=0, stream=None):
        """``sample_project`` for nprob problems of n_per candidates in one
        launch: mean (nprob, nvar) or None with xi_in (nprob, n_per, nvar),
        b_eq (nprob, 5 num_dof); problem p draws with the Philox key
        ``seed + p * seed_step``.  Returns the projected (nprob, n_per, nvar)
        tensor, bitwise the single calls on the slices."""
        return self._sample_project(int(nprob), n_per, mean, seed, counter, b_eq, maxiter, bounds, rho, xi_samples,
                                    out, xi_in, index_base, stream, seed_step=seed_step)

    def project(self, xi, b_eq, maxiter, bounds, rho=1.0, out=None, beq_shared=True, stream=None):
        return self.sample_project(xi.shape[0], None, 0, 0, b_eq, maxiter, bounds, rho, out=out, xi_in=xi,
                                   beq_shared=beq_shared, stream=stream)

    def _update(self, multi, xi, cost, stride, elite_idx, lamda, alpha_mean, alpha_cov, mean, cov, reg, stream):
        import torch
        _dev(xi, torch.float32, "xi"); _dev(cost, torch.float32, "cost")
        _dev(elite_idx, torch.int32, "elite_idx"); _dev(mean, torch.float32, "mean"); _dev(cov, torch.float32, "cov")
        lib = _lib.load()
        fn = lib.mpcr_cem_update
        if multi:
            if xi.dim() != 3 or elite_idx.dim() != 2 or elite_idx.shape[0] != xi.shape[0]:
                raise ValueError("xi must be (nprob, n_per, nvar) and elite_idx (nprob, k)")
            if mean.numel() != xi.shape[0] * self.nvar or cov.numel() != xi.shape[0] * self.nvar * self.nvar:
                raise ValueError("mean must be (nprob, nvar) and cov (nprob, nvar, nvar)")
            fn = lib.mpcr_cem_update_multi
        # xi's leading axes are the call's n or nprob, n_per; elite_idx's last is k
        check(fn(self.handle, _ptr(xi), *map(int, xi.shape[:2 if multi else 1]), _ptr(cost), int(stride),
                 _ptr(elite_idx), int(elite_idx.shape[-1]), float(lamda), float(alpha_mean), float(alpha_cov),
                 float(reg), _ptr(mean), _ptr(cov), MPCR_F_DEVICE_PTRS, self._stream(xi, stream)))

    def update(self, xi, cost, stride, elite_idx, lamda, alpha_mean, alpha_cov, mean, cov, reg=1e-4, stream=None):
        """In-place weighted elite mean/cov update (compute_mean_cov)."""
        self._update(False, xi, cost, stride, elite_idx, lamda, alpha_mean, alpha_cov, mean, cov, reg, stream)

    def update_multi(self, xi, cost, stride, elite_idx, lamda, alpha_mean, alpha_cov, mean, cov, reg=1e-4,
                     stream=None):
        """``update`` per problem, in place: xi (nprob, n_per, nvar), cost
        (nprob, n_per[, stride]), elite_idx (nprob, k) local indices
        (``topk_multi``), mean (nprob, nvar), cov (nprob, nvar, nvar)."""
        self._update(True, xi, cost, stride, elite_idx, lamda, alpha_mean, alpha_cov, mean, cov, reg, stream)


def _topk(engine, cost, nprob, k, stride, out, stream):
    """nprob None: ``topk``; else ``topk_multi``."""
    import torch
    _dev(cost, torch.float32, "cost")
    n = cost.numel() // stride
    if nprob is not None and (nprob < 1 or n % nprob):
        raise ValueError(f"{n} costs do not split evenly over nprob={nprob} problems")
    if out is None:
        out = torch.empty(k if nprob is None else (nprob, k), dtype=torch.int32, device=cost.device)
    st = stream if stream is not None else torch.cuda.current_stream(cost.device).cuda_stream
    lib = _lib.load()
    fn, shape = (lib.mpcr_topk, (n,)) if nprob is None else (lib.mpcr_topk_multi, (int(nprob), n // nprob))
    check(fn(engine.handle, _ptr(cost), int(stride), *shape, int(k), _ptr(out), MPCR_F_DEVICE_PTRS,
             ctypes.c_void_p(st)))
    return out


def topk_multi(engine, cost, nprob, k, stride=1, out=None, stream=None):
    """``topk`` for nprob problems in one launch: cost holds nprob * n_per
    entries of ``stride`` floats, problem p owning entries [p n_per,
    (p + 1) n_per); returns (nprob, k) int32 indices local to each problem."""
    return _topk(engine, cost, int(nprob), k, stride, out, stream)


def topk(engine, cost, k, stride=1, out=None, stream=None):
    """Indices of the k smallest of cost[i*stride] in stable-argsort order
    (NaN last) through ``mpcr_topk`` on ``engine``'s device."""
    return _topk(engine, cost, None, k, stride, out, stream)


__all__ = ["CemContext", "topk", "topk_multi", "NBASIS"]

