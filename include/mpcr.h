/*
 * mpcr.h — C ABI of libmpcr, the MI355X rollout engine behind the drop-in
 * cem_planner (manipulator_mujoco_amd/planner.py).
 *
 * Plain C: pointers + sizes, no torch/HIP types in the signatures.  Every
 * function returns 0 on success or a negative MPCR_E* code; the message of
 * the last failure on the calling thread is available from
 * mpcr_last_error().  Engines are independent (one per host thread / stream);
 * there is no global mutable state besides the thread-local error string and
 * the process-wide two-wave batch threshold (mpcr_set_two_wave_max_n).
 *
 * Reference interface each entry point replaces (file:line in
 * /root/reference/sampling_based_planner/):
 *   mpcr_model_*          MjModel.from_xml_path + mjx.put_model/put_data +
 *                         jit(mjx.forward) template          mjx_planner.py:100-108
 *   mpcr_engine_create    cem_planner.__init__ (basis P/Pdot, mask, ids)
 *                                                             mjx_planner.py:19-126
 *   mpcr_rollout_cost     A_thetadot @ xi + compute_rollout_batch (vmap of
 *                         compute_rollout_single / lax.scan of mjx_step) +
 *                         compute_cost_batch                  mjx_planner.py:348-354,
 *                                                             251-303
 *   best_key / mpcr_argmin / mpcr_best_key_decode
 *                         idx_min = argmin(cost_batch[-1])    mjx_planner.py:395
 *   mpcr_topk             compute_ellite_samples argsort     mjx_planner.py:305-310
 *   mpcr_cem_create       cem_planner.__init__ basis + get_Q_inv mjx_planner.py:40-46,
 *                                                             140-172
 *   mpcr_cem_factor       the Cholesky inside jax.random.multivariate_normal
 *                                                             mjx_planner.py:312-316
 *   mpcr_cem_sample_project / mpcr_project
 *                         compute_xi_samples + compute_projection_filter
 *                         (+ compute_projection)              mjx_planner.py:312-316,
 *                                                             180-249
 *   mpcr_cem_update       compute_mean_cov + comp_prod       mjx_planner.py:318-335
 *   mpcr_rollout_cost_dp  mpcr_rollout_cost with the per-tick arguments
 *                         (init_pos, weights, target pose) read from device
 *                         memory, so a whole cem_iter can be graph-captured
 *                         once and replayed every tick       mjx_planner.py:364-406
 *   mpcr_plant_*          the closed-loop plant: data.qvel[:num_dof] = thetadot;
 *                         mujoco.mj_step / mj_forward on the planner's model
 *                         (CPU MjData in the reference)      mpc_planner.py:109-114,
 *                                                             120-121,173-184
 */
#ifndef MPCR_H_
#define MPCR_H_

#include <stddef.h>
#include <stdint.h>

#include "mpcr_model.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ABI version.  4 (round 6): model format v9 without the support start
   table, which the engine builds (mpcr_model_hull_starts).  3: bit 10 reports a lost two-wave handshake
   (MPCR_STATUS_SYNC), so rows-summed moved to bit 11.  2 (round 4): the
   max-rows field widened to 8 bits (version 1: 6 bits << 2, sum << 8).
   Decode with the accessors below, not raw shifts.
   The multi-problem entry points (mpcr_rollout_cost_multi, mpcr_topk_multi,
   mpcr_cem_set_problems, mpcr_cem_*_multi) are backward-compatible additions:
   no existing signature, layout or result changed, so the version stays 4. */
#define MPCR_ABI_VERSION 4

/* the per-candidate status word of mpcr_rollout_cost / _dp */
#define MPCR_STATUS_TRUNCATED(s) ((s) & 1)                  /* constraint rows truncated  */
#define MPCR_STATUS_NONFINITE(s) (((s) >> 1) & 1)           /* non-finite state           */
#define MPCR_STATUS_MAX_ROWS(s) (((s) >> 2) & 255)          /* busiest step's rows (<= 255) */
#define MPCR_STATUS_SYNC(s) (((s) >> 10) & 1)               /* two-wave handshake timed out:
                                                                the candidate's outputs are void
                                                                and its cost is +inf */
#define MPCR_STATUS_ROWS_SUM(s) ((unsigned)(s) >> 11)       /* rows summed over the horizon */
#define MPCR_STATUS_FAILED(s) (((s) & 2) | ((s) & (1 << 10)))  /* no usable result */

enum {
  MPCR_OK = 0,
  MPCR_EINVAL = -1,   /* bad argument / shape                      */
  MPCR_EMODEL = -2,   /* model blob invalid or over capacity        */
  MPCR_EHIP = -3,     /* HIP runtime error                          */
  MPCR_ENOMEM = -4,
  MPCR_ENODEV = -5    /* no gfx950 device                           */
};

/* input layouts for mpcr_rollout_cost */
enum {
  MPCR_LAYOUT_XI = 0,       /* n x (nctrl*nbasis) Bernstein coefficients,
                               joint-major (xi_filtered, mjx_planner.py:348) */
  MPCR_LAYOUT_THETADOT = 1  /* n x (nctrl*H) joint velocities, joint-major */
};

/* flags */
enum {
  MPCR_F_DEVICE_PTRS = 1 << 0, /* every array argument is a device pointer  */
  MPCR_F_RESET_BEST  = 1 << 1, /* set *best_key to UINT64_MAX before launch */
  MPCR_F_SYNC        = 1 << 2  /* block until the stream is idle           */
};

typedef struct mpcr_model mpcr_model;   /* opaque host model handle */
typedef struct mpcr_engine mpcr_engine; /* opaque device engine      */
typedef struct mpcr_cem mpcr_cem;       /* opaque CEM context (projection tables, Cholesky factor) */

const char* mpcr_last_error(void);
int mpcr_abi_version(void);
/* gfx target name of `device` (e.g. "gfx950") into buf */
int mpcr_device_arch(int device, char* buf, int buflen);

/* models: a serialised mpcr_model_t (see mpcr_model.h) */
int mpcr_model_from_blob(const void* blob, size_t nbytes, mpcr_model** out);
/* path: an MJCF scene (.xml, or any file starting with '<') -- compiled by
   the MJCF compiler of libmpcr_mjcf.so (include/mpcr_mjcf.h), dlopened from
   this library's directory on first use: MjModel.from_xml_path,
   SBP/mjx_planner.py:100-103 -- or a serialised mpcr_model_t blob.
   timestep > 0 overrides the model's (opt.timestep = dt, :102). */
int mpcr_model_load(const char* path, double timestep, mpcr_model** out);
int mpcr_model_set_timestep(mpcr_model* m, double timestep);
int mpcr_model_info(const mpcr_model* m, int* nq, int* nv, int* nslot, int* nctrl, int* npair);
/* The model's actuators: their number, and (nullable) ctrlrange[nu][2] and
   limited[nu] (1 where the control is clamped to its range). */
int mpcr_model_actuators(const mpcr_model* m, int* nu, double* ctrlrange, int* limited);
/* The model's collision geoms as the device model orders them (the order of a
   geom-pose block's rows, mpcr_rollout_cost_world): their number and, each
   nullable, the model's own block[ngeom][8] (x y z 0 | qw qx qy qz, the world
   pose of a static geom exactly as an engine of this model holds it; a moving
   geom's row is 0 0 0 0 | 1 0 0 0 and is never read), model_geom_id[ngeom]
   (row -> geom index in the model) and is_static[ngeom]. */
int mpcr_model_geom_poses(const mpcr_model* m, int* ngeom, float* block, int* model_geom_id, int* is_static);
/* The model's robot-masked contact slots, the ones cost_c is summed over and
   a slot-weight block prices (mpcr_rollout_cost_slotw): their number and, each
   nullable, per slot in slot order geom1[nslot] and geom2[nslot] (the slot's
   two geoms in the device model's geom order: rows of mpcr_model_geom_poses)
   and pair[nslot] (the collision pair that owns the slot).  Host only: needs
   no device. */
int mpcr_model_slots(const mpcr_model* m, int* nslot, int* geom1, int* geom2, int* pair);
void mpcr_model_free(mpcr_model* m);
/* The support start table an engine builds for m's convex hulls (model
   format v9 dropped it from the blob; dev_model.h hull_start_table): R x R
   cells on each of the 6 cube faces (R = 0: the library's MPCR_LUT_R), cell
   (2 axis + negative) R^2 + iu R + iv (csrc/convex_mpr.h lut_cell), each naming
   the global hull vertex extreme along the cell centre (fp64; the lowest
   index among exact ties).  geom_adr[ngeom] (nullable) receives each geom's
   first cell (-1: no hull), cells and exact (nullable) every cell when cap
   holds the count -- exact[c] = 1 where the engine skips the climb (the
   start vertex beats each neighbour along every direction of the cell by the
   fp32 margin).  Returns the cell count (< 0: error).  Host only, no device
   (tests/test_hull_lut.py). */
int64_t mpcr_model_hull_starts(const mpcr_model* m, int R, int32_t* geom_adr, int32_t* cells, uint8_t* exact,
                               int64_t cap);
/* Test knob (the start-independence tests): engines created while seed != 0
   start every hull climb at a vertex of its hull hashed from (seed, geom,
   cell) instead of the extreme one.  Process-wide; returns the previous seed. */
uint64_t mpcr_set_hull_start_scramble(uint64_t seed);

/* engines: device copy of the model + the Pdot basis (horizon x nbasis,
   row-major fp32, bernstein_coeff_ordern_new(..)[1]) + scratch for max_n. */
int mpcr_engine_create(const mpcr_model* m, int device, int max_n, int horizon, const float* pdot,
                       int nbasis, mpcr_engine** out);
void mpcr_engine_free(mpcr_engine* e);

/* Fused basis -> H MuJoCo-semantics steps -> cost for n candidates.
   q0[nctrl]            initial joint positions (init_pos)
   w[3]                 (w_pos, w_rot, w_col)
   ptgt[3], qtgt[4]     target position / orientation (wxyz)
   cost4 [n x 4]        (cost, cost_g, cost_r, cost_c)          (required)
   theta [n x nctrl*H]  post-step joint positions, joint-major    (nullable)
   thetadot [n x nctrl*H] the applied joint velocities           (nullable)
   best_key             device uint64: atomic-min of
                        (ordered(cost) << 32 | (index_base + i)), NaN first (nullable)
   status [n]           per-candidate flags (bit0: constraint rows truncated,
                        bit1: non-finite state, bit10: two-wave handshake
                        lost) | (max constraint rows in one step, 8 bits
                        capped at 255, << 2) | (constraint rows summed over
                        the horizon << 11)                       (nullable)
   stream               hipStream_t or NULL (default stream)
   n = 0 is a no-op returning MPCR_OK (input and cost4 may then be NULL). */
int mpcr_rollout_cost(mpcr_engine* e, const float* input, int layout, int n, const double* q0,
                      const float* w, const float* ptgt, const float* qtgt, float* cost4, float* theta,
                      float* thetadot, uint64_t* best_key, int index_base, int* status, int flags,
                      void* stream);

/* Diagnostic: resident workgroups (= candidates) per CU, static LDS bytes and
   VGPRs of the two rollout kernel variants on `device`:
   info[6] = narrow (blocks, lds, vgprs), dual-arm class (blocks, lds, vgprs). */
int mpcr_rollout_occupancy(int device, int* info);
/* Narrow-variant batches of at most n candidates run two waves per candidate
   (the collision phase beside the dynamics; bitwise the one-wave results);
   dual-arm batches of at most min(n, 1024) too (MPCR_WPC2W_MAX_N overrides
   the 1024: four two-wave blocks per CU).  0 disables both.
   n < 0 only queries.  Returns the previous threshold (default: the build's
   MPCR_WPC2_MAX_N_DEFAULT, or the MPCR_WPC2_MAX_N environment variable).
   Process-wide (an atomic read by every engine's next launch; the
   environment is read once, when the library loads). */
int mpcr_set_two_wave_max_n(int n);
/* Self-test of the rollout kernels' wave reductions on `device`: in holds nvec
   vectors of 64 floats (host memory, 1 <= nvec <= 65536), one 64-lane block
   sums each with every form the kernels use, out (host, 12 floats per vector)
   receives
     [0] the reference sum (six DPP steps, lane 63)     [1] the full sum
     [2] [3] the two-value form on vectors b, b + 1     (indices cyclic in nvec)
     [4] [5] [6] the three-value form on b, b + 1, b + 2
     [7] the reference on lanes 0-15 (the rest +0)      [8] the one-row form on the same
     [9] the reference on lanes 0-31 (the rest +0)      [10] the two-row form on the same
     [11] 0.
   Every production form must equal its reference bit for bit
   (tests/test_gpu_reduce.py). */
int mpcr_selftest_reduce(int device, const float* in, int nvec, float* out);
/* Kernel dispatches one mpcr_rollout_cost call over n candidates issues on
   this engine (1, or -- dual-arm batches above the resident-block count --
   one per horizon segment and candidate group, MPCR_SEG_STEPS /
   MPCR_SEG_GROUPS): a profiler's per-dispatch counters times *out are per
   call.  No GPU work. */
int mpcr_engine_dispatches(const mpcr_engine* e, int n, int* out);

/* Same as mpcr_rollout_cost with MPCR_F_DEVICE_PTRS, except that the
   per-call arguments are a device block read when the kernel runs:
   params[20] = init_pos[8] | (w_pos, w_rot, w_col, 0) | ptgt[3], 0 | qtgt[4]
   (wxyz, normalised by the kernel).  Graph-capturable. */
int mpcr_rollout_cost_dp(mpcr_engine* e, const float* input, int layout, int n, const float* params,
                         float* cost4, float* theta, float* thetadot, uint64_t* best_key, int index_base,
                         int* status, int flags, void* stream);

/* Several independent problems in one call: problem p of nprob owns
   candidates [p n_per, (p + 1) n_per) of every per-candidate array (input,
   cost4, theta, thetadot, status: nprob n_per rows), reads its own block
   params + 20 p (the mpcr_rollout_cost_dp layout) and reduces into
   best_keys[p] (nullable) with the low word index_base + (index within the
   problem), so each key decodes like a single call's.  Bitwise what nprob
   mpcr_rollout_cost_dp calls on the slices compute, in one grid:
   compute_cem's rollout (mjx_planner.py:348-354, 395) for nprob start states
   / targets / weight triples at once.  Device pointers only
   (MPCR_F_DEVICE_PTRS); nprob, n_per >= 1 and nprob n_per <= max_n;
   MPCR_F_RESET_BEST resets all nprob keys.  Graph-capturable.
   Here and for every *_multi call below, the one-problem call is the
   nprob = 1 case of the same implementation (same launch, same kernel), and
   calling the *_multi entry with nprob = 1 runs exactly what it runs.  The
   one-problem entries alone keep their host-pointer modes, an empty batch
   (n = 0) as a no-op and mpcr_cem_sample_project's beq_stride. */
int mpcr_rollout_cost_multi(mpcr_engine* e, const float* input, int layout, int nprob, int n_per,
                            const float* params, float* cost4, float* theta, float* thetadot, uint64_t* best_keys,
                            int index_base, int* status, int flags, void* stream);

/* A state block: what a plant holds, fp32, device memory:
   qpos[DX_NQ] | qvel[DX_NV] | qacc_warmstart[DX_NV] | qacc[DX_NV] | eef[8]
   (eef: tcp site position | hande body quaternion wxyz | unused).  Returns
   the floats per block and writes the offset of each part (NULL skips one);
   the model's nq / nv entries of a part are used, the rest is padding.  Host
   only, no device. */
int mpcr_state_layout(int* qpos, int* qvel, int* qacc_warmstart, int* qacc, int* eef);

/* mpcr_rollout_cost_multi from a given full state, and / or returning the
   final states (a backward-compatible addition like the *_multi calls).
   start (nullable): problem p's candidates begin from qpos | qvel |
   qacc_warmstart of the block at start + p start_stride, where they
   otherwise begin from the model's template state with a zero warm start;
   start_stride is in floats, 0 (every problem shares one block) or at least
   the block size.  The qacc and eef parts of a start block are ignored, and
   everything else is a rollout's as ever: qpos[ctrl_qposadr[j]] = init_pos[j]
   from the parameter block applies afterwards, the hull climbs start afresh
   and the slot history at step 0 -- so a block that holds the template state
   gives bitwise the results of mpcr_rollout_cost_multi.  The reference's
   compute_cem starts every rollout from the template (mjx_planner.py:105-107);
   this departs from it on request only.  The block is read when the kernel
   runs (graph-capturable; a replay sees new contents) and never written.
   final_state (nullable): nprob n_per blocks, candidate i's receiving qpos |
   qvel | qacc_warmstart after the last step, that step's qacc and its
   pre-integration eef pose: what a plant holds after the same H steps from
   the same state.  Padding entries are left as they were.
   start == NULL && final_state == NULL runs exactly what
   mpcr_rollout_cost_multi runs.  Device pointers only. */
int mpcr_rollout_cost_state(mpcr_engine* e, const float* input, int layout, int nprob, int n_per,
                            const float* params, const float* start, int start_stride, float* final_state,
                            float* cost4, float* theta, float* thetadot, uint64_t* best_keys, int index_base,
                            int* status, int flags, void* stream);

/* mpcr_rollout_cost_state with the actuator controls as an input of the call
   (a backward-compatible addition; mpcr_rollout_cost_state is this call with
   ctrl = NULL).  ctrl (nullable): device memory, nu floats in actuator order
   (mpcr_model_actuators) per block.  Step t of problem p reads the block at
   ctrl + p ctrl_stride + t ctrl_step_stride (strides in floats):
   ctrl_stride = 0 is one block for every problem, ctrl_step_stride = 0 one
   block for the whole horizon; a non-zero step stride is at least nu, and a
   non-zero ctrl_stride holds what a problem reads (nu floats, or the H rows
   of its schedule: ctrl_step_stride (H - 1) + nu).  Each value is clamped to
   the actuator's ctrlrange where the model limits it, as the model's own
   control is when an engine is built.  Read when the kernel runs
   (graph-capturable; a replay sees new contents), never written.  Per
   problem, not per candidate.  ctrl = NULL keeps the model's own controls.
   MPCR_EINVAL: a model without actuators, host memory, a stride out of range.
   MPCR_EMODEL: an implicitfast model with a velocity-dependent actuator gain
   (gaintype affine, gainprm[2] != 0), whose implicit matrix is derived from
   the controls once, when the engine is built. */
int mpcr_rollout_cost_ctrl(mpcr_engine* e, const float* input, int layout, int nprob, int n_per,
                           const float* params, const float* start, int start_stride, float* final_state,
                           const float* ctrl, int ctrl_stride, int ctrl_step_stride, float* cost4, float* theta,
                           float* thetadot, uint64_t* best_keys, int index_base, int* status, int flags,
                           void* stream);

/* mpcr_rollout_cost_ctrl with the static collision geoms' world poses as an
   input of the call (a backward-compatible addition; mpcr_rollout_cost_ctrl
   is this call with geom_pose = NULL).  geom_pose (nullable): device memory,
   16-byte aligned, blocks of ngeom rows of 8 floats in the order of
   mpcr_model_geom_poses, row i = x y z 0 | qw qx qy qz: world position and
   unit world quaternion, used as they are.  Only rows of static geoms are
   read.  Step t of problem p reads the block at geom_pose + p geom_stride +
   t geom_step_stride (strides in floats, multiples of 4): geom_stride = 0 is
   one block for every problem, geom_step_stride = 0 one block for the whole
   horizon; a non-zero step stride is at least 8 ngeom, and a non-zero
   geom_stride holds what a problem reads (8 ngeom floats, or the H blocks of
   its schedule: geom_step_stride (H - 1) + 8 ngeom).  What moves is the
   collision geometry; tendon sites and equality anchors on static bodies
   keep their model pose.  Read when the kernel runs (graph-capturable; a
   replay sees new contents), never written.  Per problem, not per candidate.
   A block holding the model's own values (mpcr_model_geom_poses) is bitwise
   the call without one; a block taken from an edited model is bitwise an
   engine made from that model.  geom_pose = NULL keeps the model's poses.
   MPCR_EINVAL: a model without a static collision geom, host memory, a
   misaligned pointer or stride, a stride out of range. */
int mpcr_rollout_cost_world(mpcr_engine* e, const float* input, int layout, int nprob, int n_per,
                            const float* params, const float* start, int start_stride, float* final_state,
                            const float* ctrl, int ctrl_stride, int ctrl_step_stride, const float* geom_pose,
                            int geom_stride, int geom_step_stride, float* cost4, float* theta, float* thetadot,
                            uint64_t* best_keys, int index_base, int* status, int flags, void* stream);

/* mpcr_rollout_cost_world with the pose the end effector is priced against
   as an input of the call (a backward-compatible addition;
   mpcr_rollout_cost_world is this call with target = NULL).  target
   (nullable): device memory, 16-byte aligned, rows of 8 floats, x y z 0 |
   qw qx qy qz: floats 12..19 of a parameter block (ptgt | qtgt).  Float 3 is
   reserved and never read; the quaternion may have any norm and is
   normalised by the kernel exactly as the parameter block's is.  Step t of
   problem p reads the row at target + p target_stride + t target_step_stride
   (strides in floats, multiples of 4): target_stride = 0 is one schedule for
   every problem, target_step_stride = 0 one row for the whole horizon; a
   non-zero step stride is at least 8, and a non-zero target_stride holds what
   a problem reads (target_step_stride (H - 1) + 8).  With a schedule the
   parameter block's own ptgt / qtgt are not used; its init_pos and weights
   are.  Only the cost's goal and rotation terms, the total and the best key
   depend on it: cost4's collision column, theta, thetadot, final_state and
   status are bitwise the call without one.  Read when the kernel runs
   (graph-capturable; a replay sees new contents), never written.  Per
   problem, not per candidate.  A schedule repeating the parameter block's
   target is bitwise the call without one.  target = NULL keeps the parameter
   block's target.  MPCR_EINVAL: host memory, a misaligned pointer or stride,
   a stride out of range. */
int mpcr_rollout_cost_target(mpcr_engine* e, const float* input, int layout, int nprob, int n_per,
                             const float* params, const float* start, int start_stride, float* final_state,
                             const float* ctrl, int ctrl_stride, int ctrl_step_stride, const float* geom_pose,
                             int geom_stride, int geom_step_stride, const float* target, int target_stride,
                             int target_step_stride, float* cost4, float* theta, float* thetadot,
                             uint64_t* best_keys, int index_base, int* status, int flags, void* stream);

/* mpcr_rollout_cost_target with the price of each robot-masked contact slot
   as an input of the call (a backward-compatible addition;
   mpcr_rollout_cost_target is this call with slot_w = NULL).  slot_w
   (nullable): device memory, 16-byte aligned, nslot floats in slot order
   (mpcr_model_slots).  With a block
     cost_c = sum_s sum_t w[s] ([d_t,s < 0] + [t > 0] relu(0.995 d_t-1,s - d_t,s))
   and cost = w_pos cost_g + w_rot cost_r + w_col cost_c as ever; the best key
   follows the total.  The values are used as they are (0 permits a contact,
   2 charges it double).  Problem p reads the block at slot_w + p
   slot_w_stride (floats, a multiple of 4): 0 is one block for every problem,
   otherwise at least nslot.  There is no per-step stride.  Cost only: a block
   of all ones is bitwise the call without one in every output; any block
   leaves cost4's goal and rotation columns, theta, thetadot, final_state and
   status bitwise unchanged; which contacts act on the dynamics does not
   depend on it.  Doubling every weight and doubling w_col scale cost_c alike
   to fp32 rounding, not bitwise.  Read when the kernel runs (graph-capturable;
   a replay sees new contents), never written.  MPCR_EINVAL: host memory, a
   misaligned pointer, a stride that is no multiple of 4 or below nslot, a
   model without slots (nslot = 0: the dual-arm scene), host parameters. */
int mpcr_rollout_cost_slotw(mpcr_engine* e, const float* input, int layout, int nprob, int n_per,
                            const float* params, const float* start, int start_stride, float* final_state,
                            const float* ctrl, int ctrl_stride, int ctrl_step_stride, const float* geom_pose,
                            int geom_stride, int geom_step_stride, const float* target, int target_stride,
                            int target_step_stride, const float* slot_w, int slot_w_stride, float* cost4,
                            float* theta, float* thetadot, uint64_t* best_keys, int index_base, int* status,
                            int flags, void* stream);

/* mpcr_rollout_cost_slotw with the weight of each step's cost terms as an
   input of the call (a backward-compatible addition; mpcr_rollout_cost_slotw
   is this call with step_w = NULL): running against terminal cost, a
   discount, a term that counts only on arrival.  step_w (nullable): device
   memory, 16-byte aligned, H contiguous rows of 4 floats, a_pos a_rot a_col 0
   (float 3 is reserved and never read).  With a schedule
     cost_g = sum_t a_pos[t] |p_t - ptgt_t|
     cost_r = sum_t a_rot[t] 2 acos(clamp(|q_t . qtgt_t| / |q_t|))
     cost_c = sum_t sum_s (a_col[t] w[s]) ([d_t,s < 0] + [t > 0] relu(0.995 d_t-1,s - d_t,s))
   and cost = w_pos cost_g + w_rot cost_r + w_col cost_c as ever; the best key
   follows the total.  t is the absolute step of the horizon; the approach
   term of step t is priced by row t; w[s] is the slot-weight block, or 1.  The
   values are used as they are (0 switches a step off, values may exceed 1).
   Problem p reads rows step_w + p step_w_stride + 4 t: the stride is in
   floats, a multiple of 4, and 0 (one schedule for every problem) or at least
   4 H.  There is no step stride.  Cost only: a schedule of all ones is
   bitwise the call without one in every output (one multiply per term, the
   sums in the order they had); any schedule leaves theta, thetadot,
   final_state and status bitwise unchanged; a schedule that differs from ones
   in one column leaves the other two cost columns bitwise unchanged; the slot
   history records every distance, and which contacts act on the dynamics
   does not depend on it.  Read when the kernel runs (graph-capturable; a
   replay sees new contents), never written.  A model without slots takes a
   schedule (a_pos and a_rot).  MPCR_EINVAL: host memory, a misaligned
   pointer, a stride that is no multiple of 4 or lies in (0, 4 H), host
   parameters. */
int mpcr_rollout_cost_stepw(mpcr_engine* e, const float* input, int layout, int nprob, int n_per,
                            const float* params, const float* start, int start_stride, float* final_state,
                            const float* ctrl, int ctrl_stride, int ctrl_step_stride, const float* geom_pose,
                            int geom_stride, int geom_step_stride, const float* target, int target_stride,
                            int target_step_stride, const float* slot_w, int slot_w_stride, const float* step_w,
                            int step_w_stride, float* cost4, float* theta, float* thetadot, uint64_t* best_keys,
                            int index_base, int* status, int flags, void* stream);

/* Fold the costs of candidates that were rolled out in several scenarios
   (world hypotheses) into one row each.  cost4_scen holds nprob nscen n_per
   rows of 4 (a rollout's cost4: total | goal | rotation | collision):
   candidate i of problem p in scenario s is row (p nscen + s) n_per + i.
   Among a candidate's nscen rows the `worst` with the largest total are
   selected -- NaN above everything, then descending, -0 == +0, ties to the
   lower scenario -- and each column of cost4[(p n_per + i) 4 ..] is the fp32
   sum of that column over the selected rows, added in ascending scenario
   order one after the other starting from the first, divided (IEEE) by
   (float)worst.  worst = nscen is the mean, worst = 1 the worst scenario's
   own row, values between them the mean of the worst few (a CVaR).
   best_keys (nullable, nprob entries) receives the atomic minimum of the
   packed key of the aggregated total, NaN first, low word index_base + i
   (mpcr_best_key_decode; the key mpcr_argmin computes over the column);
   MPCR_F_RESET_BEST resets all nprob keys first.  1 <= worst <= nscen <= 64,
   nprob nscen n_per <= max_n.  Device pointers only, both arrays 16-byte
   aligned; no allocation, graph-capturable. */
int mpcr_scenario_reduce(mpcr_engine* e, const float* cost4_scen, int nprob, int nscen, int n_per, int worst,
                         float* cost4, uint64_t* best_keys, int index_base, int flags, void* stream);

/* One set of candidates priced in several scenarios (a backward-compatible
   addition like the *_multi calls): mpcr_rollout_cost_world over nprob nscen
   rollout problems, r = p nscen + s being scenario s of problem p, followed
   by mpcr_scenario_reduce.  Rollout problem r is an ordinary problem of that
   call -- its own block params + 20 r, its own start, ctrl and geom-pose
   block (the strides are per rollout problem) and its own n_per rows of
   cost4_scen, status and final_state (nprob nscen n_per rows each) -- except
   that the nscen scenarios of problem p all read rows [p n_per, (p + 1)
   n_per) of input (nprob n_per rows), so the samples exist once.  theta and
   thetadot (nullable, nprob n_per rows) are written by scenario 0, the
   nominal one: thetadot depends on the input alone, theta is scenario 0's
   trajectory.  cost4_scen is required.  cost4 (nullable, nprob n_per rows of
   4) receives the fold with `worst`; NULL skips that launch.  best_keys
   (nullable, nprob entries; needs cost4) comes from the fold.  Each
   scenario's slice is bitwise what mpcr_rollout_cost_world computes for that
   scenario's blocks alone, and nscen = 1 is bitwise that call in every
   output, with cost4 equal to cost4_scen.  Two launches on the caller's
   stream; graph-capturable.  MPCR_EINVAL: nscen outside [1, 64], worst
   outside [1, nscen], nprob nscen n_per > max_n, host pointers, best_keys
   without cost4, and whatever mpcr_rollout_cost_world refuses. */
int mpcr_rollout_cost_scenarios(mpcr_engine* e, const float* input, int layout, int nprob, int nscen, int worst,
                                int n_per, const float* params, const float* start, int start_stride,
                                float* final_state, const float* ctrl, int ctrl_stride, int ctrl_step_stride,
                                const float* geom_pose, int geom_stride, int geom_step_stride, float* cost4_scen,
                                float* cost4, float* theta, float* thetadot, uint64_t* best_keys, int index_base,
                                int* status, int flags, void* stream);

/* mpcr_rollout_cost_scenarios with a target schedule (a backward-compatible
   addition; mpcr_rollout_cost_scenarios is this call with target = NULL):
   target, target_stride and target_step_stride as in
   mpcr_rollout_cost_target, the strides per rollout problem r = p nscen + s,
   so each scenario may carry its own hypothesis of where the target goes.
   Each scenario's slice is bitwise what mpcr_rollout_cost_target computes
   for that scenario's blocks alone. */
int mpcr_rollout_cost_scenarios_target(mpcr_engine* e, const float* input, int layout, int nprob, int nscen,
                                       int worst, int n_per, const float* params, const float* start,
                                       int start_stride, float* final_state, const float* ctrl, int ctrl_stride,
                                       int ctrl_step_stride, const float* geom_pose, int geom_stride,
                                       int geom_step_stride, const float* target, int target_stride,
                                       int target_step_stride, float* cost4_scen, float* cost4, float* theta,
                                       float* thetadot, uint64_t* best_keys, int index_base, int* status, int flags,
                                       void* stream);

/* mpcr_rollout_cost_scenarios_target with slot weights (a backward-compatible
   addition; mpcr_rollout_cost_scenarios_target is this call with slot_w =
   NULL): slot_w and slot_w_stride as in mpcr_rollout_cost_slotw, the stride
   per rollout problem r = p nscen + s, so each hypothesis may price its own
   contacts.  The same invariants hold: ones are bitwise the call without a
   block, any block moves only the collision column, the total, the fold and
   the keys.  Each scenario's slice is bitwise what mpcr_rollout_cost_slotw
   computes for that scenario's blocks alone. */
int mpcr_rollout_cost_scenarios_slotw(mpcr_engine* e, const float* input, int layout, int nprob, int nscen,
                                      int worst, int n_per, const float* params, const float* start,
                                      int start_stride, float* final_state, const float* ctrl, int ctrl_stride,
                                      int ctrl_step_stride, const float* geom_pose, int geom_stride,
                                      int geom_step_stride, const float* target, int target_stride,
                                      int target_step_stride, const float* slot_w, int slot_w_stride,
                                      float* cost4_scen, float* cost4, float* theta, float* thetadot,
                                      uint64_t* best_keys, int index_base, int* status, int flags, void* stream);

/* mpcr_rollout_cost_scenarios_slotw with step weights (a backward-compatible
   addition; mpcr_rollout_cost_scenarios_slotw is this call with step_w =
   NULL): step_w and step_w_stride as in mpcr_rollout_cost_stepw, the stride
   per rollout problem r = p nscen + s, so each hypothesis may have its own
   schedule.  The same invariants hold.  Each scenario's slice is bitwise what
   mpcr_rollout_cost_stepw computes for that scenario's blocks alone. */
int mpcr_rollout_cost_scenarios_stepw(mpcr_engine* e, const float* input, int layout, int nprob, int nscen,
                                      int worst, int n_per, const float* params, const float* start,
                                      int start_stride, float* final_state, const float* ctrl, int ctrl_stride,
                                      int ctrl_step_stride, const float* geom_pose, int geom_stride,
                                      int geom_step_stride, const float* target, int target_stride,
                                      int target_step_stride, const float* slot_w, int slot_w_stride,
                                      const float* step_w, int step_w_stride, float* cost4_scen, float* cost4,
                                      float* theta, float* thetadot, uint64_t* best_keys, int index_base, int* status,
                                      int flags, void* stream);

/* Closed-loop plant: one environment of the model, stepped by the rollout
   kernel (fp32 state resident on the device).  Created at the template
   state (qpos_init, qvel_init, zero warm start). */
typedef struct mpcr_plant mpcr_plant;
int mpcr_plant_create(const mpcr_model* m, int device, mpcr_plant** out);
void mpcr_plant_free(mpcr_plant* p);
/* Overwrite the state (NULL leaves a part unchanged): qpos[nq], qvel[nv],
   qacc_warmstart[nv]. */
int mpcr_plant_set_state(mpcr_plant* p, const double* qpos, const double* qvel, const double* qacc_warmstart);
/* Read qpos[nq], qvel[nv], qacc[nv] (of the last step / forward) and eef[7] =
   tcp site position | hande body quaternion (wxyz) evaluated at the state the
   last step / forward started from (mj_step's kinematics run before the
   integration).  NULL skips a part. */
int mpcr_plant_get_state(mpcr_plant* p, double* qpos, double* qvel, double* qacc, double* eef);
/* commit = 1: mj_step with qvel[:nctrl] = qvel_ctrl first (NULL keeps the
   current velocities).  commit = 0: mj_forward, the state is not advanced.
   Blocks until done. */
int mpcr_plant_step(mpcr_plant* p, const double* qvel_ctrl, int commit, void* stream);
/* Asynchronous device-to-device copy of the plant's state block
   (mpcr_state_layout) to d_dst on stream: a planner's start state
   (mpcr_rollout_cost_state) without a host round trip. */
int mpcr_plant_copy_state(mpcr_plant* p, float* d_dst, void* stream);
/* The plant's actuator controls from now on: ctrl[nu], clamped to ctrlrange
   where the model limits it; NULL restores the model's own.  Blocks until
   done.  Errors as mpcr_rollout_cost_ctrl's for the model. */
int mpcr_plant_set_ctrl(mpcr_plant* p, const double* ctrl);
/* The plant's static geom poses from now on: the static rows of a host
   geom-pose block (mpcr_model_geom_poses' layout), used as they are; NULL
   restores the model's own.  Blocks until done.  MPCR_EINVAL: a model without
   a static collision geom. */
int mpcr_plant_set_geom_poses(mpcr_plant* p, const float* block);

/* argmin over cost[i*stride] with NaN-first / first-index semantics
   (jnp.argmin).  key_out (device, nullable) receives the packed key. */
int mpcr_argmin(mpcr_engine* e, const float* cost, int stride, int n, int index_base, uint64_t* key_out,
                int* idx_out, float* val_out, int flags, void* stream);

/* decode a packed best key */
void mpcr_best_key_decode(uint64_t key, int* idx, float* cost);

/* indices of the k smallest of cost[i*stride], ascending, NaN last, ties by
   index, -0 == +0 (jnp.argsort is stable): compute_ellite_samples.
   k <= min(n, 4096).  Host pointers: n <= max_n and stride <= 4. */
int mpcr_topk(mpcr_engine* e, const float* cost, int stride, int n, int k, int* idx_out, int flags,
              void* stream);

/* mpcr_topk for nprob problems in one launch (one workgroup each): problem p
   selects among cost[(p n_per + i) stride], i < n_per, and writes its k
   indices, local to the problem, to idx_out + p k (compute_ellite_samples,
   mjx_planner.py:305-310, per problem).  Device pointers only;
   k <= min(n_per, 4096), nprob n_per <= max_n. */
int mpcr_topk_multi(mpcr_engine* e, const float* cost, int stride, int nprob, int n_per, int k, int* idx_out,
                    int flags, void* stream);

/* ---- the CEM distribution step (device pointers only: MPCR_F_DEVICE_PTRS) ----
   num_dof <= 8 joints, nbasis = 11 (order-10 Bernstein), P/Pdot/Pddot
   horizon x nbasis row-major fp64 (bernstein_coeff_ordern_new).  qinv
   (nullable): the (nv+5nd)^2 fp64 KKT inverse; NULL computes get_Q_inv's
   matrix (fp32 Gram blocks, fp64 inverse, rho_ineq = 1). */
int mpcr_cem_create(int device, int num_dof, int horizon, int nbasis, const double* P, const double* Pdot,
                    const double* Pddot, const double* qinv, int max_n, mpcr_cem** out);
void mpcr_cem_free(mpcr_cem* c);

/* L = chol(cov + reg I) (nv x nv fp32, reg = 0.003 in the reference) into the
   context, for the next sampling call.  Non-PD input yields NaN samples. */
int mpcr_cem_factor(mpcr_cem* c, const float* cov, float reg, int flags, void* stream);

/* Fused sampling + projection for n candidates.
   mean != NULL: xi_samples = mean + z L^T with z ~ N(0, I) from Philox4x32-10
     keyed by seed, counter = (call counter), element (candidate, joint, block)
     -- independent of the launch shape; written to xi_samples if non-NULL.
   mean == NULL: the samples are read from xi_in (n x nv).
   Then maxiter ADMM iterations onto |Pdot xi| <= bounds[0], |Pddot xi| <=
   bounds[1], |P xi| <= bounds[2] with the boundary equalities b_eq
   (n x 5nd, per joint (theta0, thetadot0, thetaddot0, 0, 0); beq_stride 0 =
   one row shared by all candidates) and multiplier step rho; maxiter = 0
   returns the samples.  xi_out n x nv. */
int mpcr_cem_sample_project(mpcr_cem* c, int n, const float* mean, uint64_t seed, uint64_t counter,
                            int index_base, const float* xi_in, float* xi_samples, const float* b_eq, int beq_stride, int maxiter,
                            const float* bounds, float rho, float* xi_out, int flags, void* stream);
/* projection only (compute_projection_filter) */
int mpcr_project(mpcr_cem* c, const float* xi, const float* b_eq, int beq_stride, int n, int maxiter,
                 const float* bounds, float rho, float* xi_out, int flags, void* stream);

/* Elite moments, in place: w = exp(-(c - min c)/lamda) over the k elites
   xi[elite_idx[i]] (n x nv rows), cost[elite_idx[i]*stride];
   mean <- (1-alpha_mean) mean + alpha_mean sum(w xi)/sum(w);
   cov  <- (1-alpha_cov) cov + alpha_cov sum(w d d^T)/sum(w) + reg I, d = xi - mean_new.
   k <= 4096. */
int mpcr_cem_update(mpcr_cem* c, const float* xi, int n, const float* cost, int stride, const int* elite_idx, int k,
                    float lamda, float alpha_mean, float alpha_cov, float reg, float* mean, float* cov, int flags,
                    void* stream);

/* ---- several problems per call: one workgroup (factor, update) or one grid
   row (sample/project) per problem, each bitwise the single-problem call on
   its slice.  Problem p owns rows [p n_per, (p + 1) n_per) of xi / cost. ----
   Room for nprob Cholesky factors in the context (1 after mpcr_cem_create).
   Allocates, so call it outside a graph capture; it voids earlier factors. */
int mpcr_cem_set_problems(mpcr_cem* c, int nprob);
/* mpcr_cem_factor of cov + p nv^2 for every p < nprob (<= the set_problems
   count): the Cholesky of jax.random.multivariate_normal, mjx_planner.py:312-316 */
int mpcr_cem_factor_multi(mpcr_cem* c, const float* cov, int nprob, float reg, int flags, void* stream);
/* mpcr_cem_sample_project for nprob problems of n_per candidates: problem p
   samples around mean + p nv (NULL: reads xi_in) with factor p, Philox key
   seed + p seed_step and counter word 0 = index_base + (index within the
   problem) -- the draws of a single call with that seed; seed_step = 0 gives
   every problem the same draws -- and projects with its own boundary row
   b_eq + 5 nd p, shared by its candidates (compute_xi_samples +
   compute_projection_filter, mjx_planner.py:312-316, 180-249).  Sampling
   needs a mpcr_cem_factor_multi call that covered nprob problems. */
int mpcr_cem_sample_project_multi(mpcr_cem* c, int nprob, int n_per, const float* mean, uint64_t seed,
                                  uint64_t seed_step, uint64_t counter, int index_base, const float* xi_in,
                                  float* xi_samples, const float* b_eq, int maxiter, const float* bounds, float rho,
                                  float* xi_out, int flags, void* stream);
/* mpcr_cem_update per problem: elite_idx + p k holds problem p's k indices
   local to the problem (mpcr_topk_multi); mean + p nv and cov + p nv^2 are
   updated in place (compute_mean_cov / comp_prod, mjx_planner.py:318-335).
   k <= min(n_per, 4096). */
int mpcr_cem_update_multi(mpcr_cem* c, const float* xi, int nprob, int n_per, const float* cost, int stride,
                          const int* elite_idx, int k, float lamda, float alpha_mean, float alpha_cov, float reg,
                          float* mean, float* cov, int flags, void* stream);

/* ---- multi-GPU exchange over RCCL / xGMI (SURVEY.md §8b "later":
   mpcr_comm_init; §8e).  One process (or host thread) per GPU, candidates
   sharded by rank (rank r rolls out [r n, (r+1) n) with index_base = r n).
   Replaces the torch.distributed path of manipulator_mujoco_amd/dist.py for
   hosts without Python; the reference itself is single-device
   (SBP/mjx_planner.py:395 argmin, :305-310 elites).  RCCL is dlopen'ed at the
   first call (librccl.so.1).  A communicator is single-stream, like an RCCL
   communicator: mpcr_comm_gather_elites stages the local elites in scratch
   owned by the comm, so calls on one comm must be ordered on one stream (or
   use one comm per stream). */
#define MPCR_COMM_ID_BYTES 128
typedef struct mpcr_comm mpcr_comm;
/* rank 0 creates the id and hands it to the other ranks out of band */
int mpcr_comm_unique_id(unsigned char* id_out /* MPCR_COMM_ID_BYTES */);
int mpcr_comm_init(int rank, int nranks, const unsigned char* id, int device, mpcr_comm** out);
void mpcr_comm_free(mpcr_comm* c);
/* in place, device pointer: global MIN of count packed best keys (the
   rollout's fused key is unsigned-ordered, so this is the global jnp.argmin:
   NaN first, ties to the lowest global index) */
int mpcr_comm_allreduce_key(mpcr_comm* c, uint64_t* d_key, int count, void* stream);
/* rank-major all-gather of count floats per rank (device pointers) */
int mpcr_comm_allgather(mpcr_comm* c, const float* d_send, float* d_recv, size_t count, void* stream);
/* sharded elites: local top-kl (kl = min(k, n)) of d_cost[n], their rows
   (d_xi row | cost) all-gathered into d_rows (nranks x kl x (nv+1)), and
   d_sel[k] = the global top-k positions in d_rows, in the single-GPU
   argsort(kind="stable")[:k] order.  Every rank passes the same n, nv, k. */
int mpcr_comm_gather_elites(mpcr_comm* c, const float* d_cost, const float* d_xi, int n, int nv, int k, float* d_rows,
                            int* d_sel, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MPCR_H_ */
