// rollout.hip — fused basis -> H MuJoCo-semantics steps -> cost kernel for
// gfx950 (CDNA4).  One 64-lane wavefront (one workgroup) owns one candidate
// rollout for the whole horizon; per step the lanes run in parallel over
// bodies (kinematics by pointer jumping along the chain), dofs (cdof, RNE,
// passive), (dof, dof) entries (CRB mass matrix), collision pairs (narrow
// phase), (contact, dof) entries (contact Jacobians) and constraint rows
// (impedance, Newton line search).  The two dense SPD solves per step
// (M and the Newton Hessian) are done row-per-lane in registers with DPP
// row broadcasts (nv <= 16) or v_readlane (the 32-wide dual-arm variant): no
// LDS round trips inside the factorisation.  This file is the kernel; the
// device functions it calls are the headers below, one per subject.  Device
// code only, not built on
// its own: included by the two translation units that launch it,
// rollout_narrow.hip (single-arm kernels) and rollout_wide.hip (dual-arm
// kernels), each with its own flags (manipulator_mujoco_amd/build.py); host
// side in engine.hip.
//
// Semantics restated (same definitions as oracle/mpcr_oracle.c):
//   rollout / output timing  SBP/mjx_planner.py:251-274
//   cost                     SBP/mjx_planner.py:276-303
//   mjx.step                 mujoco-mjx 3.3.1 (third party)
#pragma once
#include "rollout.h"
#include "step_table.h"
// (in the order the one file had them)
#include "rollout_instruments.h"
#include "rollout_switches.h"
#include "wave.h"
#include "vecmath.h"
#include "spd_solve.h"
#include "narrow_prims.h"
#include "convex_mpr.h"
#include "manifold.h"
#include "narrow_lane.h"
#include "box_box.h"
#include "kernarg.h"
#include "contacts.h"
#include "linesearch.h"
#include "jrows.h"

namespace mpcr {

// Re-derive the model pointer from the kernel argument through an opaque
// zero offset.  The compiler then cannot hoist loop-invariant model loads out
// of the horizon loop (which kept them all live: 244 VGPRs), while the base
// stays a kernel-argument pointer so its loads remain global (uniform ones
// scalar) instead of FLAT.
#define LAUNDER_MODEL()                  \
  do {                                   \
    int z_ = 0;                          \
    asm volatile("" : "+s"(z_));         \
    m = m0 + z_;                         \
  } while (0)
// The lane index is laundered once per step the same way (narrow variant):
// otherwise every lane-mask compare (lane > k in the register Cholesky,
// lane < nv, ...) is a loop invariant the compiler hoists out of the horizon
// loop into an SGPR pair, which then spills to VGPR lanes (two v_readlane per
// use) and keeps lane-derived addresses live across the step: 178 -> 130
// VGPRs, i.e. 3 waves/SIMD instead of 2 once the LDS image fits (below).
// The dual-arm kernel too: 256 -> 241 VGPRs, scratch 304 -> 144 B, C4 49.7 -> 48.6 ms.
// (Once per step only: launders at the phase boundaries as well were not kept.)
#define LAUNDER_LANE() asm volatile("" : "+v"(lane))
// The problem of the call's candidate gi (several problems in one call,
// RolloutArgs::prob_n; 0: one problem).  A macro, so the single-arm kernels read
// prob_n before they evaluate gi, in the order the expression is written.
#define PROBLEM_OF(gi) (KA->prob_n ? (gi) / KA->prob_n : 0)

// ---------------------------------------------------------------------------
// the kernel

// Two waves per candidate, dual-arm class: wave 1 builds each Newton
// iteration's Hessian while wave 0 forms J^T f, the gradient and the stop
// test, and the implicit solve's blocked factor of M + dt D during Newton
// (hess2, impl2 in the kernel).
// The narrow variant is compiled for 4 waves/SIMD (<= 128 VGPRs; its LDS image
// fits 16 blocks per CU): at the bench's 4096 candidates = 4 per SIMD every
// candidate is resident at once (3 waves/SIMD: 3.52 ms, 4: 2.76 ms on C3).
// The dual-arm variant is compiled for 2 waves/SIMD (<= 256 registers incl.
// AGPRs; uncapped it took 274 and ran 1 wave/SIMD): with its 21.6 KB image,
// 7 blocks per CU instead of 4 (dual arm 4096 x 50: 47.5 -> 35.8 ms).
constexpr int kWideWavesPerSimd = 2, kNarrowWavesPerSimd = 4;

// WPC = waves per candidate.  WPC = 2 (narrow variant, small batches: one
// candidate per SIMD or fewer): wave 1 runs the collision
// phase while wave 0 runs the dynamics (cinert .. M^-1 qfrc_smooth) -- the two
// are independent given the step's kinematics -- and meets wave 0 at two
// workgroup barriers per step (geom poses ready; contacts ready).  Same
// instructions on the same data as WPC = 1, so the results are bitwise equal.
// MULTI: several problems in one call (RolloutArgs::prob_n > 0) -- the
// parameter block and the best key of the candidate's problem.  Its own
// instantiation, so the one-problem kernels compile from the source they had
// (the extra scalar values moved the register allocation of the whole
// kernel: C3 +0.5 % when the one kernel served both).
// STATE: a batch that starts from state blocks and / or returns its final
// states (RolloutArgs::st, mpcr_rollout_cost_state).  Its own instantiation
// for the same reason, on top of the MULTI one (which serves one problem too,
// prob_n = 0): with the eight kernels reading the pointers themselves, at the
// same resource usage, C3 measured +0.85 % per step (kernel time 1.528 ->
// 1.542 ms).  In the other instantiations the STATE terms below fold away at
// compile time.  Never the plant (plant = 0).
// SCEN: a STATE batch whose problems come in groups of scenarios that share
// their input rows (rollout.h, CallBlocks::nscen > 1; mpcr_rollout_cost_scenarios).
// Its own instantiation once more, on top of the STATE one, so the twelve
// others compile to the code they had, spill counts included -- and under
// the names they had: the flag rides on the waves-per-candidate argument
// (WPCS = WPC + WPCS_SCEN) instead of lengthening the argument list, which
// would rename every instantiation.
constexpr int WPCS_SCEN = 4;
template <int NVW, int NBW, int NGW, bool WIDE, int WPCS = 1, bool MULTI = false, bool STATE = false>
__global__ void __launch_bounds__(WAVE * (WPCS & 3), WIDE ? kWideWavesPerSimd : kNarrowWavesPerSimd)
    rollout_kernel(RolloutArgs args, const DevModel* __restrict__ mptr, StepWArgs) {  // (the third: read through KSTW)
  constexpr int WPC = WPCS & 3;
  constexpr bool SCEN = (WPCS & WPCS_SCEN) != 0;
  static_assert(WPC == 1 || WPC == 2, "waves per candidate");
  static_assert(MULTI || !STATE, "the STATE instantiations look the problem's start block up");
  static_assert(STATE || !SCEN, "scenarios are problems of a STATE launch");
#ifdef MPCR_ARGS_BY_VALUE
  StateArgs sa = {nullptr, nullptr, 0, 0, 0, nullptr, nullptr, 0, 0};
  if constexpr (STATE) sa = args.blk.st;
  constexpr unsigned aflags = 0;
#else
  // (this unit reads the arguments where it uses them: KA, KSA, ARGS_HAS)
  const unsigned aflags = args_flags(args);
#endif
  using S = typename std::conditional<WIDE, typename std::conditional<WPC == 2, SmemW2, SmemW>::type,
                                      typename std::conditional<WPC == 2, SmemN2, SmemN>::type>::type;
  const int wv = WPC == 2 ? (int)(threadIdx.x >> 6) : 0;
  const bool run_main = WPC == 1 || wv == 0, run_coll = WPC == 1 || wv == 1;
  static_assert(S::NVW == NVW && S::NBW == NBW && S::NGW == NGW, "variant widths");
  __shared__ S s;  // the candidate's LDS image
  const DevModel* __restrict__ const m0 = mptr;
  const DevModel* __restrict__ m = m0;
  int lane = threadIdx.x & (WAVE - 1);  // laundered per step (LAUNDER_LANE)
  const int b = blockIdx.x;
  if (b >= KA->n) return;
  const int H = KA->H;
  // horizon segment of this launch (dual-arm one-wave variant only)
  constexpr bool SEG = WIDE && WPC == 1;
  // lane work by kernel: the one-wave kernels only -- the two-wave kernels
  // have none of the items (with the pose cost, the centres of mass
  // and q0 built in them, C2's 1024 x 50 measured +0.5 %, past the parent's
  // pass range).  Of the one-wave kernels the STATE one takes the centres of
  // mass and q0 alone: the pose cost's three parked registers cost it two
  // scalar spills, the warm start's rows twenty spill reloads in the step loop
  // (tests/test_spill_census.py); the others fit 128 VGPRs with none new.
  constexpr bool LW_ONE = WPC == 1;
  constexpr bool LW_POSE = kLanePose<S> && LW_ONE && !STATE, LW_COM = kLaneCom<S> && LW_ONE, LW_Q0 = kLaneQ0<S> && LW_ONE;
  constexpr bool LW_JAR = kLaneJar<S> && LW_ONE && !STATE;
  const int t_begin = SEG ? KA->t0 : 0, t_end = SEG ? KA->t1 : H;
  const bool resume = SEG && t_begin > 0, suspend = SEG && t_end < H;
  float* const segs = SEG ? KA->seg_state + (size_t)b * SEG_STRIDE : nullptr;
  const int nv = m->nv, nb = m->nbody, nc = m->nctrl;
  float* const gx = S::JL < S::MAXEFC ? KA->jx + (size_t)b * (S::MAXEFC - S::JL) * S::LDJ : nullptr;
  short* const hx = S::WIDE ? KA->hints + (size_t)b * S::NHINT * 2 : nullptr;
  // mass matrix: the dense LDS image (single-arm variants), the compact LDS
  // rows of the dual-arm class (DevModel::mc_row: row i holds its tree's
  // columns; the others are 0 and rows past nv the identity), or -- a
  // dual-arm-class model whose compact M does not fit -- the candidate's HBM slab
  float* const mrow0 = S::M_SLAB ? KA->mslab + (size_t)b * NVW * S::LD : nullptr;
  const bool mcomp = S::M_SLAB && m->mc_n > 0;
  constexpr int MCW = S::MCW;
  auto m_get = [&](int i, int j) -> float {
    if constexpr (S::M_SLAB) {
      if (mcomp) {
        if (i >= nv) return i == j ? 1.f : 0.f;
        const unsigned c = (unsigned)(j - m->mc_c0[i]);
        return c < (unsigned)MCW ? s.Mc[i * MCW + c] : 0.f;
      }
      return mrow0[i * S::LD + j];
    } else {
      return s.M[i][j];
    }
  };
  auto m_set = [&](int i, int j, float v) {
    if constexpr (S::M_SLAB) {
      if (mcomp) {
        const unsigned c = (unsigned)(j - m->mc_c0[i]);
        if (i < nv && c < (unsigned)MCW) s.Mc[i * MCW + c] = v;
        return;
      }
      mrow0[i * S::LD + j] = v;
    } else {
      s.M[i][j] = v;
    }
  };
  // the window start of this lane's row (lane mod NVW), read once: the row
  // accessors below run in the Newton loop, where a dependent model load in
  // front of every LDS read cost more than the HBM slab's L2 reads had
  const int mc0_lane = S::M_SLAB ? m->mc_c0[lane & (NVW - 1)] : 0;
  // columns 4q .. 4q + 3 of row i = this lane's row (lane mod NVW)
  auto m_quad = [&](int i, int q) -> float4 {
    if constexpr (S::M_SLAB) {
      if (mcomp) {
        if (i >= nv) {
          const int k = i - 4 * q;
          return make_float4(k == 0 ? 1.f : 0.f, k == 1 ? 1.f : 0.f, k == 2 ? 1.f : 0.f, k == 3 ? 1.f : 0.f);
        }
        const unsigned c = (unsigned)(4 * q - mc0_lane);
        const float4 v = *reinterpret_cast<const float4*>(&s.Mc[i * MCW + (c & (MCW - 4))]);
        return c < (unsigned)MCW ? v : make_float4(0.f, 0.f, 0.f, 0.f);
      }
      return reinterpret_cast<const float4*>(mrow0 + i * S::LD)[q];
    } else {
      return reinterpret_cast<const float4*>(s.M[i])[q];
    }
  };
  // (M vec)[i], i = this lane's row, < nv: dotN's fmaf chain; a compact row
  // leaves out columns that are 0 (other trees') before and after its window,
  // which leaves the sum bitwise unchanged
  auto m_dot = [&](int i, const float* vec) -> float {
    if constexpr (S::M_SLAB) {
      if (mcomp) return dotN<MCW>(&s.Mc[i * MCW], vec + mc0_lane);
      return dotN<NVW>(mrow0 + i * S::LD, vec);
    } else {
      return dotN<NVW>(s.M[i], vec);
    }
  };
  // Newton Hessian H = M + J^T D_active J (+ the cone blocks) into Hs: lane
  // (row i, column quads q, q + RPW, ...) builds QPL float4s of row i, written
  // as LDS rows.  Wave 0's Newton step, or -- two waves, dual-arm class --
  // wave 1's, while wave 0 forms J^T f, the gradient and the stop test.
  auto newton_hessian = [&](int nefc, float* Hs) {
    constexpr int RPW = WAVE / NVW;
    constexpr int QPL = NVW / 4 / RPW;
    const int gi = lane & (NVW - 1), gq = lane >> S::LOG_NVW;
    float4 hq[QPL];
#pragma unroll
    for (int k = 0; k < QPL; k++) hq[k] = m_quad(gi, gq + RPW * k);
    if constexpr (NVW == 32) {  // (the narrow kernel builds H with its gradient, in the Newton loop)
      // J^T D J on v_mfma_f32_32x32x2_f32: accumulator register 4k + e of
      // lane (gi, gq) is H[gi][4 (gq + 2k) + e] in the transposed view --
      // exactly hq[k].e, the VALU build's ownership, and the same products
      // in the same row order (bitwise the VALU H)
      mfx16 acc;
#pragma unroll
      for (int k = 0; k < QPL; k++) {
        acc[4 * k] = hq[k].x; acc[4 * k + 1] = hq[k].y; acc[4 * k + 2] = hq[k].z; acc[4 * k + 3] = hq[k].w;
      }
      acc = mfma_rows32(s, gx, nefc, gi, gq, [&](int r, float a) { return s.efc_Da[r] * a; }, acc);
#pragma unroll
      for (int k = 0; k < QPL; k++) hq[k] = make_float4(acc[4 * k], acc[4 * k + 1], acc[4 * k + 2], acc[4 * k + 3]);
    }
    if constexpr (S::WIDE) {  // cone Hessian blocks J_c^T H_c J_c (wave-uniform loop)
      if (m->cone == 1)
        for (int r = 0; r < nefc; r++) {
          const int src = s.efc_src[r];
          if (!ell_head(src)) continue;
          const int p = ell_pair(src);
          const float x[3] = {s.efc_jar[r], s.efc_jar[r + 1], s.efc_jar[r + 2]};
          const float D[3] = {s.efc_D[r], s.efc_D[r + 1], s.efc_D[r + 2]};
          float f[3], h[6];
          cone_update(x, m->pair_cmu[p], m->pair_friction[p], D, f, h);
          const float* J0 = jrow_ptr(s, gx, r);
          const float* J1 = jrow_ptr(s, gx, r + 1);
          const float* J2 = jrow_ptr(s, gx, r + 2);
          const float j0 = J0[gi], j1 = J1[gi], j2 = J2[gi];
          const float c0 = h[0] * j0 + h[1] * j1 + h[2] * j2;
          const float c1 = h[1] * j0 + h[3] * j1 + h[4] * j2;
          const float c2 = h[2] * j0 + h[4] * j1 + h[5] * j2;
#pragma unroll
          for (int k = 0; k < QPL; k++) {
            const float4 v0 = reinterpret_cast<const float4*>(J0)[gq + RPW * k];
            const float4 v1 = reinterpret_cast<const float4*>(J1)[gq + RPW * k];
            const float4 v2 = reinterpret_cast<const float4*>(J2)[gq + RPW * k];
            hq[k].x += c0 * v0.x + c1 * v1.x + c2 * v2.x;
            hq[k].y += c0 * v0.y + c1 * v1.y + c2 * v2.y;
            hq[k].z += c0 * v0.z + c1 * v1.z + c2 * v2.z;
            hq[k].w += c0 * v0.w + c1 * v1.w + c2 * v2.w;
          }
        }
    }
#pragma unroll
    for (int k = 0; k < QPL; k++) reinterpret_cast<float4*>(Hs + gi * S::LD)[gq + RPW * k] = hq[k];
    sync();
  };

  // ---- rollout init: template state, qpos[:nctrl] = init_pos ----------------
  //      (plant mode: the caller's state, no init_pos override; a batch's start
  //      state, StateArgs::start: qpos | qvel | qacc_warmstart of the problem's
  //      block in the template's place, everything else as from the template)
  const bool from_state = (KA->plant & 1) != 0;
  if (run_main) {  // (WPC = 2: wave 0 sets the image up, wave 1 waits at the barrier below)
  const float* st_in = nullptr;  // STATE: the problem's start block (null: the template)
  if constexpr (MULTI) {
    // the candidate's problem (mpcr_rollout_cost_multi): wave-uniform, scalar
    const int pr = PROBLEM_OF(KA->prob_off + b);
    const float* dp = KA->dpar + (size_t)pr * PAR_N;
    if (lane < PAR_N) s.par[lane] = dp[lane];
    if constexpr (STATE) {
      if (KSA->start) st_in = KSA->start + (size_t)pr * KSA->start_stride;
      // the problem's target schedule (TargetArgs), its offset in rows' quads
      // (strides are multiples of 4 floats; the host bounds it, rollout_call),
      // kept in the image: no scalar lives across the step for it
      if (lane == 0) s.tgt_quad0 = (unsigned)(((size_t)pr * (unsigned)KTA->stride) >> 2);
    }
  } else {
    if (lane < PAR_N) s.par[lane] = KA->dpar ? KA->dpar[lane] : KA->par[lane];
  }
  if constexpr (S::SPLIT)
    if (lane == 0) s.ctok_[0] = 0;  // no step's pair cull posted yet
  if constexpr (S::WIDE) {
    // a rollout starts its hull climbs afresh; the plant keeps them across
    // steps (reset by mpcr_plant_set_state), so k plant steps = a k-step rollout
    if (!from_state && !resume) {
      int* h = reinterpret_cast<int*>(KA->hints + (size_t)b * S::NHINT * 2);
      for (int i = lane; i < S::NHINT; i += WAVE) h[i] = -1;  // both sides -1
    }
  }
  if (resume) {  // a later horizon segment: the state the previous one saved
    for (int i = lane; i < S::NQW; i += WAVE) s.qpos[i] = i < DX_NQ ? segs[SEG_QPOS + i] : 0.f;
    if (lane < NVW) {
      s.qvel[lane] = segs[SEG_QVEL + lane];
      s.qws[lane] = segs[SEG_QWS + lane];
      s.qacc[lane] = 0.f;
    }
  } else {
  // the block to start from, if any: the plant's own, or (STATE) the problem's
  const bool from_blk = STATE ? st_in != nullptr : from_state;
  const float* const blk = STATE ? st_in : KA->state;
  for (int i = lane; i < S::NQW; i += WAVE)
    s.qpos[i] = i < m->nq ? (from_blk ? blk[ST_QPOS + i] : m->qpos_init[i]) : 0.f;
  if (lane < NVW) {
    const bool v = lane < nv;
    s.qvel[lane] = v ? (from_blk ? blk[ST_QVEL + lane] : m->qvel_init[lane]) : 0.f;
    s.qws[lane] = v && from_blk ? blk[ST_QWS + lane] : 0.f;
    s.qacc[lane] = 0.f;
  }
  }
  sync();
  if (lane == 0) target_quat_unit(&s.par[PAR_QT], &s.par[PAR_QT]);  // normalise the target quaternion once
  if (lane < nc && !from_state && !resume) s.qpos[m->ctrl_qposadr[lane]] = s.par[PAR_Q0 + lane];
  sync();
  }
  if constexpr (WPC == 2) block_sync();

  // the candidate's joint velocities for the whole horizon, computed up front
  // by all lanes (theta_dot = A_thetadot xi, SBP/mjx_planner.py:348) into the
  // thetadot output (or a scratch row); each step then reads its value with a
  // load issued one step ahead, so no per-step basis latency is exposed
  // SCEN: the scenarios of a problem share its input rows -- irow, this
  // candidate's -- and scenario 0 alone writes theta and thetadot, to that row
  // (orow; -1: another scenario).  Wave-uniform scalars; b itself otherwise.
  int irow = b, orow = b;
  if constexpr (SCEN) {
    const int ns = KSCEN, pn = KA->prob_n, gi = KA->prob_off + b, pr = gi / pn, pp = pr / ns;
    irow = pp * pn + (gi - pr * pn);
    orow = pr == pp * ns ? irow : -1;
  }
  const float* tdp;
  if (KA->layout == 0) {
    // (SCEN: the other scenarios keep their own copy of the table in the scratch rows)
    float* tdw = SCEN ? (KA->thetadot && orow >= 0 ? KA->thetadot + (size_t)orow * nc * H
                                                   : KA->tdscratch + (size_t)b * nc * H)
                      : (KA->thetadot ? KA->thetadot : KA->tdscratch) + (size_t)b * nc * H;
    for (int idx = lane; run_main && !resume && idx < nc * H; idx += WAVE) {
      const int j = idx / H, tt = idx - j * H;
      const float* pd = KA->pdot + (size_t)tt * KA->nbasis;
      const float* xj = KA->input + ((size_t)(SCEN ? irow : b) * nc + j) * KA->nbasis;
      float v = 0.f;
#pragma unroll
      for (int k = 0; k < 12; k++)
        if (k < KA->nbasis) v = fmaf(pd[k], xj[k], v);
      tdw[idx] = v;
    }
    __threadfence_block();
    sync();
    if constexpr (WPC == 2) block_sync();
    tdp = tdw;
  } else {
    tdp = KA->input + (size_t)(SCEN ? irow : b) * nc * H;
  }
  float vnext = lane < nc ? tdp[lane * H + t_begin] : 0.f;
  float cost_g = 0.f, cost_r = 0.f, cost_c = 0.f;
  // Lane work, the pose cost: the three scalars of step t wait in lane t & 63
  // of these until the flush evaluates up to 64 steps' square roots, division
  // and arc cosine side by side
  float pk_d2 = 0.f, pk_qq = 0.f, pk_qd = 0.f;
  SlotHist<S> shist;
#pragma unroll
  for (int j = 0; j < SlotHist<S>::NC; j++)
#pragma unroll
    for (int c = 0; c < 4; c++) shist.v[j][c] = 0.f;
  int status = 0, nefc_sum = 0, nefc_max = 0;
  if (resume) {  // the accumulators as the previous segment left them (lane 0's scalars on every lane)
    cost_c = segs[SEG_COSTC + lane];
    const float* sc = segs + SEG_SCAL;
    cost_g = sc[0]; cost_r = sc[1];
    status = __float_as_int(sc[2]); nefc_sum = __float_as_int(sc[3]); nefc_max = __float_as_int(sc[4]);
  }
  // this lane's controlled joint addresses, held across the horizon (read
  // every step; the per-step model launder would otherwise reload them)
  const int ctrl_qa = lane < nc ? m->ctrl_qposadr[lane] : 0, ctrl_da = lane < nc ? m->ctrl_dofadr[lane] : 0;
  // STATE, dual-arm class: the problem's control block (StateArgs::ctrl;
  // null: the model's own controls, act_gain[a][3]).  Wave-uniform, a scalar
  // pair; the values themselves are loaded again every step.
  const float* ctrl_p = nullptr;
  if constexpr (STATE && S::WIDE) {
    if (KSA->ctrl) ctrl_p = KSA->ctrl + (size_t)PROBLEM_OF(KA->prob_off + b) * KSA->ctrl_stride;
  }
  // STATE: the problem's geom-pose block (StateArgs::geom_pose; null: the
  // model's own static poses, geom_pos / geom_quat).  Wave-uniform, a scalar
  // pair; the rows themselves are loaded again every step.
  const float* gpose_p = nullptr;
  if constexpr (STATE) {
    if (KSA->geom_pose)
      gpose_p = KSA->geom_pose + (size_t)PROBLEM_OF(KA->prob_off + b) * KSA->geom_stride;
  }
  PROF_DECL
  unsigned* pace = nullptr;
  int pace_own = 0;
  unsigned pace_v = ~0u;
  if (WPC == 1 && KA->pace) {
    const unsigned hw = __builtin_amdgcn_s_getreg((31 << 11) | 4);  // HW_ID
    const unsigned xcc = __builtin_amdgcn_s_getreg((3 << 11) | 20);  // XCC_ID[3:0]
    const unsigned grp = ((((xcc & 7u) * 8u + ((hw >> 13) & 7u)) * 2u + ((hw >> 12) & 1u)) * 16u + ((hw >> 8) & 15u)) *
                             4u + ((hw >> 4) & 3u);
    pace = KA->pace + grp * 16u;
    pace_own = (int)(hw & 15u);
  }
#ifdef MPCR_WAVETIME
  // diagnostic build: per-wave start / end (constant 100 MHz clock), shader
  // cycles and the hardware slot the wave ran on (load-balance study)
  const unsigned long long wt_t0 = __builtin_amdgcn_s_memrealtime(), wt_c0 = __builtin_amdgcn_s_memtime();
  unsigned wt_newton = 0, wt_ls = 0, wt_cvx = 0;  // Newton iterations, line-search passes, convex flush chunks
#endif

  // motion subspaces cdof (lanes over dofs): in the dynamics phase, or --
  // two waves per candidate -- before the first barrier, since the collision
  // wave's constraint rows need them
  auto cdof_phase = [&]() {
    if constexpr (kStepDof<S>) {
      // single-arm kernels: the dof's record of the step table (body, kind,
      // tree, free axis | joint axis | joint anchor); no anchor term when
      // every joint sits at its body's origin
      if (lane < nv) {
        const StepTable* st = step_table(m);
        const float4 d0 = recq(st->dof[lane], 0);
        const int bd = __float_as_int(d0.x), kind = __float_as_int(d0.y), tr = __float_as_int(d0.z),
                  k = __float_as_int(d0.w);
        float* c = s.cdof[lane];
        if (kind == 2) {  // free translation
          c[0] = c[1] = c[2] = 0.f;
          c[3] = k == 0 ? 1.f : 0.f;
          c[4] = k == 1 ? 1.f : 0.f;
          c[5] = k == 2 ? 1.f : 0.f;
        } else {
          float ax[3], anchor[3] = {s.xpos[bd][0], s.xpos[bd][1], s.xpos[bd][2]};
          if (kind == 3) {
            ax[0] = s.xmat[bd][k]; ax[1] = s.xmat[bd][3 + k]; ax[2] = s.xmat[bd][6 + k];  // by index, no selects
          } else {
            const float4 d1 = recq(st->dof[lane], 1);
            const float ja[3] = {d1.x, d1.y, d1.z};
            float R[9];
#pragma unroll
            for (int i = 0; i < 9; i++) R[i] = s.xmat[bd][i];
            mv(ax, R, ja);
            if (!(st->flags & ST_ANCHOR0)) {
              const float4 d2 = recq(st->dof[lane], 2);
              const float jp[3] = {d2.x, d2.y, d2.z};
              float w[3];
              mv(w, R, jp);
              anchor[0] += w[0]; anchor[1] += w[1]; anchor[2] += w[2];
            }
          }
          if (kind == 1) {
            c[0] = c[1] = c[2] = 0.f;
            c[3] = ax[0]; c[4] = ax[1]; c[5] = ax[2];
          } else {
            float off[3] = {s.com[tr][0] - anchor[0], s.com[tr][1] - anchor[1], s.com[tr][2] - anchor[2]}, cr[3];
            cross(cr, ax, off);
            c[0] = ax[0]; c[1] = ax[1]; c[2] = ax[2];
            c[3] = cr[0]; c[4] = cr[1]; c[5] = cr[2];
          }
        }
      }
    } else {
    if (lane < nv) {
      const int bd = m->dof_body[lane], kind = m->dof_kind[lane];
      const int tr = m->body_tree[bd];
      float* c = s.cdof[lane];
      float R[9];
#pragma unroll
      for (int k = 0; k < 9; k++) R[k] = s.xmat[bd][k];
      if (kind == 2) {  // free translation
        c[0] = c[1] = c[2] = 0.f;
        const int k = m->dof_sub[lane];
        c[3] = k == 0 ? 1.f : 0.f;
        c[4] = k == 1 ? 1.f : 0.f;
        c[5] = k == 2 ? 1.f : 0.f;
      } else {
        float ax[3], anchor[3];
        if (kind == 3) {
          const int k = m->dof_sub[lane];
          ax[0] = s.xmat[bd][k]; ax[1] = s.xmat[bd][3 + k]; ax[2] = s.xmat[bd][6 + k];  // by index, no selects
          anchor[0] = s.xpos[bd][0]; anchor[1] = s.xpos[bd][1]; anchor[2] = s.xpos[bd][2];
        } else {
          const int j = m->dof_jnt[lane];
          float w[3];
          mv(ax, R, m->jnt_axis[j]);
          mv(w, R, m->jnt_pos[j]);
          anchor[0] = s.xpos[bd][0] + w[0]; anchor[1] = s.xpos[bd][1] + w[1]; anchor[2] = s.xpos[bd][2] + w[2];
        }
        if (kind == 1) {
          c[0] = c[1] = c[2] = 0.f;
          c[3] = ax[0]; c[4] = ax[1]; c[5] = ax[2];
        } else {
          float off[3] = {s.com[tr][0] - anchor[0], s.com[tr][1] - anchor[1], s.com[tr][2] - anchor[2]}, cr[3];
          cross(cr, ax, off);
          c[0] = ax[0]; c[1] = ax[1]; c[2] = ax[2];
          c[3] = cr[0]; c[4] = cr[1]; c[5] = cr[2];
        }
      }
    }
    }
  };
  for (int t = t_begin; t < t_end; t++) {
    // Launder the model pointer every step: otherwise the compiler hoists
    // every loop-invariant model load out of the horizon loop and keeps them
    // all live across the whole step (244 VGPRs + SGPR spills).  The loads
    // stay in their phases and hit L1/L2.
    LAUNDER_MODEL();
    LAUNDER_LANE();
    if (pace) {  // post this step, read the SIMD mates' (consumed mid-step)
      // a plain store keeps the line in this XCD's L2 (agent scope would drop
      // it: every mate's next load then missed L2 -- the launch's largest
      // HBM stream); the readers share the CU, so their L1-bypassing (sc1)
      // loads see it in L2
      if (lane == pace_own) __hip_atomic_store(pace + lane, (unsigned)t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      if (lane < 16) pace_v = __hip_atomic_load(pace + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (run_main) {  // ---- wave 0 (WPC = 2): joint velocities .. geom poses, eef
    // ---- qvel[:nctrl] = thetadot_t ----------------------------------------------
    if (lane < nc) {
      const float v = vnext;
      if (t + 1 < H) vnext = tdp[lane * H + t + 1];  // next step's, in flight during this one
      s.qvel[ctrl_da] = v;
      if (ARGS_HAS(AF_TDOUT, KA->layout != 0 && KA->thetadot) && (!SCEN || orow >= 0))
        KA->thetadot[(size_t)(SCEN ? orow : b) * nc * H + lane * H + t] = v;
    }
    sync();

    STAMP(0);
    STOP_AT(0)
    // the call's pose of this lane's static geom for this step (STATE): in the
    // single-arm kernels its two rows are issued ahead of the kinematics and
    // consumed in the geom phase after them; the dual-arm kernels, at their
    // register limit, load them there (measured: no change against the parent,
    // where the early load cost them 0.3 - 0.6 % at 4096 x 50)
    float4 gpp = {0.f, 0.f, 0.f, 0.f}, gpq = {1.f, 0.f, 0.f, 0.f};
    bool gp_row = false;
    if constexpr (STATE && !S::WIDE) {
      if (gpose_p && lane < m->ngeom && m->geom_body[lane] < 0) {
        const float4* row = reinterpret_cast<const float4*>(gpose_p + (size_t)t * KSA->geom_step_stride) + 2 * lane;
        gpp = row[0];
        gpq = row[1];
        gp_row = true;
      }
    }
    // the call's target row of this step (STATE, TargetArgs): lane 0 loads
    // the row at the problem's parked offset (init) and refreshes the image's
    // ptgt | qtgt ahead of the pose cost, which stays as it is.  Both units
    // issue the load here, ahead of the kinematics: eight registers on one
    // lane's behalf, which the dual-arm kernels carry too (measured: loading
    // at the refresh cost their two-wave kernel 0.5 - 0.7 % at 1024 x 50)
    [[maybe_unused]] auto target_load = [&](float4& p, float4& q) -> bool {
      const float* tg = KTA->target;
      if (!tg || lane != 0) return false;
      const float4* row = reinterpret_cast<const float4*>(tg) + s.tgt_quad0 +
                          (((size_t)t * (unsigned)KTA->step_stride) >> 2);
      p = row[0];
      q = row[1];
      return true;
    };
    [[maybe_unused]] float4 tgp = {0.f, 0.f, 0.f, 0.f}, tgq = {1.f, 0.f, 0.f, 0.f};
    [[maybe_unused]] bool tg_row = false;
    if constexpr (STATE) tg_row = target_load(tgp, tgq);
    // ---- kinematics: local pose per body, then pointer jumping ----------------
    {
      float q[4] = {1.f, 0.f, 0.f, 0.f}, p[3] = {0.f, 0.f, 0.f};
      int anc = -1;
      if constexpr (kStepKin<S>) {
        // single-arm kernels: the body's record of the step table -- kind,
        // ancestor, the joint's qpos address and reference | local orientation
        // | position | axis (a slide's already in the parent frame) and, only
        // where some joint sits off its body's origin, anchor | the local
        // rotation matrix
        if (lane < nb) {
          const StepTable* st = step_table(m);
          const float4 b0 = recq(st->body[lane], 0), b1 = recq(st->body[lane], 1), b2 = recq(st->body[lane], 2);
          const int kind = __float_as_int(b0.x), qa0 = __float_as_int(b0.z);
          anc = __float_as_int(b0.y);
          q[0] = b1.x; q[1] = b1.y; q[2] = b1.z; q[3] = b1.w;
          p[0] = b2.x; p[1] = b2.y; p[2] = b2.z;
          if (kind == BK_FREE) {
            const int a = qa0;
            p[0] = s.qpos[a]; p[1] = s.qpos[a + 1]; p[2] = s.qpos[a + 2];
            q[0] = s.qpos[a + 3]; q[1] = s.qpos[a + 4]; q[2] = s.qpos[a + 5]; q[3] = s.qpos[a + 6];
            float n = sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
            if (n < kMinVal) { q[0] = 1.f; q[1] = q[2] = q[3] = 0.f; }
            else { q[0] /= n; q[1] /= n; q[2] /= n; q[3] /= n; }
          } else if (kind == BK_HINGE || kind == BK_SLIDE) {
            const float qa = s.qpos[qa0] - b0.w;
            const float4 b3 = recq(st->body[lane], 3);
            if (kind == BK_SLIDE) {
              p[0] += b3.x * qa; p[1] += b3.y * qa; p[2] += b3.z * qa;
            } else {
              float sn, cs;
              __sincosf(0.5f * qa, &sn, &cs);
              float qj[4] = {cs, b3.x * sn, b3.y * sn, b3.z * sn};
              if (!(st->flags & ST_ANCHOR0)) {
                const float4 b5 = recq(st->body[lane], 5), r0 = recq(st->body[lane], 6), r1 = recq(st->body[lane], 7),
                             r2 = recq(st->body[lane], 8);
                const float R[9] = {r0.x, r0.y, r0.z, r1.x, r1.y, r1.z, r2.x, r2.y, r2.z};
                float Rj[9], c[3] = {b5.x, b5.y, b5.z}, rc[3], d[3], w[3];
                q2m(Rj, qj);
                mv(rc, Rj, c);
                d[0] = c[0] - rc[0]; d[1] = c[1] - rc[1]; d[2] = c[2] - rc[2];
                mv(w, R, d);
                p[0] += w[0]; p[1] += w[1]; p[2] += w[2];
              }
              qmul(q, q, qj);
            }
          }
        }
      } else {
      if (lane < nb) {
        const int kind = m->body_kind[lane];
        const int j = m->body_jnt[lane];
        q[0] = m->body_bquat[lane][0]; q[1] = m->body_bquat[lane][1];
        q[2] = m->body_bquat[lane][2]; q[3] = m->body_bquat[lane][3];
        p[0] = m->body_bpos[lane][0]; p[1] = m->body_bpos[lane][1]; p[2] = m->body_bpos[lane][2];
        anc = m->body_anc[lane];
        if (kind == BK_FREE) {
          const int a = m->jnt_qposadr[j];
          p[0] = s.qpos[a]; p[1] = s.qpos[a + 1]; p[2] = s.qpos[a + 2];
          q[0] = s.qpos[a + 3]; q[1] = s.qpos[a + 4]; q[2] = s.qpos[a + 5]; q[3] = s.qpos[a + 6];
          float n = sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
          if (n < kMinVal) { q[0] = 1.f; q[1] = q[2] = q[3] = 0.f; }
          else { q[0] /= n; q[1] /= n; q[2] /= n; q[3] /= n; }
          anc = -1;
        } else if (kind == BK_HINGE || kind == BK_SLIDE) {
          const float qa = s.qpos[m->jnt_qposadr[j]] - m->jnt_qpos0[j];
          const float* ax = m->jnt_axis[j];
          float R[9];
          q2m(R, q);
          if (kind == BK_SLIDE) {
            float w[3];
            mv(w, R, ax);
            p[0] += w[0] * qa; p[1] += w[1] * qa; p[2] += w[2] * qa;
          } else {
            float sn, cs;
            __sincosf(0.5f * qa, &sn, &cs);
            float qj[4] = {cs, ax[0] * sn, ax[1] * sn, ax[2] * sn}, Rj[9], c[3], rc[3], d[3], w[3];
            c[0] = m->jnt_pos[j][0]; c[1] = m->jnt_pos[j][1]; c[2] = m->jnt_pos[j][2];
            q2m(Rj, qj);
            mv(rc, Rj, c);
            d[0] = c[0] - rc[0]; d[1] = c[1] - rc[1]; d[2] = c[2] - rc[2];
            mv(w, R, d);
            p[0] += w[0]; p[1] += w[1]; p[2] += w[2];
            qmul(q, q, qj);
          }
        }
      }
      }
      for (int r = 0; r < m->jump_rounds; r++) {
        const int src = anc >= 0 ? anc : lane;
        float aq[4], ap[3];
        aq[0] = wshfl(q[0], src); aq[1] = wshfl(q[1], src);
        aq[2] = wshfl(q[2], src); aq[3] = wshfl(q[3], src);
        ap[0] = wshfl(p[0], src); ap[1] = wshfl(p[1], src); ap[2] = wshfl(p[2], src);
        const int aanc = wshfl(anc, src);
        if (anc >= 0) {
          float R[9], w[3];
          q2m(R, aq);
          mv(w, R, p);
          p[0] = ap[0] + w[0]; p[1] = ap[1] + w[1]; p[2] = ap[2] + w[2];
          qmul(q, aq, q);
          anc = aanc;
        }
      }
      if (lane < nb) {
        float n = sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
        q[0] /= n; q[1] /= n; q[2] /= n; q[3] /= n;
        float R[9], w[3];
        q2m(R, q);
        s.xpos[lane][0] = p[0]; s.xpos[lane][1] = p[1]; s.xpos[lane][2] = p[2];
        s.xquat[lane][0] = q[0]; s.xquat[lane][1] = q[1]; s.xquat[lane][2] = q[2]; s.xquat[lane][3] = q[3];
#pragma unroll
        for (int k = 0; k < 9; k++) s.xmat[lane][k] = R[k];
        if constexpr (kStepKin<S>) {
          const float4 b4 = recq(step_table(m)->body[lane], 4);
          const float ip[3] = {b4.x, b4.y, b4.z};
          mv(w, R, ip);
        } else {
          mv(w, R, m->body_ipos[lane]);
        }
        s.xipos[lane][0] = p[0] + w[0]; s.xipos[lane][1] = p[1] + w[1]; s.xipos[lane][2] = p[2] + w[2];
      }
    }
    sync();

    STAMP(1);
    STOP_AT(1)
    // ---- geom poses, tree COMs ------------------------------------------------
    if (lane < m->ngeom) {
      const int gb = m->geom_body[lane];
      float gq[4] = {m->geom_quat[lane][0], m->geom_quat[lane][1], m->geom_quat[lane][2], m->geom_quat[lane][3]};
      if constexpr (STATE && S::WIDE) {
        if (gpose_p && gb < 0) {
          const float4* row = reinterpret_cast<const float4*>(gpose_p + (size_t)t * KSA->geom_step_stride) + 2 * lane;
          gpp = row[0];
          gpq = row[1];
          gp_row = true;
        }
      }
      if constexpr (STATE) {
        if (gp_row) { gq[0] = gpq.x; gq[1] = gpq.y; gq[2] = gpq.z; gq[3] = gpq.w; }  // the call's, as it is
      }
      float Rg[9];
      q2m(Rg, gq);
      if (gb < 0) {
        s.gxpos[lane][0] = m->geom_pos[lane][0]; s.gxpos[lane][1] = m->geom_pos[lane][1];
        s.gxpos[lane][2] = m->geom_pos[lane][2];
        if constexpr (STATE) {
          if (gp_row) { s.gxpos[lane][0] = gpp.x; s.gxpos[lane][1] = gpp.y; s.gxpos[lane][2] = gpp.z; }
        }
#pragma unroll
        for (int k = 0; k < 9; k++) s.gxmat[lane][k] = Rg[k];
      } else {
        float w[3], R[9], Rr[9];
#pragma unroll
        for (int k = 0; k < 9; k++) R[k] = s.xmat[gb][k];
        mv(w, R, m->geom_pos[lane]);
        s.gxpos[lane][0] = s.xpos[gb][0] + w[0]; s.gxpos[lane][1] = s.xpos[gb][1] + w[1];
        s.gxpos[lane][2] = s.xpos[gb][2] + w[2];
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
          for (int k = 0; k < 3; k++)
            Rr[3 * i + k] = R[3 * i] * Rg[k] + R[3 * i + 1] * Rg[3 + k] + R[3 * i + 2] * Rg[6 + k];
#pragma unroll
        for (int k = 0; k < 9; k++) s.gxmat[lane][k] = Rr[k];
      }
    }
    if constexpr (S::WIDE) {  // connect anchors in world (the body frames die with the dynamics region)
      if (lane < 2 * m->neq && m->eq_type[lane >> 1] == 0) {
        const int e = lane >> 1, side = lane & 1;
        const int bb = side ? m->eq_b2[e] : m->eq_b1[e];
        const float* a = &m->eq_data[e][4 * side];
        float pw[3] = {a[0], a[1], a[2]};
        if (bb >= 0) {
          float R[9], w[3];
#pragma unroll
          for (int k = 0; k < 9; k++) R[k] = s.xmat[bb][k];
          mv(w, R, a);
          pw[0] = s.xpos[bb][0] + w[0]; pw[1] = s.xpos[bb][1] + w[1]; pw[2] = s.xpos[bb][2] + w[2];
        }
        s.eqp[e][side][0] = pw[0]; s.eqp[e][side][1] = pw[1]; s.eqp[e][side][2] = pw[2];
      }
      if (lane < 2 * m->nten) {  // spatial-tendon sites in world
        const int t = lane >> 1, side = lane & 1, bb = m->ten_body[t][side];
        const float* a = m->ten_pos[t][side];
        float pw[3] = {a[0], a[1], a[2]};
        if (bb >= 0) {
          float R[9], w[3];
#pragma unroll
          for (int k = 0; k < 9; k++) R[k] = s.xmat[bb][k];
          mv(w, R, a);
          pw[0] = s.xpos[bb][0] + w[0]; pw[1] = s.xpos[bb][1] + w[1]; pw[2] = s.xpos[bb][2] + w[2];
        }
        s.tenp[t][side][0] = pw[0]; s.tenp[t][side][1] = pw[1]; s.tenp[t][side][2] = pw[2];
      }
    }
    // Lane work: row tr of the wave (lanes 16 tr + i) sums tree tr, lane i of
    // the row holding what lane i holds in the loop below -- the in-row steps
    // see the same operands in the same positions, so lane 15 of the row ends
    // with wsum_lo<16>'s sum (its -0 restoration done here on the lane), and
    // the rows' last lanes divide together.
    bool com_rows = false;
    if constexpr (LW_COM && NBW == 16)
      com_rows = !(m->disableflags & DEV_NO_LANE_WORK) && m->ntree <= WAVE / 16;
    if (com_rows) {
      const int tr = lane >> 4, i = lane & 15;
      const bool row = tr < m->ntree;
      const float mm = (row && i < nb && m->body_tree[i] == tr) ? m->body_mass[i] : 0.f;
      const bool in = row && i < nb;
      const float tm = row ? m->tree_mass[tr] : 1.f;  // (ahead of the sums: its wait hides behind them)
      float c[3];
#pragma unroll
      for (int k = 0; k < 3; k++) {
        c[k] = wsum_row(mm * (in ? s.xipos[i][k] : 0.f));
        if (__float_as_uint(c[k]) == 0x80000000u) c[k] = 0.f;
      }
      if (row && i == 15) {
        s.com[tr][0] = c[0] / tm; s.com[tr][1] = c[1] / tm; s.com[tr][2] = c[2] / tm;
      }
    }
    for (int tr = 0; tr < m->ntree; tr++) {
      // (the rows above did every tree; a branch in the loop and not an else
      // around it, so that the kernels without the rows keep the loop's code)
      if constexpr (LW_COM && NBW == 16)
        if (com_rows) break;
      float mm = (lane < nb && m->body_tree[lane] == tr) ? m->body_mass[lane] : 0.f;
      float cx = wsum_lo<NBW>(mm * (lane < nb ? s.xipos[lane][0] : 0.f));
      float cy = wsum_lo<NBW>(mm * (lane < nb ? s.xipos[lane][1] : 0.f));
      float cz = wsum_lo<NBW>(mm * (lane < nb ? s.xipos[lane][2] : 0.f));
      if (lane == 0) {
        float tm = m->tree_mass[tr];
        s.com[tr][0] = cx / tm; s.com[tr][1] = cy / tm; s.com[tr][2] = cz / tm;
      }
    }
    if constexpr (STATE) {
      // this step's target into the image (the sync below orders it ahead of the pose cost)
      if (tg_row) {
        s.par[PAR_PT] = tgp.x; s.par[PAR_PT + 1] = tgp.y; s.par[PAR_PT + 2] = tgp.z;
        const float q[4] = {tgq.x, tgq.y, tgq.z, tgq.w};
        target_quat_unit(q, &s.par[PAR_QT]);
      }
    }
    sync();

    // ---- eef outputs (pre-integration) + pose cost -------------------------
    if constexpr (LW_POSE) {
      // Lane work: the step keeps what needs its LDS image -- the eef point,
      // |ep - pt|^2, eq.eq and eq.qt -- and parks the three scalars in the
      // step's lane; the square roots, the division and the arc cosine run at
      // the flush for up to 64 steps side by side.  Every lane computes lane 0's
      // scalars (the reads are broadcasts, the instructions the same), so the
      // parking needs no trip through the scalar unit.  The model scalars are
      // read together ahead of the block: one wait instead of three in a row.
      const int dfl = m->disableflags, tcpb = m->tcp_body, hndb = m->hande_body;
      const float tp[3] = {m->tcp_pos[0], m->tcp_pos[1], m->tcp_pos[2]};
      const bool pose_defer = !(dfl & DEV_NO_LANE_WORK);
      if (lane == 0 || pose_defer) {
        float ep[3] = {0.f, 0.f, 0.f}, eq[4] = {1.f, 0.f, 0.f, 0.f};
        if (tcpb >= 0) {
          float w[3], R[9];
#pragma unroll
          for (int k = 0; k < 9; k++) R[k] = s.xmat[tcpb][k];
          mv(w, R, tp);
          ep[0] = s.xpos[tcpb][0] + w[0]; ep[1] = s.xpos[tcpb][1] + w[1]; ep[2] = s.xpos[tcpb][2] + w[2];
        }
        if (hndb >= 0) {
          eq[0] = s.xquat[hndb][0]; eq[1] = s.xquat[hndb][1]; eq[2] = s.xquat[hndb][2]; eq[3] = s.xquat[hndb][3];
        }
        const float* pt = &s.par[PAR_PT];
        const float* qt = &s.par[PAR_QT];
        float dx = ep[0] - pt[0], dy = ep[1] - pt[1], dz = ep[2] - pt[2];
        if (pose_defer) {
          // (single-arm kernels: the horizon starts at 0; one opaque use of the
          // step counter, so the slot grows no induction variable of its own,
          // which cost a scalar spill)
          int slot = t;
          asm volatile("" : "+s"(slot));
          slot &= WAVE - 1;
          const float d2 = dx * dx + dy * dy + dz * dz;
          const float qq = eq[0] * eq[0] + eq[1] * eq[1] + eq[2] * eq[2] + eq[3] * eq[3];
          const float qd = eq[0] * qt[0] + eq[1] * qt[1] + eq[2] * qt[2] + eq[3] * qt[3];
          if (lane == slot) { pk_d2 = d2; pk_qq = qq; pk_qd = qd; }
          // at the last step, and every 64 steps, lanes 0 .. slot run the
          // parent's expressions on their step's scalars and the costs take the
          // results in step order: the parent's sums, operand for operand
          if (slot == WAVE - 1 || t == H - 1) {
            const float pg = sqrtf(pk_d2);
            const float qn = sqrtf(pk_qq);
            const float dq = fabsf(pk_qd / qn);
            const float pr = 2.f * acosf(clampf(dq, -1.f, 1.f));
            for (int i = 0; i <= slot; i++) {
              cost_g += rdlane(pg, i);
              cost_r += rdlane(pr, i);
            }
          }
        } else {
          cost_g += sqrtf(dx * dx + dy * dy + dz * dz);
          float qn = sqrtf(eq[0] * eq[0] + eq[1] * eq[1] + eq[2] * eq[2] + eq[3] * eq[3]);
          float dq = fabsf((eq[0] * qt[0] + eq[1] * qt[1] + eq[2] * qt[2] + eq[3] * qt[3]) / qn);
          cost_r += 2.f * acosf(clampf(dq, -1.f, 1.f));
        }
        if (lane == 0 && ARGS_HAS(AF_TRACE_EEF, KA->trace_eef)) {
          float* e = KA->trace_eef + ((size_t)b * H + t) * 7;
          e[0] = ep[0]; e[1] = ep[1]; e[2] = ep[2]; e[3] = eq[0]; e[4] = eq[1]; e[5] = eq[2]; e[6] = eq[3];
        }
        // the last step's pre-integration pose (the step first, the argument read behind it)
        // (LW_POSE: no STATE kernel here)
        if (lane == 0 && ARGS_LAST_STEP_FIRST(t, H) && KA->plant != 0 && t == H - 1) {
          float* e = KA->state + ST_EEF;
          e[0] = ep[0]; e[1] = ep[1]; e[2] = ep[2]; e[3] = eq[0]; e[4] = eq[1]; e[5] = eq[2]; e[6] = eq[3];
        }
      }
    } else
    if (lane == 0) {
      float ep[3] = {0.f, 0.f, 0.f}, eq[4] = {1.f, 0.f, 0.f, 0.f};
      if (m->tcp_body >= 0) {
        float w[3], R[9];
#pragma unroll
        for (int k = 0; k < 9; k++) R[k] = s.xmat[m->tcp_body][k];
        mv(w, R, m->tcp_pos);
        ep[0] = s.xpos[m->tcp_body][0] + w[0]; ep[1] = s.xpos[m->tcp_body][1] + w[1];
        ep[2] = s.xpos[m->tcp_body][2] + w[2];
      }
      if (m->hande_body >= 0) {
        eq[0] = s.xquat[m->hande_body][0]; eq[1] = s.xquat[m->hande_body][1];
        eq[2] = s.xquat[m->hande_body][2]; eq[3] = s.xquat[m->hande_body][3];
      }
      const float* pt = &s.par[PAR_PT];
      const float* qt = &s.par[PAR_QT];
      float dx = ep[0] - pt[0], dy = ep[1] - pt[1], dz = ep[2] - pt[2];
      // the call's step weights (STATE, StepWArgs): this step's a_pos and a_rot
      // price the two terms, one multiply each and the sums in step order (1,
      // without a schedule or in it, leaves them bitwise what they were)
      float a_pos = 1.f, a_rot = 1.f;
      if constexpr (STATE) {
        if (const float* row = step_w_row(b, t)) { a_pos = row[0]; a_rot = row[1]; }
      }
      cost_g += a_pos * sqrtf(dx * dx + dy * dy + dz * dz);
      float qn = sqrtf(eq[0] * eq[0] + eq[1] * eq[1] + eq[2] * eq[2] + eq[3] * eq[3]);
      float dq = fabsf((eq[0] * qt[0] + eq[1] * qt[1] + eq[2] * qt[2] + eq[3] * qt[3]) / qn);
      cost_r += a_rot * (2.f * acosf(clampf(dq, -1.f, 1.f)));
      if (ARGS_HAS(AF_TRACE_EEF, KA->trace_eef)) {
        float* e = KA->trace_eef + ((size_t)b * H + t) * 7;
        e[0] = ep[0]; e[1] = ep[1]; e[2] = ep[2]; e[3] = eq[0]; e[4] = eq[1]; e[5] = eq[2]; e[6] = eq[3];
      }
      // the last step's pre-integration pose (single-arm kernels: the step first, the argument read behind it)
      if (ARGS_LAST_STEP_FIRST(t, H) && (STATE ? KSA->final_state != nullptr : KA->plant != 0) && t == H - 1) {
        float* e = (STATE ? KSA->final_state + (size_t)b * ST_N : KA->state) + ST_EEF;
        e[0] = ep[0]; e[1] = ep[1]; e[2] = ep[2]; e[3] = eq[0]; e[4] = eq[1]; e[5] = eq[2]; e[6] = eq[3];
      }
    }

    if constexpr (WPC == 2) {
      if (m->coll_rows) cdof_phase();
      sync();
    }
    }  // run_main
    if constexpr (WPC == 2) block_sync();  // geom poses, tree COMs, cdof ready for both waves

    STAMP(2);
    STOP_AT(2)
    if (run_main) {  // ---- wave 0: the dynamics (cinert .. M^-1 qfrc_smooth)
    // ---- cinert, cdof (+ actuator forces) -------------------------------------
    if constexpr (S::WIDE) {
      if (lane < m->nu) {
        // the call's control of this step (STATE), issued ahead of the
        // transmission loop so the load overlaps its len / vel chain
        float cv = 0.f;
        if constexpr (STATE)
          if (ctrl_p) cv = ctrl_p[(size_t)t * KSA->ctrl_step_stride + lane];
        float len = 0.f, vel = 0.f;
        for (int k = 0; k < m->act_ntrn[lane]; k++) {
          len = fmaf(m->act_moment[lane][k], s.qpos[m->act_qadr[lane][k]], len);
          vel = fmaf(m->act_moment[lane][k], s.qvel[m->act_dof[lane][k]], vel);
        }
        const float* g = m->act_gain[lane];
        const float* bp = m->act_bias[lane];
        float gain = g[0];
        if (m->act_gaffine[lane]) gain += g[1] * len + g[2] * vel;
        const float bias = m->act_baffine[lane] ? bp[0] + bp[1] * len + bp[2] * vel : 0.f;
        float ctrl = g[3];
        if constexpr (STATE)
          if (ctrl_p) ctrl = clampf(cv, m->act_ctrlrange[lane][0], m->act_ctrlrange[lane][1]);
        s.actf[lane] = clampf(gain * ctrl + bias, m->act_frc[lane][0], m->act_frc[lane][1]);
      }
    }
    if (lane < nb) {
      const int tr = m->body_tree[lane];
      float R[9], I[6];
#pragma unroll
      for (int k = 0; k < 9; k++) R[k] = s.xmat[lane][k];
      const float* Il = m->body_Iloc[lane];
      // I_w = R Il R^T
      float A[9] = {Il[0], Il[3], Il[4], Il[3], Il[1], Il[5], Il[4], Il[5], Il[2]}, RA[9];
#pragma unroll
      for (int i = 0; i < 3; i++)
#pragma unroll
        for (int k = 0; k < 3; k++) RA[3 * i + k] = R[3 * i] * A[k] + R[3 * i + 1] * A[3 + k] + R[3 * i + 2] * A[6 + k];
      I[0] = RA[0] * R[0] + RA[1] * R[1] + RA[2] * R[2];
      I[1] = RA[3] * R[3] + RA[4] * R[4] + RA[5] * R[5];
      I[2] = RA[6] * R[6] + RA[7] * R[7] + RA[8] * R[8];
      I[3] = RA[0] * R[3] + RA[1] * R[4] + RA[2] * R[5];
      I[4] = RA[0] * R[6] + RA[1] * R[7] + RA[2] * R[8];
      I[5] = RA[3] * R[6] + RA[4] * R[7] + RA[5] * R[8];
      const float mass = m->body_mass[lane];
      float d[3] = {s.xipos[lane][0] - s.com[tr][0], s.xipos[lane][1] - s.com[tr][1],
                    s.xipos[lane][2] - s.com[tr][2]};
      const float dd = dot3(d, d);
      float* c = s.cinert[lane];
      c[0] = I[0] + mass * (dd - d[0] * d[0]);
      c[1] = I[1] + mass * (dd - d[1] * d[1]);
      c[2] = I[2] + mass * (dd - d[2] * d[2]);
      c[3] = I[3] - mass * d[0] * d[1];
      c[4] = I[4] - mass * d[0] * d[2];
      c[5] = I[5] - mass * d[1] * d[2];
      c[6] = mass * d[0]; c[7] = mass * d[1]; c[8] = mass * d[2];
      c[9] = mass;
    }
    if (WPC == 1 || !m->coll_rows) cdof_phase();
    sync();

    STAMP(3);
    STOP_AT(3)
    // ---- CRB, velocity, RNE + gravcomp (subtree sums by bitmask) -----------
    constexpr bool MFMA_DYN = NVW == 16 && NBW == 16;
    float* dscr = &s.xquat[0][0];  // xquat + xmat (256 floats) are dead after the cdof phase
    if constexpr (MFMA_DYN) {
      const int mr = lane & 15, kq = lane >> 4;
      const float* qv = s.qvel;
      const mfx4 z4 = {0.f, 0.f, 0.f, 0.f};
      // crb[b] = sum of cinert over b's subtree
      {
        const uint32_t sub = mr < nb ? m->body_submask[mr] : 0u;
        const mfx4 acc = mm16<4>([&](int, int k) { return ((sub >> k) & 1u) ? 1.f : 0.f; },
                                 [&](int k, int j) { return (k < nb && j < 10) ? s.cinert[k][j] : 0.f; }, z4, lane);
#pragma unroll
        for (int v = 0; v < 4; v++)
          if (4 * kq + v < nb && mr < 10) s.crb[4 * kq + v][mr] = acc[v];
      }
      // cvel[b] = sum over b's chain of qvel x cdof; the velocity before each
      // dof (its velmask) likewise, into the scratch for cdof_dot
      {
        const uint32_t bm = mr < nb ? m->body_dofmask[mr] : 0u, vm = mr < nv ? m->dof_velmask[mr] : 0u;
        mfx4 cv = z4, vv = z4;
#pragma unroll
        for (int s4 = 0; s4 < 4; s4++) {
          const int k = 4 * s4 + kq;
          const float q = k < nv ? qv[k] : 0.f;
          const float bcd = (k < nv && mr < 6) ? s.cdof[k][mr] : 0.f;
          cv = __builtin_amdgcn_mfma_f32_16x16x4f32(((bm >> k) & 1u) ? q : 0.f, bcd, cv, 0, 0, 0);
          vv = __builtin_amdgcn_mfma_f32_16x16x4f32(((vm >> k) & 1u) ? q : 0.f, bcd, vv, 0, 0, 0);
        }
#pragma unroll
        for (int v = 0; v < 4; v++) {
          if (4 * kq + v < nb && mr < 6) s.cvel[4 * kq + v][mr] = cv[v];
          if (mr < 6) dscr[(4 * kq + v) * 8 + mr] = vv[v];
        }
      }
      sync();
      if (lane < nv) {  // cdof_dot = cvel_before x cdof (0 for free translation)
        float v[6], r[6];
#pragma unroll
        for (int k = 0; k < 6; k++) v[k] = dscr[lane * 8 + k];
        cross_motion(r, v, s.cdof[lane]);
        const bool zero = m->dof_kind[lane] == 2;
#pragma unroll
        for (int k = 0; k < 6; k++) s.cdofdot[lane][k] = zero ? 0.f : r[k];
      }
      sync();
      // RNE accelerations: (0, -g) + sum over the chain of qvel x cdof_dot
      {
        const uint32_t bm = mr < nb ? m->body_dofmask[mr] : 0u;
        mfx4 a4;
#pragma unroll
        for (int v = 0; v < 4; v++) a4[v] = (mr >= 3 && mr < 6) ? -m->gravity[mr - 3] : 0.f;
        a4 = mm16<4>([&](int, int k) { return ((bm >> k) & 1u) ? (k < nv ? qv[k] : 0.f) : 0.f; },
                     [&](int k, int j) { return (k < nv && j < 6) ? s.cdofdot[k][j] : 0.f; }, a4, lane);
#pragma unroll
        for (int v = 0; v < 4; v++)
          if (mr < 6) dscr[128 + (4 * kq + v) * 8 + mr] = a4[v];
      }
    } else {
    for (int idx = lane; idx < nb * 10; idx += WAVE) {
      const int bb = idx / 10, k = idx - bb * 10;
      uint32_t sm = m->body_submask[bb];
      float acc = 0.f;
      while (sm) {
        const int c = __builtin_ctz(sm);
        sm &= sm - 1;
        acc += s.cinert[c][k];
      }
      s.crb[bb][k] = acc;
    }
    if (lane < nb) {  // cvel = sum over the chain of cdof * qvel
      uint32_t dm = m->body_dofmask[lane];
      float v[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      while (dm) {
        const int d = __builtin_ctz(dm);
        dm &= dm - 1;
        const float qd = s.qvel[d];
#pragma unroll
        for (int k = 0; k < 6; k++) v[k] = fmaf(s.cdof[d][k], qd, v[k]);
      }
#pragma unroll
      for (int k = 0; k < 6; k++) s.cvel[lane][k] = v[k];
    }
    if (lane < nv) {  // cdof_dot = cvel_before x cdof (0 for free translation)
      uint32_t dm = m->dof_velmask[lane];
      float v[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, r[6];
      while (dm) {
        const int d = __builtin_ctz(dm);
        dm &= dm - 1;
        const float qd = s.qvel[d];
#pragma unroll
        for (int k = 0; k < 6; k++) v[k] = fmaf(s.cdof[d][k], qd, v[k]);
      }
      cross_motion(r, v, s.cdof[lane]);
      const bool zero = m->dof_kind[lane] == 2;
#pragma unroll
      for (int k = 0; k < 6; k++) s.cdofdot[lane][k] = zero ? 0.f : r[k];
    }
    }
    sync();
    if (lane < nv) {  // f_i = crb[body(i)] * cdof_i
      float f[6];
      mul_inert_vec(f, s.crb[m->dof_body[lane]], s.cdof[lane]);
#pragma unroll
      for (int k = 0; k < 6; k++) s.fvec[lane][k] = f[k];
    }
    if (lane < nb) {  // cfrc_body = I*cacc + v x* (I v) - gravcomp wrench
      float a[6];
      if constexpr (MFMA_DYN) {
#pragma unroll
        for (int k = 0; k < 6; k++) a[k] = dscr[128 + lane * 8 + k];
      } else {
        uint32_t dm = m->body_dofmask[lane];
        a[0] = a[1] = a[2] = 0.f;
        a[3] = -m->gravity[0]; a[4] = -m->gravity[1]; a[5] = -m->gravity[2];
        while (dm) {
          const int d = __builtin_ctz(dm);
          dm &= dm - 1;
          const float qd = s.qvel[d];
#pragma unroll
          for (int k = 0; k < 6; k++) a[k] = fmaf(s.cdofdot[d][k], qd, a[k]);
        }
      }
      float f[6], iv[6], vf[6], cv[6];
#pragma unroll
      for (int k = 0; k < 6; k++) cv[k] = s.cvel[lane][k];
      mul_inert_vec(f, s.cinert[lane], a);
      mul_inert_vec(iv, s.cinert[lane], cv);
      cross_force(vf, cv, iv);
      const float gc = m->body_gravcomp[lane] * m->body_mass[lane];
      const int tr = m->body_tree[lane];
      float F[3] = {-m->gravity[0] * gc, -m->gravity[1] * gc, -m->gravity[2] * gc};
      float rr[3] = {s.xipos[lane][0] - s.com[tr][0], s.xipos[lane][1] - s.com[tr][1],
                     s.xipos[lane][2] - s.com[tr][2]}, tq[3];
      float Tv[3] = {0.f, 0.f, 0.f};
      if constexpr (S::WIDE) {  // inertia-box viscosity at xipos: v = v_com + w x rr
        const float vl = m->body_visc[lane][0], va = m->body_visc[lane][1];
        float wr[3];
        cross(wr, cv, rr);
#pragma unroll
        for (int k = 0; k < 3; k++) { F[k] += vl * (cv[3 + k] + wr[k]); Tv[k] = va * cv[k]; }
      }
      cross(tq, rr, F);
      tq[0] += Tv[0]; tq[1] += Tv[1]; tq[2] += Tv[2];
      s.cfrc[lane][0] = f[0] + vf[0] - tq[0];
      s.cfrc[lane][1] = f[1] + vf[1] - tq[1];
      s.cfrc[lane][2] = f[2] + vf[2] - tq[2];
      s.cfrc[lane][3] = f[3] + vf[3] - F[0];
      s.cfrc[lane][4] = f[4] + vf[4] - F[1];
      s.cfrc[lane][5] = f[5] + vf[5] - F[2];
    }
    sync();
    STAMP(4);
    STOP_AT(4)
    // mass matrix entries (chain-masked) + bias forces
    if constexpr (MFMA_DYN) {
      // P = fvec cdof^T (K = 6 in two instructions); M[i][j] = P[i][j] for j on
      // i's chain, mirrored to M[j][i]; the bias forces' subtree sums of cfrc
      const int mr = lane & 15, kq = lane >> 4;
      const mfx4 z4 = {0.f, 0.f, 0.f, 0.f};
      const mfx4 P = mm16<2>([&](int i, int c) { return (i < nv && c < 6) ? s.fvec[i][c] : 0.f; },
                             [&](int c, int j) { return (j < nv && c < 6) ? s.cdof[j][c] : 0.f; }, z4, lane);
      const int j = mr;
      if constexpr (kStepLoad<S>) {
        // the four rows' chain masks, the column's and its armature (the
        // diagonal's: i == j) loaded in one batch ahead of the branches (the
        // arrays hold DX_NV >= 16 entries: rows past nv read zeros)
        uint32_t cmi[4];
#pragma unroll
        for (int v = 0; v < 4; v++) cmi[v] = m->dof_chainmask[4 * kq + v];
        const uint32_t cmj = m->dof_chainmask[j];
        const float arm = m->dof_armature[j];
#pragma unroll
        for (int v = 0; v < 4; v++) {
          const int i = 4 * kq + v;
          if (i < nv && j < nv) {
            if ((cmi[v] >> j) & 1u) {
              const float x = i == j ? P[v] + arm : P[v];
              m_set(i, j, x);
              m_set(j, i, x);
            } else if (!((cmj >> i) & 1u)) {
              m_set(i, j, 0.f);
            }
          } else {
            m_set(i, j, i == j ? 1.f : 0.f);
          }
        }
      } else {
#pragma unroll
      for (int v = 0; v < 4; v++) {
        const int i = 4 * kq + v;
        if (i < nv && j < nv) {
          if ((m->dof_chainmask[i] >> j) & 1u) {
            const float x = i == j ? P[v] + m->dof_armature[i] : P[v];
            m_set(i, j, x);
            m_set(j, i, x);
          } else if (!((m->dof_chainmask[j] >> i) & 1u)) {
            m_set(i, j, 0.f);
          }
        } else {
          m_set(i, j, i == j ? 1.f : 0.f);
        }
      }
      }
      const uint32_t sub = mr < nv ? m->dof_submask[mr] : 0u;
      const mfx4 fb = mm16<4>([&](int, int b) { return ((sub >> b) & 1u) ? 1.f : 0.f; },
                              [&](int b, int c) { return (b < nb && c < 6) ? s.cfrc[b][c] : 0.f; }, z4, lane);
#pragma unroll
      for (int v = 0; v < 4; v++)
        if (mr < 6) dscr[(4 * kq + v) * 8 + mr] = fb[v];
      sync();
    } else {
    for (int idx = lane; idx < NVW * NVW; idx += WAVE) {
      const int i = idx >> S::LOG_NVW, j = idx & (NVW - 1);
      float v = 0.f;
      if (i < nv && j < nv) {
        if ((m->dof_chainmask[i] >> j) & 1u) {
#pragma unroll
          for (int k = 0; k < 6; k++) v = fmaf(s.cdof[j][k], s.fvec[i][k], v);
        } else if ((m->dof_chainmask[j] >> i) & 1u) {
#pragma unroll
          for (int k = 0; k < 6; k++) v = fmaf(s.cdof[i][k], s.fvec[j][k], v);
        }
        if (i == j) v += m->dof_armature[i];
      } else if (i == j) {
        v = 1.f;
      }
      m_set(i, j, v);
    }
    }
    if (lane < nv) {
      float f[6];
      if constexpr (MFMA_DYN) {
#pragma unroll
        for (int k = 0; k < 6; k++) f[k] = dscr[lane * 8 + k];
      } else {
      uint32_t sm = m->dof_submask[lane];
      f[0] = f[1] = f[2] = f[3] = f[4] = f[5] = 0.f;
      while (sm) {
        const int c = __builtin_ctz(sm);
        sm &= sm - 1;
#pragma unroll
        for (int k = 0; k < 6; k++) f[k] += s.cfrc[c][k];
      }
      }
      float bias = 0.f;
#pragma unroll
      for (int k = 0; k < 6; k++) bias = fmaf(s.cdof[lane][k], f[k], bias);
      float qf = -bias - m->dof_damping[lane] * s.qvel[lane];
      if constexpr (S::WIDE) {
        if (m->has_spring) qf -= m->dof_stiffness[lane] * (s.qpos[m->dof_qposadr[lane]] - m->dof_springref[lane]);
        float fa = 0.f;
        for (int k = 0; k < m->dof_actn[lane]; k++) fa = fmaf(m->dof_actm[lane][k], s.actf[m->dof_acta[lane][k]], fa);
        qf += clampf(fa, m->dof_actfrc[lane][0], m->dof_actfrc[lane][1]);
      }
      s.qfs[lane] = qf;
    } else if (lane < NVW) {
      s.qfs[lane] = 0.f;
    }
    sync();

    STAMP(5);
    STOP_AT(5)
    // ---- qacc_smooth = M^-1 qfrc_smooth (row-per-lane Cholesky) -------------
    if (blk_usable<NVW>(m)) {
      // M is block diagonal by kinematic tree: one chain for all trees
      if (lane >= nv && lane < NVW) s.qas[lane] = 0.f;
      blk_solve<NVW>(m, [&](int i, int j) { return m_get(i, j); }, s.qfs, s.qas, lane, &s.xpos[0][0]);
    } else {
      float Lm[NVW];
      if constexpr (!S::M_SLAB) {
        // single-arm kernels: the row under one predicate, as quads (an
        // element at a time, each select was an exec region of its own)
#pragma unroll
        for (int j = 0; j < NVW; j++) Lm[j] = 0.f;
        if (lane < NVW) {
#pragma unroll
          for (int q = 0; q < NVW / 4; q++) {
            const float4 v = m_quad(lane, q);
            Lm[4 * q] = v.x; Lm[4 * q + 1] = v.y; Lm[4 * q + 2] = v.z; Lm[4 * q + 3] = v.w;
          }
        }
      } else {
#pragma unroll
      for (int j = 0; j < NVW; j++) Lm[j] = lane < NVW ? m_get(lane, j) : 0.f;
      }
      // the dynamics region (xpos..fvec) is dead once M is assembled
      float x;
      if constexpr (NVW == 16) {
        float dinv;
        chol16(Lm, dinv, lane);
        x = chol16_solve<S::LD>(Lm, dinv, lane < NVW ? s.qfs[lane] : 0.f, lane, &s.xpos[0][0]);
      } else {
        chol_rows(Lm, lane);
        x = chol_solve<NVW, S::LD>(Lm, lane < NVW ? s.qfs[lane] : 0.f, lane, &s.xpos[0][0]);
      }
      if (lane < NVW) s.qas[lane] = lane < nv ? x : 0.f;
    }

    }  // run_main (dynamics)

    STAMP(6);
    STOP_AT(6)
    PACE_SETPRIO();
    // Swap mode (two waves, dual-arm class without cost slots, round 5): the
    // collision wave only culls the pairs and lists the convex ones, posts
    // the list (an LDS step token, no barrier) and goes on to their MPRs (the
    // lead flush below); wave 0, after the dynamics, runs the other pairs'
    // narrow phase, so both waves reach the manifold queue together.  The
    // contacts keep the one-wave order (these pairs' first, chunk by chunk,
    // then the convex ones).  With more convex pairs than the lead flush
    // takes, the collision wave runs that narrow phase itself, as before.
    const bool swapm = WPC == 2 && S::WIDE && m->cvx_joint && m->nslot == 0;
    // the call's step weights (STATE, StepWArgs), single-arm kernels: this
    // step's a_col, read once ahead of the collision phase on the wave that
    // prices the contacts and held in one vector register over it -- uniform,
    // but a scalar would sit on top of the phase's masks, and a read at each
    // use in emit_contacts cost the one-wave kernel two more spilled scalars.
    // emit_contacts folds it into the slot weights.  The dual-arm kernels,
    // with no vector register to spare, read it there, at the use.
    [[maybe_unused]] float a_col = 1.f;
    if constexpr (STATE && !S::WIDE) {
      if (run_coll) {
        if (const float* row = step_w_row(b, t)) a_col = row[2];
        asm volatile("" : "+v"(a_col));
      }
    }
    for (int pass = 0; pass < 2 && (run_coll || swapm); pass++) {
    bool do_list = false, do_narrow = false;
    if (run_coll) {
      if (pass == 0) { do_list = true; do_narrow = !swapm; }
      else do_narrow = swapm && s.ncvx > m->w2_lead_max;
    } else if (pass == 1) {  // wave 0 (swap mode): the list is posted for this step
      bool posted = true;
      if constexpr (S::SPLIT) {  // (bounded: a lost post flags the candidate instead of hanging the launch)
        int guard = 0;
        while (__hip_atomic_load(&s.ctok_[0], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) != t + 1 &&
               ++guard < (1 << 22))
          __builtin_amdgcn_s_sleep(1);
        // a lost post: its own status bit (MPCR_STATUS_SYNC, the outputs are
        // void), and the list is not read -- wave 1 may still be writing it
        if (guard >= (1 << 22)) { status |= 1 << 10; posted = false; }
      }
      do_narrow = posted && s.ncvx <= m->w2_lead_max;
    }
    if (do_list || do_narrow) {
    // ---- collision: lanes over pairs (typed segments); cost_c on the masked
    //      slots; active contacts compacted into the list; box-box pairs
    //      that pass the bounding-sphere cull are solved wave-cooperatively
    if (do_list) {
      if (lane == 0) { s.ncon = 0; s.ncvx = 0; }
      sync();
    }
    // (the general-convex pairs are sorted last, from DevModel::cvx_base: a
    // list-only pass starts at their chunk, a narrow-only pass ends there)
    const int k_lo = do_narrow ? 0 : m->cvx_base / WAVE, p_hi = do_list ? m->npair : min(m->npair, m->cvx_base);
    for (int k = k_lo; k * WAVE < p_hi; k++) {
      const int p = lane + k * WAVE;
      const bool valid = p < m->npair;
      // single-arm kernels: the pair's set-up record (function, slot address,
      // geoms | geom types, bounding radii, margin), two quads fetched
      // together in place of the chain pair -> geoms -> types / radii (the
      // narrow phase and emit_contacts read these two as well)
      float4 ps0 = {0.f, 0.f, 0.f, 0.f}, ps1 = ps0;
      if constexpr (kStepLoad<S>) {
        if (valid) {
          const StepPairSetup& ps = step_records(m)->pair[p];
          ps0 = recq(ps, 0);
          ps1 = recq(ps, 1);
        }
      }
      const int func = valid ? (kStepLoad<S> ? __float_as_int(ps0.x) : m->pair_func[p]) : -1;
      const bool defer = S::WIDE && func >= 9;  // general convex: the list
      bool run = valid && (defer ? do_list : do_narrow);
      if constexpr (kStepLoad<S>) {
        if (run && __float_as_int(ps0.y) < 0) {
          const int g1 = __float_as_int(ps0.z), g2 = __float_as_int(ps0.w);
          const float dx = s.gxpos[g2][0] - s.gxpos[g1][0], dy = s.gxpos[g2][1] - s.gxpos[g1][1],
                      dz = s.gxpos[g2][2] - s.gxpos[g1][2];
          if ((__float_as_int(ps1.x) & 255) != 0) {
            run = sqrtf(dx * dx + dy * dy + dz * dz) <= ps1.y + ps1.z + ps1.w;
          } else {  // plane vs the other geom's bounding sphere
            const float* R1 = s.gxmat[g1];
            run = R1[2] * dx + R1[5] * dy + R1[8] * dz <= ps1.z + ps1.w;
          }
        }
      } else
      if (run && m->pair_slotadr[p] < 0) {
        const int g1 = m->pair_g1[p], g2 = m->pair_g2[p];
        const float dx = s.gxpos[g2][0] - s.gxpos[g1][0], dy = s.gxpos[g2][1] - s.gxpos[g1][1],
                    dz = s.gxpos[g2][2] - s.gxpos[g1][2];
        if (m->geom_type[g1] != 0) {
          run = sqrtf(dx * dx + dy * dy + dz * dz) <= m->geom_rbound[g1] + m->geom_rbound[g2] + m->pair_margin[p];
          if constexpr (S::WIDE) {  // box vs the other geom's bounding sphere (exact cull, as the oracle)
            if (run && func == 9 && (m->geom_type[g1] == 6 || m->geom_type[g2] == 6)) {
              const bool b1 = m->geom_type[g1] == 6;
              const int gb = b1 ? g1 : g2;
              const float sg = b1 ? 1.f : -1.f;
              float d[3] = {sg * dx, sg * dy, sg * dz}, l[3];
              mtv(l, s.gxmat[gb], d);
              float o2 = 0.f;
#pragma unroll
              for (int k2 = 0; k2 < 3; k2++) {
                const float e = fmaxf(fabsf(l[k2]) - m->geom_size[gb][k2], 0.f);
                o2 += e * e;
              }
              run = sqrtf(o2) <= m->geom_rbound[b1 ? g2 : g1] + m->pair_margin[p];
            }
          }
        } else {  // plane vs the other geom's bounding sphere (C3: the box far above the floor)
          const float* R1 = s.gxmat[g1];
          run = R1[2] * dx + R1[5] * dy + R1[8] * dz <= m->geom_rbound[g2] + m->pair_margin[p];
        }
      }
      // general convex pairs (sorted last) that survive the cull are compacted
      // into a list and solved 64 at a time below, instead of leaving most
      // lanes of every 64-pair chunk idle behind a few MPR lanes
      if (S::WIDE && do_list) {
        const unsigned long long dm = __ballot(defer && run);
        if (defer && run) s.cvx[s.ncvx + lanes_below(dm)] = p;
        sync();
        if (lane == 0) s.ncvx += __popcll(dm);
      }
      if (!do_narrow) continue;
      float dist[4] = {1e30f, 1e30f, 1e30f, 1e30f}, pos[4][3] = {}, nrm[4][3] = {};
      int nsl = 0;
      const float4 rq[2] = {ps0, ps1};
      if (run && func != 4 && !defer) nsl = narrow_lane(m, s, hx, p, dist, pos, nrm, nullptr, rq);
      STAMP(11);
      const unsigned long long bbm = __ballot(run && func == 4);
      emit_contacts<S, STATE>(m, s, args, aflags, b, t, H, valid && func != 4 && !defer, p, nsl, dist, pos, nrm, cost_c, shist, k, rq, a_col);
      STAMP(12);
      if (bbm && !(m->disableflags & 16)) {
        unsigned long long mm = bbm;
        while (mm) {
          const int q = __builtin_ctzll(mm);
          mm &= mm - 1;
          box_box_wave(m, s, k * WAVE + q, lane);
        }
      }
      STAMP(16);
    }
    if constexpr (!S::WIDE) {
      if (s.ncon > S::MAXACT) {
        status |= 1;
        sync();
        if (lane == 0) s.ncon = S::MAXACT;
        sync();
      }
    }
    }  // do_list || do_narrow
    if constexpr (S::SPLIT) {
      if (swapm && run_coll && pass == 0) {  // post the list (every lane's entries first)
        sync();
        if (lane == 0) __hip_atomic_store(&s.ctok_[0], t + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
      }
    }
    }  // pass
    if constexpr (S::WIDE) {
      // ---- the convex flush: every general-convex pair that survived the
      //      cull (the list holds all of a model's, so this is the step's only
      //      flush), MPR per lane, then the pending manifolds wave-cooperatively
      //      one pair at a time.  Two waves per candidate (round 5): the
      //      dynamics wave joins after the mass-matrix solve and the pairs are
      //      dealt over both (item i on wave i & 1, rounds of 128), each wave
      //      running the manifolds of its own pairs with its own clip scratch;
      //      the contacts go to the list in pair order (a prefix over both
      //      waves' counts), so the list -- and every result -- is bitwise the
      //      one-wave kernel's.  Models with cost slots on convex pairs keep
      //      the flush on the collision wave (cost_c accumulates per lane).
      const bool split = WPC == 2 && m->cvx_joint;
      const bool mine = WPC == 1 || split || wv == 1;
      PolyScratchT<S::PMAXW>* const psc = reinterpret_cast<PolyScratchT<S::PMAXW>*>(
          (WPC == 2 && wv == 0) ? &s.xpos[0][0] : &s.polyw[0][0][0]);
      int* const jcnt = reinterpret_cast<int*>(&s.xpos[0][0]) + sizeof(PolyScratchT<S::PMAXW>) / 4;
      // Lead flush (two waves, round 5): with at most W2_LEAD_MAX pairs in the
      // list, the collision wave runs every pair's MPR (one lane each) as soon
      // as its list is complete -- while wave 0 still runs the dynamics --
      // and queues the polyhedron manifolds; after the hand-over both waves
      // take manifolds from the queue (an LDS counter), wave 0 returning its
      // results through a mailbox in the dead dynamics region, and the
      // collision wave emits the contacts in pair order.  Each pair's MPR and
      // manifold are the same instructions on the same data wherever they
      // run: bitwise the one-wave kernel.
      int* const jq = reinterpret_cast<int*>(&s.cvx[0]);  // [0] next job, [1] jobs, records from [2]
      float* const mbox = reinterpret_cast<float*>(jcnt);  // wave 0's manifold results, W2_JOB_OUT floats per job
      int lpc = 0, ljob = 0, lsl = 0;
      float ld[4] = {1e30f, 1e30f, 1e30f, 1e30f}, lp[4][3] = {}, ln[4][3] = {};
      if (split && wv == 1 && s.ncvx <= m->w2_lead_max) {
        const bool v = lane < s.ncvx;
        lpc = v ? s.cvx[lane] : 0;
        lsl = v ? narrow_lane(m, s, hx, lpc, ld, lp, ln, (DBG_LAST()) ? KA->dbg : nullptr)
                : 0;
        STAMP(21);
        for (unsigned long long pm = __ballot(lsl == kPendingManifold); pm; pm &= pm - 1) {
          const int q = __builtin_ctzll(pm);
          const int pq = __shfl(lpc, q);
          const float dq = __shfl(ld[0], q);
          const int gp = m->pair_g1[pq];
          const float* Rp = s.gxmat[gp];
          const float nq[3] = {Rp[2], Rp[5], Rp[8]};
          plane_mesh_manifold_wave(m, s, m->pair_g2[pq], nq, s.gxpos[gp], -dq, q, lane, ld, lp, ln, lsl);
        }
        STAMP(22);
        // the manifold queue: (pair | lane << 16, MPR depth, normal, point) per job
        const unsigned long long pm = __ballot(lsl == kPendingPoly);
        ljob = lanes_below(pm);
        if (lsl == kPendingPoly) {
          int* r = jq + 2 + W2_JOB_REC * ljob;
          r[0] = lpc | (lane << 16);
          r[1] = __float_as_int(ld[0]);
#pragma unroll
          for (int e = 0; e < 3; e++) { r[2 + e] = __float_as_int(ln[0][e]); r[5 + e] = __float_as_int(lp[0][e]); }
        }
        if (lane == 0) { jq[0] = 0; jq[1] = __popcll(pm); }
      }
      if constexpr (WPC == 2) block_sync();  // the list is complete; the dynamics are done
      const int ncv = s.ncvx, rstep = split ? 2 * WAVE : WAVE;
      const bool lead = split && ncv <= m->w2_lead_max;
      int ncon_w = s.ncon;
      if (lead) {
        STAMP(16);  // (profile build: wave 0's wait for the queue)
        const int njob = jq[1];
        for (;;) {
          int j = 0;
          if (lane == 0) j = __hip_atomic_fetch_add(jq, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          j = __builtin_amdgcn_readfirstlane(j);
          if (j >= njob) break;
          const int* r = jq + 2 + W2_JOB_REC * j;
          const int pq = r[0] & 0xffff, q = r[0] >> 16;
          const float dq = __int_as_float(r[1]);
          const float nq[3] = {__int_as_float(r[2]), __int_as_float(r[3]), __int_as_float(r[4])};
          if (wv == 0) {  // lane q stands in for the collision wave's lane q
            lsl = lane == q ? kPendingPoly : 0;
            ld[0] = dq; ld[1] = ld[2] = ld[3] = 1e30f;
#pragma unroll
            for (int e = 0; e < 3; e++) { ln[0][e] = nq[e]; lp[0][e] = __int_as_float(r[5 + e]); }
          }
          poly_manifold_wave(m, s, *psc, hx, pq, nq, -dq, q, lane, ld, lp, ln, lsl);
          if (wv == 0 && lane == q) {
            float* o = mbox + W2_JOB_OUT * j;
#pragma unroll
            for (int c = 0; c < 4; c++) {
              o[c] = ld[c];
#pragma unroll
              for (int e = 0; e < 3; e++) { o[4 + 3 * c + e] = lp[c][e]; o[16 + 3 * c + e] = ln[c][e]; }
            }
            o[28] = __int_as_float(lsl);
          }
        }
        STAMP(17);
        block_sync();  // every manifold done
        if (wv == 1) {
          if (lsl == kPendingPoly) {  // run by wave 0
            const float* o = mbox + W2_JOB_OUT * ljob;
#pragma unroll
            for (int c = 0; c < 4; c++) {
              ld[c] = o[c];
#pragma unroll
              for (int e = 0; e < 3; e++) { lp[c][e] = o[4 + 3 * c + e]; ln[c][e] = o[16 + 3 * c + e]; }
            }
            lsl = __float_as_int(o[28]);
          }
          emit_contacts<S, STATE>(m, s, args, aflags, b, t, H, lane < ncv, lpc, lsl, ld, lp, ln, cost_c, shist, -1, nullptr, a_col);
        }
        STAMP(18);
      }
      for (int i0 = 0; !lead && i0 < ncv; i0 += rstep) {
#ifdef MPCR_WAVETIME
        wt_cvx++;
#endif
        const int i = split ? i0 + 2 * lane + wv : i0 + lane;
        const bool v = mine && i < ncv;
        const int pc = v ? s.cvx[i] : 0;
        float cd[4] = {1e30f, 1e30f, 1e30f, 1e30f}, cp[4][3] = {}, cn[4][3] = {};
        int cn_sl = v ? narrow_lane(m, s, hx, pc, cd, cp, cn, (DBG_LAST()) ? KA->dbg
                                                                                           : nullptr)
                      : 0;
        STAMP(21);
        for (unsigned long long pm = __ballot(cn_sl == kPendingManifold); pm; pm &= pm - 1) {
          const int q = __builtin_ctzll(pm);  // penetrating plane-mesh pairs, one at a time, all lanes
          const int pq = __shfl(pc, q);
          const float dq = __shfl(cd[0], q);
          const int gp = m->pair_g1[pq];
          const float* Rp = s.gxmat[gp];
          const float nq[3] = {Rp[2], Rp[5], Rp[8]};
          plane_mesh_manifold_wave(m, s, m->pair_g2[pq], nq, s.gxpos[gp], -dq, q, lane, cd, cp, cn, cn_sl);
        }
        STAMP(22);
        for (unsigned long long pm = __ballot(cn_sl == kPendingPoly); pm; pm &= pm - 1) {
          const int q = __builtin_ctzll(pm);  // penetrating polyhedron pairs, one at a time, all lanes
          const int pq = __shfl(pc, q);
          const float dq = __shfl(cd[0], q);
          const float nq[3] = {__shfl(cn[0][0], q), __shfl(cn[0][1], q), __shfl(cn[0][2], q)};
          poly_manifold_wave(m, s, *psc, hx, pq, nq, -dq, q, lane, cd, cp, cn, cn_sl);
        }
        STAMP(17);
        if (split) {
          // this item's active contacts; their list offsets from both waves'
          // counts in item order (lane l holds items 2l and 2l + 1)
          int act = 0;
          if (v && !(m->disableflags & 16)) {
            const float mg = m->pair_margin[pc];
#pragma unroll
            for (int c = 0; c < 4; c++) act += (c < cn_sl && cd[c] < mg) ? 1 : 0;
          }
          jcnt[2 * lane + wv] = act;
          block_sync();
          const int a0 = jcnt[2 * lane], a1 = jcnt[2 * lane + 1];
          int tot;
          const int pre = wscan_excl<4>(a0 + a1, tot) + (wv ? a0 : 0);  // two items: up to 8
          if (act) put_contacts(m, s, ncon_w + pre, pc, cn_sl, cd, cp, cn);
          ncon_w += tot;
          block_sync();  // jcnt is the next round's
        } else if (mine) {
          emit_contacts<S, STATE>(m, s, args, aflags, b, t, H, v, pc, cn_sl, cd, cp, cn, cost_c, shist, -1, nullptr, a_col);
        }
        STAMP(18);
      }
      if (split && !lead && run_coll && lane == 0) s.ncon = ncon_w;
      sync();
      if (run_coll && s.ncon > S::MAXACT) {
        status |= 1;
        sync();
        if (lane == 0) s.ncon = S::MAXACT;
        sync();
      }
    }
    // WPC = 2 and DevModel::coll_rows: the collision wave builds the
    // constraint rows too, still beside wave 0's dynamics (they need the
    // contacts, qpos, qvel, cdof and the tree COMs, all ready before the first
    // barrier) and hands them over at the second; otherwise wave 0 builds them
    // after the contact list is handed over
    const bool rows_c = WPC == 2 && m->coll_rows;
    // two waves per candidate, dual-arm class, rows after the hand-over (round
    // 5): both waves build the constraint rows, the Jacobian entries and the
    // row parameters dealt over 128 lanes (the bookkeeping -- row counts,
    // sources, offsets -- computed identically on both), and wave 1 leaves at
    // the barrier that follows; same values in the same places as one wave
    const bool rows_j = WPC == 2 && S::WIDE && !rows_c;
    // ... and wave 1 then builds the Newton Hessians (round 5)
    const bool hess2 = rows_j && NVW == 32;
    // ... and factors the implicit solve's M + dt D (blocked path) for wave 0
    // to sweep after Newton: the factor needs only M, wave 1 is otherwise
    // idle then, and its element gather was most of the solve's time
    const bool impl2 = hess2 && S::WIDE && m->integrator == 3 && !m->impl_cross && blk_usable<NVW>(m);
    constexpr int BLK_N = NVW == 16 ? 8 : 16;
    static_assert(!S::SPLIT || (BLK_N + 1) * WAVE <= S::DYN_FLOATS, "the implicit factor inside the dynamics region");
    float* const implf = &s.xpos[0][0];  // the factor: BLK_N + 1 floats per lane (dynamics region, dead until Euler)
    const int rl0 = rows_j ? wv * WAVE : 0, rls = rows_j ? 2 * WAVE : WAVE;
    if constexpr (WPC == 2) {
      if (!rows_c) {
        block_sync();  // the contact list is ready; wave 1 waits for the next step's geom poses
        if (!run_main && !rows_j) continue;
      }
    }

    STAMP(7);
    STOP_AT(7)
    // ---- constraint rows: equality, limits, contacts ------------------------
    bool coupled = true;  // a constraint row spans two kinematic trees (Newton's H not block diagonal)
    if (WPC == 1 || rows_j || (rows_c ? run_coll : run_main)) {
      const int ncon = s.ncon;
      const int neq = (m->disableflags & 64) ? 0 : (S::WIDE ? m->neqrow : m->neq);
      int nlim_l = 0, lsides = 0;
      if constexpr (kStepRow<S>) {
        // single-arm kernels: the joint's row record of the step table
        // (margin, flags | range, qpos address)
        if (lane < m->njnt && !(m->disableflags & 32)) {
          const StepRow& rj = step_table(m)->row[ST_ROW_JNT + lane];
          const float4 j2 = recq(rj, 2), j3 = recq(rj, 3);
          if (__float_as_int(j2.z) & ST_LIMITED) {
            const float q = s.qpos[__float_as_int(j3.z)];
            if (q - j3.x < j2.x) { nlim_l++; lsides |= 1; }
            if (j3.y - q < j2.x) { nlim_l++; lsides |= 2; }
          }
        }
      } else
      if (lane < m->njnt && !(m->disableflags & 32) && m->jnt_limited[lane] &&
          (m->jnt_type[lane] == 2 || m->jnt_type[lane] == 3)) {
        const float q = s.qpos[m->jnt_qposadr[lane]];
        if (q - m->jnt_range[lane][0] < m->jnt_margin[lane]) { nlim_l++; lsides |= 1; }
        if (m->jnt_range[lane][1] - q < m->jnt_margin[lane]) { nlim_l++; lsides |= 2; }
      }
      int nlim;
      const int lim_pre = wscan_excl(nlim_l, nlim);
      // spatial-tendon limit rows after the joint limits (wave-uniform)
      int ntr = 0, tsides = 0;
      if constexpr (S::WIDE) {
        if (!(m->disableflags & 32))
          for (int t = 0; t < m->nten; t++) {
            if (!m->ten_limited[t]) continue;
            const float dx = s.tenp[t][1][0] - s.tenp[t][0][0], dy = s.tenp[t][1][1] - s.tenp[t][0][1],
                        dz = s.tenp[t][1][2] - s.tenp[t][0][2];
            const float len = sqrtf(dx * dx + dy * dy + dz * dz);
            if (len - m->ten_range[t][0] < m->ten_margin[t]) { tsides |= 1 << (2 * t); ntr++; }
            if (m->ten_range[t][1] - len < m->ten_margin[t]) { tsides |= 2 << (2 * t); ntr++; }
          }
      }
      const bool ell = S::WIDE && m->cone == 1;
      int ncr = 0;
      // single-arm kernels: quad 3 of the contact's pair row (StepPairJ), one
      // load for the row count here and the tree test below
      float4 pj = {0.f, 0.f, 0.f, 0.f};
      if constexpr (kStepLoad<S>) {
        if (lane < ncon) {
          pj = recq(step_table(m)->row[ST_ROW_PAIR + s.con_pair[lane]], 3);
          ncr = (__float_as_int(pj.z) >> 16) & 1 ? 1 : 4;
        }
      } else
      if (lane < ncon) ncr = m->pair_condim[s.con_pair[lane]] == 1 ? 1 : (ell ? 3 : 4);
      int ncrow;
      const int con_pre = wscan_excl(ncr, ncrow);
      int nefc = neq + nlim + ntr + ncrow;
      int keep_con = ncon;
      if (nefc > S::MAXEFC) {  // keep the longest prefix of contacts that fits
        const int room = S::MAXEFC - neq - nlim - ntr;
        const unsigned long long fit = __ballot(lane < ncon && con_pre + ncr <= room);
        keep_con = __popcll(fit);
        nefc = neq + nlim + ntr + (keep_con > 0 ? wshfl(con_pre + ncr, keep_con - 1) : 0);
        status |= 1;
      }
      // equality rows: joint (side 0) or connect component side - 1
      if (lane < neq)
        s.efc_src[lane] = S::WIDE ? ((1 << 24) | (m->eqrow_eq[lane] << 4) | m->eqrow_k[lane]) : ((1 << 24) | (lane << 4));
      if (nlim_l) {
        int o = neq + lim_pre;
        if (lsides & 1) s.efc_src[o++] = (2 << 24) | (lane << 4) | 0;
        if (lsides & 2) s.efc_src[o++] = (2 << 24) | (lane << 4) | 1;
      }
      if constexpr (S::WIDE) {
        if (lane == 0 && ntr) {
          int o = neq + nlim;
          for (int t = 0; t < m->nten; t++)
            for (int side = 0; side < 2; side++)
              if ((tsides >> (2 * t + side)) & 1) s.efc_src[o++] = (4 << 24) | (t << 4) | side;
        }
      }
      if (lane < keep_con) {
        const int o = neq + nlim + ntr + con_pre;
        s.con_row[lane] = o;
        if (ncr == 3) {  // elliptic (wide variant only)
          const int p = s.con_pair[lane];
          for (int r = 0; r < 3; r++) s.efc_src[o + r] = (5 << 24) | (lane << 14) | (p << 4) | r;
        } else {
          for (int r = 0; r < ncr; r++) s.efc_src[o + r] = (3 << 24) | (lane << 4) | r;
        }
      }
      {
        bool cross = false;
        if constexpr (kStepLoad<S>) {
          const int tr = __float_as_int(pj.z);
          cross = lane < keep_con && __float_as_int(pj.x) != 0 && __float_as_int(pj.y) != 0 &&
                  (tr & 255) != ((tr >> 8) & 255);
        } else
        if (lane < keep_con) {
          const int4 ji = m->pair_jinfo[s.con_pair[lane]];
          cross = ji.x != 0 && ji.y != 0 && ji.z != ji.w;
        }
        coupled = m->eq_cross || __ballot(cross) != 0ull;
      }
      if (lane == 0) s.nefc = nefc;
      sync();
      ROWS_STAMP(23);
      // Jacobian entries of equality/limit rows: (row, dof)
      const int nsimple = neq + nlim + ntr;
      if constexpr (kStepLoad<S>) {
        // single-arm kernels (equality and limit rows only): the equality's
        // record (StepEq) and the joint row's dof address, both fetched ahead
        // of the branch on the row's kind -- one wait per pass (a row of the
        // other kind reads a record it does not use: the index is masked into
        // the array)
        static_assert((ST_NEQ & (ST_NEQ - 1)) == 0 && (ST_NJ & (ST_NJ - 1)) == 0, "the masks below need powers of two");
        for (int idx = lane + rl0; idx < nsimple * NVW; idx += rls) {
          const int r = idx >> S::LOG_NVW, i = idx & (NVW - 1);
          const int src = s.efc_src[r], kind = src >> 24, id = (src >> 4) & 0xfffff, side = src & 15;
          const StepEq& eq = step_records(m)->eq[id & (ST_NEQ - 1)];
          const float4 e0 = recq(eq, 0), e1 = recq(eq, 1), e2 = recq(eq, 2);
          const int ldof = step_table(m)->row[ST_ROW_JNT + (id & (ST_NJ - 1))].dofadr;
          float v = 0.f;
          if (kind == 1) {
            if (i == __float_as_int(e0.y)) v += 1.f;
            if (__float_as_int(e0.z) >= 0 && i == __float_as_int(e0.w)) {
              const float dif = s.qpos[__float_as_int(e0.z)] - e1.y;
              v -= e1.w + dif * (2.f * e2.x + dif * (3.f * e2.y + dif * 4.f * e2.z));
            }
          } else if (i == ldof) {
            v = side == 0 ? 1.f : -1.f;
          }
          jstore(s, gx, r, i, v);
        }
      } else
      for (int idx = lane + rl0; idx < nsimple * NVW; idx += rls) {
        const int r = idx >> S::LOG_NVW, i = idx & (NVW - 1);
        const int src = s.efc_src[r], kind = src >> 24, id = (src >> 4) & 0xfffff, side = src & 15;
        float v = 0.f;
        if (S::WIDE && kind == 1 && side > 0) {  // connect: (J_p(b1, p1) - J_p(b2, p2))[side - 1]
          const int comp = side - 1;
          if (i < nv) {
            const float* cd = s.cdof[i];
#pragma unroll
            for (int e2 = 0; e2 < 2; e2++) {
              const int bb = e2 == 0 ? m->eq_b1[id] : m->eq_b2[id];
              if (bb >= 0 && ((m->body_dofmask[bb] >> i) & 1u)) {
                const int tr = m->body_tree[bb];
                float r[3] = {s.eqp[id][e2][0] - s.com[tr][0], s.eqp[id][e2][1] - s.com[tr][1],
                              s.eqp[id][e2][2] - s.com[tr][2]}, cr[3];
                cross(cr, cd, r);
                const float jv = cd[3 + comp] + cr[comp];
                v += e2 == 0 ? jv : -jv;
              }
            }
          }
        } else if (kind == 1) {
          const int j1 = m->eq_j1[id], j2 = m->eq_j2[id];
          if (i == m->jnt_dofadr[j1]) v += 1.f;
          if (j2 >= 0 && i == m->jnt_dofadr[j2]) {
            const float* c = m->eq_data[id];
            const float dif = s.qpos[m->jnt_qposadr[j2]] - m->jnt_qpos0[j2];
            v -= c[1] + dif * (2.f * c[2] + dif * (3.f * c[3] + dif * 4.f * c[4]));
          }
        } else if (S::WIDE && kind == 4) {  // tendon: +-(dif / len) . (J_p(site2) - J_p(site1))
          if (i < nv) {
            const float dif[3] = {s.tenp[id][1][0] - s.tenp[id][0][0], s.tenp[id][1][1] - s.tenp[id][0][1],
                                  s.tenp[id][1][2] - s.tenp[id][0][2]};
            const float il = 1.f / fmaxf(sqrtf(dot3(dif, dif)), kMinVal);
            const float* cd = s.cdof[i];
#pragma unroll
            for (int e2 = 0; e2 < 2; e2++) {
              const int bb = m->ten_body[id][e2];
              if (bb >= 0 && ((m->body_dofmask[bb] >> i) & 1u)) {
                const int tr = m->body_tree[bb];
                float rr[3] = {s.tenp[id][e2][0] - s.com[tr][0], s.tenp[id][e2][1] - s.com[tr][1],
                               s.tenp[id][e2][2] - s.com[tr][2]}, cr[3];
                cross(cr, cd, rr);
                const float jp = (dif[0] * (cd[3] + cr[0]) + dif[1] * (cd[4] + cr[1]) + dif[2] * (cd[5] + cr[2])) * il;
                v += e2 == 0 ? -jp : jp;
              }
            }
            if (side) v = -v;
          }
        } else if (i == m->jnt_dofadr[id]) {
          v = side == 0 ? 1.f : -1.f;
        }
        jstore(s, gx, r, i, v);
      }
      ROWS_STAMP(24);
      // contact Jacobians: (contact, dof) -> J_n +- mu J_t rows
      for (int idx = lane + rl0; idx < keep_con * NVW; idx += rls) {
        const int c = idx >> S::LOG_NVW, i = idx & (NVW - 1);
        const int p = s.con_pair[c];
        // one load: both bodies' dof masks and trees (single-arm kernels: with
        // the friction and the condim-1 bit, quad 3 of the pair's row)
        int4 ji;
        float muq = 0.f;
        bool condim1 = false;
        if constexpr (kStepLoad<S>) {
          const float4 q3 = recq(step_table(m)->row[ST_ROW_PAIR + p], 3);
          const int tr = __float_as_int(q3.z);
          ji = make_int4(__float_as_int(q3.x), __float_as_int(q3.y), tr & 255, (tr >> 8) & 255);
          condim1 = (tr >> 16) & 1;
          muq = q3.w;
        } else {
          ji = m->pair_jinfo[p];
        }
        float jd[3] = {0.f, 0.f, 0.f};
        if (i < nv) {
          const float* cd = s.cdof[i];
#pragma unroll
          for (int side = 0; side < 2; side++) {
            if (((unsigned)(side == 0 ? ji.x : ji.y) >> i) & 1u) {
              const int tr = side == 0 ? ji.z : ji.w;
              float r[3] = {s.con_pos[c][0] - s.com[tr][0], s.con_pos[c][1] - s.com[tr][1],
                            s.con_pos[c][2] - s.com[tr][2]}, cr[3];
              cross(cr, cd, r);
              const float sg = side == 0 ? -1.f : 1.f;
              jd[0] += sg * (cd[3] + cr[0]); jd[1] += sg * (cd[4] + cr[1]); jd[2] += sg * (cd[5] + cr[2]);
            }
          }
        }
        // the contact frame (the wide image keeps only its normal row: the
        // tangents are make_frame's of it, bitwise what emit computed)
        float fw[9];
        const float* f = s.con_frame[c];
        if constexpr (S::FRAMEW == 3) {
          make_frame(fw, s.con_frame[c]);
          f = fw;
        }
        const float jn = f[0] * jd[0] + f[1] * jd[1] + f[2] * jd[2];
        const int off = s.con_row[c];
        if (kStepLoad<S> ? condim1 : m->pair_condim[p] == 1) {
          jstore(s, gx, off, i, jn);
        } else if (S::WIDE && m->cone == 1) {  // elliptic: J_n, J_t1, J_t2
          jstore(s, gx, off + 0, i, jn);
          jstore(s, gx, off + 1, i, f[3] * jd[0] + f[4] * jd[1] + f[5] * jd[2]);
          jstore(s, gx, off + 2, i, f[6] * jd[0] + f[7] * jd[1] + f[8] * jd[2]);
        } else {
          const float mu = kStepLoad<S> ? muq : m->pair_friction[p];
          const float jt1 = f[3] * jd[0] + f[4] * jd[1] + f[5] * jd[2];
          const float jt2 = f[6] * jd[0] + f[7] * jd[1] + f[8] * jd[2];
          jstore(s, gx, off + 0, i, jn + mu * jt1);
          jstore(s, gx, off + 1, i, jn - mu * jt1);
          jstore(s, gx, off + 2, i, jn + mu * jt2);
          jstore(s, gx, off + 3, i, jn - mu * jt2);
        }
      }
      // (also orders the J rows past JL written to the HBM slab by other lanes,
      // and with rows_j the other wave's rows)
      if (rows_j) block_sync();
      else sync();
      ROWS_STAMP(25);
      // row parameters: vel, impedance, D, aref
      if constexpr (kStepRow<S>) {
        // single-arm kernels: the constraint source's record of the step
        // table holds what depends on solref / solimp / timestep alone -- the
        // clamped impedance bounds, 1 / width, 1 / mid, 1 / (1 - mid), the
        // reference's stiffness K and damping B, margin and the diagonal
        // (a pyramid's 1 + mu^2 folded in)
        for (int r = lane + rl0; r < nefc; r += rls) {
          const int src = s.efc_src[r], kind = src >> 24, id = (src >> 4) & 0xfffff, side = src & 15;
          const StepTable* st = step_table(m);
          float pos;
          int ri;
          float4 a0, a1, a2;
          if constexpr (kStepLoad<S>) {
            // the row record's four quads issued together ahead of the branch
            // on the kind (the record's index needs only the source and the
            // contact's pair); an equality adds its own record (StepEq) in
            // one level behind them
            ri = kind == 1 ? ST_ROW_EQ + id : (kind == 2 ? ST_ROW_JNT + id : ST_ROW_PAIR + s.con_pair[kind == 3 ? id : 0]);
            a0 = recq(st->row[ri], 0); a1 = recq(st->row[ri], 1); a2 = recq(st->row[ri], 2);
            const float4 j3 = recq(st->row[ri], 3);
            if (kind == 1) {
              const StepEq& eq = step_records(m)->eq[id & (ST_NEQ - 1)];
              const float4 e0 = recq(eq, 0), e1 = recq(eq, 1), e2 = recq(eq, 2);
              const float q1 = s.qpos[__float_as_int(e0.x)] - e1.x;
              if (__float_as_int(e0.z) >= 0) {
                const float dif = s.qpos[__float_as_int(e0.z)] - e1.y;
                pos = q1 - (e1.z + dif * (e1.w + dif * (e2.x + dif * (e2.y + dif * e2.z))));
              } else {
                pos = q1 - e1.z;
              }
            } else if (kind == 2) {
              const float q = s.qpos[__float_as_int(j3.z)];
              pos = side == 0 ? q - j3.x : j3.y - q;
            } else {
              pos = s.con_dist[id];
            }
          } else {
          if (kind == 1) {
            const int j1 = m->eq_j1[id], j2 = m->eq_j2[id];
            const float* c = m->eq_data[id];
            const float q1 = s.qpos[m->jnt_qposadr[j1]] - m->jnt_qpos0[j1];
            if (j2 >= 0) {
              const float dif = s.qpos[m->jnt_qposadr[j2]] - m->jnt_qpos0[j2];
              pos = q1 - (c[0] + dif * (c[1] + dif * (c[2] + dif * (c[3] + dif * c[4]))));
            } else {
              pos = q1 - c[0];
            }
            ri = ST_ROW_EQ + id;
          } else if (kind == 2) {
            ri = ST_ROW_JNT + id;
            const float4 j3 = recq(st->row[ri], 3);
            const float q = s.qpos[__float_as_int(j3.z)];
            pos = side == 0 ? q - j3.x : j3.y - q;
          } else {
            ri = ST_ROW_PAIR + s.con_pair[id];
            pos = s.con_dist[id];
          }
          a0 = recq(st->row[ri], 0); a1 = recq(st->row[ri], 1); a2 = recq(st->row[ri], 2);
          }
          const float vel = jdot(s, gx, r, s.qvel);
          const float dpos = pos - a2.x;
          const float x = fabsf(dpos * a0.z);
          float imp;
          if (x >= 1.f) {
            imp = a0.y;
          } else if (x <= 0.f) {
            imp = a0.x;
          } else {
            const int fl = __float_as_int(a2.z);
            const float mid = a0.w, power = a2.w;
            float y;
            if (fl & ST_POW1) y = x;
            else if (fl & ST_POW2) y = x <= mid ? x * x * a1.x : 1.f - (1.f - x) * (1.f - x) * a1.y;  // default solimp
            else if (x <= mid) y = powf(x, power) / powf(mid, power - 1.f);
            else y = 1.f - powf(1.f - x, power) / powf(1.f - mid, power - 1.f);
            imp = a0.x + y * (a0.y - a0.x);
          }
          const float R = fmaxf((1.f - imp) / imp * a2.y, kMinVal);
          s.efc_D[r] = 1.f / R;
          s.efc_aref[r] = -a1.w * vel - a1.z * imp * dpos;
          if (DBG_LAST() && r < DBG_MAXROW) {
            float* o = KA->dbg + DBG_ROW + 3 * r;
            o[0] = s.efc_D[r]; o[1] = s.efc_aref[r]; o[2] = vel;
          }
        }
      } else
      for (int r = lane + rl0; r < nefc; r += rls) {
        const int src = s.efc_src[r], kind = src >> 24, id = (src >> 4) & 0xfffff, side = src & 15;
        float pos, margin, diag;
        const float* sref;
        const float* simp;
        if (S::WIDE && kind == 1 && side > 0) {  // connect component
          pos = s.eqp[id][0][side - 1] - s.eqp[id][1][side - 1];
          margin = 0.f;
          diag = m->eq_diag[id];
          sref = m->eq_solref[id];
          simp = m->eq_solimp[id];
        } else if (kind == 1) {
          const int j1 = m->eq_j1[id], j2 = m->eq_j2[id];
          const float* c = m->eq_data[id];
          const float q1 = s.qpos[m->jnt_qposadr[j1]] - m->jnt_qpos0[j1];
          if (j2 >= 0) {
            const float dif = s.qpos[m->jnt_qposadr[j2]] - m->jnt_qpos0[j2];
            pos = q1 - (c[0] + dif * (c[1] + dif * (c[2] + dif * (c[3] + dif * c[4]))));
          } else {
            pos = q1 - c[0];
          }
          margin = 0.f;
          diag = m->eq_diag[id];
          sref = m->eq_solref[id];
          simp = m->eq_solimp[id];
        } else if (kind == 2) {
          const float q = s.qpos[m->jnt_qposadr[id]];
          pos = side == 0 ? q - m->jnt_range[id][0] : m->jnt_range[id][1] - q;
          margin = m->jnt_margin[id];
          diag = m->dof_invweight0[m->jnt_dofadr[id]];
          sref = m->jnt_solref[id];
          simp = m->jnt_solimp[id];
        } else if (S::WIDE && kind == 4) {
          const float dx = s.tenp[id][1][0] - s.tenp[id][0][0], dy = s.tenp[id][1][1] - s.tenp[id][0][1],
                      dz = s.tenp[id][1][2] - s.tenp[id][0][2];
          const float len = sqrtf(dx * dx + dy * dy + dz * dz);
          pos = side == 0 ? len - m->ten_range[id][0] : m->ten_range[id][1] - len;
          margin = m->ten_margin[id];
          diag = m->ten_invw[id];
          sref = m->ten_solref[id];
          simp = m->ten_solimp[id];
        } else if (S::WIDE && kind == 5) {  // elliptic: all rows take the normal's impedance
          const int c = (src >> 14) & 1023, p = ell_pair(src);
          pos = s.con_dist[c];
          margin = m->pair_margin[p];
          diag = m->pair_diag[p];
          sref = m->pair_solref[p];
          simp = m->pair_solimp[p];
        } else {
          const int p = s.con_pair[id];
          pos = s.con_dist[id];
          margin = m->pair_margin[p];
          const float mu = m->pair_friction[p];
          diag = m->pair_condim[p] == 1 ? m->pair_diag[p] : m->pair_diag[p] * (1.f + mu * mu);
          sref = m->pair_solref[p];
          simp = m->pair_solimp[p];
        }
        const float vel = jdot(s, gx, r, s.qvel);
        const float imp = impedance(simp, pos, margin);
        float R = fmaxf((1.f - imp) / imp * diag, kMinVal);
        // elliptic friction rows: R_t = R_n / impratio (equal sliding
        // frictions), no position term in aref
        const bool efric = S::WIDE && kind == 5 && side > 0;
        if (efric) R = R / m->impratio;
        float tc = sref[0];
        const float dr = sref[1];
        const float dmax = clampf(simp[1], kMinImp, kMaxImp);
        float K, B;
        if (tc > 0.f) {
          if (!(m->disableflags & 2)) tc = fmaxf(tc, 2.f * m->timestep);
          K = 1.f / (dmax * dmax * tc * tc * dr * dr);
          B = 2.f / (dmax * tc);
        } else {
          K = -tc / (dmax * dmax);
          B = -dr / dmax;
        }
        s.efc_D[r] = 1.f / R;
        s.efc_aref[r] = -B * vel - K * imp * (efric ? 0.f : pos - margin);
        if (DBG_LAST() && r < DBG_MAXROW) {
          float* o = KA->dbg + DBG_ROW + 3 * r;
          o[0] = s.efc_D[r]; o[1] = s.efc_aref[r]; o[2] = vel;
        }
      }
      if (DBG_LAST() && run_main) {
        if (lane == 0) { KA->dbg[DBG_NCON] = (float)s.ncon; KA->dbg[DBG_NEFC] = (float)s.nefc; }
        if (lane < s.ncon && lane < DBG_MAXCON) {
          float* o = KA->dbg + DBG_CON + 8 * lane;
          o[0] = s.con_pos[lane][0]; o[1] = s.con_pos[lane][1]; o[2] = s.con_pos[lane][2];
          o[3] = s.con_dist[lane]; o[4] = (float)s.con_pair[lane];
          o[5] = s.con_frame[lane][0]; o[6] = s.con_frame[lane][1]; o[7] = s.con_frame[lane][2];
        }
      }
      sync();
    }  // constraint rows
    if constexpr (WPC == 2) {
      if (rows_j) {
        block_sync();  // the rows are ready
        if (!run_main) {
          // wave 1: each Newton iteration's Hessian (two barriers per
          // iteration, the same count as wave 0's loop), then it waits for
          // the next step's geom poses
          STAMP(8);
          const int nefc = s.nefc;
          // the implicit factor: in the first iteration's wait (wave 0's
          // solve, line search and next active set), else after the loop
          bool fdone = !impl2;
          auto impl_factor = [&]() {
            const float dt = m->timestep;
            float fa[BLK_N], fdinv;
            blocked_factor<BLK_N>(m, [&](int i, int j) { return fmaf(dt, m->impl_D[i][j], m_get(i, j)); }, lane, fa,
                                  fdinv);
#pragma unroll
            for (int j = 0; j < BLK_N; j++) implf[j * WAVE + lane] = fa[j];
            implf[BLK_N * WAVE + lane] = fdinv;
            fdone = true;
          };
          if (hess2 && nefc > 0)
            for (int it = 0; it < m->iterations; it++) {
              block_sync();  // wave 0: efc_Da / efc_jar of this iteration
              STAMP(29);
              newton_hessian(nefc, &s.gxpos[0][0]);
              STAMP(31);
              block_sync();  // wave 0: gradient and stop test
              STAMP(30);
              if (s.pad_) break;
              if (!fdone) impl_factor();
            }
          if (!fdone) impl_factor();
          if (impl2) block_sync();  // the implicit factor, to wave 0's solve
          continue;
        }
      }
      if (rows_c) {
        if (run_coll && lane == 0) s.pad_ = coupled ? 1 : 0;
        block_sync();  // contacts and constraint rows ready; wave 1 waits for the next step's geom poses
        if (!run_main) continue;
        coupled = s.pad_ != 0;
      }
    }
    if (DBG_LAST() && lane < NVW) KA->dbg[DBG_QAS + lane] = s.qas[lane];
    nefc_sum += s.nefc;
    nefc_max = max(nefc_max, s.nefc);

    STAMP(8);
    STOP_AT(8)
    // ---- Newton solver (primal), MJX-style line search ------------------------
    {
      const int nefc = s.nefc;
      float qacc_l = lane < NVW ? s.qas[lane] : 0.f;  // this lane's dof value
      // Single-arm kernels: the warm-start choice below evaluates M a, the
      // Gauss term and the cost at both candidates, and Newton's first
      // iteration starts at the one it picks -- the same expressions on the
      // same data.  So the choice keeps M a_w and the chosen side's reduced
      // sums, and iteration 0 takes them instead of an m_dot and two wave sums
      // (-24 VALU per C3 candidate-step).  The first 64 rows' J a - aref come
      // from the choice too where LW_JAR holds (lane work, below; -23 more);
      // elsewhere they are recomputed.  DEV_NO_NEWTON_REUSE in the
      // device model's flags (MPCR_NEWTON_REUSE=0, tests) recomputes all.
      bool ws_keep = false, ws_won = false;
      float ws_maw = 0.f, ws_gw = 0.f, ws_cost = 0.f;
      // Lane work (MPCR_LANE_WORK, single-arm kernels; all wave-uniform):
      // lw, the device model's flags allow it; ws_jar, the first rows' J a - aref
      // at the warm-start candidate the choice picks, kept in two registers
      // through the choice (no LDS store in its loop; the one-wave kernels end
      // at 128 VGPRs) for Newton's first iteration, whose rows 64 and up are
      // recomputed.
      bool lw = false;
      float ws_jar = 0.f;
      if (nefc > 0) {
        // warm start: the better of qacc_warmstart and qacc_smooth
        const int dflags = m->disableflags;
        if constexpr (!S::WIDE) {
          lw = !(dflags & DEV_NO_LANE_WORK);
        }
        if (!(dflags & 4)) {
          if constexpr (!S::WIDE) ws_keep = !(dflags & DEV_NO_NEWTON_REUSE);
          // (the Gauss term of qacc_smooth itself is (M a_s - f_s)'(a_s - a_s) = 0)
          const float maw = lane < nv ? m_dot(lane, s.qws) : 0.f;
          const float gw = lane < nv ? (maw - s.qfs[lane]) * (s.qws[lane] - s.qas[lane]) : 0.f;
          float cw = 0.f, cs = 0.f;
          float jw0 = 0.f, js0 = 0.f;
          if constexpr (LW_JAR) {  // the same rows in the same order, the first trip's values kept
            auto ws_row = [&](int r, float& jw, float& js) {
              jw = jdot(s, gx, r, s.qws) - s.efc_aref[r];
              js = jdot(s, gx, r, s.qas) - s.efc_aref[r];
              const bool eq = (s.efc_src[r] >> 24) == 1;
              if (eq || jw < 0.f) cw += s.efc_D[r] * jw * jw;
              if (eq || js < 0.f) cs += s.efc_D[r] * js * js;
            };
            if (lane < nefc) ws_row(lane, jw0, js0);
            for (int r = lane + WAVE; r < nefc; r += WAVE) {
              float jw, js;
              ws_row(r, jw, js);
            }
          } else
          for (int r = lane; r < nefc; r += WAVE) {
            const float jw = jdot(s, gx, r, s.qws) - s.efc_aref[r];
            const float js = jdot(s, gx, r, s.qas) - s.efc_aref[r];
            const bool eq = (s.efc_src[r] >> 24) == 1;
            if constexpr (S::WIDE) {
              if (ell_row(s.efc_src[r])) {
                if (ell_head(s.efc_src[r])) {  // the cone cost of the whole contact
                  const int p = ell_pair(s.efc_src[r]);
                  const float D[3] = {s.efc_D[r], s.efc_D[r + 1], s.efc_D[r + 2]};
                  float xw[3] = {jw, 0.f, 0.f}, xs[3] = {js, 0.f, 0.f}, f[3], h[6];
#pragma unroll
                  for (int k = 1; k < 3; k++) {
                    xw[k] = jdot(s, gx, r + k, s.qws) - s.efc_aref[r + k];
                    xs[k] = jdot(s, gx, r + k, s.qas) - s.efc_aref[r + k];
                  }
                  cw += 2.f * cone_update(xw, m->pair_cmu[p], m->pair_friction[p], D, f, h);
                  cs += 2.f * cone_update(xs, m->pair_cmu[p], m->pair_friction[p], D, f, h);
                }
                continue;
              }
            }
            if (eq || jw < 0.f) cw += s.efc_D[r] * jw * jw;
            if (eq || js < 0.f) cs += s.efc_D[r] * js * js;
          }
          wsum2(cw, cs);
          const float gws = wsum_lo<NVW>(gw);
          const float costw = 0.5f * gws + 0.5f * cw;
          const float costs = 0.5f * cs;
          if (costw < costs && lane < NVW) qacc_l = s.qws[lane];
          if constexpr (LW_JAR) ws_jar = costw < costs ? jw0 : js0;
          if constexpr (!S::WIDE) {
            ws_won = costw < costs;
            ws_maw = maw;
            ws_gw = ws_won ? gws : 0.f;  // (the Gauss term at qacc_smooth is 0)
            ws_cost = ws_won ? costw : costs;
          }
          if (DBG_LAST() && lane == 0) {
            KA->dbg[DBG_INFO + 0] = costw < costs ? 1.f : 0.f;
            KA->dbg[DBG_INFO + 1] = costw;
            KA->dbg[DBG_INFO + 2] = costs;
          }
        }
        if (lane < NVW) s.qacc[lane] = qacc_l;
        sync();
        STAMP(13);
        STOP_AT(13)
        const float scale = 1.f / (m->meaninertia * (float)(nv > 1 ? nv : 1));
        float prev_cost = 3.4e38f;
        for (int it = 0;; it++) {
          // the iteration cap ends the solve before anything below matters
          // (cost / gradient only feed the stop test)
          if (it >= m->iterations) break;
#ifdef MPCR_PROFILE
          prof_acc[15] += 1;  // Newton iterations (low half of the counter, not cycles)
#endif
#ifdef MPCR_WAVETIME
          wt_newton++;
#endif
          // Ma, jar, cost at the current qacc; per-row force and active D
          const bool reuse = !S::WIDE && ws_keep;  // wave-uniform; the first iteration only (cleared below)
          float ma;
          if (reuse && ws_won) ma = ws_maw;
          else ma = lane < nv ? m_dot(lane, s.qacc) : 0.f;
          float cc = 0.f;
          if constexpr (LW_JAR) {
            auto it_row = [&](int r, float jar) {
              const bool act = ((s.efc_src[r] >> 24) == 1) || jar < 0.f;
              const float D = s.efc_D[r];
              s.efc_jar[r] = jar;
              s.efc_f[r] = act ? -D * jar : 0.f;
              s.efc_Da[r] = act ? D : 0.f;
              cc += act ? D * jar * jar : 0.f;
            };
            int r = lane;
            if (reuse && lw) {  // the first iteration: rows 0-63 from the warm-start choice
              if (r < nefc) it_row(r, ws_jar);
              r += WAVE;
            }
            for (; r < nefc; r += WAVE) it_row(r, jdot(s, gx, r, s.qacc) - s.efc_aref[r]);
          } else
          for (int r = lane; r < nefc; r += WAVE) {
            const float jar = jdot(s, gx, r, s.qacc) - s.efc_aref[r];
            bool act = ((s.efc_src[r] >> 24) == 1) || jar < 0.f;
            if constexpr (S::WIDE) act = act && !ell_row(s.efc_src[r]);  // cone pass below
            const float D = s.efc_D[r];
            s.efc_jar[r] = jar;
            s.efc_f[r] = act ? -D * jar : 0.f;
            s.efc_Da[r] = act ? D : 0.f;
            cc += act ? D * jar * jar : 0.f;
          }
          if constexpr (S::WIDE) {  // elliptic contacts: cone cost and forces
            if (m->cone == 1) {
              sync();
              for (int r = lane; r < nefc; r += WAVE) {
                const int src = s.efc_src[r];
                if (!ell_head(src)) continue;
                const int p = ell_pair(src);
                const float x[3] = {s.efc_jar[r], s.efc_jar[r + 1], s.efc_jar[r + 2]};
                const float D[3] = {s.efc_D[r], s.efc_D[r + 1], s.efc_D[r + 2]};
                float f[3], h[6];
                cc += 2.f * cone_update(x, m->pair_cmu[p], m->pair_friction[p], D, f, h);
                s.efc_f[r] = f[0]; s.efc_f[r + 1] = f[1]; s.efc_f[r + 2] = f[2];
              }
            }
          }
          float gauss, cost;
          if (reuse) {
            gauss = ws_gw;
            cost = ws_cost;
          } else {
            gauss = wsum_lo<NVW>(lane < nv ? (ma - s.qfs[lane]) * (s.qacc[lane] - s.qas[lane]) : 0.f);
            cost = 0.5f * gauss + 0.5f * wsum(cc);
          }
          sync();
          if (hess2) block_sync();  // this iteration's active set, to wave 1
          STAMP(29);
          constexpr bool MFMA_HESS = NVW == 16;  // else the 32-wide MFMA gradient, and newton_hessian
          const int gi = lane & (NVW - 1), gq = lane >> S::LOG_NVW;
          float* Hs = &s.gxpos[0][0];  // geom poses are dead during Newton
          float grad;
          if constexpr (MFMA_HESS) {
            // J^T f and H = M + J^T D_active J together on the matrix core,
            // 4 rows per v_mfma_f32_16x16x4_f32: lane (dof gi, row r0 + gq)
            // supplies A = J[r][gi] and B = D_a J[r][gi] (Hessian) / f[r]
            // (gradient); accumulator register v of lane l is column gi of
            // row 4 gq + v -- read as row gi of H that is the float4
            // H[gi][4 gq ..], the same products in the same row order as the
            // VALU build (the MFMA is a k-ordered fmaf chain), so H is
            // bitwise the VALU one
            const float4 m4 = m_quad(gi, gq);
            mfx4 hacc = {m4.x, m4.y, m4.z, m4.w};
            mfx4 gacc = {0.f, 0.f, 0.f, 0.f};
            for (int r0 = 0; r0 < nefc; r0 += 4) {
              const int r = r0 + gq;
              const bool ok = r < nefc;
              const float a = ok ? jrow_ptr(s, gx, r)[gi] : 0.f;
              const float da = ok ? s.efc_Da[r] : 0.f;
              const float fr = ok ? s.efc_f[r] : 0.f;
              hacc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, da * a, hacc, 0, 0, 0);
              gacc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, fr, gacc, 0, 0, 0);
            }
            reinterpret_cast<float4*>(Hs + gi * S::LD)[gq] = make_float4(hacc[0], hacc[1], hacc[2], hacc[3]);
            float* qcs = Hs + NVW * S::LD;  // J^T f: lanes 0, 16, 32, 48 hold dofs 4 gq ..
            if (gi == 0) reinterpret_cast<float4*>(qcs)[gq] = make_float4(gacc[0], gacc[1], gacc[2], gacc[3]);
            sync();
            grad = lane < nv ? ma - s.qfs[lane] - qcs[gi] : 0.f;
          } else {
            // 32-wide: J^T f on v_mfma_f32_32x32x2_f32, 2 rows per instruction
            // (lane: A = J[r0 + gq][gi], B = f[r0 + gq]); accumulator register
            // v of lane l holds (J^T f)[(v & 3) + 8 (v >> 2) + 4 gq]
            mfx16 gacc;
#pragma unroll
            for (int v = 0; v < 16; v++) gacc[v] = 0.f;
            gacc = mfma_rows32(s, gx, nefc, gi, gq, [&](int r, float) { return s.efc_f[r]; }, gacc);
            float* qcs = s.srch;  // free until this iteration's search direction
            if (gi == 0) {
#pragma unroll
              for (int k = 0; k < 4; k++)
                reinterpret_cast<float4*>(qcs + 8 * k + 4 * gq)[0] =
                    make_float4(gacc[4 * k], gacc[4 * k + 1], gacc[4 * k + 2], gacc[4 * k + 3]);
            }
            sync();
            grad = lane < nv ? ma - s.qfs[lane] - qcs[gi] : 0.f;
            sync();  // qcs (srch) is rewritten below
          }
          STAMP(30);
          const float gn = sqrtf(wsum_lo<NVW>(grad * grad));
          // MuJoCo's stop test, plus its fp32 floor: an improvement within ~8 ulp
          // of the cost is rounding noise (without it fp32 iterates on noise
          // where the fp64 solve has converged: 3.9 vs 1.9 iterations per
          // dual-arm step)
          const bool stop = scale * (prev_cost - cost) < m->tolerance || scale * gn < m->tolerance ||
                            prev_cost - cost <= 1e-6f * fabsf(cost);
          if (hess2) {  // hand the decision to wave 1, take its Hessian
            if (lane == 0) s.pad_ = stop ? 1 : 0;
            block_sync();
          }
          if (stop) break;
          if constexpr (!MFMA_HESS) {
            if (!hess2) newton_hessian(nefc, Hs);  // (two waves: wave 1 built it meanwhile)
          }
          STAMP(31);
          float mg;
          if (!coupled && blk_usable<NVW>(m)) {
            // no row couples two trees: H is block diagonal like M
            if (lane < NVW) s.srch[lane] = lane < nv ? grad : 0.f;
            sync();
            blk_solve<NVW>(m, [&](int i, int j) { return Hs[i * S::LD + j]; }, s.srch, s.srch, lane, &s.gxpos[0][0]);
            sync();
            mg = lane < nv ? s.srch[lane] : 0.f;
            sync();  // srch is rewritten below
          } else {
            float h[NVW];
            {
              const float4* row = reinterpret_cast<const float4*>(Hs + (lane & (NVW - 1)) * S::LD);
#pragma unroll
              for (int q = 0; q < NVW / 4; q++) {
                const float4 v = row[q];
                h[4 * q] = v.x; h[4 * q + 1] = v.y; h[4 * q + 2] = v.z; h[4 * q + 3] = v.w;
              }
            }
            if constexpr (NVW == 16) {
              float dinv;
              chol16(h, dinv, lane);
              mg = chol16_solve<S::LD>(h, dinv, lane < nv ? grad : 0.f, lane, &s.gxpos[0][0]);
            } else {
              chol_rows(h, lane);
              mg = chol_solve<NVW, S::LD>(h, lane < nv ? grad : 0.f, lane, &s.gxpos[0][0]);
            }
          }
          const float search = lane < nv ? -mg : 0.f;
          if (DBG_LAST() && it == 0 && lane < NVW) {
            KA->dbg[DBG_GRAD + lane] = grad;
            KA->dbg[DBG_SRCH + lane] = search;
          }
          STAMP(14);
          if (lane < NVW) s.srch[lane] = search;
          sync();
          // Mv, jv, quadratic coefficients
          const float mvv = lane < nv ? m_dot(lane, s.srch) : 0.f;
          for (int r = lane; r < nefc; r += WAVE) s.efc_jv[r] = jdot(s, gx, r, s.srch);
          const float sn = sqrtf(wsum_lo<NVW>(search * search));
          const float gtol = m->tolerance * m->ls_tolerance * sn * m->meaninertia * (float)(nv > 1 ? nv : 1);
          float qg[3];
          qg[0] = 0.5f * gauss;
          qg[1] = wsum_lo<NVW>(lane < nv ? search * (ma - s.qfs[lane]) : 0.f);
          qg[2] = 0.5f * wsum_lo<NVW>(search * mvv);
          sync();
          using LT = LsReal<S>;
          using LsPt = LsPtT<LT>;
          // alpha = 0: the rows' active set is the iteration's (jar < 0) and
          // 0.5 sum D jar^2 + 0.5 gauss is the cost above: halving is exact unless
          // a row term D jar^2 is subnormal (fp32 denormals are on), where the
          // two may round apart in the last subnormal bit -- not met in any batch
          // run, and the on / off tests compare bit for bit.  So with lane work
          // p0 takes it and sums q1, q2 alone
          LsPt p0;
          if (LW_Q0 && lw) {
            p0 = ls_eval<S, false>(s, lane, qg, (LT)0);
            p0.cost = cost;
            p0.full = true;
          } else {
            p0 = ls_eval(s, lane, qg, (LT)0);
          }
          const bool ell_ls = S::WIDE && m->cone == 1;
          if (ell_ls) {
            const LT al[3] = {0, 0, 0};
            float e[9];
            ls_cones3(s, m, lane, al, e);
            ls_add(p0, e[0], e[1], e[2]);
          }
          constexpr bool LSQ0 = S::WIDE;  // narrow: q0 deferred to ls_finish
          LsPt lo = ls_eval<S, LSQ0>(s, lane, qg, p0.alpha - p0.d0 / p0.d1);
          if (ell_ls) {
            const LT al[3] = {lo.alpha, 0, 0};
            float e[9];
            ls_cones3(s, m, lane, al, e);
            ls_add(lo, e[0], e[1], e[2]);
          }
          LsPt hi;
          if (lo.d0 < p0.d0) { hi = p0; } else { hi = lo; lo = p0; }
          bool swap = true;
          for (int ls = 0; ls < m->ls_iterations; ls++) {
            if (!swap) break;
#ifdef MPCR_PROFILE
            prof_acc[15] += 1ull << 32;  // line-search passes (high half of the counter)
#endif
#ifdef MPCR_WAVETIME
            wt_ls++;
#endif
            if (DBG_LAST() && lane == 0 && it == 0) KA->dbg[DBG_INFO + 5] = (float)ls;
            if (lo.d0 < 0.f && lo.d0 > -gtol) break;
            if (hi.d0 > 0.f && hi.d0 < gtol) break;
            // bracket closed to fp32 resolution: further passes only move alpha
            // by rounding noise (gtol sits below fp32 resolution; without this the
            // dual arm ran ~20 passes per Newton iteration against ~2.4 in fp64)
            {
              const LT da = hi.alpha - lo.alpha, la = lo.alpha < 0 ? -lo.alpha : lo.alpha,
                       ha = hi.alpha < 0 ? -hi.alpha : hi.alpha;
              if ((da < 0 ? -da : da) <= (LT)1e-6f * (la > ha ? la : ha)) break;
            }
            LsPt lo_next, hi_next, mid;
            ls_eval3<S, LSQ0>(s, lane, qg, lo.alpha - lo.d0 / lo.d1, hi.alpha - hi.d0 / hi.d1,
                              (LT)0.5 * (lo.alpha + hi.alpha), lo_next, hi_next, mid);
            if (ell_ls) {
              const LT al[3] = {lo_next.alpha, hi_next.alpha, mid.alpha};
              float e[9];
              ls_cones3(s, m, lane, al, e);
              ls_add(lo_next, e[0], e[1], e[2]);
              ls_add(hi_next, e[3], e[4], e[5]);
              ls_add(mid, e[6], e[7], e[8]);
            }
            const bool s1 = lo.d0 > 0.f || lo.d0 < lo_next.d0;
            if (s1) lo = lo_next;
            const bool s2 = mid.d0 < 0.f && lo.d0 < mid.d0;
            if (s2) lo = mid;
            const bool s3 = hi.d0 < 0.f || hi.d0 > hi_next.d0;
            if (s3) hi = hi_next;
            const bool s4 = mid.d0 > 0.f && hi.d0 > mid.d0;
            if (s4) hi = mid;
            swap = s1 || s2 || s3 || s4;
          }
          if constexpr (!LSQ0) ls_finish(s, lane, qg, lo, hi);
          const bool improved = lo.cost < p0.cost || hi.cost < p0.cost;
          const LT alpha = lo.cost < hi.cost ? lo.alpha : hi.alpha;
          if (DBG_LAST() && lane == 0 && it == 0) {
            KA->dbg[DBG_INFO + 3] = (float)p0.cost;
            KA->dbg[DBG_INFO + 4] = (float)alpha;
            KA->dbg[DBG_INFO + 6] = (float)(lo.cost < hi.cost ? lo.cost : hi.cost);
          }
          if (DBG_LAST() && lane == 0) KA->dbg[DBG_INFO + 7] = (float)(it + 1);
          if (improved && lane < NVW) s.qacc[lane] = (float)((LT)s.qacc[lane] + alpha * (LT)s.srch[lane]);
          prev_cost = cost;
          ws_keep = false;
          sync();
          STAMP(9);
        }
      } else {
        if (lane < NVW) s.qacc[lane] = qacc_l;
        sync();
      }
    }

    if (DBG_LAST() && lane < NVW) KA->dbg[DBG_QACC + lane] = s.qacc[lane];
    STAMP(9);
    STOP_AT(9)
    // ---- implicitfast (dual-arm class): (M + dt D) a = qfrc_smooth + J^T f at
    //      the final qacc; the velocity update uses a, the warm start qacc --
    bool implicit = false;
    if constexpr (S::WIDE) {
      if (m->integrator == 3) {
        implicit = true;
        const int nefc = s.nefc;
        for (int r = lane; r < nefc; r += WAVE) {
          const float jar = jdot(s, gx, r, s.qacc) - s.efc_aref[r];
          const bool act = ((s.efc_src[r] >> 24) == 1) || jar < 0.f;
          s.efc_f[r] = act ? -s.efc_D[r] * jar : 0.f;
          s.efc_jar[r] = jar;
        }
        sync();
        if (m->cone == 1) {  // elliptic contacts: cone forces at the final qacc
          for (int r = lane; r < nefc; r += WAVE) {
            const int src = s.efc_src[r];
            if (!ell_head(src)) continue;
            const int p = ell_pair(src);
            const float x[3] = {s.efc_jar[r], s.efc_jar[r + 1], s.efc_jar[r + 2]};
            const float D[3] = {s.efc_D[r], s.efc_D[r + 1], s.efc_D[r + 2]};
            float f[3], h[6];
            cone_update(x, m->pair_cmu[p], m->pair_friction[p], D, f, h);
            s.efc_f[r] = f[0]; s.efc_f[r + 1] = f[1]; s.efc_f[r + 2] = f[2];
          }
          sync();
        }
        constexpr int RPW = WAVE / NVW;
        const int gi = lane & (NVW - 1), gq = lane >> S::LOG_NVW;
        float qc = 0.f;
        jrows(s, gx, gq, RPW, nefc, [&](const float* J, int r) { qc = fmaf(J[gi], s.efc_f[r], qc); });
#pragma unroll
        for (int o = NVW; o < WAVE; o <<= 1) qc += __shfl_xor(qc, o);
        const float dt = m->timestep;
        if (!m->impl_cross && blk_usable<NVW>(m)) {  // M + dt D block diagonal by tree
          if (lane < NVW) s.srch[lane] = lane < nv ? s.qfs[lane] + qc : 0.f;
          sync();
          if (impl2) {  // wave 1's factor
            block_sync();
            float fa[BLK_N];
#pragma unroll
            for (int j = 0; j < BLK_N; j++) fa[j] = implf[j * WAVE + lane];
            blocked_sweep<BLK_N>(m, fa, implf[BLK_N * WAVE + lane], s.srch, s.srch, lane, &s.gxpos[0][0]);
          } else {
            blk_solve<NVW>(m, [&](int i, int j) { return fmaf(dt, m->impl_D[i][j], m_get(i, j)); }, s.srch, s.srch,
                           lane, &s.gxpos[0][0]);
          }
          sync();
        } else {
          float Lm[NVW];
#pragma unroll
          for (int j = 0; j < NVW; j++) Lm[j] = lane < NVW ? fmaf(dt, m->impl_D[lane][j], m_get(lane, j)) : 0.f;
          chol_rows(Lm, lane);
          const float a = chol_solve<NVW, S::LD>(Lm, lane < nv ? s.qfs[lane] + qc : 0.f, lane, &s.gxpos[0][0]);
          if (lane < NVW) s.srch[lane] = lane < nv ? a : 0.f;
          sync();
        }
      }
    }
    // ---- Euler: qvel += dt qacc; integrate qpos; warm start -----------------
    {
      const float dt = m->timestep;
      if (lane < nv) {
        s.qvel[lane] = s.qvel[lane] + dt * (implicit ? s.srch[lane] : s.qacc[lane]);
        s.qws[lane] = s.qacc[lane];
      }
      sync();
      if (lane < m->njnt) {
        const int a = m->jnt_qposadr[lane], v = m->jnt_dofadr[lane], type = m->jnt_type[lane];
        if (type == 0) {
          s.qpos[a] += dt * s.qvel[v];
          s.qpos[a + 1] += dt * s.qvel[v + 1];
          s.qpos[a + 2] += dt * s.qvel[v + 2];
          float w[3] = {s.qvel[v + 3], s.qvel[v + 4], s.qvel[v + 5]};
          float q[4] = {s.qpos[a + 3], s.qpos[a + 4], s.qpos[a + 5], s.qpos[a + 6]};
          const float wn = sqrtf(dot3(w, w));
          const float ang = wn * dt;
          if (ang > kMinVal) {
            float sn, cs;
            __sincosf(0.5f * ang, &sn, &cs);
            float dq[4] = {cs, w[0] / wn * sn, w[1] / wn * sn, w[2] / wn * sn};
            qmul(q, q, dq);
          }
          float n = sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
          s.qpos[a + 3] = q[0] / n; s.qpos[a + 4] = q[1] / n; s.qpos[a + 5] = q[2] / n; s.qpos[a + 6] = q[3] / n;
        } else if (type == 2 || type == 3) {
          s.qpos[a] += dt * s.qvel[v];
        }
      }
      sync();
      if (lane < nc && ARGS_HAS(AF_THETA, KA->theta) && (!SCEN || orow >= 0))
        KA->theta[(size_t)(SCEN ? orow : b) * nc * H + lane * H + t] = s.qpos[ctrl_qa];
    }
  }

  STAMP(10);
  PROF_FLUSH
  // the state after the last step, with that step's qacc: the single
  // environment's block (plant; advanced only when plant & 2) or candidate b's
  // block of a batch's final states (STATE; written by the segment that ends at H)
  const bool wr_state = STATE ? KSA->final_state != nullptr && !suspend : KA->plant != 0;
  float* const sout = STATE ? KSA->final_state + (size_t)b * ST_N : KA->state;
  if (wr_state && run_main) {
    if (lane < nv) sout[ST_QACC + lane] = s.qacc[lane];
    if (STATE || (KA->plant & 2)) {
      if (lane < m->nq) sout[ST_QPOS + lane] = s.qpos[lane];
      if (lane < nv) {
        sout[ST_QVEL + lane] = s.qvel[lane];
        sout[ST_QWS + lane] = s.qws[lane];
      }
    }
  }
  if (suspend) {  // not the last segment: save the state and the accumulators, no outputs
    for (int i = lane; i < DX_NQ; i += WAVE) segs[SEG_QPOS + i] = i < S::NQW ? s.qpos[i] : 0.f;
    if (lane < NVW) {
      segs[SEG_QVEL + lane] = s.qvel[lane];
      segs[SEG_QWS + lane] = s.qws[lane];
    }
    segs[SEG_COSTC + lane] = cost_c;
    if (lane == 0) {
      float* sc = segs + SEG_SCAL;
      sc[0] = cost_g; sc[1] = cost_r;
      sc[2] = __int_as_float(status); sc[3] = __int_as_float(nefc_sum); sc[4] = __int_as_float(nefc_max);
    }
    if (pace && lane == pace_own) __hip_atomic_store(pace + lane, ~0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    return;
  }
  // ---- final reductions, outputs ----------------------------------------------
  cost_c = wsum(cost_c);
  if constexpr (WPC == 2) {  // the collision wave's cost_c and truncation flag
    block_sync();  // wave 0's last step is done with the image (srch)
    if (wv == 1 && lane == 0) { s.srch[0] = cost_c; s.pad_ = status; }
    block_sync();
    if (wv == 1) return;
    cost_c = s.srch[0];
    status |= s.pad_;
  }
  bool finite = true;
  if (lane < m->nq) finite = isfinite(s.qpos[lane]);
  finite = __ballot(!finite) == 0;
  if (!finite) status |= 2;
  if (lane == 0) {
    // a lost two-wave handshake (MPCR_STATUS_SYNC) voids the rollout: +inf
    // keeps it out of the argmin and the elites (a NaN would win the argmin)
    const float cost = (status & (1 << 10)) ? __builtin_inff()
                                            : s.par[PAR_W] * cost_g + s.par[PAR_W + 1] * cost_r + s.par[PAR_W + 2] * cost_c;
    KA->cost4[4 * (size_t)b + 0] = cost;
    KA->cost4[4 * (size_t)b + 1] = cost_g;
    KA->cost4[4 * (size_t)b + 2] = cost_r;
    KA->cost4[4 * (size_t)b + 3] = cost_c;
    if (KA->status) KA->status[b] = status | (min(nefc_max, 255) << 2) | (nefc_sum << 11);
    if (KA->best_key) {
      const uint32_t u = __float_as_uint(cost);
      uint32_t key = isnan(cost) ? 0u : ((u & 0x80000000u) ? ~u : (u | 0x80000000u));
      if constexpr (MULTI) {  // problem pr's key, the index within the problem
        const int gi = KA->prob_off + b, pr = PROBLEM_OF(gi);
        const int li = KA->prob_n ? gi - pr * KA->prob_n : gi;
        const unsigned long long k64 = ((unsigned long long)key << 32) | (uint32_t)(KA->index_base + li);
        atomicMin(KA->best_key + pr, k64);
      } else {
        const unsigned long long k64 = ((unsigned long long)key << 32) | (uint32_t)(KA->index_base + b);
        atomicMin(KA->best_key, k64);
      }
    }
  }
  if (pace && lane == pace_own) __hip_atomic_store(pace + lane, ~0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#ifdef MPCR_WAVETIME
  if (lane == 0 && KA->prof) {
    const unsigned long long c1 = __builtin_amdgcn_s_memtime(), t1 = __builtin_amdgcn_s_memrealtime();
    const unsigned hwid = __builtin_amdgcn_s_getreg((31 << 11) | 4), xcc = __builtin_amdgcn_s_getreg((31 << 11) | 20);
    KA->prof[4 * (size_t)b + 0] = wt_t0;
    KA->prof[4 * (size_t)b + 1] = t1;
    KA->prof[4 * (size_t)b + 2] = c1 - wt_c0;
    KA->prof[4 * (size_t)b + 3] = ((unsigned long long)xcc << 32) | hwid;
    KA->prof[4 * (size_t)KA->n + 2 * (size_t)b] = ((unsigned long long)wt_ls << 32) | wt_newton;
    KA->prof[4 * (size_t)KA->n + 2 * (size_t)b + 1] = wt_cvx;
  }
#endif
}

}  // namespace mpcr
