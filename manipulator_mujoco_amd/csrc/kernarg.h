// kernarg.h -- how the rollout kernels read their launch arguments (KA, KSA, KSCEN,
// KTA, KSW, KSTW, ARGS_HAS, DBG_LAST).
#pragma once
#include "rollout.h"

namespace mpcr {

// How a kernel reads its RolloutArgs (KA->field).  The dual-arm kernels read
// the by-value argument itself, as ever.  The single-arm kernels read each
// field where it is used, from the kernarg segment (RolloutArgs is the first
// kernel argument: offset 0), through a pointer laundered at every read: a
// by-value field is loaded in the prologue and, when it is needed once a step
// or only in the epilogue, held in scalar registers across the whole horizon
// loop -- with the masks and model scalars the loop needs that was more than
// the 106 SGPRs, and the register allocator kept the surplus in VGPR lanes
// (v_writelane / v_readlane: VALU instructions, and a VALU -> SALU wait in
// front of every use).  The segment stays in the constant address space, so
// the reads are s_load from the scalar cache.
static_assert(offsetof(RolloutArgs, blk) % 8 == 0, "the blocks' pointers aligned inside the kernarg segment");
// (kernarg_at<T>(offset): the T at that byte of the kernarg segment)
template <class T>
__device__ __forceinline__ const __attribute__((address_space(4))) T* kernarg_at(size_t offset) {
  const __attribute__((address_space(4))) char* p =
      (const __attribute__((address_space(4))) char*)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(p));
  return (const __attribute__((address_space(4))) T*)(p + offset);
}
// Which optional outputs a call asked for (ARGS_HAS): the single-arm kernels
// keep the answers as bits of one scalar (aflags), taken from the by-value
// argument in the prologue, and read a pointer only behind its bit.
enum { AF_TRACE_SLOTS = 1, AF_TRACE_EEF = 2, AF_THETA = 4, AF_TDOUT = 8 };  // AF_TDOUT: thetadot, theta-dot input layout
// KA->field: the by-value argument (dual-arm kernels) or the laundered kernarg
// segment (single-arm kernels); `args` is the kernel's by-value parameter or,
// in a device function, a reference to it
// The choice is the translation unit's (rollout_wide.hip defines
// MPCR_ARGS_BY_VALUE before it includes this file; each unit instantiates
// its own class only): with it the macros below are the text the kernels
// had, and the dual-arm unit compiles to the code it had.
#ifdef MPCR_ARGS_BY_VALUE
#define KA (&args)
#define KSA (&sa)
#define KSCEN (args.blk.nscen)
#define ARGS_HAS(f, expr) (expr)
#define ARGS_LAST_STEP_FIRST(t, H) true
#else
#define KA kernarg_at<RolloutArgs>(0)
__device__ __forceinline__ unsigned args_flags(const RolloutArgs& a) {
  return (a.trace_slots ? AF_TRACE_SLOTS : 0) | (a.trace_eef ? AF_TRACE_EEF : 0) | (a.theta ? AF_THETA : 0) |
         (a.layout != 0 && a.thetadot ? AF_TDOUT : 0);
}
// ARGS_HAS(bit, the by-value units' own test): laundering the word at the
// test, so that a bit's test is not hoisted out of the horizon loop as a lane
// mask, does not compile (inside a divergent region the word may sit in a
// vector register)
#define ARGS_HAS(f, expr) ((aflags & (f)) != 0)
// a test of an argument on the last step only: the step first, the read behind it
#define ARGS_LAST_STEP_FIRST(t, H) ((t) == (H) - 1)
// the call's blocks the same way (KSA->field, KSCEN; the STATE kernels read them in the
// kernarg segment, where they live in RolloutArgs::blk)
#define KSA kernarg_at<StateArgs>(offsetof(RolloutArgs, blk) + offsetof(CallBlocks, st))
#define KSCEN (*kernarg_at<int>(offsetof(RolloutArgs, blk) + offsetof(CallBlocks, nscen)))
#endif
// The target schedule (KTA->field): both units read it where they use it, once a
// step, from the kernarg segment through a laundered pointer -- the dual-arm
// kernels too, whose by-value copy of it held four more scalars across the
// horizon loop (a fifth spilled VGPR and 32 bytes of scratch in the one-wave
// kernel)
#define KTA kernarg_at<TargetArgs>(offsetof(RolloutArgs, blk) + offsetof(CallBlocks, tg))
// The slot weights (KSW->field) likewise, in both units: read at the use, in
// emit_contacts, so nothing of them lives across the step loop
#define KSW kernarg_at<SlotWArgs>(offsetof(RolloutArgs, sw))
// The step weights (KSTW->field) likewise -- the kernels' third argument, at
// STW_KERNARG of the segment: read at the two uses, the pose cost and the head
// of the collision phase, once a step each
#define KSTW kernarg_at<StepWArgs>(STW_KERNARG)
// the schedule row (a_pos a_rot a_col 0) of absolute step t for candidate b's
// problem, null without a schedule: the pointer, the stride and the problem
// fields from the segment at the use (as emit_contacts reads the slot weights),
// so no register holds anything of the schedule across the step loop and a
// resumed horizon segment finds the same row
__device__ __forceinline__ const float* step_w_row(int b, int t) {
  const float* sp = KSTW->step_w;
  if (!sp) return nullptr;
  const int pn = *kernarg_at<int>(offsetof(RolloutArgs, prob_n));
  const int po = *kernarg_at<int>(offsetof(RolloutArgs, prob_off));
  return sp + (size_t)(pn ? (po + b) / pn : 0) * (unsigned)KSTW->stride + 4 * (size_t)t;
}

// The debug dump's test (candidate 0's last step, RolloutArgs::dbg given).  The
// single-arm kernels test the step and the candidate first, values the loop
// holds anyway, and read the pointer only behind them: no register and no
// load for the dump in any other step.
#ifdef MPCR_ARGS_BY_VALUE
#define DBG_LAST() (KA->dbg && b == 0 && t == H - 1)
#else
#define DBG_LAST() (t == H - 1 && b == 0 && KA->dbg)
#endif

}  // namespace mpcr
