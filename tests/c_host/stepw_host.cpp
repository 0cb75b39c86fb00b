// A stand-alone host of what csrc/rollout.h holds for the step weights as a
// call input (no libmpcr, nothing launched, no GPU opened): the schedule's
// arguments are the kernels' third argument, behind RolloutArgs and the model
// pointer, so RolloutArgs keeps the layout tests/c_host/slotw_host.cpp pins.
// It checks
//   - sizeof(StepWArgs) == 16 with the pointer at 0 and the stride at 8;
//   - RolloutArgs as it was: the union at byte 216, the slot weights at 296,
//     prob_n / prob_off at 312 / 316, 320 bytes in all; the step weights at
//     byte 328 of the kernarg segment (STW_KERNARG), 8-byte aligned;
//   - an argument image laid out as the launch lays it out (RolloutArgs, the
//     model pointer, StepWArgs) round-trips the schedule at 328 / 336 and
//     leaves the other two arguments' bytes alone;
//   - has_state() / scenarios() for every combination of a state block, a
//     scenario count, a slot-weight block and a schedule, with and without
//     dpar: a call with only step_w set picks a STATE kernel;
//   - the stride rule (step_w_stride_ok): 0 or a multiple of 4 floats that is
//     at least 4 H
// and prints "OK stepw_host", or "FAIL why" with exit status 1.  Built with
// the address and undefined-behaviour sanitizers and run by
// tests/test_stepw_lib.py.
#include <limits.h>
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include "../../manipulator_mujoco_amd/csrc/rollout.h"

using namespace mpcr;

static_assert(sizeof(StepWArgs) == 16 && offsetof(StepWArgs, step_w) == 0 && offsetof(StepWArgs, stride) == 8,
              "StepWArgs: the pointer at 0, the stride at 8");
static_assert(offsetof(RolloutArgs, par) == 216 && offsetof(RolloutArgs, blk) == 216 &&
                  offsetof(RolloutArgs, sw) == 296 && sizeof(CallBlocks) == 80 && sizeof(SlotWArgs) == 16,
              "everything up to the slot weights where it was");
static_assert(offsetof(RolloutArgs, prob_n) == 312 && offsetof(RolloutArgs, prob_off) == 316 &&
                  sizeof(RolloutArgs) == 320,
              "RolloutArgs keeps its layout: the step weights are not a member");
static_assert(STW_KERNARG == 328 && STW_KERNARG == sizeof(RolloutArgs) + sizeof(void*) && STW_KERNARG % 8 == 0,
              "the step weights behind the model pointer in the kernarg segment");

// the explicit arguments of a rollout kernel, in order: what the segment holds
struct KernelArgs {
  RolloutArgs a;
  const DevModel* m;
  StepWArgs stw;
};
static_assert(offsetof(KernelArgs, m) == 320 && offsetof(KernelArgs, stw) == STW_KERNARG && sizeof(KernelArgs) == 344,
              "RolloutArgs | model pointer | StepWArgs");

static int fail(const char* why) {
  printf("FAIL %s\n", why);
  return 1;
}

int main() {
  static const float dummy[64] = {};
  const TargetArgs tg = {dummy + 16, 96, 8};
  const SlotWArgs sw = {dummy + 20, 188, 0};
  const StepWArgs stw = {dummy + 24, 48, 0};
  // round trips at the raw offsets of the argument image
  {
    KernelArgs k;
    memset(&k, 0, sizeof(k));
    const char* raw = reinterpret_cast<const char*>(&k);
    k.stw = stw;
    const float* p = nullptr;
    int st = 0;
    memcpy(&p, raw + 328, sizeof(p));
    memcpy(&st, raw + 336, sizeof(st));
    if (p != stw.step_w || st != 48) return fail("step-weight arguments at offsets 328, 336 of the segment");
    for (size_t i = 0; i < sizeof(k); i++)
      if (raw[i] != 0 && !(i >= 328 && i < 344)) return fail("the step weights wrote outside their bytes");
    k.a.dpar = dummy;
    k.a.blk.nscen = 5;
    k.a.blk.tg = tg;
    k.a.sw = sw;
    k.a.prob_n = 7;
    k.a.prob_off = 9;
    int n = 0, pn[2] = {0, 0};
    memcpy(&n, raw + 216 + 56, sizeof(n));
    memcpy(pn, raw + 312, sizeof(pn));
    if (n != 5 || pn[0] != 7 || pn[1] != 9) return fail("scenario count at 216 + 56, prob_n / prob_off at 312 / 316");
    memcpy(&p, raw + 296, sizeof(p));
    if (p != sw.slot_w) return fail("slot-weight pointer at 296");
    for (int i = 0; i < PAR_N; i++) k.a.par[i] = 1.5f + i;  // (a host-parameter call's values)
    if (k.stw.step_w != stw.step_w || k.stw.stride != 48 || k.m != nullptr)
      return fail("RolloutArgs disturbed the arguments behind it");
  }
  // has_state() / scenarios() for each combination
  for (int with_dpar = 0; with_dpar < 2; with_dpar++)
    for (int with_state = 0; with_state < 2; with_state++)
      for (int nscen = 0; nscen < 4; nscen++)
        for (int with_sw = 0; with_sw < 2; with_sw++)
          for (int with_stw = 0; with_stw < 2; with_stw++) {
            RolloutArgs a;
            memset(&a, 0, sizeof(a));
            a.dpar = with_dpar ? dummy : nullptr;
            if (with_state) a.blk.st.start = dummy;
            a.blk.nscen = nscen;
            a.sw = with_sw ? sw : SlotWArgs{nullptr, 0, 0};
            const StepWArgs w = with_stw ? stw : StepWArgs{nullptr, 0, 0};
            const bool want_state = with_dpar && (with_state || nscen > 1 || with_sw || with_stw);
            const int want_scen = with_dpar && nscen > 1 ? nscen : 0;
            if (has_state(a, w) != want_state || scenarios(a) != want_scen ||
                has_state(a) != (with_dpar && (with_state || nscen > 1 || with_sw))) {
              printf("FAIL has_state / scenarios: dpar %d state %d nscen %d slot_w %d step_w %d -> %d, %d\n", with_dpar,
                     with_state, nscen, with_sw, with_stw, (int)has_state(a, w), scenarios(a));
              return 1;
            }
          }
  // the stride rule, H = 12: rows of 48 floats
  {
    const int H = 12;
    const int good[] = {0, 48, 52, 96, 4096, INT_MAX - 3};
    const int bad[] = {4, 44, 47, 49, 50, 46, -48, -4, 2, INT_MIN, INT_MAX};
    for (int v : good)
      if (!step_w_stride_ok(v, H)) {
        printf("FAIL stride %d refused for H = %d\n", v, H);
        return 1;
      }
    for (int v : bad)
      if (step_w_stride_ok(v, H)) {
        printf("FAIL stride %d accepted for H = %d\n", v, H);
        return 1;
      }
    if (!step_w_stride_ok(4, 1) || step_w_stride_ok(4, 2)) return fail("the bound is 4 H");
  }
  printf("OK stepw_host\n");
  return 0;
}
