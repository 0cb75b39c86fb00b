// A stand-alone host of what csrc/rollout.h holds for the slot weights as a
// call input (no libmpcr, nothing launched, no GPU opened): where the block's
// arguments sit in RolloutArgs, beside the bytes a call with a device
// parameter block carries its other blocks in (CallBlocks, RolloutArgs::blk).
// It checks
//   - sizeof(StateArgs) == 56 with the field offsets it had, the scenario
//     count at byte 56 of the union, the target arguments at 64..80;
//   - the union at byte 216 of RolloutArgs, the slot weights behind it at 296
//     (pointer) and 304 (stride), prob_n / prob_off behind them at 312 / 316,
//     320 bytes in all;
//   - the slot-weight arguments round-trip at those raw offsets, and neither
//     they nor the StateArgs, the count, the target arguments or the problem
//     fields disturb one another, in any order of setting;
//   - has_state() / scenarios() for every combination of a state block, a
//     scenario count, a target schedule and a slot-weight block, with and
//     without dpar
// and prints "OK slotw_host", or "FAIL why" with exit status 1.  Built with
// the address and undefined-behaviour sanitizers and run by
// tests/test_slotw_lib.py.
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include "../../manipulator_mujoco_amd/csrc/rollout.h"

using namespace mpcr;

static_assert(sizeof(StateArgs) == 56, "StateArgs: 56 of par's 80 bytes");
static_assert(offsetof(StateArgs, start) == 0 && offsetof(StateArgs, final_state) == 8 &&
                  offsetof(StateArgs, start_stride) == 16 && offsetof(StateArgs, ctrl_stride) == 20 &&
                  offsetof(StateArgs, ctrl_step_stride) == 24 && offsetof(StateArgs, ctrl) == 32 &&
                  offsetof(StateArgs, geom_pose) == 40 && offsetof(StateArgs, geom_stride) == 48 &&
                  offsetof(StateArgs, geom_step_stride) == 52,
              "StateArgs keeps its field order");
static_assert(offsetof(CallBlocks, nscen) == 56 && offsetof(CallBlocks, tg) == 64 && sizeof(TargetArgs) == 16 &&
                  sizeof(float) * PAR_N == 80 && sizeof(CallBlocks) == 80 && offsetof(CallBlocks, st) == 0,
              "the count at 56, the target schedule at 64..80");
static_assert(offsetof(RolloutArgs, par) == 216 && offsetof(RolloutArgs, blk) == 216 &&
                  offsetof(RolloutArgs, prob_n) == 312 && offsetof(RolloutArgs, prob_off) == 316,
              "the union where it was, the problem fields at the arguments' end");
static_assert(offsetof(RolloutArgs, sw) == 296 && sizeof(SlotWArgs) == 16 && offsetof(SlotWArgs, slot_w) == 0 &&
                  offsetof(SlotWArgs, stride) == 8 && sizeof(RolloutArgs) == 320,
              "the slot weights behind the union: pointer at 296, stride at 304");

static int fail(const char* why) {
  printf("FAIL %s\n", why);
  return 1;
}

static bool same_state(const StateArgs& a, const StateArgs& b) {
  return a.start == b.start && a.final_state == b.final_state && a.start_stride == b.start_stride &&
         a.ctrl_stride == b.ctrl_stride && a.ctrl_step_stride == b.ctrl_step_stride && a.ctrl == b.ctrl &&
         a.geom_pose == b.geom_pose && a.geom_stride == b.geom_stride && a.geom_step_stride == b.geom_step_stride;
}

int main() {
  static const float dummy[32] = {};
  static float out[8];
  const StateArgs none = {nullptr, nullptr, 0, 0, 0, nullptr, nullptr, 0, 0};
  const StateArgs full = {dummy, out, 60, 12, 4, dummy + 4, dummy + 8, 16, 8};
  const TargetArgs tg = {dummy + 16, 96, 8};
  const SlotWArgs sw = {dummy + 20, 188, 0};
  // round trips at the raw offsets
  {
    RolloutArgs a;
    memset(&a, 0, sizeof(a));
    const char* raw = reinterpret_cast<const char*>(&a);
    a.dpar = dummy;
    a.sw = sw;
    const float* p = nullptr;
    int st = 0;
    memcpy(&p, raw + 296, sizeof(p));
    memcpy(&st, raw + 304, sizeof(st));
    if (p != sw.slot_w || st != 188) return fail("slot-weight arguments at offsets 296, 304");
    // nothing outside bytes 296..312 but dpar was written
    for (size_t i = 0; i < sizeof(a); i++)
      if (raw[i] != 0 && !(i >= 296 && i < 312) &&
          !(i >= offsetof(RolloutArgs, dpar) && i < offsetof(RolloutArgs, dpar) + sizeof(a.dpar)))
        return fail("the slot weights wrote outside their bytes");
    a.blk.nscen = 5;
    a.blk.tg = tg;
    a.blk.st = full;
    a.prob_n = 7;
    a.prob_off = 9;
    int n = 0, pn[2] = {0, 0};
    memcpy(&n, raw + 216 + 56, sizeof(n));
    memcpy(pn, raw + 312, sizeof(pn));
    if (n != 5 || pn[0] != 7 || pn[1] != 9) return fail("scenario count at 216 + 56, prob_n / prob_off at 312 / 316");
    memcpy(&p, raw + 216 + 64, sizeof(p));
    if (p != tg.target) return fail("target pointer at 216 + 64");
    if (a.sw.slot_w != sw.slot_w || a.sw.stride != 188)
      return fail("the blocks or the problem fields disturbed the slot weights");
    if (!same_state(a.blk.st, full) || a.blk.nscen != 5 || a.blk.tg.target != tg.target || a.blk.tg.stride != 96 ||
        a.blk.tg.step_stride != 8)
      return fail("CallBlocks round trip beside the slot weights");
    a.sw = SlotWArgs{nullptr, 0, 0};
    if (!same_state(a.blk.st, full) || a.blk.nscen != 5 || a.blk.tg.target != tg.target || a.prob_n != 7 ||
        a.prob_off != 9)
      return fail("clearing the slot weights disturbed the rest");
    // the parameter values of a call without dpar do not reach them either
    for (int k = 0; k < PAR_N; k++) a.par[k] = 1.5f + k;
    if (a.sw.slot_w || a.sw.stride || a.prob_n != 7) return fail("par's values reached the slot weights");
  }
  // has_state() / scenarios() for each combination
  for (int with_dpar = 0; with_dpar < 2; with_dpar++)
    for (int with_state = 0; with_state < 2; with_state++)
      for (int nscen = 0; nscen < 4; nscen++)
        for (int with_target = 0; with_target < 2; with_target++)
          for (int with_sw = 0; with_sw < 2; with_sw++) {
            RolloutArgs a;
            memset(&a, 0, sizeof(a));
            a.dpar = with_dpar ? dummy : nullptr;
            StateArgs s = none;
            if (with_state) s.geom_pose = dummy;
            a.blk.st = s;
            a.blk.nscen = nscen;
            a.blk.tg = with_target ? tg : TargetArgs{nullptr, 0, 0};
            a.sw = with_sw ? sw : SlotWArgs{nullptr, 0, 0};
            const bool want_state = with_dpar && (with_state || nscen > 1 || with_target || with_sw);
            const int want_scen = with_dpar && nscen > 1 ? nscen : 0;
            if (has_state(a) != want_state || scenarios(a) != want_scen) {
              printf("FAIL has_state / scenarios: dpar %d state %d nscen %d target %d slot_w %d -> %d, %d\n", with_dpar,
                     with_state, nscen, with_target, with_sw, (int)has_state(a), scenarios(a));
              return 1;
            }
          }
  printf("OK slotw_host\n");
  return 0;
}
