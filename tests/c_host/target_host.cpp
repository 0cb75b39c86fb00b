// A stand-alone host of what csrc/rollout.h holds for the target schedule as
// a call input (no libmpcr, nothing launched, no GPU opened): the bytes of
// RolloutArgs::par a call with a device parameter block carries its blocks
// in (CallBlocks, RolloutArgs::blk).  It checks
//   - sizeof(StateArgs) == 56 with the field offsets it had;
//   - the scenario count round-trips at byte 56;
//   - the target arguments round-trip at bytes 64..80, and neither the
//     StateArgs nor the count nor the target arguments disturb one another,
//     in any order of setting;
//   - has_state() / scenarios() for every combination of a state block, a
//     scenario count and a target schedule, with and without dpar;
//   - target_quat_unit: a scaled quaternion's unit, in place as well
// and prints "OK target_host", or "FAIL why" with exit status 1.  Built with
// the address and undefined-behaviour sanitizers and run by
// tests/test_target_lib.py.
#include <math.h>
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
static_assert(offsetof(TargetArgs, target) == 0 && offsetof(TargetArgs, stride) == 8 &&
                  offsetof(TargetArgs, step_stride) == 12,
              "one pointer and two ints");

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
  // round trips at the raw offsets
  {
    RolloutArgs a;
    memset(&a, 0, sizeof(a));
    a.dpar = dummy;
    a.blk.nscen = 5;
    int n = 0;
    memcpy(&n, reinterpret_cast<const char*>(a.par) + 56, sizeof(n));
    if (n != 5 || a.blk.nscen != 5) return fail("scenario count at offset 56");
    a.blk.tg = tg;
    const float* p = nullptr;
    int st[2] = {0, 0};
    memcpy(&p, reinterpret_cast<const char*>(a.par) + 64, sizeof(p));
    memcpy(st, reinterpret_cast<const char*>(a.par) + 72, sizeof(st));
    if (p != tg.target || st[0] != 96 || st[1] != 8) return fail("target arguments at offsets 64, 72, 76");
    if (a.blk.nscen != 5) return fail("the target arguments disturbed the scenario count");
    a.blk.st = full;
    if (!same_state(a.blk.st, full)) return fail("StateArgs round trip");
    TargetArgs t = a.blk.tg;
    if (t.target != tg.target || t.stride != 96 || t.step_stride != 8 || a.blk.nscen != 5)
      return fail("the StateArgs disturbed the count or the target arguments");
    a.blk.nscen = 3;
    a.blk.tg = TargetArgs{nullptr, 0, 0};
    if (!same_state(a.blk.st, full) || a.blk.nscen != 3) return fail("clearing the target disturbed the rest");
    t = a.blk.tg;
    if (t.target || t.stride || t.step_stride) return fail("cleared target arguments");
    // bytes 60..64 stay what they were (zero)
    int pad = 1;
    memcpy(&pad, reinterpret_cast<const char*>(a.par) + 60, sizeof(pad));
    if (pad != 0) return fail("bytes 60..64 written");
  }
  // has_state() / scenarios() for each combination
  for (int with_dpar = 0; with_dpar < 2; with_dpar++)
    for (int with_state = 0; with_state < 2; with_state++)
      for (int nscen = 0; nscen < 4; nscen++)
        for (int with_target = 0; with_target < 2; with_target++) {
          RolloutArgs a;
          memset(&a, 0, sizeof(a));
          a.dpar = with_dpar ? dummy : nullptr;
          StateArgs s = none;
          if (with_state) s.geom_pose = dummy;
          a.blk.st = s;
          a.blk.nscen = nscen;
          a.blk.tg = with_target ? tg : TargetArgs{nullptr, 0, 0};
          const bool want_state = with_dpar && (with_state || nscen > 1 || with_target);
          const int want_scen = with_dpar && nscen > 1 ? nscen : 0;
          if (has_state(a) != want_state || scenarios(a) != want_scen) {
            printf("FAIL has_state / scenarios: dpar %d state %d nscen %d target %d -> %d, %d\n", with_dpar,
                   with_state, nscen, with_target, (int)has_state(a), scenarios(a));
            return 1;
          }
        }
  // the one normalisation
  {
    const float q[4] = {0.f, 2.f, 0.f, 0.f};
    float u[4], v[4] = {0.6f, -0.8f, 1.2f, 0.4f};
    target_quat_unit(q, u);
    if (u[0] != 0.f || u[1] != 1.f || u[2] != 0.f || u[3] != 0.f) return fail("target_quat_unit of a scaled axis");
    const float n = sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3]);
    const float want[4] = {v[0] / n, v[1] / n, v[2] / n, v[3] / n};
    target_quat_unit(v, v);
    if (memcmp(v, want, sizeof(want))) return fail("target_quat_unit in place");
  }
  printf("OK target_host\n");
  return 0;
}
