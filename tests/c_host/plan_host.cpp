// A stand-alone host of the launch planning (csrc/rollout_plan.h; no libmpcr,
// nothing launched, no GPU opened), on hand-filled RolloutArgs and thresholds
// of its own.  It checks
//   - rollout_dispatches: 0 for an empty grid; 1 wherever seg_plan declines
//     (single-arm class, a grid within the two-wave threshold, seg == 0, seg >=
//     H, no seg_state, plant mode, dbg set, grid <= seg_min_n); G ceil(H / seg)
//     otherwise, G = groups only with streams and grid >= 2 groups, else 1
//     (H = 12 and 14 with seg = 7, groups 2);
//   - plan_wpc: two waves up to the class's threshold, one above;
//   - group_args on a several-problem call: prob_off advances and index_base
//     stays, every per-candidate pointer advances by its own row size,
//     blk.st.final_state by off ST_N, and start, ctrl, geom_pose and tg stay;
//     on a one-problem call index_base advances instead; with scenarios input,
//     theta and thetadot stay where they are, without they advance
// and prints "OK plan_host", or "FAIL why" with exit status 1.  Built with the
// address and undefined-behaviour sanitizers and run by tests/test_plan_lib.py.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../manipulator_mujoco_amd/csrc/rollout.h"
#include "../../manipulator_mujoco_amd/csrc/rollout_plan.h"

using namespace mpcr;

static int fail(const char* why) {
  printf("FAIL %s\n", why);
  return 1;
}

int main() {
  const PlanThresholds th = {2048, 1024};
  if (plan_wpc(false, 2048, th) != 2 || plan_wpc(false, 2049, th) != 1 || plan_wpc(true, 1024, th) != 2 ||
      plan_wpc(true, 1025, th) != 1 || plan_wpc(true, 5, PlanThresholds{0, 0}) != 1)
    return fail("plan_wpc at the thresholds");

  // a dual-arm call that runs as segments: grid above the two-wave threshold and seg_min_n
  static float segbuf[4], dbgbuf[4];
  RolloutArgs s;
  memset(&s, 0, sizeof(s));
  s.H = 12;
  s.seg = 7;
  s.seg_state = segbuf;
  s.seg_min_n = 2048;
  const unsigned grid = 4096;
  const int groups = 2;
  // dispatches
  {
    if (rollout_dispatches(true, s, 0, groups, true, th) != 0 || rollout_dispatches(false, s, 0, groups, true, th) != 0)
      return fail("an empty grid dispatches nothing");
    if (rollout_dispatches(true, s, grid, groups, true, th) != 2 * 2) return fail("H 12, seg 7, two groups: 4");
    if (rollout_dispatches(true, s, grid, groups, false, th) != 2) return fail("no streams: one group");
    if (rollout_dispatches(true, s, grid, 1, true, th) != 2 || rollout_dispatches(true, s, grid, 0, true, th) != 2)
      return fail("groups <= 1: one group");
    RolloutArgs a = s;
    a.seg_min_n = 2;
    if (rollout_dispatches(true, a, 3, groups, true, PlanThresholds{0, 0}) != 2) return fail("grid < 2 groups: one group");
    if (rollout_dispatches(true, a, 4, groups, true, PlanThresholds{0, 0}) != 4) return fail("grid == 2 groups: groups");
    a = s;
    a.H = 14;
    if (rollout_dispatches(true, a, grid, groups, true, th) != 2 * 2) return fail("H 14, seg 7, two groups: 4");
    a.H = 15;
    if (rollout_dispatches(true, a, grid, groups, true, th) != 2 * 3) return fail("H 15, seg 7, two groups: 6");
    // seg_plan declines
    int G = 7;
    if (seg_plan(false, s, grid, groups, true, th, &G) || rollout_dispatches(false, s, grid, groups, true, th) != 1)
      return fail("the single-arm class has no segments");
    if (rollout_dispatches(true, s, 1024, groups, true, PlanThresholds{2048, 1024}) != 1) return fail("two-wave grid");
    a = s; a.seg_min_n = 0;
    if (rollout_dispatches(true, a, 1024, groups, true, th) != 1) return fail("two-wave grid above seg_min_n");
    if (rollout_dispatches(true, a, 1025, groups, true, th) != 4) return fail("one past the two-wave threshold");
    a = s; a.seg = 0;
    if (rollout_dispatches(true, a, grid, groups, true, th) != 1) return fail("seg == 0");
    a = s; a.seg = 12;
    if (rollout_dispatches(true, a, grid, groups, true, th) != 1) return fail("seg == H");
    a = s; a.seg = 13;
    if (rollout_dispatches(true, a, grid, groups, true, th) != 1) return fail("seg > H");
    a = s; a.seg_state = nullptr;
    if (rollout_dispatches(true, a, grid, groups, true, th) != 1) return fail("no seg_state");
    a = s; a.plant = 1;
    if (rollout_dispatches(true, a, grid, groups, true, th) != 1) return fail("plant mode");
    a = s; a.dbg = dbgbuf;
    if (rollout_dispatches(true, a, grid, groups, true, th) != 1) return fail("dbg set");
    a = s; a.seg_min_n = (int)grid;
    if (rollout_dispatches(true, a, grid, groups, true, th) != 1) return fail("grid == seg_min_n");
    a.seg_min_n = (int)grid - 1;
    if (rollout_dispatches(true, a, grid, groups, true, th) != 4) return fail("grid == seg_min_n + 1");
    if (G != 7) return fail("a declined plan wrote the group count");
    if (!seg_plan(true, s, grid, groups, true, th, &G) || G != 2) return fail("seg_plan's group count");
  }

  // group_args: candidates [off, off + n) of a call of N
  const int N = 8, off = 3, n = 4, H = 12, nctrl = 6, nbasis = 5, nslot = 9;
  const size_t jx_row = (size_t)(SmemW::MAXEFC - SmemW::JL) * SmemW::LDJ, hint_row = (size_t)SmemW::NHINT * 2,
               m_row = (size_t)SmemW::NVW * SmemW::LD, th_row = (size_t)nctrl * H;
  std::vector<float> input(N * th_row), theta(N * th_row), thetadot(N * th_row), cost4(N * 4), eef((size_t)N * H * 7),
      slots((size_t)N * H * nslot), prev((size_t)N * nslot), jx(N * jx_row), mslab((N + 1) * m_row),
      td((N + 1) * th_row), seg((size_t)N * SEG_STRIDE), fin((size_t)N * ST_N), start(ST_N), ctrl(8), gpose(16), tgt(8),
      dpar(2 * PAR_N);
  std::vector<int> status(N);
  std::vector<short> hints(N * hint_row);
  for (int layout = 0; layout < 2; layout++)
    for (int nprob = 1; nprob <= 2; nprob++)
      for (int nscen = 0; nscen <= 2; nscen += 2)
        for (int blocks = 0; blocks < 2; blocks++) {
          if (nscen && nprob == 1) continue;  // scenarios are problems of a several-problem call
          RolloutArgs a;
          memset(&a, 0, sizeof(a));
          a.layout = layout; a.n = N; a.H = H; a.nbasis = nbasis; a.nctrl = nctrl; a.nslot = nslot;
          a.index_base = 100; a.prob_n = nprob > 1 ? N / nprob : 0; a.prob_off = nprob > 1 ? 16 : 0;
          a.input = input.data(); a.theta = theta.data(); a.thetadot = thetadot.data(); a.cost4 = cost4.data();
          a.status = status.data(); a.trace_eef = eef.data(); a.trace_slots = slots.data(); a.slot_prev = prev.data();
          a.jx = jx.data(); a.hints = hints.data(); a.mslab = mslab.data(); a.tdscratch = td.data();
          a.seg_state = seg.data(); a.dpar = dpar.data();
          a.blk.nscen = nscen;
          if (blocks) {
            a.blk.st = StateArgs{start.data(), fin.data(), 0, 0, 4, ctrl.data(), gpose.data(), 0, 8};
            a.blk.tg = TargetArgs{tgt.data(), 0, 8};
          }
          const RolloutArgs g = group_args(a, off, n);
          if (g.n != n) return fail("group_args: n");
          if (nprob > 1 ? g.prob_off != 16 + off || g.index_base != 100 : g.index_base != 100 + off || g.prob_off != 0)
            return fail("group_args: prob_off (several problems) or index_base (one) advances, the other stays");
          const size_t in_row = layout == 0 ? (size_t)nctrl * nbasis : th_row;
          if (scenarios(a) != nscen) return fail("scenarios()");
          if (nscen) {
            if (g.input != a.input || g.theta != a.theta || g.thetadot != a.thetadot)
              return fail("group_args: scenarios leave input, theta and thetadot");
          } else if (g.input != a.input + off * in_row || g.theta != a.theta + off * th_row ||
                     g.thetadot != a.thetadot + off * th_row) {
            return fail("group_args: input, theta, thetadot rows");
          }
          if (g.cost4 != a.cost4 + 4 * off || g.status != a.status + off) return fail("group_args: cost4, status");
          if (g.trace_eef != a.trace_eef + (size_t)off * H * 7 || g.trace_slots != a.trace_slots + (size_t)off * H * nslot)
            return fail("group_args: traces");
          if (g.jx != a.jx + off * jx_row || g.hints != a.hints + off * hint_row || g.mslab != a.mslab + off * m_row)
            return fail("group_args: jx, hints, mslab");
          if (g.tdscratch != a.tdscratch + off * th_row || g.slot_prev != a.slot_prev + (size_t)off * nslot ||
              g.seg_state != a.seg_state + (size_t)off * SEG_STRIDE)
            return fail("group_args: tdscratch, slot_prev, seg_state");
          if (g.blk.st.final_state != (blocks ? a.blk.st.final_state + (size_t)off * ST_N : nullptr))
            return fail("group_args: final_state by off ST_N");
          CallBlocks want = a.blk;
          want.st.final_state = g.blk.st.final_state;
          if (memcmp(&g.blk, &want, sizeof(want))) return fail("group_args: start, ctrl, geom_pose, nscen, tg stay");
          if (g.m != a.m || g.pdot != a.pdot || g.best_key != a.best_key || g.dpar != a.dpar || g.H != a.H ||
              g.prob_n != a.prob_n)
            return fail("group_args: the call's own fields stay");
        }
  // null optional outputs stay null, a model without slots keeps one word per candidate
  {
    RolloutArgs a;
    memset(&a, 0, sizeof(a));
    a.H = H; a.nctrl = nctrl; a.nbasis = nbasis;
    a.input = input.data(); a.cost4 = cost4.data(); a.slot_prev = prev.data(); a.jx = jx.data(); a.hints = hints.data();
    a.mslab = mslab.data(); a.tdscratch = td.data(); a.seg_state = seg.data();
    const RolloutArgs g = group_args(a, off, n);
    if (g.theta || g.thetadot || g.status || g.trace_eef || g.trace_slots) return fail("group_args: null outputs");
    if (g.slot_prev != a.slot_prev + off) return fail("group_args: slot_prev without slots");
  }
  printf("OK plan_host\n");
  return 0;
}
