// rollout_plan.h -- how a rollout call becomes kernel launches, host code only
// (engine.hip includes it): waves per candidate by batch size, horizon
// segments over candidate groups on their own streams.  The kernels and their
// class launchers are rollout_narrow.hip's and rollout_wide.hip's; the
// planning is pure in (RolloutArgs, grid, groups, PlanThresholds), which
// tests/c_host/plan_host.cpp pins without a GPU, and rollout_launch issues it.
#pragma once
#include <algorithm>
#include <atomic>
#include <cstdlib>

#include "rollout.h"

namespace mpcr {

inline int env_int(const char* name, int dflt) {
  const char* e = getenv(name);
  return e ? atoi(e) : dflt;
}
// batches up to this many candidates run the narrow variant with two waves
// per candidate (MPCR_WPC2_MAX_N overrides; 0 disables): below one
// candidate per SIMD pair the second wave of a SIMD is otherwise idle
// (process-wide, atomic: read by every engine's launches, initialised once
// from the environment when the library loads)
#ifndef MPCR_WPC2_MAX_N_DEFAULT
#define MPCR_WPC2_MAX_N_DEFAULT 2048  // C3 512 / 1024 / 2048: 1.38 / 1.43 / 1.52 -> 1.07 / 1.09 / 1.20 ms,
                                      // 4096: 1.77 -> 3.03 ms, the one-wave kernel stays
#endif
inline std::atomic<int> g_wpc2_max_n{env_int("MPCR_WPC2_MAX_N", MPCR_WPC2_MAX_N_DEFAULT)};
#ifdef MPCR_STOP_AFTER
// attribution builds stop a wave mid-step; the two-wave kernels would leave
// its partner at an unmatched barrier, so these builds run one wave only
inline int wpc2_max_n() { return 0; }
#else
inline int wpc2_max_n() { return g_wpc2_max_n.load(std::memory_order_relaxed); }
#endif
// two waves per candidate up to n (narrow variant); returns the previous
inline int rollout_set_wpc2_max_n(int n) { return n >= 0 ? g_wpc2_max_n.exchange(n) : wpc2_max_n(); }
// Dual-arm batches up to min(this, the narrow threshold above) run two waves
// per candidate too (rollout_kernel<32, 32, 72, true, 2>: collision, the MPR
// flush and the manifolds beside the dynamics).  Its 29 KB image and 235
// VGPRs leave 4 blocks per CU, so the default is 4 x 256 CUs: every candidate
// resident in one round (measured on MI355X, H = 100: 1024 candidates 22.6 ->
// 21.2 ms; 2048 would take two rounds, 24.5 -> 46.3 ms).  Bitwise the one-wave
// results.  MPCR_WPC2W_MAX_N overrides.
inline const int g_wpc2w_max_n = env_int("MPCR_WPC2W_MAX_N", 1024);
// the two thresholds a plan is made with: the process's, or a test's own
struct PlanThresholds {
  int narrow2, wide2;  // two waves per candidate for grids up to these (single-arm, dual-arm class)
};
inline PlanThresholds plan_thresholds() { return {wpc2_max_n(), std::min(g_wpc2w_max_n, wpc2_max_n())}; }
// waves per candidate of a launch over `grid` candidates
inline int plan_wpc(bool wide, unsigned grid, const PlanThresholds& th) {
  return (int)grid <= (wide ? th.wide2 : th.narrow2) ? 2 : 1;
}

// RolloutArgs of candidates [off, off + n) of a launch: the per-candidate
// pointers advanced by off (the kernel indexes them by its block)
inline RolloutArgs group_args(const RolloutArgs& a, int off, int n) {
  RolloutArgs g = a;
  const size_t o = (size_t)off;
  g.n = n;
  if (a.prob_n) {
    // several problems: the kernel derives problem and local index from the
    // candidate's place in the call (a group need not start at a problem)
    g.prob_off = a.prob_off + off;
  } else {
    g.index_base = a.index_base + off;
  }
  const size_t in_row = a.layout == 0 ? (size_t)a.nctrl * a.nbasis : (size_t)a.nctrl * a.H;
  const size_t th_row = (size_t)a.nctrl * a.H;
  // scenarios share their input rows, which the kernel finds through
  // prob_off: input, theta and thetadot stay the call's
  if (!scenarios(a)) {
    g.input = a.input + o * in_row;
    if (a.theta) g.theta = a.theta + o * th_row;
    if (a.thetadot) g.thetadot = a.thetadot + o * th_row;
  }
  g.cost4 = a.cost4 + 4 * o;
  if (a.status) g.status = a.status + o;
  if (a.trace_eef) g.trace_eef = a.trace_eef + o * a.H * 7;
  if (a.trace_slots) g.trace_slots = a.trace_slots + o * a.H * a.nslot;
  g.jx = a.jx + o * (SmemW::MAXEFC - SmemW::JL) * SmemW::LDJ;
  g.hints = a.hints + o * SmemW::NHINT * 2;
  g.mslab = a.mslab + o * SmemW::NVW * SmemW::LD;
  g.tdscratch = a.tdscratch + o * th_row;
  g.slot_prev = a.slot_prev + o * (a.nslot > 0 ? a.nslot : 1);
  g.seg_state = a.seg_state + o * SEG_STRIDE;
  // final states are per candidate; the other blocks are per problem, which
  // prob_off locates (one problem: the one block), so they stay put
  if (has_state(a) && g.blk.st.final_state) g.blk.st.final_state += o * ST_N;
  return g;
}

// whether rollout_launch runs a batch as horizon segments, and over how many
// candidate groups (*G)
inline bool seg_plan(bool wide, const RolloutArgs& a, unsigned grid, int groups, bool streams,
                     const PlanThresholds& th, int* G) {
  if (!wide || plan_wpc(wide, grid, th) == 2) return false;
  if (!(a.seg > 0 && a.seg < a.H && a.seg_state && !a.plant && !a.dbg && (int)grid > a.seg_min_n)) return false;
  *G = groups > 1 && streams && (int)grid >= 2 * groups ? groups : 1;
  return true;
}

// kernel dispatches rollout_launch issues for the same arguments (streams:
// gstream / gev given)
inline int rollout_dispatches(bool wide, const RolloutArgs& a, unsigned grid, int groups, bool streams,
                              const PlanThresholds& th) {
  int G = 1;
  if (grid == 0) return 0;
  if (!seg_plan(wide, a, grid, groups, streams, th, &G)) return 1;
  return G * ((a.H + a.seg - 1) / a.seg);
}

// The rollout kernel variant for the model class over `grid` blocks.
// Dual-arm batches of the one-wave variant with a.seg > 0 and H > a.seg run as
// horizon segments of a.seg steps over `groups` candidate groups, group g on
// gstream[g] (forked from st by gev[0] and joined back by gev[1 + g]); every
// group's segments in stream order.  The launches of different groups overlap,
// so one segment's tail is filled by the other groups' work.
inline void rollout_launch(bool wide, const RolloutArgs& a0, const DevModel* dm, unsigned grid, hipStream_t st,
                           int groups = 0, hipStream_t* gstream = nullptr, hipEvent_t* gev = nullptr,
                           const StepWArgs& stw = StepWArgs{nullptr, 0, 0}) {
  RolloutArgs a = a0;
  a.t0 = 0;
  a.t1 = a.H;
  const PlanThresholds th = plan_thresholds();
  int G = 1;
  if (!wide) {
    rollout_narrow_launch(plan_wpc(wide, grid, th), grid, st, a, dm, stw);
  } else if (!seg_plan(wide, a, grid, groups, gstream && gev, th, &G)) {
    rollout_wide_launch(plan_wpc(wide, grid, th), grid, st, a, dm, stw);
  } else {
    // horizon segments over candidate groups on their own streams: each
    // group's segments in its stream's order, the groups overlapping
    if (G > 1) {
      (void)hipEventRecord(gev[0], st);
      for (int g = 0; g < G; g++) (void)hipStreamWaitEvent(gstream[g], gev[0], 0);
    }
    const int per = ((int)grid + G - 1) / G;
    for (int g = 0; g < G; g++) {
      const int off = g * per, ng = std::min(per, (int)grid - off);
      if (ng <= 0) break;
      RolloutArgs ga = G > 1 ? group_args(a, off, ng) : a;
      hipStream_t gs = G > 1 ? gstream[g] : st;
      for (int t0 = 0; t0 < a.H; t0 += a.seg) {
        ga.t0 = t0;
        ga.t1 = std::min(a.H, t0 + a.seg);
        rollout_wide_launch(1, ng, gs, ga, dm, stw);  // (the schedule is per problem, which prob_off locates)
      }
    }
    if (G > 1)
      for (int g = 0; g < G; g++) {
        (void)hipEventRecord(gev[1 + g], gstream[g]);
        (void)hipStreamWaitEvent(st, gev[1 + g], 0);
      }
  }
}

}  // namespace mpcr
