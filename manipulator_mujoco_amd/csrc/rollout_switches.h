// rollout_switches.h -- the rollout device code's build switches that more than the kernel
// reads (rollout.hip), and the step table behind the device model.
#pragma once
#include "rollout.h"
#include "step_table.h"

namespace mpcr {

#ifndef MPCR_CB_SKIP
#define MPCR_CB_SKIP 1  // capsule-box: skip the interior knots when no lane's minimum is inside (narrow_lane)
#endif

// MPCR_STEP_TABLE: which phases of the single-arm kernels read the step table
// (bit 0 kinematics, 1 motion subspaces, 2 constraint rows, 3 the load
// records: one-level batched loads in place of dependent chains -- rows
// phase, mass matrix, collision cull, narrow_lane's head, emit_contacts); 15
// is the shipped build, the others attribute a change in results or time
#ifndef MPCR_STEP_TABLE
#define MPCR_STEP_TABLE 15
#endif
template <class S> constexpr bool kStepKin = !S::WIDE && (MPCR_STEP_TABLE & 1) != 0;
template <class S> constexpr bool kStepDof = !S::WIDE && (MPCR_STEP_TABLE & 2) != 0;
template <class S> constexpr bool kStepRow = !S::WIDE && (MPCR_STEP_TABLE & 4) != 0;
template <class S> constexpr bool kStepLoad = !S::WIDE && (MPCR_STEP_TABLE & 8) != 0;
// MPCR_LANE_WORK: which one-lane or repeated work of the single-arm step is
// built in its cheaper form (bit 0 the pose cost's transcendental tail deferred
// and spread over lanes, 1 the trees' centres of mass in one reduction, 2
// Newton's first rows from the warm-start choice, 3 the line search's q0 at
// alpha = 0 from Newton's cost).  Every built form sits behind
// DEV_NO_LANE_WORK in the device model's flags (the environment's
// MPCR_LANE_WORK=0 at engine creation, tests -- an on / off switch for all
// items, not this mask): the former path stays reachable in the same build.
// 15 is the shipped build; the others attribute a change in results or time
// (tools/build_variant.py).
#ifndef MPCR_LANE_WORK
#define MPCR_LANE_WORK 15
#endif
template <class S> constexpr bool kLanePose = !S::WIDE && (MPCR_LANE_WORK & 1) != 0;
template <class S> constexpr bool kLaneCom = !S::WIDE && (MPCR_LANE_WORK & 2) != 0;
template <class S> constexpr bool kLaneJar = !S::WIDE && (MPCR_LANE_WORK & 4) != 0;
template <class S> constexpr bool kLaneQ0 = !S::WIDE && (MPCR_LANE_WORK & 8) != 0;
// The step table (step_table.h) behind the device model, and quad q (16
// bytes: one dwordx4 load) of one of its records.  Single-arm kernels only.
__device__ __forceinline__ const StepTable* step_table(const DevModel* m) {
  return reinterpret_cast<const StepTable*>(m + 1);
}
// ... and the load records behind the table
__device__ __forceinline__ const StepRecords* step_records(const DevModel* m) {
  return reinterpret_cast<const StepRecords*>(step_table(m) + 1);
}
template <class R>
__device__ __forceinline__ float4 recq(const R& r, int q) {
  return reinterpret_cast<const float4*>(&r)[q];
}

}  // namespace mpcr
