// rollout_instruments.h -- the rollout kernel's diagnostic macros (rollout.hip): phase stamps and
// counters of the profiling builds, the pacing priority, the attribution stop.
#pragma once

namespace mpcr {

// ---------------------------------------------------------------------------
// diagnostic phase stamps (separate -DMPCR_PROFILE build; never in the timed one)
#ifdef MPCR_PROFILE
#define PROF_DECL unsigned long long prof_acc[32] = {0}; unsigned long long prof_last = __builtin_amdgcn_s_memtime();
#define STAMP(i)                                              \
  do {                                                        \
    unsigned long long now_ = __builtin_amdgcn_s_memtime();   \
    prof_acc[i] += now_ - prof_last;                          \
    prof_last = now_;                                         \
  } while (0)
// (a candidate's second wave, WPC = 2, into slots 32..63: per-wave critical paths)
#define PROF_FLUSH                                                          \
  if (lane == 0 && KA->prof)                                               \
    for (int i_ = 0; i_ < 32; i_++) atomicAdd(&KA->prof[i_ + 32 * (threadIdx.x >> 6)], prof_acc[i_]);
// wave-level event counter (first active lane adds 1; -DMPCR_PROFILE_COUNTS
// only: the shared atomics distort the cycle shares)
#ifdef MPCR_PROFILE_COUNTS
#define PROF_COUNT(m, i)                                                                  \
  do {                                                                                    \
    if ((m)->prof && (int)__lane_id() == __builtin_ctzll(__ballot(1))) atomicAdd((m)->prof + (i), 1ull); \
  } while (0)
#else
#define PROF_COUNT(m, i)
#endif
// sub-phase stamps inside a device function (one atomic per stamp and wave)
#define PSTAMP_DECL unsigned long long pst_ = __builtin_amdgcn_s_memtime();
#define PSTAMP(m, i)                                                                       \
  do {                                                                                     \
    const unsigned long long now_ = __builtin_amdgcn_s_memtime();                          \
    if ((m)->prof && (int)__lane_id() == 0) atomicAdd((m)->prof + (i) + 32 * (threadIdx.x >> 6), now_ - pst_); \
    pst_ = now_;                                                                           \
  } while (0)
#else
#define PSTAMP_DECL
#define PSTAMP(m, i)
#define PROF_DECL
#define STAMP(i)
#define PROF_FLUSH
#define PROF_COUNT(m, i)
#endif
// Pacing (load balance of a one-round launch): at N = 4096 every candidate is
// resident at once (4 waves per SIMD) and the launch ends with the slowest
// candidate, ~18 % after the mean one (tools/wavetime.py).  Each wave posts
// the step it is on in its SIMD's slot group and takes an issue priority
// equal to the number of its SIMD mates ahead of it, so the waves sharing a
// SIMD progress together and the SIMD drains when its total work is done.
// Pacing in the dual-arm kernel too: 1.7 % slower at 7 blocks per CU (2.3
// backfilled rounds), ~0.8 % faster at 8 (C4 4096 x 100: 33.6-34.0 vs
// 34.1 ms; 8192 x 50: 30.35-30.45 vs 30.57-30.79 ms).
// The mates' progress read at the step start is consumed before the
// collision phase (mid-step).
#define PACE_SETPRIO() \
  if (pace) {  /* priority = SIMD mates ahead of this wave (0..3) */ \
  const int ahead = __popcll(__ballot(lane < 16 && lane != pace_own && pace_v != ~0u && pace_v > (unsigned)t)); \
  if (ahead >= 3) __builtin_amdgcn_s_setprio(3); \
  else if (ahead == 2) __builtin_amdgcn_s_setprio(2); \
  else if (ahead == 1) __builtin_amdgcn_s_setprio(1); \
  else __builtin_amdgcn_s_setprio(0); \
  }

// instruction-count attribution builds (-DMPCR_STOP_AFTER=k, diagnostic only):
// the step ends right after phase stamp k, so PMC differences between k and
// the previous stop are that phase's instructions
#ifdef MPCR_STOP_AFTER
#define STOP_AT(k) \
  if (MPCR_STOP_AFTER == (k)) continue;
#else
#define STOP_AT(k)
#endif
// sub-stamps inside the constraint-rows phase (-DMPCR_PROFILE -DMPCR_PROFILE_ROWS,
// single-arm kernels: slots 23..25 are the dual-arm polyhedron manifold's):
// 23 head, 24 equality / limit Jacobians, 25 contact Jacobians; the row
// parameters are then what is left in slot 8
#if defined(MPCR_PROFILE) && defined(MPCR_PROFILE_ROWS)
#define ROWS_STAMP(i) STAMP(i)
#else
#define ROWS_STAMP(i)
#endif

}  // namespace mpcr
