// rollout_narrow.hip -- the single-arm rollout kernels (rollout.hip) and the
// launch logic: which variant a batch runs, horizon segments over stream
// groups, occupancy.  Compiled with the fast-math device flags of
// manipulator_mujoco_amd/build.py (C3 is VALU-bound: 1.60 ms, 1.86 ms without
// them); the dual-arm kernels are rollout_wide.hip's.
#include <cstdlib>
#include <atomic>

#include "rollout.hip"

namespace mpcr {

static int env_int(const char* name, int dflt) {
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
static std::atomic<int> g_wpc2_max_n{env_int("MPCR_WPC2_MAX_N", MPCR_WPC2_MAX_N_DEFAULT)};
#ifdef MPCR_STOP_AFTER
// attribution builds stop a wave mid-step; the two-wave kernels would leave
// its partner at an unmatched barrier, so these builds run one wave only
static int wpc2_max_n() { return 0; }
#else
static int wpc2_max_n() { return g_wpc2_max_n.load(std::memory_order_relaxed); }
#endif
int rollout_set_wpc2_max_n(int n) {
  return n >= 0 ? g_wpc2_max_n.exchange(n) : wpc2_max_n();
}
// Dual-arm batches up to min(this, the narrow threshold above) run two waves
// per candidate too (rollout_kernel<32, 32, 72, true, 2>: collision, the MPR
// flush and the manifolds beside the dynamics).  Its 29 KB image and 235
// VGPRs leave 4 blocks per CU, so the default is 4 x 256 CUs: every candidate
// resident in one round (measured on MI355X, H = 100: 1024 candidates 22.6 ->
// 21.2 ms; 2048 would take two rounds, 24.5 -> 46.3 ms).  Bitwise the one-wave
// results.  MPCR_WPC2W_MAX_N overrides.
static const int g_wpc2w_max_n = env_int("MPCR_WPC2W_MAX_N", 1024);
static int wpc2w_max_n() { return min(g_wpc2w_max_n, wpc2_max_n()); }

// RolloutArgs of candidates [off, off + n) of a launch: the per-candidate
// pointers advanced by off (the kernel indexes them by its block)
static RolloutArgs group_args(const RolloutArgs& a, int off, int n) {
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
  // final states are per candidate; the start states are per problem, which
  // prob_off locates (one problem: the one block), so start stays put
  if (has_state(a)) {
    StateArgs sa = state_args(a);
    if (sa.final_state) sa.final_state += o * ST_N;
    set_state_args(g, sa);
  }
  return g;
}

// whether rollout_launch runs a batch as horizon segments, and over how many
// candidate groups (*G)
static bool seg_plan(bool wide, const RolloutArgs& a, unsigned grid, int groups, bool streams, int* G) {
  if (!wide) return false;
  if ((int)grid <= wpc2w_max_n()) return false;
  if (!(a.seg > 0 && a.seg < a.H && a.seg_state && !a.plant && !a.dbg && (int)grid > a.seg_min_n)) return false;
  *G = groups > 1 && streams && (int)grid >= 2 * groups ? groups : 1;
  return true;
}

int rollout_dispatches(bool wide, const RolloutArgs& a, unsigned grid, int groups, bool streams) {
  int G = 1;
  if (grid == 0) return 0;
  if (!seg_plan(wide, a, grid, groups, streams, &G)) return 1;
  return G * ((a.H + a.seg - 1) / a.seg);
}

void rollout_launch(bool wide, const RolloutArgs& a0, const DevModel* dm, unsigned grid, hipStream_t st, int groups,
                    hipStream_t* gstream, hipEvent_t* gev) {
  RolloutArgs a = a0;
  a.t0 = 0;
  a.t1 = a.H;
  int G = 1;
  if (wide && (int)grid <= wpc2w_max_n()) {
    rollout_wide_launch(2, grid, st, a, dm);
  } else if (wide) {
    if (seg_plan(wide, a, grid, groups, gstream && gev, &G)) {
      // horizon segments over candidate groups on their own streams: each
      // group's segments in its stream's order, the groups overlapping
      if (G > 1) {
        (void)hipEventRecord(gev[0], st);
        for (int g = 0; g < G; g++) (void)hipStreamWaitEvent(gstream[g], gev[0], 0);
      }
      const int per = ((int)grid + G - 1) / G;
      for (int g = 0; g < G; g++) {
        const int off = g * per, ng = min(per, (int)grid - off);
        if (ng <= 0) break;
        RolloutArgs ga = G > 1 ? group_args(a, off, ng) : a;
        hipStream_t gs = G > 1 ? gstream[g] : st;
        for (int t0 = 0; t0 < a.H; t0 += a.seg) {
          ga.t0 = t0;
          ga.t1 = min(a.H, t0 + a.seg);
          rollout_wide_launch(1, ng, gs, ga, dm);
        }
      }
      if (G > 1)
        for (int g = 0; g < G; g++) {
          (void)hipEventRecord(gev[1 + g], gstream[g]);
          (void)hipStreamWaitEvent(st, gev[1 + g], 0);
        }
    } else {
      rollout_wide_launch(1, grid, st, a, dm);
    }
  } else {
    const bool multi = a.prob_n > 0;  // several problems: the MULTI instantiations
    // (the STATE instantiations last: the code object lays the kernels out
    // in the order this chain names them, and the others keep their places)
    const bool state = has_state(a);  // state blocks: the STATE instantiations (one problem or several)
    if (!state && (int)grid <= wpc2_max_n() && multi)
      hipLaunchKernelGGL((rollout_kernel<16, 16, 24, false, 2, true>), dim3(grid), dim3(2 * WAVE), 0, st, a, dm);
    else if (!state && (int)grid <= wpc2_max_n())
      hipLaunchKernelGGL((rollout_kernel<16, 16, 24, false, 2>), dim3(grid), dim3(2 * WAVE), 0, st, a, dm);
    else if (!state && multi)
      hipLaunchKernelGGL((rollout_kernel<16, 16, 24, false, 1, true>), dim3(grid), dim3(WAVE), 0, st, a, dm);
    else if (!state)
      hipLaunchKernelGGL((rollout_kernel<16, 16, 24, false>), dim3(grid), dim3(WAVE), 0, st, a, dm);
    else if (!scenarios(a) && (int)grid <= wpc2_max_n())
      hipLaunchKernelGGL((rollout_kernel<16, 16, 24, false, 2, true, true>), dim3(grid), dim3(2 * WAVE), 0, st, a, dm);
    else if (!scenarios(a))
      hipLaunchKernelGGL((rollout_kernel<16, 16, 24, false, 1, true, true>), dim3(grid), dim3(WAVE), 0, st, a, dm);
    // (scenarios: the SCEN instantiations, after every other for the same reason)
    else if ((int)grid <= wpc2_max_n())
      hipLaunchKernelGGL((rollout_kernel<16, 16, 24, false, 2 + WPCS_SCEN, true, true>), dim3(grid), dim3(2 * WAVE), 0, st, a,
                         dm);
    else
      hipLaunchKernelGGL((rollout_kernel<16, 16, 24, false, 1 + WPCS_SCEN, true, true>), dim3(grid), dim3(WAVE), 0, st, a, dm);
  }
}

hipError_t rollout_occupancy(int* info) {
  const void* k = reinterpret_cast<const void*>(&rollout_kernel<16, 16, 24, false>);
  int blocks = 0;
  hipFuncAttributes fa;
  hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, k, WAVE, 0);
  if (e != hipSuccess) return e;
  e = hipFuncGetAttributes(&fa, k);
  if (e != hipSuccess) return e;
  info[0] = blocks;
  info[1] = (int)fa.sharedSizeBytes;
  info[2] = fa.numRegs;
  return rollout_wide_occupancy(info + 3);
}

// mpcr_selftest_reduce: every wave-sum form of rollout.hip on caller-given
// vectors, one 64-lane block per vector.  out[12 b ..] = wsum_ref, wsum,
// wsum2 (a, b), wsum3 (a, b, c), wsum_ref of lanes 0-15, wsum_lo<16>,
// wsum_ref of lanes 0-31, wsum_lo<32>, 0; the second and third values of the
// multi-value forms are vectors b + 1 and b + 2 (cyclic).  Each form gets its
// own opaque copy of the input, so it runs its own instructions start to end.
__device__ __forceinline__ float opaque(float v) {
  asm volatile("" : "+v"(v));
  return v;
}
__global__ __launch_bounds__(WAVE) void reduce_selftest_kernel(const float* __restrict__ in, int n,
                                                               float* __restrict__ out) {
  const int lane = threadIdx.x, b = blockIdx.x;
  const float v = in[(size_t)b * WAVE + lane];
  const float w = in[(size_t)((b + 1) % n) * WAVE + lane];
  const float x = in[(size_t)((b + 2) % n) * WAVE + lane];
  float r[REDUCE_SELFTEST_OUT];
  r[0] = wsum_ref(opaque(v));
  r[1] = wsum(opaque(v));
  r[2] = opaque(v); r[3] = opaque(w);
  wsum2(r[2], r[3]);
  r[4] = opaque(v); r[5] = opaque(w); r[6] = opaque(x);
  wsum3(r[4], r[5], r[6]);
  r[7] = wsum_ref(opaque(lane < 16 ? v : 0.f));
  r[8] = wsum_lo<16>(opaque(lane < 16 ? v : 0.f));
  r[9] = wsum_ref(opaque(lane < 32 ? v : 0.f));
  r[10] = wsum_lo<32>(opaque(lane < 32 ? v : 0.f));
  r[11] = 0.f;
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < REDUCE_SELFTEST_OUT; k++) out[(size_t)b * REDUCE_SELFTEST_OUT + k] = r[k];
  }
}
hipError_t rollout_selftest_reduce(const float* in, int n, float* out) {
  float *din = nullptr, *dout = nullptr;
  const size_t nin = (size_t)n * WAVE * sizeof(float), nout = (size_t)n * REDUCE_SELFTEST_OUT * sizeof(float);
  hipError_t e = hipMalloc(&din, nin);
  if (e == hipSuccess) e = hipMalloc(&dout, nout);
  if (e == hipSuccess) e = hipMemcpy(din, in, nin, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(reduce_selftest_kernel, dim3(n), dim3(WAVE), 0, 0, din, n, dout);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(out, dout, nout, hipMemcpyDeviceToHost);
  (void)hipFree(din);
  (void)hipFree(dout);
  return e;
}

}  // namespace mpcr
