// wave.h -- wave-level helpers of the rollout device code (rollout.hip): address-space
// assumptions, wave sums on DPP, ballot scans, the phase barrier.
#pragma once
#include <hip/hip_runtime.h>

#include "mpcr_device.h"

namespace mpcr {

// ---------------------------------------------------------------------------
// wave helpers

// Address spaces at the entry of a non-inlined device function: its pointer
// arguments are generic, so without these the model reads, the LDS image and
// the caller's contact arrays all go through flat instructions (which also
// count against the LDS wait counter)
// (device pass only: the host pass parses device bodies with other builtin signatures)
#if defined(__HIP_DEVICE_COMPILE__)
#define ASSUME_GLOBAL(p) __builtin_assume(!__builtin_amdgcn_is_shared((const void*)(p)) && \
                                          !__builtin_amdgcn_is_private((const void*)(p)))
#define ASSUME_LDS(p) __builtin_assume(__builtin_amdgcn_is_shared((const void*)(p)))
#define ASSUME_PRIVATE(p) __builtin_assume(__builtin_amdgcn_is_private((const void*)(p)))
#else
#define ASSUME_GLOBAL(p)
#define ASSUME_LDS(p)
#define ASSUME_PRIVATE(p)
#endif
// the model pointer as a wave-uniform (SGPR) global pointer: a non-inlined
// function receives it in VGPRs, and its field reads then become per-lane
// vector loads instead of scalar ones
__device__ __forceinline__ const MPCR_GMEM DevModel* uniform_model(const DevModel* p) {
  const unsigned long long a = reinterpret_cast<unsigned long long>(p);
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)a), hi = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32));
  return reinterpret_cast<const MPCR_GMEM DevModel*>(((unsigned long long)hi << 32) | lo);
}

__device__ __forceinline__ float rdlane(float v, int l) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}
template <int CTRL>
__device__ __forceinline__ float dppf(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}
// full-wave sum, result uniform: DPP inside each 16-lane row (quad_perm
// [1,0,3,2], [2,3,0,1], row_ror:4, row_ror:8), then the GCN row_bcast:15 /
// row_bcast:31 steps carry the row sums into lane 63, one readlane.  No LDS
// traffic (a __shfl_xor butterfly is 6 dependent ds_bpermute round trips).
template <int CTRL, int ROWS>
__device__ __forceinline__ float dppf_rows(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, ROWS, 0xF, false));
}
// the reference form, every step a builtin: the compiler folds the in-row
// steps into v_add_f32_dpp but leaves each cross-row step as v_mov (old = 0),
// v_mov_b32_dpp, v_add_f32 -- 11 VALU.  Kept for mpcr_selftest_reduce, which
// holds every production form below to its bits.
__device__ __forceinline__ float wsum_ref(float v) {
  v += dppf<0xB1>(v);
  v += dppf<0x4E>(v);
  v += dppf<0x124>(v);
  v += dppf<0x128>(v);
  v += dppf_rows<0x142, 0xA>(v);  // row_bcast:15 into rows 1, 3
  v += dppf_rows<0x143, 0xC>(v);  // row_bcast:31 into rows 2, 3
  return rdlane(v, 63);
}
// the four in-row steps: lane 15 of each row ends with its row's sum
__device__ __forceinline__ float wsum_row(float v) {
  v += dppf<0xB1>(v);
  v += dppf<0x4E>(v);
  v += dppf<0x124>(v);
  v += dppf<0x128>(v);
  return v;
}
// The cross-row steps as one v_add_f32_dpp each (the rows a step does not
// write keep their value where the reference adds 0 to it; only lane 63 is
// read, and it sees the same sums in the same order): 7 VALU.  The hazard
// recogniser does not look inside the string, so the two wait states between a
// VALU write and a DPP read of the same register stand in it, and the one
// ahead of the caller's v_readlane closes it.  wsum2 / wsum3 reduce
// independent values side by side, each in its own six-step order: the other
// values' adds stand where the s_nop would.
#define MPCR_DPP15 " row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
#define MPCR_DPP31 " row_bcast:31 row_mask:0xc bank_mask:0xf\n\t"
__device__ __forceinline__ float wsum(float v) {
  v = wsum_row(v);
  asm("s_nop 1\n\t"
      "v_add_f32_dpp %0, %0, %0" MPCR_DPP15
      "s_nop 1\n\t"
      "v_add_f32_dpp %0, %0, %0" MPCR_DPP31
      "s_nop 0"
      : "+v"(v));
  return rdlane(v, 63);
}
__device__ __forceinline__ void wsum2(float& a, float& b) {
  a = wsum_row(a);
  b = wsum_row(b);
  asm("s_nop 1\n\t"
      "v_add_f32_dpp %0, %0, %0" MPCR_DPP15
      "v_add_f32_dpp %1, %1, %1" MPCR_DPP15
      "s_nop 0\n\t"
      "v_add_f32_dpp %0, %0, %0" MPCR_DPP31
      "v_add_f32_dpp %1, %1, %1" MPCR_DPP31
      "s_nop 0"
      : "+v"(a), "+v"(b));
  a = rdlane(a, 63);
  b = rdlane(b, 63);
}
__device__ __forceinline__ void wsum3(float& a, float& b, float& c) {
  a = wsum_row(a);
  b = wsum_row(b);
  c = wsum_row(c);
  asm("s_nop 1\n\t"
      "v_add_f32_dpp %0, %0, %0" MPCR_DPP15
      "v_add_f32_dpp %1, %1, %1" MPCR_DPP15
      "v_add_f32_dpp %2, %2, %2" MPCR_DPP15
      "v_add_f32_dpp %0, %0, %0" MPCR_DPP31
      "v_add_f32_dpp %1, %1, %1" MPCR_DPP31
      "v_add_f32_dpp %2, %2, %2" MPCR_DPP31
      "s_nop 0"
      : "+v"(a), "+v"(b), "+v"(c));
  a = rdlane(a, 63);
  b = rdlane(b, 63);
  c = rdlane(c, 63);
}
// Sum of a value that is +0 in every lane from W on (W = 16: one row, the
// in-row steps alone; W = 32: two rows, the row_bcast:15 step joins them):
// the steps left out add +0 in the reference.  Its one visible effect, -0
// becoming +0 (a row whose lanes are all -0), is restored on the scalar unit,
// so the value is wsum's bit for bit.  5 VALU (W = 16), 6 (W = 32).
template <int W>
__device__ __forceinline__ float wsum_lo(float v) {
  static_assert(W == 16 || W == 32, "one or two rows");
  v = wsum_row(v);
  if constexpr (W == 32)
    asm("s_nop 1\n\t"
        "v_add_f32_dpp %0, %0, %0" MPCR_DPP15
        "s_nop 0"
        : "+v"(v));
  const unsigned u = (unsigned)__builtin_amdgcn_readlane(__float_as_int(v), W - 1);
  return __uint_as_float(u == 0x80000000u ? 0u : u);
}
__device__ __forceinline__ int lanes_below(unsigned long long mask) {
  return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
}
// exclusive prefix sum of small per-lane counts (0 .. 2^BITS - 1) by bit-plane ballots
template <int BITS = 3>
__device__ __forceinline__ int wscan_excl(int v, int& total) {
  int pre = 0, tot = 0;
#pragma unroll
  for (int bit = 0; bit < BITS; bit++) {
    const unsigned long long mk = __ballot((v >> bit) & 1);
    pre += lanes_below(mk) << bit;
    tot += __popcll(mk) << bit;
  }
  total = tot;
  return pre;
}
// Phase barrier of one candidate's wave: orders its lanes' LDS / global
// accesses (the workgroup-scope fences of __syncthreads, without s_barrier).
// A one-wave workgroup measured the same with either (1.963 vs 1.964 ms on C3);
// the two-wave variant (WPC = 2) needs the wave-local form, its waves meet at
// block_sync() only.
__device__ __forceinline__ void sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
__device__ __forceinline__ void block_sync() { __syncthreads(); }
// __shfl behind a forceinline wrapper, for the kinematics' ancestor reads and
// the constraint-row count: inlined with the kernel's other helpers, ahead of
// the optimiser (called directly there, __shfl is inlined later and the
// source-lane mask of a lane known to be in range is no longer folded away)
template <class T>
__device__ __forceinline__ T wshfl(T x, int src) { return __shfl(x, src); }

}  // namespace mpcr
