// rollout_narrow.hip -- the single-arm rollout kernels (rollout.hip), their
// launches and occupancy, and the wave-sum self-test.  Compiled with the
// fast-math device flags of manipulator_mujoco_amd/build.py (C3 is VALU-bound:
// 1.60 ms, 1.86 ms without them); the dual-arm kernels are rollout_wide.hip's,
// the launch planning over both is rollout_plan.h.
#include "rollout.hip"

namespace mpcr {

// the single-arm kernels' launches (rollout_launch's single-arm branch calls these)
void rollout_narrow_launch(int wpc, unsigned grid, hipStream_t st, const RolloutArgs& a, const DevModel* dm,
                           const StepWArgs& stw) {
  const bool multi = a.prob_n > 0;  // several problems: the MULTI instantiations
  // (the STATE instantiations last: the code object lays the kernels out
  // in the order this chain names them, and the others keep their places)
  const bool state = has_state(a, stw);  // state blocks: the STATE instantiations (one problem or several)
  if (!state && wpc == 2 && multi)
    hipLaunchKernelGGL((rollout_kernel<16, 16, 24, false, 2, true>), dim3(grid), dim3(2 * WAVE), 0, st, a, dm, stw);
  else if (!state && wpc == 2)
    hipLaunchKernelGGL((rollout_kernel<16, 16, 24, false, 2>), dim3(grid), dim3(2 * WAVE), 0, st, a, dm, stw);
  else if (!state && multi)
    hipLaunchKernelGGL((rollout_kernel<16, 16, 24, false, 1, true>), dim3(grid), dim3(WAVE), 0, st, a, dm, stw);
  else if (!state)
    hipLaunchKernelGGL((rollout_kernel<16, 16, 24, false>), dim3(grid), dim3(WAVE), 0, st, a, dm, stw);
  else if (!scenarios(a) && wpc == 2)
    hipLaunchKernelGGL((rollout_kernel<16, 16, 24, false, 2, true, true>), dim3(grid), dim3(2 * WAVE), 0, st, a, dm, stw);
  else if (!scenarios(a))
    hipLaunchKernelGGL((rollout_kernel<16, 16, 24, false, 1, true, true>), dim3(grid), dim3(WAVE), 0, st, a, dm, stw);
  // (scenarios: the SCEN instantiations, after every other for the same reason)
  else if (wpc == 2)
    hipLaunchKernelGGL((rollout_kernel<16, 16, 24, false, 2 + WPCS_SCEN, true, true>), dim3(grid), dim3(2 * WAVE), 0, st, a,
                       dm, stw);
  else
    hipLaunchKernelGGL((rollout_kernel<16, 16, 24, false, 1 + WPCS_SCEN, true, true>), dim3(grid), dim3(WAVE), 0, st, a, dm, stw);
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

// mpcr_selftest_reduce: every wave-sum form of wave.h on caller-given
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
