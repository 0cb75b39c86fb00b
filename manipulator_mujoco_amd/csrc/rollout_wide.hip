// rollout_wide.hip -- the dual-arm rollout kernels (rollout.hip) and
// their launches, compiled without the fast-math device flags (IEEE division /
// square root, no reassociation; manipulator_mujoco_amd/build.py): the
// latency-bound dual arm pays ~5 % and its fp32 rollouts stay within the
// scalar fp32 restatement's drift (C4 shard well-conditioned misses 22 -> 8,
// worst 4.8e-3 -> 7.8e-4).
// the dual-arm kernels read their arguments from the by-value parameter, as
// ever (kernarg.h, KA / KSA): this unit's device code stays what it was
#define MPCR_ARGS_BY_VALUE 1
#include "rollout.hip"

namespace mpcr {

// the dual-arm kernels' launches (rollout_launch's wide branch calls these)
void rollout_wide_launch(int wpc, unsigned grid, hipStream_t st, const RolloutArgs& a, const DevModel* dm,
                         const StepWArgs& stw) {
  const bool multi = a.prob_n > 0;  // several problems: the MULTI instantiations
  const bool state = has_state(a, stw);  // state blocks: the STATE instantiations (one problem or several), named last
  if (!state && wpc == 2 && multi)
    hipLaunchKernelGGL((rollout_kernel<32, 32, 72, true, 2, true>), dim3(grid), dim3(2 * WAVE), 0, st, a, dm, stw);
  else if (!state && wpc == 2)
    hipLaunchKernelGGL((rollout_kernel<32, 32, 72, true, 2>), dim3(grid), dim3(2 * WAVE), 0, st, a, dm, stw);
  else if (!state && multi)
    hipLaunchKernelGGL((rollout_kernel<32, 32, 72, true, 1, true>), dim3(grid), dim3(WAVE), 0, st, a, dm, stw);
  else if (!state)
    hipLaunchKernelGGL((rollout_kernel<32, 32, 72, true>), dim3(grid), dim3(WAVE), 0, st, a, dm, stw);
  else if (!scenarios(a) && wpc == 2)
    hipLaunchKernelGGL((rollout_kernel<32, 32, 72, true, 2, true, true>), dim3(grid), dim3(2 * WAVE), 0, st, a, dm, stw);
  else if (!scenarios(a))
    hipLaunchKernelGGL((rollout_kernel<32, 32, 72, true, 1, true, true>), dim3(grid), dim3(WAVE), 0, st, a, dm, stw);
  // scenarios (CallBlocks::nscen > 1): the SCEN instantiations, named after every other
  else if (wpc == 2)
    hipLaunchKernelGGL((rollout_kernel<32, 32, 72, true, 2 + WPCS_SCEN, true, true>), dim3(grid), dim3(2 * WAVE), 0, st, a,
                       dm, stw);
  else
    hipLaunchKernelGGL((rollout_kernel<32, 32, 72, true, 1 + WPCS_SCEN, true, true>), dim3(grid), dim3(WAVE), 0, st, a, dm, stw);
}
hipError_t rollout_wide_occupancy(int* info) {
  const void* k = reinterpret_cast<const void*>(&rollout_kernel<32, 32, 72, true>);
  int blocks = 0;
  hipFuncAttributes fa;
  hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, k, WAVE, 0);
  if (e != hipSuccess) return e;
  e = hipFuncGetAttributes(&fa, k);
  if (e != hipSuccess) return e;
  info[0] = blocks;
  info[1] = (int)fa.sharedSizeBytes;
  info[2] = fa.numRegs;
  return hipSuccess;
}

}  // namespace mpcr
