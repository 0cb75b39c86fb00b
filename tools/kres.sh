#!/bin/bash
# Register / LDS / scratch usage of the rollout kernel variants (compile only,
# CPU container):  tools/kres.sh [-D...]
# "SGPRs Spill" counts scalars kept in VGPR lanes (v_writelane / v_readlane):
# they cost no scratch, so ScratchSize 0 says nothing about them;
# tools/spill_census.py counts the reloads by loop depth.
cd "$(dirname "$0")/.." || exit 1
for unit in rollout_narrow.hip rollout_wide.hip; do
/opt/rocm/bin/hipcc --offload-arch=gfx950 -c -O3 -std=c++17 -fPIC -Wno-pass-failed \
  -fno-hip-fp32-correctly-rounded-divide-sqrt -Xarch_device -freciprocal-math -Xarch_device -fapprox-func \
  -mllvm -simplifycfg-sink-common=false -Xarch_device -fno-slp-vectorize -Xarch_device -fassociative-math \
  -Xarch_device -fno-signed-zeros -Xarch_device -fno-trapping-math "$@" \
  -Rpass-analysis=kernel-resource-usage -o /tmp/kres.o manipulator_mujoco_amd/csrc/$unit 2>&1 |
  grep -A12 "Function Name: .*rollout_kernel" | grep -E "Function Name|VGPRs:|AGPRs:|ScratchSize|Occupancy|LDS Size|SGPRs:|SGPRs Spill|VGPRs Spill" |
  sed -e 's/.*remark: *//' -e 's/ \[-Rpass.*//'
done
