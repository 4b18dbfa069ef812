#!/bin/bash
# scripts/kernel_resources.sh [extra hipcc flags] — VGPR / SGPR / scratch / LDS / occupancy of the kernels (compiler remarks), of every
# unit of the library, each compiled as __graft_entry__.build_hip compiles it (hip_compile_cmd)
cd "$(dirname "$0")/.."
python3 -c '
import subprocess, sys
import __graft_entry__ as ge
for unit in ge.HIP_UNITS:
    cmd = ge.hip_compile_cmd(unit, flags=["--cuda-device-only", "-c", "-o", "/dev/null", "-Rpass-analysis=kernel-resource-usage", *sys.argv[1:]])
    sys.stdout.write(subprocess.run(cmd, stderr=subprocess.PIPE, text=True, check=True).stderr)
' "$@" | grep "remark:" | sed 's/ \[-Rpass.*//' | \
  awk '/Function Name:/{name=$NF} / VGPRs:/{v=$NF} /TotalSGPRs:/{s=$NF} /ScratchSize/{p=$NF} /Occupancy/{o=$NF} /VGPRs Spill/{sp=$NF} /LDS Size/{if (name ~ /pom_(step|step_mixed|policy|forecast|rollout|rollout_policy|expand|move_safety|reach|view_memory|imagine|deal)_kernel/) printf "%-62s vgpr %3s sgpr %3s scratch %4s vspill %3s occupancy %2s lds %6s\n", name, v, s, p, sp, o, $NF}'
