#!/bin/bash
# dev tool: builds the instrumented library tools/team_timing.py and tools/esc_timing.py load (phase cycle counters compiled in).
# Always rebuilds: a timing library older than the sources misses the symbols the tools ask for (and times another build's kernels).
set -euo pipefail
cd "$(dirname "$0")/../robot-control-stack_amd/csrc"
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared \
  -Wno-unused-value -mllvm -amdgpu-sched-strategy=iterative-ilp -DRCSH_PHASE_TIMING rcs_hip.hip model.cpp episode_host.cpp -o "${1:-../rcs_amd/librcs_hip_timing.so}"
