#!/bin/bash
# Per-workgroup timeline of k_decode on the headline step: a second library built with -DOBB_DECODE_TRACE (wall-clock stamps kept in
# a __device__ buffer), the bench batch in a child process of its own.  Build (no GPU needed): tools/decode_trace.sh build
# then on the GPU box: tools/decode_trace.sh run <report.md>      (OBB_TRACE_LIB: another trace build to read)
set -o pipefail
D=$(cd "$(dirname "$0")/.." && pwd)
if [ "$1" = build ]; then
  make -s -j"${JOBS:-8}" -C "$D/yolov5_obb_amd/csrc" trace && nm -D "$D/yolov5_obb_amd/libobb_hip_trace.so" | grep -q obb_debug_decode_trace && echo built
  exit
fi
cd "$D" || exit 1
O=${2:-tools/scratch/decode_trace.md}; mkdir -p "$(dirname "$O")"
OBB_HIP_LIB=${OBB_TRACE_LIB:-$D/yolov5_obb_amd/libobb_hip_trace.so} timeout -k 10 "${TRACE_TIMEOUT:-240}" python tools/decode_trace_report.py 2>&1 | grep -v amdgpu.ids | tee "$O"
