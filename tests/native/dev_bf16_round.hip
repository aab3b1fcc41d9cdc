// Device build of the float <-> bf16 element access the kernels use (yolov5_obb_amd/csrc/dtype_device.h: st_from_float,
// round_to_dtype and ld_as_float for bf16_t) as a tiny shared library of its own, so that tests/test_bf16_round_gpu.py can run
// the pattern set of tests/test_bf16_round_host.py through the gfx950 code path.  Built by yolov5_obb_amd/csrc/Makefile with the
// library's own compiler flags; not part of libobb_hip.so.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dtype_device.h"

__global__ void k_probe_round(const float* __restrict__ in, long n, uint16_t* __restrict__ stored, float* __restrict__ rounded) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  obb::st_from_float<obb::bf16_t>(reinterpret_cast<obb::bf16_t*>(stored) + i, in[i]);
  rounded[i] = obb::round_to_dtype<obb::bf16_t>(in[i]);
}
__global__ void k_probe_widen(const uint16_t* __restrict__ in, long n, float* __restrict__ out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = obb::ld_as_float<obb::bf16_t>(reinterpret_cast<const obb::bf16_t*>(in) + i);
}

extern "C" {
// device pointers; enqueued on `stream`; returns 0 or the HIP error of the launch
int probe_bf16_round(const float* in, long n, uint16_t* stored, float* rounded, void* stream) {
  if (n <= 0) return 0;
  k_probe_round<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream>>>(in, n, stored, rounded);
  return (int)hipGetLastError();
}
int probe_bf16_widen(const uint16_t* in, long n, float* out, void* stream) {
  if (n <= 0) return 0;
  k_probe_widen<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream>>>(in, n, out);
  return (int)hipGetLastError();
}
}
