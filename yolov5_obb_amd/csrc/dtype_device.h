// Element access in the tensor's own dtype (fp32 / fp16 / bf16) for the kernels that read the Detect head (HIP only), and the
// host-side dispatch from the C ABI's dtype code (include/obb_hip.h: OBB_DTYPE_*) to the element type.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include "obb_hip.h"
#include "bf16_bits.h"

namespace obb {

template <typename T> __device__ __forceinline__ float ld_as_float(const T* p);
template <> __device__ __forceinline__ float ld_as_float<float>(const float* p) { return *p; }
template <> __device__ __forceinline__ float ld_as_float<__half>(const __half* p) { return __half2float(*p); }
template <> __device__ __forceinline__ float ld_as_float<bf16_t>(const bf16_t* p) { return bf16_bits_to_float(p->x); }

template <typename T> __device__ __forceinline__ void st_from_float(T* p, float v);
template <> __device__ __forceinline__ void st_from_float<float>(float* p, float v) { *p = v; }
template <> __device__ __forceinline__ void st_from_float<__half>(__half* p, float v) { *p = __float2half_rn(v); }
template <> __device__ __forceinline__ void st_from_float<bf16_t>(bf16_t* p, float v) { p->x = bf16_bits_from_float(v); }

// value rounded to the tensor dtype and widened again (what an op "in the input dtype" produces)
template <typename T> __device__ __forceinline__ float round_to_dtype(float v);
template <> __device__ __forceinline__ float round_to_dtype<float>(float v) { return v; }
template <> __device__ __forceinline__ float round_to_dtype<__half>(float v) { return __half2float(__float2half_rn(v)); }
template <> __device__ __forceinline__ float round_to_dtype<bf16_t>(float v) { return bf16_bits_to_float(bf16_bits_from_float(v)); }

// the 16 bits of a value rounded to a 16-bit tensor dtype (for kernels that assemble 32-bit words of two elements)
template <typename T> __device__ __forceinline__ uint32_t bits16_from_float(float v);
template <> __device__ __forceinline__ uint32_t bits16_from_float<__half>(float v) { return (uint32_t)__half_as_ushort(__float2half_rn(v)); }
template <> __device__ __forceinline__ uint32_t bits16_from_float<bf16_t>(float v) { return (uint32_t)bf16_bits_from_float(v); }

// ---- the C ABI's dtype code.  Code 2 is reserved and refused like every unknown code.
inline bool dtype_known(int dtype) { return dtype == OBB_DTYPE_F32 || dtype == OBB_DTYPE_F16 || dtype == OBB_DTYPE_BF16; }
inline size_t dtype_size(int dtype) { return dtype == OBB_DTYPE_F32 ? 4 : 2; }

}  // namespace obb

// Runs the statement(s) once with the type name T bound to the element type of `dtype` (a code dtype_known() accepted: the
// entries check their arguments before they come here).  `return` inside the statement leaves the calling function.
#define OBB_DISPATCH_DTYPE(dtype, T, ...)                                                                                          \
  do {                                                                                                                              \
    if ((dtype) == OBB_DTYPE_F32) { using T = float; __VA_ARGS__; }                                                                 \
    else if ((dtype) == OBB_DTYPE_F16) { using T = __half; __VA_ARGS__; }                                                           \
    else { using T = ::obb::bf16_t; __VA_ARGS__; }                                                                                  \
  } while (0)
