// Per-element decode of the Detect head (models/yolo.py:71-74), shared by the Detect decode kernels (head.hip) and the NMS front
// kernel that reads the conv outputs directly (nms_head.h): both must produce the same bits for every element.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include "dtype_device.h"
#include "loss_math.h"

namespace obb {

// y = x.sigmoid() in the tensor dtype, then (models/yolo.py:71-74, inplace branch)
//   xy = (y*2 - 0.5 + grid) * stride     y*2 and -0.5 in the tensor dtype; grid is a float32 tensor -> fp32 from there
//   wh = (y*2)**2 * anchor_grid          (y*2)**2 in the tensor dtype; anchor_grid is float32 -> fp32 product
// and the result is rounded to the tensor dtype by the slice assignment.
// sigmoid in the precision the comparison with the reference allows: fp32 tensors get the correctly rounded expf and
// division; fp16 tensors are rounded to 11 bits right after, so the hardware exp2 / reciprocal (1 ulp of fp32 each) can
// only move a result that sits within 2^-12 relative of an fp16 rounding boundary -- the same 1-ulp-of-fp16 freedom the
// reference's own libm has (tests/test_head_gpu.py states the tolerance)
template <typename T> __device__ __forceinline__ float detect_sigmoid(float x) { return sigmoid_f(x); }
template <> __device__ __forceinline__ float detect_sigmoid<__half>(float x) {
  return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.44269504088896341f * x));
}
// bf16 tensors: the same hardware pair, deliberately.  The result is rounded to 8 significand bits right after, so the pair's
// error (the product's rounding, 1 ulp of fp32 each for exp2 and the reciprocal: about 2^-22 relative in all) can only move
// a result that sits within that distance of a bf16 rounding boundary, where the spacing is 2^-8 relative -- fewer than one
// element in ten thousand, and then by one bf16 step, the freedom the reference's own libm has against a correctly rounded
// sigmoid.  The correctly rounded expf and division of the fp32 path would buy nothing that survives the rounding
// (tests/test_bf16_head_gpu.py caps the elements off the reference's rounding at 1 % and at one step).
template <> __device__ __forceinline__ float detect_sigmoid<bf16_t>(float x) {
  return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.44269504088896341f * x));
}

template <typename T>
__device__ __forceinline__ float detect_decode_one(float raw, int ch, float gx, float gy, float stride, float aw, float ah) {
  const float y = round_to_dtype<T>(detect_sigmoid<T>(raw));
  if (ch >= 4) return y;
  const float t = round_to_dtype<T>(y * 2.0f);
  if (ch < 2) {
    const float u = round_to_dtype<T>(t - 0.5f);
    return round_to_dtype<T>((u + (ch == 0 ? gx : gy)) * stride);
  }
  const float q = round_to_dtype<T>(t * t);
  return round_to_dtype<T>(q * (ch == 2 ? aw : ah));
}

// Augmented inference (models/yolo.py:183-198 _descale_pred, in-place branch) on a decoded box channel ch < 4, every step rounded
// to the tensor dtype like the torch op it stands for:
//   p[..., :4] /= scale          torch divides by a Python scalar as a multiplication with 1 / scale, the reciprocal taken once in
//                                DOUBLE and rounded to fp32 (inv_scale, computed on the host; scale == 1 is the identity)
//   p[..., 0] = img_w - p[..., 0]   flip 3 (left-right)          p[..., 1] = img_h - p[..., 1]   flip 2 (up-down)
// the subtraction in fp32 on the integer image size.
template <typename T>
__device__ __forceinline__ float detect_descale_one(float v, int ch, float inv_scale, int flip, float img_w, float img_h) {
  v = round_to_dtype<T>(v * inv_scale);
  if (flip == 3 && ch == 0) v = round_to_dtype<T>(img_w - v);
  if (flip == 2 && ch == 1) v = round_to_dtype<T>(img_h - v);
  return v;
}

}  // namespace obb
