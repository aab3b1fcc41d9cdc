// The float32 polygon of a detection row as val.py:226-236 builds it: corners of one rbox (utils/rboxs_utils.py:106-145), then
// scale_polys (utils/general.py:636-650).  Shared by the post-NMS tail (head.hip: k_val_post and the batch kernels) and by the
// in-memory tile merge (tile_merge.h), whose rows must carry the tail's bits.
#pragma once
#include <hip/hip_runtime.h>

namespace obb {

__device__ __forceinline__ void vt_rbox2poly(float x, float y, float w, float h, float th, float* p) {
  const float Cos = cosf(th), Sin = sinf(th);
  const float v1x = w / 2 * Cos, v1y = -w / 2 * Sin, v2x = -h / 2 * Sin, v2y = -h / 2 * Cos;
  p[0] = x + v1x + v2x; p[1] = y + v1y + v2y; p[2] = x + v1x - v2x; p[3] = y + v1y - v2y;
  p[4] = x - v1x - v2x; p[5] = y - v1y - v2y; p[6] = x - v1x + v2x; p[7] = y - v1y + v2y;
}
// scale_polys: (x - pad_x) / gain, (y - pad_y) / gain     native image space
__device__ __forceinline__ void vt_scale_poly(const float* p, float pad_x, float pad_y, float gain, float* pn) {
#pragma unroll
  for (int k = 0; k < 8; k++) pn[k] = (p[k] - ((k & 1) ? pad_y : pad_x)) / gain;
}

}  // namespace obb
