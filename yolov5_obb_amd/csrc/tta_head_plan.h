// tta_head_plan.h -- the entry table of obb_non_max_suppression_obb_tta_head, as plain host code: the argument checks of the entry
// and the table its front kernel (nms_head.h: k_decode_head<T, true>) takes as a kernel argument.  No HIP, no allocation, no global
// state; tests/test_lazy_tta_host.py drives it without a GPU (tests/native/host_tta_head_plan.cpp), like nms_plan.h / ws_layout.h.
//
// One entry per surviving (pass, level) of augmented inference, in the order torch.cat(_clip_augmented(y), 1) lays their rows out
// (models/yolo.py:149-209; tta_plan of this package's models/yolo.py): pass after pass, level after level.
#pragma once
#include <cmath>
#include <stdint.h>

#include "obb_hip.h"

namespace obb {

constexpr int kHeadTtaMaxEntries = OBB_TTA_MAX_PASSES * OBB_DETECT_MAX_LEVELS;   // 16
constexpr int kHeadTileBytes = 256;        // a tile is one 256-byte line of positions per channel (nms_head.h: kHeadTile<T>)

// HeadFront (nms_head.h) over (pass, level) entries; the fields the two share have the same names.  About 1.9 KB of kernel arguments.
struct HeadFrontTta {
  const void* in[kHeadTtaMaxEntries];      // conv output of the entry: (bs, na*no, ny, nx), contiguous
  long long a_off[kHeadTtaMaxEntries];     // first row of the entry in the concatenated z (the rows of the entries before)
  int ny[kHeadTtaMaxEntries], nx[kHeadTtaMaxEntries];
  int tile_end[kHeadTtaMaxEntries];        // running sum of the entries' tile counts
  float stride[kHeadTtaMaxEntries];
  float anchor_px[kHeadTtaMaxEntries][OBB_LOSS_MAX_ANCHORS][2];
  float inv_scale[kHeadTtaMaxEntries];     // (float)(1.0 / scale) of the entry's pass: what torch's `/= python_float` multiplies with
  float img_w[kHeadTtaMaxEntries], img_h[kHeadTtaMaxEntries];
  int flip[kHeadTtaMaxEntries];            // 0, 2 (up-down) or 3 (left-right)
  // bytes per load of the entry's channel lines: 16 or 8 when every channel plane of the entry starts on such a boundary (the
  // conv output does and ny*nx elements are a multiple of it), 0 = element-wise.  Per entry: one odd map costs the others nothing.
  int vec[kHeadTtaMaxEntries];
  int nl, na;                              // nl: the number of entries
};

inline int head_tta_elem_size(int dtype) {
  return dtype == OBB_DTYPE_F32 ? 4 : (dtype == OBB_DTYPE_F16 || dtype == OBB_DTYPE_BF16) ? 2 : 0;
}

// Checks the arguments and fills *h.  OBB_ERR_BAD_ARG for: npass outside 1..OBB_TTA_MAX_PASSES, a pass's nl outside
// 1..OBB_DETECT_MAX_LEVELS, a flip other than 0 / 2 / 3, a scale <= 0 or not finite, an image size < 1, NULL passes or a NULL listed
// conv_out, a map size < 1, bs < 1, na outside 1..OBB_LOSS_MAX_ANCHORS, nc = no - 185 outside 1..256, an unknown dtype,
// bs * na > 65535 (grid.y), a_total smaller than the rows listed, a_total * nc past the 32-bit row field of the sort key, more
// tiles than grid.x holds.  *rows_out (may be NULL): the rows listed.
inline int head_tta_build(int npass, const obb_tta_pass* passes, int dtype, int64_t bs, int64_t na, int64_t no, int64_t a_total,
                          HeadFrontTta* h, int64_t* rows_out) {
  const int64_t nc = no - 5 - 180;
  const int esz = head_tta_elem_size(dtype);
  if (!h || npass < 1 || npass > OBB_TTA_MAX_PASSES || !passes || bs < 1 || na < 1 || na > OBB_LOSS_MAX_ANCHORS || nc < 1 || nc > 256 ||
      esz == 0 || bs * na > 65535 || a_total < 1)
    return OBB_ERR_BAD_ARG;
  // the key's low word holds row * nc + class (nms_head.h); run_nms_obb keeps the label rows (n_extra) inside it as well
  if (a_total > 0xffffffffLL / nc) return OBB_ERR_BAD_ARG;
  const int TP = kHeadTileBytes / esz;
  int n = 0;
  int64_t rows = 0, tiles = 0;
  for (int p = 0; p < npass; p++) {
    const obb_tta_pass& ps = passes[p];
    if (ps.nl < 1 || ps.nl > OBB_DETECT_MAX_LEVELS || (ps.flip != 0 && ps.flip != 2 && ps.flip != 3) || !(ps.scale > 0.0) ||
        !std::isfinite(ps.scale) || ps.img_h < 1 || ps.img_w < 1)
      return OBB_ERR_BAD_ARG;
    for (int l = 0; l < ps.nl; l++, n++) {
      if (!ps.conv_out[l] || ps.ny[l] < 1 || ps.nx[l] < 1 || ps.ny[l] > 0x7fffffffLL || ps.nx[l] > 0x7fffffffLL ||
          ps.ny[l] * ps.nx[l] > 0x7fffffffLL / (na * no))
        return OBB_ERR_BAD_ARG;
      const int64_t HW = ps.ny[l] * ps.nx[l];
      h->in[n] = ps.conv_out[l]; h->ny[n] = (int)ps.ny[l]; h->nx[n] = (int)ps.nx[l]; h->a_off[n] = rows; h->stride[n] = ps.stride[l];
      for (int a = 0; a < OBB_LOSS_MAX_ANCHORS; a++) {
        h->anchor_px[n][a][0] = a < na ? ps.anchors_px[l][a][0] : 0.f;
        h->anchor_px[n][a][1] = a < na ? ps.anchors_px[l][a][1] : 0.f;
      }
      h->inv_scale[n] = (float)(1.0 / ps.scale);
      h->flip[n] = ps.flip; h->img_w[n] = (float)ps.img_w; h->img_h[n] = (float)ps.img_h;
      const uintptr_t base = (uintptr_t)ps.conv_out[l];
      const int64_t plane = HW * esz;
      h->vec[n] = ((base | (uintptr_t)plane) & 15) == 0 ? 16 : ((base | (uintptr_t)plane) & 7) == 0 ? 8 : 0;
      tiles += (HW + TP - 1) / TP;
      if (tiles > 0x7fffffffLL) return OBB_ERR_BAD_ARG;
      h->tile_end[n] = (int)tiles;
      rows += na * HW;
      if (rows > a_total) return OBB_ERR_BAD_ARG;         // more rows listed than the concatenation has
    }
  }
  h->nl = n; h->na = (int)na;
  for (int k = n; k < kHeadTtaMaxEntries; k++) {
    h->in[k] = nullptr; h->ny[k] = h->nx[k] = 0; h->a_off[k] = rows; h->tile_end[k] = (int)tiles; h->stride[k] = 0.f;
    for (int a = 0; a < OBB_LOSS_MAX_ANCHORS; a++) h->anchor_px[k][a][0] = h->anchor_px[k][a][1] = 0.f;
    h->inv_scale[k] = 1.f; h->flip[k] = 0; h->img_w[k] = h->img_h[k] = 0.f; h->vec[k] = 0;
  }
  if (rows_out) *rows_out = rows;
  return OBB_OK;
}

}  // namespace obb
