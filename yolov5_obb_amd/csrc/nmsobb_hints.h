// nmsobb_hints.h -- the caller's side of the fused NMS driver's protocol (include/obb_hip.h: expected_cand, status, the retry cases)
// as plain host code: what a caller keeps per input shape between calls, the word it hands in, and what it does with the words
// the last kernel of a call wrote.  No HIP, no allocation, no global state: a pure function of the struct and bs + 2 words.
// Compiled into libobb_hip.so (nms.hip includes it); both bindings of this repository call it instead of restating it, and
// tests/test_nms_hints_host.py drives it without a GPU.
#pragma once
#include <stdint.h>

#include "obb_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OBB_HINTS_HOLD 8   /* calls the larger regime is held after a repeated call, see obb_nms_obb_hints_update */

void obb_nms_obb_hints_init(obb_nms_obb_hints* h) {
  // No history: assume the regime of the reference's default thresholds (a few thousand candidates per image: the in-LDS sort;
  // a few hundred boxes per image and class: the small-segment kernel).  A batch that turns out larger reports it and is run once
  // more, which the hints then select directly -- the first call of a shape is the fast path, not the slow one.
  h->cap = 0;
  h->cand = OBB_NMS_SORT_LDS_HINT;
  h->seg = 1;
  h->hold_cand = h->hold_seg = h->small_boxes = h->small_resolved = h->reserved = 0;
}

int64_t obb_nms_obb_hints_cap(const obb_nms_obb_hints* h, int64_t worst) {
  const int64_t cap = h->cap > 65536 ? h->cap : 65536;
  return worst < cap ? worst : cap;
}

int64_t obb_nms_obb_hints_word(const obb_nms_obb_hints* h) {
  return (h->cand & 0xffffffffll) | ((h->seg & 0x1fffffffll) << 32) | (h->small_boxes ? (int64_t)1 << 62 : 0);
}

int obb_nms_obb_hints_update(obb_nms_obb_hints* h, int64_t* cap_img, int64_t worst, const int64_t* out_count, int64_t bs,
                             const int64_t* status) {
  const int64_t hint = h->cand & 0xffffffffll;                         // what this call was given
  const int64_t st0 = status[0], st1 = status[1];
  const int64_t cand_max = st1 & 0xffffffffll, seg_max = (st1 >> 32) & 0x1fffffffll;
  h->small_boxes = (st1 >> 62) & 1;
  h->small_resolved = (st1 >> 61) & 1;
  if (st0 == -1) {                                                     // a segment above the small kernel's limit: nothing is valid
    h->seg = seg_max > OBB_NMS_SMALL_SEG + 1 ? seg_max : OBB_NMS_SMALL_SEG + 1;
    h->hold_seg = OBB_HINTS_HOLD;
    return OBB_HINTS_RETRY;
  }
  for (int64_t b = 0; b < bs; b++)
    if (out_count[b] < 0) return OBB_HINTS_RETRY_SMALL_GRID;           // a team barrier of the NMS kernel timed out
  if (st0 > *cap_img) {                                                // an image produced more candidates than slots
    const int64_t cap = st0 > 2 * *cap_img ? st0 : 2 * *cap_img;
    *cap_img = worst < cap ? worst : cap;
    return OBB_HINTS_RETRY;
  }
  if (hint > 0 && hint <= OBB_NMS_SORT_LDS_HINT && cand_max > OBB_NMS_SORT_LDS_MAX) {   // the hint undersold this batch: such images were left out
    h->cand = cand_max;
    h->hold_cand = OBB_HINTS_HOLD;
    return OBB_HINTS_RETRY;
  }
  h->cap = *cap_img;
  // The hints of the next call.  After a repeated call the larger regime is held for OBB_HINTS_HOLD calls unless the batch falls
  // clearly (25 %) below the limit: a stream whose batches hover around a limit does not pay the repeat on every other batch.
  if (h->hold_cand > 0 && cand_max > OBB_NMS_SORT_LDS_HINT * 3 / 4) {
    h->hold_cand--;
    h->cand = cand_max > OBB_NMS_SORT_LDS_HINT + 1 ? cand_max : OBB_NMS_SORT_LDS_HINT + 1;
  } else {
    h->hold_cand = 0;
    h->cand = cand_max;
  }
  if (h->hold_seg > 0 && (seg_max == 0 || seg_max > OBB_NMS_SMALL_SEG * 3 / 4)) {       // (0: the sort path of this call does not report it)
    h->hold_seg--;
    h->seg = seg_max > OBB_NMS_SMALL_SEG + 1 ? seg_max : OBB_NMS_SMALL_SEG + 1;
  } else {
    h->hold_seg = 0;
    h->seg = seg_max;
  }
  return OBB_HINTS_DONE;
}

#ifdef __cplusplus
}
#endif
