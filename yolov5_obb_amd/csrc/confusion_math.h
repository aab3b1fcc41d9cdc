// Scalar rules of ConfusionMatrix.process_batch (utils/metrics.py:125-163 of the reference) -- plain C++ (host + device) so that
// tests/native/host_confusion.cpp can compile them with g++ and run the golden cases on the CPU.  float32 throughout, to be
// compiled with -ffp-contract=off: the IoU is box_iou's (utils/metrics.py:246-268), operation for operation.
//
// THE TIE RULE.  The reference orders the candidate pairs with `matches[:, 2].argsort()[::-1]`, numpy's
// unstable default sort: pairs of equal IoU meet its two np.unique passes in an unspecified order.  Pinned here: every argsort
// stable.  A stable ascending sort reversed puts equal IoUs in DESCENDING order of their position in torch.where's row-major
// (label, detection) list, and np.unique(return_index=True) keeps the first row of every value, so
//   1. each kept detection chooses its candidate label of highest IoU, ties to the HIGHER label index    (better_label)
//   2. each label keeps, among the detections that chose it, the one of highest IoU, ties to the HIGHER detection index
//      (winner_key: one 64-bit maximum)
// Indices are positions in the image's own label / detection lists, in the caller's order.
#pragma once
#include "obb_device.h"

namespace obb {
namespace cm {

// step 1: detections[:, 4] > conf (strict; a NaN conf fails)
OBB_HD bool keeps(float conf, float conf_thres) { return conf > conf_thres; }

// box_iou of a label box b1 and a detection box b2 (both x1 y1 x2 y2); *iou is valid when the pair is a candidate: iou > iou_thres,
// strict, NaN fails.  With a threshold >= 0 a pair without a positive intersection cannot pass (its IoU is +-0 or NaN), so the
// division is skipped for it -- most pairs of an image.
OBB_HD bool candidate(const float* b1, const float* b2, float iou_thres, float* iou) {
  const float iw = fmaxf(fminf(b1[2], b2[2]) - fmaxf(b1[0], b2[0]), 0.f);
  const float ih = fmaxf(fminf(b1[3], b2[3]) - fmaxf(b1[1], b2[1]), 0.f);
  const float inter = iw * ih;
  if (!(inter > 0.f) && iou_thres >= 0.f) return false;
  const float area1 = (b1[2] - b1[0]) * (b1[3] - b1[1]);
  const float area2 = (b2[2] - b2[0]) * (b2[3] - b2[1]);
  *iou = inter / (area1 + area2 - inter);
  return *iou > iou_thres;
}

// rule 1: candidate (iou, l) against the best so far (best_l < 0: none yet)
OBB_HD bool better_label(float iou, int l, float best_iou, int best_l) {
  return best_l < 0 || iou > best_iou || (iou == best_iou && l > best_l);
}

// rule 2: (iou, d) as one unsigned key whose maximum is "highest IoU, then higher detection index".  The float's bits are mapped
// to an order-preserving unsigned integer (sign flipped for positives, all bits for negatives), so the rule also holds for the
// negative IoUs that inverted boxes and a negative threshold can produce.  No key is 0: 0 marks a label nobody chose.
OBB_HD unsigned long long winner_key(float iou, int d) {
  uint32_t u;
  __builtin_memcpy(&u, &iou, 4);
  u ^= (u >> 31) ? 0xffffffffu : 0x80000000u;
  return ((unsigned long long)u << 32) | (uint32_t)d;
}
OBB_HD int winner_det(unsigned long long key) { return (int)(uint32_t)key; }

// .int() of a class value, or -1 when the row or column it names does not exist (outside [0, nc), NaN included)
OBB_HD int class_index(float c, int nc) { return (c > -1.0f && c < (float)nc) ? (int)c : -1; }

}  // namespace cm
}  // namespace obb
