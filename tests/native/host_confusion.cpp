// Host build of the PRODUCT's ConfusionMatrix rules (yolov5_obb_amd/csrc/confusion_math.h): a serial driver with the phases and the
// outputs of obb_confusion_process_batch_f32, so that tests/test_confusion_host.py can run the golden cases on the CPU (no GPU
// needed).  A stand-alone program when built with -DHOST_CONFUSION_MAIN (for a sanitizer run of this file and the header).
#include <stdint.h>
#include <vector>

#include "confusion_math.h"

extern "C" {
// det6 (n, 6) [x1 y1 x2 y2 conf cls], lab5 (m, 5) [cls x1 y1 x2 y2] -> matrix[(nc + 1)^2 + 1] += counts (row-major
// [predicted][true]; the last element counts cells whose class lies outside [0, nc)).  flip: 0 the pinned tie rule; 1 the lower
// label index on ties; 2 the lower detection index on ties (what a test must be able to tell apart from 0).
int hc_confusion(const float* det6, long n, const float* lab5, long m, int nc, float conf_thres, float iou_thres, int64_t* matrix, int flip) {
  using namespace obb::cm;
  if (n <= 0 || m <= 0) return 0;                                // val.py:217-246: such an image takes no part
  std::vector<int> blab(n);
  std::vector<float> biou(n, 0.f);
  std::vector<unsigned long long> win(m, 0ull);
  bool any = false;
  for (long d = 0; d < n; d++) {
    const float* b2 = det6 + d * 6;
    int bl = keeps(b2[4], conf_thres) ? -1 : -2, brank = -1;     // rank: the index the tie compare sees (flip 1: reversed)
    float bi = 0.f;
    for (long l = 0; l < m && bl != -2; l++) {
      const int rank = (int)(flip == 1 ? m - 1 - l : l);
      float iou;
      if (candidate(lab5 + l * 5 + 1, b2, iou_thres, &iou) && better_label(iou, rank, bi, brank)) { bi = iou; bl = (int)l; brank = rank; }
    }
    blab[d] = bl; biou[d] = bi;
  }
  for (long d = 0; d < n; d++) {
    if (blab[d] < 0) continue;
    const unsigned long long key = winner_key(biou[d], flip == 2 ? (int)(n - 1 - d) : (int)d);
    if (key > win[blab[d]]) win[blab[d]] = key;
    any = true;
  }
  auto det_of = [&](unsigned long long key) { return flip == 2 ? (int)(n - 1 - winner_det(key)) : winner_det(key); };
  auto count = [&](int row, int col) {
    if (row < 0 || col < 0) matrix[(nc + 1) * (nc + 1)]++;
    else matrix[row * (nc + 1) + col]++;
  };
  for (long l = 0; l < m; l++) {
    const int lc = class_index(lab5[l * 5], nc);
    if (win[l]) count(class_index(det6[det_of(win[l]) * 6 + 5], nc), lc);
    else count(nc, lc);
  }
  if (any)
    for (long d = 0; d < n; d++) {
      if (blab[d] == -2) continue;
      if (blab[d] < 0 || det_of(win[blab[d]]) != d) count(class_index(det6[d * 6 + 5], nc), nc);
    }
  return 0;
}
}

#ifdef HOST_CONFUSION_MAIN
#include <stdio.h>
// the 3 x 3 block of equal IoUs and the out-of-range classes, checked against the cells the rules give
int main() {
  const float det[4 * 6] = {0, 0, 10, 10, .9f, 0, 0, 0, 10, 10, .8f, 1, 0, 0, 10, 10, .7f, 2, 50, 50, 60, 60, .9f, 3};
  const float lab[4 * 5] = {0, 0, 0, 10, 10, 1, 0, 0, 10, 10, 2, 0, 0, 10, 10, -1, 50, 50, 60, 60};
  int64_t mat[17] = {0};
  hc_confusion(det, 4, lab, 4, 3, 0.25f, 0.45f, mat, 0);
  const int64_t want[17] = {0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 1, 0, 1, 1, 0, 0, 1};
  for (int i = 0; i < 17; i++)
    if (mat[i] != want[i]) { printf("cell %d: %lld, expected %lld\n", i, (long long)mat[i], (long long)want[i]); return 1; }
  printf("host_confusion ok\n");
  return 0;
}
#endif
