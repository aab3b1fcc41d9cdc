// Host build of the PRODUCT's tile-merge arithmetic (yolov5_obb_amd/csrc/tile_merge_math.h) behind array drivers, so that
// tests/test_tile_merge_math_host.py can compare it with Python's round / str / float on the CPU (no GPU needed).
#include "tile_merge_math.h"

extern "C" {

void hc_round_dec(const float* v, long n, int decimals, double* out) {
  for (long i = 0; i < n; i++) out[i] = decimals == 1 ? obb::tmm::round_dec1(v[i]) : obb::tmm::round_dec5(v[i]);
}

void hc_to_source(const double* v, const int* off, long n, double rate, double* out) {
  for (long i = 0; i < n; i++) out[i] = obb::tmm::to_source(v[i], off[i], rate);
}

void hc_class_of(const float* v, long n, int nc, int* out) {
  for (long i = 0; i < n; i++) out[i] = obb::tmm::class_of(v[i], nc);
}

void hc_sort_key(const int* seg, const float* conf, long n, int text_rounding, unsigned long long* out) {
  for (long i = 0; i < n; i++) out[i] = obb::tmm::sort_key(seg[i], obb::tmm::score_key(conf[i], text_rounding != 0));
}

}  // extern "C"
