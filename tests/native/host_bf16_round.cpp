// Host build of the PRODUCT's float <-> bf16 conversions (yolov5_obb_amd/csrc/bf16_bits.h: the functions ld_as_float,
// st_from_float and round_to_dtype of csrc/dtype_device.h call for bf16 tensors) as a tiny shared library so that
// tests/test_bf16_round_host.py can compare them with torch's c10::BFloat16 on the CPU (no GPU needed).
#include "bf16_bits.h"
extern "C" {
// in: n float bit patterns; out: the 16 bits of each rounded to bf16
void hb_round(const uint32_t* in, long n, uint16_t* out) {
  for (long i = 0; i < n; i++) out[i] = obb::bf16_bits_from_float(__builtin_bit_cast(float, in[i]));
}
// in: n bf16 bit patterns; out: the bit patterns of the floats they widen to
void hb_widen(const uint16_t* in, long n, uint32_t* out) {
  for (long i = 0; i < n; i++) out[i] = __builtin_bit_cast(uint32_t, obb::bf16_bits_to_float(in[i]));
}
}
