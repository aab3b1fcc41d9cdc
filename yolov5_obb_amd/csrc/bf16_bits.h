// bfloat16 as 16 bits: the float <-> bf16 conversions of the kernels that read the Detect head.  Off the device they are plain
// C++ on the bit patterns, so that tests/native/host_bf16_round.cpp compiles exactly these functions with g++ and compares them
// with torch's c10::BFloat16 on the CPU (tests/test_bf16_round_host.py) before any GPU time is spent; in gfx950 device code the
// rounding is the hardware's packed conversion, and tests/test_bf16_round_gpu.py runs the same pattern set through the device
// code (tests/native/dev_bf16_round.hip) against the host function and torch.
#pragma once
#include "obb_device.h"

namespace obb {

// the element type of a torch.bfloat16 tensor: the upper 16 bits of the float with the same value
struct bf16_t { uint16_t x; };
static_assert(sizeof(bf16_t) == 2 && alignof(bf16_t) == 2, "bf16_t is the tensor element");

// float -> bf16, round to nearest even, as c10::detail::round_to_nearest_even does it: the bias 0x7FFF + (lowest kept bit)
// carries into the kept half exactly when the dropped half is above 0x8000, or equal to it with an odd kept half.  The carry
// may run through the exponent: the largest finite floats round to inf (0x7F80), subnormals round like any other value (no
// flush to zero).  +-inf have a zero dropped half and stay.  A NaN becomes the quiet NaN 0x7FC0 (adding the bias to a NaN
// whose payload lives in the dropped half would otherwise carry it to inf or, from 0xFFFFxxxx, wrap to +0).
// gfx950 has the conversion in hardware (v_cvt_pk_bf16_f32: round to nearest even, the same overflow and subnormal behaviour,
// a NaN stays a NaN and is made quiet): one instruction where the bit arithmetic is five, which the decode kernel notices --
// it rounds every element twice (the value "in the tensor dtype", then the store) and is otherwise HBM bound.
OBB_HD uint16_t bf16_bits_from_float(float v) {
#if defined(__HIP_DEVICE_COMPILE__) && defined(__gfx950__)
  return __builtin_bit_cast(uint16_t, (__bf16)v);
#else
  const uint32_t u = __builtin_bit_cast(uint32_t, v);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)0x7fc0;
  return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
#endif
}
// bf16 -> float: exact (every bf16 value, subnormals, infinities and NaN payloads included, is the float with a zero lower half)
OBB_HD float bf16_bits_to_float(uint16_t h) { return __builtin_bit_cast(float, (uint32_t)h << 16); }

}  // namespace obb
