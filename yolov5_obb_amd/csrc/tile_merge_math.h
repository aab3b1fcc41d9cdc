// Scalar math of the in-memory tile -> full-image merge (csrc/tile_merge.h) -- plain C++ (host + device) so that tests/native can
// compile it with g++ and compare it with Python on the CPU.  Everything is double and must be compiled with -ffp-contract=off.
//
// What it restates is the text hand-off of the reference's DOTA workflow: val.py:50-66 (save_one_json) rounds a tile's
// float32 polygon to 1 decimal and its score to 5 with Python's round(), tools/TestJson2VocClassTxt.py prints them with %s,
// and DOTA_devkit/ResultMerge_multi_process.py:175-213 parses the line back with float() and moves the polygon into the source
// image with poly2origpoly.  round_dec1 / round_dec5 are float(str(round(float(v), d))), to_source is poly2origpoly.
//
// Why rint(v * 10^d) / 10^d is exact:
//   * a float32 has 24 significant bits.  Widened to double and multiplied by 10 = 2 * 5 it needs at most 24 + 3 + 1 = 28,
//     multiplied by 1e5 = 2^5 * 3125 (3125 < 2^12) at most 24 + 12 = 36: both products fit the 53 bits of a double, so the
//     multiply does not round;
//   * rint of the exact product, half to even, is therefore the integer k that CPython's round() chooses (it rounds the exact
//     binary value correctly, ties to even: Objects/floatobject.c double_round, _Py_dg_dtoa mode 3);
//   * round() returns, and str() / float() carry through the text unchanged, the double nearest to the decimal k / 10^d; 10 and
//     1e5 are exact doubles and IEEE division rounds correctly, so k / 10.0 and k / 1e5 are that double.
// The multiply must stay a multiply of its own (no FMA with anything behind it: -ffp-contract=off, and rint sits in between).
// The sign of zero survives: rint(-0.4) is -0.0 and -0.0 / 10 is -0.0, as round(-0.04, 1) is -0.0.  Infinities and NaN pass through.
#pragma once
#include "ap_math.h"
#include "obb_device.h"

namespace obb {
namespace tmm {

OBB_HD double round_dec1(float v) {
  const double k = rint((double)v * 10.0);
  return k / 10.0;
}
OBB_HD double round_dec5(float v) {
  const double k = rint((double)v * 1e5);
  return k / 1e5;
}

// poly2origpoly (ResultMerge_multi_process.py:175-182): float(v + off) / float(rate), off the tile's integer origin
OBB_HD double to_source(double v, int off, double rate) { return (v + (double)off) / rate; }

// a class id as the detections carry it (a float): an integer in [0, nc), else -1 (NaN fails every comparison)
OBB_HD int class_of(float v, int nc) {
  if (!(v >= 0.0f && v < (float)nc)) return -1;
  const int c = (int)v;
  return (float)c == v ? c : -1;
}

// The sort key of a row: segment (src_image * nc + cls) in the high word, ascending; the score in the low word, DESCENDING.
//   text rounding on:  the integer k = rint(conf * 1e5) of round_dec5, so that scores that print alike are one key.  k is
//                      clamped to +-(2^31 - 1) -- confidences beyond +-21474 share a key -- and NaN sorts first, where numpy's
//                      argsort()[::-1] puts it.
//   text rounding off: the float's order-preserving bits (apm::conf_key_desc: -0 and +0 are one value).
// Equal keys are ordered by ascending input row (tile order, then the row inside the tile) by the sort itself.
OBB_HD uint32_t score_key_text(float conf) {
  const double k = rint((double)conf * 1e5);
  if (k != k) return 0u;
  const double lim = 2147483647.0;
  const double c = k > lim ? lim : (k < -lim ? -lim : k);
  return (uint32_t)(2147483647LL - (long long)c);
}
OBB_HD uint32_t score_key(float conf, bool text_rounding) { return text_rounding ? score_key_text(conf) : apm::conf_key_desc(conf); }
OBB_HD unsigned long long sort_key(int seg, uint32_t score_key_desc) { return ((unsigned long long)(uint32_t)seg << 32) | score_key_desc; }

}  // namespace tmm
}  // namespace obb
