// Serial driver of the workspace cursor (yolov5_obb_amd/csrc/ws_layout.h), compiled with g++ for tests/test_ws_layout_host.py.
// -DWS_LAYOUT_MAIN adds a main() of its own: a stand-alone program for a sanitizer build (it writes every byte of every block).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ws_layout.h"

namespace {
struct E16 { uint64_t a, b; };

void* take(obb::WsCursor& w, int64_t esize, int64_t count) {
  switch (esize) {
    case 1: return w.take<uint8_t>((size_t)count);
    case 2: return w.take<uint16_t>((size_t)count);
    case 4: return w.take<uint32_t>((size_t)count);
    case 8: return w.take<uint64_t>((size_t)count);
    case 16: return w.take<E16>((size_t)count);
    default: return w.bytes((size_t)(esize * count));           // the untyped form
  }
}
}  // namespace

// Takes (esize[i], count[i]) for i < n from a cursor over `base` (NULL: a sizing pass); the takes [nest_lo, nest_hi) go through
// nest() as a layout of their own.  ptr_out[i]: the pointer handed out; totals_out: {total(), the nested layout's total()}.
extern "C" void wl_run(void* base, const int64_t* esize, const int64_t* count, int n, int nest_lo, int nest_hi, void** ptr_out,
                       uint64_t* totals_out) {
  obb::WsCursor w(base);
  totals_out[1] = 0;
  for (int i = 0; i < n; i++) {
    if (i == nest_lo && nest_hi > nest_lo) {
      w.nest([&](void* b) {
        obb::WsCursor in(b);
        for (int k = nest_lo; k < nest_hi; k++) ptr_out[k] = take(in, esize[k], count[k]);
        return totals_out[1] = in.total();
      });
      i = nest_hi - 1;
    } else ptr_out[i] = take(w, esize[i], count[i]);
  }
  totals_out[0] = w.total();
}

extern "C" int wl_ok(const void* ws, uint64_t ws_bytes, uint64_t need) { return obb::ws_ok(ws, (size_t)ws_bytes, (size_t)need) ? 1 : 0; }
extern "C" uint64_t wl_align_up(uint64_t v) { return obb::align_up((size_t)v); }

#ifdef WS_LAYOUT_MAIN
int main() {
  const int64_t esize[] = {8, 4, 16, 1, 2, 3, 4, 8, 16, 4}, count[] = {100, 0, 1, 257, 64, 85, 1, 0, 33, 64};
  const int n = 10;
  void* p0[n]; void* p1[n];
  uint64_t t0[2], t1[2];
  wl_run(nullptr, esize, count, n, 4, 8, p0, t0);
  for (int i = 0; i < n; i++) if (p0[i]) { printf("sizing pass handed out a pointer\n"); return 1; }
  char* base = (char*)aligned_alloc(256, t0[0]);
  wl_run(base, esize, count, n, 4, 8, p1, t1);
  if (t0[0] != t1[0] || t0[1] != t1[1] || t0[0] % 256) { printf("totals differ\n"); return 1; }
  for (int i = 0; i < n; i++) memset(p1[i], 0x5a, (size_t)(esize[i] * count[i]));      // inside the allocation, or the sanitizer says so
  const int ok = wl_ok(base, t0[0], t0[0]) && !wl_ok(nullptr, t0[0], t0[0]) && !wl_ok(base + 8, t0[0], t0[0]) &&
                 !wl_ok(base + 128, t0[0], t0[0]) && !wl_ok(base, t0[0] - 1, t0[0]) && wl_ok(base, t0[0] + 1, t0[0]);
  free(base);
  printf(ok ? "ws_layout ok: %llu bytes\n" : "ws_ok is wrong (%llu bytes)\n", (unsigned long long)t0[0]);
  return ok ? 0 : 1;
}
#endif
