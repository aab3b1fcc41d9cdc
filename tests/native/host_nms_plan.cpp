// Serial driver of the NMS drivers' path decisions (yolov5_obb_amd/csrc/nms_plan.h), compiled with g++ for
// tests/test_nms_plan_host.py.  -DNMS_PLAN_MAIN adds a main() of its own: a stand-alone program for a sanitizer build.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <initializer_list>

#include "nms_plan.h"

namespace {
// env8: mk, mk_xlds, small_helpers, self_sort, mk_steps, mk_pend, phase_prof, quad_skip -- as the parse functions return them
obb::NmsEnv env_from(const int* e) {
  obb::NmsEnv v{};
  v.mk = e[0]; v.mk_xlds = e[1]; v.small_helpers = e[2]; v.self_sort = e[3];
  v.mk_steps = e[4]; v.mk_pend = e[5]; v.phase_prof = e[6]; v.quad_skip = e[7];
  return v;
}
}  // namespace

// which: the index of the switch in env8; s: what getenv returned (NULL: not set)
extern "C" int np_env_parse(int which, const char* s) {
  switch (which) {
    case 0: return obb::env_mk(s);
    case 1: return obb::env_mk_xlds(s);
    case 2: return obb::env_small_helpers(s);
    case 3: return obb::env_self_sort(s);
    case 4: return obb::env_mk_steps(s);
    case 5: return obb::env_mk_pend(s);
    case 6: return obb::env_phase_prof(s);
    default: return obb::env_poly_strict(s);
  }
}

// the environment as the library's one reader sees it, in env8 order
extern "C" void np_env_read(int* out8) {
  const obb::NmsEnv v = obb::nms_env();
  const int o[8] = {v.mk, v.mk_xlds, v.small_helpers, v.self_sort, v.mk_steps, v.mk_pend, v.phase_prof, v.quad_skip};
  for (int i = 0; i < 8; i++) out8[i] = o[i];
}

// words: the eight feedback words (read once, through fb_snapshot) or NULL; out8: use_grid, use_mk, use_slabs, cap_first, slab_cap,
// xlds, steps, pend_cap.  Returns whether the call advances the size class's call counter.
extern "C" int np_single(int kind, int64_t n, float thr, int64_t max_keep, int has_grid, int has_mk, const int* words, unsigned calls,
                         const int* env8, int* out8) {
  const obb::NmsEnv env = env_from(env8);
  obb::FbSnapshot snap{};
  if (words) snap = obb::fb_snapshot(words);
  const obb::SingleListPlan p = obb::plan_single_list(kind, n, thr, max_keep, has_grid != 0, has_mk != 0, words ? &snap : nullptr, calls, env);
  const int o[8] = {p.use_grid, p.use_mk, p.use_slabs, p.cap_first, p.slab_cap, p.xlds, p.steps, p.pend_cap};
  for (int i = 0; i < 8; i++) out8[i] = o[i];
  return obb::mk_counts_call(env, words != nullptr && obb::single_list_mk_possible(kind, n, thr, max_keep, has_grid != 0, has_mk != 0)) ? 1 : 0;
}

// in16: bs, A, nc, agnostic, multi_label, n_extra, cap_img, max_nms, max_det, expected_cand, out_packed, hw_cus, cus, ecap,
// sort_tmp_bytes, ps_scratch_bytes; out20: the plan's fields in the order of the struct
extern "C" void np_obb(const int64_t* in16, float iou_thres, float max_wh, const int* env8, int64_t* out20) {
  obb::ObbPlanIn in{};
  in.bs = in16[0]; in.A = in16[1]; in.nc = (int)in16[2]; in.agnostic = (int)in16[3]; in.multi_label = (int)in16[4];
  in.iou_thres = iou_thres; in.max_wh = max_wh;
  in.n_extra = in16[5]; in.cap_img = in16[6]; in.max_nms = in16[7]; in.max_det = in16[8]; in.expected_cand = in16[9];
  in.out_packed = (int)in16[10]; in.hw_cus = (int)in16[11]; in.cus = (int)in16[12]; in.ecap = in16[13];
  in.sort_tmp_bytes = (size_t)in16[14]; in.ps_scratch_bytes = (size_t)in16[15];
  const obb::ObbPlan p = obb::plan_nms_obb(in, env_from(env8));
  const int64_t o[20] = {p.ncs, p.class_ok, p.multi_label, p.expected_cand, p.seg_hint, p.small_hint, p.lds_sort, p.small_nms, p.self_sort,
                         p.helpers, p.fused_out, p.rows_per_thread, p.parts, p.plan_nb, p.plan_chunk, p.max_seg, (int64_t)p.radix_mask,
                         p.psrs, (int64_t)p.gparts, p.window};
  for (int i = 0; i < 20; i++) out20[i] = o[i];
}

extern "C" uint64_t np_help_bytes(int helpers, int64_t nseg, int64_t n_pos) { return obb::small_help_bytes(helpers, nseg, n_pos); }
// the helpers' blocks placed at `base`: offsets of work, seg_np, seg_ticket, part_main, part_help
extern "C" void np_help_place(void* base, int helpers, int64_t nseg, int64_t n_pos, uint64_t* off5) {
  obb::WsCursor w(base);
  const obb::SmallHelpBlocks b = obb::small_help_layout(w, helpers, nseg, n_pos);
  const void* p[5] = {b.work, b.seg_np, b.seg_ticket, b.part_main, b.part_help};
  for (int i = 0; i < 5; i++) off5[i] = (uint64_t)((const char*)p[i] - (const char*)base);
}
extern "C" int np_nms_grid(int64_t nseg, int64_t n_slots, int cap_first, int cus) { return obb::nms_grid(nseg, n_slots, cap_first, cus); }
extern "C" int np_nms_window(int64_t max_keep) { return obb::nms_window(max_keep); }
// the class filter's bits: out5 = w[0..3], all
extern "C" void np_class_mask(const int32_t* classes, int n_classes, uint64_t* out5) {
  unsigned long long w[4]; int all = -1;
  obb::class_mask_fill(classes, n_classes, w, &all);
  for (int i = 0; i < 4; i++) out5[i] = w[i];
  out5[4] = (uint64_t)(int64_t)all;
}

#ifdef NMS_PLAN_MAIN
// Every decision on a grid of values around its thresholds (the hand-written cases of the test lie on it), every parser on the
// test's strings, the reader on a changed environment, the helpers' blocks written to their last byte.
int main() {
  const char* strs[] = {nullptr, "", "0", "1", "2", "3", "-1", "999", "x"};
  long long sum = 0;
  for (int w = 0; w < 8; w++) for (const char* s : strs) sum += np_env_parse(w, s);
  setenv("OBB_NMS_MK", "1", 1); setenv("OBB_NMS_SMALL_HELPERS", "999", 1); setenv("OBB_NMS_SELF_SORT", "x", 1);
  int env[8];
  np_env_read(env);
  if (env[0] != 1 || env[1] != -1 || env[2] != obb::kSmallHelpMax || env[3] != 2 || env[5] != obb::kMkPend1 || env[7] != 3) { printf("nms_env is wrong\n"); return 1; }
  const int vals[] = {-2, -1, 0, 1, 4, 16, 33, 255, 256, 300, 2047, 2048, 2049, 6144, 6145, 12500, 12501, 100000};
  const int64_t ns[] = {0, 8191, 8192, 16383, 16384, 100000, (1 << 24) - 1, 1 << 24};
  int out[8];
  unsigned seed = 1;
  auto pick = [&] { seed = seed * 1664525u + 1013904223u; return vals[(seed >> 8) % (sizeof vals / sizeof *vals)]; };
  for (int kind = 0; kind < 2; kind++) for (int64_t n : ns) for (int mode = 0; mode < 3; mode++) for (unsigned calls : {0u, 1u, 32u, 64u, 96u})
    for (int rep = 0; rep < 40; rep++) {
      int words[8];
      for (int& x : words) x = pick();
      int e[8] = {mode, rep % 3 - 1, -1, 2, rep % 5 == 0 ? 40 : 0, obb::kMkPend1, 0, 3};
      sum += np_single(kind, n, rep % 7 ? 0.4f : -1.f, rep % 11 ? 0 : 300, rep % 13 != 0, rep % 17 != 0, rep % 4 ? words : nullptr, calls, e, out);
      for (int x : out) sum += x;
    }
  int64_t o20[20];
  for (int64_t bs : {1, 4, 8, 16, 4096}) for (int nc : {1, 7, 8, 16, 256}) for (int64_t cand : {0, 1700, 2048, 2049, 6144, 6145, 20000})
    for (int64_t seg : {0, 300, 384, 385}) for (int self : {0, 1, 2}) for (int helpers : {-1, 0, 7}) for (int packed : {0, 1}) {
      const int64_t nseg = bs * nc, C = obb::cap_max(nseg);
      const int64_t in16[16] = {bs, 64512, nc, 0, 1, 3, 65536 / (bs > 16 ? 64 : 1), 30000, 300, cand | (seg << 32) | ((int64_t)packed << 62), packed, 256, self ? 256 : 8,
                                helpers == 7 ? 1000 : C * (C - 1) / 2, 394496, 394496};
      const int e[8] = {2, -1, helpers, self, 0, obb::kMkPend1, 0, 3};
      np_obb(in16, packed && nc == 7 ? -0.5f : 0.45f, 4096.f, e, o20);
      for (int64_t x : o20) sum += x;
    }
  {
    const int32_t ids[] = {-1, 0, 63, 64, 127, 128, 255, 256, 1000, 63};
    uint64_t m5[5];
    np_class_mask(ids, (int)(sizeof ids / sizeof *ids), m5);
    if (m5[0] != ((1ull << 63) | 1ull) || m5[1] != ((1ull << 63) | 1ull) || m5[2] != 1ull || m5[3] != (1ull << 63) || m5[4] != 0) { printf("class mask is wrong\n"); return 1; }
    np_class_mask(nullptr, 3, m5);
    if (m5[4] != 1 || (m5[0] | m5[1] | m5[2] | m5[3])) { printf("class mask (no list) is wrong\n"); return 1; }
  }
  const int helpers = 5; const int64_t nseg = 33, n_pos = 1000;
  const uint64_t need = np_help_bytes(helpers, nseg, n_pos);
  unsigned char* base = (unsigned char*)aligned_alloc(256, need);
  uint64_t off[5];
  np_help_place(base, helpers, nseg, n_pos, off);
  const uint64_t len[5] = {(uint64_t)helpers * 4, (uint64_t)nseg * 4, (uint64_t)nseg * 4, (uint64_t)n_pos * obb::kSmallWords * 8,
                           (uint64_t)helpers * obb::kSmallMax * obb::kSmallWords * 8};
  for (int i = 0; i < 5; i++) for (uint64_t k = 0; k < len[i]; k++) base[off[i] + k] = 0x5a;   // inside the allocation, or the sanitizer says so
  const bool ok = off[4] + len[4] <= need && need % 256 == 0;
  free(base);
  printf(ok ? "nms_plan ok: checksum %lld, %llu bytes\n" : "helpers' layout is wrong (%lld, %llu bytes)\n", sum, (unsigned long long)need);
  return ok ? 0 : 1;
}
#endif
