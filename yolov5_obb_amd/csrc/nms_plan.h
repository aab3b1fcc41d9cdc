// nms_plan.h -- which path a call of the NMS drivers takes, as plain host code.  run_nms (nms_single.h) and run_nms_obb (nmsobb_impl.h)
// take a snapshot of what the decision depends on, ask plan_single_list / plan_nms_obb, and launch what the plan says: every `if`
// of a driver that chooses a path reads a field of a plan.  Pure functions of their arguments (the one reader of the environment,
// nms_env, aside): no HIP, no allocation, no global state; tests/test_nms_plan_host.py drives them without a GPU.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#include "nms_limits.h"
#include "ws_layout.h"

namespace obb {

// ---------------------------------------------------------------- call-to-call feedback of a long single list
// Per calling thread and size class (floor(log2 n)): eight pinned words the DEVICE writes when a call completes (k_finalize,
// nms_mk.h: mk_finish / mk_select_phase; kFbEnqueued alone is the host's) and the host reads, without synchronising, when the
// thread's next call of that size is set up.  Nothing but the choice of path and the number of enqueued steps depends on them; the
// result of a call does not.  -1: never written.
enum FbWord {
  kFbSteps = 0,        // steps the phase-kernel path needed, or -2 "started / handed over to the persistent kernel"
  kFbKept = 1,         // boxes the call kept
  kFbSlabs = 2,        // whether the persistent kernel found independent slabs
  kFbEnqueued = 3,     // steps the call enqueued (written by the host)
  kFbTicksPersist = 4, // 10 ns ticks from the call's first kernel to its k_finalize: persistent kernel ...
  kFbTicksMk = 5,      // ... phase kernels
  kFbKeptPersist = 6,  // the kept count that came with kFbTicksPersist ...
  kFbKeptMk = 7,       // ... with kFbTicksMk
  kFbWords = 8
};
// The words as ONE read per call saw them, before the call enqueued anything: every decision of the call uses this copy (the
// device may write the words while the call is set up; two reads of one word could disagree).
struct FbSnapshot { int w[kFbWords]; };
static inline FbSnapshot fb_snapshot(const int* words) {
  FbSnapshot s;
  for (int i = 0; i < kFbWords; i++) s.w[i] = *(const volatile int*)(words + i);
  return s;
}

// ---------------------------------------------------------------- environment switches
// One parse function per switch (const char* as getenv returns it -> value), one reader.
static inline int env_mk(const char* e) { return e ? atoi(e) : 2; }   // 0: never, 1: always, 2: by feedback
static inline int env_mk_xlds(const char* e) { return (e && (e[0] == '0' || e[0] == '1')) ? e[0] - '0' : -1; }   // 0 / 1 pins the cross probe
// OBB_NMS_SMALL_HELPERS = n pins the number of k_nms_small's helper workgroups (0: every segment stays whole); -1: not set
static inline int env_small_helpers(const char* e) { const int v = (e && *e) ? atoi(e) : -1; return v > kSmallHelpMax ? kSmallHelpMax : v; }
// OBB_NMS_SELF_SORT: 0 = always the sort kernel, 1 = self-sorting segments where no helpers would run, 2 = default:
// self-sorting segments wherever they are possible (no helpers then: the sort kernel is what hands them out)
static inline int env_self_sort(const char* e) { return (e && *e >= '0' && *e <= '2') ? *e - '0' : 2; }
static inline int env_mk_steps(const char* e) { return e ? atoi(e) : 0; }   // (measurement aid) > 0: the number of enqueued steps
// (OBB_NMS_MK_PEND: a smaller pending list, so that tests reach the overflow hand-over without two million undecided pairs)
static inline int env_mk_pend(const char* e) { const int v = e ? atoi(e) : 0; return (v > 0 && v < kMkPend1) ? v : kMkPend1; }
static inline int env_phase_prof(const char* e) { return (e && atoi(e)) ? 1 : 0; }
// Skip rules of the quad NMS (piou_device.h): bit 0 = the two exact cone rules (proved), bit 1 = the bounding-box rule (measured noise
// bound).  OBB_NMS_POLY_STRICT=1: cone rule only (every other pair is clipped); =2: no rule at all, every pair is clipped.
static inline int env_poly_strict(const char* e) { const int v = e ? atoi(e) : 0; return v == 1 ? 1 : (v >= 2 ? 0 : 3); }

struct NmsEnv {
  // read on every call: tests switch paths inside one process
  int mk;             // OBB_NMS_MK
  int mk_xlds;        // OBB_NMS_MK_XLDS
  int small_helpers;  // OBB_NMS_SMALL_HELPERS
  int self_sort;      // OBB_NMS_SELF_SORT
  // read once per process, by the first call
  int mk_steps;       // OBB_NMS_MK_STEPS
  int mk_pend;        // OBB_NMS_MK_PEND
  int phase_prof;     // OBB_NMS_PHASE_PROF
  int quad_skip;      // OBB_NMS_POLY_STRICT, as the skip-rule bits
};
static inline NmsEnv nms_env() {
  static const NmsEnv process = [] {
    NmsEnv e{};
    e.mk_steps = env_mk_steps(getenv("OBB_NMS_MK_STEPS")); e.mk_pend = env_mk_pend(getenv("OBB_NMS_MK_PEND"));
    e.phase_prof = env_phase_prof(getenv("OBB_NMS_PHASE_PROF")); e.quad_skip = env_poly_strict(getenv("OBB_NMS_POLY_STRICT"));
    return e;
  }();
  NmsEnv e = process;
  e.mk = env_mk(getenv("OBB_NMS_MK")); e.mk_xlds = env_mk_xlds(getenv("OBB_NMS_MK_XLDS"));
  e.small_helpers = env_small_helpers(getenv("OBB_NMS_SMALL_HELPERS")); e.self_sort = env_self_sort(getenv("OBB_NMS_SELF_SORT"));
  return e;
}

// ---------------------------------------------------------------- launch geometry both drivers use
// window of positions opened at a time when the caller limits the number of kept boxes (nms_core.h)
static inline int nms_window(long long max_keep) {
  if (max_keep <= 0) return 0;
  long long w = 4 * max_keep;
  if (w < 8192) w = 8192;
  if (w > (1 << 30)) w = 1 << 30;
  return (int)((w + 63) / 64 * 64);
}
// grid of the persistent launch on `cus` compute units.  n_slots: number of sorted positions that can hold a box (bounds the
// useful parallelism)
static inline int nms_grid(int64_t nseg, int64_t n_slots, int cap_first_, int cus) {
  int64_t nb = (n_slots + 511) / 512;                 // 8 waves x 64 columns per workgroup
  {                                                   // ... and one wave per tile of the first chunk's triangle
    const int64_t per_seg = (n_slots + nseg - 1) / nseg;
    const int64_t c = per_seg < cap_first_ ? per_seg : cap_first_;
    const int64_t tiles = ((c + 63) / 64) * ((c + 63) / 64 + 1) / 2 * nseg;
    if (nb < (tiles + 7) / 8) nb = (tiles + 7) / 8;
  }
  if (n_slots >= 8192) nb = cus;                      // enough work for the whole chip
  if (nb < nseg) nb = nseg;
  if (nb > cus) nb = cus;
  if (nb < 1) nb = 1;
  return (int)nb;
}

// ---------------------------------------------------------------- one list (run_nms)
// Steps of the phase-kernel path are enqueued without knowing how many the data needs (stream-ordered: nothing is read back).
// The device records the number of steps a call needed in kFbSteps; the thread's next call of that size enqueues that many.
struct SingleListPlan {
  int use_grid;     // spatial index for the cross phases (grid.h)
  int use_mk;       // the phase kernels (nms_mk.h) in front of the persistent kernel
  int use_slabs;    // the persistent kernel looks for independent slabs
  int cap_first;    // first chunk of the phase kernels (use_mk, else 0)
  int slab_cap;     // chunk capacity of a slab team (use_slabs, else 0)
  int xlds;         // cross probe from a table in LDS (use_mk)
  int steps;        // steps to enqueue (use_mk, else 0)
  int pend_cap;     // capacity of the pending list (use_mk, else 0)
};

// long lists without a limit on the kept boxes may take the phase-kernel path: such a call has feedback words
static inline bool single_list_grid(int kind, int64_t n, float thr, bool has_grid) {
  // rotated boxes, one list, conservative rejects allowed (thr >= 0)
  return kind == 0 && has_grid && thr >= 0.f && n < (1ll << 24);
}
static inline bool single_list_mk_possible(int kind, int64_t n, float thr, int64_t max_keep, bool has_grid, bool has_mk) {
  return single_list_grid(kind, n, thr, has_grid) && has_mk && n >= kMkMinN && max_keep <= 0;
}
// the per-thread call counter of a size class advances exactly when the feedback rule is asked
static inline bool mk_counts_call(const NmsEnv& env, bool have_feedback) { return env.mk != 0 && env.mk != 1 && have_feedback; }

// Which path the next call takes.  The phase kernels win where a chunk keeps many rows (thousands of objects, sparse data); the
// persistent kernel wins where two or three steps with a few hundred kept rows each do it, and where the list falls apart into
// independent slabs (class offsets: one team per slab steps concurrently).  Both report what the rule needs; the first call of a
// size class, and every 64th after it, takes the persistent kernel (it is the one that can see slabs).
// Round 6: the rule above only says where the phase kernels are WORTH TRYING.  Both paths report how long the call took on the device
// (kFbTicksPersist, kFbTicksMk: 10 ns ticks between the call's first kernel and its k_finalize), and where both are
// known the faster one is taken (S-clustered K=3000 + 18 class offsets keeps 40,000 boxes, finds no slabs -- and still runs 0.58 ms
// on the persistent kernel against 0.67 ms here); the other one is measured again every 64th call, the data may have changed.
// fb == NULL: no feedback words; k: the counter's value before this call (mk_counts_call).
static inline bool mk_choose(const NmsEnv& env, const FbSnapshot* fb, unsigned k) {
  if (env.mk == 0) return false;
  if (env.mk == 1 || fb == nullptr) return env.mk == 1;
  const int kept = fb->w[kFbKept], slab = fb->w[kFbSlabs];
  if (kept < 0 || (k & 63u) == 0u) return false;
  if (!(slab != 1 && kept >= kMkMinKept)) return false;
  const int t_persist = fb->w[kFbTicksPersist], t_mk = fb->w[kFbTicksMk];
  // a time only counts for data like the data it was measured on: the kept count it came with (kFbKeptPersist, kFbKeptMk) within a
  // quarter of the previous call's.  (bench.py switches regimes of one size class every 24 calls: K=3000 + 18 class offsets inherited
  // "phase kernels are faster" from K=3000 and stayed on them at 0.62 ms against the persistent kernel's 0.51 until the 64th call.)
  const int k_persist = fb->w[kFbKeptPersist], k_mk = fb->w[kFbKeptMk];
  auto stale = [&](int kk) { const int d = kk > kept ? kk - kept : kept - kk; return kk < 0 || d > kept / 4 + 16; };
  if (t_mk <= 0 || stale(k_mk)) return true;           // (the phase kernels have not reported on such data yet: try them)
  if (t_persist <= 0 || stale(k_persist)) return false;
  if ((k & 63u) == 32u) return t_mk >= t_persist;      // the slower one's turn
  return t_mk < t_persist;
}
// Which cross probe: the table of the kept rows in every workgroup's LDS (k_mk_cross_lds) where a step keeps a few thousand rows
// at most -- the previous call of the size class kept <= 2 passes' worth in all -- the chunk's table in global memory otherwise
// (S-uniform keeps 36,000 of 100,000: six passes over the queries would cost more than the L2 round trips they save).
// OBB_NMS_MK_XLDS = 0 / 1 pins the choice (read per call: tests run both on the same data).
static inline bool mk_cross_in_lds(const NmsEnv& env, int kept_prev) {
  if (env.mk_xlds >= 0) return env.mk_xlds == 1;
  return kept_prev >= 0 && kept_prev <= 2 * kMkXRows;
}
static inline int mk_step_count(const NmsEnv& env, const FbSnapshot* fb) {
  // (-2: the previous call of this size class was finished by the persistent kernel behind its steps: twice as many this time)
  int steps = 4;
  if (fb) {
    const int h = fb->w[kFbSteps];
    if (h >= 0) steps = h;
    else if (h == -2) { const int last = fb->w[kFbEnqueued]; steps = last > 0 ? 2 * last : 8; }
  }
  if (env.mk_steps > 0) steps = env.mk_steps;
  if (steps > 32) steps = 32;
  if (steps < 1) steps = 1;
  return steps;
}

// has_grid / has_mk: the workspace holds the spatial index / the phase kernels' blocks (carve); fb: the call's snapshot, NULL
// when the call has no feedback words; calls: the counter's value before this call
static inline SingleListPlan plan_single_list(int kind, int64_t n, float thr, int64_t max_keep, bool has_grid, bool has_mk,
                                              const FbSnapshot* fb, unsigned calls, const NmsEnv& env) {
  SingleListPlan p{};
  if (!single_list_mk_possible(kind, n, thr, max_keep, has_grid, has_mk)) fb = nullptr;   // (only such a call has feedback words)
  // spatial index for the cross phases (grid.h): rotated boxes, one list, conservative rejects allowed (thr >= 0)
  p.use_grid = single_list_grid(kind, n, thr, has_grid) ? 1 : 0;
  // long lists without a limit on the kept boxes: the phase-kernel path (nms_mk.h) -- no index of all boxes, no slab decomposition
  p.use_mk = (single_list_mk_possible(kind, n, thr, max_keep, has_grid, has_mk) && mk_choose(env, fb, calls)) ? 1 : 0;   // (mode 1: with or without words)
  p.use_slabs = (p.use_grid && !p.use_mk && max_keep <= 0) ? 1 : 0;   // (a limit on the kept boxes keeps the call one list: the windows are per list)
  const int kept_prev = fb ? fb->w[kFbKept] : -1;
  const bool sparse = kept_prev >= 0 && (int64_t)kept_prev * 8 > n;   // the previous call of the size class kept more than an eighth of its boxes
  if (p.use_mk) {
    // first chunk: 2048, or 4096 when the previous call of the size class kept more than an eighth of its boxes (sparse data: few
    // conflicts inside a chunk, the steps are what costs -- measured at 100k: S-uniform 1.05 -> 0.94 ms, S-clustered K=3000 0.54 -> 0.58).
    // (the edge list holds the worst case of kMkTile = C members; a larger chunk that outgrows it hands over to the persistent kernel)
    p.cap_first = sparse ? 4096 : 2048;
    p.xlds = mk_cross_in_lds(env, kept_prev) ? 1 : 0;
    p.steps = mk_step_count(env, fb);
    p.pend_cap = env.mk_pend;
  }
  if (p.use_slabs) {
    // chunk capacity of a slab team: 1024 measured best at 100k / 18 slabs (512: 363 us, 1024: 330, 1536: 362, 1920: 383 --
    // a team has ~14 workgroups: the pair phase grows with the square of the chunk, smaller chunks add steps)
    // Round 6: twice that when the previous call of the size class kept more than an eighth of its boxes (thousands of objects per
    // slab: few conflicts inside a chunk, the steps are what costs) -- S-clustered K=3000 + 18 class offsets (40,000 of 100,000 kept)
    // 0.579 -> 0.506 ms, while K=300 + 18 offsets (6,900 kept) would lose 0.05 ms with it.
    p.slab_cap = sparse ? 2048 : 1024;
  }
  return p;
}

// ---------------------------------------------------------------- the fused driver (run_nms_obb)
// k_nms_small's helper blocks, inside the persistent kernel's edge lists (which that path does not use)
struct SmallHelpBlocks { int *work, *seg_np, *seg_ticket; unsigned long long *part_main, *part_help; };
static inline SmallHelpBlocks small_help_layout(WsCursor& w, int helpers, int64_t nseg, int64_t n_pos) {
  SmallHelpBlocks b;
  b.work = w.take<int>((size_t)helpers);
  b.seg_np = w.take<int>((size_t)nseg); b.seg_ticket = w.take<int>((size_t)nseg);
  b.part_main = w.take<unsigned long long>((size_t)n_pos * kSmallWords);
  b.part_help = w.take<unsigned long long>((size_t)helpers * kSmallMax * kSmallWords);
  return b;
}
static inline size_t small_help_bytes(int helpers, int64_t nseg, int64_t n_pos) {
  WsCursor w(nullptr);
  small_help_layout(w, helpers, nseg, n_pos);
  return w.total();
}

// The caller's class filter (utils/general.py:835) as the bits of ClassMask (nmsobb_front.h): bit c & 63 of w[c >> 6] for every
// listed class id in 0 .. 255; ids outside that range are ignored (nc <= 256: no candidate carries them), a repeated id sets its
// bit once.  NULL or n_classes <= 0: no filter (*all = 1, no bit set).
static inline void class_mask_fill(const int32_t* classes_host, int n_classes, unsigned long long w[4], int* all) {
  *all = (classes_host == nullptr || n_classes <= 0) ? 1 : 0;
  for (int i = 0; i < 4; i++) w[i] = 0ull;
  for (int i = 0; i < n_classes && classes_host; i++) {
    const int c = classes_host[i];
    if (c >= 0 && c < 256) w[c >> 6] |= 1ull << (c & 63);
  }
}

struct ObbPlanIn {
  int64_t bs, A;
  int nc, agnostic, multi_label;
  float iou_thres, max_wh;
  int64_t n_extra;
  int64_t cap_img;           // rounded (round_cap)
  int64_t max_nms, max_det;
  int64_t expected_cand;     // the caller's word, all 64 bits
  int out_packed;
  int hw_cus, cus;           // the current device's, as the call read them once (nms_driver.h: DeviceCus; cus is capped by obb_nms_set_max_grid)
  long long ecap;            // of the nested NMS carve
  size_t sort_tmp_bytes;     // of the nested NMS carve ...
  size_t ps_scratch_bytes;   // ... and what the three-launch sort needs of it
};
struct ObbPlan {
  int ncs;                   // NMS segments per image
  int class_ok;              // one NMS segment per class where the image qualifies
  int multi_label;
  int64_t expected_cand, seg_hint;   // the two counts of the caller's word
  int small_hint;            // the previous call met short-sided boxes: run k_tiny_cross
  int lds_sort;              // the in-LDS regime (k_sort_prep_lds, or no sort launch at all: self_sort)
  int small_nms;             // k_nms_small, else the persistent kernel
  int self_sort;             // no sort launch: k_nms_small orders its segments itself
  int helpers;               // k_nms_small's helper workgroups
  int fused_out;             // the output stage runs inside k_nms_small
  int rows_per_thread;       // of k_decode
  int parts;                 // workgroups per image of k_sort_prep_lds (0: not launched)
  int plan_nb, plan_chunk;   // grid and first chunk of the persistent launch, for the planner inside k_sort_prep_lds
  int64_t max_seg;
  unsigned radix_mask;       // key bytes the radix sort orders by (0: neither it nor the three-launch sort runs)
  int psrs;                  // the three-launch sort (psrs_sort.h) instead of the radix sort
  unsigned gparts;           // k_gather_out's parts per image (0: fused_out)
  int window;                // nms_window(max_det)
  // State of the later launches that the call's first kernel zeroes (the filter kernel of a call with caller-kept counters, else
  // k_reset_state).  Every call zeroes what ITS path reads, so a call never depends on what an earlier call of another path left:
  int zero_bar;              // the persistent kernel's barrier block, which also holds the abort flag k_gather_out reads
  int zero_alive;            // the alive bitmap k_sort_prep_lds ORs its bits into (the radix-sort path clears it itself)
};

static inline ObbPlan plan_nms_obb(const ObbPlanIn& in, const NmsEnv& env) {
  ObbPlan p{};
  const int64_t bs = in.bs, cap_img = in.cap_img;
  // expected_cand: low 32 bits = the previous call's largest candidate count of an image (0: unknown), high 32 bits = its
  // largest NMS segment (0: unknown) -- both as status[1] reported them
  p.seg_hint = (in.expected_cand >> 32) & 0x1fffffff;
  p.small_hint = ((in.expected_cand >> 62) & 1) != 0;        // the previous call met short-sided boxes: run k_tiny_cross
  p.expected_cand = in.expected_cand & 0xffffffffll;
  p.ncs = in.agnostic ? 1 : in.nc;                           // NMS segments per image
  const int64_t nseg = bs * p.ncs;
  // class segmentation needs the class in 8 and the anchor index in 24 key bits
  // (iou_thres < 0: IoU = 0 > thr, boxes of different classes DO suppress each other in the reference's single list)
  p.class_ok = (!in.agnostic && in.nc > 1 && in.A + in.n_extra < (1ll << 24) && in.iou_thres >= 0.f && in.max_wh > 0.f) ? 1 : 0;
  p.multi_label = (in.multi_label && in.nc > 1) ? 1 : 0;     // :797
  p.lds_sort = p.expected_cand > 0 && p.expected_cand <= kSortLdsHint;
  // rows per workgroup: 2048 when that still gives two workgroups per CU, else 1024 / 512 (small batches, the TTA tensor)
  p.rows_per_thread = (bs * in.A >= 4LL * kDecThreads * 480) ? 4 : (bs * in.A >= 2LL * kDecThreads * 480) ? 2 : 1;
  p.max_seg = (in.max_nms > 0 && in.max_nms < cap_img) ? in.max_nms : cap_img;
  p.window = nms_window(in.max_det);
  // grid of the NMS launch (needed by the planner inside the fused kernel)
  const int nms_capmax = cap_max(nseg);
  p.plan_chunk = kCapFirst < nms_capmax ? kCapFirst : nms_capmax;
  // Which NMS kernel: one workgroup per segment, everything in LDS (nms_small.h), when the previous call's largest segment fits it
  // (class segments, the in-LDS sort, thr >= 0: its first decision stage uses the conservative bounds); else the persistent kernel.
  p.small_nms = p.lds_sort && p.class_ok && p.seg_hint > 0 && p.seg_hint <= kSmallMax && in.iou_thres >= 0.f && nseg <= 65535;
  p.plan_nb = (nseg > 1 && !p.small_nms) ? nms_grid(nseg, bs * p.max_seg, kCapFirst, in.cus) : 0;
  // k_nms_small's helper workgroups (nms_small.h: a large segment is shared by several workgroups).  A workgroup takes a whole CU
  // (160 KB of LDS), so helpers only run at once with the segments' own workgroups on the CUs the segments leave free: as many as
  // that, none for the bs16 x 16-class step whose 256 segments fill the device (measured there with 256 helpers: 0.121 -> 0.132 ms,
  // the helpers start when the first small segments are through).  Their lists and the parts' bit matrices live in the persistent
  // kernel's edge lists, which this path does not use.  OBB_NMS_SMALL_HELPERS = n pins the number (0: every segment stays whole).
  const bool self_possible = p.small_nms && !in.out_packed && (int64_t)p.ncs * kSmallMax <= cap_img && env.self_sort != 0;
  if (p.small_nms && !(self_possible && env.self_sort == 2 && env.small_helpers < 0)) {
    const int64_t free_cus = (int64_t)in.hw_cus - nseg;
    p.helpers = env.small_helpers >= 0 ? env.small_helpers : (int)(free_cus < 0 ? 0 : (free_cus > kSmallHelpMax ? kSmallHelpMax : free_cus));
  }
  if (p.helpers > 0) {
    const size_t have = (size_t)(nseg < (int64_t)in.cus ? nseg : (int64_t)in.cus) * (size_t)in.ecap * 4;   // (carve: nteams x ecap)
    if (small_help_bytes(p.helpers, nseg, bs * cap_img) > have) p.helpers = 0;
  }
  // Self-sorting segments (SmallSelfSort): no sort launch when the small-segment kernel writes the rows itself and every segment is
  // one workgroup's.  OBB_NMS_SELF_SORT=0 keeps the sort kernel (read per call: tests compare the two in one process).
  p.self_sort = self_possible && p.helpers == 0;
  if (p.lds_sort) {
    if (!p.self_sort) p.parts = (p.class_ok && p.ncs >= 8) ? 4 : 1;   // class-segment images: four workgroups each take every fourth class
  } else {
    // Several images, or one: every image spread over many workgroups (segsort.h's LSD radix sort, two launches per key byte) --
    // or, ONE large image (the TTA tensor) of up to kPsMaxN slots: the three-launch sort of psrs_sort.h over the image's
    // candidates (keys are unique: the tie word; the count lives on the device).  This branch is what an un-hinted first call of a
    // shape takes as well (the fused in-LDS path needs the previous call's largest candidate count).
    int tb = 0;
    while ((1ll << tb) < in.A * in.nc + in.n_extra + 1) tb++;           // significant bits of the tie word
    unsigned mask = 0xF0u;                                            // single-list key: score in bytes 4..7
    for (int d = 0; d < 4; d++) if (tb > d * 8) mask |= 1u << d;
    if (p.class_ok) mask = 0xFFu;                                     // + class-mode key: anchor 0..2, score 3..6, class 7
    p.radix_mask = mask;
    p.psrs = bs == 1 && cap_img <= kPsMaxN && in.sort_tmp_bytes >= in.ps_scratch_bytes;
  }
  // the output stage runs inside k_nms_small unless the caller wants packed rows (SmallGather)
  p.fused_out = p.small_nms && !in.out_packed;
  // parts per image: one up to ~2k expected candidates (the kept rows fit the kernel's LDS and 256 threads), then one per 1024
  if (!p.fused_out)
    p.gparts = p.expected_cand <= 2048 ? 1u : (unsigned)((p.expected_cand + 1023) / 1024 > 16 ? 16 : (p.expected_cand + 1023) / 1024);
  // k_nms_small with its fused output stage reads neither the barrier block nor the abort flag; self-sorting segments build their
  // alive words in LDS.  (A call that k_nms_small gives up on -- a segment too big -- is repeated by the caller with another hint:
  // the repeat's own plan takes the persistent kernel and says zero_bar.)
  p.zero_bar = (!p.small_nms || !p.fused_out) ? 1 : 0;
  p.zero_alive = (p.lds_sort && !p.self_sort) ? 1 : 0;
  return p;
}

}  // namespace obb
