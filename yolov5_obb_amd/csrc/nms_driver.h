// What both NMS drivers share (namespace obb): the single-list / merge drivers of nms_single.h and the fused driver of
// nmsobb_impl.h.  Per-stage timing, the score key, the workspace layout of one NMS launch (Carve), the current device's CU
// count, and the launch of the persistent kernel (nms_core.h) with the two small kernels around it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "grid.h"
#include "launch_once.h"
#include "nms_core.h"
#include "nms_limits.h"
#include "nms_mk.h"
#include "nms_plan.h"
#include "obb_device.h"
#include "obb_hip.h"
#include "psrs_sort.h"
#include "segsort.h"
#include "ws_layout.h"

namespace obb {

// ---------------------------------------------------------------- optional per-stage timing (HIP events)
// bench.py switches this on to time the dominant kernels on the stream they are launched on.
enum { PROF_DECODE = 0, PROF_SEGSORT, PROF_PREP, PROF_STEPS, PROF_GATHER, PROF_NMS_SORT, PROF_NMS_PREP, PROF_NMS_STEPS, PROF_N };
struct ProfState {
  int on = 0;          // 0 off, 1 every stage, 2 only the NMS kernels (PROF_STEPS / PROF_NMS_STEPS: the dominant kernel of a call)
  static constexpr int kMax = 8192;
  hipEvent_t ev0[kMax], ev1[kMax];
  int id[kMax];
  int created = 0, used = 0;
};
static ProfState g_prof;
struct ProfScope {
  int slot = -1; hipStream_t st;
  __attribute__((noinline)) ProfScope(int stage, hipStream_t s) : st(s) {          // (one out-of-line copy for every stage of every driver)
    if (!g_prof.on || g_prof.used >= ProfState::kMax) return;
    if (g_prof.on == 2 && stage != PROF_STEPS && stage != PROF_NMS_STEPS) return;
    slot = g_prof.used++;
    if (slot >= g_prof.created) { hipEventCreate(&g_prof.ev0[slot]); hipEventCreate(&g_prof.ev1[slot]); g_prof.created = slot + 1; }
    g_prof.id[slot] = stage;
    hipEventRecord(g_prof.ev0[slot], st);
  }
  ~ProfScope() { if (slot >= 0) hipEventRecord(g_prof.ev1[slot], st); }
};

// ---------------------------------------------------------------- small kernels
// Sort key: segments ascending, score descending, NaN first (torch's order),
// -0 == +0, ties keep ascending original index (LSD radix sort is stable) or the
// caller's explicit tie word.  Boxes flagged invalid sort last in their segment.
__device__ __forceinline__ uint32_t score_desc_key(float s) {
  uint32_t u = __float_as_uint(s);
  uint32_t k;
  if (s != s) k = 0xFFFFFFFFu;
  else {
    if (s == 0.f) u = 0u;
    k = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  }
  return ~k;
}

// min / max of four ordered ints over the workgroup (<= 1024 threads); every thread returns the result
__device__ __forceinline__ void block_minmax4(int& a0, int& a1, int& b0, int& b1, int (*s_red)[4]) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    a0 = min(a0, __shfl_xor(a0, d)); a1 = min(a1, __shfl_xor(a1, d));
    b0 = max(b0, __shfl_xor(b0, d)); b1 = max(b1, __shfl_xor(b1, d));
  }
  const int wv = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) { s_red[wv][0] = a0; s_red[wv][1] = a1; s_red[wv][2] = b0; s_red[wv][3] = b1; }
  __syncthreads();
  for (int k = 0; k < nw; k++) { a0 = min(a0, s_red[k][0]); a1 = min(a1, s_red[k][1]); b0 = max(b0, s_red[k][2]); b1 = max(b1, s_red[k][3]); }
}

// ---------------------------------------------------------------- spatial index (grid.h): counting sort by cell
// (everything except the bounding-box partials is produced inside the NMS kernel, when a step needs the index: nms_core.h grid_build)
struct GridDev {
  GridMeta* meta;              // zeroed before the launch
  int* bbpart; int nparts;     // per-block bounding boxes written by k_make_keys32
  int* cnt;                    // [M + 4] boxes per table slot (zeroed before the launch; the in-kernel build leaves zeros)
  int* start;                  // [M + 4] exclusive prefix, start[M] = total
  int* wsum;                   // [kMaxTeams] per-workgroup totals of the in-kernel scan
  float4* sorted;              // [n] {x, y, r, position}
  uint32_t* slot_of;           // [n] position -> entry of `sorted`
  uint32_t* ulist;             // [n] positions kept out of the index
  uint32_t mask;               // M - 1
  // independent slabs (grid.h; nms_core.h slab_setup): coverage bitmap + flag live in the zeroed block behind GridMeta
  uint32_t* slab_cover; int* slab_flag;
  int* slab_cnt;               // [kMaxTeams][kMaxSlabs] boxes per (workgroup, slab)
  int* slab_tot;               // [1 + kMaxTeams / 16][kMaxSlabs] totals (in the zeroed block)
  int* slab_keep;              // [kMaxSlabs] kept boxes per slab
  float4* rec2; uint32_t* order2; uint32_t* pos_old; u64* alive2; u64* kept_bits;   // the slab-major copy of the list
  size_t alive2_words, kept_words;
  SlabPlan* slab_plan;         // written by k_slab_split
};

__global__ void k_seg_from_offsets(const int32_t* __restrict__ seg_off, int nseg, int* seg_begin, int* seg_end, int* keep_cnt) {
  int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= nseg) return;
  seg_begin[g] = seg_off[g]; seg_end[g] = seg_off[g + 1];
  keep_cnt[g] = 0;
}

// num_keep[g] = -1 when the persistent kernel gave up on a barrier (abort flag): the host layer raises
// feedback != NULL (a long single list of rotated boxes): what the calling thread's NEXT call of this size class chooses its path
// by (nms_plan.h: mk_choose) -- the number of kept boxes and whether the list fell apart into independent slabs.
struct FinalizeFeedback {          // default-constructed: none
  int* feedback = nullptr; const SlabPlan* slab_plan = nullptr; int feedback_slab = 0; const u64* tstart = nullptr;
  const NmsResume* mk_ctl = nullptr; int mk_enqueued = 0;
};
__global__ void k_finalize(const int* __restrict__ keep_cnt, const int* __restrict__ seg_begin, int nseg, long long max_keep,
                           const int* __restrict__ abort_flag, int64_t* __restrict__ num_keep, int64_t* __restrict__ seg_begin_out,
                           FinalizeFeedback fb) {
  int* const feedback = fb.feedback; const SlabPlan* const slab_plan = fb.slab_plan; const int feedback_slab = fb.feedback_slab;
  const u64* const tstart = fb.tstart; const NmsResume* const mk_ctl = fb.mk_ctl; const int mk_enqueued = fb.mk_enqueued;
  int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= nseg) return;
  if (seg_begin_out) seg_begin_out[g] = seg_begin[g];
  long long c = keep_cnt[g];
  if (max_keep > 0 && c > max_keep) c = max_keep;
  num_keep[g] = (abort_flag && *abort_flag) ? -1 : c;
  if (feedback != nullptr && g == 0) {
    __hip_atomic_store(feedback + kFbKept, (int)c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    // (only a call that looked for slabs reports on them: the phase-kernel path leaves the word alone)
    if (feedback_slab) __hip_atomic_store(feedback + kFbSlabs, (slab_plan != nullptr && slab_plan->mode == 1) ? 1 : 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    // how long the call took on the device (10 ns ticks from its first kernel to this one) and which path it was
    // (a phase-kernel call that merely ran out of enqueued steps -- a stale step count from other data of this size class -- and was
    //  finished by the persistent kernel says nothing about the phase kernels' speed: its time is not recorded, the thread's next
    //  call enqueues twice the steps (hint -2) and reports then.  A call that bailed out, or had 32 steps, does report.)
    const bool starved = mk_ctl != nullptr && mk_ctl->done == 0 && mk_ctl->bail == 0 && mk_enqueued < 32;
    if (tstart != nullptr && !starved) {
      const u64 dtk = wall_clock64() - *tstart;
      __hip_atomic_store(feedback + (feedback_slab ? kFbTicksPersist : kFbTicksMk), (int)(dtk > 0x3fffffffull ? 0x3fffffffull : dtk), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      // ... and on how many kept boxes: a time measured on other data of the size class is not compared (mk_choose)
      __hip_atomic_store(feedback + (feedback_slab ? kFbKeptPersist : kFbKeptMk), (int)c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}

// ---------------------------------------------------------------- workspace (ws_layout.h)
// (chunk capacities kCapFirst / cap_max: nms_limits.h)
constexpr int kMaxTeams = 1024;     // >= number of CUs of any gfx950 part

struct Carve {
  unsigned long long *keys_a, *keys_b;
  uint32_t *vals_a, *vals_b;
  void* sort_tmp; size_t sort_tmp_bytes; uint32_t* sort_hist;
  float4* rec; u64* alive; size_t alive_bytes;
  int *seg_begin, *seg_end, *keep_cnt;
  int* bar; size_t bar_bytes;          // team barrier counters, abort flag, per-team nrows / nedges (zeroed before every launch)
  int *abort_flag, *nrows, *nedges;
  u64* prof;                           // in-kernel phase timing (OBB_NMS_PHASE_PROF=1)
  int4* plan;                          // per-workgroup team plan (k_plan_teams)
  uint32_t *rows, *edges;
  long long ecap;
  GridDev grid;                        // spatial index (rotated boxes, single list); grid.meta == NULL: not carved
  // the phase-kernel path of a long single list (nms_mk.h); mk_cidx == NULL: not carved.  Its control block mk_ctl is a block of its own.
  int* mk_ctl; uint32_t* mk_cidx; float4* mk_ent; uint16_t* mk_start; u64* mk_kbits; uint4* mk_pend1; uint8_t* mk_hasin; u64* tstart;   // mk_ctl: 1 KB (control block, edge counter at int 64)
  size_t grid_zero_bytes;              // GridMeta + slot counters: one contiguous block, zeroed before every build
  size_t total;
};

// table slots of the spatial index (power of two, multiple of 4096)
// cells of side 2 R_L / 2^fine (grid.h): 1 measured best at 100k (K=3000: 716 -> 648 us, uniform 2361 -> 2138; 2: no further gain)
constexpr int kGridFine = 1;
static uint32_t grid_slots(int64_t n) { return n >= 32768 ? 65536u : 16384u; }

// One persistent launch runs the whole step loop (nms_core.h).  Grid: one 512-thread workgroup per CU at most --
// all workgroups must be resident because they meet at team barriers; smaller problems get fewer workgroups
// (cheaper barriers).
static thread_local int g_max_grid = 0;   // obb_nms_set_max_grid: per calling thread (a retry of one thread never shrinks another thread's launches)
// The CU counts are the CURRENT device's (a process may drive differently partitioned GPUs): asked once per device; a device that
// cannot be told (dev < 0) is asked every time.
static int hw_cu_count(int dev) {
  static IntPerDevice cache;
  int cus = cache.get(dev);
  if (!cus) {
    hipDeviceProp_t p;
    if (dev >= 0 && hipGetDeviceProperties(&p, dev) == hipSuccess) cus = p.multiProcessorCount;
    if (cus < 1) cus = 1;
    if (cus > kMaxTeams) cus = kMaxTeams;
    cache.set(dev, cus);
  }
  return cus;
}
static int cu_count(int hw_cus) { return (g_max_grid > 0 && g_max_grid < hw_cus) ? g_max_grid : hw_cus; }
// What a call knows of its device: read ONCE when the call starts and handed on (carve, the planner, nms_steps, launch_persist).
struct DeviceCus {
  int dev;       // index of the current device, -1: it cannot be told
  int hw_cus;    // its compute units (at most kMaxTeams)
  int cus;       // ... capped by the calling thread's obb_nms_set_max_grid
};
static DeviceCus device_cus() {
  DeviceCus d;
  d.dev = current_device();
  d.hw_cus = hw_cu_count(d.dev);
  d.cus = cu_count(d.hw_cus);
  return d;
}

// cus: DeviceCus::cus of the call (it sizes the per-team scratch)
static Carve carve(void* base, int64_t n, int64_t nseg, int recq, int C, int cus) {
  Carve cv{};                            // (grid.meta, mk_*: NULL unless carved below)
  WsCursor w(base);
  size_t nn = (size_t)(n > 0 ? n : 1), ns = (size_t)(nseg > 0 ? nseg : 1);
  cv.keys_a = w.take<unsigned long long>(nn); cv.keys_b = w.take<unsigned long long>(nn);
  cv.vals_a = w.take<uint32_t>(nn); cv.vals_b = w.take<uint32_t>(nn);
  // scratch of the sorts: samples + cut table of the three-launch sort (psrs_sort.h), tile histograms of the radix sort (segsort.h)
  cv.sort_tmp_bytes = ps_scratch_bytes();
  cv.sort_tmp = w.bytes(cv.sort_tmp_bytes);
  cv.sort_hist = w.take<uint32_t>((((nn + kSrsTile - 1) / kSrsTile) + 1) * 256);
  cv.rec = w.take<float4>(nn * recq);
  cv.alive_bytes = (nn / 64 + 10) * 8;      // + guard words (zeroed by the prep kernels)
  cv.alive = (u64*)w.bytes(cv.alive_bytes);
  cv.bar_bytes = ((size_t)kMaxTeams * 128 + 64 + 2 * (size_t)kMaxTeams + 2 * (size_t)kBarGroups * 64) * 4;   // (+ the group counters of the two grid-wide barriers)
  cv.bar = (int*)w.bytes(cv.bar_bytes);
  if (cv.bar) { cv.abort_flag = cv.bar + (size_t)kMaxTeams * 128; cv.nrows = cv.abort_flag + 64; cv.nedges = cv.nrows + kMaxTeams; }
  cv.prof = w.take<u64>(56); cv.tstart = w.take<u64>(8); cv.plan = w.take<int4>(kMaxTeams);
  cv.seg_begin = w.take<int>(ns); cv.seg_end = w.take<int>(ns); cv.keep_cnt = w.take<int>(ns);
  // scratch that only the segment a team is working on needs: one copy per team, not per segment
  size_t nteams = ns < (size_t)cus ? ns : (size_t)cus;
  cv.rows = w.take<uint32_t>(nn + 64 * kMaxSlabs);            // (+ the padding of the slab-major layout)
  cv.ecap = (long long)C * (C - 1) / 2; if (cv.ecap < 1) cv.ecap = 1;
  cv.edges = w.take<uint32_t>(nteams * (size_t)cv.ecap);
  if (recq == RotGeom::RECQ && nseg == 1 && n >= kGridMinN) {
    const uint32_t M = grid_slots(n);
    cv.grid.mask = M - 1;
    // GridMeta, the slab words and the slot counters are consecutive blocks: one contiguous range, zeroed before every build
    const size_t zero_begin = w.total();
    cv.grid.meta = w.take<GridMeta>(1);
    cv.grid.slab_cover = w.take<uint32_t>((size_t)kSlabCopies * kSlabWords);
    static_assert((size_t)kSlabCopies * kSlabWords * 4 % kWsAlign == 0, "slab_flag follows the cover words without a gap");
    cv.grid.slab_flag = w.take<int>(16);
    cv.grid.slab_tot = w.take<int>((size_t)(1 + kMaxTeams / 16) * kMaxSlabs);   // slab totals + group totals (slab_setup)
    cv.grid_zero_bytes = w.total() - zero_begin + ((size_t)M + 4) * 4;
    cv.grid.cnt = w.take<int>((size_t)M + 4);
    cv.grid.start = w.take<int>((size_t)M + 4);
    cv.grid.wsum = w.take<int>(1024);
    cv.grid.nparts = (int)((nn + 255) / 256);
    cv.grid.bbpart = w.take<int>((size_t)cv.grid.nparts * kBbInts);
    cv.grid.sorted = w.take<float4>(nn);
    cv.grid.slot_of = w.take<uint32_t>(nn);
    cv.grid.ulist = w.take<uint32_t>(nn);
    const size_t n2 = nn + 64 * (size_t)kMaxSlabs;            // every slab starts on a 64-position boundary
    cv.grid.slab_cnt = w.take<int>((size_t)kMaxTeams * kMaxSlabs);
    cv.grid.slab_keep = w.take<int>(kMaxSlabs);
    cv.grid.rec2 = w.take<float4>(n2 * RotGeom::RECQ);
    cv.grid.order2 = w.take<uint32_t>(n2);
    cv.grid.pos_old = w.take<uint32_t>(n2);
    cv.grid.alive2_words = n2 / 64 + 10;
    cv.grid.alive2 = w.take<u64>(cv.grid.alive2_words);
    cv.grid.kept_words = nn / 64 + 2;
    cv.grid.kept_bits = w.take<u64>(cv.grid.kept_words);
    cv.grid.slab_plan = w.take<SlabPlan>(1);
    cv.mk_ctl = w.take<int>(256);
    cv.mk_cidx = w.take<uint32_t>(kMkCapMax);
    cv.mk_ent = w.take<float4>(kMkCapMax);
    cv.mk_start = w.take<uint16_t>(kMkSlots + 8);
    cv.mk_kbits = w.take<u64>(kMkCapMax / 64);
    cv.mk_hasin = w.take<uint8_t>(kMkCapMax);
    cv.mk_pend1 = w.take<uint4>(kMkPend1);
  }
  cv.total = w.total();
  return cv;
}

// the fields of a launch that are the layout's own; the caller adds order, keep_out, max_keep, window, thr, thr64 and cull
static void nms_args_from(const Carve& cv, int C, NmsArgs* a) {
  a->rec = cv.rec; a->alive = cv.alive; a->seg_begin = cv.seg_begin; a->seg_end = cv.seg_end; a->keep_cnt = cv.keep_cnt;
  a->rows = cv.rows; a->nrows = cv.nrows; a->edges = cv.edges; a->nedges = cv.nedges; a->ecap = cv.ecap; a->capmax = C;
}
// the caller's limit on the kept boxes (0: none) with its window, the threshold, and whether rejects may be culled: they predict
// IoU <= 0 or IoU <= thr; with thr < 0 even IoU == 0 suppresses
static void nms_args_limit(NmsArgs* a, int64_t max_keep, float thr) {
  a->max_keep = (int)(max_keep > 0x7fffffffLL ? 0x7fffffffLL : (max_keep < 0 ? 0 : max_keep));
  a->window = nms_window(a->max_keep);
  a->thr = thr; a->cull = (thr >= 0.f) ? 1 : 0;
}
// a call without boxes: the counts of nseg empty segments (table: the segment table is written already)
static int finalize_empty(const Carve& cv, int64_t nseg, bool table, long long max_keep, int64_t* num_keep, hipStream_t st) {
  if (!table && (hipMemsetAsync(cv.keep_cnt, 0, nseg * 4, st) != hipSuccess || hipMemsetAsync(cv.seg_begin, 0, nseg * 4, st) != hipSuccess))
    return OBB_ERR_LAUNCH;
  k_finalize<<<(unsigned)((nseg + 255) / 256), 256, 0, st>>>(cv.keep_cnt, cv.seg_begin, (int)nseg, max_keep, nullptr, num_keep, nullptr, FinalizeFeedback{});
  return hipGetLastError() == hipSuccess ? OBB_OK : OBB_ERR_LAUNCH;
}

constexpr size_t kPersistLdsMax = 159 * 1024;   // of the 160 KB per CU: exactly one workgroup per CU

template <class G, bool GRID>
static int launch_persist(const NmsArgs& a, unsigned nb, const DeviceCus& dc, hipStream_t st) {   // nb <= number of CUs (nms_grid); static teams and plans are made for that grid
  static OncePerDevice attr;
  if (!raise_lds_once_on(dc.dev, attr, kPersistLdsMax, k_nms_persist<G, GRID>)) return OBB_ERR_LAUNCH;
  // every workgroup of the launch must be resident at once (team barriers): the grid is bounded by what the occupancy
  // calculation gives for this instantiation with its largest LDS footprint -- asked once per device, not assumed
  static IntPerDevice wg_per_cu_of;
  int wg_per_cu = wg_per_cu_of.get(dc.dev);
  if (wg_per_cu < 1) {
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&wg_per_cu, (const void*)k_nms_persist<G, GRID>, kNmsThreads, kPersistLdsMax) != hipSuccess) return OBB_ERR_LAUNCH;
    if (wg_per_cu < 1) return OBB_ERR_LAUNCH;
    wg_per_cu_of.set(dc.dev, wg_per_cu);
  }
  { const long long resident = (long long)wg_per_cu * dc.hw_cus; if ((long long)nb > resident) nb = (unsigned)resident; }
  size_t lds = sizeof(WaveLds<G>) * kNmsWaves;                // pair phases: one scratch block per wave
  if (lds < (size_t)6 * a.capmax) return OBB_ERR_INTERNAL;    // (aliased by resolve: state + blocked bytes of one chunk + its ordered output list)
  lds += (size_t)a.capmax * 4;                                // + this workgroup's copy of the chunk list
  if (lds > kPersistLdsMax) return OBB_ERR_INTERNAL;
  // (a cooperative launch -- the runtime guarantees residency instead of the kernel finding out by a barrier time-out -- was
  //  measured in round 3: +18 us per call; the abort + retry with 8 workgroups stays the answer to a grid that is not resident)
  k_nms_persist<G, GRID><<<nb, kNmsThreads, lds, st>>>(a);
  return OBB_OK;
}

constexpr int kNmsBarZeroed = 1;    // the caller has zeroed the barrier block on this stream already
constexpr int kNmsPlanned = 2;      // the team plan for this launch has been written already (fused sort/prep kernel)
static int nms_steps(int kind, NmsArgs& a, const Carve& cv, int64_t nseg, int64_t n_slots, const DeviceCus& dc, hipStream_t st, int pre = 0) {
  if (!(pre & kNmsBarZeroed) && hipMemsetAsync(cv.bar, 0, cv.bar_bytes, st) != hipSuccess) return OBB_ERR_LAUNCH;
  a.bar = cv.bar; a.abort_flag = cv.abort_flag; a.nseg = (int)nseg;
  a.bar_sub = cv.nedges + kMaxTeams;                 // group counters of the grid-wide barrier, behind the per-team words
  a.cap_first = kCapFirst;
  static const int phase_prof = nms_env().phase_prof;   // (a once-per-process switch)
  a.prof = nullptr;
  if (phase_prof && a.resume == nullptr) {   // development aid: print the previous call's phase times (synchronises!)
    u64 h[56];
    if (hipMemcpy(h, cv.prof, sizeof h, hipMemcpyDeviceToHost) == hipSuccess && h[6] > 0 && h[6] < (1ull << 40)) {
      fprintf(stderr, "[nms phases, wg0, us] select %.1f pairs %.1f wait-resolve %.1f cross %.1f barrier %.1f steps %llu | resolve (any wg) %.1f rounds %llu [first round %.1f other rounds %.1f output %.1f]\n",
              h[1] * 0.01, h[2] * 0.01, h[3] * 0.01, h[5] * 0.01, h[0] * 0.01, h[6], h[9] * 0.01, h[11], h[12] * 0.01, h[13] * 0.01, h[14] * 0.01);
      fprintf(stderr, "    resolve: edges total %llu, max per chunk %llu, chunk sizes total %llu, chunks resolved from LDS %llu\n", h[25], h[27], h[28], h[26]);
      fprintf(stderr, "    pairs phase per workgroup (wave 0): longest %.1f us, sum over steps and workgroups / workgroups %.1f us; cross: longest single %.1f us\n", h[29] * 0.01, h[24] ? h[30] * 0.01 / h[24] : 0.0, h[31] * 0.01);
      fprintf(stderr, "    workgroups: %llu, busy time max %.1f us, mean %.1f us; cross phases: mean over workgroups %.1f us (sum over steps; wg0: cross + barrier = the slowest workgroup of every step)\n",
              h[24], h[22] * 0.01, h[24] ? h[23] * 0.01 / h[24] : 0.0, h[24] ? h[51] * 0.01 / h[24] : 0.0);
      fprintf(stderr, "    cross, wave 0: items %llu row-loops / scans %.1f us, stage-1 drains %llu = %.1f us | exhaustive: stage-2 drains %llu = %.1f us | indexed: per-item setup %.1f us, blocks %llu, queued pairs %llu, parts (sum over steps) %llu\n",
              h[21], h[16] * 0.01, h[19], h[17] * 0.01, h[20], h[18] * 0.01, h[18] * 0.01, h[20], h[15], h[10]);
      fprintf(stderr, "    pairs, wg0 wave 0: items %llu = %.1f us (loads %.1f), stage-1a drains %llu = %.1f us, stage-1b drains %llu = %.1f us, exact drains %llu = %.1f us | slab set-up %.1f us, merge %.1f us (wg0)\n",
              h[32], h[33] * 0.01, h[40] * 0.01, h[34], h[35] * 0.01, h[36], h[37] * 0.01, h[38], h[39] * 0.01, h[41] * 0.01, h[8] * 0.01);
      if (h[43]) fprintf(stderr, "    slab set-up (wg0): runs %.1f, count %.1f, barrier %.1f, table %.1f (copy %.1f, sums %.1f, decision %.1f), scatter %.1f + plan %.1f, barrier %.1f us\n",
                         h[42] * 0.01, h[43] * 0.01, h[44] * 0.01, (h[48] + h[49] + h[45]) * 0.01, h[48] * 0.01, h[49] * 0.01, h[45] * 0.01, h[50] * 0.01,
                         h[46] * 0.01, h[47] * 0.01);
    }
    if (hipMemsetAsync(cv.prof, 0, 56 * 8, st) != hipSuccess) return OBB_ERR_LAUNCH;
    a.prof = cv.prof;
  }
  const int nb = nms_grid(nseg, n_slots, a.cap_first, dc.cus);
  a.plan = nullptr;
  if (nseg > 1) {                                      // workgroups in proportion to the (non-empty) segments' sizes
    int c1 = a.cap_first < a.capmax ? a.cap_first : a.capmax;
    if (!(pre & kNmsPlanned)) k_plan_teams<<<1, 1024, 0, st>>>(a.seg_begin, a.seg_end, (int)nseg, (int)nb, c1, cv.plan);
    a.plan = cv.plan;
  }
  if (kind == 0 && a.gmeta != nullptr && a.slab_cover != nullptr && a.slab_plan != nullptr && nseg == 1 && a.max_keep <= 0 && a.cull != 0 &&
      a.bbpart != nullptr) {
    // independent slabs (grid.h): the set-up is a launch of its own on the persistent kernel's grid (nms_core.h: k_slab_split)
    k_slab_split<RotGeom><<<(unsigned)nb, kNmsThreads, 0, st>>>(a, const_cast<SlabPlan*>(a.slab_plan));
  } else {
    a.slab_plan = nullptr;
  }
  if (kind == 5) return launch_persist<HbbGeom64, false>(a, (unsigned)nb, dc, st);
  if (kind == 4) return launch_persist<QuadGeom64All, false>(a, (unsigned)nb, dc, st);
  if (kind == 3) return launch_persist<RotGeom64, false>(a, (unsigned)nb, dc, st);
  if (kind == 2) return launch_persist<QuadGeom64, false>(a, (unsigned)nb, dc, st);
  if (kind == 1) return launch_persist<QuadGeom, false>(a, (unsigned)nb, dc, st);
  return a.gmeta != nullptr ? launch_persist<RotGeom, true>(a, (unsigned)nb, dc, st) : launch_persist<RotGeom, false>(a, (unsigned)nb, dc, st);
}

}  // namespace obb
