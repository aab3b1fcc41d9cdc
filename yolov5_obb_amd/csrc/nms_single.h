// The single-list and merge side of the NMS unit (namespace obb): rotated / quad NMS of one list (run_nms, run_nms_rot64) and the
// tile -> full-image merge NMS (run_merge_nms), with their key, sort and record kernels.  The C entries are in nms.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "geom.h"
#include "grid.h"
#include "launch_once.h"
#include "nms_core.h"
#include "nms_driver.h"
#include "nms_limits.h"
#include "nms_mk.h"
#include "nms_plan.h"
#include "obb_device.h"
#include "obb_hip.h"
#include "psrs_sort.h"
#include "segsort.h"

namespace obb {

// Single list: the runs of the sort (psrs_sort.h) straight from the scores -- key = descending-score bits in the high word,
// original index in the low word (unique: ties keep ascending index, the documented rule) -- plus everything the old key
// kernel did on the side: the single segment's table, the zeroing of the team-barrier block and of the index / slab block,
// and the bounding-box partial of the block's boxes (one per run) for the spatial index.
struct LocalExtras {
  int *seg_begin, *seg_end, *keep_cnt;
  uint4* bar16; long long n_bar16;
  uint4* grid16; long long n_grid16;
  uint4* mk16; long long n_mk16;   // control block of the phase-kernel path (nms_mk.h)
  int* bbpart;                 // [runs][kBbInts] or NULL
  u64* tstart;                 // optional: the device's wall clock when the call's first kernel runs (k_finalize reports the call's duration)
};
__device__ __forceinline__ void local_extras(const LocalExtras& x, const float* __restrict__ dets5, int drop_small, int n, int i, bool in_range,
                                             int (*s_red)[4], uint32_t* key_out) {
  if (i == 0) { x.seg_begin[0] = 0; x.seg_end[0] = n; x.keep_cnt[0] = 0; if (x.tstart) *x.tstart = wall_clock64(); }
  for (long long k = i; k < x.n_bar16; k += (long long)gridDim.x * blockDim.x) x.bar16[k] = make_uint4(0u, 0u, 0u, 0u);
  for (long long k = i; k < x.n_grid16; k += (long long)gridDim.x * blockDim.x) x.grid16[k] = make_uint4(0u, 0u, 0u, 0u);   // GridMeta + slot counters
  for (long long k = i; k < x.n_mk16; k += (long long)gridDim.x * blockDim.x) x.mk16[k] = make_uint4(0u, 0u, 0u, 0u);
  int bx0 = 0x7fffffff, by0 = 0x7fffffff, bx1 = (int)0x80000000, by1 = (int)0x80000000;
  int d2 = 0;                                          // largest w^2 + h^2 of the block, as float bits (>= 0: ordered like ints)
  float rsum = 0.f; int rcnt = 0;
  if (in_range) {
    bool ok = true;
    float w = 0.f, h = 0.f;
    if (drop_small || x.bbpart != nullptr) { w = dets5[(size_t)i * 5 + 2]; h = dets5[(size_t)i * 5 + 3]; }
    if (drop_small) {
      // nms_rotated_wrapper.py:32  too_small = dets[:, [2, 3]].min(1)[0] < 0.001   (NaN in either side: kept, obb_device.h)
      if (box_too_small(w, h)) { *key_out = 0xFFFFFFFFu; ok = false; }
    }
    if (x.bbpart != nullptr && ok) {
      // bounding box of the finite centres of the boxes that take part: the extent of the data for the spatial index
      // (grid.h), one partial per block, reduced by the blocks of the prep kernel (no atomics)
      const float cx = dets5[(size_t)i * 5], cy = dets5[(size_t)i * 5 + 1];
      if ((cx - cx == 0.f) && (cy - cy == 0.f)) { bx0 = bx1 = grid_f2o(cx); by0 = by1 = grid_f2o(cy); }
      const float q = w * w + h * h;
      if (q - q == 0.f) { d2 = __float_as_int(q); rsum = sqrtf(q); rcnt = 1; }
    }
  }
  if (x.bbpart != nullptr) {
    int d2b = d2, dummy = d2;
    block_minmax4(bx0, by0, bx1, by1, s_red);
    { int lo0 = 0x7fffffff, lo1 = 0x7fffffff; block_minmax4(lo0, lo1, d2b, dummy, s_red); }
    // (nms_mk.h: the mean diagonal of the finite boxes, for the radius limit of its tables -- a heuristic, any order of summation will do)
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { rsum += __shfl_xor(rsum, d); rcnt += __shfl_xor(rcnt, d); }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { s_red[threadIdx.x >> 6][0] = __float_as_int(rsum); s_red[threadIdx.x >> 6][1] = rcnt; }
    __syncthreads();
    if (threadIdx.x == 0) {
      float rs = 0.f; int rc = 0;
      for (int k = 0; k < (int)((blockDim.x + 63) >> 6); k++) { rs += __int_as_float(s_red[k][0]); rc += s_red[k][1]; }
      int* o = x.bbpart + (size_t)blockIdx.x * kBbInts;
      o[0] = bx0; o[1] = by0; o[2] = bx1; o[3] = by1; o[4] = d2b; o[5] = __float_as_int(rs); o[6] = rc; o[7] = 0;
    }
  }
}
__global__ __launch_bounds__(kPsRun) void k_ps_local_scores(PsBuf b, const float* __restrict__ scores, int score_stride,
                                                            const float* __restrict__ dets5, int drop_small, LocalExtras x) {
  __shared__ unsigned long long s_k[kPsRun];
  __shared__ uint32_t s_v[kPsRun];
  __shared__ int s_red[16][4];
  const int n = b.n, tid = threadIdx.x;
  const int i = blockIdx.x * kPsRun + tid;
  uint32_t k32 = 0xFFFFFFFFu;
  if (i < n) k32 = score_desc_key(scores[(size_t)i * score_stride]);
  local_extras(x, dets5, drop_small, n, i, i < n, s_red, &k32);
  s_k[tid] = ((unsigned long long)k32 << 32) | (unsigned long long)(uint32_t)i;      // (a pad: 0xFFFFFFFF | position >= n)
  s_v[tid] = (uint32_t)i;
  ps_local_tail(b, n, s_k, s_v);
}
// ... and the plain key kernel for lists the three-launch sort does not take (n > kPsMaxN): 64-bit keys (score bits << 32 |
// index) for segsort.h's LSD radix sort over the four score bytes (stable: ties keep ascending index)
__global__ __launch_bounds__(kPsRun) void k_make_keys_wide(const float* __restrict__ scores, int score_stride, const float* __restrict__ dets5,
                                                           int drop_small, int n, unsigned long long* __restrict__ keys, uint32_t* __restrict__ vals,
                                                           LocalExtras x) {
  __shared__ int s_red[16][4];
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t k32 = 0xFFFFFFFFu;
  if (i < n) k32 = score_desc_key(scores[(size_t)i * score_stride]);
  local_extras(x, dets5, drop_small, n, i, i < n, s_red, &k32);
  if (i < n) { keys[i] = ((unsigned long long)k32 << 32) | (unsigned long long)(uint32_t)i; vals[i] = (uint32_t)i; }
}

// the extent of the data from the key kernel's per-block partials (every block reduces them itself: a few hundred int4)
__device__ __forceinline__ GridPlan plan_from_partials(const int* __restrict__ bbpart, int nparts, int (*s_red)[4], float* max_w2h2) {
  int bx0 = 0x7fffffff, by0 = 0x7fffffff, bx1 = (int)0x80000000, by1 = (int)0x80000000, d2 = 0, d2b = 0;
  for (int i = threadIdx.x; i < nparts; i += blockDim.x) {
    const int4 q = reinterpret_cast<const int4*>(bbpart)[2 * i];
    bx0 = min(bx0, q.x); by0 = min(by0, q.y); bx1 = max(bx1, q.z); by1 = max(by1, q.w);
    d2 = max(d2, bbpart[(size_t)i * kBbInts + 4]);
  }
  block_minmax4(bx0, by0, bx1, by1, s_red);
  { int lo0 = 0x7fffffff, lo1 = 0x7fffffff; d2b = d2; block_minmax4(lo0, lo1, d2, d2b, s_red); }
  *max_w2h2 = __int_as_float(d2);
  const int bb[4] = {bx0, by0, bx1, by1};
  return grid_plan(bb);
}

// blockDim.x is a multiple of 64 and p starts at 0: every wave covers one word of the alive bitmap
// slab_cover != NULL: every box that takes part also marks the x bins its circle interval touches (grid.h, "independent
// slabs"), first in a bitmap of the block in LDS, then with one atomicOr per non-zero word.
__global__ __launch_bounds__(256) void k_prep_rot(const float* __restrict__ dets5, const uint32_t* __restrict__ order, int drop_small, int n,
                                                  float4* __restrict__ rec, u64* __restrict__ alive, const int* __restrict__ bbpart,
                                                  int nparts, uint32_t* __restrict__ slab_cover, int* __restrict__ slab_flag) {
  __shared__ int s_red[16][4];
  __shared__ uint32_t s_cover[kSlabWords];
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  bool ok = false, bad = false;
  float x = 0.f, y = 0.f, r = 0.f, ms2 = 0.f;
  if (p < n) {
    const float* d = dets5 + (size_t)order[p] * 5;
    float w = d[2], h = d[3], a = d[4];
    x = d[0]; y = d[1];
    RBoxFeat f = rbox_make_feat(x, y, w, h, a);
    float4 q[4];
    RotGeom::pack(f, q);
#pragma unroll
    for (int k = 0; k < 4; k++) rec[(size_t)p * 4 + k] = q[k];
    ok = !(drop_small && box_too_small(w, h));
    r = q[0].z; ms2 = q[0].w;
  }
  const u64 m = __ballot(ok);
  if ((threadIdx.x & 63) == 0 && (p & ~63) < n) alive[p >> 6] = m;
  if (p < 8) alive[((n + 63) >> 6) + p] = 0ull;      // guard words behind the last box (the bitmap is not memset)
  if (slab_cover == nullptr) return;
  // ---- independent slabs (grid.h): is the data wide enough to look for them at all (slab_flag[2], written by block 0;
  // every block derives the same answer from the same partials)?  If so, the x bins this block's boxes touch, first in
  // a bitmap of the block in LDS, then OR-ed into one of kSlabCopies global copies
  float max_w2h2 = 0.f;
  const GridPlan gp = plan_from_partials(bbpart, nparts, s_red, &max_w2h2);
  const bool gate = slab_gate(gp, max_w2h2);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    slab_flag[2] = gate ? 1 : 0;
    slab_flag[4] = __float_as_int(gp.x0);                    // the bins' origin and scale: the NMS kernel reads them instead of
    slab_flag[5] = __float_as_int(slab_inv_bin(gp));         // reducing the partials once more
  }
  if (!gate) return;
  for (int k = threadIdx.x; k < kSlabWords; k += blockDim.x) s_cover[k] = 0u;
  __syncthreads();
  const float inv = slab_inv_bin(gp);
  if (ok) {
    if (!slab_box_ok(gp, x, y, r, ms2)) bad = true;
    else {
      const float hw = slab_halfwidth(gp, x, r);
      const int b0 = slab_bin(x - hw, gp.x0, inv), b1 = slab_bin(x + hw, gp.x0, inv);
      for (int wd = b0 >> 5; wd <= (b1 >> 5); wd++) {
        const int lo = max(b0, wd * 32) & 31, hi = min(b1, wd * 32 + 31) & 31;
        const uint32_t mk = (hi == 31 ? 0xffffffffu : ((1u << (hi + 1)) - 1u)) & ~((1u << lo) - 1u);
        if ((s_cover[wd] & mk) != mk) atomicOr(&s_cover[wd], mk);
      }
    }
  }
  const int anybad = __syncthreads_or(bad ? 1 : 0);
  if (anybad && threadIdx.x == 0) atomicOr(slab_flag, 1);
  uint32_t* dst = slab_cover + (size_t)(blockIdx.x % kSlabCopies) * kSlabWords;
  for (int k = threadIdx.x; k < kSlabWords; k += blockDim.x) {
    const uint32_t v = s_cover[k];
    if (v && (__hip_atomic_load(dst + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & v) != v) atomicOr(dst + k, v);
  }
}

// ---- float64 rotated boxes (RotGeom64): 64-bit keys from the double scores, records from the double boxes
__device__ __forceinline__ uint64_t score_desc_key64(double s) {
  uint64_t u = (uint64_t)__double_as_longlong(s);
  uint64_t k;
  if (s != s) k = ~0ull;                                   // NaN first (torch's order), as score_desc_key
  else {
    if (s == 0.0) u = 0ull;                                // -0 == +0
    k = (u & 0x8000000000000000ull) ? ~u : (u | 0x8000000000000000ull);
  }
  return ~k;
}
__global__ void k_make_keys_f64(const double* __restrict__ scores, const double* __restrict__ dets5, int drop_small, int n,
                                unsigned long long* __restrict__ keys, uint32_t* __restrict__ vals, int* seg_begin, int* seg_end, int* keep_cnt) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) { seg_begin[0] = 0; seg_end[0] = n; keep_cnt[0] = 0; }
  if (i >= n) return;
  uint64_t k = score_desc_key64(scores[i]);
  if (drop_small) {
    const double w = dets5[(size_t)i * 5 + 2], h = dets5[(size_t)i * 5 + 3];
    if (box_too_small(w, h)) k = ~0ull;                           // nms_rotated_wrapper.py:32, compared in the tensor's dtype
  }
  keys[i] = k;
  vals[i] = (uint32_t)i;
}
__global__ __launch_bounds__(256) void k_prep_rot64(const double* __restrict__ dets5, const uint32_t* __restrict__ order, int drop_small, int n,
                                                    float4* __restrict__ rec, u64* __restrict__ alive) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  bool ok = false;
  if (p < n) {
    const double* d = dets5 + (size_t)order[p] * 5;
    const double x = d[0], y = d[1], w = d[2], h = d[3], a = d[4];
    float4 q[RotGeom64::RECQ];
    RotGeom64::pack(x, y, w, h, a, q);
#pragma unroll
    for (int k = 0; k < RotGeom64::RECQ; k++) rec[(size_t)p * RotGeom64::RECQ + k] = q[k];
    ok = !(drop_small && box_too_small(w, h));
  }
  const u64 m = __ballot(ok);
  if ((threadIdx.x & 63) == 0 && (p & ~63) < n) alive[p >> 6] = m;
  if (p < 8) alive[((n + 63) >> 6) + p] = 0ull;      // guard words behind the last box (the bitmap is not memset)
}

__global__ void k_prep_quad(const float* __restrict__ polys, int stride, const uint32_t* __restrict__ order, int n, float thr, int skip,
                            float4* __restrict__ rec, u64* __restrict__ alive) {
  int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p < n) {
    const float* d = polys + (size_t)order[p] * stride;
    float c[8];
#pragma unroll
    for (int k = 0; k < 8; k++) c[k] = d[k];
    // skip bit 1: the bounding-box rule (thr <= 0 or bit clear: budget -inf); bit 0: the exact cone rule
    const QuadFeat qf = quad_make_feat(c);
    const QuadSkip sk = quad_skip_record(qf, (skip & 2) ? thr : 0.f);
    const uint32_t cone = (skip & 1) ? quad_cone_bits(qf) : kConeNone;
    uint32_t w0 = sk.lo, w1 = sk.hi;
    QuadCone2 c2w; c2w.ext = kConeNone; c2w.rm = kRmNone;
    if (skip & 1) c2w = quad_cone2_bits(qf);
    if ((skip & 1) && sk.f == -__builtin_huge_valf()) {
      // a quad without a budget takes no part in the bounding-box rule: its two box words carry what the SECOND proved rule
      // needs instead (piou_device.h: the extended cone and (r, M); QuadGeom::cheap_reject reads them when both budgets are -inf)
      w0 = c2w.ext; w1 = c2w.rm;
    }
    float4* r = rec + (size_t)p * QuadGeom::RECQ;
    r[0] = make_float4(__builtin_bit_cast(float, w0), __builtin_bit_cast(float, w1), sk.f, __builtin_bit_cast(float, cone));
    r[1] = make_float4(c[0], c[1], c[2], c[3]);
    r[2] = make_float4(c[4], c[5], c[6], c[7]);
    r[3] = make_float4(__builtin_bit_cast(float, c2w.ext), __builtin_bit_cast(float, c2w.rm), 0.f, 0.f);     // the second cone rule's words (QuadGeom::classify_quick)
  }
  const u64 m = __ballot(p < n);
  if ((threadIdx.x & 63) == 0 && (p & ~63) < n) alive[p >> 6] = m;
  if (p < 8) alive[((n + 63) >> 6) + p] = 0ull;      // guard words behind the last box (the bitmap is not memset)
}

// merge NMS (QuadGeom64): rows arrive as (n, 9) doubles, `order` lists the row indices in processing order, segment by
// segment.  Record = fp32 AABB rounded outward + the 8 doubles.
__device__ __forceinline__ float f32_down(double v) { float f = (float)v; return ((double)f > v) ? nextafterf(f, -INFINITY) : f; }
__device__ __forceinline__ float f32_up(double v) { float f = (float)v; return ((double)f < v) ? nextafterf(f, INFINITY) : f; }
// allow_reject = 0 (a negative or NaN threshold: even a ratio of 0 removes a box) or a coordinate that is not finite: the hot
// loop's box is the whole plane, i.e. the pair always reaches hit_exact, which applies numpy's rules to it
__global__ void k_prep_quad64(const double* __restrict__ dets9, const int32_t* __restrict__ order, int n, int allow_reject,
                              float4* __restrict__ rec, u64* __restrict__ alive) {
  int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p < n) {
    const double* d = dets9 + (size_t)order[p] * 9;
    double v[8];
#pragma unroll
    for (int k = 0; k < 8; k++) v[k] = d[k];
    const double x1 = fmin(fmin(v[0], v[2]), fmin(v[4], v[6])), x2 = fmax(fmax(v[0], v[2]), fmax(v[4], v[6]));
    const double y1 = fmin(fmin(v[1], v[3]), fmin(v[5], v[7])), y2 = fmax(fmax(v[1], v[3]), fmax(v[5], v[7]));
    float4* r = rec + (size_t)p * QuadGeom64::RECQ;
    bool fin = true;
#pragma unroll
    for (int k = 0; k < 8; k++) fin = fin && (v[k] - v[k] == 0.0);
    const float inf = __builtin_huge_valf();
    r[0] = (allow_reject && fin) ? make_float4(f32_down(x1), f32_down(y1), f32_up(x2), f32_up(y2)) : make_float4(-inf, -inf, inf, inf);
    double2* q = reinterpret_cast<double2*>(r + 1);
#pragma unroll
    for (int k = 0; k < 4; k++) q[k] = make_double2(v[2 * k], v[2 * k + 1]);
  }
  const u64 m = __ballot(p < n);
  if ((threadIdx.x & 63) == 0 && (p & ~63) < n) alive[p >> 6] = m;
  if (p < 8) alive[((n + 63) >> 6) + p] = 0ull;      // guard words behind the last box (the bitmap is not memset)
}

// records of the horizontal-box merge NMS (HbbGeom64): columns 0..3 of rows of `stride` doubles, in processing order
__global__ void k_prep_hbb64(const double* __restrict__ dets, int stride, const int32_t* __restrict__ order, int n, int allow_reject,
                             float4* __restrict__ rec, u64* __restrict__ alive) {
  int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p < n) {
    const double* d = dets + (size_t)order[p] * stride;
    const double x1 = d[0], y1 = d[1], x2 = d[2], y2 = d[3];
    const double area = (x2 - x1 + 1) * (y2 - y1 + 1);
    const bool fin = (x1 - x1 == 0.0) && (y1 - y1 == 0.0) && (x2 - x2 == 0.0) && (y2 - y2 == 0.0);
    float4* r = rec + (size_t)p * HbbGeom64::RECQ;
    const float inf = __builtin_huge_valf();
    r[0] = (allow_reject && fin && area > 0.0 && area - area == 0.0) ? make_float4(f32_down(x1), f32_down(y1), f32_up(x2 + 1), f32_up(y2 + 1))
                                                                    : make_float4(-inf, -inf, inf, inf);
    double2* q = reinterpret_cast<double2*>(r + 1);
    q[0] = make_double2(x1, y1); q[1] = make_double2(x2, y2);
  }
  const u64 m = __ballot(p < n);
  if ((threadIdx.x & 63) == 0 && (p & ~63) < n) alive[p >> 6] = m;
  if (p < 8) alive[((n + 63) >> 6) + p] = 0ull;      // guard words behind the last box (the bitmap is not memset)
}

// ---------------------------------------------------------------- the phase-kernel path of a long single list (nms_mk.h)
// Steps are enqueued without knowing how many the data needs (stream-ordered: nothing is read back).  Every kernel of a step
// returns at once when the control block says the call is complete, and whatever the enqueued steps leave undone is finished by
// the persistent kernel launched behind them (NmsResume) -- which returns at once when nothing is left.  The device records the
// number of steps a call needed in a pinned word of the calling thread (one per size class); the thread's next call of that size
// enqueues that many.  Which path a call takes, how many steps it enqueues and the feedback words' names: nms_plan.h.
struct MkFeedback { int* words; unsigned calls; };
static MkFeedback* mk_feedback(int64_t n) {
  static thread_local int* base = nullptr;
  static thread_local MkFeedback fb[64];
  if (!base) {
    void* p = nullptr;
    if (hipHostMalloc(&p, 64 * kFbWords * sizeof(int), hipHostMallocPortable) != hipSuccess) return nullptr;
    base = (int*)p;
    for (int i = 0; i < 64 * kFbWords; i++) base[i] = -1;
    for (int i = 0; i < 64; i++) { fb[i].words = base + kFbWords * i; fb[i].calls = 0; }
  }
  int b = 0;
  while ((n >> b) > 1 && b < 63) b++;
  return &fb[b];
}
static int mk_steps(MkArgs& a, const SingleListPlan& plan, const DeviceCus& dc, hipStream_t st) {
  static OncePerDevice attr, attr_cross;                // (two limits: one record each)
  static_assert(sizeof(MkLdsSelect) <= kMkSerialLds && (size_t)RotGeom::SCR * 64 * 4 * kMkWaves <= kMkSerialLds, "serial-phase LDS");
  if (!raise_lds_once_on(dc.dev, attr, kMkSerialLds, k_mk_select, k_mk_decide<false>, k_mk_decide<true>) ||
      !raise_lds_once_on(dc.dev, attr_cross, sizeof(MkLdsCross), k_mk_cross_lds))
    return OBB_ERR_LAUNCH;
  const int steps = plan.steps;
  if (a.hint_host) { *(volatile int*)(a.hint_host + kFbEnqueued) = steps; }
  const unsigned cus = (unsigned)dc.hw_cus;
  const unsigned gp = 4 * cus;                         // (k_mk_probe: four 256-thread workgroups per CU)
  k_mk_select<<<1, kMkThreads, kMkSerialLds, st>>>(a);
  for (int s = 0; s < steps; s++) {
    k_mk_probe<false><<<gp, kMkProbeThreads, 0, st>>>(a);
    k_mk_decide<false><<<cus, kMkThreads, kMkSerialLds, st>>>(a);      // ... + resolve in its last workgroup
    // (the step that completes a call has nothing behind its chunk: no cross half for the last enqueued step -- two empty launches,
    //  ~10 us; a call that needs more steps than were enqueued goes on in the persistent kernel with this cross phase, NmsResume stage 3)
    if (s == steps - 1) break;
    if (plan.xlds) k_mk_cross_lds<<<2 * cus, kMkXThreads, sizeof(MkLdsCross), st>>>(a);
    else k_mk_probe<true><<<gp, kMkProbeThreads, 0, st>>>(a);
    k_mk_decide<true><<<cus, kMkThreads, kMkSerialLds, st>>>(a);       // ... + the next select in its last workgroup
  }
  return hipGetLastError() == hipSuccess ? OBB_OK : OBB_ERR_LAUNCH;
}

// One list sorted by descending score, ties by ascending index (nms_rotated_cuda.cu:81-82 leaves the tie order to an
// unstable sort; this is the documented rule here): sorted keys in cv.keys_b, order in cv.vals_b.  Up to kPsMaxN elements:
// three launches (psrs_sort.h); longer lists: key kernel + LSD radix sort over the four score bytes (segsort.h).
// (Writing the NMS records in the tail of the sort's last kernel instead of a launch of their own was built and measured in
//  round 4: the bucket kernel went from 16.6 to 34 us -- one workgroup per CU because of its 104 KB of LDS, the double-precision
//  sin / cos and the gathers of the boxes at that occupancy -- against 8 us for k_prep_rot: 9 us slower per call.  Not kept.)
static int sort_single_list(const float* scores, int score_stride, const float* dets5, int drop_small, int64_t n, const Carve& cv,
                            const LocalExtras& x, int* nparts_out, hipStream_t st) {
  if (n <= kPsMaxN) {
    PsBuf b{};
    b.run_k = cv.keys_a; b.run_v = cv.vals_a; b.out_k = cv.keys_b; b.out_v = cv.vals_b; b.n = (int)n; b.n_dev = nullptr; b.err = nullptr;
    ps_carve_scratch(cv.sort_tmp, &b);
    const int runs = (int)((n + kPsRun - 1) / kPsRun);
    k_ps_local_scores<<<(unsigned)runs, kPsRun, 0, st>>>(b, scores, score_stride, dets5, drop_small, x);
    *nparts_out = runs;
    return ps_finish(b, runs, st);
  }
  const unsigned gb = (unsigned)((n + kPsRun - 1) / kPsRun);
  k_make_keys_wide<<<gb, kPsRun, 0, st>>>(scores, score_stride, dets5, drop_small, (int)n, cv.keys_a, cv.vals_a, x);
  *nparts_out = (int)gb;
  return seg_radix_sort_large(cv.keys_a, cv.keys_b, cv.vals_a, cv.vals_b, cv.seg_begin, cv.seg_end, 1, n, n, 0xF0u, cv.sort_hist, st);
}

// kind: 0 rotated (5 floats + score array), 1 quad (rows of `stride` floats, score in column 8)
static int run_nms(int kind, const float* boxes, int stride, const float* scores, int score_stride, int64_t n, float thr, int flags,
                   int64_t max_keep, int64_t* keep_out, int64_t* num_keep, void* ws, size_t ws_bytes, hipStream_t st) {
  const int64_t nseg = 1;
  if (n < 0 || n > 0x7fffffffLL) return OBB_ERR_BAD_ARG;
  if (!num_keep || (n > 0 && (!boxes || !scores || !keep_out))) return OBB_ERR_BAD_ARG;
  const int C = cap_max(nseg);
  const int recq = kind == 0 ? RotGeom::RECQ : QuadGeom::RECQ;
  const DeviceCus dc = device_cus();
  Carve cv = carve(ws, n, nseg, recq, C, dc.cus);
  if (!ws_ok(ws, ws_bytes, cv.total)) return OBB_ERR_WORKSPACE;
  const int T = 256;
  const int drop_small = (flags & OBB_NMS_DROP_SMALL) ? 1 : 0;
  const unsigned gseg = 1;

  if (n == 0) return finalize_empty(cv, nseg, false, max_keep, num_keep, st);

  const unsigned gb = (unsigned)((n + T - 1) / T);
  int pre = 0;
  // the call's path (nms_plan.h), from ONE read of the thread's feedback words, before anything is enqueued
  const NmsEnv env = nms_env();
  const bool has_grid = cv.grid.meta != nullptr, has_mk = cv.mk_cidx != nullptr;
  MkFeedback* const fbk = single_list_mk_possible(kind, n, thr, max_keep, has_grid, has_mk) ? mk_feedback(n) : nullptr;
  FbSnapshot snap{};
  if (fbk) snap = fb_snapshot(fbk->words);
  const unsigned calls = mk_counts_call(env, fbk != nullptr) ? fbk->calls++ : 0u;
  const SingleListPlan plan = plan_single_list(kind, n, thr, max_keep, has_grid, has_mk, fbk ? &snap : nullptr, calls, env);
  const bool use_grid = plan.use_grid, use_mk = plan.use_mk, use_slabs = plan.use_slabs;
  {
    ProfScope ps(PROF_NMS_SORT, st);
    LocalExtras x{};
    x.seg_begin = cv.seg_begin; x.seg_end = cv.seg_end; x.keep_cnt = cv.keep_cnt;
    x.bar16 = reinterpret_cast<uint4*>(cv.bar); x.n_bar16 = (long long)(cv.bar_bytes / 16);
    x.grid16 = reinterpret_cast<uint4*>(cv.grid.meta); x.n_grid16 = use_grid ? (long long)(cv.grid_zero_bytes / 16) : 0ll;
    x.mk16 = reinterpret_cast<uint4*>(cv.mk_ctl); x.n_mk16 = use_mk ? 64 : 0;
    x.bbpart = (use_grid && kind == 0) ? cv.grid.bbpart : nullptr;
    x.tstart = fbk ? cv.tstart : nullptr;
    if (const int rc = sort_single_list(scores, score_stride, kind == 0 ? boxes : nullptr, kind == 0 ? drop_small : 0, n, cv, x, &cv.grid.nparts, st)) return rc;
    pre = kNmsBarZeroed;
  }
  {
    ProfScope ps(PROF_NMS_PREP, st);
    if (kind == 0) k_prep_rot<<<gb, T, 0, st>>>(boxes, cv.vals_b, drop_small, (int)n, cv.rec, cv.alive, cv.grid.bbpart, cv.grid.nparts,
                                                use_slabs ? cv.grid.slab_cover : nullptr, cv.grid.slab_flag);
    else k_prep_quad<<<gb, T, 0, st>>>(boxes, stride, cv.vals_b, (int)n, thr, env.quad_skip, cv.rec, cv.alive);
  }

  MkArgs m{};
  if (use_mk) {
    static_assert(sizeof(MkCtl) <= 256, "the control block and its counters share one zeroed KB");
    m.rec = cv.rec; m.order = cv.vals_b; m.alive = cv.alive; m.n = (int)n;
    m.ctl = reinterpret_cast<MkCtl*>(cv.mk_ctl);
    m.cidx = cv.mk_cidx; m.ent = cv.mk_ent; m.start = cv.mk_start; m.kbits = cv.mk_kbits; m.hasin = cv.mk_hasin;
    m.edges = cv.edges; m.nedges = cv.mk_ctl + 64; m.ecap = cv.ecap;
    m.rows = cv.rows; m.nrows = cv.mk_ctl + 128; m.keep_cnt = cv.keep_cnt; m.keep_out = keep_out;
    m.bbpart = cv.grid.bbpart; m.nparts = cv.grid.nparts;
    m.capmax = kMkCapMax; m.cap_first = plan.cap_first;
    static_assert(kMkTile == 8192, "cap_max(1)");
    m.thr = thr;
    m.pend1 = cv.mk_pend1; m.cap1 = plan.pend_cap; m.num_keep = nullptr;    // (k_finalize below writes the count)
    m.hint_host = fbk ? fbk->words : nullptr;
    if (env.phase_prof) {   // development aid: print the previous call's serial-phase times (synchronises!)
      u64 h[56];
      if (hipMemcpy(h, cv.prof, sizeof h, hipMemcpyDeviceToHost) == hipSuccess && h[37] > 0 && h[37] < (1ull << 20)) {
        fprintf(stderr, "[mk phases, us, sums over %llu steps] pairs: decide+ticket %.1f (pending %llu) resolve %.1f [first round %.1f other rounds %.1f output %.1f; rounds %llu] | "
                        "cross: decide+ticket %.1f (pending %llu) select %.1f chunk-table %.1f | edges %llu chunk members %llu kept %llu\n",
                h[37], h[32] * 0.01, h[42], h[33] * 0.01, h[12] * 0.01, h[13] * 0.01, h[14] * 0.01, h[11], h[41] * 0.01, h[43], h[35] * 0.01, h[36] * 0.01, h[38], h[39], h[40]);
        fprintf(stderr, "    chunk table: loads %.1f statistics %.1f counts %.1f scan %.1f scatter %.1f\n", h[44] * 0.01, h[45] * 0.01, h[46] * 0.01, h[47] * 0.01, h[48] * 0.01);
        if (h[53]) fprintf(stderr, "    cross probe in LDS, per workgroup (%llu workgroup-steps): table %.1f (longest %.1f) wave 0's items %.1f (longest %.1f) whole %.1f (longest %.1f)\n",
                           h[53], h[49] * 0.01 / h[53], h[54] * 0.01, h[50] * 0.01 / h[53], h[55] * 0.01, h[51] * 0.01 / h[53], h[52] * 0.01);
      }
      if (hipMemsetAsync(cv.prof, 0, 56 * 8, st) != hipSuccess) return OBB_ERR_LAUNCH;
      m.prof = cv.prof;
    }
  }

  NmsArgs a{};
  if (use_grid) {
    a.gmeta = cv.grid.meta; a.bbpart = cv.grid.bbpart; a.nparts = cv.grid.nparts; a.gcnt = cv.grid.cnt; a.gstart = cv.grid.start;
    a.gsorted = cv.grid.sorted; a.gslot = cv.grid.slot_of; a.gwsum = cv.grid.wsum; a.ulist = cv.grid.ulist; a.gmask = cv.grid.mask; a.gfine = kGridFine;
  }
  if (use_slabs) {
    a.slab_cover = cv.grid.slab_cover; a.slab_flag = cv.grid.slab_flag; a.slab_cnt = cv.grid.slab_cnt; a.slab_tot = cv.grid.slab_tot; a.slab_keep = cv.grid.slab_keep;
    a.rec2 = cv.grid.rec2; a.order2 = cv.grid.order2; a.pos_old = cv.grid.pos_old; a.alive2 = cv.grid.alive2; a.kept_bits = cv.grid.kept_bits;
    a.alive2_words = (int)cv.grid.alive2_words; a.kept_words = (int)cv.grid.kept_words;
    a.slab_plan = cv.grid.slab_plan;
    a.slab_cap = plan.slab_cap;
  }
  nms_args_from(cv, C, &a);
  a.order = cv.vals_b; a.keep_out = keep_out; a.n = (int)n;
  nms_args_limit(&a, max_keep, thr);
  a.thr64 = thr;

  {
    ProfScope ps(PROF_NMS_STEPS, st);
    if (use_mk) {
      if (const int rc = mk_steps(m, plan, dc, st)) return rc;
      a.resume = reinterpret_cast<const NmsResume*>(cv.mk_ctl);   // the persistent kernel behind them: returns at once when they completed the call
    }
    if (const int rc = nms_steps(kind, a, cv, nseg, n, dc, st, pre)) return rc;
  }
  FinalizeFeedback ff;
  if (fbk) { ff.feedback = fbk->words; ff.tstart = cv.tstart; }
  ff.slab_plan = a.slab_plan; ff.feedback_slab = use_mk ? 0 : 1;
  if (use_mk) { ff.mk_ctl = reinterpret_cast<const NmsResume*>(cv.mk_ctl); ff.mk_enqueued = fbk ? plan.steps : 0; }
  k_finalize<<<gseg, T, 0, st>>>(cv.keep_cnt, cv.seg_begin, (int)nseg, max_keep, cv.abort_flag, num_keep, nullptr, ff);
  return hipGetLastError() == hipSuccess ? OBB_OK : OBB_ERR_LAUNCH;
}

static int kind_recq(int kind) {
  return kind == 0 ? RotGeom::RECQ : (kind == 1 ? QuadGeom::RECQ : (kind == 2 || kind == 4 ? QuadGeom64::RECQ : (kind == 5 ? HbbGeom64::RECQ : RotGeom64::RECQ)));
}

// Tile -> full-image merge NMS: nseg independent lists, the caller fixes the processing order (numpy's argsort()[::-1] of
// the reference is not a stable sort: its tie order is the host's business).  keep_out receives ROW indices, the kept rows of
// segment g at keep_out[seg_off[g] ...], in processing order.
// kind 2: py_cpu_nms_poly_fast (rows of 9 doubles), 4: py_cpu_nms_poly (the same rows, no horizontal-box gate), 5: py_cpu_nms
// (horizontal boxes in columns 0..3 of rows of `stride` doubles).
static int run_merge_nms(int kind, const double* dets9, int stride, int64_t n, const int32_t* order, const int32_t* seg_off, int64_t nseg,
                         double thr, int64_t* keep_out, int64_t* num_keep, void* ws, size_t ws_bytes, hipStream_t st) {
  if (n < 0 || nseg < 1 || n > 0x7fffffffLL || !num_keep || !seg_off) return OBB_ERR_BAD_ARG;
  if (n > 0 && (!dets9 || !order || !keep_out)) return OBB_ERR_BAD_ARG;
  if (kind == 5 && stride < 4) return OBB_ERR_BAD_ARG;
  const int C = cap_max(nseg);
  const DeviceCus dc = device_cus();
  const Carve cv = carve(ws, n, nseg, kind_recq(kind), C, dc.cus);
  if (!ws_ok(ws, ws_bytes, cv.total)) return OBB_ERR_WORKSPACE;
  const int T = 256;
  const unsigned gseg = (unsigned)((nseg + T - 1) / T);
  k_seg_from_offsets<<<gseg, T, 0, st>>>(seg_off, (int)nseg, cv.seg_begin, cv.seg_end, cv.keep_cnt);
  if (n == 0) return finalize_empty(cv, nseg, true, 0, num_keep, st);
  if (kind == 5) k_prep_hbb64<<<(unsigned)((n + T - 1) / T), T, 0, st>>>(dets9, stride, order, (int)n, (thr >= 0.0) ? 1 : 0, cv.rec, cv.alive);
  else k_prep_quad64<<<(unsigned)((n + T - 1) / T), T, 0, st>>>(dets9, order, (int)n, (thr >= 0.0) ? 1 : 0, cv.rec, cv.alive);
  NmsArgs a{};
  nms_args_from(cv, C, &a);
  a.order = reinterpret_cast<const uint32_t*>(order); a.keep_out = keep_out; a.n = (int)n;
  nms_args_limit(&a, 0, (float)thr);
  a.thr64 = thr; a.cull = 1;                                 // (thr < 0: the records carry the rule, k_prep_*64)
  if (const int rc = nms_steps(kind, a, cv, nseg, n, dc, st)) return rc;
  k_finalize<<<gseg, T, 0, st>>>(cv.keep_cnt, cv.seg_begin, (int)nseg, 0, cv.abort_flag, num_keep, nullptr, FinalizeFeedback{});
  return hipGetLastError() == hipSuccess ? OBB_OK : OBB_ERR_LAUNCH;
}

// float64 rotated NMS (one list): the reference's double instantiation (nms_rotated_cuda.cu:96), RotGeom64
static int run_nms_rot64(const double* dets5, const double* scores, int64_t n, float thr, int flags, int64_t max_keep, int64_t* keep_out,
                         int64_t* num_keep, void* ws, size_t ws_bytes, hipStream_t st) {
  if (n < 0 || n > 0x7fffffffLL || !num_keep || (n > 0 && (!dets5 || !scores || !keep_out))) return OBB_ERR_BAD_ARG;
  const int C = cap_max(1);
  const DeviceCus dc = device_cus();
  const Carve cv = carve(ws, n, 1, RotGeom64::RECQ, C, dc.cus);
  if (!ws_ok(ws, ws_bytes, cv.total)) return OBB_ERR_WORKSPACE;
  const int T = 256;
  if (n == 0) return finalize_empty(cv, 1, false, max_keep, num_keep, st);
  const unsigned gb = (unsigned)((n + T - 1) / T);
  const int drop_small = (flags & OBB_NMS_DROP_SMALL) ? 1 : 0;
  k_make_keys_f64<<<gb, T, 0, st>>>(scores, dets5, drop_small, (int)n, cv.keys_a, cv.vals_a, cv.seg_begin, cv.seg_end, cv.keep_cnt);
  // 64-bit score keys are not unique: the stable LSD radix sort of segsort.h keeps ties in ascending index (eight passes; this
  // entry serves float64 callers, the double clip behind it costs orders of magnitude more than its sort)
  if (const int rc = seg_radix_sort_large(cv.keys_a, cv.keys_b, cv.vals_a, cv.vals_b, cv.seg_begin, cv.seg_end, 1, n, n, 0xFFu, cv.sort_hist, st)) return rc;
  k_prep_rot64<<<gb, T, 0, st>>>(dets5, cv.vals_b, drop_small, (int)n, cv.rec, cv.alive);
  NmsArgs a{};
  nms_args_from(cv, C, &a);
  a.order = cv.vals_b; a.keep_out = keep_out; a.n = (int)n;
  nms_args_limit(&a, max_keep, thr);
  a.thr64 = (double)thr;                                   // the kernel's threshold is a float (nms_rotated_cuda.cu:14)
  if (const int rc = nms_steps(3, a, cv, 1, n, dc, st)) return rc;
  k_finalize<<<1, T, 0, st>>>(cv.keep_cnt, cv.seg_begin, 1, max_keep, cv.abort_flag, num_keep, nullptr, FinalizeFeedback{});
  return hipGetLastError() == hipSuccess ? OBB_OK : OBB_ERR_LAUNCH;
}

}  // namespace obb
