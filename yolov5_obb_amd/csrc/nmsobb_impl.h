// Fused non_max_suppression_obb for gfx950 (namespace obb): the kernels behind the front and the driver.  The front kernels are
// in nmsobb_front.h (k_decode) and nms_head.h (the conv-layout fronts), which this header includes; the C entries are in nms.hip.
//
// Replaces the per-image Python loop of utils/general.py:772-862 (>= 10 tiny ATen kernels and >= 3 host
// syncs per image, then obb_nms with a device->host mask copy) by ONE stream-ordered call for the whole batch:
//
//   k_decode      workgroup = 256..1024 anchors: objectness of every row (the dense column a coupled Detect decode left, or
//                 2-4 B of each 400-800 B row), rows that pass `obj > conf` compacted into LDS; each listed row is then
//                 processed by a whole wave -- coalesced class scores, conf = obj*cls rounded in the input dtype,
//                 multi-label expansion by ballot, CSL decode = wave arg-max over the 180 angle bins (first maximum),
//                 theta = (idx-90)/180*3.141592, class filter -- and appended to the image's candidate region together
//                 with a 64-bit sort key (descending conf, then ascending anchor*nc+class: a deterministic tie rule).
//   sort per image (in LDS, k_sort_prep_lds; larger images: segsort.h / psrs_sort.h), top max_nms (30000) kept   (:845-846)
//   k_prep_cand   class offset xy += cls*max_wh (:849-851), rotated-box records, too-small filter of obb_nms
//   LC-NMS        (nms_core.h) with max_keep = max_det                           (:853-855)
//   k_gather_out  rows [x y l s theta conf cls] of the kept candidates, [bs][max_det][7] + counts
//
// Class segmentation.  The reference runs ONE greedy NMS per image over boxes shifted by cls*4096 so that boxes of
// different classes never overlap (:849-851).  Whenever that premise provably holds for what the reference's IoU
// code computes -- no candidate with 0.001 <= min(l,s) < 1 px (a box that thin, seen from >= 2.5k px away, is where the
// reference's fp32 corner rounding can fabricate an overlap, riou_device.h), at most max_nms candidates, not agnostic
// -- the image is split into one NMS segment per class: the sort key gets the class in its top byte (k_rekey), the
// segments are found by binary search (k_class_bounds), and the per-class kept lists (each in descending score) are
// merged back into the reference's global descending-score order by rank counting (k_gather_out).  The kept set and
// its order are identical to the single-list NMS; the work drops by about the number of classes and the segments
// (bs*nc of them) each get their own workgroup, so no inter-workgroup barrier is left on the path.  Images that do not
// qualify keep the single-list path inside the same launch (segment 0 of the image holds everything).
//
// The only host<->device traffic is the caller reading the bs counts (+ the overflow word) afterwards.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "geom.h"
#include "launch_once.h"
#include "nms_core.h"
#include "nms_driver.h"
#include "nms_head.h"
#include "nms_limits.h"
#include "nms_plan.h"
#include "nms_small.h"
#include "nmsobb_front.h"
#include "obb_device.h"
#include "obb_hip.h"
#include "psrs_sort.h"
#include "segsort.h"
#include "tta_head_plan.h"
#include "ws_layout.h"

namespace obb {

// Cross-class check of the images that hold short-sided boxes (kImgSmall, see the flag table above): every pair (short-sided
// box T, box B of ANOTHER class) that rbox_pair_well_conditioned does not vouch for goes through the reference's own arithmetic
// in the reference's argument order (the higher-scored box first, nms_rotated_cuda.cu:44-60), in the coordinates the reference
// uses (xy + cls * max_wh): first the COUNT of the clip's candidate points (rbox_npoints: the 16 edge crossings and the contained
// corners in the reference's fp32 operations, ~400 flops, no scratch) -- at most two points and the reference returns IoU = 0
// (box_iou_rotated_utils.h:322-324), which is what happens for all but a few thin boxes that point along the diagonal of the class
// offsets -- and the whole clip only for the pairs with more.  No IoU > thr among them: the classes of the image cannot interact
// (well-conditioned cross-class pairs have disjoint circles inside their windows: the reference returns exactly 0), its class
// segments give the reference's kept set.  Otherwise the image keeps the reference's single list -- and so does an image with more
// than kTinyMax short-sided boxes or more than kTinyPairs (box, candidate) combinations: the check is for the stray sub-pixel box of
// a trained detector (microseconds), and bounded at a few tens of microseconds per image.  (Measured on the conv stand-in's random-
// initialised heads, which put hundreds of sub-pixel boxes into some images: with bounds of 512 / 2 x 10^6 the check cost 0.7 ms per
// batch there and saved 0.4 ms of NMS kernel; such images keep the single list.)
// Launched only when the caller's previous call of the shape met such boxes (expected_cand bit 62): grid (kTinyParts, bs),
// blocks of images without the flag return at once.  Candidates beyond the top-max_nms cut are tested as well: conservative.
constexpr int kTinyMax = 64;              // short-sided boxes of an image the check takes ...
constexpr long long kTinyPairs = 262144;  // ... and candidates x short-sided boxes: above either the image is not checked (single list)
constexpr int kTinyParts = 32;
__global__ __launch_bounds__(256) void k_tiny_cross(const float4* __restrict__ cand, const unsigned long long* __restrict__ keys,
                                                    const int* __restrict__ cnt, long long cap_img, float class_offset, float thr,
                                                    int* __restrict__ tiny) {
  __shared__ float scr[RotGeom::SCR * 256];                     // clip scratch (the rare full clip): one column per thread inside its wave's block
  __shared__ RBoxFeat s_feat[kTinyMax];                         // the short-sided boxes in the reference's coordinates
  __shared__ unsigned long long s_key[kTinyMax];
  __shared__ float s_cls[kTinyMax];
  __shared__ int s_list[kTinyMax];
  __shared__ int s_n;
  const int b = blockIdx.y, part = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  if ((tiny[b] & (kImgSmall | kImgWide)) != kImgSmall) return;
  long long n = cnt[b * kCntPad];
  if (n > cap_img) n = cap_img;                                  // (a call that overflowed its slots is repeated by the caller)
  const size_t base = (size_t)b * cap_img;
  if (tid == 0) s_n = 0;
  __syncthreads();
  for (long long j = tid; j < n; j += 256) {                     // the image's short-sided candidates: every part builds the same set
    const float4 c0 = cand[(base + j) * 2];
    const float mn = min_nan(c0.z, c0.w);
    if (mn >= 0.001f && mn < 1.0f) { const int k = atomicAdd(&s_n, 1); if (k < kTinyMax) s_list[k] = (int)j; }
  }
  __syncthreads();
  const int nt = s_n;
  if (nt > kTinyMax || (long long)nt * n > kTinyPairs) return;   // not checked: single list
  if (part == 0 && tid == 0) atomicOr(&tiny[b], kImgChecked);
  for (int t = tid; t < nt; t += 256) {
    const int jt = s_list[t];
    const float4 t0 = cand[(base + jt) * 2], t1 = cand[(base + jt) * 2 + 1];
    const float offT = t1.z * class_offset;
    s_feat[t] = rbox_make_feat(t0.x + offT, t0.y + offT, t0.z, t0.w, t1.x);
    s_key[t] = keys[base + jt];
    s_cls[t] = t1.z;
  }
  __syncthreads();
  bool hit = false;
  float* myscr = scr + wv * (RotGeom::SCR * 64) + lane;
  for (long long j = (long long)part * 256 + tid; j < n; j += (long long)gridDim.x * 256) {
    const float4 c0 = cand[(base + j) * 2], c1 = cand[(base + j) * 2 + 1];
    if (box_too_small(c0.z, c0.w)) continue;                      // dropped by obb_nms (nms_rotated_wrapper.py:32): never a partner
    const float offB = c1.z * class_offset;
    const RBoxFeat B = rbox_make_feat(c0.x + offB, c0.y + offB, c0.z, c0.w, c1.x);
    const unsigned long long kB = keys[base + j];
    for (int t = 0; t < nt; t++) {
      if (s_cls[t] == c1.z) continue;                            // same class: decided inside the class segment, as in the single list
      const RBoxFeat T = s_feat[t];
      if (rbox_pair_well_conditioned(T, B)) continue;            // circles apart (different windows) and well conditioned: exactly 0
      const bool t_first = s_key[t] < kB;                        // smaller key = sorts first = the row box of the reference's kernel
      const int np = t_first ? rbox_npoints(T, B) : rbox_npoints(B, T);
      if (np <= 2) continue;                                     // the reference returns 0 (:322-324 / :353)
      const float v = t_first ? rbox_iou<64>(T, B, myscr, myscr + 24 * 64) : rbox_iou<64>(B, T, myscr, myscr + 24 * 64);
      if (v > thr) hit = true;
    }
  }
  if (__ballot(hit) && lane == 0) atomicOr(&tiny[b], kImgCross);
}

// per image: sort range, number of positions that take part, mode:
//   0  single list (the reference's formulation) -- also every image with more than max_nms candidates (the top max_nms by
//      confidence must be cut first, :845-846)
//   1  one NMS segment per class, class in the top key byte (k_rekey) -- needs <= max_nms candidates
__global__ void k_cand_segments(const int* __restrict__ cnt, const int* __restrict__ tiny, int bs, long long cap_img, long long max_nms,
                                int class_ok, int* sort_begin, int* sort_end, int* img_end, int* mode) {
  int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= bs) return;
  long long c = cnt[g * kCntPad];
  const bool over_cap = c > cap_img;
  if (over_cap) c = cap_img;
  const int b0 = (int)(g * cap_img);
  sort_begin[g] = b0; sort_end[g] = b0 + (int)c;
  const bool over_nms = max_nms > 0 && c > max_nms;
  if (over_nms) c = max_nms;                                 // :845-846 top max_nms by confidence
  img_end[g] = b0 + (int)c;
  mode[g] = (class_ok && !over_cap && !img_single_list(tiny[g]) && !over_nms) ? 1 : 0;
}

// class-segmented images: key (score_desc << 32 | anchor*nc + cls)  ->  (cls << 56 | score_desc << 24 | anchor)
// (ascending key order inside a class = descending score, ties by ascending anchor; extra rows count as anchors A, A+1, ..)
__global__ void k_rekey(const float4* __restrict__ cand, unsigned long long* __restrict__ keys, const int* __restrict__ sort_begin,
                        const int* __restrict__ sort_end, const int* __restrict__ mode, long long A, int nc) {
  const int g = blockIdx.y;
  if (mode[g] != 1) return;
  const int p = sort_begin[g] + blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= sort_end[g]) return;
  const unsigned long long k = keys[p];
  const unsigned long long score = k >> 32, tie = k & 0xffffffffull;
  const unsigned long long cls = (unsigned long long)(int)cand[(size_t)p * 2 + 1].z;
  const unsigned long long lim = (unsigned long long)A * nc;
  const unsigned long long anchor = tie < lim ? tie / nc : (unsigned long long)A + (tie - lim);
  keys[p] = (cls << 56) | (score << 24) | (anchor & 0xffffffull);
}

__device__ __forceinline__ int key_lower_bound_range(const unsigned long long* keys, int lo, int hi, unsigned long long target) {
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (keys[mid] < target) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// segment table: ncs segments per image (ncs = nc, or 1 when the call is class-agnostic)
__global__ void k_class_bounds(const unsigned long long* __restrict__ keys_sorted, const int* __restrict__ sort_begin,
                               const int* __restrict__ img_end, const int* __restrict__ mode, int bs, int ncs, int* __restrict__ seg_begin,
                               int* __restrict__ seg_end, int* __restrict__ keep_cnt) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= bs * ncs) return;
  const int g = s / ncs, c = s - g * ncs;
  const int b0 = sort_begin[g], e0 = img_end[g];
  int lo = b0, hi = b0;
  if (mode[g] == 1) {
    lo = key_lower_bound_range(keys_sorted, b0, e0, (unsigned long long)c << 56);
    hi = (c >= 255) ? e0 : key_lower_bound_range(keys_sorted, b0, e0, (unsigned long long)(c + 1) << 56);
  } else if (c == 0) {
    hi = e0;                                                   // single list: everything in segment 0 of the image
  }
  seg_begin[s] = lo; seg_end[s] = hi; keep_cnt[s] = 0;
}

__global__ void k_prep_cand(const float4* __restrict__ cand, const uint32_t* __restrict__ vals_sorted,
                            const int* __restrict__ img_begin, const int* __restrict__ img_end, long long cap_img,
                            float class_offset, float4* __restrict__ rec, u64* __restrict__ alive) {
  // img_begin[g] = g * cap_img with cap_img a multiple of 64: every wave covers exactly one word of the alive bitmap
  const int g = blockIdx.y;
  const int p = img_begin[g] + blockIdx.x * blockDim.x + threadIdx.x;
  const int se = img_end[g];
  bool ok = false;
  if (p < se) {
    const size_t ci = (size_t)g * cap_img + vals_sorted[p];
    const float4 c0 = cand[ci * 2], c1 = cand[ci * 2 + 1];
    const float off = c1.z * class_offset;                       // :849  c = x[:, 6:7] * (0 if agnostic else max_wh)
    const float x = c0.x + off, y = c0.y + off;                  // :851
    RBoxFeat f = rbox_make_feat(x, y, c0.z, c0.w, c1.x);
    float4 q[4];
    RotGeom::pack(f, q);
#pragma unroll
    for (int k = 0; k < 4; k++) rec[(size_t)p * 4 + k] = q[k];
    ok = !box_too_small(c0.z, c0.w);                             // nms_rotated_wrapper.py:32
  }
  const u64 m = __ballot(ok);
  if ((threadIdx.x & 63) == 0 && m) alive[p >> 6] = m;           // the bitmap was zeroed before
}

// One launch instead of four memsets: candidate counters, tiny-box flags, the caller's status words, the fused kernel's
// ticket and the team-barrier block of the NMS kernel.
__global__ void k_reset_state(int* __restrict__ cnt, int n_cnt, int* __restrict__ tiny, int bs, int64_t* __restrict__ status,
                              int* __restrict__ ticket, int n_ticket, uint4* __restrict__ bar16, long long n_bar16, uint4* __restrict__ alive16,
                              long long n_alive16) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x, n = (long long)gridDim.x * blockDim.x;
  for (long long k = i; k < n_cnt; k += n) cnt[k] = 0;
  for (long long k = i; k < bs; k += n) tiny[k] = 0;
  (void)status;                                                 // (both status words are written by the output stage)
  if (i < n_ticket) ticket[i] = 0;                              // [0] the planner's ticket, [4] largest NMS segment, [8] a segment k_nms_small left out,
                                                                // [16 .. 16 + bs] the tickets of k_nms_small's output stage
  for (long long k = i; k < n_bar16; k += n) bar16[k] = make_uint4(0u, 0u, 0u, 0u);
  // (the in-LDS sort path ORs its alive bits into zeroed words: several workgroups share the words of an image)
  for (long long k = i; k < n_alive16; k += n) alive16[k] = make_uint4(0u, 0u, 0u, 0u);
}

// the slots behind the image's candidates get the largest key (single image, device-wide sort over the whole capacity)
__global__ void k_pad_keys(unsigned long long* __restrict__ keys, uint32_t* __restrict__ vals, const int* __restrict__ sort_end, long long cap) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < cap && i >= (long long)sort_end[0]) { keys[i] = ~0ull; vals[i] = 0u; }
}

// Small and medium images (at most kSortLdsMax candidates each, the regime of the reference's default thresholds): ONE
// workgroup per image does everything between the decode kernel and the NMS kernel -- segment bookkeeping
// (k_cand_segments), class keys (k_rekey), the sort (a bitonic network on (key, slot) pairs in LDS), the class segment table (k_class_bounds), the NMS records and the alive
// bitmap including its zero words (k_prep_cand + memset): six launches become one.  An image with more candidates than
// the network takes is left empty; the caller sees its count in status[1] and calls again with that hint.
constexpr int kSortLdsMax = OBB_NMS_SORT_LDS_MAX;
__global__ __launch_bounds__(1024) void k_sort_prep_lds(const float4* __restrict__ cand, const unsigned long long* __restrict__ keys_in,
                                                        const uint32_t* __restrict__ vals_in, unsigned long long* __restrict__ keys_out,
                                                        uint32_t* __restrict__ vals_out, const int* __restrict__ cnt,
                                                        const int* __restrict__ tiny, int bs, long long cap_img, long long max_nms,
                                                        int class_ok, long long A, int nc, int ncs, float class_offset, int* sort_begin,
                                                        int* sort_end, int* img_end, int* mode,
                                                        int* __restrict__ seg_begin, int* __restrict__ seg_end, int* __restrict__ keep_cnt,
                                                        float4* __restrict__ rec, u64* __restrict__ alive, int* __restrict__ ticket,
                                                        int plan_nb, int plan_chunk, int4* __restrict__ plan, int* __restrict__ seg_size, int P,
                                                        int helpers, int* __restrict__ help_work, int* __restrict__ seg_np, int* __restrict__ seg_ticket) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  __shared__ PlanLds s_plan;
  __shared__ int s_hist[256], s_cls_off[256], s_cls_cur[256], s_cls_task[257], s_cls_max, s_cls_ntask;
  __shared__ u64 s_abits[kSortLdsMax / 2 / 64];
  unsigned long long* s_keys = reinterpret_cast<unsigned long long*>(s_raw);
  uint32_t* s_vals = reinterpret_cast<uint32_t*>(s_keys + kSortLdsMax);
  // blockIdx.x = image * P + part (class-segment images: part q orders and prepares the classes c with c % P == q; every
  // part reads the image's keys and builds the whole histogram itself), the last block is the planner
  const int g = blockIdx.x / P, q = blockIdx.x - g * P, tid = threadIdx.x, T = 1024;
  if (g == bs) {
    // The planner block (launched only when there is a plan to make): the NMS launch is planned from the segment SIZES,
    // which every image's workgroup knows after its first pass over the keys -- long before its sort is done.  This block
    // waits for the bs size tables (the other workgroups never wait for anything, so it cannot hang however the blocks
    // are scheduled) and plans while they sort: the 16 us of plan_teams_block used to be the tail of the last workgroup.
#ifdef OBB_SORT_TRACE
    const unsigned long long tp0 = wall_clock64();
#endif
    if (tid == 0) {
      while (__hip_atomic_load(ticket, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) < bs) __builtin_amdgcn_s_sleep(4);
    }
    __syncthreads();
#ifdef OBB_SORT_TRACE
    const unsigned long long tp1 = wall_clock64();
#endif
    plan_teams_block(nullptr, nullptr, seg_size, bs * ncs, plan_nb, plan_chunk, plan, s_plan);
#ifdef OBB_SORT_TRACE
    __syncthreads();
    if (tid == 0) printf("planner: waited %llu planned %llu (x10 ns)\n", tp1 - tp0, wall_clock64() - tp1);
#endif
    return;
  }
  long long c = cnt[g * kCntPad];
  const bool over_cap = c > cap_img;
  if (over_cap) c = cap_img;
  const int b0 = (int)(g * cap_img);
  if (c > kSortLdsMax) c = 0;                                  // not this kernel's regime: reported through status[1]
  const bool over_nms = max_nms > 0 && c > max_nms;
  const int e = (int)(over_nms ? max_nms : c);                 // :845-846 top max_nms by confidence
  const int m = (class_ok && !over_cap && !img_single_list(tiny[g]) && !over_nms) ? 1 : 0;
  const int n = (int)c;
  if (q > 0 && m != 1) return;                                 // one list per image: part 0 does it all
  if (tid == 0 && q == 0) {
    sort_begin[g] = b0; sort_end[g] = b0 + n; img_end[g] = b0 + e; mode[g] = m;
  }
  if (tid < 256) s_hist[tid] = 0;
  if (tid < kSortLdsMax / 2 / 64) s_abits[tid] = 0ull;
  __syncthreads();
#ifdef OBB_SORT_TRACE
  unsigned long long tt[12]; int ti_ = 0;
#define TSTAMP() do { __syncthreads(); tt[ti_++] = wall_clock64(); } while (0)
#else
#define TSTAMP() do {} while (0)
#endif
  TSTAMP();
  int npad = 64;
  while (npad < n) npad <<= 1;
  const unsigned long long lim = (unsigned long long)A * nc;
  for (int i = tid; i < npad; i += T) {
    unsigned long long k = ~0ull;
    uint32_t v = 0;
    if (i < n) {
      k = keys_in[b0 + i]; v = vals_in[b0 + i];
      if (m == 1) {                                            // k_rekey: (cls << 56 | score_desc << 24 | anchor)
        const unsigned long long score = k >> 32, tie = k & 0xffffffffull;
        const unsigned long long cls = (unsigned long long)(int)cand[(size_t)(b0 + i) * 2 + 1].z;
        const unsigned long long anchor = tie < lim ? tie / nc : (unsigned long long)A + (tie - lim);
        k = (cls << 56) | (score << 24) | (anchor & 0xffffffull);
        atomicAdd(&s_hist[(int)cls & 255], 1);
      }
    }
    s_keys[i] = k; s_vals[i] = v;
  }
  __syncthreads();
  if (plan != nullptr && q == 0) {                             // the size table of this image, for the planner block
    // write-through stores, drained, then a RELAXED arrival: a release fence here writes back every dirty line of this XCD's
    // L2 -- the records the other parts are storing at this very moment (measured: this handshake 4.8 -> 10.4 us)
    for (int sgm = tid; sgm < ncs; sgm += T) stg_agent(seg_size + g * ncs + sgm, (m == 1) ? s_hist[sgm] : (sgm == 0 ? e : 0));
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) __hip_atomic_fetch_add(ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  TSTAMP();
  // ascending; keys are unique (the tie word), so the result is the one total order
  // elements per thread: as few as the 1024 threads allow (measured: 8 per thread with 256 busy threads moves four more
  // levels into registers but is 16 us slower at 2048 candidates -- the lane shuffles become the bottleneck)
  // Class-segment images of up to 4096 candidates (the reference's default thresholds: ~1.7k per image in 15-18 classes): the
  // order wanted is class-major, so the candidates are first dealt into their class buckets (the histogram exists already;
  // scan, one LDS atomic per element) and every bucket is then ordered on its own, without a workgroup barrier inside --
  // instead of the 66 stages + 5 rank-merge levels of the 2048-element network (19.3 us).
  bool by_class = false;
  if (m == 1 && n <= kSortLdsMax / 2) {              // (workgroup-uniform)
    if (tid < 64) {
      int c4[4], sum = 0, mx = 0;
#pragma unroll
      for (int u = 0; u < 4; u++) { c4[u] = s_hist[tid * 4 + u]; sum += c4[u]; mx = c4[u] > mx ? c4[u] : mx; }
      int incl = sum;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) { const int up = __shfl_up(incl, d); if (tid >= d) incl += up; }
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) { const int o = __shfl_xor(mx, d); mx = o > mx ? o : mx; }
      int run = incl - sum;
#pragma unroll
      for (int u = 0; u < 4; u++) { s_cls_off[tid * 4 + u] = run; s_cls_cur[tid * 4 + u] = run; run += c4[u]; }
      // tasks of the rank-counting pass below: one per 64 elements of a class
      int t4[4], tsum = 0;
#pragma unroll
      for (int u = 0; u < 4; u++) { t4[u] = ((tid * 4 + u) % P == q) ? (c4[u] + 63) >> 6 : 0; tsum += t4[u]; }
      int tincl = tsum;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) { const int up = __shfl_up(tincl, d); if (tid >= d) tincl += up; }
      int trun = tincl - tsum;
#pragma unroll
      for (int u = 0; u < 4; u++) { s_cls_task[tid * 4 + u] = trun; trun += t4[u]; }
      if (tid == 63) { s_cls_task[256] = tincl; s_cls_ntask = tincl; }
      if (tid == 0) s_cls_max = mx;
    }
    __syncthreads();
    // (the rank counting is quadratic in the bucket: beyond 512 elements -- two classes, one dominant class -- the 16-wave network takes over)
    by_class = s_cls_max <= 512;
  }
  // the call's largest NMS segment (feedback for the caller's choice of the NMS kernel, include/obb_hip.h: status[1])
  if (q == 0 && tid == 0) atomicMax(ticket + 4, (m == 1 && n <= kSortLdsMax / 2) ? s_cls_max : e);
  TSTAMP();
  if (!by_class) {
    if (q > 0) return;                               // (workgroup-uniform) the network orders the whole image in part 0
    for (int sgm = tid; sgm < ncs; sgm += T) {
      seg_begin[g * ncs + sgm] = b0; seg_end[g * ncs + sgm] = b0; keep_cnt[g * ncs + sgm] = 0;
      if (helpers > 0) seg_np[g * ncs + sgm] = 1;                // (segments of this path stay whole)
    }
    __syncthreads();
  }
  if (by_class) {
    // segment table of this part's classes: straight from the histogram
    for (int c = q + P * tid; c < ncs; c += P * T) {
      const int cc = s_hist[c], sb = cc ? b0 + s_cls_off[c] : b0;
      seg_begin[g * ncs + c] = sb; seg_end[g * ncs + c] = sb + cc; keep_cnt[g * ncs + c] = 0;
      if (helpers > 0) {
        // k_nms_small shares a large segment among several workgroups (nms_small.h: SmallArgs): the helpers are handed out here,
        // where the sizes are known -- ticket[12] counts the slots; a segment that does not get its full set stays whole
        int np = (cc <= kSmallMax) ? small_parts(cc) : 1, base = 0;
        if (np > 1) {
          base = atomicAdd(ticket + 12, np - 1);
          const bool fits = base + np - 1 <= helpers;
          for (int p = 1; p < np; p++) if (base + p - 1 < helpers) help_work[base + p - 1] = fits ? ((g * ncs + c) | (p << 24)) : -1;
          if (!fits) np = 1;
        }
        seg_np[g * ncs + c] = np | (base << 8);
        seg_ticket[g * ncs + c] = 0;
      }
    }
    unsigned long long* s_keys2 = s_keys + kSortLdsMax / 2;
    uint32_t* s_vals2 = s_vals + kSortLdsMax / 2;
    unsigned long long kr[4];
    uint32_t vr[4];
#pragma unroll
    for (int u = 0; u < 4; u++) { const int i = tid + u * T; if (i < n) { kr[u] = s_keys[i]; vr[u] = s_vals[i]; } }
    __syncthreads();                                 // (the scatter's target overlaps nothing that is still being read: n <= 4096)
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int i = tid + u * T;
      if (i < n && (int)(kr[u] >> 56) % P == q) {
        const int pos = atomicAdd(&s_cls_cur[(int)(kr[u] >> 56)], 1);
        s_keys2[pos] = kr[u]; s_vals2[pos] = vr[u];
      }
    }
    __syncthreads();
    TSTAMP();
    // Every bucket is ordered by RANK COUNTING: a task is (class, 64 of its elements); each lane holds one of them and counts
    // the bucket's keys below its own -- the bucket is read 64 keys at a time (one LDS read per lane) and handed round with
    // v_readlane, so a comparison is two scalar broadcasts, one 64-bit compare and one add-with-carry, no LDS traffic.  Keys
    // are unique, so the rank is the element's place.  (The in-wave bitonic network on the same buckets: 11.3 us -- three
    // ds_bpermute per element and stage, 16 waves on one LDS; this: see DESIGN 4.2b.)
    const int wv = tid >> 6, lane = tid & 63;
    const int ntask = s_cls_ntask;
    for (int t = wv; t < ntask; t += T / 64) {
      int c = 0;
      {                                              // the class whose task range holds t (<= 256 classes: four per lane)
        u64 found = 0ull;
        int base_c = 0;
#pragma unroll
        for (int u = 0; u < 4; u++) {
          const int cc = u * 64 + lane;
          const bool in = t >= s_cls_task[cc] && t < s_cls_task[cc + 1];
          const u64 b = __ballot(in);
          if (b) { found = b; base_c = u * 64; }
        }
        c = base_c + __builtin_ctzll(found);
      }
      const int off = s_cls_off[c], cnt = s_hist[c], mine_i = (t - s_cls_task[c]) * 64 + lane;
      const bool have = mine_i < cnt;
      const unsigned long long mine = have ? s_keys2[off + mine_i] : 0ull;
      const uint32_t myv = have ? s_vals2[off + mine_i] : 0u;
      int rank = 0;
      for (int cb = 0; cb < cnt; cb += 64) {
        const unsigned long long ck = (cb + lane < cnt) ? s_keys2[off + cb + lane] : ~0ull;   // pads above every key: never counted
        const uint32_t clo = (uint32_t)ck, chi = (uint32_t)(ck >> 32);
        const int mm = min(64, cnt - cb);
        int j = 0;
        for (; j + 4 <= mm; j += 4) {
#pragma unroll
          for (int z = 0; z < 4; z++) {
            const unsigned long long kj = ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)chi, j + z) << 32) |
                                          (uint32_t)__builtin_amdgcn_readlane((int)clo, j + z);
            rank += (kj < mine) ? 1 : 0;
          }
        }
        for (; j < mm; j++) {
          const unsigned long long kj = ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)chi, j) << 32) |
                                        (uint32_t)__builtin_amdgcn_readlane((int)clo, j);
          rank += (kj < mine) ? 1 : 0;
        }
      }
      // the element's place is known: its sorted (key, slot) pair, its NMS record and its alive bit go out from here (the
      // generic tail below is the network's)
      if (have) {
        const int p = off + rank;
        keys_out[b0 + p] = mine; vals_out[b0 + p] = myv;
        const size_t ci = (size_t)b0 + myv;
        const float4 c0 = cand[ci * 2], c1 = cand[ci * 2 + 1];
        const float coff = c1.z * class_offset;                  // :849
        RBoxFeat f = rbox_make_feat(c0.x + coff, c0.y + coff, c0.z, c0.w, c1.x);
        float4 rq[4];
        RotGeom::pack(f, rq);
#pragma unroll
        for (int u = 0; u < 4; u++) rec[(size_t)(b0 + p) * 4 + u] = rq[u];
        if (!box_too_small(c0.z, c0.w)) atomicOr(&s_abits[p >> 6], 1ull << (p & 63));   // nms_rotated_wrapper.py:32
      }
    }
    __syncthreads();
    // the image's bitmap words were zeroed by k_reset_state; a word can hold positions of classes of several parts
    if (tid < kSortLdsMax / 2 / 64) { const u64 w = s_abits[tid]; if (w) atomicOr(alive + ((size_t)b0 >> 6) + tid, w); }
    if (g == bs - 1 && q == 0 && tid < 8) alive[(((size_t)bs * cap_img) >> 6) + tid] = 0ull;   // the bitmap's guard words
    TSTAMP();
#ifdef OBB_SORT_TRACE
    if (tid == 0 && g == 0) { printf("sortprep g %d part %d n %d by class, max %d:", g, q, n, s_cls_max); for (int z = 1; z < ti_; z++) printf(" %llu", tt[z] - tt[z - 1]); printf(" (x10 ns)\n"); }
#endif
    return;
  } else {
    switch (npad >> 10) {
      case 0: case 1: sort_lds_regs<1>(s_keys, s_vals, npad, tid); break;
      case 2: sort_lds_regs<2>(s_keys, s_vals, npad, tid); break;
      case 4: sort_lds_regs<4>(s_keys, s_vals, npad, tid); break;
      default: sort_lds_regs<8>(s_keys, s_vals, npad, tid); break;
    }
  }
  TSTAMP();
  for (int i = tid; i < n; i += T) { keys_out[b0 + i] = s_keys[i]; vals_out[b0 + i] = s_vals[i]; }
  // segment table (k_class_bounds): class runs of the sorted keys, or everything in segment 0
  if (m == 1) {
    for (int i = tid; i < e; i += T) {
      const int cls = (int)(s_keys[i] >> 56);
      if (i == 0 || cls != (int)(s_keys[i - 1] >> 56)) seg_begin[g * ncs + cls] = b0 + i;
      if (i == e - 1 || cls != (int)(s_keys[i + 1] >> 56)) seg_end[g * ncs + cls] = b0 + i + 1;
    }
  } else if (tid == 0) {
    seg_end[g * ncs] = b0 + e;
  }
  TSTAMP();
  // NMS records + every word of the image's part of the alive bitmap (k_prep_cand; cap_img is a multiple of 64)
  const int e64 = (e + 63) & ~63;
  for (long long w = (e64 >> 6) + tid; w < (cap_img >> 6); w += T) alive[((size_t)b0 >> 6) + w] = 0ull;   // words behind the boxes
  for (int base = 0; base < e64; base += T) {
    const int i = base + tid;
    bool ok = false;
    if (i < e) {
      const size_t ci = (size_t)b0 + s_vals[i];
      const float4 c0 = cand[ci * 2], c1 = cand[ci * 2 + 1];
      const float off = c1.z * class_offset;                     // :849
      RBoxFeat f = rbox_make_feat(c0.x + off, c0.y + off, c0.z, c0.w, c1.x);
      float4 q[4];
      RotGeom::pack(f, q);
#pragma unroll
      for (int u = 0; u < 4; u++) rec[(size_t)(b0 + i) * 4 + u] = q[u];
      ok = !box_too_small(c0.z, c0.w);                           // nms_rotated_wrapper.py:32
    }
    const u64 bits = __ballot(ok);
    if ((tid & 63) == 0 && i < e64) alive[(size_t)(b0 + i) >> 6] = bits;
  }
  TSTAMP();
  if (g == bs - 1 && tid < 8) alive[(((size_t)bs * cap_img) >> 6) + tid] = 0ull;   // the bitmap's guard words
#ifdef OBB_SORT_TRACE
  TSTAMP();
  if (tid == 0 && g == 0) { printf("sortprep g %d n %d by_class %d max %d:", g, n, (int)by_class, s_cls_max); for (int q = 1; q < ti_; q++) printf(" %llu", tt[q] - tt[q - 1]); printf(" (x10 ns)\n"); }
#endif
#undef TSTAMP
}

// Output: the kept boxes of the image's segments merged into descending-score order (the order of the reference's single
// greedy pass), first max_det of them.  One workgroup per image.  Each segment's kept list is already in ascending key
// order; the global rank of an entry = its index in its own list + the number of entries of every other list that
// precede it -- binary searches on merge keys (score, anchor, class) staged in LDS.
constexpr int kMergeLds = 4096;
__global__ __launch_bounds__(256) void k_gather_out(const float4* __restrict__ cand, const uint32_t* __restrict__ vals_sorted,
                                                    const unsigned long long* __restrict__ keys_sorted, const int64_t* __restrict__ keep,
                                                    const int* __restrict__ seg_begin, const int* __restrict__ keep_cnt,
                                                    const int* __restrict__ mode, int ncs, long long max_det, float* __restrict__ out,
                                                    int64_t* __restrict__ out_count, const int* __restrict__ cnt, long long cap_img,
                                                    int64_t* __restrict__ status, const int* __restrict__ abort_flag, int packed,
                                                    const int* __restrict__ info, const int* __restrict__ tiny, int* __restrict__ clean_cnt,
                                                    int* __restrict__ clean_tiny) {
  __shared__ int s_pre[257], s_seg[256];
  __shared__ long long s_rows[4], s_mx[4];
  __shared__ int s_tf[4];
  __shared__ unsigned long long s_key[kMergeLds];
  __shared__ uint32_t s_val[kMergeLds];
  const int g = blockIdx.x, tid = threadIdx.x;
  // blockIdx.y = part of gridDim.y: the entries of an image with many kept rows are shared out (every part repeats the prologue;
  // part 0 writes the counters).  One part per image in the small-image regime.
  const int part = blockIdx.y, nparts = gridDim.y;
  // The kernel is a chain of dependent global reads (counts -> kept positions -> keys / slots -> candidate rows); everything
  // that does not depend on an earlier read is requested up front: seven latencies became four.
  // kept per segment (clipped to max_det: a class contributes at most max_det rows to the first max_det overall)
  for (int c = tid; c < ncs; c += 256) {
    long long k = keep_cnt[g * ncs + c];
    if (max_det > 0 && k > max_det) k = max_det;
    s_pre[c + 1] = (int)k;
    s_seg[c] = seg_begin[g * ncs + c];
  }
  if (tid == 0) s_pre[0] = 0;
  // (packed) rows of the images before this one; (workgroup 0) the largest candidate count -- same round trip as above
  long long mine = 0, mx = 0;
  int tf = 0;
  if (packed) {
    for (int b2 = tid; b2 < g; b2 += 256) {
      long long t = 0;
      for (int c = 0; c < ncs; c++) { long long k = keep_cnt[b2 * ncs + c]; if (max_det > 0 && k > max_det) k = max_det; t += k; }
      if (max_det > 0 && t > max_det) t = max_det;
      mine += t;
    }
  }
  if (g == 0)
    for (int b2 = tid; b2 < (int)gridDim.x; b2 += 256) {
      const long long c = cnt[b2 * kCntPad];
      if (c > mx) mx = c;
      const int t = tiny[b2];
      tf |= t & kImgSmall;
      if ((t & kImgSmall) && !img_single_list(t)) tf |= 16;      // ... and kept its class segments (k_tiny_cross vouched for it)
    }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) { mine += __shfl_xor(mine, d); const long long o = __shfl_xor(mx, d); if (o > mx) mx = o; tf |= __shfl_xor(tf, d); }
  if ((tid & 63) == 0) { s_rows[tid >> 6] = mine; s_mx[tid >> 6] = mx; s_tf[tid >> 6] = tf; }
  __syncthreads();
  if (tid == 0) for (int c = 0; c < ncs; c++) s_pre[c + 1] += s_pre[c];
  __syncthreads();
  const int total = s_pre[ncs];
  if (tid == 0 && part == 0) {
    long long nk = total;
    if (max_det > 0 && nk > max_det) nk = max_det;
    out_count[g] = *abort_flag ? -1 : nk;                        // -1: the NMS kernel gave up on a barrier (host raises)
  }
  // status[0]: the largest candidate count if an image overflowed its slots (the caller retries), else 0; status[1]: the largest
  // candidate count (feedback for the caller's next call).  Plain stores by one workgroup -- out_count and status may be pinned
  // host memory (the host layer reads them without a device->host copy).
  if (g == 0 && tid == 0 && part == 0) {
    long long m4 = s_mx[0];
    for (int k = 1; k < 4; k++) if (s_mx[k] > m4) m4 = s_mx[k];
    // info[8] != 0: k_nms_small met a segment above its limit -- nothing of this call is valid, the caller repeats it with
    // the persistent kernel (status[0] = -1); info[4]: the largest NMS segment where the sort kernel knew it (else 0)
    status[0] = info[8] ? -1 : (m4 > cap_img ? m4 : 0);
    // bit 62: an image of this call held short-sided boxes (kImgSmall) -- the caller's next call asks for k_tiny_cross;
    // bit 61: such an image kept its class segments in THIS call (informational)
    const int tfa = s_tf[0] | s_tf[1] | s_tf[2] | s_tf[3];
    const long long small_seen = ((tfa & kImgSmall) ? (1ll << 62) : 0ll) | ((tfa & 16) ? (1ll << 61) : 0ll);
    status[1] = m4 | (((long long)(info[8] > info[4] ? info[8] : info[4]) & 0x1fffffffll) << 32) | small_seen;
  }
  // caller-kept counters (obb_non_max_suppression_obb_st) are left zeroed for the next call: this workgroup was their last
  // reader whose reading matters (the other parts of image 0 read them too, but only this one writes the status words)
  if (clean_cnt != nullptr && g == 0 && part == 0)
    for (int b2 = tid; b2 < (int)gridDim.x; b2 += 256) { clean_cnt[b2 * kCntPad] = 0; clean_tiny[b2] = 0; }
  // first output row of the image: g * max_det, or (packed) the number of rows of the images before it
  const long long row0 = packed ? s_rows[0] + s_rows[1] + s_rows[2] + s_rows[3] : (long long)g * max_det;
  const int md = mode[g];
  const bool single = md == 0;
  // merge key of entry e = (class c, index k): the mode-1 key rotated so that it orders by (score, anchor, class)
  auto entry_pos = [&](int c, int k) -> uint32_t { return (uint32_t)keep[(size_t)s_seg[c] + k]; };
  auto mkey_at = [&](uint32_t p) -> unsigned long long {
    const unsigned long long k = keys_sorted[p];
    return md == 1 ? ((k << 8) | (k >> 56)) : k;
  };
  const bool in_lds = total <= kMergeLds;
  if (!single && in_lds) {
    for (int e = tid; e < total; e += 256) {
      int c = 0;
      while (s_pre[c + 1] <= e) c++;
      const uint32_t p = entry_pos(c, e - s_pre[c]);
      s_key[e] = mkey_at(p);
      s_val[e] = vals_sorted[p];
    }
    __syncthreads();
  }
  for (int e = tid + 256 * part; e < total; e += 256 * nparts) {
    int c = 0;
    while (s_pre[c + 1] <= e) c++;
    const int k = e - s_pre[c];
    const bool staged = !single && in_lds;                      // key and slot of the entry are in LDS
    const uint32_t p = staged ? 0u : entry_pos(c, k);
    long long rank = k;
    if (!single) {
      const unsigned long long mk = in_lds ? s_key[e] : mkey_at(p);
      for (int c2 = 0; c2 < ncs; c2++) {
        if (c2 == c) continue;
        int lo = 0, hi = s_pre[c2 + 1] - s_pre[c2];
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          const unsigned long long mk2 = in_lds ? s_key[s_pre[c2] + mid] : mkey_at(entry_pos(c2, mid));
          if (mk2 < mk) lo = mid + 1; else hi = mid;
        }
        rank += lo;
      }
    }
    if (max_det > 0 && rank >= max_det) continue;
    const size_t ci = (size_t)g * cap_img + (staged ? s_val[e] : vals_sorted[p]);
    const float4 c0 = cand[ci * 2], c1 = cand[ci * 2 + 1];
    float* o = out + ((size_t)row0 + rank) * 7;
    o[0] = c0.x; o[1] = c0.y; o[2] = c0.z; o[3] = c0.w; o[4] = c1.x; o[5] = c1.y; o[6] = c1.z;
  }
}

// The FRONT of k_nms_small without a sort launch (round 6, fourth part).  At the reference's default thresholds an image holds a few
// thousand candidates in ~16 classes: k_sort_prep_lds spent 17 us (+ its launch) on four workgroups per image ordering what the 256
// segment workgroups of the NMS launch can order themselves -- every workgroup reads its image's keys (8 bytes per candidate, from
// L2), keeps the candidates of ITS class (the class is the key's tie word modulo nc; label rows carry it in their record), ranks
// them by counting (keys are unique: the rank is the place; <= 384 members, the keys broadcast from LDS two at a time) and builds
// records, alive bits (nms_rotated_wrapper.py:32) and publishing keys where the pair phase wants them: in LDS.  Same keys, same
// order, same records as the sort kernel's (k_sort_prep_lds: "by_class"); an image that keeps ONE list (img_single_list, more than
// max_nms candidates) is segment 0's if it fits.  What does not fit a segment raises too_big like a segment of the sort's: the caller
// repeats the call on the persistent kernel.
// (the front end's alternatives -- fewer keys per thread and trip, the first trip requested after the image's counter, the rank
//  count one read at a time -- were measured within 1 us of this form on the bs16 step and not kept)
struct SmallSelfSort {
  static constexpr bool kSelf = true;
  // an image's candidate count, its top-max_nms cut and its mode exactly as k_sort_prep_lds decides them (class_ok holds: the
  // small-segment kernel is only chosen with it)
  static __device__ __forceinline__ int image_mode(long long c, int tf, long long cap_img, long long max_nms, int& n, int& e) {
    const bool over_cap = c > cap_img;
    if (over_cap) c = cap_img;
    if (c > kSortLdsMax) c = 0;                                  // not this path's regime: reported through status[1]
    const bool over_nms = max_nms > 0 && c > max_nms;
    e = (int)(over_nms ? max_nms : c);                           // :845-846
    n = (int)c;
    return (!over_cap && !img_single_list(tf) && !over_nms) ? 1 : 0;
  }
  // returns boxes of the segment (> kSmallMax: too many, nothing was built) | mode of the image << 16
  template <class G>
  static __device__ __forceinline__ int load(const SmallArgs& a, int seg, float4* s_rec, u64* s_mask, unsigned long long* s_pk,
                                                       uint32_t* s_pv, int* s_n) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int g = seg / a.ncs, c = seg - g * a.ncs;
    constexpr int KPT = 8;                                       // keys per thread and trip
    const size_t b0 = (size_t)g * (size_t)a.cap_img;
    // the first trip's keys are requested TOGETHER with the image's counter (slots behind the count hold stale keys of the
    // workspace: read, never used) -- one round trip less in front of every segment
    const int spec = a.cap_img < (long long)KPT * kSmallThreads ? (int)a.cap_img : KPT * kSmallThreads;
    unsigned long long k[KPT];
#pragma unroll
    for (int u = 0; u < KPT; u++) { const int i = u * kSmallThreads + tid; k[u] = i < spec ? a.keys_in[b0 + i] : 0ull; }
    int n, e;
    const int m = image_mode(a.cnt[g * kCntPad], a.tiny[g], a.cap_img, a.max_nms, n, e);
    if (n == 0 || (m == 0 && c != 0)) return m << 16;            // (workgroup-uniform)
    u64* s_alive = s_mask + (size_t)kSmallMax * kSmallWords;
    unsigned long long* st_key = reinterpret_cast<unsigned long long*>(s_mask);        // staged members: the bit matrix is not in use yet
    uint32_t* st_slot = reinterpret_cast<uint32_t*>(st_key + kSmallMax);
    if (tid == 0) *s_n = 0;
    if (tid < 8) s_alive[tid] = 0ull;
    __syncthreads();
    const uint32_t nc = (uint32_t)a.nc, lim = (uint32_t)((unsigned long long)a.A * nc);   // (A * nc + label rows < 2^32: checked by the launcher)
    for (int i0 = 0; i0 < n; i0 += KPT * kSmallThreads) {        // (workgroup-uniform trip count: ballots inside)
      if (i0 > 0) {
#pragma unroll
        for (int u = 0; u < KPT; u++) { const int i = i0 + u * kSmallThreads + tid; k[u] = i < n ? a.keys_in[b0 + i] : 0ull; }
      }
#pragma unroll
      for (int u = 0; u < KPT; u++) {
        const int i = i0 + u * kSmallThreads + tid;
        if (i0 + u * kSmallThreads >= n) break;                  // (workgroup-uniform)
        bool mine = false;
        unsigned long long nk = k[u];
        if (i < n) {
          if (m == 1) {                                          // k_rekey: (cls << 56 | score_desc << 24 | anchor)
            const uint32_t tie = (uint32_t)k[u];
            uint32_t cls, anchor;
            if (tie < lim) { anchor = tie / nc; cls = tie - anchor * nc; }
            else { cls = (uint32_t)(int)a.cand[(b0 + i) * 2 + 1].z; anchor = (uint32_t)a.A + (tie - lim); }     // (an apriori label row)
            mine = cls == (uint32_t)c;
            nk = ((unsigned long long)cls << 56) | ((k[u] >> 32) << 24) | (unsigned long long)(anchor & 0xffffffu);
          } else mine = true;
        }
        const u64 mk = __ballot(mine);
        if (mk) {                                                // (wave-uniform)
          int base = 0;
          if (lane == 0) base = atomicAdd(s_n, __popcll(mk));
          base = __shfl(base, 0);
          const int at = base + __popcll(mk & lanemask_lt());
          if (mine && at < kSmallMax) { st_key[at] = nk; st_slot[at] = (uint32_t)i; }
        }
      }
    }
    __syncthreads();
    const int nm = *s_n;
    if (nm > kSmallMax) return (nm > 0xffff ? 0xffff : nm) | (m << 16);
    const int ec = (m == 1 || nm < e) ? nm : e;                  // one list: the first max_nms by key
    if (tid == 0 && nm > 0) atomicMax(a.seg_max, ec);
    if (tid < nm) {
      const unsigned long long mine = st_key[tid];
      const uint32_t slot = st_slot[tid];
      const size_t ci = b0 + slot;
      const float4 c0 = a.cand[ci * 2], c1 = a.cand[ci * 2 + 1]; // under way during the count
      int rank = 0, j = 0;
      const ulonglong2* p2 = reinterpret_cast<const ulonglong2*>(st_key);
      for (; j + 16 <= nm; j += 16) {                                           // eight 16-byte broadcast reads in flight (one at a time: 64 cycles each)
        ulonglong2 v[8];
#pragma unroll
        for (int z = 0; z < 8; z++) v[z] = p2[(j >> 1) + z];
#pragma unroll
        for (int z = 0; z < 8; z++) rank += (v[z].x < mine ? 1 : 0) + (v[z].y < mine ? 1 : 0);
      }
      for (; j + 2 <= nm; j += 2) { const ulonglong2 v = p2[j >> 1]; rank += (v.x < mine ? 1 : 0) + (v.y < mine ? 1 : 0); }
      if (j < nm) rank += st_key[j] < mine ? 1 : 0;
      if (rank < ec) {
        s_pk[rank] = mine; s_pv[rank] = slot;
        const float coff = c1.z * a.class_offset;                // :849
        const RBoxFeat f = rbox_make_feat(c0.x + coff, c0.y + coff, c0.z, c0.w, c1.x);
        float4 rq[4];
        G::pack(f, rq);
#pragma unroll
        for (int u = 0; u < 4; u++) s_rec[rank * G::RECQ + u] = rq[u];
        if (!box_too_small(c0.z, c0.w)) atomicOr(&s_alive[rank >> 6], 1ull << (rank & 63));        // nms_rotated_wrapper.py:32
      }
    }
    __syncthreads();                                             // the staged members are read: their place becomes the bit matrix
    for (int t = tid; t < ec * kSmallWords; t += kSmallThreads) s_mask[t] = 0ull;
    return ec | (m << 16);
  }
};

// The same output stage INSIDE k_nms_small (its TAIL): the segments of an image count themselves on a ticket and the workgroup
// that arrives last merges the image's kept lists and writes its rows -- the launch of k_gather_out, its start-up and two of its
// four dependent round trips (kept positions -> keys / slots: the segments publish merge keys and slots themselves) are gone
// from the step.  Rows of image g start at g * max_det (a packed output needs the totals of ALL earlier images: that stays with
// k_gather_out).  The image that finishes last writes the two status words.  No workgroup waits for another one.
struct SmallGather {
  struct Args {
    const float4* cand; const int* cnt; const int* tiny; const int* info;
    int* ticket;               // [bs] segments of the image that are done, then [1] images that are done (zeroed by k_reset_state or k_decode)
    float* out; int64_t* out_count; int64_t* status;
    long long cap_img, max_det;
    int bs;
    int* clean_cnt; int* clean_tiny;   // caller-kept counters to leave zeroed (obb_non_max_suppression_obb_st), or NULL
  };
  static constexpr int kLds = kSortLdsMax;                       // entries staged in LDS: an image of the in-LDS sort has no more candidates
  static constexpr size_t kLdsBytes = 2064 + (size_t)kLds * 16;
  static __device__ __forceinline__ void run(const SmallArgs& a, const Args& ga, unsigned char* s_raw, int seg) {
    __shared__ int s_flag, s_maxc;
    const int tid = threadIdx.x, lane = tid & 63, ncs = a.ncs, g = seg / ncs;
#ifdef OBB_SMALL_TRACE
    unsigned long long tt[10]; int ti_ = 0;
#define GSTAMP() do { tt[ti_++] = wall_clock64(); } while (0)
#else
#define GSTAMP() do {} while (0)
#endif
    GSTAMP();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");            // this wave's published entries are written through
    __syncthreads();
    // The stage is a chain of dependent round trips (~1 us each), so everything is requested as early as its address is known:
    // thread (c, k) of the first `spec` threads per segment asks for the k-th published entry of segment c TOGETHER with the
    // segment's count (most segments keep fewer than `spec` boxes: no second trip); the segment's first position comes from the
    // sort kernel and is requested while the ticket is under way.
    int spec = 2;
    while (spec * 2 * ncs <= kSmallThreads) spec <<= 1;          // (ncs <= 256)
    const int myc = tid / spec, myk = tid - myc * spec;
    const bool mine = myc < ncs;
    const bool self = a.keys_in != nullptr;                      // (kernel-uniform) self-sorting segments publish at fixed places
    // (the image's mode: from its counter, read BEFORE this workgroup arrives -- the image that is done last zeroes the counters)
    int single_self = 0;
    if (self) { int n_, e_; single_self = SmallSelfSort::image_mode(ga.cnt[g * kCntPad], ga.tiny[g], ga.cap_img, a.max_nms, n_, e_) == 0 ? 1 : 0; }
    asm volatile("" : "+v"(single_self));
    const int sb_c = !mine ? 0 : (self ? (int)((long long)g * ga.cap_img) + myc * kSmallMax : a.seg_begin[g * ncs + myc]);
    int t2 = -1;                                                 // (thread 0) images that were done before this one
    if (tid == 0) {
      const int last = __hip_atomic_fetch_add(ga.ticket + g, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == ncs - 1 ? 1 : 0;
      // every segment of this image is done -- the image counts as done for the status words (which do not wait for its rows)
      if (last) t2 = __hip_atomic_fetch_add(ga.ticket + ga.bs, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      s_flag = last;
    }
    __syncthreads();
    if (!s_flag) return;                                         // (workgroup-uniform)
    GSTAMP();
    // ---- the image's output (the segment state in s_raw is dead).  What other workgroups of this launch wrote is read with
    // agent-scope loads (they wrote it through); the rest comes from earlier launches.
    int* s_pre = reinterpret_cast<int*>(s_raw);                  // [257]
    int* s_seg = s_pre + 260;                                    // [256]
    unsigned long long* s_key = reinterpret_cast<unsigned long long*>(s_raw + 2064);
    uint32_t* s_val = reinterpret_cast<uint32_t*>(s_key + kLds);
    uint32_t* s_ck = s_val + kLds;                               // (segment << 16 | index in its list) of a staged entry
    const long long max_det = ga.max_det;
    int cnt_c = 0;
    unsigned long long key = 0ull;
    uint32_t val = 0u;
    if (mine) {
      cnt_c = ldg_agent(a.keep_cnt + g * ncs + myc);
      size_t p = (size_t)sb_c + myk;
      if (p >= (size_t)a.n_pos) p = (size_t)a.n_pos - 1;        // (beyond the segment's count the entry is not used)
      val = ldg_agent(a.pub_val + p);
      key = ldg_agent(a.pub_key + p);
    }
    // (wave 0) the inputs of the status words come from earlier launches: under way during the trips above
    long long mx = 0;
    int tf = 0, big = 0;
    if (tid < 64) {
      for (int b2 = lane; b2 < ga.bs; b2 += 64) {
        const long long c = ga.cnt[b2 * kCntPad];
        if (c > mx) mx = c;
        const int t = ga.tiny[b2];
        tf |= t & kImgSmall;
        if ((t & kImgSmall) && !img_single_list(t)) tf |= 16;
      }
      // the image that is done last reads the too-big word now: every segment of every image has arrived
      if (tid == 0 && t2 == ga.bs - 1) big = ldg_agent(ga.info + 8);
    }
    if (max_det > 0 && cnt_c > max_det) cnt_c = (int)max_det;   // a class contributes at most max_det rows to the first max_det overall
    if (mine && myk == 0) { s_pre[myc + 1] = cnt_c; s_seg[myc] = sb_c; }
    if (tid == 0) s_pre[0] = 0;
    const int more = __syncthreads_or(cnt_c > spec ? 1 : 0);
    if (tid < 64) {                                              // inclusive scan of s_pre[1 .. ncs], four per lane (ncs <= 256), and the largest
      int v[4], sum = 0, m = 0;
#pragma unroll
      for (int j = 0; j < 4; j++) { const int c = lane * 4 + j; v[j] = c < ncs ? s_pre[c + 1] : 0; sum += v[j]; m = v[j] > m ? v[j] : m; }
      int inc = sum;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(inc, d); if (lane >= d) inc += t; }
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) { const int o = __shfl_xor(m, d); m = o > m ? o : m; }
      int run = inc - sum;
#pragma unroll
      for (int j = 0; j < 4; j++) { const int c = lane * 4 + j; run += v[j]; if (c < ncs) s_pre[c + 1] = run; }
      if (lane == 0) s_maxc = m;
    }
    __syncthreads();
    const int total = s_pre[ncs], maxc = s_maxc;
    GSTAMP();
    if (tid == 0) ga.out_count[g] = (max_det > 0 && total > max_det) ? max_det : (long long)total;
    const bool single = self ? single_self != 0 : a.mode[g] == 0;
    const bool in_lds = total <= kLds;
    auto seg_of = [&](int e) -> int {                            // the segment c with s_pre[c] <= e < s_pre[c + 1]
      int lo = 0, hi = ncs - 1;
      while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (s_pre[mid] <= e) lo = mid; else hi = mid - 1; }
      return lo;
    };
    if (in_lds) {
      if (mine && myk < cnt_c) { const int e = s_pre[myc] + myk; s_val[e] = val; s_key[e] = key; s_ck[e] = ((uint32_t)myc << 16) | (uint32_t)myk; }
      if (more)                                                  // (workgroup-uniform) a segment kept more than `spec` boxes: the rest of it
        for (int e = tid; e < total; e += kSmallThreads) {
          const int c = seg_of(e), k = e - s_pre[c];
          if (k < spec) continue;
          const size_t p = (size_t)s_seg[c] + k;
          s_val[e] = ldg_agent(a.pub_val + p);
          s_key[e] = ldg_agent(a.pub_key + p);
          s_ck[e] = ((uint32_t)c << 16) | (uint32_t)k;
        }
      __syncthreads();
    }
    GSTAMP();
    // rank of an entry = its index in its own list + the entries of every other list in front of it (binary searches on the
    // merge keys); up to 16 lanes share the lists of one entry when the image has few entries.  A lane runs the searches of eight
    // lists in lock step (same number of halving steps for all: the loads of a step are independent of each other).
    int tpe = 1;
    if (!single) while (tpe < 16 && total * tpe * 2 <= kSmallThreads) tpe <<= 1;
    int top = 1;
    while (top * 2 <= maxc) top <<= 1;                           // the largest power of two <= the longest list
    const int sub = tid & (tpe - 1), per_round = kSmallThreads / tpe, nlist = (ncs + tpe - 1) / tpe;
    for (int e0 = 0; e0 < total; e0 += per_round) {
      const int e = e0 + tid / tpe;
      const bool valid = e < total;
      int c = 0, k = 0, rank = 0;
      if (valid) {
        if (in_lds) { const uint32_t ck = s_ck[e]; c = (int)(ck >> 16); k = (int)(ck & 0xffffu); }
        else { c = seg_of(e); k = e - s_pre[c]; }
      }
      const bool writer = valid && sub == 0;
      float4 c0 = make_float4(0.f, 0.f, 0.f, 0.f), c1 = c0;
      if (writer) {                                              // the row is under way while the rank is computed
        const uint32_t slot = in_lds ? s_val[e] : ldg_agent(a.pub_val + (size_t)s_seg[c] + k);
        const size_t ci = (size_t)g * ga.cap_img + slot;
        c0 = ga.cand[ci * 2]; c1 = ga.cand[ci * 2 + 1];
      }
      GSTAMP();
      if (valid && !single) {
        if (in_lds) {
          const unsigned long long mk = s_key[e];
          for (int j0 = 0; j0 < nlist; j0 += 8) {
            int base[8], len[8], pos[8];
#pragma unroll
            for (int j = 0; j < 8; j++) {
              const int c2 = sub + (j0 + j) * tpe;
              const bool ok = c2 < ncs && c2 != c;
              base[j] = ok ? s_pre[c2] : 0;
              len[j] = ok ? s_pre[c2 + 1] - base[j] : 0;
              pos[j] = 0;
            }
            for (int st = top; st >= 1; st >>= 1) {
              unsigned long long k2[8];                          // (all eight loads first: written as one conditional per list the
#pragma unroll                                                   //  compiler branches around each load and waits for it in turn)
              for (int j = 0; j < 8; j++) {
                const int q = pos[j] + st;
                int at = base[j] + (q <= len[j] ? q : len[j]) - 1;
                at = at < 0 ? 0 : at;
                k2[j] = s_key[at];
              }
#pragma unroll
              for (int j = 0; j < 8; j++) {
                const int q = pos[j] + st;
                const bool take = (q <= len[j]) & (k2[j] < mk);
                pos[j] = take ? q : pos[j];
              }
            }
#pragma unroll
            for (int j = 0; j < 8; j++) rank += pos[j];
          }
        } else {
          const unsigned long long mk = ldg_agent(a.pub_key + (size_t)s_seg[c] + k);
          for (int c2 = sub; c2 < ncs; c2 += tpe) {
            if (c2 == c) continue;
            int lo = 0, hi = s_pre[c2 + 1] - s_pre[c2];
            while (lo < hi) {
              const int mid = (lo + hi) >> 1;
              if (ldg_agent(a.pub_key + (size_t)s_seg[c2] + mid) < mk) lo = mid + 1; else hi = mid;
            }
            rank += lo;
          }
        }
      }
      GSTAMP();
      for (int d = 1; d < tpe; d <<= 1) rank += __shfl_xor(rank, d);
      rank += k;
#ifdef OBB_SMALL_TRACE
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      GSTAMP();
#endif
      if (!writer || (max_det > 0 && rank >= max_det)) continue;
      float* o = ga.out + ((size_t)g * max_det + rank) * 7;
      o[0] = c0.x; o[1] = c0.y; o[2] = c0.z; o[3] = c0.w; o[4] = c1.x; o[5] = c1.y; o[6] = c1.z;
    }
    GSTAMP();
#ifdef OBB_SMALL_TRACE
    if (tid == 0 && blockIdx.x < 2048) { unsigned long long* o_ = g_small_trace_tail + blockIdx.x * 4; o_[0] = 1ull + (unsigned long long)g; o_[1] = (unsigned long long)total; o_[2] = tt[0]; o_[3] = tt[7]; }
#endif
#undef GSTAMP
    // ---- the call's status words, by the image that was done last (k_gather_out: workgroup 0; see there for their meaning)
    if (tid >= 64) return;
    const int writes = __shfl(t2, 0) == ga.bs - 1;               // (wave-uniform)
    if (!writes) return;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { const long long o = __shfl_xor(mx, d); if (o > mx) mx = o; tf |= __shfl_xor(tf, d); }
    // (the counters were read above; the images still at work on their rows do not use theirs)
    if (ga.clean_cnt != nullptr)
      for (int b2 = lane; b2 < ga.bs; b2 += 64) { ga.clean_cnt[b2 * kCntPad] = 0; ga.clean_tiny[b2] = 0; }
    if (lane == 0) {
      const int seg4 = ldg_agent(ga.info + 4);                  // (self-sorting segments raise it in this launch)
      ga.status[0] = big ? -1 : (mx > ga.cap_img ? mx : 0);
      const long long small_seen = ((tf & kImgSmall) ? (1ll << 62) : 0ll) | ((tf & 16) ? (1ll << 61) : 0ll);
      ga.status[1] = mx | (((long long)(big > seg4 ? big : seg4) & 0x1fffffffll) << 32) | small_seen;
    }
  }
};
static_assert(SmallGather::kLdsBytes <= (size_t)kSmallMax * RotGeom::RECQ * 16 + (size_t)kSmallMax * kSmallWords * 8 + 64 + sizeof(SmallWave<RotGeom>) * kSmallWaves,
              "SmallGather: the merge lists live where the segment state was");

static inline size_t obb_state_bytes(int64_t bs) { return align_up((size_t)bs * kCntPad * 4 + (size_t)bs * 4); }   // cnt lines + tiny flags

struct ObbCarve {
  float4* cand; unsigned long long *keys_a, *keys_b; uint32_t *vals_a, *vals_b; int* cnt; int *sort_begin, *sort_end;
  int *img_end, *mode, *tiny, *ticket;
  uint32_t* srs_hist;
  int* seg_size;      // [bs][256] segment sizes for the planner of the in-LDS sort path
  int64_t* keep;
  Carve nms;          // rec/dead/segment state reuse the NMS carve (keys/vals/sort_tmp of it unused)
  size_t total;
};

static inline int64_t round_cap(int64_t cap_img) { return (cap_img + 63) / 64 * 64; }   // image regions start on alive-bitmap words

static ObbCarve obb_carve(void* base, int64_t bs, int64_t cap_img, int64_t ncs, int cus) {
  cap_img = round_cap(cap_img);
  ObbCarve cv{};
  WsCursor w(base);
  const size_t n = (size_t)bs * cap_img;
  cv.cand = w.take<float4>(n * 2);
  cv.keys_a = w.take<unsigned long long>(n); cv.keys_b = w.take<unsigned long long>(n);
  cv.vals_a = w.take<uint32_t>(n); cv.vals_b = w.take<uint32_t>(n);
  cv.cnt = w.take<int>(bs * kCntPad); cv.sort_begin = w.take<int>(bs); cv.sort_end = w.take<int>(bs);
  cv.img_end = w.take<int>(bs); cv.mode = w.take<int>(bs); cv.tiny = w.take<int>(bs);
  cv.ticket = w.take<int>(16 + (size_t)(bs + 1));            // 16 words + k_nms_small's output stage: [bs] + [1]
  cv.seg_size = w.take<int>((size_t)bs * 256);
  cv.srs_hist = w.take<uint32_t>((size_t)bs * ((size_t)(cap_img + kSrsTile - 1) / kSrsTile) * 256);
  cv.keep = w.take<int64_t>(n);
  // NMS state sized for bs * cap_img positions
  w.nest([&](void* b) { return (cv.nms = carve(b, (int64_t)n, bs * ncs, RotGeom::RECQ, cap_max(bs * ncs), cus)).total; });
  cv.total = w.total();
  return cv;
}

// ---------------------------------------------------------------- the fused driver
// One call, by name.  The front is ONE of: pred (+ objcol, the dense objectness column a coupled Detect decode left, or NULL);
// head: the candidates come from the conv outputs it describes (k_decode_head) and pred / objcol are not read; tta: from the
// (pass, level) entries of augmented inference (k_decode_head<T, true>), likewise.
struct NmsObbCall {
  const void* pred = nullptr; const void* objcol = nullptr;
  const HeadFront* head = nullptr; const HeadFrontTta* tta = nullptr;
  int dtype = 0;
  int64_t bs = 0, A = 0, no = 0;
  float conf_thres = 0.f, iou_thres = 0.f;
  const int32_t* classes_host = nullptr; int n_classes = 0;
  int agnostic = 0, multi_label = 0;
  int64_t max_det = 0, max_nms = 0;
  float max_wh = 0.f;
  const float* extra8 = nullptr; int64_t n_extra = 0;      // the apriori label rows
  int64_t cap_img = 0, expected_cand = 0;
  float* out = nullptr; int out_packed = 0; int64_t* out_count = nullptr; int64_t* status = nullptr;
  void* ws = nullptr; size_t ws_bytes = 0;
  void* state = nullptr; size_t state_bytes = 0;            // caller-kept counters (obb_non_max_suppression_obb_st), or NULL
  hipStream_t stream = nullptr;
};

// what the C entries of the fused driver have in common (nms.hip); each adds its front, and its state block if it takes one
static NmsObbCall nms_obb_call(int dtype, int64_t bs, int64_t A, int64_t no, float conf_thres, float iou_thres, const int32_t* classes_host,
                               int n_classes, int agnostic, int multi_label, int64_t max_det, int64_t max_nms, float max_wh,
                               const float* extra8, int64_t n_extra, int64_t cap_img, int64_t expected_cand, float* out, int out_packed,
                               int64_t* out_count, int64_t* status, void* ws, size_t ws_bytes, void* stream) {
  NmsObbCall c;
  c.dtype = dtype; c.bs = bs; c.A = A; c.no = no; c.conf_thres = conf_thres; c.iou_thres = iou_thres;
  c.classes_host = classes_host; c.n_classes = n_classes; c.agnostic = agnostic; c.multi_label = multi_label;
  c.max_det = max_det; c.max_nms = max_nms; c.max_wh = max_wh; c.extra8 = extra8; c.n_extra = n_extra;
  c.cap_img = cap_img; c.expected_cand = expected_cand; c.out = out; c.out_packed = out_packed ? 1 : 0; c.out_count = out_count;
  c.status = status; c.ws = ws; c.ws_bytes = ws_bytes; c.stream = (hipStream_t)stream;
  return c;
}

// What the steps of a call hand to each other.  Nothing here is allocated: pointers into the caller's workspace, and the plan.
struct NmsObbRun {
  const NmsObbCall& c;
  int nc;                    // :784
  int64_t cap_img;           // rounded (round_cap)
  DeviceCus dc;              // the current device, read once
  ObbCarve cv;
  ObbPlan plan;
  bool kept;                 // caller-kept counters: cv.cnt / cv.tiny live in c.state
  SmallHelpBlocks hb;        // k_nms_small's helper blocks (plan.helpers > 0)
  long long bar16, alive16;  // 16-byte pieces of the barrier block / the alive bitmap that the call's first kernel zeroes
  DecodeArgs d;
};

// ---- 1. argument checks: OBB_ERR_BAD_ARG before the workspace is looked at
static int obb_check_args(const NmsObbCall& c) {
  const int nc = (int)(c.no - 5 - 180);                            // :784
  if (c.bs < 1 || c.A < 1 || nc < 1 || nc > 256 || c.max_det < 1 || c.cap_img < 1 || (!c.pred && !c.head && !c.tta) || !c.out ||
      !c.out_count || !c.status)
    return OBB_ERR_BAD_ARG;
  if (c.A * nc + c.n_extra > 0xffffffffLL || c.bs * c.cap_img > 0x7fffffffLL) return OBB_ERR_BAD_ARG;
  if (!dtype_known(c.dtype)) return OBB_ERR_BAD_ARG;
  return OBB_OK;
}

// ---- 2. the workspace layout and its size check
static int obb_carve_call(NmsObbRun& r) {
  const NmsObbCall& c = r.c;
  r.nc = (int)(c.no - 5 - 180);
  r.cap_img = round_cap(c.cap_img);
  r.dc = device_cus();
  r.cv = obb_carve(c.ws, c.bs, r.cap_img, c.agnostic ? 1 : r.nc, r.dc.cus);
  return ws_ok(c.ws, c.ws_bytes, r.cv.total) ? OBB_OK : OBB_ERR_WORKSPACE;
}

// ---- 3. the call's path (nms_plan.h): every choice of the later steps reads a field of the plan.  The caller-kept counters are
// bound here, behind the plan, where their size has always been checked.
static int obb_plan_call(NmsObbRun& r) {
  const NmsObbCall& c = r.c;
  ObbCarve& cv = r.cv;
  ObbPlanIn pin{};
  pin.bs = c.bs; pin.A = c.A; pin.nc = r.nc; pin.agnostic = c.agnostic; pin.multi_label = c.multi_label; pin.iou_thres = c.iou_thres; pin.max_wh = c.max_wh;
  pin.n_extra = c.n_extra; pin.cap_img = r.cap_img; pin.max_nms = c.max_nms; pin.max_det = c.max_det; pin.expected_cand = c.expected_cand;
  pin.out_packed = c.out_packed; pin.hw_cus = r.dc.hw_cus; pin.cus = r.dc.cus; pin.ecap = cv.nms.ecap;
  pin.sort_tmp_bytes = cv.nms.sort_tmp_bytes; pin.ps_scratch_bytes = ps_scratch_bytes();
  r.plan = plan_nms_obb(pin, nms_env());
  // caller-kept counters: zero when the call starts (the caller's memset, or the previous call's last kernel) -- no reset launch
  r.kept = c.state != nullptr;
  if (r.kept) {
    if (!ws_ok(c.state, c.state_bytes, obb_state_bytes(c.bs))) return OBB_ERR_WORKSPACE;
    cv.cnt = (int*)c.state;
    cv.tiny = cv.cnt + c.bs * kCntPad;
  }
  // k_nms_small's helper blocks live in the persistent kernel's edge lists, which that path does not use (the plan has checked the fit)
  r.hb = SmallHelpBlocks{};
  if (r.plan.helpers > 0) { WsCursor w(cv.nms.edges); r.hb = small_help_layout(w, r.plan.helpers, c.bs * r.plan.ncs, c.bs * r.cap_img); }
  return OBB_OK;
}

// ---- 4. the front kernel's arguments: class filter, candidate blocks, and the state of the later launches it zeroes on its way
static void obb_fill_decode(NmsObbRun& r) {
  const NmsObbCall& c = r.c;
  const ObbCarve& cv = r.cv;
  DecodeArgs& d = r.d;
  d.pred = c.pred; d.objcol = c.objcol; d.A = c.A; d.no = (int)c.no; d.nc = r.nc; d.bs = (int)c.bs; d.conf_thres = c.conf_thres;
  d.multi_label = r.plan.multi_label;
  d.rows_per_thread = r.plan.rows_per_thread;
  class_mask_fill(c.classes_host, c.n_classes, d.cm.w, &d.cm.all);
  d.cap_img = r.cap_img; d.cand = cv.cand; d.keys = cv.keys_a; d.vals = cv.vals_a; d.cnt = cv.cnt; d.tiny = cv.tiny;
  d.win_lo = -0.35f * c.max_wh; d.win_hi = 0.6f * c.max_wh;        // 0.95 max_wh wide: circles of different classes cannot touch
  // (cap_img is a multiple of 64 -> bs * cap_img / 64 words; + the guard words, rounded up to 16 bytes)
  // only what the planned path reads (plan.zero_bar / zero_alive): the headline's self-sorting segments need neither block
  r.alive16 = r.plan.zero_alive ? (long long)((((size_t)c.bs * r.cap_img) >> 6) + 8 + 1) / 2 : 0ll;
  r.bar16 = r.plan.zero_bar ? (long long)(cv.nms.bar_bytes / 16) : 0ll;
  d.z_ticket = nullptr; d.n_ticket = 0; d.z_bar16 = nullptr; d.n_bar16 = 0; d.z_alive16 = nullptr; d.n_alive16 = 0;
  if (r.kept) {                                                    // the filter kernel zeroes what the later launches need
    d.z_ticket = cv.ticket; d.n_ticket = (int)(16 + c.bs + 1);
    d.z_bar16 = r.bar16 ? reinterpret_cast<uint4*>(cv.nms.bar) : nullptr; d.n_bar16 = r.bar16;
    d.z_alive16 = r.alive16 ? reinterpret_cast<uint4*>(cv.nms.alive) : nullptr; d.n_alive16 = r.alive16;
  }
}

// ---- 5. the front: the reset launch of a call without caller-kept counters, the filter kernel of the call's front, the label
// rows, and the cross-class check of short-sided boxes when the previous call met some
static int obb_front_stage(NmsObbRun& r) {
  const NmsObbCall& c = r.c;
  const ObbCarve& cv = r.cv;
  const DecodeArgs& d = r.d;
  hipStream_t st = c.stream;
  if (!r.kept)
    k_reset_state<<<256, 256, 0, st>>>(cv.cnt, (int)(c.bs * kCntPad), cv.tiny, (int)c.bs, c.status, cv.ticket, (int)(16 + c.bs + 1),
                                       reinterpret_cast<uint4*>(cv.nms.bar), r.bar16, reinterpret_cast<uint4*>(cv.nms.alive), r.alive16);
  dim3 gd((unsigned)((c.A + kDecThreads * d.rows_per_thread - 1) / (kDecThreads * d.rows_per_thread)), (unsigned)c.bs);
  {
    ProfScope ps(PROF_DECODE, st);
    if (c.head || c.tta) {
      const int rc = c.head ? launch_decode_head(*c.head, d, c.dtype, r.dc.dev, st) : launch_decode_head_tta(*c.tta, d, c.dtype, r.dc.dev, st);
      if (rc) return rc;
    } else OBB_DISPATCH_DTYPE(c.dtype, T, k_decode<T><<<gd, kDecThreads, 0, st>>>(d));
  }
  if (c.n_extra > 0 && c.extra8) k_append_extra<<<(unsigned)((c.n_extra + 255) / 256), 256, 0, st>>>(c.extra8, (int)c.n_extra, c.A, r.nc, d);
  if (r.plan.small_hint && r.plan.class_ok)
    k_tiny_cross<<<dim3(kTinyParts, (unsigned)c.bs), 256, 0, st>>>(cv.cand, cv.keys_a, cv.cnt, r.cap_img, c.max_wh, c.iou_thres, cv.tiny);
  return OBB_OK;
}

// ---- 6. the sort stage: nothing (k_nms_small orders its segments itself), the in-LDS sort with segment table and records in one
// launch, or segment bookkeeping + radix / three-launch sort + class bounds + records
static int obb_sort_stage(NmsObbRun& r) {
  const NmsObbCall& c = r.c;
  const ObbCarve& cv = r.cv;
  const Carve& nv = cv.nms;
  const ObbPlan& plan = r.plan;
  const SmallHelpBlocks& hb = r.hb;
  hipStream_t st = c.stream;
  const int64_t bs = c.bs, A = c.A, cap_img = r.cap_img, max_nms = c.max_nms;
  const int nc = r.nc, ncs = plan.ncs, class_ok = plan.class_ok, helpers = plan.helpers, agnostic = c.agnostic;
  const float max_wh = c.max_wh;
  if (plan.self_sort) return OBB_OK;                              // no sort launch: k_nms_small orders its segments itself
  if (plan.lds_sort) {
    ProfScope ps(PROF_SEGSORT, st);
    static OncePerDevice attr;
    const size_t lds = (size_t)kSortLdsMax * 12;
    if (!raise_lds_once_on(r.dc.dev, attr, lds, k_sort_prep_lds)) return OBB_ERR_LAUNCH;
    k_sort_prep_lds<<<(unsigned)(bs * plan.parts) + (plan.plan_nb > 0 ? 1u : 0u), 1024, lds, st>>>(cv.cand, cv.keys_a, cv.vals_a, cv.keys_b, cv.vals_b, cv.cnt, cv.tiny, (int)bs, cap_img,
                                                   max_nms, class_ok, A, nc, ncs, agnostic ? 0.f : max_wh, cv.sort_begin, cv.sort_end,
                                                   cv.img_end, cv.mode, nv.seg_begin, nv.seg_end, nv.keep_cnt,
                                                   nv.rec, nv.alive, cv.ticket, plan.plan_nb, plan.plan_chunk, plan.plan_nb > 0 ? nv.plan : nullptr,
                                                   cv.seg_size, plan.parts,
                                                   helpers, hb.work, hb.seg_np, hb.seg_ticket);
    return OBB_OK;
  }
  {
    ProfScope ps(PROF_SEGSORT, st);
    const unsigned gs = (unsigned)((bs + 255) / 256);
    k_cand_segments<<<gs, 256, 0, st>>>(cv.cnt, cv.tiny, (int)bs, cap_img, max_nms, class_ok, cv.sort_begin, cv.sort_end, cv.img_end,
                                        cv.mode);
    if (class_ok) {
      dim3 gr((unsigned)((cap_img + 255) / 256), (unsigned)bs);
      k_rekey<<<gr, 256, 0, st>>>(cv.cand, cv.keys_a, cv.sort_begin, cv.sort_end, cv.mode, A, nc);
    }
    // the radix sort of segsort.h, or the three-launch sort of psrs_sort.h over ONE large image's candidates (nms_plan.h)
    if (plan.psrs) {
      PsBuf b{};
      b.run_k = cv.keys_a; b.run_v = cv.vals_a; b.out_k = cv.keys_b; b.out_v = cv.vals_b;      // (the runs are sorted in place)
      b.n = (int)cap_img; b.n_dev = cv.sort_end; b.err = nullptr;
      ps_carve_scratch(nv.sort_tmp, &b);
      const int runs = (int)((cap_img + kPsRun - 1) / kPsRun);
      k_ps_local_pairs<<<(unsigned)runs, kPsRun, 0, st>>>(b, cv.keys_a, cv.vals_a);
      if (const int rc = ps_finish(b, runs, st)) return rc;
    } else {
      if (const int rc = seg_radix_sort_large(cv.keys_a, cv.keys_b, cv.vals_a, cv.vals_b, cv.sort_begin, cv.sort_end, (int)bs, cap_img, bs * cap_img,
                                              plan.radix_mask, cv.srs_hist, st))
        return rc;
    }
    const int64_t nseg = bs * ncs;
    k_class_bounds<<<(unsigned)((nseg + 255) / 256), 256, 0, st>>>(cv.keys_b, cv.sort_begin, cv.img_end, cv.mode, (int)bs, ncs,
                                                                   nv.seg_begin, nv.seg_end, nv.keep_cnt);
  }
  dim3 gp((unsigned)((plan.max_seg + 255) / 256), (unsigned)bs);
  {
    ProfScope ps(PROF_PREP, st);
    if (hipMemsetAsync(nv.alive, 0, nv.alive_bytes, st) != hipSuccess) return OBB_ERR_LAUNCH;
    k_prep_cand<<<gp, 256, 0, st>>>(cv.cand, cv.vals_b, cv.sort_begin, cv.img_end, cap_img, agnostic ? 0.f : max_wh, nv.rec, nv.alive);
  }
  return OBB_OK;
}

// ---- 7. the NMS stage: k_nms_small (one workgroup per segment; with its output stage inside unless the rows are packed), or
// the persistent kernel
static int obb_nms_stage(NmsObbRun& r) {
  const NmsObbCall& c = r.c;
  const ObbCarve& cv = r.cv;
  const Carve& nv = cv.nms;
  const ObbPlan& plan = r.plan;
  const SmallHelpBlocks& hb = r.hb;
  hipStream_t st = c.stream;
  const int64_t bs = c.bs, cap_img = r.cap_img, max_det = c.max_det;
  const int ncs = plan.ncs, helpers = plan.helpers;
  ProfScope ps(PROF_STEPS, st);
  if (!plan.small_nms) {
    NmsArgs a{};
    nms_args_from(nv, cap_max(bs * ncs), &a);
    a.order = nullptr; a.keep_out = cv.keep; a.n = (int)(bs * cap_img);                  // keep_out: sorted positions
    a.max_keep = (int)max_det; a.window = plan.window; a.thr = c.iou_thres; a.cull = (c.iou_thres >= 0.f) ? 1 : 0;
    return nms_steps(0, a, nv, bs * ncs, bs * plan.max_seg, r.dc, st, kNmsBarZeroed | ((plan.lds_sort && plan.plan_nb > 0) ? kNmsPlanned : 0));
  }
  static OncePerDevice attr;
  const size_t lds = small_lds_bytes<RotGeom>();
  if (!raise_lds_once_on(r.dc.dev, attr, lds, k_nms_small<RotGeom, SmallNoTail>, k_nms_small<RotGeom, SmallGather>, k_nms_small<RotGeom, SmallGather, SmallSelfSort>))
    return OBB_ERR_LAUNCH;
  SmallArgs sa{};
  sa.rec = nv.rec; sa.alive = nv.alive; sa.seg_begin = nv.seg_begin; sa.seg_end = nv.seg_end; sa.keep_cnt = nv.keep_cnt;
  sa.keep_out = cv.keep; sa.too_big = cv.ticket + 8; sa.thr = c.iou_thres; sa.max_keep = (int)max_det;
  sa.ncs = ncs; sa.mode = cv.mode;
  sa.helpers = helpers; sa.help_cnt = cv.ticket + 12; sa.work = hb.work; sa.seg_np = hb.seg_np; sa.seg_ticket = hb.seg_ticket;
  sa.part_main = hb.part_main; sa.part_help = hb.part_help;
  const unsigned gsmall = (unsigned)(bs * ncs + helpers);      // (the helpers are the FIRST blocks: dispatched before the segments' own workgroups)
  if (!plan.fused_out) {
    k_nms_small<RotGeom, SmallNoTail><<<gsmall, kSmallThreads, lds, st>>>(sa, SmallNoTail::Args{});
    return OBB_OK;
  }
  // the output stage runs inside k_nms_small (SmallGather)
  // (keys_a / vals_a, the sort's input, are free: they take what the segments publish)
  sa.keys_sorted = cv.keys_b; sa.vals_sorted = cv.vals_b; sa.pub_key = cv.keys_a; sa.pub_val = cv.vals_a; sa.n_pos = bs * cap_img;
  SmallGather::Args ga{};
  ga.cand = cv.cand; ga.cnt = cv.cnt; ga.tiny = cv.tiny; ga.info = cv.ticket; ga.ticket = cv.ticket + 16;
  ga.out = c.out; ga.out_count = c.out_count; ga.status = c.status; ga.cap_img = cap_img; ga.max_det = max_det; ga.bs = (int)bs;
  ga.clean_cnt = r.kept ? cv.cnt : nullptr; ga.clean_tiny = r.kept ? cv.tiny : nullptr;
  if (plan.self_sort) {
    // (the segments read keys_a, the filter kernel's output, while others publish: keys_b / vals_b, the sort's output places, are free)
    sa.pub_key = cv.keys_b; sa.pub_val = cv.vals_b; sa.keys_sorted = nullptr; sa.vals_sorted = nullptr;
    sa.keys_in = cv.keys_a; sa.cand = cv.cand; sa.cnt = cv.cnt; sa.tiny = cv.tiny; sa.cap_img = cap_img; sa.max_nms = c.max_nms; sa.A = c.A; sa.nc = r.nc;
    sa.class_offset = c.max_wh; sa.seg_max = cv.ticket + 4;
    k_nms_small<RotGeom, SmallGather, SmallSelfSort><<<gsmall, kSmallThreads, lds, st>>>(sa, ga);
  } else {
    k_nms_small<RotGeom, SmallGather><<<gsmall, kSmallThreads, lds, st>>>(sa, ga);
  }
  return OBB_OK;
}

// ---- 8. the output stage, unless k_nms_small had it inside; the call's launch errors are collected here
static int obb_output_stage(NmsObbRun& r) {
  const NmsObbCall& c = r.c;
  const ObbCarve& cv = r.cv;
  hipStream_t st = c.stream;
  if (!r.plan.fused_out) {
    ProfScope ps(PROF_GATHER, st);
    k_gather_out<<<dim3((unsigned)c.bs, r.plan.gparts), 256, 0, st>>>(cv.cand, cv.vals_b, cv.keys_b, cv.keep, cv.nms.seg_begin, cv.nms.keep_cnt, cv.mode, r.plan.ncs, c.max_det,
                                              c.out, c.out_count, cv.cnt, r.cap_img, c.status, cv.nms.abort_flag, c.out_packed, cv.ticket, cv.tiny,
                                              r.kept ? cv.cnt : nullptr, r.kept ? cv.tiny : nullptr);
  }
  return hipGetLastError() == hipSuccess ? OBB_OK : OBB_ERR_LAUNCH;
}

static int run_nms_obb(const NmsObbCall& c) {
  if (const int rc = obb_check_args(c)) return rc;
  NmsObbRun r{c};
  if (const int rc = obb_carve_call(r)) return rc;
  if (const int rc = obb_plan_call(r)) return rc;
  obb_fill_decode(r);
  if (const int rc = obb_front_stage(r)) return rc;
  if (const int rc = obb_sort_stage(r)) return rc;
  if (const int rc = obb_nms_stage(r)) return rc;
  return obb_output_stage(r);
}

}  // namespace obb

