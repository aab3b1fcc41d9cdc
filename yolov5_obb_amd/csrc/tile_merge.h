// In-memory tile -> full-image merge (namespace obb): the device front of run_merge_nms.  The reference hands the per-tile NMS
// outputs to its merge through text (val.py:50-66 save_one_json -> tools/TestJson2VocClassTxt.py ->
// DOTA_devkit/ResultMerge_multi_process.py:183-234 mergesingle); here the rows, the processing order and the segment table of
// obb_merge_nms_poly_f64 are produced on the device, bit for bit what that text would carry (tile_merge_math.h).  The C entry is
// in nms.hip.
//
// Tie rule: the rounded score descending, ties by ASCENDING INPUT ROW (tile order, then the row inside the tile).  The sort key is
// (source image * nc + class, score descending, row index): every key is distinct, as in metrics.hip.
//
// Launch chain (no exchange between workgroups inside a launch):
//   k_tm_rows            per row: polygon (valpost_device.h, the bits of k_val_post), text rounding, poly2origpoly -> (n, 9) doubles,
//                        key, row index; LDS class histogram of the workgroup's tile, one global atomic per workgroup and segment.
//                        One launch per kTmTiles tiles: their table travels in the kernel arguments.
//   bitonic_sort_pairs   (bitonic_sort.h) by (key, row)
//   k_tm_scan            exclusive scan of the histogram -> seg_off (empty segments stay in: run_merge_nms takes them anywhere)
//   run_merge_nms        nms_single.h, on order / seg_off / rows in the workspace
//   k_tm_scan            exclusive scan of the kept counts -> first output row of every segment, out_count, the abort flag
//   k_tm_emit            kept rows -> out (m, 11)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bitonic_sort.h"
#include "nms_driver.h"
#include "nms_single.h"
#include "obb_hip.h"
#include "tile_merge_math.h"
#include "valpost_device.h"
#include "ws_layout.h"

namespace obb {

constexpr int kTmThreads = 256;
constexpr int kTmTiles = 64;            // tiles per k_tm_rows launch
constexpr int kTmMaxNc = 256;           // one histogram slot per thread

struct TmChunk {                        // by value in the kernel arguments (2.6 KB)
  int det_off[kTmTiles + 1];            // rows of tile t: [det_off[t], det_off[t + 1])
  int blk_off[kTmTiles + 1];            // workgroups of tile t: [blk_off[t], blk_off[t + 1]), none for an empty tile
  int src[kTmTiles], left[kTmTiles], up[kTmTiles];
  double rate[kTmTiles];
  float pad_x[kTmTiles], pad_y[kTmTiles], gain[kTmTiles];
  int nt;
};

struct TmWs {
  double* rows9;                        // [n][9]
  unsigned long long* key;              // [n]
  int* idx;                             // [n]   sorted: the `order` of run_merge_nms
  int* seg_cnt;                         // [nseg]
  int* seg_off;                         // [nseg + 1]
  int* out_off;                         // [nseg + 1]
  int64_t* keep;                        // [n]
  int64_t* num_keep;                    // [nseg]
  void* merge_ws; size_t merge_bytes;   // run_merge_nms's own layout
  size_t bytes;
};

static TmWs tm_layout(void* base, int64_t n, int64_t nseg, int kind, int cus) {
  const size_t rows = (size_t)(n > 0 ? n : 1), segs = (size_t)(nseg > 0 ? nseg : 1);
  TmWs w;
  WsCursor c(base);
  w.rows9 = c.take<double>(rows * 9);
  w.key = c.take<unsigned long long>(rows);
  w.idx = c.take<int>(rows);
  w.seg_cnt = c.take<int>(segs);
  w.seg_off = c.take<int>(segs + 1);
  w.out_off = c.take<int>(segs + 1);
  w.keep = c.take<int64_t>(rows);
  w.num_keep = c.take<int64_t>(segs);
  w.merge_bytes = carve(nullptr, n, nseg, kind_recq(kind), cap_max(nseg), cus).total;
  w.merge_ws = c.bytes(w.merge_bytes);
  w.bytes = c.total();
  return w;
}

__global__ __launch_bounds__(kTmThreads) void k_tm_rows(const float* __restrict__ det7, TmChunk ch, int nc, int text_rounding,
                                                         double* __restrict__ rows9, unsigned long long* __restrict__ key,
                                                         int* __restrict__ idx, int* __restrict__ seg_cnt, int* __restrict__ info) {
  __shared__ int hist[kTmMaxNc];
  __shared__ int s_bad;
  const int tid = threadIdx.x;
  hist[tid] = 0;
  if (tid == 0) s_bad = 0;
  __syncthreads();
  int t = 0;                                                     // (workgroup-uniform: a short scan of kernel-argument registers)
  while (t + 1 < ch.nt && (int)blockIdx.x >= ch.blk_off[t + 1]) t++;
  const int i = ch.det_off[t] + ((int)blockIdx.x - ch.blk_off[t]) * kTmThreads + tid;
  const int src = ch.src[t];
  if (i < ch.det_off[t + 1]) {
    const float* r = det7 + (size_t)i * 7;
    const float conf = r[5];
    float p[8], pn[8];
    vt_rbox2poly(r[0], r[1], r[2], r[3], r[4], p);
    vt_scale_poly(p, ch.pad_x[t], ch.pad_y[t], ch.gain[t], pn);
    int c = tmm::class_of(r[6], nc);
    if (c < 0) c = 0, s_bad = 1;                                 // counted as class 0 so that the segments still add up to n; the call reports it
    const int left = ch.left[t], up = ch.up[t];
    const double rate = ch.rate[t];
    double* o = rows9 + (size_t)i * 9;
#pragma unroll
    for (int k = 0; k < 8; k++) o[k] = tmm::to_source(text_rounding ? tmm::round_dec1(pn[k]) : (double)pn[k], (k & 1) ? up : left, rate);
    o[8] = text_rounding ? tmm::round_dec5(conf) : (double)conf;
    key[i] = tmm::sort_key(src * nc + c, tmm::score_key(conf, text_rounding != 0));
    idx[i] = i;
    atomicAdd(&hist[c], 1);
  }
  __syncthreads();
  if (tid < nc && hist[tid]) atomicAdd(&seg_cnt[(size_t)src * nc + tid], hist[tid]);
  if (tid == 0 && s_bad) atomicOr(&info[0], 1);
}

// off[0 .. nseg] = exclusive scan of max(cnt, 0), one workgroup: thread t sums a contiguous span, the spans are scanned in LDS.
// cnt64 (the kept counts of run_merge_nms; -1: the device gave up) or cnt32; out_count / abort: written when not NULL.
__global__ __launch_bounds__(kTmThreads) void k_tm_scan(const int* __restrict__ cnt32, const int64_t* __restrict__ cnt64, int nseg,
                                                         int* __restrict__ off, int64_t* __restrict__ out_count, int* __restrict__ abort_flag) {
  __shared__ int part[kTmThreads];
  const int tid = threadIdx.x;
  const int span = (nseg + kTmThreads - 1) / kTmThreads;
  const int lo = min(tid * span, nseg), hi = min(lo + span, nseg);
  int sum = 0, bad = 0;
  for (int g = lo; g < hi; g++) {
    const long long v = cnt64 ? (long long)cnt64[g] : (long long)cnt32[g];
    if (v < 0) bad = 1;
    sum += v > 0 ? (int)v : 0;
  }
  part[tid] = sum;
  __syncthreads();
  for (int d = 1; d < kTmThreads; d <<= 1) {                     // inclusive scan of the spans' sums
    const int add = tid >= d ? part[tid - d] : 0;
    __syncthreads();
    part[tid] += add;
    __syncthreads();
  }
  int run = part[tid] - sum;
  for (int g = lo; g < hi; g++) {
    const long long v = cnt64 ? (long long)cnt64[g] : (long long)cnt32[g];
    off[g] = run;
    if (out_count) out_count[g] = v > 0 ? v : 0;
    run += v > 0 ? (int)v : 0;
  }
  if (tid == kTmThreads - 1) off[nseg] = part[tid];
  if (bad && abort_flag) atomicOr(abort_flag, 1);
}

// sorted position p lies in segment key[p] >> 32; the first num_keep[g] positions of a segment carry its kept rows
__global__ __launch_bounds__(kTmThreads) void k_tm_emit(const double* __restrict__ rows9, const unsigned long long* __restrict__ key,
                                                         const int* __restrict__ seg_off, const int* __restrict__ out_off,
                                                         const int64_t* __restrict__ keep, const int64_t* __restrict__ num_keep, int n, int nc,
                                                         double* __restrict__ out) {
  const int p = blockIdx.x * kTmThreads + threadIdx.x;
  if (p >= n) return;
  const int g = (int)(key[p] >> 32);
  const int j = p - seg_off[g];
  if ((long long)j >= (long long)num_keep[g]) return;
  const double* r = rows9 + (size_t)keep[p] * 9;
  double* o = out + ((size_t)out_off[g] + j) * 11;
#pragma unroll
  for (int k = 0; k < 9; k++) o[k] = r[k];
  o[9] = (double)(g % nc);
  o[10] = (double)(g / nc);
}

static int run_tile_merge(const float* det7, const int64_t* det_off_host, const obb_tile_rec* tiles_host, int64_t ntile, int64_t n_src,
                          int64_t nc, double thr, int flags, double* out, int64_t* out_count, int32_t* info, void* ws, size_t ws_bytes,
                          hipStream_t st) {
  if (ntile < 0 || ntile > 0x7fffffffLL || n_src < 1 || n_src > 0x7fffffffLL || nc < 1 || nc > kTmMaxNc || n_src * nc > 0x7fffffffLL || !out_count || !info ||
      !det_off_host || (ntile > 0 && !tiles_host) || (flags & ~(OBB_TILE_MERGE_TEXT_ROUNDING | OBB_TILE_MERGE_POLY_ALL)))
    return OBB_ERR_BAD_ARG;
  const int64_t n = det_off_host[ntile], nseg = n_src * nc;
  if (det_off_host[0] != 0 || n < 0 || n > 0x7fffffffLL || (n > 0 && (!det7 || !out))) return OBB_ERR_BAD_ARG;
  for (int64_t t = 0; t < ntile; t++) {
    const obb_tile_rec& r = tiles_host[t];
    if (det_off_host[t + 1] < det_off_host[t] || r.src_image < 0 || r.src_image >= n_src || !(r.rate > 0.0) || !(r.gain > 0.f))
      return OBB_ERR_BAD_ARG;
  }
  const int kind = (flags & OBB_TILE_MERGE_POLY_ALL) ? 4 : 2;
  const TmWs w = tm_layout(ws, n, nseg, kind, device_cus().cus);
  if (!ws_ok(ws, ws_bytes, w.bytes)) return OBB_ERR_WORKSPACE;
  if (hipMemsetAsync(info, 0, 2 * sizeof(int32_t), st) != hipSuccess) return OBB_ERR_LAUNCH;
  if (n == 0) return hipMemsetAsync(out_count, 0, (size_t)nseg * 8, st) == hipSuccess ? OBB_OK : OBB_ERR_LAUNCH;
  if (hipMemsetAsync(w.seg_cnt, 0, (size_t)nseg * 4, st) != hipSuccess) return OBB_ERR_LAUNCH;
  for (int64_t t0 = 0; t0 < ntile; t0 += kTmTiles) {
    TmChunk ch = {};
    ch.nt = (int)(ntile - t0 < kTmTiles ? ntile - t0 : kTmTiles);
    ch.det_off[0] = (int)det_off_host[t0];
    for (int t = 0; t < ch.nt; t++) {
      const obb_tile_rec& r = tiles_host[t0 + t];
      ch.det_off[t + 1] = (int)det_off_host[t0 + t + 1];
      ch.blk_off[t + 1] = ch.blk_off[t] + (ch.det_off[t + 1] - ch.det_off[t] + kTmThreads - 1) / kTmThreads;
      ch.src[t] = r.src_image; ch.left[t] = r.left; ch.up[t] = r.up; ch.rate[t] = r.rate;
      ch.pad_x[t] = r.pad_x; ch.pad_y[t] = r.pad_y; ch.gain[t] = r.gain;
    }
    if (ch.blk_off[ch.nt] > 0)
      k_tm_rows<<<(unsigned)ch.blk_off[ch.nt], kTmThreads, 0, st>>>(det7, ch, (int)nc, flags & OBB_TILE_MERGE_TEXT_ROUNDING, w.rows9, w.key, w.idx,
                                                                  w.seg_cnt, info);
  }
  bitonic_sort_pairs(w.key, w.idx, (unsigned)n, st);
  k_tm_scan<<<1, kTmThreads, 0, st>>>(w.seg_cnt, nullptr, (int)nseg, w.seg_off, nullptr, nullptr);
  if (hipGetLastError() != hipSuccess) return OBB_ERR_LAUNCH;
  if (const int rc = run_merge_nms(kind, w.rows9, 9, n, w.idx, w.seg_off, nseg, thr, w.keep, w.num_keep, w.merge_ws, w.merge_bytes, st)) return rc;
  k_tm_scan<<<1, kTmThreads, 0, st>>>(nullptr, w.num_keep, (int)nseg, w.out_off, out_count, info + 1);
  k_tm_emit<<<(unsigned)((n + kTmThreads - 1) / kTmThreads), kTmThreads, 0, st>>>(w.rows9, w.key, w.seg_off, w.out_off, w.keep, w.num_keep, (int)n,
                                                                                (int)nc, out);
  return hipGetLastError() == hipSuccess ? OBB_OK : OBB_ERR_LAUNCH;
}

}  // namespace obb
