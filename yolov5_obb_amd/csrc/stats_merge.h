// Merge of the validation statistics of several ranks (namespace obb): the rows that `world` runs of the validation tail wrote,
// each run holding the images of one rank back to back, are put in GLOBAL IMAGE ORDER -- the order a single process would have
// written them in, which is what the tie rule of metrics.hip (conf descending, then ascending row index) is defined on.  The C
// entry is in metrics.hip.
//
// An image is a contiguous range of rows in its run and a contiguous range of rows in the merged array; nothing is reordered
// inside an image.  Launch chain (plain launches, no exchange between workgroups inside a launch, nothing read back):
//   k_sm_scatter   one workgroup per run: exclusive scan of the run's per-image counts (tiles of kSmThreads with a carry) -> the
//                  image's first source row; count and source row go to slot img_id.  A slot is claimed with one atomic: the
//                  second claim of an id is reported, not written.  The run's total is held against rows_per_run_host.
//   k_sm_scan      one workgroup: exclusive scan over the n_images_total slots (tiles of kSmThreads x kSmItems with a carry) ->
//                  first merged row of every image, the total, the capacity check
//   k_sm_copy      one WAVE per image (grid-stride over the images): the image's count x width floats, lanes along the range --
//                  lane l moves elements l, l + 64, ...: every wave instruction reads and writes 256 consecutive bytes (a row
//                  boundary inside it when a stride is wider than `width`), four loads in flight per lane on packed rows.
//                  It does nothing when info[0] is set: offsets made from inconsistent counts are never followed.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "obb_hip.h"
#include "ws_layout.h"

namespace obb {

constexpr int kSmThreads = 256;
constexpr int kSmItems = 4;             // slots per thread and tile of k_sm_scan
constexpr int kSmRuns = 64;             // runs per k_sm_scatter launch: their table travels in the kernel arguments
constexpr int kSmWave = 64;
constexpr int kSmMaxBlocks = 2048;      // k_sm_copy: 8 workgroups per CU, the rest by grid stride

constexpr int kSmBadId = 1, kSmTwice = 2, kSmRunTotal = 4, kSmCapacity = 8;      // bits of info[0]

struct SmChunk {                        // by value in the kernel arguments
  int images[kSmRuns];                  // images of run r0 + r
  int rows[kSmRuns];                    // rows_per_run_host of run r0 + r
  int r0, nr;
};

struct SmWs {
  int* slot_cnt;                        // [n_images_total]  rows of image id (0: never supplied)
  int* slot_claim;                      // [n_images_total]  claims of the id
  long long* slot_src;                  // [n_images_total]  first source row, counted from src
  int* slot_off;                        // [n_images_total]  first merged row
  size_t bytes;
};

static SmWs sm_layout(void* base, int64_t n_images_total) {
  const size_t slots = (size_t)(n_images_total > 0 ? n_images_total : 1);
  SmWs w;
  WsCursor c(base);
  w.slot_cnt = c.take<int>(slots);
  w.slot_claim = c.take<int>(slots);
  w.slot_src = c.take<long long>(slots);
  w.slot_off = c.take<int>(slots);
  w.bytes = c.total();
  return w;
}

// exclusive scan of one value per thread over the workgroup (Hillis-Steele in LDS, as metrics.hip: block_scan_excl), and the
// workgroup's total; s is free again on return
__device__ __forceinline__ long long sm_scan_excl(long long v, long long* s, int tid, long long* total) {
  s[tid] = v;
  __syncthreads();
  for (int d = 1; d < kSmThreads; d <<= 1) {
    const long long x = tid >= d ? s[tid - d] : 0;
    __syncthreads();
    s[tid] += x;
    __syncthreads();
  }
  const long long r = s[tid] - v;
  *total = s[kSmThreads - 1];
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(kSmThreads) void k_sm_scatter(const int32_t* __restrict__ counts, const int64_t* __restrict__ img_id,
                                                            int64_t max_images, SmChunk ch, int64_t run_stride, int64_t n_total,
                                                            int* __restrict__ slot_cnt, int* __restrict__ slot_claim,
                                                            long long* __restrict__ slot_src, int* __restrict__ info) {
  __shared__ long long s[kSmThreads];
  const int tid = threadIdx.x, r = blockIdx.x, k = ch.images[r];
  const int64_t run = (int64_t)ch.r0 + r;
  const int32_t* cnt = counts + run * max_images;
  const int64_t* ids = img_id + run * max_images;
  long long carry = 0;
  int bad = 0;
  for (int base = 0; base < k; base += kSmThreads) {             // (k is uniform: every thread meets every barrier)
    const int j = base + tid;
    int c = 0;
    int64_t id = -1;
    if (j < k) {
      c = cnt[j];
      id = ids[j];
      if (c < 0) c = 0, bad |= kSmRunTotal;                      // (a negative count: the run cannot add up)
    }
    long long total;
    const long long first = carry + sm_scan_excl(c, s, tid, &total);
    if (j < k) {
      if (id < 0 || id >= n_total) {
        bad |= kSmBadId;
      } else if (atomicAdd(&slot_claim[id], 1) != 0) {
        bad |= kSmTwice;
        info[2] = (int)id;                                       // (any one of them)
      } else {
        slot_cnt[id] = c;
        slot_src[id] = run * run_stride + first;
      }
    }
    carry += total;
  }
  if (tid == 0 && carry != (long long)ch.rows[r]) bad |= kSmRunTotal, info[3] = (int)run;
  if (bad) atomicOr(&info[0], bad);
}

__global__ __launch_bounds__(kSmThreads) void k_sm_scan(const int* __restrict__ slot_cnt, int64_t n_total, int64_t dst_rows,
                                                         int* __restrict__ slot_off, int32_t* __restrict__ counts_out,
                                                         int* __restrict__ info) {
  __shared__ long long s[kSmThreads];
  const int tid = threadIdx.x;
  long long carry = 0;
  for (int64_t base = 0; base < n_total; base += kSmThreads * kSmItems) {
    const int64_t i0 = base + (int64_t)tid * kSmItems;
    int c[kSmItems];
    long long sum = 0;
#pragma unroll
    for (int q = 0; q < kSmItems; q++) {
      c[q] = i0 + q < n_total ? slot_cnt[i0 + q] : 0;
      sum += c[q];
    }
    long long total;
    long long at = carry + sm_scan_excl(sum, s, tid, &total);
#pragma unroll
    for (int q = 0; q < kSmItems; q++) {
      if (i0 + q < n_total) {
        slot_off[i0 + q] = (int)(at < 0x7fffffffLL ? at : 0x7fffffffLL);      // (beyond: the capacity bit below is set, nothing is copied)
        if (counts_out) counts_out[i0 + q] = c[q];
      }
      at += c[q];
    }
    carry += total;
  }
  if (tid == 0) {
    info[1] = (int)(carry < 0x7fffffffLL ? carry : 0x7fffffffLL);
    if (carry > dst_rows || carry >= 0x7fffffffLL) atomicOr(&info[0], kSmCapacity);
  }
}

__global__ __launch_bounds__(kSmThreads) void k_sm_copy(const float* __restrict__ src, int64_t src_stride, const int* __restrict__ slot_cnt,
                                                         const long long* __restrict__ slot_src, const int* __restrict__ slot_off,
                                                         int64_t n_total, int width, float* __restrict__ dst, int64_t dst_stride,
                                                         const int* __restrict__ info) {
  if (info[0]) return;                                           // (written by the launches in front of this one)
  constexpr int kWaves = kSmThreads / kSmWave;
  const int lane = threadIdx.x % kSmWave;
  const int64_t waves = (int64_t)gridDim.x * kWaves;
  const bool packed = src_stride == width && dst_stride == width;
  const int step_rows = kSmWave / width, step_cols = kSmWave % width;      // 64 elements further along rows of `width`
  for (int64_t i = (int64_t)blockIdx.x * kWaves + threadIdx.x / kSmWave; i < n_total; i += waves) {
    const int c = slot_cnt[i];                                   // (one address for the whole wave)
    if (c == 0) continue;
    const float* s = src + slot_src[i] * src_stride;
    float* d = dst + (int64_t)slot_off[i] * dst_stride;
    const int64_t len = (int64_t)c * width;
    if (packed) {
      int64_t e = lane;
      for (; e + 3 * kSmWave < len; e += 4 * kSmWave) {
        const float a0 = s[e], a1 = s[e + kSmWave], a2 = s[e + 2 * kSmWave], a3 = s[e + 3 * kSmWave];
        d[e] = a0, d[e + kSmWave] = a1, d[e + 2 * kSmWave] = a2, d[e + 3 * kSmWave] = a3;
      }
      for (; e < len; e += kSmWave) d[e] = s[e];
    } else {
      int64_t row = lane / width;
      int col = lane % width;
      for (int64_t e = lane; e < len; e += kSmWave) {
        d[row * dst_stride + col] = s[row * src_stride + col];
        row += step_rows, col += step_cols;
        if (col >= width) col -= width, row++;
      }
    }
  }
}

static int run_stats_merge(const float* src, int64_t src_stride, int64_t run_stride, const int64_t* rows_per_run_host, const int32_t* counts,
                           const int64_t* img_id, int64_t max_images, const int64_t* images_per_run_host, int64_t world, int64_t n_total,
                           int64_t width, float* dst, int64_t dst_stride, int64_t dst_rows, int32_t* counts_out, int32_t* info, void* ws,
                           size_t ws_cap, hipStream_t st) {
  if (world < 1 || world > 0x7fffffffLL || width < 1 || width > 0x7fffffffLL || src_stride < width || dst_stride < width || run_stride < 0 ||
      n_total < 0 || n_total >= 0x7fffffffLL || max_images < 0 || max_images > 0x7fffffffLL || dst_rows < 0 || !rows_per_run_host ||
      !images_per_run_host || !info)
    return OBB_ERR_BAD_ARG;
  int64_t rows = 0, images = 0;
  for (int64_t r = 0; r < world; r++) {
    const int64_t nr = rows_per_run_host[r], ni = images_per_run_host[r];
    if (nr < 0 || nr > run_stride || ni < 0 || ni > max_images) return OBB_ERR_BAD_ARG;
    rows += nr, images += ni;
    if (rows >= 0x7fffffffLL) return OBB_ERR_BAD_ARG;
  }
  if ((rows > 0 && !src) || (images > 0 && (!counts || !img_id)) || (dst_rows > 0 && !dst)) return OBB_ERR_BAD_ARG;
  const SmWs w = sm_layout(ws, n_total);
  if (!ws_ok(ws, ws_cap, w.bytes)) return OBB_ERR_WORKSPACE;
  if (hipMemsetAsync(info, 0, 4 * sizeof(int32_t), st) != hipSuccess) return OBB_ERR_LAUNCH;
  if (n_total > 0 && (hipMemsetAsync(w.slot_cnt, 0, (size_t)n_total * 4, st) != hipSuccess ||
                      hipMemsetAsync(w.slot_claim, 0, (size_t)n_total * 4, st) != hipSuccess))
    return OBB_ERR_LAUNCH;
  for (int64_t r0 = 0; r0 < world; r0 += kSmRuns) {
    SmChunk ch = {};
    ch.r0 = (int)r0;
    ch.nr = (int)(world - r0 < kSmRuns ? world - r0 : kSmRuns);
    for (int r = 0; r < ch.nr; r++) ch.images[r] = (int)images_per_run_host[r0 + r], ch.rows[r] = (int)rows_per_run_host[r0 + r];
    k_sm_scatter<<<(unsigned)ch.nr, kSmThreads, 0, st>>>(counts, img_id, max_images, ch, run_stride, n_total, w.slot_cnt, w.slot_claim, w.slot_src,
                                                       info);
  }
  k_sm_scan<<<1, kSmThreads, 0, st>>>(w.slot_cnt, n_total, dst_rows, w.slot_off, counts_out, info);
  if (n_total > 0 && rows > 0) {
    constexpr int kWaves = kSmThreads / kSmWave;
    const int64_t blocks = (n_total + kWaves - 1) / kWaves;
    k_sm_copy<<<(unsigned)(blocks < kSmMaxBlocks ? blocks : kSmMaxBlocks), kSmThreads, 0, st>>>(src, src_stride, w.slot_cnt, w.slot_src, w.slot_off,
                                                                                              n_total, (int)width, dst, dst_stride, info);
  }
  return hipGetLastError() == hipSuccess ? OBB_OK : OBB_ERR_LAUNCH;
}

}  // namespace obb
