// ap_per_class (utils/metrics.py:21-114 of the reference) on the device: the validation statistics that
// obb_val_tail_batch_f32 writes never leave device memory.  The arithmetic is csrc/ap_math.h (double, numpy's order).
//
// Tie rule: conf descending, ties by ASCENDING ROW INDEX (np.argsort(-conf, kind='stable')).  The sort key is
// (class, conf descending, row index): every key is distinct, so any correct sort yields the one pinned order.
//
// Launch chain (no exchange between workgroups inside a launch, guide Guideline 16):
//   k_ap_keys / k_ap_labels   keys + LDS class histograms (one atomic per workgroup and class), flags, true positives at column 0
//   k_ap_tables               segment offsets per class; tiles of kApTile rows that never straddle a class
//   bitonic_sort_pairs        (bitonic_sort.h) bitonic network with every comparator pointing up: rows >= n act as +inf and are
//                             never touched; the steps inside blocks of 2048 rows run in LDS, the wider ones one launch each
//   k_ap_tile_sum -> k_ap_class_scan -> k_ap_tile_tpc      prefix sums of `correct` (integers): reduce, scan of totals, apply
//   k_ap_class_rmax -> k_ap_tile_env                        reverse running maximum of precision: scan of tile maxima, apply
//   k_ap_ap, k_ap_pr, k_ap_best                             101 / 1000 binary searches per curve, trapezoid, F1, best index
#include <hip/hip_runtime.h>

#include "ap_math.h"
#include "bitonic_sort.h"
#include "obb_hip.h"
#include "stats_merge.h"
#include "ws_layout.h"

namespace obb {
namespace {

constexpr int kApTile = 1024;      // rows per scan tile: kApThreads x kApItems
constexpr int kApThreads = 256;
constexpr int kApItems = 4;
constexpr int kApMaxIou = 16;
constexpr int kApMaxNc = 256;
constexpr int kApPx = apm::kPrPoints;

struct ApWs {
  unsigned long long* key;   // [n]
  int* idx;                  // [n]
  int* tpc;                  // [n][niou]   inclusive true positives within the class, sorted order
  double* env;               // [n][niou]   reverse running maximum of precision within the class
  int* tile_tp;              // [tiles][niou]
  double* tile_max;          // [tiles][niou]
  int* seg_off;              // [nc_max + 1]
  int* tile_start;           // [nc_max + 1]
  double* curves;            // [3][nc_max][1000] when the caller passes none
  size_t bytes;
};

ApWs ap_layout(void* base, int64_t n, int niou, int nc_max) {
  const size_t rows = (size_t)(n > 0 ? n : 1), tiles = rows / kApTile + (size_t)nc_max;
  ApWs w;
  WsCursor c(base);
  w.key = c.take<unsigned long long>(rows);
  w.idx = c.take<int>(rows);
  w.tpc = c.take<int>(rows * niou);
  w.env = c.take<double>(rows * niou);
  w.tile_tp = c.take<int>(tiles * niou);
  w.tile_max = c.take<double>(tiles * niou);
  w.seg_off = c.take<int>((size_t)nc_max + 1);
  w.tile_start = c.take<int>((size_t)nc_max + 1);
  w.curves = c.take<double>((size_t)3 * nc_max * kApPx);
  w.bytes = c.total();
  return w;
}

// a class id as the reference stores it (a float): an integer in [0, nc_max), else -1 (NaN fails every comparison)
__device__ __forceinline__ int class_of(float v, int nc_max) {
  if (!(v >= 0.0f && v < (float)nc_max)) return -1;
  const int c = (int)v;
  return (float)c == v ? c : -1;
}

__global__ __launch_bounds__(kApThreads) void k_ap_keys(const float* __restrict__ stats, int64_t row_stride, int n, int niou, int nc_max,
                                                         unsigned long long* __restrict__ key, int* __restrict__ idx,
                                                         int* __restrict__ counts, int* __restrict__ info) {
  __shared__ int hist[kApMaxNc];
  __shared__ int s_tp, s_flags;
  const int tid = threadIdx.x;
  hist[tid] = 0;
  if (tid == 0) s_tp = 0, s_flags = 0;
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * kApThreads + tid;
  if (i < n) {
    const float* row = stats + i * row_stride;
    const float conf = row[niou];
    int c = class_of(row[niou + 1], nc_max);
    int flags = 0;
    if (c < 0) c = 0, flags |= 1;              // counted as class 0 so that the segments still add up to n; the call reports it
    if (conf != conf) flags |= 2;
    key[i] = ((unsigned long long)c << 32) | apm::conf_key_desc(conf);
    idx[i] = (int)i;
    atomicAdd(&hist[c], 1);
    if (row[0] > 0.5f) atomicAdd(&s_tp, 1);
    if (flags) atomicOr(&s_flags, flags);
  }
  __syncthreads();
  if (tid < nc_max && hist[tid]) atomicAdd(&counts[nc_max + tid], hist[tid]);
  if (tid == 0) {
    if (s_tp) atomicAdd(&info[1], s_tp);
    if (s_flags & 1) atomicOr(&info[2], 1);
    if (s_flags & 2) atomicOr(&info[3], 1);
  }
}

__global__ __launch_bounds__(kApThreads) void k_ap_labels(const float* __restrict__ target_cls, int m, int nc_max, int* __restrict__ counts,
                                                           int* __restrict__ info) {
  __shared__ int hist[kApMaxNc];
  __shared__ int s_bad;
  const int tid = threadIdx.x;
  hist[tid] = 0;
  if (tid == 0) s_bad = 0;
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * kApThreads + tid;
  if (i < m) {
    const int c = class_of(target_cls[i], nc_max);
    if (c < 0) atomicOr(&s_bad, 1);
    else atomicAdd(&hist[c], 1);
  }
  __syncthreads();
  if (tid < nc_max && hist[tid]) atomicAdd(&counts[tid], hist[tid]);
  if (tid == 0 && s_bad) atomicOr(&info[2], 1);
}

// nc_max <= 256 entries: one thread walks them
__global__ void k_ap_tables(const int* __restrict__ counts, int nc_max, int* __restrict__ seg_off, int* __restrict__ tile_start) {
  if (threadIdx.x || blockIdx.x) return;
  int rows = 0, tiles = 0;
  for (int c = 0; c < nc_max; c++) {
    seg_off[c] = rows;
    tile_start[c] = tiles;
    const int np = counts[nc_max + c];
    rows += np;
    tiles += (np + kApTile - 1) / kApTile;
  }
  seg_off[nc_max] = rows;
  tile_start[nc_max] = tiles;
}

struct Tile {
  int cls, start, len, first;   // class, first sorted row, rows, first sorted row of the class
};

// the tile of this workgroup, or len = 0 for a workgroup past the last tile (the grid is an upper bound known on the host)
__device__ __forceinline__ Tile tile_of(int t, const int* __restrict__ seg_off, const int* __restrict__ tile_start, int nc_max) {
  Tile r = {0, 0, 0, 0};
  if (t >= tile_start[nc_max]) return r;
  int lo = 0, hi = nc_max;      // the last class with tile_start[c] <= t that owns a tile
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (tile_start[mid] <= t) lo = mid; else hi = mid;
  }
  r.cls = lo;
  r.first = seg_off[lo];
  r.start = r.first + (t - tile_start[lo]) * kApTile;
  const int left = seg_off[lo + 1] - r.start;
  r.len = left < kApTile ? left : kApTile;
  return r;
}

__global__ __launch_bounds__(kApThreads) void k_ap_tile_sum(const float* __restrict__ stats, int64_t row_stride, int niou, int nc_max,
                                                             const int* __restrict__ idx, const int* __restrict__ seg_off,
                                                             const int* __restrict__ tile_start, int* __restrict__ tile_tp) {
  __shared__ int sum[kApMaxIou];
  const int tid = threadIdx.x;
  const Tile T = tile_of(blockIdx.x, seg_off, tile_start, nc_max);
  if (T.len == 0) return;
  if (tid < kApMaxIou) sum[tid] = 0;
  __syncthreads();
  for (int q = tid; q < T.len; q += kApThreads) {
    const float* row = stats + (int64_t)idx[T.start + q] * row_stride;
    for (int j = 0; j < niou; j++)
      if (row[j] > 0.5f) atomicAdd(&sum[j], 1);
  }
  __syncthreads();
  if (tid < niou) tile_tp[(size_t)blockIdx.x * niou + tid] = sum[tid];
}

// per class and IoU column: exclusive prefix sum of the tile totals, one thread per column
__global__ void k_ap_class_scan(int niou, const int* __restrict__ tile_start, int* __restrict__ tile_tp) {
  const int c = blockIdx.x, j = threadIdx.x;
  if (j >= niou) return;
  int run = 0;
  for (int t = tile_start[c]; t < tile_start[c + 1]; t++) {
    const int v = tile_tp[(size_t)t * niou + j];
    tile_tp[(size_t)t * niou + j] = run;
    run += v;
  }
}

// exclusive scan of one value per thread over the workgroup (Hillis-Steele in LDS); s is free again on return
template <typename T, typename Op>
__device__ __forceinline__ T block_scan_excl(T v, T identity, T* s, int lane, Op op) {
  s[lane] = v;
  __syncthreads();
  for (int d = 1; d < kApThreads; d <<= 1) {
    const T x = lane >= d ? s[lane - d] : identity;
    __syncthreads();
    s[lane] = op(x, s[lane]);
    __syncthreads();
  }
  const T r = lane ? s[lane - 1] : identity;
  __syncthreads();
  return r;
}

struct OpAdd { __device__ int operator()(int a, int b) const { return a + b; } };
struct OpMax { __device__ double operator()(double a, double b) const { return a > b ? a : b; } };

// tpc of the tile's rows (offset of the tile + scan inside it) and the tile's maximum of precision
__global__ __launch_bounds__(kApThreads) void k_ap_tile_tpc(const float* __restrict__ stats, int64_t row_stride, int niou, int nc_max,
                                                             const int* __restrict__ idx, const int* __restrict__ seg_off,
                                                             const int* __restrict__ tile_start, const int* __restrict__ tile_tp,
                                                             int* __restrict__ tpc, double* __restrict__ tile_max) {
  __shared__ int s[kApThreads];
  __shared__ unsigned long long s_max;
  const int tid = threadIdx.x;
  const Tile T = tile_of(blockIdx.x, seg_off, tile_start, nc_max);
  if (T.len == 0) return;
  int rowi[kApItems];
  for (int q = 0; q < kApItems; q++) {
    const int r = tid * kApItems + q;
    rowi[q] = r < T.len ? idx[T.start + r] : -1;
  }
  for (int j = 0; j < niou; j++) {
    if (tid == 0) s_max = 0ull;
    int a[kApItems], run = 0;
    for (int q = 0; q < kApItems; q++) {
      run += (rowi[q] >= 0 && stats[(int64_t)rowi[q] * row_stride + j] > 0.5f) ? 1 : 0;
      a[q] = run;
    }
    const int before = block_scan_excl(run, 0, s, tid, OpAdd()) + tile_tp[(size_t)blockIdx.x * niou + j];   // (barriers inside)
    double mx = 0.0;
    for (int q = 0; q < kApItems; q++) {
      if (rowi[q] < 0) break;
      const int pos = T.start + tid * kApItems + q, v = before + a[q];
      tpc[(size_t)pos * niou + j] = v;
      const double p = apm::precision_of(v, (int64_t)(pos - T.first) + 1);
      mx = p > mx ? p : mx;
    }
    // precision >= 0: the bit patterns order like the values
    if (mx > 0.0) atomicMax(&s_max, (unsigned long long)__double_as_longlong(mx));
    __syncthreads();
    if (tid == 0) tile_max[(size_t)blockIdx.x * niou + j] = __longlong_as_double((long long)s_max);
    __syncthreads();
  }
}

// per class and IoU column: the maximum over the tiles AFTER each tile (0 after the last: mpre's closing sentinel)
__global__ void k_ap_class_rmax(int niou, const int* __restrict__ tile_start, double* __restrict__ tile_max) {
  const int c = blockIdx.x, j = threadIdx.x;
  if (j >= niou) return;
  double run = 0.0;
  for (int t = tile_start[c + 1] - 1; t >= tile_start[c]; t--) {
    const double v = tile_max[(size_t)t * niou + j];
    tile_max[(size_t)t * niou + j] = run;
    run = v > run ? v : run;
  }
}

// env = reverse running maximum of precision: thread `lane` owns the rows kApItems * lane .. from the END of the tile
__global__ __launch_bounds__(kApThreads) void k_ap_tile_env(int niou, int nc_max, const int* __restrict__ seg_off,
                                                             const int* __restrict__ tile_start, const int* __restrict__ tpc,
                                                             const double* __restrict__ tile_max, double* __restrict__ env) {
  __shared__ double s[kApThreads];
  const int tid = threadIdx.x;
  const Tile T = tile_of(blockIdx.x, seg_off, tile_start, nc_max);
  if (T.len == 0) return;
  for (int j = 0; j < niou; j++) {
    double a[kApItems], run = 0.0;
    for (int q = 0; q < kApItems; q++) {          // q-th row from the end of this thread's share
      const int r = T.len - 1 - (tid * kApItems + q);
      if (r >= 0) {
        const int pos = T.start + r;
        const double p = apm::precision_of(tpc[(size_t)pos * niou + j], (int64_t)(pos - T.first) + 1);
        run = p > run ? p : run;
      }
      a[q] = run;
    }
    double after = block_scan_excl(run, 0.0, s, tid, OpMax());
    const double carry = tile_max[(size_t)blockIdx.x * niou + j];
    after = carry > after ? carry : after;
    for (int q = 0; q < kApItems; q++) {
      const int r = T.len - 1 - (tid * kApItems + q);
      if (r < 0) break;
      env[(size_t)(T.start + r) * niou + j] = a[q] > after ? a[q] : after;
    }
  }
}

struct TpcAt {
  const int* p; int64_t stride;
  OBB_HD int operator()(int64_t i) const { return p[i * stride]; }
};
struct EnvAt {
  const double* p; int64_t stride;
  OBB_HD double operator()(int64_t i) const { return p[i * stride]; }
};
struct ConfAt {
  const float* stats; const int* idx; int64_t row_stride;
  OBB_HD double operator()(int64_t i) const { return (double)stats[(int64_t)idx[i] * row_stride]; }
};
struct RecallAt {
  TpcAt tpc; double nl_eps;
  OBB_HD double operator()(int64_t i) const { return apm::recall_of(tpc(i), nl_eps); }
};
struct PrecisionAt {
  TpcAt tpc;
  OBB_HD double operator()(int64_t i) const { return apm::precision_of(tpc(i), i + 1); }
};

// grid (class, IoU column): 101 interpolation points, then the trapezoid rule in numpy's summation order
__global__ __launch_bounds__(128) void k_ap_ap(int niou, int nc_max, const int* __restrict__ counts, const int* __restrict__ seg_off,
                                                const int* __restrict__ tpc, const double* __restrict__ env, double* __restrict__ ap) {
  __shared__ double y[apm::kApPoints];
  const int c = blockIdx.x, j = blockIdx.y, k = threadIdx.x;
  const int n_l = counts[c], first = seg_off[c], np = seg_off[c + 1] - first;
  if (n_l == 0 || np == 0) return;                   // rows stay zero (metrics.py:51-52)
  if (k < apm::kApPoints) {
    const TpcAt t = {tpc + (size_t)first * niou + j, niou};
    const EnvAt e = {env + (size_t)first * niou + j, niou};
    y[k] = apm::ap_interp(apm::ap_x(k), (int64_t)np, (double)n_l + apm::kEps, t, e);
  }
  __syncthreads();
  if (k == 0) ap[c * niou + j] = apm::trapz101(y);
}

// grid (class, 4 x 256 points of px): p, r, f1 over px at IoU column 0
__global__ __launch_bounds__(kApThreads) void k_ap_pr(const float* __restrict__ stats, int64_t row_stride, int niou, int nc_max,
                                                       const int* __restrict__ counts, const int* __restrict__ seg_off,
                                                       const int* __restrict__ idx, const int* __restrict__ tpc, double* __restrict__ curves) {
  const int c = blockIdx.x, k = blockIdx.y * kApThreads + threadIdx.x;
  const int n_l = counts[c], first = seg_off[c], np = seg_off[c + 1] - first;
  if (k >= kApPx || n_l == 0 || np == 0) return;
  const TpcAt t = {tpc + (size_t)first * niou, niou};
  const ConfAt cf = {stats + niou, idx + first, row_stride};
  const RecallAt rc = {t, (double)n_l + apm::kEps};
  const PrecisionAt pc = {t};
  const double px = apm::pr_x(k);
  const double r = apm::pr_interp(px, (int64_t)np, cf, rc, 0.0);
  const double p = apm::pr_interp(px, (int64_t)np, cf, pc, 1.0);
  const size_t plane = (size_t)nc_max * kApPx, at = (size_t)c * kApPx + k;
  curves[at] = p;
  curves[plane + at] = r;
  curves[2 * plane + at] = apm::f1_of(p, r);
}

// the first argmax of the class-mean F1 curve (f1.mean(0).argmax(): rows added in class order, then divided), p r f1 tp fp there
__global__ __launch_bounds__(1024) void k_ap_best(int nc_max, const int* __restrict__ counts, const double* __restrict__ curves,
                                                   double* __restrict__ prf, int* __restrict__ info) {
  __shared__ double val[1024];
  __shared__ int at[1024];
  const int k = threadIdx.x;
  const size_t plane = (size_t)nc_max * kApPx;
  double sum = 0.0;
  int ncls = 0;
  if (k < kApPx)
    for (int c = 0; c < nc_max; c++)
      if (counts[c] > 0) sum += curves[2 * plane + (size_t)c * kApPx + k], ncls++;
  val[k] = (k < kApPx && ncls) ? sum / (double)ncls : -1.0;      // (F1 >= 0)
  at[k] = k;
  __syncthreads();
  for (int d = 512; d > 0; d >>= 1) {
    if (k < d && (val[k + d] > val[k] || (val[k + d] == val[k] && at[k + d] < at[k]))) val[k] = val[k + d], at[k] = at[k + d];
    __syncthreads();
  }
  const int best = val[0] >= 0.0 ? at[0] : 0;
  if (k == 0) info[0] = best;
  if (k < nc_max && counts[k] > 0) {
    const double p = curves[(size_t)k * kApPx + best], r = curves[plane + (size_t)k * kApPx + best];
    const double tp = apm::tp_of(r, counts[k]);
    double* o = prf + (size_t)k * 5;
    o[0] = p, o[1] = r, o[2] = curves[2 * plane + (size_t)k * kApPx + best], o[3] = tp, o[4] = apm::fp_of(tp, p);
  }
}

}  // namespace
}  // namespace obb

extern "C" {

size_t obb_ap_per_class_workspace_bytes(int64_t n, int niou, int nc_max) {
  if (n < 0 || n > 0x7fffffff || niou < 1 || niou > obb::kApMaxIou || nc_max < 1 || nc_max > obb::kApMaxNc) return 0;
  return obb::ap_layout(nullptr, n, niou, nc_max).bytes;
}

int obb_ap_per_class_f32(const float* stats, int64_t row_stride, int64_t n, int niou, const float* target_cls, int64_t m, int nc_max,
                         double* ap, double* prf, int32_t* counts, int32_t* info, double* curves, void* ws, size_t ws_bytes,
                         void* stream) {
  using namespace obb;
  if (n < 0 || n >= 0x7fffffffLL || m < 0 || m >= 0x7fffffffLL || niou < 1 || niou > kApMaxIou || nc_max < 1 || nc_max > kApMaxNc)
    return OBB_ERR_BAD_ARG;
  if (!ap || !prf || !counts || !info || (n > 0 && (!stats || row_stride < niou + 2)) || (m > 0 && !target_cls)) return OBB_ERR_BAD_ARG;
  const ApWs w = ap_layout(ws, n, niou, nc_max);
  if (!ws_ok(ws, ws_bytes, w.bytes)) return OBB_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  double* cur = curves ? curves : w.curves;
  if (hipMemsetAsync(ap, 0, (size_t)nc_max * niou * 8, st) != hipSuccess || hipMemsetAsync(prf, 0, (size_t)nc_max * 5 * 8, st) != hipSuccess ||
      hipMemsetAsync(counts, 0, (size_t)nc_max * 2 * 4, st) != hipSuccess || hipMemsetAsync(info, 0, 16, st) != hipSuccess ||
      hipMemsetAsync(cur, 0, (size_t)3 * nc_max * kApPx * 8, st) != hipSuccess)
    return OBB_ERR_LAUNCH;
  if (m > 0) k_ap_labels<<<(unsigned)((m + kApThreads - 1) / kApThreads), kApThreads, 0, st>>>(target_cls, (int)m, nc_max, counts, info);
  if (n > 0) {
    const unsigned rows = (unsigned)n, grid = (rows + kApThreads - 1) / kApThreads;
    const unsigned tiles = rows / kApTile + (unsigned)nc_max;      // >= the number of class-aligned tiles
    k_ap_keys<<<grid, kApThreads, 0, st>>>(stats, row_stride, (int)n, niou, nc_max, w.key, w.idx, counts, info);
    k_ap_tables<<<1, 64, 0, st>>>(counts, nc_max, w.seg_off, w.tile_start);
    bitonic_sort_pairs(w.key, w.idx, rows, st);
    k_ap_tile_sum<<<tiles, kApThreads, 0, st>>>(stats, row_stride, niou, nc_max, w.idx, w.seg_off, w.tile_start, w.tile_tp);
    k_ap_class_scan<<<nc_max, 64, 0, st>>>(niou, w.tile_start, w.tile_tp);
    k_ap_tile_tpc<<<tiles, kApThreads, 0, st>>>(stats, row_stride, niou, nc_max, w.idx, w.seg_off, w.tile_start, w.tile_tp, w.tpc, w.tile_max);
    k_ap_class_rmax<<<nc_max, 64, 0, st>>>(niou, w.tile_start, w.tile_max);
    k_ap_tile_env<<<tiles, kApThreads, 0, st>>>(niou, nc_max, w.seg_off, w.tile_start, w.tpc, w.tile_max, w.env);
    k_ap_ap<<<dim3(nc_max, niou), 128, 0, st>>>(niou, nc_max, counts, w.seg_off, w.tpc, w.env, ap);
    k_ap_pr<<<dim3(nc_max, (kApPx + kApThreads - 1) / kApThreads), kApThreads, 0, st>>>(stats, row_stride, niou, nc_max, counts, w.seg_off, w.idx,
                                                                                       w.tpc, cur);
  }
  k_ap_best<<<1, 1024, 0, st>>>(nc_max, counts, cur, prf, info);
  return hipGetLastError() == hipSuccess ? OBB_OK : OBB_ERR_LAUNCH;
}

size_t obb_stats_merge_workspace_bytes(int64_t n_images_total) {
  if (n_images_total < 0 || n_images_total >= 0x7fffffffLL) return 0;
  return obb::sm_layout(nullptr, n_images_total).bytes;
}

int obb_stats_merge_f32(const float* src, int64_t src_stride, int64_t run_stride, const int64_t* rows_per_run_host, const int32_t* counts,
                        const int64_t* img_id, int64_t max_images_per_run, const int64_t* images_per_run_host, int64_t world,
                        int64_t n_images_total, int64_t width, float* dst, int64_t dst_stride, int64_t dst_rows, int32_t* counts_out,
                        int32_t* info, void* ws, size_t ws_cap, void* stream) {
  return obb::run_stats_merge(src, src_stride, run_stride, rows_per_run_host, counts, img_id, max_images_per_run, images_per_run_host, world,
                              n_images_total, width, dst, dst_stride, dst_rows, counts_out, info, ws, ws_cap, (hipStream_t)stream);
}

}  // extern "C"
