// In-memory DOTA Task-1 evaluation (namespace obb): merged full-image rows + a resident ground-truth set -> per-class AP, the whole of
// voc_eval (DOTA_devkit/dota_evaluation_task1.py:88-249 of the reference) for every class in one launch chain.  The reference reads
// Task1_<class>.txt back, sorts per class on the host and walks the detections one by one; here nothing leaves the device but the
// nc APs.  The arithmetic of the curve and of voc_ap is csrc/voc_ap_math.h (IEEE double, numpy's order, np.sum's grouping).  The C
// entry is in pairwise.hip, next to k_eval_best_gt, which this chain launches unchanged.
//
// Tie rule: score descending, NaN scores last, -0.0 and +0.0 one value (np.argsort(-confidence)); equal scores in ASCENDING INPUT
// ROW -- the package's pinned rule (np.argsort(..., kind='stable')); numpy's default sort leaves ties to its introsort.
//
// Launch chain (plain launches on the caller's stream; no exchange between workgroups inside a launch, no co-residency, no spin):
//   k_t1_npos            npos[c] = the non-difficult records of class c
//   k_t1_key             per row: class and image validated (info[0]), 64-bit score key, row index, segment cls * n_img + img
//   bitonic_sort_pairs   (bitonic_sort.h) by (score key, row): the global score order
//   k_t1_hist            class histogram of every tile of kT1Tile sorted positions
//   k_t1_class_scan      per class: exclusive scan over the tiles; cls_off
//   k_t1_scatter         stable partition by class: order, the segment and the 8 coordinates of every sorted position
//   k_eval_best_gt       (pairwise.hip) ovmax / jmax per sorted detection over the records of its (class, image) segment
//   k_t1_claim           one int32 slot per record: atomicMin of the sorted positions that hit it (order-independent)
//   k_t1_mark            TP / FP marks, inclusive sums inside a tile (both counts in one 64-bit word), tile totals
//   k_t1_tile_scan       exclusive scan of the tile totals
//   k_t1_curve           per-class inclusive TP / FP counts (differences of the global sums: integers, exact) -> rec, prec
//   k_t1_ap              one workgroup per class: the 11-point maxima, or the envelope, the kept terms and np.sum of voc_ap
//
// Serial steps, sized for validation sets (nd up to a few million rows): k_t1_class_scan walks the nd / 1024 tiles with one thread
// per class, and thread 0 of a k_t1_ap workgroup sums the class's kept terms (at most one per true positive, so at most npos + 1;
// the envelope and the compaction in front of it are spread over the workgroup).  Both grow linearly with nd in one thread; the
// entry accepts nd below 2^31 for the sake of its index types, not as a promise of speed there.
//
// Resources (hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage; wave64, no scratch anywhere):
//   kernel            VGPR  SGPR  LDS bytes  scratch  waves/SIMD
//   k_t1_npos           13    22          4        0   8
//   k_t1_key            20    28          4        0   8
//   k_t1_hist           12    20       1024        0   8
//   k_t1_class_scan     16    18       1024        0   8
//   k_t1_scatter        36    38       4096        0   8
//   k_t1_claim           6    18          0        0   8
//   k_t1_mark           18    46       2048        0   8
//   k_t1_tile_scan      14    14       2048        0   8
//   k_t1_curve          24    20          0        0   8
//   k_t1_ap             66    48       4080        0   7
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bitonic_sort.h"
#include "obb_hip.h"
#include "voc_ap_math.h"
#include "ws_layout.h"

namespace obb {

// k_eval_best_gt on `st` (defined by the translation unit that holds the kernel, pairwise.hip)
int launch_eval_best_gt(const double* dets8, const int32_t* det_img, int64_t nd, const double* gts8, const int32_t* gt_off,
                        double* ovmax, int32_t* jmax, hipStream_t st);

constexpr int kT1Threads = 256;
constexpr int kT1Items = 4;
constexpr int kT1Tile = kT1Threads * kT1Items;   // sorted positions per histogram / scan tile
constexpr int kT1MaxNc = 256;                    // one histogram slot per thread
constexpr int kT1Waves = kT1Threads / 64;

typedef unsigned long long t1_u64;

struct T1Ws {
  t1_u64* key;          // [nd]      score key, sorted
  int* idx;             // [nd]      input row, in global score order
  int* seg_in;          // [nd]      cls * n_img + img of an input row (0 for a row that failed the check)
  int* order;           // [nd]      input row of every sorted position (when the caller passes no `order`)
  int* seg;             // [nd]      segment of every sorted position: k_eval_best_gt's det_img
  double* dets8;        // [nd][8]   gathered coordinates
  double* ovmax;        // [nd]
  int* jmax;            // [nd]
  int* slot;            // [ng]      the lowest sorted position that hits a record
  t1_u64* cum;          // [nd]      inclusive (fp << 32 | tp) inside a tile
  int* tile_hist;       // [tiles][nc]
  t1_u64* tile_sum;     // [tiles]
  double* rec;          // [nd]      when the caller passes none
  double* prec;         // [nd]
  double* terms;        // [nd + nc] the kept terms of voc_ap, class c at cls_off[c] + c
  size_t bytes;
};

static T1Ws t1_layout(void* base, int64_t nd, int64_t ng, int64_t nc) {
  const size_t rows = (size_t)(nd > 0 ? nd : 1), gts = (size_t)(ng > 0 ? ng : 1), tiles = (rows + kT1Tile - 1) / kT1Tile;
  T1Ws w;
  WsCursor c(base);
  w.key = c.take<t1_u64>(rows);
  w.idx = c.take<int>(rows);
  w.seg_in = c.take<int>(rows);
  w.order = c.take<int>(rows);
  w.seg = c.take<int>(rows);
  w.dets8 = c.take<double>(rows * 8);
  w.ovmax = c.take<double>(rows);
  w.jmax = c.take<int>(rows);
  w.slot = c.take<int>(gts);
  w.cum = c.take<t1_u64>(rows);
  w.tile_hist = c.take<int>(tiles * (size_t)nc);
  w.tile_sum = c.take<t1_u64>(tiles);
  w.rec = c.take<double>(rows);
  w.prec = c.take<double>(rows);
  w.terms = c.take<double>(rows + (size_t)nc);
  w.bytes = c.total();
  return w;
}

static bool t1_args_ok(int64_t det_stride, int64_t nd, int64_t ng, int64_t n_img, int64_t nc) {
  return det_stride >= 11 && nc >= 1 && nc <= kT1MaxNc && nd >= 0 && ng >= 0 && n_img >= 0 && nd < 0x80000000LL && ng < 0x80000000LL &&
         n_img < 0x80000000LL && nc * n_img < 0x80000000LL;
}

// the records of class c: gt_off[c * n_img] .. gt_off[(c + 1) * n_img], held inside [0, ng]
__global__ __launch_bounds__(kT1Threads) void k_t1_npos(const int32_t* __restrict__ gt_off, const uint8_t* __restrict__ difficult, int ng,
                                                         int n_img, int64_t* __restrict__ npos) {
  __shared__ int s_cnt;
  const int tid = threadIdx.x, c = blockIdx.x;
  if (tid == 0) s_cnt = 0;
  __syncthreads();
  const int g0 = max(0, min(gt_off[(size_t)c * n_img], ng)), g1 = max(g0, min(gt_off[(size_t)(c + 1) * n_img], ng));
  int cnt = 0;
  for (int g = g0 + tid; g < g1; g += kT1Threads) cnt += difficult[g] ? 0 : 1;
  if (cnt) atomicAdd(&s_cnt, cnt);
  __syncthreads();
  if (tid == 0) npos[c] = s_cnt;
}

__global__ __launch_bounds__(kT1Threads) void k_t1_key(const double* __restrict__ dets, long long det_stride, int nd, int nc, int n_img,
                                                        t1_u64* __restrict__ key, int* __restrict__ idx, int* __restrict__ seg_in,
                                                        int32_t* __restrict__ info) {
  __shared__ int s_bad;
  const int tid = threadIdx.x;
  if (tid == 0) s_bad = 0;
  __syncthreads();
  const long long i = (long long)blockIdx.x * kT1Threads + tid;
  if (i < nd) {
    const double* r = dets + i * det_stride;
    const long long c = vap::index_of(r[9], nc), im = vap::index_of(r[10], n_img);
    const bool bad = c < 0 || im < 0;
    if (bad) s_bad = 1;                                          // kept as segment 0 so that nothing is read out of bounds; the call reports it
    key[i] = vap::score_key_desc(r[8]);
    idx[i] = (int)i;
    seg_in[i] = bad ? 0 : (int)(c * n_img + im);
  }
  __syncthreads();
  if (tid == 0 && s_bad) atomicOr(&info[0], 1);
}

__global__ __launch_bounds__(kT1Threads) void k_t1_hist(const int* __restrict__ idx, const int* __restrict__ seg_in, int nd, int nc, int n_img,
                                                         int* __restrict__ tile_hist) {
  __shared__ int hist[kT1MaxNc];
  const int tid = threadIdx.x;
  hist[tid] = 0;
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kT1Items; k++) {
    const long long p = (long long)blockIdx.x * kT1Tile + k * kT1Threads + tid;
    if (p < nd) atomicAdd(&hist[seg_in[idx[p]] / n_img], 1);
  }
  __syncthreads();
  if (tid < nc) tile_hist[(size_t)blockIdx.x * nc + tid] = hist[tid];
}

// one workgroup, thread c = class c: tile_hist[t][c] becomes the rows of class c in the tiles before t; cls_off = exclusive scan of the totals
__global__ __launch_bounds__(kT1Threads) void k_t1_class_scan(int* __restrict__ tile_hist, int ntile, int nc, int nd, int32_t* __restrict__ cls_off) {
  __shared__ int tot[kT1MaxNc];
  const int tid = threadIdx.x;
  int run = 0;
  if (tid < nc)
    for (int t = 0; t < ntile; t++) {
      const int v = tile_hist[(size_t)t * nc + tid];
      tile_hist[(size_t)t * nc + tid] = run;
      run += v;
    }
  tot[tid] = run;
  __syncthreads();
  if (tid == 0) {
    int acc = 0;
    for (int c = 0; c < nc; c++) { const int v = tot[c]; tot[c] = acc; acc += v; }
  }
  __syncthreads();
  if (tid < nc) cls_off[tid] = tot[tid];
  if (tid == 0) cls_off[nc] = nd;
}

// Stable partition of the score order by class.  Wave w of a workgroup owns the positions tile * kT1Tile + w * 256 .. + 255 in four
// rounds of 64; the rank of a position among the earlier ones of its class: the wave's running count (LDS, one row per wave) + the
// lanes below it in the round (ballot), then the counts of the waves in front, the tiles in front and the class's first position.
__global__ __launch_bounds__(kT1Threads) void k_t1_scatter(const double* __restrict__ dets, long long det_stride, const int* __restrict__ idx,
                                                            const int* __restrict__ seg_in, int nd, int nc, int n_img,
                                                            const int* __restrict__ tile_hist, const int32_t* __restrict__ cls_off,
                                                            int32_t* __restrict__ order, int* __restrict__ seg, double* __restrict__ dets8) {
  __shared__ int wh[kT1Waves][kT1MaxNc];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
#pragma unroll
  for (int q = 0; q < kT1Waves; q++) wh[q][tid] = 0;
  __syncthreads();
  int row[kT1Items], sg[kT1Items], rk[kT1Items];
#pragma unroll
  for (int k = 0; k < kT1Items; k++) {
    const long long p = (long long)blockIdx.x * kT1Tile + w * (kT1Items * 64) + k * 64 + lane;
    const bool valid = p < nd;
    row[k] = valid ? idx[p] : 0;
    sg[k] = valid ? seg_in[row[k]] : -1;
    rk[k] = 0;
    const int c = valid ? sg[k] / n_img : -1;
    unsigned long long todo = __ballot(valid);
    while (todo) {                                               // one pass per class present in the round (wave-uniform)
      const int lead = __ffsll((long long)todo) - 1;
      const int cl = __shfl(c, lead);
      const unsigned long long m = __ballot(c == cl);
      if (c == cl) rk[k] = wh[w][cl] + __popcll(m & ((1ull << lane) - 1ull));
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");       // every lane has read the count before its lead moves it on,
      __builtin_amdgcn_wave_barrier();
      if (lane == lead) wh[w][cl] += __popcll(m);
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");       // and the next pass (or round) reads the new one
      __builtin_amdgcn_wave_barrier();
      todo &= ~m;
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kT1Items; k++) {
    if (sg[k] < 0) continue;
    const int c = sg[k] / n_img;
    int dst = cls_off[c] + tile_hist[(size_t)blockIdx.x * nc + c] + rk[k];
    for (int q = 0; q < w; q++) dst += wh[q][c];
    order[dst] = row[k];
    seg[dst] = sg[k];
    const double* r = dets + (long long)row[k] * det_stride;
    double2* o = reinterpret_cast<double2*>(dets8 + (size_t)dst * 8);
#pragma unroll
    for (int q = 0; q < 4; q++) o[q] = make_double2(r[2 * q], r[2 * q + 1]);
  }
}

// the record a detection points at, or -1: no hit (ovmax > ovthresh is false for NaN and -inf), or an index outside the set
__device__ __forceinline__ int t1_hit_record(double ov, int j, int sgm, const int32_t* __restrict__ gt_off, int ng, double ovthresh) {
  if (!(ov > ovthresh)) return -1;
  const long long g = (long long)gt_off[sgm] + j;
  return (j >= 0 && g >= 0 && g < ng) ? (int)g : -2;
}

__global__ __launch_bounds__(kT1Threads) void k_t1_claim(const double* __restrict__ ovmax, const int* __restrict__ jmax, const int* __restrict__ seg,
                                                          const int32_t* __restrict__ gt_off, const uint8_t* __restrict__ difficult, int nd, int ng,
                                                          double ovthresh, int* __restrict__ slot) {
  const long long p = (long long)blockIdx.x * kT1Threads + threadIdx.x;
  if (p >= nd) return;
  const int g = t1_hit_record(ovmax[p], jmax[p], seg[p], gt_off, ng, ovthresh);
  if (g >= 0 && !difficult[g]) atomicMin(&slot[g], (int)p);
}

// :225-233 per sorted position: no hit -> FP; a hit on a difficult record -> neither; on an easy one -> TP for the lowest position
// that hits it, FP for the others.  Thread t owns four consecutive positions; cum = the inclusive sum inside the tile.
__global__ __launch_bounds__(kT1Threads) void k_t1_mark(const double* __restrict__ ovmax, const int* __restrict__ jmax, const int* __restrict__ seg,
                                                         const int32_t* __restrict__ gt_off, const uint8_t* __restrict__ difficult,
                                                         const int* __restrict__ slot, int nd, int ng, double ovthresh, t1_u64* __restrict__ cum,
                                                         t1_u64* __restrict__ tile_sum) {
  __shared__ t1_u64 part[kT1Threads];
  const int tid = threadIdx.x;
  const long long p0 = (long long)blockIdx.x * kT1Tile + tid * kT1Items;
  t1_u64 v[kT1Items], sum = 0;
#pragma unroll
  for (int k = 0; k < kT1Items; k++) {
    const long long p = p0 + k;
    t1_u64 f = 0;
    if (p < nd) {
      const int g = t1_hit_record(ovmax[p], jmax[p], seg[p], gt_off, ng, ovthresh);
      if (g == -1) f = 1ull << 32;
      else if (g >= 0 && !difficult[g]) f = slot[g] == (int)p ? 1ull : 1ull << 32;
    }
    sum += f;
    v[k] = sum;
  }
  part[tid] = sum;
  __syncthreads();
  for (int d = 1; d < kT1Threads; d <<= 1) {
    const t1_u64 add = tid >= d ? part[tid - d] : 0;
    __syncthreads();
    part[tid] += add;
    __syncthreads();
  }
  const t1_u64 before = part[tid] - sum;
#pragma unroll
  for (int k = 0; k < kT1Items; k++)
    if (p0 + k < nd) cum[p0 + k] = before + v[k];
  if (tid == kT1Threads - 1) tile_sum[blockIdx.x] = part[tid];
}

// tile_sum[0 .. ntile) -> its exclusive scan in place, one workgroup: thread t sums a contiguous span, the spans are scanned in LDS
__global__ __launch_bounds__(kT1Threads) void k_t1_tile_scan(t1_u64* __restrict__ tile_sum, int ntile) {
  __shared__ t1_u64 part[kT1Threads];
  const int tid = threadIdx.x;
  const int span = (ntile + kT1Threads - 1) / kT1Threads;
  const int lo = (int)min((long long)tid * span, (long long)ntile), hi = min(lo + span, ntile);
  t1_u64 sum = 0;
  for (int t = lo; t < hi; t++) sum += tile_sum[t];
  part[tid] = sum;
  __syncthreads();
  for (int d = 1; d < kT1Threads; d <<= 1) {
    const t1_u64 add = tid >= d ? part[tid - d] : 0;
    __syncthreads();
    part[tid] += add;
    __syncthreads();
  }
  t1_u64 run = part[tid] - sum;
  for (int t = lo; t < hi; t++) {
    const t1_u64 v = tile_sum[t];
    tile_sum[t] = run;
    run += v;
  }
}

// counts up to and including position p, both in one word (fp << 32 | tp; each below 2^31: the halves never carry)
__device__ __forceinline__ t1_u64 t1_counts(const t1_u64* __restrict__ cum, const t1_u64* __restrict__ tile_base, long long p) {
  return cum[p] + tile_base[p / kT1Tile];
}

__global__ __launch_bounds__(kT1Threads) void k_t1_curve(const t1_u64* __restrict__ cum, const t1_u64* __restrict__ tile_base, const int* __restrict__ seg,
                                                          const int32_t* __restrict__ cls_off, const int64_t* __restrict__ npos, int nd, int n_img,
                                                          double* __restrict__ rec, double* __restrict__ prec) {
  const long long p = (long long)blockIdx.x * kT1Threads + threadIdx.x;
  if (p >= nd) return;
  const int c = seg[p] / n_img;
  const int first = cls_off[c];
  const t1_u64 d = t1_counts(cum, tile_base, p) - (first > 0 ? t1_counts(cum, tile_base, first - 1) : 0ull);
  const long long tp = (long long)(d & 0xffffffffull), fp = (long long)(d >> 32);
  rec[p] = vap::rec_of(tp, npos[c]);
  prec[p] = vap::prec_of(tp, fp);
}

// voc_ap of one class per workgroup.
// 11-point: every thread keeps the 11 running maxima of its strided share, waves join by shuffles, the four waves through LDS.
// All-point: the n + 1 terms are cut into one contiguous span per thread.  Pass 1: the span's np.maximum of mpre and its number of
// kept terms; a suffix scan of the maxima and a prefix scan of the counts in LDS; pass 2 walks the span backwards with the
// envelope and writes its kept terms at their final places; thread 0 then sums them as np.sum does (voc_ap_math.h).
__global__ __launch_bounds__(kT1Threads) void k_t1_ap(const double* __restrict__ rec, const double* __restrict__ prec,
                                                       const int32_t* __restrict__ cls_off, int use_07, double* __restrict__ terms,
                                                       double* __restrict__ ap) {
  __shared__ double s_max[kT1Threads];
  __shared__ int s_cnt[kT1Threads];
  __shared__ unsigned char s_has[kT1Threads];
  __shared__ double s_p[kT1Waves][vap::kPoints11];
  __shared__ unsigned s_any[kT1Waves];
  __shared__ vap::SumStack s_stack;
  const int tid = threadIdx.x, c = blockIdx.x;
  const int first = cls_off[c];
  const long long n = cls_off[c + 1] - first;
  const double* R = rec + first;
  const double* P = prec + first;
  if (use_07) {
    double m[vap::kPoints11];
    unsigned any = 0;
#pragma unroll
    for (int t = 0; t < vap::kPoints11; t++) m[t] = 0.;
    for (long long i = tid; i < n; i += kT1Threads) {
      const double r = R[i], pr = P[i];
#pragma unroll
      for (int t = 0; t < vap::kPoints11; t++)
        if (r >= vap::thr11(t)) {
          m[t] = ((any >> t) & 1u) ? vap::np_max(m[t], pr) : pr;
          any |= 1u << t;
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const unsigned oany = (unsigned)__shfl_xor((int)any, off);
#pragma unroll
      for (int t = 0; t < vap::kPoints11; t++) {
        const double om = __shfl_xor(m[t], off);
        if ((oany >> t) & 1u) m[t] = ((any >> t) & 1u) ? vap::np_max(m[t], om) : om;
      }
      any |= oany;
    }
    if ((tid & 63) == 0) {
#pragma unroll
      for (int t = 0; t < vap::kPoints11; t++) s_p[tid >> 6][t] = m[t];
      s_any[tid >> 6] = any;
    }
    __syncthreads();
    if (tid == 0) {
      for (int q = 1; q < kT1Waves; q++) {
        const unsigned oany = s_any[q];
#pragma unroll
        for (int t = 0; t < vap::kPoints11; t++)
          if ((oany >> t) & 1u) m[t] = ((any >> t) & 1u) ? vap::np_max(m[t], s_p[q][t]) : s_p[q][t];
        any |= oany;
      }
      ap[c] = vap::ap11_of(m, any);
    }
    return;
  }
  auto recf = [&](long long i) { return R[i]; };
  auto precf = [&](long long i) { return P[i]; };
  const long long ne = n + 1;                                    // terms e = 0 .. n
  const long long span = (ne + kT1Threads - 1) / kT1Threads;
  const long long lo = min((long long)tid * span, ne), hi = min(lo + span, ne);
  double lm = 0.;
  bool lany = false;
  int cnt = 0;
  for (long long e = lo; e < hi; e++) {
    vap::max_take(lm, lany, vap::mpre_at(e + 1, n, precf));
    cnt += vap::term_kept(vap::mrec_at(e + 1, n, recf), vap::mrec_at(e, n, recf)) ? 1 : 0;
  }
  s_max[tid] = lm; s_has[tid] = lany ? 1 : 0; s_cnt[tid] = cnt;
  __syncthreads();
  for (int d = 1; d < kT1Threads; d <<= 1) {
    const bool in = tid + d < kT1Threads;
    const double om = in ? s_max[tid + d] : 0.;
    const bool oh = in && s_has[tid + d];
    const int add = tid >= d ? s_cnt[tid - d] : 0;
    __syncthreads();
    double mm = s_max[tid];
    bool hh = s_has[tid] != 0;
    vap::max_join(mm, hh, om, oh);
    s_max[tid] = mm; s_has[tid] = hh ? 1 : 0; s_cnt[tid] += add;
    __syncthreads();
  }
  // the envelope behind the span: the spans of the threads above (none above the last one, whose span ends with mpre[n + 1] = 0)
  double env = tid + 1 < kT1Threads ? s_max[tid + 1] : 0.;
  bool eany = tid + 1 < kT1Threads && s_has[tid + 1];
  const long long kept = s_cnt[kT1Threads - 1];
  double* T = terms + first + c;
  long long wpos = s_cnt[tid];                                   // one behind the span's last kept term
  for (long long e = hi - 1; e >= lo; e--) {
    const double v = vap::mpre_at(e + 1, n, precf);
    env = eany ? vap::np_max(v, env) : v;
    eany = true;
    const double r1 = vap::mrec_at(e + 1, n, recf), r0 = vap::mrec_at(e, n, recf);
    if (vap::term_kept(r1, r0)) T[--wpos] = vap::term_of(r1, r0, env);
  }
  __threadfence_block();
  __syncthreads();
  if (tid == 0) ap[c] = vap::np_sum([&](long long i) { return T[i]; }, kept, &s_stack);
}

static int run_task1_eval(const double* dets, int64_t det_stride, int64_t nd, const double* gts8, const int32_t* gt_off, const uint8_t* difficult,
                          int64_t ng, int64_t n_img, int64_t nc, double ovthresh, int flags, double* ap, int64_t* npos, int32_t* cls_off,
                          int32_t* order, double* rec, double* prec, int32_t* info, void* ws, size_t ws_extent, hipStream_t st) {
  if (!t1_args_ok(det_stride, nd, ng, n_img, nc) || (flags & ~OBB_TASK1_EVAL_07_METRIC) || !ap || !npos || !cls_off || !info || !gt_off ||
      (nd > 0 && !dets) || (ng > 0 && (!gts8 || !difficult)))
    return OBB_ERR_BAD_ARG;
  const T1Ws w = t1_layout(ws, nd, ng, nc);
  if (!ws_ok(ws, ws_extent, w.bytes)) return OBB_ERR_WORKSPACE;
  if (hipMemsetAsync(info, 0, 2 * sizeof(int32_t), st) != hipSuccess) return OBB_ERR_LAUNCH;
  k_t1_npos<<<(unsigned)nc, kT1Threads, 0, st>>>(gt_off, difficult, (int)ng, (int)n_img, npos);
  if (nd == 0 || n_img == 0) {                                   // no image: every row names one that is not listed
    if (hipMemsetAsync(ap, 0, (size_t)nc * sizeof(double), st) != hipSuccess) return OBB_ERR_LAUNCH;
    if (hipMemsetAsync(cls_off, 0, (size_t)(nc + 1) * sizeof(int32_t), st) != hipSuccess) return OBB_ERR_LAUNCH;
    if (nd > 0 && hipMemsetD32Async((hipDeviceptr_t)info, 1, 1, st) != hipSuccess) return OBB_ERR_LAUNCH;
    return hipGetLastError() == hipSuccess ? OBB_OK : OBB_ERR_LAUNCH;
  }
  const unsigned rows_grid = (unsigned)((nd + kT1Threads - 1) / kT1Threads), ntile = (unsigned)((nd + kT1Tile - 1) / kT1Tile);
  int32_t* ord = order ? order : w.order;
  double* r = rec ? rec : w.rec;
  double* p = prec ? prec : w.prec;
  k_t1_key<<<rows_grid, kT1Threads, 0, st>>>(dets, det_stride, (int)nd, (int)nc, (int)n_img, w.key, w.idx, w.seg_in, info);
  bitonic_sort_pairs(w.key, w.idx, (unsigned)nd, st);
  k_t1_hist<<<ntile, kT1Threads, 0, st>>>(w.idx, w.seg_in, (int)nd, (int)nc, (int)n_img, w.tile_hist);
  k_t1_class_scan<<<1, kT1Threads, 0, st>>>(w.tile_hist, (int)ntile, (int)nc, (int)nd, cls_off);
  k_t1_scatter<<<ntile, kT1Threads, 0, st>>>(dets, det_stride, w.idx, w.seg_in, (int)nd, (int)nc, (int)n_img, w.tile_hist, cls_off, ord, w.seg, w.dets8);
  if (hipGetLastError() != hipSuccess) return OBB_ERR_LAUNCH;
  if (const int rc = launch_eval_best_gt(w.dets8, w.seg, nd, gts8, gt_off, w.ovmax, w.jmax, st)) return rc;
  if (hipMemsetD32Async((hipDeviceptr_t)w.slot, 0x7fffffff, (size_t)(ng > 0 ? ng : 1), st) != hipSuccess) return OBB_ERR_LAUNCH;   // above every position
  k_t1_claim<<<rows_grid, kT1Threads, 0, st>>>(w.ovmax, w.jmax, w.seg, gt_off, difficult, (int)nd, (int)ng, ovthresh, w.slot);
  k_t1_mark<<<ntile, kT1Threads, 0, st>>>(w.ovmax, w.jmax, w.seg, gt_off, difficult, w.slot, (int)nd, (int)ng, ovthresh, w.cum, w.tile_sum);
  k_t1_tile_scan<<<1, kT1Threads, 0, st>>>(w.tile_sum, (int)ntile);
  k_t1_curve<<<rows_grid, kT1Threads, 0, st>>>(w.cum, w.tile_sum, w.seg, cls_off, npos, (int)nd, (int)n_img, r, p);
  k_t1_ap<<<(unsigned)nc, kT1Threads, 0, st>>>(r, p, cls_off, flags & OBB_TASK1_EVAL_07_METRIC, w.terms, ap);
  return hipGetLastError() == hipSuccess ? OBB_OK : OBB_ERR_LAUNCH;
}

}  // namespace obb
