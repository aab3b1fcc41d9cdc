// The front of the fused non_max_suppression_obb (namespace obb; the pipeline is described in nmsobb_impl.h): the filter kernel
// k_decode over the decoded prediction tensor, k_append_extra for the apriori label rows, and what every front kernel shares with
// them -- the class mask, the products and thresholds in the tensor dtype, the wave arg-max, DecodeArgs and the per-image flags.
// nms_head.h builds the conv-layout front kernels on the same pieces.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>

#include "dtype_device.h"
#include "nms_driver.h"
#include "nms_limits.h"
#include "obb_device.h"

namespace obb {

struct ClassMask { unsigned long long w[4]; int all; };   // allowed classes (nc <= 256), all != 0: no filter

// product rounded to the tensor dtype: x[:, 5:ci] *= x[:, 4:5] happens in the input dtype (utils/general.py:820)
template <typename T> __device__ __forceinline__ float mul_in_dtype(float a, float b);
template <> __device__ __forceinline__ float mul_in_dtype<float>(float a, float b) { return a * b; }
template <> __device__ __forceinline__ float mul_in_dtype<__half>(float a, float b) { return __half2float(__float2half_rn(a * b)); }
// (bf16: two 8-bit significands give a 16-bit product, exact in fp32, so the one rounding below is torch's bf16 multiply bit for bit)
template <> __device__ __forceinline__ float mul_in_dtype<bf16_t>(float a, float b) { return round_to_dtype<bf16_t>(a * b); }
// python float threshold compared against a tensor of the input dtype: the scalar is cast to that dtype
template <typename T> __device__ __forceinline__ float thr_in_dtype(float t);
template <> __device__ __forceinline__ float thr_in_dtype<float>(float t) { return t; }
template <> __device__ __forceinline__ float thr_in_dtype<__half>(float t) { return __half2float(__float2half_rn(t)); }
template <> __device__ __forceinline__ float thr_in_dtype<bf16_t>(float t) { return round_to_dtype<bf16_t>(t); }

// wave arg-max with "first maximum" tie rule (torch.max over a dimension: utils/general.py:822, :830).  Value and index
// travel as ONE 64-bit key -- order-preserving image of the float in the high word (-0 counts as +0; every NaN, of either
// sign and any payload, maps to the one key 0xFFFFFFFF above +inf: torch.max / torch.argmax rank a NaN as the maximum and
// take the first of several), ~index in the low word -- so the reduction is a plain unsigned max: four DPP steps inside the
// 16-lane rows (quad swaps, half-row and row mirrors: a few cycles each, where ds_bpermute costs an LDS round trip per
// step), then the four row results meet through v_readlane.
__device__ __forceinline__ unsigned long long argmax_key(float v, int i) {
  const uint32_t b = __float_as_uint(v + 0.0f);
  const uint32_t m = (v != v) ? 0xFFFFFFFFu : (b & 0x80000000u) ? ~b : (b | 0x80000000u);   // (unkeyed: a NaN)
  return ((unsigned long long)m << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)i);
}
template <int CTRL>
__device__ __forceinline__ unsigned long long dpp_max_u64(unsigned long long k) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)k, CTRL, 0xF, 0xF, true);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(k >> 32), CTRL, 0xF, 0xF, true);
  const unsigned long long o = ((unsigned long long)hi << 32) | lo;
  return o > k ? o : k;
}
__device__ __forceinline__ unsigned long long row_max_u64(unsigned long long k) {    // all 64 lanes active
  k = dpp_max_u64<0xB1>(k);      // quad_perm [1,0,3,2]
  k = dpp_max_u64<0x4E>(k);      // quad_perm [2,3,0,1]
  k = dpp_max_u64<0x141>(k);     // row_half_mirror
  return dpp_max_u64<0x140>(k);  // row_mirror: every lane holds the max of its 16-lane row
}
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long k) {   // all 64 lanes active
  k = row_max_u64(k);
  unsigned long long r[4];
#pragma unroll
  for (int j = 0; j < 4; j++)
    r[j] = ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(k >> 32), j * 16) << 32) |
           (unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)k, j * 16);
  const unsigned long long a = r[0] > r[1] ? r[0] : r[1], b = r[2] > r[3] ? r[2] : r[3];
  return a > b ? a : b;
}
__device__ __forceinline__ void argmax_unkey(unsigned long long k, float& v, int& i) {
  const uint32_t m = (uint32_t)(k >> 32);
  v = __uint_as_float((m & 0x80000000u) ? (m ^ 0x80000000u) : ~m);
  i = (int)(0xFFFFFFFFu - (uint32_t)k);
}
__device__ __forceinline__ void wave_argmax_first(float& v, int& i) {
  argmax_unkey(wave_max_u64(argmax_key(v, i)), v, i);
}

struct DecodeArgs {
  const void* pred;          // [bs][A][no]
  const void* objcol;        // [bs][A] = pred[..., 4] stored densely by the producer (obb_detect_decode_col), or null
  long long A;
  int no, nc, bs;
  float conf_thres;
  int multi_label;
  int rows_per_thread;       // G: a workgroup of k_decode covers kDecThreads * G rows
  ClassMask cm;
  long long cap_img;         // candidate slots per image
  float4* cand;              // [bs*cap_img][2]: {x,y,l,s} {theta,conf,cls,0}
  unsigned long long* keys;  // [bs*cap_img]
  uint32_t* vals;            // [bs*cap_img] slot index inside the image region
  int* cnt;                  // [bs * kCntPad] candidates produced (may exceed cap_img: overflow), one 256-B line each
  int* tiny;                 // [bs] flags of the image (kImg*): what decides whether its classes may run as independent NMS segments
  float win_lo, win_hi;      // every candidate's circle must lie in win_lo < x < win_hi (a window narrower than max_wh), else kImgWide
  // state of the LATER launches that this kernel zeroes on its way (a call with caller-kept counters has no reset launch:
  // obb_non_max_suppression_obb_st); all NULL / 0: k_reset_state did it
  int* z_ticket; int n_ticket;
  uint4* z_bar16; long long n_bar16;
  uint4* z_alive16; long long n_alive16;
};

// Per-image flags (DecodeArgs::tiny).  The reference runs ONE list per image with xy += cls * max_wh (utils/general.py:849-851);
// one NMS segment per class gives the same kept set exactly when no pair of boxes of DIFFERENT classes can interact:
//   kImgSmall   a candidate has a short side in [0.001, 1) px: the reference's fp32 corner arithmetic is ill conditioned for such a
//               box against a partner tens of thousands of pixels away (riou_device.h: rbox_pair_well_conditioned) and can
//               report an overlap there.  Such an image keeps its class segments only if k_tiny_cross has CHECKED every
//               ill-conditioned cross-class pair with the exact clip and found no IoU > thr (round 5; rounds 1-4: single list);
//   kImgWide    a candidate's circle leaves the window [win_lo, win_hi] on x (an oversized or far-out box, NaN / inf): circles
//               of different classes could really touch -- always the single list;
//   kImgChecked k_tiny_cross ran for the image and completed its list of small boxes;   kImgCross  it found a cross-class hit.
constexpr int kImgSmall = 1, kImgWide = 2, kImgChecked = 4, kImgCross = 8;
__host__ __device__ __forceinline__ bool img_single_list(int t) {
  return (t & kImgWide) || ((t & kImgSmall) && (!(t & kImgChecked) || (t & kImgCross)));
}
__device__ __forceinline__ int cand_flags(float x, float l, float s, float win_lo, float win_hi) {
  const float mn = min_nan(l, s);
  const float rr = sqrtf(l * l + s * s) * 0.501f + 0.5f;
  int f = (mn >= 0.001f && mn < 1.0f) ? kImgSmall : 0;
  if (!(x - rr > win_lo && x + rr < win_hi)) f |= kImgWide;     // (NaN / inf anywhere: the comparisons fail)
  return f;
}

__device__ __forceinline__ bool class_allowed(const ClassMask& cm, int c) {
  const int q = (c >> 6) & 3;   // select chain instead of a dynamic index: the mask lives in kernel-argument SGPRs
  const unsigned long long w = q == 0 ? cm.w[0] : q == 1 ? cm.w[1] : q == 2 ? cm.w[2] : cm.w[3];
  return cm.all || ((w >> (c & 63)) & 1ull);
}

// Candidate counters are padded to one 256-byte line each: same-word device atomics retire at ~11 ns apiece
// (MI355X_MICROARCH.md "fanin"/"dequeue"), and 16 counters packed in one line would share one L2 channel.
constexpr int kCntPad = 64;   // ints

// Rows of a workgroup = kDecThreads * G (G = 1, 2 or 4 rows per thread, chosen by the host so that small batches still fill the
// chip).  History: with one wave per 64 consecutive rows that also processed ITS passing rows one after the other, the
// kernel took 52 us on a warm and 78-91 us on a freshly written configs[1] tensor -- even with the dense objectness column:
// detector output is clustered (an object fires on neighbouring cells), so a few waves carried long serial chains of cold
// row reads while most had none.  Now the workgroup compacts its passing rows into LDS and its four waves take them
// round-robin, kDecDepth rows in flight per wave.
constexpr int kDecWaves = kDecThreads / 64;
constexpr int kDecMaxG = 4;
constexpr int kDecDepth = 2;          // groups of four rows in flight per wave
constexpr int kDecStage = 128;         // staged candidates per wave (LDS) before a flush

// Phase 2 of k_decode works on FOUR rows per wave, one per 16-lane DPP row: a row of the head output holds ~200 elements,
// and with a whole wave per row most of every instruction was bookkeeping (measured: ~450 wave instructions per row,
// VALU-bound).  Lane l16 of a group holds angle bins l16, l16+16, ... (12 registers), classes l16 and 16+l16 (further
// class groups of 16 are loaded on demand: nc > 32), and the box.  Everything a group needs is requested up front.
constexpr int kDecCslRegs = 12;          // ceil(180 / 16)
constexpr int kDecClsRegs = 2;           // class groups of 16 that travel with the row
#ifdef OBB_DECODE_TRACE
// (development builds, tools/decode_trace.sh) 16 words per workgroup of the last k_decode launch: 1, entry, after the first barrier,
// objectness used by the first / the last wave, list built, rows reduced by the first / the last wave, slot atomic returned, exit
// (wall_clock64 ticks of 10 ns), then n_rows and the candidates the workgroup staged.  The waves meet in LDS; thread 0 stores the record.
constexpr int kDecTraceWgs = 2048;
__device__ unsigned long long g_decode_trace[kDecTraceWgs * 16];
#define DTRACE_DECL() __shared__ unsigned long long s_tr[16]; if (threadIdx.x < 16) s_tr[threadIdx.x] = (threadIdx.x == 3 || threadIdx.x == 6) ? ~0ull : 0ull; \
  if (threadIdx.x == 0) s_tr[1] = wall_clock64()
#define DTRACE_T0(slot) do { if (threadIdx.x == 0) s_tr[slot] = wall_clock64(); } while (0)
#define DTRACE_WAVE(slot_min, slot_max) do { if ((threadIdx.x & 63) == 0) { const unsigned long long t_ = wall_clock64(); \
  atomicMin(&s_tr[slot_min], t_); atomicMax(&s_tr[slot_max], t_); } } while (0)
#define DTRACE_ADD(slot, v) do { if ((threadIdx.x & 63) == 0) atomicAdd(&s_tr[slot], (unsigned long long)(v)); } while (0)
#define DTRACE_END(n_rows) do { DTRACE_WAVE(15, 9); __syncthreads(); \
  const unsigned wg_ = blockIdx.y * gridDim.x + blockIdx.x; \
  if (threadIdx.x < 16 && wg_ < (unsigned)kDecTraceWgs) g_decode_trace[wg_ * 16 + threadIdx.x] = threadIdx.x == 0 ? 1ull : threadIdx.x == 10 ? (unsigned long long)(n_rows) : s_tr[threadIdx.x]; } while (0)
#else
#define DTRACE_DECL() do {} while (0)
#define DTRACE_T0(slot) do {} while (0)
#define DTRACE_WAVE(slot_min, slot_max) do {} while (0)
#define DTRACE_ADD(slot, v) do {} while (0)
#define DTRACE_END(n_rows) do {} while (0)
#endif

template <typename T>
struct DecQuad {
  float csl[kDecCslRegs];
  float cls[kDecClsRegs];
  float box[4];
  float obj;
  uint32_t row;
  bool valid;
};

// Every load of a row is UNCONDITIONAL: a lane that wants nothing reads element 0 of its row (of row 0 for a lane without a row), and
// what it read is dropped where it would be USED (reduce_quad: the key of a bin >= 180 is 0, a class >= nc is not looked at), never by
// a select on the loaded value here.  A load under `cond ? *p : x` -- and a select straight on a loaded value, which the compiler
// turns back into such a branch -- is compiled with the wait for its result inside the branch: that made the 18 (and, in phase 1,
// the 4) loads of a lane 18 dependent round trips (profiles/decode_trace_before.md).  Check the assembly after touching this.
template <typename T>
__device__ __forceinline__ DecQuad<T> dec_load_quad(const T* img, int no, int nc, const uint32_t* s_row, const float* s_obj,
                                                    int j, int n_rows, int l16) {
  DecQuad<T> r;
  r.valid = j < n_rows;
  r.row = r.valid ? s_row[j] : 0u;
  r.obj = r.valid ? s_obj[j] : 0.f;
  const T* base = img + (size_t)r.row * (uint32_t)no;
  const T* csl = base + 5 + nc;
#pragma unroll
  for (int k = 0; k < kDecCslRegs; k++) r.csl[k] = ld_as_float<T>((k * 16 + l16 < 180) ? csl + k * 16 + l16 : base);
#pragma unroll
  for (int g = 0; g < kDecClsRegs; g++) r.cls[g] = ld_as_float<T>((g * 16 + l16 < nc) ? base + 5 + g * 16 + l16 : base);
#pragma unroll
  for (int k = 0; k < 4; k++) r.box[k] = ld_as_float<T>(base + k);
  return r;
}

// k_decode: workgroup = 512 threads x G rows.  Phase 1 reads the objectness of every row -- from the dense column when the
// producer stored one (obb_detect_decode_col), else one 2-4 byte element of each 400-800 byte row -- and compacts the rows
// with obj > conf into an LDS list (wave ballot + one LDS atomic per wave).  Phase 2: the four waves take the listed rows
// round-robin in groups of four (DecQuad above), kDecDepth groups in flight per wave, and stage the candidates in LDS.  Slots in the image's candidate region are claimed with ONE atomic per workgroup (plus
// one per wave whenever its 128-entry stage fills up) and the staged records are written out coalesced.
template <typename T>
__global__ __launch_bounds__(kDecThreads) void k_decode(DecodeArgs a) {
  __shared__ float4 s_c0[kDecWaves][kDecStage], s_c1[kDecWaves][kDecStage];
  __shared__ unsigned long long s_key[kDecWaves][kDecStage];
  __shared__ int s_cnt[kDecWaves], s_base, s_n;
  __shared__ uint32_t s_row[kDecThreads * kDecMaxG];
  __shared__ float s_obj[kDecThreads * kDecMaxG];

  const T* pred = (const T*)a.pred;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int b = blockIdx.y;
  const int G = a.rows_per_thread;
  const float thr = thr_in_dtype<T>(a.conf_thres);
  const T* img = pred + (size_t)b * a.A * a.no;
  float4* cand = a.cand + (size_t)b * a.cap_img * 2;
  unsigned long long* keys = a.keys + (size_t)b * a.cap_img;
  uint32_t* vals = a.vals + (size_t)b * a.cap_img;
  float4* c0s = s_c0[wv]; float4* c1s = s_c1[wv]; unsigned long long* kys = s_key[wv];
  int staged = 0;   // wave-uniform
  int flags_seen = 0;
  if (tid == 0) s_n = 0;
  DTRACE_DECL();

  auto write_out = [&](long long base, int count) {
    for (int i = lane; i < count; i += 64) {
      const long long slot = base + i;
      if (slot < a.cap_img) {
        cand[slot * 2] = c0s[i];
        cand[slot * 2 + 1] = c1s[i];
        keys[slot] = kys[i];
        vals[slot] = (uint32_t)slot;
      }
    }
  };
  auto flush_wave = [&]() {   // mid-kernel flush of a full stage: one atomic for the wave
    int base = 0;
    if (lane == 0) base = atomicAdd(&a.cnt[b * kCntPad], staged);
    base = __shfl(base, 0);
    write_out(base, staged);
    staged = 0;
  };

  // ---- phase 1: objectness of the workgroup's rows                    :785  xc = prediction[..., 4] > conf_thres
  float obj[kDecMaxG];
  // 16-row chunks are dealt to the workgroups of the image round-robin (chunk c -> workgroup c % gridDim.x): detector output
  // is clustered -- a coarse level holds hundreds of passing rows in a few thousand consecutive rows.  Contiguous 1024-row
  // blocks left a handful of workgroups with ten times the average number of rows to reduce, 64-row chunks still three
  // times (0 / 14 / 44 rows: min / median / max on the planted-object batch); the objectness reads do not care (a strided
  // read is one line per row anyway, the dense column is read in 32-byte pieces).
  auto row_of = [&](int q) -> long long { return ((long long)(q * (kDecThreads / 16) + (tid >> 4)) * gridDim.x + blockIdx.x) * 16 + (tid & 15); };
  // (unconditional loads, all kDecMaxG in flight before the first is used: a lane without a row -- q >= G, or behind the image's
  // last row -- reads the image's last row, and the value is not looked at)
  const T* ocol = a.objcol ? (const T*)a.objcol + (size_t)b * a.A : img + 4;          // 128 bytes per wave : one line per row
  const long long ostride = a.objcol ? 1 : a.no;
#pragma unroll
  for (int q = 0; q < kDecMaxG; q++) {
    const long long row = row_of(q);
    obj[q] = ld_as_float<T>(ocol + (size_t)(row < a.A ? row : a.A - 1) * ostride);
  }
  // The state of the later launches that the call's plan wants zeroed (kernel-uniform: what k_reset_state zeroes for a call without
  // caller-kept counters).  Nothing in this kernel reads it: the stores go out behind the objectness loads and are not waited for.
  if (a.z_ticket != nullptr) {
    const long long i = ((long long)blockIdx.y * gridDim.x + blockIdx.x) * kDecThreads + tid, n = (long long)gridDim.x * gridDim.y * kDecThreads;
    if (i < a.n_ticket) a.z_ticket[i] = 0;
    for (long long k = i; k < a.n_bar16; k += n) a.z_bar16[k] = make_uint4(0u, 0u, 0u, 0u);
    for (long long k = i; k < a.n_alive16; k += n) a.z_alive16[k] = make_uint4(0u, 0u, 0u, 0u);
  }
  __syncthreads();                                               // (s_n = 0 before the first wave counts its rows)
  DTRACE_T0(2);
#pragma unroll
  for (int q = 0; q < kDecMaxG; q++) {
    const bool p = q < G && row_of(q) < a.A && obj[q] > thr;
    const unsigned long long mk = __ballot(p);
    if (mk) {
      int base = 0;
      if (lane == 0) base = atomicAdd(&s_n, __popcll(mk));
      base = __shfl(base, 0);
      if (p) {
        const int i = base + __popcll(mk & lanemask_lt());
        s_row[i] = (uint32_t)row_of(q);
        s_obj[i] = obj[q];
      }
    }
  }
  DTRACE_WAVE(3, 4);
  __syncthreads();
  DTRACE_T0(5);
  const int n_rows = s_n;

  // ---- phase 2: the listed rows in groups of four (one per 16-lane row); wave wv takes groups wv, wv + 8, ...,
  // kDecDepth groups requested before the first is reduced
  const int l16 = lane & 15, sub = lane >> 4;
  const int ncg = (a.nc + 15) >> 4;
  // what every candidate of a row shares
  struct RowOut { float bx, by, bl, bs_, theta; int bflags; long long rw; };
  auto stage = [&](const RowOut& o, bool p, float conf, int c) {        // one candidate per lane with p set
    const unsigned long long pb = __ballot(p);
    const int np = __popcll(pb);
    if (np == 0) return;
    if (staged + np > kDecStage) flush_wave();
    if (p) {
      const int i = staged + __popcll(pb & lanemask_lt());
      c0s[i] = make_float4(o.bx, o.by, o.bl, o.bs_);
      c1s[i] = make_float4(o.theta, conf, (float)c, 0.f);
      kys[i] = ((unsigned long long)score_desc_key(conf) << 32) | (unsigned long long)(uint32_t)(o.rw * a.nc + c);
      flags_seen |= o.bflags;
    }
    staged += np;
    DTRACE_ADD(11, np);
  };
  auto row_out = [&](float bx, float by, float bl, float bs_, unsigned long long tk, uint32_t row) {
    float tv; int ti;
    argmax_unkey(row_max_u64(tk), tv, ti);     // CSL decode: first arg-max over the 180 bins (:822-823), inside the 16-lane row
    RowOut o;
    o.bx = bx; o.by = by; o.bl = bl; o.bs_ = bs_;
    o.theta = ((float)(ti - 90) / 180.0f) * 3.141592f;
    o.bflags = cand_flags(bx, bl, bs_, a.win_lo, a.win_hi);
    o.rw = (long long)row;
    return o;
  };
  // :830 best class of the row (a NaN maximum fails bv > thr: the row is dropped), :831, :835
  auto stage_best = [&](const RowOut& o, bool valid, unsigned long long bestk) {
    float bv; int bi;
    argmax_unkey(row_max_u64(bestk), bv, bi);
    stage(o, valid && l16 == 0 && bv > thr && class_allowed(a.cm, bi), bv, bi);
  };
  auto reduce_quad = [&](const DecQuad<T>& cur) __attribute__((always_inline)) {
    unsigned long long tk = argmax_key(cur.csl[0], l16);
#pragma unroll
    for (int k = 1; k < kDecCslRegs; k++) {             // (key 0, below the key of every value, for what a lane read in place of a bin >= 180)
      const unsigned long long kk = (k * 16 + l16 < 180) ? argmax_key(cur.csl[k], k * 16 + l16) : 0ull;
      tk = kk > tk ? kk : tk;
    }
    const RowOut o = row_out(cur.box[0], cur.box[1], cur.box[2], cur.box[3], tk, cur.row);
    // class confidences (:820 conf = obj * cls in the input dtype)
    unsigned long long bestk = argmax_key(-__builtin_inff(), 0x7fffffff);
    for (int g = 0; g < ncg; g++) {
      const int c = g * 16 + l16;
      float raw;
      if (g < kDecClsRegs) raw = (g == 0) ? cur.cls[0] : cur.cls[1];
      else raw = (cur.valid && c < a.nc) ? ld_as_float<T>(img + (size_t)cur.row * a.no + 5 + c) : 0.f;
      const float v = (cur.valid && c < a.nc) ? mul_in_dtype<T>(raw, cur.obj) : -__builtin_inff();
      if (a.multi_label) stage(o, cur.valid && c < a.nc && v > thr && class_allowed(a.cm, c), v, c);             // :827, :835
      else if (c < a.nc) { const unsigned long long kk = argmax_key(v, c); bestk = kk > bestk ? kk : bestk; }   // a NaN wins
    }
    if (!a.multi_label) stage_best(o, cur.valid, bestk);
  };
  static_assert(kDecClsRegs == 2, "reduce_quad selects cls[0] / cls[1] explicitly");
  for (int g0 = wv; g0 * 4 < n_rows; g0 += kDecWaves * kDecDepth) {
    DecQuad<T> quads[kDecDepth];
#pragma unroll
    for (int i = 0; i < kDecDepth; i++) {
      const int g = g0 + kDecWaves * i;
      if (g * 4 < n_rows) quads[i] = dec_load_quad<T>(img, a.no, a.nc, s_row, s_obj, g * 4 + sub, n_rows, l16);
    }
#pragma unroll
    for (int i = 0; i < kDecDepth; i++) {
      const int g = g0 + kDecWaves * i;
      if (g * 4 < n_rows) reduce_quad(quads[i]);
    }
  }

  {
    const int fl = (__ballot(flags_seen & kImgSmall) ? kImgSmall : 0) | (__ballot(flags_seen & kImgWide) ? kImgWide : 0);
    if (fl && lane == 0) atomicOr(&a.tiny[b], fl);
  }
  DTRACE_WAVE(6, 7);
  // ---- one atomic per workgroup for whatever is still staged
  if (lane == 0) s_cnt[wv] = staged;
  __syncthreads();
  if (threadIdx.x == 0) {
    int tot = 0;
    for (int w = 0; w < kDecWaves; w++) tot += s_cnt[w];
    s_base = tot ? atomicAdd(&a.cnt[b * kCntPad], tot) : 0;
  }
  __syncthreads();
  DTRACE_T0(8);
  int base = s_base;
  for (int w = 0; w < wv; w++) base += s_cnt[w];
  write_out(base, staged);
  DTRACE_END(n_rows);
}

// apriori label rows (utils/general.py:807-813), prepared by the host layer as [img, x, y, l, s, theta, conf, cls]
__global__ void k_append_extra(const float* __restrict__ extra8, int m, long long A, int nc, DecodeArgs a) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const float* e = extra8 + (size_t)i * 8;
  const int b = (int)e[0];
  if (b < 0 || b >= a.bs) return;
  // a label row is a candidate like any other (:807-813 append it in front of the filters): conf = 1 > conf_thres (:827 / :831) and
  // the class filter (:835) apply to it -- until round 6 the class filter did not (found by tools/self_fuzz.py: `labels` + `classes`)
  if (!(e[6] > a.conf_thres) || !class_allowed(a.cm, (int)e[7])) return;
  const int slot = atomicAdd(&a.cnt[b * kCntPad], 1);
  { const int fl = cand_flags(e[1], e[3], e[4], a.win_lo, a.win_hi); if (fl) atomicOr(&a.tiny[b], fl); }
  if (slot >= a.cap_img) return;
  const size_t g = (size_t)b * a.cap_img + slot;
  a.cand[g * 2] = make_float4(e[1], e[2], e[3], e[4]);
  a.cand[g * 2 + 1] = make_float4(e[5], e[6], e[7], 0.f);
  a.keys[g] = ((unsigned long long)score_desc_key(e[6]) << 32) | (unsigned long long)(uint32_t)(A * nc + i);
  a.vals[g] = (uint32_t)slot;
}

}  // namespace obb
