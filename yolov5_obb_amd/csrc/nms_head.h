// Front kernel of obb_non_max_suppression_obb_head (namespace obb; built on nmsobb_front.h, launched by the driver of nmsobb_impl.h).
//
// k_decode_head does the work of k_decode -- confidence filter, conf = obj * cls, multi-label expansion or best class, CSL
// arg-max, class filter, candidate records and sort keys -- but reads the Detect head's 1x1-conv outputs (bs, na*no, ny, nx)
// instead of the decoded prediction tensor z (bs, A, no) that Detect.forward would build from them (models/yolo.py:61-81).
// The decode is a per-element function of the conv output (detect_math.h), so every value k_decode would read from z is
// recomputed here with the same arithmetic and rounding; z and the permuted raw head x are never written.
//
// Workgroup = (level tile of kHeadTile<T> consecutive positions p = y*nx + x, image b, anchor a): 256 threads.
//   phase 1  the tile's objectness line (channel a*no + 4: kHeadTile<T> contiguous elements, 256 bytes), decoded exactly as z[..., 4]
//            is -- round_to_dtype(sigmoid(raw)) -- and compared with the threshold in the tensor dtype (utils/general.py:785).  A
//            tile where nothing passes is done after this one line.
//   phase 2  the tile's no channel lines (256 bytes each) are staged in LDS, and each passing position is reduced from there by a
//            16-lane group exactly as k_decode's reduce_quad reduces a row of z.  Rows of z are numbered as Detect numbers them,
//            a_off[level] + a*ny*nx + p: the sort keys, and with them tie order and kept list, are those of the eager chain.
//
// k_decode_head<T, true> is the front kernel of obb_non_max_suppression_obb_tta_head (augmented inference, models/yolo.py:149-209):
// the same workgroup over the (pass, level) entries of HeadFrontTta (tta_head_plan.h) instead of the levels of HeadFront.  What differs:
// the table is searched over up to 16 entries; the load width of phase 2a is the ENTRY's (16, 8 bytes or element-wise); the four box
// channels go through detect_descale_one with the entry's inv_scale / flip / image size after detect_decode_one, as
// k_detect_decode_tta writes them into z (channel 4 and above are not de-scaled: phase 1 is the same).  a_off[entry] is the row the
// entry starts at in torch.cat(_clip_augmented(y), 1), so keys, tie order and kept list are those of obb_detect_decode_tta followed
// by the eager NMS.  Everything under `if constexpr (TTA)` is compiled into that instantiation only.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>

#include "detect_math.h"
#include "dtype_device.h"
#include "launch_once.h"
#include "nms_driver.h"
#include "nmsobb_front.h"
#include "obb_device.h"
#include "obb_hip.h"
#include "tta_head_plan.h"

namespace obb {

constexpr int kHeadMaxLevels = 4;          // P3 .. P6, the limit of obb_detect_decode_levels
constexpr int kHeadThreads = 256;
constexpr int kHeadWaves = kHeadThreads / 64;
constexpr int kHeadStage = 128;            // staged candidates per wave before a flush (k_decode's kDecStage)
constexpr int kHeadPitchDw = 65;           // LDS pitch of a channel line: 256 bytes + one bank, so that the 16 lanes of a group
                                           // (16 consecutive channels of one position) hit 16 different banks
template <typename T> constexpr int kHeadTile = 256 / (int)sizeof(T);   // positions per tile: one 256-byte line per channel (fp16 and bf16: 128)

struct HeadFront {
  const void* in[kHeadMaxLevels];          // conv output of level l: (bs, na*no, ny, nx), contiguous
  int ny[kHeadMaxLevels], nx[kHeadMaxLevels];
  long long a_off[kHeadMaxLevels];         // first row of level l in z (the rows of the levels before)
  int tile_end[kHeadMaxLevels];            // running sum of the levels' tile counts
  float stride[kHeadMaxLevels];
  float anchor_px[kHeadMaxLevels][OBB_LOSS_MAX_ANCHORS][2];   // anchors * stride (anchor_grid, models/yolo.py:90-91)
  int nl, na;
  int vec;                                 // every plane starts 16-byte aligned and ny*nx is a multiple of 16 bytes: 16-byte loads
};

typedef unsigned int head_u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int head_u32x2 __attribute__((ext_vector_type(2)));

template <typename T>
__device__ __forceinline__ float head_ld(const uint32_t* tile, int c, int p) {          // channel c, position p of the staged tile
  return ld_as_float<T>(reinterpret_cast<const T*>(tile + c * kHeadPitchDw) + p);
}

template <bool TTA> struct HeadFrontOf { typedef HeadFront type; };
template <> struct HeadFrontOf<true> { typedef HeadFrontTta type; };

template <typename T, bool TTA = false>
__global__ __launch_bounds__(kHeadThreads) void k_decode_head(DecodeArgs a, typename HeadFrontOf<TTA>::type h) {
  constexpr int TP = kHeadTile<T>;
  extern __shared__ __attribute__((aligned(16))) uint32_t s_tile[];                    // [no][kHeadPitchDw]
  __shared__ float4 s_c0[kHeadWaves][kHeadStage], s_c1[kHeadWaves][kHeadStage];
  __shared__ unsigned long long s_key[kHeadWaves][kHeadStage];
  __shared__ int s_cnt[kHeadWaves], s_base, s_n;
  __shared__ int s_pos[TP];
  __shared__ float s_obj[TP];

  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  // (kernel-uniform) the state of the later launches, as k_decode does: only the blocks the call's path reads (nms_plan.h:
  // zero_bar / zero_alive -- a block the path does not read comes with a count of 0)
  if (a.z_ticket != nullptr) {
    const long long i = ((long long)blockIdx.y * gridDim.x + blockIdx.x) * kHeadThreads + tid, n = (long long)gridDim.x * gridDim.y * kHeadThreads;
    if (i < a.n_ticket) a.z_ticket[i] = 0;
    for (long long k = i; k < a.n_bar16; k += n) a.z_bar16[k] = make_uint4(0u, 0u, 0u, 0u);
    for (long long k = i; k < a.n_alive16; k += n) a.z_alive16[k] = make_uint4(0u, 0u, 0u, 0u);
  }
  const int bx = (int)blockIdx.x;
  int l = 0;
  while (l + 1 < h.nl && bx >= h.tile_end[l]) l++;
  const int ba = (int)blockIdx.y, b = ba / h.na, an = ba - b * h.na;
  const int nx = h.nx[l], HW = h.ny[l] * nx;
  const int p0 = (bx - (l ? h.tile_end[l - 1] : 0)) * TP;
  const int nt = min(TP, HW - p0);
  const int no = a.no;
  const T* in = (const T*)h.in[l] + (size_t)ba * no * HW + p0;                          // channel c of the tile: in + c*HW
  const float thr = thr_in_dtype<T>(a.conf_thres);
  if (tid == 0) s_n = 0;
  __syncthreads();

  // ---- phase 1: the objectness line                                  :785  xc = prediction[..., 4] > conf_thres
  {
    float obj = 0.f;
    bool p = false;
    if (tid < nt) {
      obj = round_to_dtype<T>(detect_sigmoid<T>(ld_as_float<T>(in + (size_t)4 * HW + tid)));      // z[..., 4] bit for bit
      p = obj > thr;
    }
    const unsigned long long mk = __ballot(p);
    if (mk) {
      int base = 0;
      if (lane == 0) base = atomicAdd(&s_n, __popcll(mk));
      base = __shfl(base, 0);
      if (p) {
        const int i = base + __popcll(mk & lanemask_lt());
        s_pos[i] = tid;
        s_obj[i] = obj;
      }
    }
  }
  __syncthreads();
  const int n_rows = s_n;
  if (n_rows == 0) return;                                       // (workgroup-uniform)

  // ---- phase 2a: the tile's channel lines into LDS (coalesced along p)
  int vec;                                                       // (workgroup-uniform)
  if constexpr (TTA) vec = h.vec[l]; else vec = h.vec;
  if (TTA && vec == 8) {
    if constexpr (TTA) {                                        // 8-byte pieces, 32 per full line: planes on 8-byte boundaries (54x54 fp16)
      constexpr int E = 8 / (int)sizeof(T);
      constexpr int kBatch = 8;
      const int q = tid & 31, c8 = tid >> 5;
      const bool live = q * E < nt;                              // (nt is a multiple of E on this path)
      for (int c0 = c8; c0 < no; c0 += 8 * kBatch) {
        head_u32x2 v[kBatch];
#pragma unroll
        for (int u = 0; u < kBatch; u++) {
          const int c = c0 + u * 8;
          if (c < no && live) v[u] = __builtin_nontemporal_load(reinterpret_cast<const head_u32x2*>(in + (size_t)c * HW) + q);
        }
#pragma unroll
        for (int u = 0; u < kBatch; u++) {
          const int c = c0 + u * 8;
          if (c < no && live) {
            uint32_t* d = s_tile + c * kHeadPitchDw + q * 2;
            d[0] = v[u].x; d[1] = v[u].y;
          }
        }
      }
    }
  } else if (vec) {
    constexpr int E = 16 / (int)sizeof(T);                       // elements per 16-byte piece; 16 pieces per full line
    constexpr int kBatch = 8;
    const int q = tid & 15, c16 = tid >> 4;
    const bool live = q * E < nt;                                // (nt is a multiple of E on this path)
    for (int c0 = c16; c0 < no; c0 += 16 * kBatch) {
      head_u32x4 v[kBatch];
#pragma unroll
      for (int u = 0; u < kBatch; u++) {
        const int c = c0 + u * 16;
        if (c < no && live) v[u] = __builtin_nontemporal_load(reinterpret_cast<const head_u32x4*>(in + (size_t)c * HW) + q);
      }
#pragma unroll
      for (int u = 0; u < kBatch; u++) {
        const int c = c0 + u * 16;
        if (c < no && live) {
          uint32_t* d = s_tile + c * kHeadPitchDw + q * 4;
          d[0] = v[u].x; d[1] = v[u].y; d[2] = v[u].z; d[3] = v[u].w;
        }
      }
    }
  } else {
    const int p = tid % TP;
    for (int c = tid / TP; c < no; c += kHeadThreads / TP)
      if (p < nt) reinterpret_cast<T*>(s_tile + c * kHeadPitchDw)[p] = in[(size_t)c * HW + p];
  }
  __syncthreads();

  // ---- phase 2b: the passing positions in groups of four (one per 16-lane row), as k_decode's reduce_quad
  float4* c0s = s_c0[wv]; float4* c1s = s_c1[wv]; unsigned long long* kys = s_key[wv];
  float4* cand = a.cand + (size_t)b * a.cap_img * 2;
  unsigned long long* keys = a.keys + (size_t)b * a.cap_img;
  uint32_t* vals = a.vals + (size_t)b * a.cap_img;
  int staged = 0;   // wave-uniform
  int flags_seen = 0;
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
  auto flush_wave = [&]() {
    int base = 0;
    if (lane == 0) base = atomicAdd(&a.cnt[b * kCntPad], staged);
    base = __shfl(base, 0);
    write_out(base, staged);
    staged = 0;
  };

  const int l16 = lane & 15, sub = lane >> 4;
  const int ncg = (a.nc + 15) >> 4;
  const float aw = h.anchor_px[l][an][0], ah = h.anchor_px[l][an][1], stride = h.stride[l];
  const long long row0 = h.a_off[l] + (long long)an * HW + p0;                          // row of z of the tile's first position
  for (int g0 = wv; g0 * 4 < n_rows; g0 += kHeadWaves) {
    const int j = g0 * 4 + sub;
    const bool valid = j < n_rows;
    const int p = valid ? s_pos[j] : 0;
    const float obj = valid ? s_obj[j] : 0.f;
    // CSL decode: first arg-max over the 180 rounded bins (:822-823) inside the 16-lane row
    unsigned long long tk = 0ull;
#pragma unroll
    for (int k = 0; k < kDecCslRegs; k++) {
      const int bin = k * 16 + l16;
      const float v = (valid && bin < 180) ? round_to_dtype<T>(detect_sigmoid<T>(head_ld<T>(s_tile, 5 + a.nc + bin, p))) : -__builtin_inff();
      const unsigned long long kk = argmax_key(v, bin);
      tk = (k == 0 || kk > tk) ? kk : tk;
    }
    float tv; int ti;
    argmax_unkey(row_max_u64(tk), tv, ti);
    const float theta = ((float)(ti - 90) / 180.0f) * 3.141592f;
    const int pos = p0 + p, gyi = pos / nx;
    const float gx = (float)(pos - gyi * nx), gy = (float)gyi;
    float box[4];
#pragma unroll
    for (int k = 0; k < 4; k++) box[k] = valid ? detect_decode_one<T>(head_ld<T>(s_tile, k, p), k, gx, gy, stride, aw, ah) : 0.f;
    if constexpr (TTA) {                                         // _descale_pred on the decoded box, as k_detect_decode_tta writes z[..., :4]
      const float inv_scale = h.inv_scale[l], img_w = h.img_w[l], img_h = h.img_h[l];
      const int flip = h.flip[l];
#pragma unroll
      for (int k = 0; k < 4; k++) box[k] = valid ? detect_descale_one<T>(box[k], k, inv_scale, flip, img_w, img_h) : 0.f;
    }
    const float bx_ = box[0], by = box[1], bl = box[2], bs_ = box[3];
    const int bflags = cand_flags(bx_, bl, bs_, a.win_lo, a.win_hi);
    const long long rw = row0 + p;
    auto stage = [&](bool pp, float conf, int c) {         // one candidate per lane with pp set
      const unsigned long long pb = __ballot(pp);
      const int np = __popcll(pb);
      if (np == 0) return;
      if (staged + np > kHeadStage) flush_wave();
      if (pp) {
        const int i = staged + __popcll(pb & lanemask_lt());
        c0s[i] = make_float4(bx_, by, bl, bs_);
        c1s[i] = make_float4(theta, conf, (float)c, 0.f);
        kys[i] = ((unsigned long long)score_desc_key(conf) << 32) | (unsigned long long)(uint32_t)(rw * a.nc + c);
        flags_seen |= bflags;
      }
      staged += np;
    };
    // class confidences (:820 conf = obj * cls in the input dtype)
    unsigned long long bestk = argmax_key(-__builtin_inff(), 0x7fffffff);
    for (int g = 0; g < ncg; g++) {
      const int c = g * 16 + l16;
      const float raw = (valid && c < a.nc) ? round_to_dtype<T>(detect_sigmoid<T>(head_ld<T>(s_tile, 5 + c, p))) : 0.f;
      const float v = (valid && c < a.nc) ? mul_in_dtype<T>(raw, obj) : -__builtin_inff();
      if (a.multi_label) stage(valid && c < a.nc && v > thr && class_allowed(a.cm, c), v, c);             // :827, :835
      else if (c < a.nc) { const unsigned long long kk = argmax_key(v, c); bestk = kk > bestk ? kk : bestk; }   // a NaN wins
    }
    if (!a.multi_label) {
      float bv; int bi;
      argmax_unkey(row_max_u64(bestk), bv, bi);                         // :830 (a NaN maximum fails bv > thr: the row is dropped)
      stage(valid && l16 == 0 && bv > thr && class_allowed(a.cm, bi), bv, bi);                                // :831, :835
    }
  }

  {
    const int fl = (__ballot(flags_seen & kImgSmall) ? kImgSmall : 0) | (__ballot(flags_seen & kImgWide) ? kImgWide : 0);
    if (fl && lane == 0) atomicOr(&a.tiny[b], fl);
  }
  // ---- one atomic per workgroup for whatever is still staged
  if (lane == 0) s_cnt[wv] = staged;
  __syncthreads();
  if (tid == 0) {
    int tot = 0;
    for (int w = 0; w < kHeadWaves; w++) tot += s_cnt[w];
    s_base = tot ? atomicAdd(&a.cnt[b * kCntPad], tot) : 0;
  }
  __syncthreads();
  int base = s_base;
  for (int w = 0; w < wv; w++) base += s_cnt[w];
  write_out(base, staged);
}

// The table of obb_non_max_suppression_obb_head from the caller's level arrays, with the limits of obb_detect_decode_levels and
// obb_non_max_suppression_obb checked on the way; *A_out: the rows of z the levels make up
static int head_front_build(int nl, const void* const* conv_out, int dtype, int64_t bs, int64_t na, int64_t no, const int64_t* ny,
                            const int64_t* nx, const float* anchors_px_host, const float* strides_host, HeadFront* h_out, int64_t* A_out) {
  HeadFront& h = *h_out;
  const int64_t nc = no - 5 - 180;
  if (nl < 1 || nl > kHeadMaxLevels || !conv_out || !ny || !nx || !anchors_px_host || !strides_host || bs < 1 || na < 1 ||
      na > OBB_LOSS_MAX_ANCHORS || nc < 1 || nc > 256 || !dtype_known(dtype) || bs * na > 65535)
    return OBB_ERR_BAD_ARG;
  const size_t esz = dtype_size(dtype);
  const int TP = 256 / (int)esz;                                  // kHeadTile<T> of the dtype's element type
  h.nl = nl; h.na = (int)na; h.vec = 1;
  int64_t A = 0, tiles = 0;
  for (int l = 0; l < kHeadMaxLevels; l++) {
    if (l >= nl) { h.in[l] = nullptr; h.ny[l] = h.nx[l] = 0; h.a_off[l] = A; h.tile_end[l] = (int)tiles; h.stride[l] = 0.f; continue; }
    if (!conv_out[l] || ny[l] < 1 || nx[l] < 1 || ny[l] * nx[l] * na * no > 0x7fffffffLL) return OBB_ERR_BAD_ARG;
    const int64_t HW = ny[l] * nx[l];
    h.in[l] = conv_out[l]; h.ny[l] = (int)ny[l]; h.nx[l] = (int)nx[l]; h.a_off[l] = A; h.stride[l] = strides_host[l];
    for (int a = 0; a < OBB_LOSS_MAX_ANCHORS; a++) {
      h.anchor_px[l][a][0] = a < na ? anchors_px_host[((size_t)l * na + a) * 2] : 0.f;
      h.anchor_px[l][a][1] = a < na ? anchors_px_host[((size_t)l * na + a) * 2 + 1] : 0.f;
    }
    if ((((uintptr_t)conv_out[l]) & 15) != 0 || ((size_t)HW * esz) % 16 != 0) h.vec = 0;
    tiles += (HW + TP - 1) / TP;
    if (tiles > 0x7fffffffLL) return OBB_ERR_BAD_ARG;
    h.tile_end[l] = (int)tiles;
    A += na * HW;
  }
  *A_out = A;
  return OBB_OK;
}

static size_t head_lds_bytes(int64_t no) { return (size_t)no * kHeadPitchDw * 4; }

// the launch run_nms_obb makes in place of k_decode (grid: the levels' tiles x bs*na); dev: current_device() as the call read it
template <bool TTA>
static int launch_decode_head_of(const typename HeadFrontOf<TTA>::type& h, const DecodeArgs& d, int dtype, int dev, hipStream_t st) {
  static OncePerDevice attr;
  if (!raise_lds_once_on(dev, attr, head_lds_bytes(5 + 256 + 180), k_decode_head<float, TTA>, k_decode_head<__half, TTA>, k_decode_head<bf16_t, TTA>))
    return OBB_ERR_LAUNCH;
  const dim3 grid((unsigned)h.tile_end[h.nl - 1], (unsigned)(d.bs * h.na));
  const size_t lds = head_lds_bytes(d.no);
  OBB_DISPATCH_DTYPE(dtype, T, k_decode_head<T, TTA><<<grid, kHeadThreads, lds, st>>>(d, h));
  return OBB_OK;
}
static int launch_decode_head(const HeadFront& h, const DecodeArgs& d, int dtype, int dev, hipStream_t st) { return launch_decode_head_of<false>(h, d, dtype, dev, st); }
// ... over the (pass, level) entries of augmented inference
static int launch_decode_head_tta(const HeadFrontTta& h, const DecodeArgs& d, int dtype, int dev, hipStream_t st) { return launch_decode_head_of<true>(h, d, dtype, dev, st); }

}  // namespace obb
