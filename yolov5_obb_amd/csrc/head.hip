// Detect-head inference decode, CSL label encode and the small box conversions -- gfx950 kernels + C ABI.
//
//   obb_detect_decode   models/yolo.py:61-79 (Detect.forward, inference branch) for one level in ONE pass over the
//                       1x1-conv output: the reference runs view+permute+contiguous (1 read + 1 write of the level),
//                       sigmoid (1+1), two in-place slice updates and a torch.cat (1+1).  Here a workgroup moves a
//                       64-position x no-channel tile through LDS (coalesced 128-256 byte reads along the spatial
//                       axis, one contiguous 64*no-element write per output) and emits both results of the
//                       reference: the permuted raw head x[i] (bs,na,ny,nx,no) and the decoded rows, written straight
//                       into their slice of the concatenated (bs, sum A_i, no) prediction tensor.
//   obb_csl_encode      utils/rboxs_utils.py:9-26 gaussian_label_cpu for a batch of angles on the device.
//   obb_rbox2poly       utils/rboxs_utils.py:106-145 (+ poly2hbb :147-181) for (n,5) long-edge boxes.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>
#include <cmath>
#include <type_traits>
#include "obb_hip.h"
#include "dtype_device.h"
#include "detect_math.h"
#include "confusion_math.h"
#include "geom.h"
#include "valpost_device.h"
#include "ws_layout.h"

namespace obb {

struct DetectArgs {
  const void* in;      // (bs, na*no, ny, nx) conv output
  void* xperm;         // (bs, na, ny, nx, no) or null
  void* z;             // (bs, a_total, no) or null
  void* objcol;        // (bs, a_total) or null: z[..., 4] once more, densely (what the confidence filter of the NMS reads first)
  int bs, na, no, ny, nx;
  long long a_total, a_off;
  float stride;
  float anchor_px[OBB_LOSS_MAX_ANCHORS][2];   // anchors * stride (anchor_grid, models/yolo.py:90-91)
};

// detect_sigmoid / detect_decode_one: detect_math.h (shared with the NMS front kernel of nms_head.h)

// positions per tile (template parameter kTileHW): 128 = 256-byte runs of every channel row (fp16) on the read side when
// the tile fits LDS comfortably, 64 otherwise

template <typename T> struct Pack16;                                   // 16 bytes of T
template <> struct Pack16<float> { static constexpr int V = 4; };
template <> struct Pack16<__half> { static constexpr int V = 8; };
template <> struct Pack16<bf16_t> { static constexpr int V = 8; };

// VEC: the input rows are 4-element aligned (HW % 4 == 0) and both outputs are 16-byte aligned at every tile start,
// so the tile is read with 8/16-byte loads and written with 16-byte stores; otherwise element-wise accesses.
typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2_t __attribute__((ext_vector_type(2)));

// what augmented inference does to the box channels of one pass after the decode (detect_descale_one, detect_math.h)
struct DetectDescale {
  float inv_scale;     // (float)(1.0 / scale), the division in double
  int flip;            // 0 none, 2 up-down, 3 left-right (the dims torch.flip takes)
  float img_w, img_h;  // size of the un-scaled input
};

// NTS: the tile is read and both outputs are written with non-temporal accesses (every byte is touched once)
// TTA: channels 0..3 go through detect_descale_one with *ds after the decode (the other instantiations do not look at ds)
template <typename T, bool VEC, int kTileHW, int NT, int SK, bool NTS, bool NTL, bool TTA = false>
__device__ __forceinline__ void detect_decode_tile(const DetectArgs& d, const int tile_x, const int ba /* b * na + a */,
                                                   const DetectDescale* ds = nullptr) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  T* tile = reinterpret_cast<T*>(smem_raw);            // [no] rows of 64 positions, skewed (tix)
  const int tid = threadIdx.x;
  const int HW = d.ny * d.nx;
  const int a = ba % d.na, b = ba / d.na;
  const int hw0 = tile_x * kTileHW;
  const int nhw = min(kTileHW, HW - hw0);
  const int no = d.no;
  const T* in = (const T*)d.in + ((size_t)ba * no) * HW + hw0;
  // LDS layout: channel row c starts at c*64 + 2*(c>>3) elements.  The store phase reads 8 consecutive channels of one
  // position per lane, i.e. lane stride = 8 rows = 512 + 2 elements: one 32-bit bank further per lane (fp16; two for fp32)
  // instead of the same eight banks again (8-way conflict with a plain 64 / 65 pitch).
  auto tix = [](int c, int hw) -> int { return c * kTileHW + (c >> 3) * SK + hw; };   // SK = 2: one bank per lane in the store phase; 4: two banks, and 4-position groups stay 8-byte aligned (one LDS store per load)

  // ---- load (coalesced along hw)
  if constexpr (VEC) {
    // kTileHW/4 threads x 4 positions cover the positions of one channel row; 256/(kTileHW/4) channel rows per step
    constexpr int TPR = kTileHW / 4, RPS = NT / TPR;
    const int q = tid % TPR, c16 = tid / TPR;
    const int hw = q * 4;
    if (nhw == kTileHW) {
      // full tile (all but the last of a plane): kLoadBatch channel rows in flight per thread before the first LDS store --
      // the loop over 200 rows otherwise waits for every load (one HBM round trip per row and thread)
      constexpr int kLoadBatch = 8;
      using Vec = typename std::conditional<sizeof(T) == 2, uint2, float4>::type;
      for (int c0 = c16; c0 < no; c0 += RPS * kLoadBatch) {
        Vec v[kLoadBatch];
#pragma unroll
        for (int u = 0; u < kLoadBatch; u++) {
          const int c = c0 + u * RPS;
          if (c < no) {
            if constexpr (NTL) {
              using NV = typename std::conditional<sizeof(T) == 2, u32x2_t, u32x4_t>::type;
              const NV t = __builtin_nontemporal_load(reinterpret_cast<const NV*>(in + (size_t)c * HW + hw));
              v[u] = __builtin_bit_cast(Vec, t);
            } else v[u] = *reinterpret_cast<const Vec*>(in + (size_t)c * HW + hw);
          }
        }
#pragma unroll
        for (int u = 0; u < kLoadBatch; u++) {
          const int c = c0 + u * RPS;
          if (c < no) {
            if constexpr (SK == 4) *reinterpret_cast<Vec*>(&tile[tix(c, hw)]) = v[u];
            else {
              const T* e = reinterpret_cast<const T*>(&v[u]);
#pragma unroll
              for (int j = 0; j < 4; j++) tile[tix(c, hw + j)] = e[j];
            }
          }
        }
      }
    } else
    for (int c = c16; c < no; c += RPS) {
      if (hw + 3 < nhw) {
        T v[4];
        if constexpr (sizeof(T) == 2) *reinterpret_cast<uint2*>(v) = *reinterpret_cast<const uint2*>(in + (size_t)c * HW + hw);
        else *reinterpret_cast<float4*>(v) = *reinterpret_cast<const float4*>(in + (size_t)c * HW + hw);
        if constexpr (SK == 4) {                              // aligned group: one 8- / 16-byte LDS store
          if constexpr (sizeof(T) == 2) *reinterpret_cast<uint2*>(&tile[tix(c, hw)]) = *reinterpret_cast<const uint2*>(v);
          else *reinterpret_cast<float4*>(&tile[tix(c, hw)]) = *reinterpret_cast<const float4*>(v);
        } else {
#pragma unroll
          for (int j = 0; j < 4; j++) tile[tix(c, hw + j)] = v[j];
        }
      } else {
        for (int j = 0; j < 4; j++) if (hw + j < nhw) tile[tix(c, hw + j)] = in[(size_t)c * HW + hw + j];
      }
    }
  } else {
    const int hw = tid % kTileHW, c4 = tid / kTileHW;
    for (int c = c4; c < no; c += NT / kTileHW)
      if (hw < nhw) tile[tix(c, hw)] = in[(size_t)c * HW + hw];
  }
  __syncthreads();

  // ---- store: the tile's nhw*no output elements are contiguous in both outputs
  const int nel = nhw * no;
  if (d.objcol && tid < nhw)   // the objectness of the tile's positions, bit-identical to z[..., 4]
    st_from_float<T>((T*)d.objcol + (size_t)b * d.a_total + d.a_off + (size_t)a * HW + hw0 + tid,
                     round_to_dtype<T>(detect_sigmoid<T>(ld_as_float<T>(&tile[tix(4, tid)]))));
  T* xo = d.xperm ? (T*)d.xperm + ((size_t)ba * HW + hw0) * no : nullptr;
  T* zo = d.z ? (T*)d.z + ((size_t)b * d.a_total + d.a_off + (size_t)a * HW + hw0) * no : nullptr;
  const float aw = d.anchor_px[a][0], ah = d.anchor_px[a][1];
  auto decode_at = [&](T raw, int c, int hw) -> float {
    const float r = ld_as_float<T>(&raw);
    if (c >= 4) return round_to_dtype<T>(detect_sigmoid<T>(r));      // 196 of the 200 channels: no grid arithmetic
    const int pos = hw0 + hw;
    const int gyi = pos / d.nx;
    const float v = detect_decode_one<T>(r, c, (float)(pos - gyi * d.nx), (float)gyi, d.stride, aw, ah);
    if constexpr (TTA) return detect_descale_one<T>(v, c, ds->inv_scale, ds->flip, ds->img_w, ds->img_h);
    else return v;
  };
  if constexpr (VEC) {
    constexpr int V = Pack16<T>::V;
    const int nvec = nel / V;                           // full 16-byte groups; the tail (< V elements) goes element-wise
    for (int g = tid; g < nvec; g += NT) {
      const int e0 = g * V;
      int hw = e0 / no, c = e0 - hw * no;
      alignas(16) T rawv[V];
      alignas(16) T decv[V];
#pragma unroll
      for (int j = 0; j < V; j++) {
        const T raw = tile[tix(c, hw)];
        rawv[j] = raw;
        if (zo) { T o; st_from_float<T>(&o, decode_at(raw, c, hw)); decv[j] = o; }
        if (++c == no) { c = 0; hw++; }
      }
      if constexpr (NTS) {
        if (xo) __builtin_nontemporal_store(*reinterpret_cast<const u32x4_t*>(rawv), reinterpret_cast<u32x4_t*>(xo + e0));
        if (zo) __builtin_nontemporal_store(*reinterpret_cast<const u32x4_t*>(decv), reinterpret_cast<u32x4_t*>(zo + e0));
      } else {
        if (xo) *reinterpret_cast<uint4*>(xo + e0) = *reinterpret_cast<const uint4*>(rawv);
        if (zo) *reinterpret_cast<uint4*>(zo + e0) = *reinterpret_cast<const uint4*>(decv);
      }
    }
    for (int e = nvec * V + tid; e < nel; e += NT) {
      const int hw = e / no, c = e - hw * no;
      const T raw = tile[tix(c, hw)];
      if (xo) xo[e] = raw;
      if (zo) st_from_float<T>(zo + e, decode_at(raw, c, hw));
    }
  } else {
    int c = tid % no, hw = tid / no;
    const int dc = NT % no, dh = NT / no;
    for (int e = tid; e < nel; e += NT) {
      const T raw = tile[tix(c, hw)];
      if (xo) xo[e] = raw;
      if (zo) st_from_float<T>(zo + e, decode_at(raw, c, hw));
      c += dc; hw += dh;
      if (c >= no) { c -= no; hw++; }
    }
  }
}

template <typename T, bool VEC, int kTileHW, int NT, int SK, bool NTS = false, bool NTL = NTS>
__global__ __launch_bounds__(NT) void k_detect_decode(DetectArgs d) {
  detect_decode_tile<T, VEC, kTileHW, NT, SK, NTS, NTL>(d, (int)blockIdx.x, (int)blockIdx.y);
}

// All levels of the head in ONE launch: blockIdx.x runs over the tiles of level 0, then level 1, ...; blockIdx.y = b * na + a.
// Three back-to-back launches leave the chip draining and refilling twice (the 32 x 32 level alone is a 20 us launch for
// 5 % of the bytes); in one grid the small levels' tiles fill the gaps of the large one.
constexpr int kDetectMaxLevels = 4;                      // P3 .. P6
struct DetectLevels {
  DetectArgs lv[kDetectMaxLevels];
  int tile_end[kDetectMaxLevels];                        // running sum of the levels' tile counts
  int nl;
};
template <typename T, bool VEC, int kTileHW, int NT, int SK, bool NTS>
__global__ __launch_bounds__(NT) void k_detect_decode_levels(DetectLevels m) {
  const int bx = (int)blockIdx.x;
  int l = 0;
  while (l + 1 < m.nl && bx >= m.tile_end[l]) l++;
  detect_decode_tile<T, VEC, kTileHW, NT, SK, NTS, NTS>(m.lv[l], bx - (l ? m.tile_end[l - 1] : 0), (int)blockIdx.y);
}

// Augmented inference (models/yolo.py:149-161 _forward_augment): the surviving levels of every pass in ONE launch, each an entry of
// the table with the row offset its rows have in torch.cat(_clip_augmented(y), 1) and its pass's de-scale / de-flip.  blockIdx.x
// runs over the tiles of entry 0, then entry 1, ...; blockIdx.y = b * na + a.  The vector path is chosen per entry (the conditions
// of obb_detect_decode_levels, with the entry's own a_off): one odd level does not take it from the others.  Workgroup-uniform.
constexpr int kTtaMaxEntries = OBB_TTA_MAX_PASSES * kDetectMaxLevels;
struct TtaEntry {
  DetectArgs d;
  DetectDescale ds;
  int vec;
};
struct TtaTable {
  TtaEntry e[kTtaMaxEntries];
  int tile_end[kTtaMaxEntries];                          // running sum of the entries' tile counts
  int n;
};
template <typename T, int kTileHW, int NT, int SK>
__global__ __launch_bounds__(NT) void k_detect_decode_tta(TtaTable m) {
  const int bx = (int)blockIdx.x;
  int l = 0;
  while (l + 1 < m.n && bx >= m.tile_end[l]) l++;
  const TtaEntry& e = m.e[l];
  const int tx = bx - (l ? m.tile_end[l - 1] : 0);
  if (e.vec) detect_decode_tile<T, true, kTileHW, NT, SK, true, true, true>(e.d, tx, (int)blockIdx.y, &e.ds);
  else detect_decode_tile<T, false, kTileHW, NT, SK, false, false, true>(e.d, tx, (int)blockIdx.y, &e.ds);
}

// ------------------------------------------------------------------ CSL encode (utils/rboxs_utils.py:9-26)
// out[i][k] = y_sig[(k + index_i) mod n],  y_sig[j] = exp(-((j - n/2) - u)^2 / (2 sig^2)),  index_i = int(n/2 - label_i)
// (python slice semantics: |index| > n leaves the window unrolled).  Evaluated in double like numpy, stored as float.
__global__ void k_csl_encode(const float* __restrict__ labels, long long n, int num_class, double u, double sig,
                             float* __restrict__ out) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n * num_class) return;
  const long long i = e / num_class;
  const int k = (int)(e - i * num_class);
  const double half = (double)num_class / 2.0;
  const double v = half - (double)labels[i];
  long long index = (long long)v;                       // int() truncates toward zero
  long long shift = 0;
  if (index <= num_class && index >= -(long long)num_class) { shift = index % num_class; if (shift < 0) shift += num_class; }
  const int j = (int)((k + shift) % num_class);
  const double x = (double)j - half;
  out[e] = (float)exp(-((x - u) * (x - u)) / (2.0 * sig * sig));
}

// ------------------------------------------------------------------ rbox2poly / poly2hbb (utils/rboxs_utils.py:106-181)
__global__ void k_rbox2poly(const float* __restrict__ rb, long long n, int stride_in, float* __restrict__ poly8,
                            float* __restrict__ hbb4) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float* r = rb + i * stride_in;
  const float x = r[0], y = r[1], w = r[2], h = r[3], th = r[4];
  const float Cos = cosf(th), Sin = sinf(th);
  const float v1x = w / 2 * Cos, v1y = -w / 2 * Sin;      // vector1 :127
  const float v2x = -h / 2 * Sin, v2y = -h / 2 * Cos;     // vector2 :129
  float p[8];
  p[0] = x + v1x + v2x; p[1] = y + v1y + v2y;             // :131-134
  p[2] = x + v1x - v2x; p[3] = y + v1y - v2y;
  p[4] = x - v1x - v2x; p[5] = y - v1y - v2y;
  p[6] = x - v1x + v2x; p[7] = y - v1y + v2y;
  if (poly8) {
#pragma unroll
    for (int k = 0; k < 8; k++) poly8[i * 8 + k] = p[k];
  }
  if (hbb4) {                                              // :166-171
    const float xmax = fmaxf(fmaxf(p[0], p[2]), fmaxf(p[4], p[6])), xmin = fminf(fminf(p[0], p[2]), fminf(p[4], p[6]));
    const float ymax = fmaxf(fmaxf(p[1], p[3]), fmaxf(p[5], p[7])), ymin = fminf(fminf(p[1], p[3]), fminf(p[5], p[7]));
    hbb4[i * 4 + 0] = (xmax + xmin) / 2.0f; hbb4[i * 4 + 1] = (ymax + ymin) / 2.0f;
    hbb4[i * 4 + 2] = xmax - xmin; hbb4[i * 4 + 3] = ymax - ymin;
  }
}

}  // namespace obb

using namespace obb;

extern "C" {

int obb_detect_decode(const void* conv_out, int dtype, int64_t bs, int64_t na, int64_t no, int64_t ny, int64_t nx,
                      const float* anchors_px_host, float stride, void* x_perm_out, void* z_out, int64_t a_total,
                      int64_t a_offset, void* stream) {
  return obb_detect_decode_col(conv_out, dtype, bs, na, no, ny, nx, anchors_px_host, stride, x_perm_out, z_out, a_total, a_offset,
                               nullptr, stream);
}

int obb_detect_decode_col(const void* conv_out, int dtype, int64_t bs, int64_t na, int64_t no, int64_t ny, int64_t nx,
                          const float* anchors_px_host, float stride, void* x_perm_out, void* z_out, int64_t a_total,
                          int64_t a_offset, void* objcol_out, void* stream) {
  if (!conv_out || bs < 1 || na < 1 || na > OBB_LOSS_MAX_ANCHORS || no < 6 || no > 5 + 256 + 180 || ny < 1 || nx < 1 ||
      !dtype_known(dtype) || !anchors_px_host)
    return OBB_ERR_BAD_ARG;
  if (!x_perm_out && !z_out && !objcol_out) return OBB_OK;
  if ((z_out || objcol_out) && (a_offset < 0 || a_offset + na * ny * nx > a_total)) return OBB_ERR_BAD_ARG;
  if (bs * na > 65535 || ny * nx > 0x7fffffffLL) return OBB_ERR_BAD_ARG;
  DetectArgs d;
  d.in = conv_out; d.xperm = x_perm_out; d.z = z_out; d.objcol = objcol_out;
  d.bs = (int)bs; d.na = (int)na; d.no = (int)no; d.ny = (int)ny; d.nx = (int)nx;
  d.a_total = a_total; d.a_off = a_offset; d.stride = stride;
  for (int a = 0; a < OBB_LOSS_MAX_ANCHORS; a++) {
    d.anchor_px[a][0] = a < na ? anchors_px_host[a * 2] : 0.f;
    d.anchor_px[a][1] = a < na ? anchors_px_host[a * 2 + 1] : 0.f;
  }
  const int HW = (int)(ny * nx);
  const size_t esz = dtype_size(dtype);
  // 64-position tiles, 256 threads, 2-element skew, eight channel rows in flight per thread, non-temporal loads and stores
  // (every byte is touched once; a streaming store does not push the lines other workgroups are about to read out of L2).
  // Measured against it in round 3 on (16, 3*200, 128..32, ..) and removed: a 4-element skew with one LDS store per 4-position
  // group (fp32 0.80 against 0.48 ms: the 16-byte LDS stores conflict), 128-position tiles with 512 threads (fp16 0.277
  // against 0.266, fp32 0.95), non-temporal stores only (0.268-0.280) / loads only (0.281).
  const int tile_hw = 64;
  const int skew = 2;
  const size_t lds = ((size_t)no * tile_hw + (size_t)skew * (size_t)(no / 8 + 2)) * esz;   // skewed rows (tix in the kernel)
  dim3 grid((unsigned)((HW + tile_hw - 1) / tile_hw), (unsigned)(bs * na));
  hipStream_t st = (hipStream_t)stream;
  // vector path: input rows 4-element aligned, every tile of both outputs 16-byte aligned
  auto al16 = [](const void* p) { return p == nullptr || (((uintptr_t)p) & 15) == 0; };
  bool vec = (HW % 4 == 0) && al16(conv_out) && al16(x_perm_out) && al16(z_out);
  vec = vec && ((size_t)HW * no * esz) % 16 == 0 && ((size_t)a_total * no * esz) % 16 == 0 && ((size_t)a_offset * no * esz) % 16 == 0;
  if (lds > 150 * 1024) return OBB_ERR_BAD_ARG;
#define OBB_LAUNCH_DETECT(T, VEC, TILE, NTH, SKW, ...)                                                                             \
  do {                                                                                                                              \
    if (lds > 48 * 1024 &&                                                                                                          \
        hipFuncSetAttribute((const void*)k_detect_decode<T, VEC, TILE, NTH, SKW, ##__VA_ARGS__>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) \
      return OBB_ERR_LAUNCH;                                                                                                        \
    k_detect_decode<T, VEC, TILE, NTH, SKW, ##__VA_ARGS__><<<grid, NTH, lds, st>>>(d);                                              \
  } while (0)
#define OBB_LAUNCH_DETECT_T(T)                                                                                                      \
  do {                                                                                                                              \
    if (vec) { OBB_LAUNCH_DETECT(T, true, 64, 256, 2, true); } else { OBB_LAUNCH_DETECT(T, false, 64, 256, 2); }                    \
  } while (0)
  OBB_DISPATCH_DTYPE(dtype, T, OBB_LAUNCH_DETECT_T(T));
#undef OBB_LAUNCH_DETECT_T
#undef OBB_LAUNCH_DETECT
  return hipGetLastError() == hipSuccess ? OBB_OK : OBB_ERR_LAUNCH;
}

int obb_detect_decode_levels(int nl, const void* const* conv_out, int dtype, int64_t bs, int64_t na, int64_t no, const int64_t* ny,
                             const int64_t* nx, const float* anchors_px_host, const float* strides_host, void* const* x_perm_out,
                             void* z_out, int64_t a_total, void* objcol_out, void* stream) {
  if (nl < 1 || nl > kDetectMaxLevels || !conv_out || !ny || !nx || !anchors_px_host || !strides_host || bs < 1 || na < 1 ||
      na > OBB_LOSS_MAX_ANCHORS || no < 6 || no > 5 + 256 + 180 || !dtype_known(dtype))
    return OBB_ERR_BAD_ARG;
  if (bs * na > 65535) return OBB_ERR_BAD_ARG;
  const size_t esz = dtype_size(dtype);
  constexpr int tile_hw = 64, skew = 2;
  auto al16 = [](const void* p) { return p == nullptr || (((uintptr_t)p) & 15) == 0; };
  DetectLevels m;
  m.nl = nl;
  int64_t off = 0, tiles = 0;
  bool vec = al16(z_out) && ((size_t)a_total * no * esz) % 16 == 0;
  bool any_out = z_out != nullptr || objcol_out != nullptr;
  for (int l = 0; l < kDetectMaxLevels; l++) {
    DetectArgs& d = m.lv[l];
    if (l >= nl) { d = m.lv[0]; m.tile_end[l] = (int)tiles; continue; }
    if (!conv_out[l] || ny[l] < 1 || nx[l] < 1 || ny[l] * nx[l] > 0x7fffffffLL) return OBB_ERR_BAD_ARG;
    void* xp = x_perm_out ? x_perm_out[l] : nullptr;
    any_out = any_out || xp != nullptr;
    d.in = conv_out[l]; d.xperm = xp; d.z = z_out; d.objcol = objcol_out;
    d.bs = (int)bs; d.na = (int)na; d.no = (int)no; d.ny = (int)ny[l]; d.nx = (int)nx[l];
    d.a_total = a_total; d.a_off = off; d.stride = strides_host[l];
    for (int a = 0; a < OBB_LOSS_MAX_ANCHORS; a++) {
      d.anchor_px[a][0] = a < na ? anchors_px_host[((size_t)l * na + a) * 2] : 0.f;
      d.anchor_px[a][1] = a < na ? anchors_px_host[((size_t)l * na + a) * 2 + 1] : 0.f;
    }
    const int64_t HW = ny[l] * nx[l];
    vec = vec && (HW % 4 == 0) && al16(conv_out[l]) && al16(xp) && ((size_t)HW * no * esz) % 16 == 0 && ((size_t)off * no * esz) % 16 == 0;
    tiles += (HW + tile_hw - 1) / tile_hw;
    if (tiles > 0x7fffffffLL) return OBB_ERR_BAD_ARG;
    m.tile_end[l] = (int)tiles;
    off += na * HW;
  }
  if ((z_out || objcol_out) && off > a_total) return OBB_ERR_BAD_ARG;
  if (!any_out) return OBB_OK;
  const size_t lds = ((size_t)no * tile_hw + (size_t)skew * (size_t)(no / 8 + 2)) * esz;
  if (lds > 150 * 1024) return OBB_ERR_BAD_ARG;
  dim3 grid((unsigned)tiles, (unsigned)(bs * na));
  hipStream_t st = (hipStream_t)stream;
#define OBB_LAUNCH_LEVELS(T, VEC, NTS)                                                                                              \
  do {                                                                                                                              \
    if (lds > 48 * 1024 &&                                                                                                          \
        hipFuncSetAttribute((const void*)k_detect_decode_levels<T, VEC, tile_hw, 256, skew, NTS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) \
      return OBB_ERR_LAUNCH;                                                                                                        \
    k_detect_decode_levels<T, VEC, tile_hw, 256, skew, NTS><<<grid, 256, lds, st>>>(m);                                             \
  } while (0)
  OBB_DISPATCH_DTYPE(dtype, T, if (vec) OBB_LAUNCH_LEVELS(T, true, true); else OBB_LAUNCH_LEVELS(T, false, false));
#undef OBB_LAUNCH_LEVELS
  return hipGetLastError() == hipSuccess ? OBB_OK : OBB_ERR_LAUNCH;
}

int obb_detect_decode_tta(int npass, const obb_tta_pass* passes_host, int dtype, int64_t bs, int64_t na, int64_t no, void* z_out,
                          int64_t a_total, void* objcol_out, void* stream) {
  if (npass < 1 || npass > OBB_TTA_MAX_PASSES || !passes_host || !z_out || bs < 1 || na < 1 || na > OBB_LOSS_MAX_ANCHORS || no < 6 ||
      no > 5 + 256 + 180 || !dtype_known(dtype) || a_total < 1)
    return OBB_ERR_BAD_ARG;
  if (bs * na > 65535) return OBB_ERR_BAD_ARG;
  const size_t esz = dtype_size(dtype);
  constexpr int tile_hw = 64, skew = 2;
  auto al16 = [](const void* p) { return (((uintptr_t)p) & 15) == 0; };
  // rows of image b start at b * a_total: 16-byte aligned for every b (or there is no b > 0)
  const bool vec_all = al16(z_out) && (bs == 1 || ((size_t)a_total * no * esz) % 16 == 0);
  TtaTable m;
  int n = 0;
  int64_t off = 0, tiles = 0;
  for (int p = 0; p < npass; p++) {
    const obb_tta_pass& ps = passes_host[p];
    if (ps.nl < 1 || ps.nl > kDetectMaxLevels || (ps.flip != 0 && ps.flip != 2 && ps.flip != 3) || !(ps.scale > 0.0) ||
        !std::isfinite(ps.scale) || ps.img_h < 1 || ps.img_w < 1)
      return OBB_ERR_BAD_ARG;
    for (int l = 0; l < ps.nl; l++) {
      if (!ps.conv_out[l] || ps.ny[l] < 1 || ps.nx[l] < 1 || ps.ny[l] * ps.nx[l] > 0x7fffffffLL) return OBB_ERR_BAD_ARG;
      TtaEntry& e = m.e[n];
      DetectArgs& d = e.d;
      d.in = ps.conv_out[l]; d.xperm = nullptr; d.z = z_out; d.objcol = objcol_out;
      d.bs = (int)bs; d.na = (int)na; d.no = (int)no; d.ny = (int)ps.ny[l]; d.nx = (int)ps.nx[l];
      d.a_total = a_total; d.a_off = off; d.stride = ps.stride[l];
      for (int a = 0; a < OBB_LOSS_MAX_ANCHORS; a++) {
        d.anchor_px[a][0] = a < na ? ps.anchors_px[l][a][0] : 0.f;
        d.anchor_px[a][1] = a < na ? ps.anchors_px[l][a][1] : 0.f;
      }
      e.ds.inv_scale = (float)(1.0 / ps.scale);           // what torch's `/= python_float` multiplies with (detect_math.h)
      e.ds.flip = ps.flip; e.ds.img_w = (float)ps.img_w; e.ds.img_h = (float)ps.img_h;
      const int64_t HW = ps.ny[l] * ps.nx[l];
      e.vec = vec_all && (HW % 4 == 0) && al16(ps.conv_out[l]) && ((size_t)HW * no * esz) % 16 == 0 && ((size_t)off * no * esz) % 16 == 0;
      tiles += (HW + tile_hw - 1) / tile_hw;
      if (tiles > 0x7fffffffLL) return OBB_ERR_BAD_ARG;
      m.tile_end[n] = (int)tiles;
      off += na * HW;
      if (off > a_total) return OBB_ERR_BAD_ARG;          // more rows listed than z_out has
      n++;
    }
  }
  m.n = n;
  for (int k = n; k < kTtaMaxEntries; k++) { m.e[k] = m.e[0]; m.tile_end[k] = (int)tiles; }
  const size_t lds = ((size_t)no * tile_hw + (size_t)skew * (size_t)(no / 8 + 2)) * esz;
  if (lds > 150 * 1024) return OBB_ERR_BAD_ARG;
  dim3 grid((unsigned)tiles, (unsigned)(bs * na));
  hipStream_t st = (hipStream_t)stream;
#define OBB_LAUNCH_TTA(T)                                                                                                           \
  do {                                                                                                                              \
    if (lds > 48 * 1024 &&                                                                                                          \
        hipFuncSetAttribute((const void*)k_detect_decode_tta<T, tile_hw, 256, skew>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) \
      return OBB_ERR_LAUNCH;                                                                                                        \
    k_detect_decode_tta<T, tile_hw, 256, skew><<<grid, 256, lds, st>>>(m);                                                          \
  } while (0)
  OBB_DISPATCH_DTYPE(dtype, T, OBB_LAUNCH_TTA(T));
#undef OBB_LAUNCH_TTA
  return hipGetLastError() == hipSuccess ? OBB_OK : OBB_ERR_LAUNCH;
}

int obb_csl_encode_f32(const float* labels, int64_t n, int num_class, double u, double sig, float* out, void* stream) {
  if (n < 0 || num_class < 1 || !(sig > 0.0)) return OBB_ERR_BAD_ARG;
  if (n == 0) return OBB_OK;
  if (!labels || !out) return OBB_ERR_BAD_ARG;
  const long long tot = (long long)n * num_class;
  k_csl_encode<<<(unsigned)((tot + 255) / 256), 256, 0, (hipStream_t)stream>>>(labels, n, num_class, u, sig, out);
  return hipGetLastError() == hipSuccess ? OBB_OK : OBB_ERR_LAUNCH;
}

int obb_rbox2poly_f32(const float* rboxes, int64_t n, int64_t row_stride, float* poly8, float* hbb4, void* stream) {
  if (n < 0 || row_stride < 5) return OBB_ERR_BAD_ARG;
  if (n == 0) return OBB_OK;
  if (!rboxes || (!poly8 && !hbb4)) return OBB_ERR_BAD_ARG;
  k_rbox2poly<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream>>>(rboxes, n, (int)row_stride, poly8, hbb4);
  return hipGetLastError() == hipSuccess ? OBB_OK : OBB_ERR_LAUNCH;
}

}  // extern "C"

// ====================================================================== post-NMS tail of val.py
namespace obb {

// val.py:226-236 for one image's detections (n,7) [x y l s theta conf cls]:
//   pred_poly  (n,10) = [rbox2poly, conf, cls]                       model-input space
//   pred_hbb   (n,6)  = [xywh2xyxy(poly2hbb(poly)), conf, cls]
//   pred_polyn (n,10) = scale_polys(pred_poly): (x - pad_x) / gain, (y - pad_y) / gain     native image space
//   pred_hbbn  (n,6)  = [xywh2xyxy(poly2hbb(polyn)), conf, cls]
// (utils/rboxs_utils.py:106-181, utils/general.py:590-597 xywh2xyxy, :636-650 scale_polys)
// corners of one rbox and scale_polys: valpost_device.h (vt_rbox2poly, vt_scale_poly); the horizontal box around 8 coordinates
// (poly2hbb + xywh2xyxy):
__device__ __forceinline__ void vt_hbb_xyxy(const float* q, float* o) {
  const float xmax = fmaxf(fmaxf(q[0], q[2]), fmaxf(q[4], q[6])), xmin = fminf(fminf(q[0], q[2]), fminf(q[4], q[6]));
  const float ymax = fmaxf(fmaxf(q[1], q[3]), fmaxf(q[5], q[7])), ymin = fminf(fminf(q[1], q[3]), fminf(q[5], q[7]));
  const float xc = (xmax + xmin) / 2.0f, yc = (ymax + ymin) / 2.0f, bw = xmax - xmin, bh = ymax - ymin;   // poly2hbb
  o[0] = xc - bw / 2; o[1] = yc - bh / 2; o[2] = xc + bw / 2; o[3] = yc + bh / 2;                          // xywh2xyxy
}
// the four outputs of val.py:226-236 for detection row i (any output pointer may be NULL); returns pred_hbbn's box in o4n
__device__ __forceinline__ void vt_post_one(const float* __restrict__ r, long long i, float pad_x, float pad_y, float gain,
                                            float* __restrict__ poly10, float* __restrict__ hbb6, float* __restrict__ polyn10,
                                            float* __restrict__ hbbn6, float* o4n) {
  const float conf = r[5], cls = r[6];
  float p[8], o4[4];
  vt_rbox2poly(r[0], r[1], r[2], r[3], r[4], p);
  if (poly10) { for (int k = 0; k < 8; k++) poly10[i * 10 + k] = p[k]; poly10[i * 10 + 8] = conf; poly10[i * 10 + 9] = cls; }
  if (hbb6) { vt_hbb_xyxy(p, o4); for (int k = 0; k < 4; k++) hbb6[i * 6 + k] = o4[k]; hbb6[i * 6 + 4] = conf; hbb6[i * 6 + 5] = cls; }
  float pn[8];
  vt_scale_poly(p, pad_x, pad_y, gain, pn);
  if (polyn10) { for (int k = 0; k < 8; k++) polyn10[i * 10 + k] = pn[k]; polyn10[i * 10 + 8] = conf; polyn10[i * 10 + 9] = cls; }
  vt_hbb_xyxy(pn, o4n);
  if (hbbn6) { for (int k = 0; k < 4; k++) hbbn6[i * 6 + k] = o4n[k]; hbbn6[i * 6 + 4] = conf; hbbn6[i * 6 + 5] = cls; }
}
__global__ void k_val_post(const float* __restrict__ det7, long long n, float pad_x, float pad_y, float gain,
                           float* __restrict__ poly10, float* __restrict__ hbb6, float* __restrict__ polyn10,
                           float* __restrict__ hbbn6) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float o4n[4];
  vt_post_one(det7 + i * 7, i, pad_x, pad_y, gain, poly10, hbb6, polyn10, hbbn6, o4n);
}

// val.py:69-90 process_batch.  The reference keeps, per detection, its highest-IoU label among those with the same class and
// IoU >= iouv[0]; then, per label, the match with the LOWEST detection index (np.unique after the first de-duplication
// has re-ordered the matches by detection index; the re-sort by IoU is commented out at val.py:86).
__global__ void k_pb_best(const float* __restrict__ det6, int n, const float* __restrict__ lab5, int m, const float* __restrict__ iouv,
                          int* __restrict__ best_label, float* __restrict__ best_iou, int* __restrict__ winner) {
  const int d = blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= n) return;
  const float thr0 = iouv[0];                                            // val.py:81  iou >= iouv[0]
  const float* b2 = det6 + (size_t)d * 6;
  const float area2 = (b2[2] - b2[0]) * (b2[3] - b2[1]);
  int bl = -1; float bi = -1.f;
  for (int l = 0; l < m; l++) {
    const float* b1 = lab5 + (size_t)l * 5 + 1;
    if (lab5[(size_t)l * 5] != b2[5]) continue;
    const float area1 = (b1[2] - b1[0]) * (b1[3] - b1[1]);
    const float iw = fmaxf(fminf(b1[2], b2[2]) - fmaxf(b1[0], b2[0]), 0.f);
    const float ih = fmaxf(fminf(b1[3], b2[3]) - fmaxf(b1[1], b2[1]), 0.f);
    const float inter = iw * ih;
    const float iou = inter / (area1 + area2 - inter);                 // utils/metrics.py:265-268
    if (iou >= thr0 && iou > bi) { bi = iou; bl = l; }
  }
  best_label[d] = bl; best_iou[d] = bi;
  if (bl >= 0) atomicMin(&winner[bl], d);
}
__global__ void k_pb_correct(const int* __restrict__ best_label, const float* __restrict__ best_iou, const int* __restrict__ winner,
                             const float* __restrict__ iouv, int n, int niou, uint8_t* __restrict__ correct) {
  const int d = blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= n) return;
  const int bl = best_label[d];
  const bool win = bl >= 0 && winner[bl] == d;
  for (int k = 0; k < niou; k++) correct[(size_t)d * niou + k] = (win && best_iou[d] >= iouv[k]) ? 1 : 0;
}


// ---- the tail for ALL images of a batch (val.py:209-250): two launches (round 4: three) and one device -> host copy per batch instead of
// two launches + a memset + three copies per image.
constexpr int kValTailMaxBs = 64;
struct ValTailImgs {                       // by value in the kernel arguments (bs <= kValTailMaxBs)
  int det_off[kValTailMaxBs + 1];          // detections of image b: rows [det_off[b], det_off[b + 1]) of the packed list (and of every output)
  int det_row[kValTailMaxBs];              // row of det7 that holds the FIRST detection of image b (packed input: det_off[b])
  float pad_x[kValTailMaxBs], pad_y[kValTailMaxBs], gain[kValTailMaxBs], shape_w[kValTailMaxBs], shape_h[kValTailMaxBs];
  int bs;
};
// a label's box (val.py:238-241, in the reference's operation order): rbox2poly -> poly2hbb -> xywh2xyxy in the letterboxed frame,
// THEN scale_coords: subtract the pad, divide by the gain, clip to the native shape (utils/general.py:621-633) -> [x1 y1 x2 y2]
__device__ __forceinline__ void vt_label_box(const float* t, const ValTailImgs& im, int b, float* o) {
  float p[8];
  vt_rbox2poly(t[2], t[3], t[4], t[5], t[6], p);                // t = [img cls cx cy l s theta ...]
  vt_hbb_xyxy(p, o);
  o[0] -= im.pad_x[b]; o[2] -= im.pad_x[b]; o[1] -= im.pad_y[b]; o[3] -= im.pad_y[b];
#pragma unroll
  for (int k = 0; k < 4; k++) o[k] /= im.gain[b];
  o[0] = fminf(fmaxf(o[0], 0.f), im.shape_w[b]); o[2] = fminf(fmaxf(o[2], 0.f), im.shape_w[b]);
  o[1] = fminf(fmaxf(o[1], 0.f), im.shape_h[b]); o[3] = fminf(fmaxf(o[3], 0.f), im.shape_h[b]);
}
// Round 5: two launches (round 4: three -- a label kernel in front, and an atomicMin "winner" table that needed it for its
// initialisation).  The label boxes are computed where they are used (a detection meets one or two labels of its image and class),
// and the winner of a label -- the lowest-indexed detection of the image whose best label it is (process_batch's first np.unique
// pass, val.py:84-86) -- is found by the stats kernel with a scan over the earlier detections of the image.
// per detection: the four outputs of val.py:226-236 and its best label (process_batch, see k_pb_best) among the labels of ITS image.
// The label boxes of the one or two images a workgroup's 128 detections belong to are computed once into LDS (a detection
// computing the box of every label it meets -- double-precision sin / cos on divergent lanes -- made the kernel slower than the
// launch it saved); more than kVtLabLds labels in range: computed where they are met.
constexpr int kVtLabLds = 512;
__global__ void k_vt_dets(const float* __restrict__ det7, int n, ValTailImgs im, const float* __restrict__ targets, int nt, int tcols,
                          const float* __restrict__ iouv, float* __restrict__ poly10, float* __restrict__ hbb6, float* __restrict__ polyn10,
                          float* __restrict__ hbbn6, int* __restrict__ best_label, float* __restrict__ best_iou, int* __restrict__ counter) {
  __shared__ float s_lab[kVtLabLds][4];
  __shared__ float s_lc[kVtLabLds];
  __shared__ int s_li[kVtLabLds], s_lb[kVtLabLds];
  __shared__ int s_nl;
  if (blockIdx.x == 0 && threadIdx.x == 0) *counter = 0;       // k_vt_stats' arrival counter (that kernel runs behind this one)
  const int d = blockIdx.x * blockDim.x + threadIdx.x;
  const int d_first = blockIdx.x * blockDim.x, d_last = (d_first + (int)blockDim.x < n ? d_first + (int)blockDim.x : n) - 1;
  int b_lo = 0, b_hi = 0;
  while (b_lo + 1 < im.bs && d_first >= im.det_off[b_lo + 1]) b_lo++;   // (bs <= 64: short scans of kernel-argument registers)
  b_hi = b_lo;
  while (b_hi + 1 < im.bs && d_last >= im.det_off[b_hi + 1]) b_hi++;
  if (threadIdx.x == 0) s_nl = 0;
  __syncthreads();
  for (int l = threadIdx.x; l < nt; l += blockDim.x) {
    const float* t = targets + (size_t)l * tcols;
    const int lb = (int)t[0];
    if (lb >= b_lo && lb <= b_hi) {
      const int k = atomicAdd(&s_nl, 1);
      if (k < kVtLabLds) { s_li[k] = l; s_lb[k] = lb; s_lc[k] = t[1]; vt_label_box(t, im, lb, s_lab[k]); }
    }
  }
  __syncthreads();
  const int nl = s_nl;
  if (d >= n) return;
  int b = b_lo;
  while (b + 1 < im.bs && d >= im.det_off[b + 1]) b++;
  float b2[4];
  const float* row = det7 + ((size_t)im.det_row[b] + (d - im.det_off[b])) * 7;
  vt_post_one(row, d, im.pad_x[b], im.pad_y[b], im.gain[b], poly10, hbb6, polyn10, hbbn6, b2);
  const float cls = row[6];
  const float thr0 = iouv[0];                                            // val.py:81  iou >= iouv[0]
  const float area2 = (b2[2] - b2[0]) * (b2[3] - b2[1]);
  int bl = -1; float bi = -1.f;
  auto consider = [&](const float* b1, int l) {
    const float area1 = (b1[2] - b1[0]) * (b1[3] - b1[1]);
    const float iw = fmaxf(fminf(b1[2], b2[2]) - fmaxf(b1[0], b2[0]), 0.f);
    const float ih = fmaxf(fminf(b1[3], b2[3]) - fmaxf(b1[1], b2[1]), 0.f);
    const float inter = iw * ih;
    const float iou = inter / (area1 + area2 - inter);                 // utils/metrics.py:265-268
    // the best label = the first maximum in label order (the staged list is in arrival order: the tie goes to the lower index)
    if (iou >= thr0 && (iou > bi || (iou == bi && l < bl))) { bi = iou; bl = l; }
  };
  if (nl <= kVtLabLds) {
    for (int k = 0; k < nl; k++)
      if (s_lb[k] == b && s_lc[k] == cls) consider(s_lab[k], s_li[k]);
  } else {
    for (int l = 0; l < nt; l++) {
      const float* t = targets + (size_t)l * tcols;
      if ((int)t[0] != b || t[1] != cls) continue;
      float b1[4];
      vt_label_box(t, im, b, b1);
      consider(b1, l);
    }
  }
  best_label[d] = bl; best_iou[d] = bi;
}
// stats row of detection d: correct[0 .. niou) as 0 / 1, then conf, then cls (val.py:250's tuple, one copy for the batch)
// `done` (optional, pinned host memory like `stats` may be): receives n once EVERY row has landed -- each workgroup makes its
// rows visible system-wide (fence), then arrives on a device counter; the last one stores the flag.  The host polls it instead of
// copying the rows back and waiting for the stream.
// TOut = float: the rows above.  TOut = uint8_t (process_batch_obb's one-image form): correct[0 .. niou) alone, as bytes.
template <typename TOut = float>
__global__ void k_vt_stats(const float* __restrict__ det7, const int* __restrict__ best_label, const float* __restrict__ best_iou,
                           ValTailImgs im, const float* __restrict__ iouv, int n, int niou, TOut* __restrict__ stats,
                           int* __restrict__ counter, long long* __restrict__ done) {
  const int d = blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & 63;
  // the winner of a label = the lowest-indexed detection of the image that chose it (detection indices grow inside the image).  A
  // matched detection looks for an earlier one with the same label; the wave scans that prefix TOGETHER, 64 entries per trip (a
  // lane on its own walked up to a few hundred dependent loads: the first version of this kernel took longer than the launch it saved)
  int bl = -1, off_b = 0, row_b = 0;
  if (d < n) {
    bl = best_label[d];
    int b = 0;
    while (b + 1 < im.bs && d >= im.det_off[b + 1]) b++;
    off_b = im.det_off[b]; row_b = im.det_row[b];
  }
  bool win = bl >= 0;
  for (unsigned long long todo = __ballot(win); todo; todo &= todo - 1) {
    const int l0 = __builtin_ctzll(todo);
    const int bl0 = __shfl(bl, l0), d0 = __shfl(d, l0), o0 = __shfl(off_b, l0);
    bool found = false;
    for (int e0 = o0; e0 < d0 && !found; e0 += 64) {
      const int e = e0 + lane;
      found = __ballot(e < d0 && best_label[e] == bl0) != 0ull;
    }
    if (found && lane == l0) win = false;
  }
  if constexpr (std::is_same<TOut, float>::value) {
  if (d < n) {
    float* o = stats + (size_t)d * (niou + 2);
    for (int k = 0; k < niou; k++) o[k] = (win && best_iou[d] >= iouv[k]) ? 1.f : 0.f;
    const float* row = det7 + ((size_t)row_b + (d - off_b)) * 7;
    o[niou] = row[5]; o[niou + 1] = row[6];
  }
  } else {
    if (d < n)
      for (int k = 0; k < niou; k++) stats[(size_t)d * niou + k] = (win && best_iou[d] >= iouv[k]) ? 1 : 0;
  }
  if (done != nullptr) {                                          // (kernel-uniform)
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0 && atomicAdd(counter, 1) == (int)gridDim.x - 1)
      __hip_atomic_store(done, (long long)n, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// ---- process_batch with the ROTATED IoU (the oriented-box mAP): val.py:69-90 with box_iou replaced by
// single_box_iou_rotated<float>(label [cx cy l s theta], detection [cx cy l s theta]) in the letterboxed frame of the rows -- the
// value obb_rotated_iou_pairs_f32(a5 = label, b5 = detection) returns, bit for bit (riou_device.h).  Every other rule is
// k_vt_dets': class equality as a float compare, iou >= iouv[0] non-strict (a NaN IoU is no candidate), a detection keeps its
// candidate of highest IoU, ties to the lower label index; the label's winner and the rows are k_vt_stats' on the two arrays below.
//   * one lane per detection; the labels of the one or two images a workgroup's detections belong to are staged in LDS as packed
//     RotGeom records -- rbox_make_feat's double sin / cos once per label per workgroup -- with the class, the label's row and
//     its image in the free slots of quad 3.  One tile when they fit kVtLabLds records (staged optimistically); else tiles over
//     consecutive runs of kVtLabLds label rows, the queue drained before a tile is replaced.
//   * a lane walks the tile (broadcast reads) and drops a pair of its image and class only on a PROOF that iou < iouv[0]:
//     RotGeom::cheap_reject / rbox_certainly_disjoint prove "the reference returns exactly 0", the area-ratio bound and
//     rbox_quick_bounds prove an upper bound -- all of them only while iouv[0] > 0 (`cull`); with iouv[0] <= 0 (or NaN) an IoU
//     of 0 is itself a candidate and every pair of the class is clipped.
//   * survivors go into the wave's LDS queue as (lane << 16 | tile slot); whenever it holds 64 entries, and at the end of a tile,
//     one pair per lane runs the exact clip on the lane's scratch column -- the ~10^3-flop clip never runs for a handful of lanes.
//     The detection's features come from their owner's registers (12 __shfl), the label's from the tile.
//   * the result returns to its detection through a 64-bit LDS atomic max on (ordered IoU bits << 32 | ~label row): k_confusion's
//     winner-slot idiom (cm::winner_key); the complement sends equal IoUs to the lower label row.
// LDS: the tile 512 x 64 B = 32 KiB, clip scratch 2 waves x 12 KiB, 128 slots x 8 B, 2 queues x 128 x 4 B: 58.0 KiB + 4 B --
// two workgroups in a CU's 160 KiB.  kBatch = false: one image, labels (m, 6) [cls cx cy l s theta] (im.bs = 1).
constexpr int kVoThreads = 128, kVoWaves = kVoThreads / 64, kVoQueue = 128;
// true only when the IoU the reference computes for (A, B) is PROVED to lie below thr (for thr > 0 only)
__device__ __forceinline__ bool vo_proved_below(const RBoxFeat& A, const RBoxFeat& B, float thr) {
  if (rbox_certainly_disjoint(A, B)) return true;                 // exactly 0
  if (rbox_iou_upper_bound(A, B) < thr) return true;              // area ratio (+inf when it does not vouch)
  IouBounds qb;
  return rbox_quick_bounds(A, B, &qb) && qb.hi < thr;
}
template <bool kBatch>
__global__ __launch_bounds__(kVoThreads) void k_vo_match(const float* __restrict__ det7, int n, ValTailImgs im,
                                                         const float* __restrict__ labels, int nt, int lcols,
                                                         const float* __restrict__ iouv, int* __restrict__ match_label,
                                                         float* __restrict__ match_iou) {
  __shared__ float4 s_lab[kVtLabLds * RotGeom::RECQ];
  __shared__ float s_scr[kVoWaves][RotGeom::SCR * 64];
  __shared__ unsigned long long s_best[kVoThreads];
  __shared__ int s_q[kVoWaves][kVoQueue];
  __shared__ int s_nl;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int d = blockIdx.x * kVoThreads + tid;
  const bool valid = d < n;
  const int d_first = blockIdx.x * kVoThreads, d_last = (d_first + kVoThreads < n ? d_first + kVoThreads : n) - 1;
  int b_lo = 0;
  while (b_lo + 1 < im.bs && d_first >= im.det_off[b_lo + 1]) b_lo++;
  int b_hi = b_lo;
  while (b_hi + 1 < im.bs && d_last >= im.det_off[b_hi + 1]) b_hi++;
  // the lane's detection: features in registers (every lane stays to the end: the drain reads them with __shfl)
  int b = b_lo;
  RBoxFeat D = {};
  float4 dq0 = make_float4(0.f, 0.f, 0.f, 0.f);
  float cls = 0.f;
  if (valid) {
    while (b + 1 < im.bs && d >= im.det_off[b + 1]) b++;
    const float* row = det7 + ((size_t)im.det_row[b] + (d - im.det_off[b])) * 7;
    D = rbox_make_feat(row[0], row[1], row[2], row[3], row[4]);
    float4 q[RotGeom::RECQ];
    RotGeom::pack(D, q);
    dq0 = q[0];
    cls = row[6];
  }
  const float thr0 = iouv[0];                                      // val.py:81  iou >= iouv[0]
  const bool cull = thr0 > 0.f;
  s_best[tid] = 0ull;                                              // (no key is 0)
  int* q_w = s_q[wave];
  float* scr = s_scr[wave] + lane;
  int qn = 0;                                                      // entries in the wave's queue (wave-uniform)
  // the exact IoU of the queue's last `cnt` (<= 64) entries, one per lane
  auto drain = [&](int cnt) {
    qn -= cnt;
    __builtin_amdgcn_wave_barrier();
    const bool has = lane < cnt;
    const int ent = has ? q_w[qn + lane] : 0;
    const int ql = ent >> 16, k = ent & 0xffff;
    RBoxFeat B;
    B.x = __shfl(D.x, ql); B.y = __shfl(D.y, ql); B.w = __shfl(D.w, ql); B.h = __shfl(D.h, ql);
    B.sh = __shfl(D.sh, ql); B.cw = __shfl(D.cw, ql); B.ch = __shfl(D.ch, ql); B.sw = __shfl(D.sw, ql);
    B.r = __shfl(D.r, ql); B.c = __shfl(D.c, ql); B.s = __shfl(D.s, ql); B.area = __shfl(D.area, ql);
    if (has) {
      const float4 l3 = s_lab[k * 4 + 3];
      const RBoxFeat A = RotGeom::unpack(s_lab[k * 4], s_lab[k * 4 + 1], s_lab[k * 4 + 2], l3);
      const float iou = rot_iou_value(A, B, scr);                  // (label, detection): the argument order is part of the value
      if (iou >= thr0) atomicMax(&s_best[wave * 64 + ql], cm::winner_key(iou, ~__float_as_int(l3.z)));
    }
    __builtin_amdgcn_wave_barrier();
  };
  // rows [r0, r1) of the labels: the ones of the workgroup's images -> the tile, in arrival order (slots past the tile are dropped)
  auto stage = [&](int r0, int r1) {
    for (int l = r0 + tid; l < r1; l += kVoThreads) {
      const float* t = labels + (size_t)l * lcols;
      const int lb = kBatch ? (int)t[0] : 0;
      if (lb < b_lo || lb > b_hi) continue;
      const int k = atomicAdd(&s_nl, 1);
      if (k >= kVtLabLds) continue;
      const float* r = t + (kBatch ? 1 : 0);                       // [cls cx cy l s theta]
      float4 q[RotGeom::RECQ];
      RotGeom::pack(rbox_make_feat(r[1], r[2], r[3], r[4], r[5]), q);
      q[3].y = r[0]; q[3].z = __int_as_float(l); q[3].w = __int_as_float(lb);
      s_lab[k * 4] = q[0]; s_lab[k * 4 + 1] = q[1]; s_lab[k * 4 + 2] = q[2]; s_lab[k * 4 + 3] = q[3];
    }
  };
  auto walk = [&](int tn) {
    for (int k = 0; k < tn; k++) {
      const float4 l0 = s_lab[k * 4], l3 = s_lab[k * 4 + 3];
      bool push = valid && __float_as_int(l3.w) == b && l3.y == cls;
      if (push && cull) {
        if (RotGeom::cheap_reject(l0, dq0)) push = false;
        else push = !vo_proved_below(RotGeom::unpack(l0, s_lab[k * 4 + 1], s_lab[k * 4 + 2], l3), D, thr0);
      }
      const unsigned long long mask = __ballot(push);
      if (push) q_w[qn + __popcll(mask & ((1ull << lane) - 1ull))] = (lane << 16) | k;
      qn += __popcll(mask);
      if (qn >= 64) drain(64);                                     // (qn < 64 before the push: never more than 127 entries)
    }
    if (qn > 0) drain(qn);
  };
  if (tid == 0) s_nl = 0;
  __syncthreads();
  stage(0, nt);
  __syncthreads();
  const int nl = s_nl;
  if (nl <= kVtLabLds) {
    walk(nl);
  } else {
    for (int r0 = 0; r0 < nt; r0 += kVtLabLds) {                   // (a run of kVtLabLds rows cannot overflow the tile)
      __syncthreads();
      if (tid == 0) s_nl = 0;
      __syncthreads();
      stage(r0, r0 + kVtLabLds < nt ? r0 + kVtLabLds : nt);
      __syncthreads();
      walk(s_nl);
    }
  }
  __builtin_amdgcn_wave_barrier();                                 // (a slot is written by the lanes of its own wave only)
  if (valid) {
    const unsigned long long key = s_best[tid];
    uint32_t u = (uint32_t)(key >> 32);
    u ^= (u >> 31) ? 0x80000000u : 0xffffffffu;                    // cm::winner_key's bit map, inverted
    match_label[d] = key ? (int)~(uint32_t)key : -1;
    match_iou[d] = key ? __uint_as_float(u) : -1.f;
  }
}


// ---- ConfusionMatrix.process_batch (utils/metrics.py:125-163) for every image of a batch in ONE launch: a workgroup is an
// image, workgroups exchange nothing, and the only traffic between them is the final atomic adds into the matrix.  The rules
// (strict compares, the pinned tie order) are csrc/confusion_math.h; the boxes are the bytes of pred_hbbn (vt_post_one) and of
// k_vt_dets' label boxes (vt_label_box).  kBatch = false: one image on boxes already computed (det6 / lab5), the same core.
//   phase 0  the image's labels, in the order of `targets`, boxes computed once -> workspace; its detections -> workspace
//   phase 1  label tiles of kVtLabLds boxes through LDS; every kept detection keeps its best candidate label (rule 1)
//   phase 2  one 64-bit atomic max per matched detection into its label's winner slot (rule 2); block-wide "any match"
//   phase 3  labels: the winner's cell, else the background row          phase 4  detections that won nothing: background column
// Winner slots: LDS when the image has <= kVtLabLds labels, else the workspace.  Cells: an LDS histogram, flushed with one global
// atomic per non-zero cell, when (nc + 1)^2 <= kCmHistLds (nc <= 109); else global atomics directly.  Per-image counts < 2^32.
constexpr int kCmThreads = 1024;
constexpr int kCmHistLds = 110 * 110;      // 48,400 B beside the 14 KiB of label tile and slots: 61.4 KiB, two workgroups in a CU's 160 KiB
struct CmWs {                              // the call's workspace, laid out by cm_layout (labels by position, detections by packed row)
  unsigned long long* win;                 // [nt] winner slot per label
  float* lbox; int* lcls;                  // [nt][4], [nt] class index or -1
  float* dbox; int* dcls;                  // [n][4], [n] class index or -1
  float* biou; int* blab;                  // [n] best candidate label (position in the image's list), -1 none, -2 dropped by conf
};
template <bool kBatch>
__global__ __launch_bounds__(kCmThreads) void k_confusion(const float* __restrict__ dets, ValTailImgs im, int n1,
                                                          const float* __restrict__ labels, int nt, int tcols, int nc, float conf_thres,
                                                          float iou_thres, unsigned long long* __restrict__ matrix, CmWs ws) {
  __shared__ float s_lab[kVtLabLds][4];
  __shared__ int s_lc[kVtLabLds];
  __shared__ unsigned long long s_win[kVtLabLds];
  __shared__ unsigned int s_hist[kCmHistLds];
  __shared__ int s_wave[kCmThreads / 64][2];
  __shared__ int s_any, s_oor;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  constexpr int kWaves = kCmThreads / 64;
  const int b = blockIdx.x;
  const int d0 = kBatch ? im.det_off[b] : 0;                     // first packed row of the image's detections
  const int n = kBatch ? im.det_off[b + 1] - d0 : n1;
  if (n == 0) return;                                            // val.py:217-220: no detections, nothing is counted
  // ---- the image's labels: m of them, stored from position l0 of the label arrays (= the labels of earlier images: disjoint ranges)
  int m = nt, l0 = 0;
  if (kBatch) {
    int eq = 0, less = 0;
    for (int l = tid; l < nt; l += kCmThreads) {
      const int lb = (int)labels[(size_t)l * tcols];
      eq += lb == b; less += lb >= 0 && lb < b;
    }
    for (int o = 32; o; o >>= 1) { eq += __shfl_xor(eq, o); less += __shfl_xor(less, o); }
    if (lane == 0) { s_wave[wave][0] = eq; s_wave[wave][1] = less; }
    __syncthreads();
    m = 0;
    for (int w = 0; w < kWaves; w++) { m += s_wave[w][0]; l0 += s_wave[w][1]; }
    __syncthreads();
  }
  if (m == 0) return;                                            // val.py:238: no labels, nothing is counted
  const bool win_lds = m <= kVtLabLds, hist_lds = (nc + 1) * (nc + 1) <= kCmHistLds;
  const int cells = (nc + 1) * (nc + 1);
  if (tid == 0) { s_any = 0; s_oor = 0; }
  if (win_lds) for (int l = tid; l < m; l += kCmThreads) s_win[l] = 0ull;
  if (hist_lds) for (int c = tid; c < cells; c += kCmThreads) s_hist[c] = 0u;
  // phase 0, labels: ordered compaction of the rows with t[0] == b, kCmThreads rows a trip (the tie rule needs their order)
  for (int base = 0, at = 0; base < nt; base += kCmThreads) {
    const int l = base + tid;
    const float* t = labels + (size_t)l * (kBatch ? tcols : 5);
    const bool mine = l < nt && (!kBatch || (int)t[0] == b);
    const unsigned long long bal = __ballot(mine);
    if (kBatch) {
      if (lane == 0) s_wave[wave][0] = __popcll(bal);
      __syncthreads();
    }
    int pos = at + __popcll(bal & ((1ull << lane) - 1ull)), total = 0;
    if (kBatch) {
      for (int w = 0; w < kWaves; w++) { const int c = s_wave[w][0]; if (w < wave) pos += c; total += c; }
    } else {
      pos = l;
    }
    if (mine) {
      float* o = ws.lbox + (size_t)(l0 + pos) * 4;
      if (kBatch) {
        float bx[4];
        vt_label_box(t, im, b, bx);
        o[0] = bx[0]; o[1] = bx[1]; o[2] = bx[2]; o[3] = bx[3];
      } else {
        o[0] = t[1]; o[1] = t[2]; o[2] = t[3]; o[3] = t[4];
      }
      ws.lcls[l0 + pos] = cm::class_index(t[kBatch ? 1 : 0], nc);
      if (!win_lds) __hip_atomic_store(&ws.win[l0 + pos], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    at += total;
    if (kBatch) __syncthreads();                                 // (s_wave is rewritten by the next trip)
  }
  // phase 0, detections: pred_hbbn's box, the class index and the conf filter
  for (int d = tid; d < n; d += kCmThreads) {
    float bx[4], conf, cls;
    if (kBatch) {
      const float* row = dets + ((size_t)im.det_row[b] + d) * 7;
      vt_post_one(row, 0, im.pad_x[b], im.pad_y[b], im.gain[b], nullptr, nullptr, nullptr, nullptr, bx);
      conf = row[5]; cls = row[6];
    } else {
      const float* row = dets + (size_t)d * 6;
      bx[0] = row[0]; bx[1] = row[1]; bx[2] = row[2]; bx[3] = row[3]; conf = row[4]; cls = row[5];
    }
    float* o = ws.dbox + (size_t)(d0 + d) * 4;
    o[0] = bx[0]; o[1] = bx[1]; o[2] = bx[2]; o[3] = bx[3];
    ws.dcls[d0 + d] = cm::class_index(cls, nc);
    ws.biou[d0 + d] = 0.f;
    ws.blab[d0 + d] = cm::keeps(conf, conf_thres) ? -1 : -2;
  }
  __syncthreads();
  // phase 1: a tile of labels in LDS, every thread's detections against it (a thread meets only its own detections' records)
  for (int t0 = 0; t0 < m; t0 += kVtLabLds) {
    const int tn = m - t0 < kVtLabLds ? m - t0 : kVtLabLds;
    for (int k = tid; k < tn; k += kCmThreads) {
      const float* q = ws.lbox + (size_t)(l0 + t0 + k) * 4;
      s_lab[k][0] = q[0]; s_lab[k][1] = q[1]; s_lab[k][2] = q[2]; s_lab[k][3] = q[3];
      s_lc[k] = ws.lcls[l0 + t0 + k];
    }
    __syncthreads();
    for (int d = tid; d < n; d += kCmThreads) {
      int bl = ws.blab[d0 + d];
      if (bl == -2) continue;
      float bi = ws.biou[d0 + d];
      const float* q = ws.dbox + (size_t)(d0 + d) * 4;
      const float b2[4] = {q[0], q[1], q[2], q[3]};
      for (int k = 0; k < tn; k++) {
        float iou;
        if (cm::candidate(s_lab[k], b2, iou_thres, &iou) && cm::better_label(iou, t0 + k, bi, bl)) { bi = iou; bl = t0 + k; }
      }
      ws.biou[d0 + d] = bi; ws.blab[d0 + d] = bl;
    }
    __syncthreads();
  }
  // phase 2: the winner of every label
  for (int d = tid; d < n; d += kCmThreads) {
    const int bl = ws.blab[d0 + d];
    if (bl < 0) continue;
    const unsigned long long key = cm::winner_key(ws.biou[d0 + d], d);
    if (win_lds) atomicMax(&s_win[bl], key); else atomicMax(&ws.win[l0 + bl], key);
    s_any = 1;
  }
  __syncthreads();
  const bool any = s_any != 0;
  auto winner_of = [&](int l) {
    return win_lds ? s_win[l] : __hip_atomic_load(&ws.win[l0 + l], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  };
  auto count = [&](int row, int col) {                           // matrix[predicted][true] += 1; a class outside [0, nc): the counter
    if (row < 0 || col < 0) { atomicAdd(&s_oor, 1); return; }
    const int c = row * (nc + 1) + col;
    if (hist_lds) atomicAdd(&s_hist[c], 1u); else atomicAdd(&matrix[c], 1ull);
  };
  // phase 3: labels
  for (int l = tid; l < m; l += kCmThreads) {
    const unsigned long long key = winner_of(l);
    const int lc = ws.lcls[l0 + l];
    if (key) count(ws.dcls[d0 + cm::winner_det(key)], lc);       // taken whether or not the classes agree (metrics.py:156)
    else count(nc, lc);                                          // background row (metrics.py:158)
  }
  // phase 4: kept detections that are no label's winner -- only in an image with a match (`if n:`, metrics.py:160)
  if (any) {
    for (int d = tid; d < n; d += kCmThreads) {
      const int bl = ws.blab[d0 + d];
      if (bl == -2) continue;
      if (bl < 0 || cm::winner_det(winner_of(bl)) != d) count(ws.dcls[d0 + d], nc);
    }
  }
  __syncthreads();
  if (hist_lds) {
    for (int c = tid; c < cells; c += kCmThreads) {
      const unsigned int v = s_hist[c];
      if (v) atomicAdd(&matrix[c], (unsigned long long)v);
    }
  }
  if (tid == 0 && s_oor) atomicAdd(&matrix[cells], (unsigned long long)s_oor);
}

// the two launches of the oriented tail: the match arrays, then k_vt_stats on them (TOut = float rows / uint8_t correct)
template <bool kBatch, typename TOut>
static int vo_launch(const float* det7, int64_t n, const ValTailImgs& im, const float* labels, int64_t nt, int64_t lcols,
                     const float* iouv, int niou, TOut* out, int32_t* match_label, float* match_iou, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  k_vo_match<kBatch><<<(unsigned)((n + kVoThreads - 1) / kVoThreads), kVoThreads, 0, st>>>(
      det7, (int)n, im, labels, (int)nt, (int)lcols, iouv, match_label, match_iou);
  k_vt_stats<TOut><<<(unsigned)((n + 255) / 256), 256, 0, st>>>(det7, match_label, match_iou, im, iouv, (int)n, niou, out, nullptr, nullptr);
  return hipGetLastError() == hipSuccess ? OBB_OK : OBB_ERR_LAUNCH;
}

}  // namespace obb

extern "C" {

int obb_val_postprocess_f32(const float* det7, int64_t n, float pad_x, float pad_y, float gain, float* poly10, float* hbb6,
                            float* polyn10, float* hbbn6, void* stream) {
  if (n < 0 || !(gain > 0.f)) return OBB_ERR_BAD_ARG;
  if (n == 0) return OBB_OK;
  if (!det7) return OBB_ERR_BAD_ARG;
  obb::k_val_post<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream>>>(det7, n, pad_x, pad_y, gain, poly10, hbb6, polyn10, hbbn6);
  return hipGetLastError() == hipSuccess ? OBB_OK : OBB_ERR_LAUNCH;
}

// the workspace of the val tail: the match arrays of k_vt_dets and k_vt_stats' arrival counter (nothing in it grows with nt)
struct VtWs { int* best_label; float* best_iou; int* counter; size_t bytes; };
static VtWs vt_layout(void* base, int64_t n) {
  const size_t nn = (size_t)(n > 0 ? n : 0);
  obb::WsCursor c(base);
  VtWs w;
  w.best_label = c.take<int>(nn); w.best_iou = c.take<float>(nn); w.counter = c.take<int>(1);
  w.bytes = c.total();
  return w;
}
size_t obb_val_tail_batch_workspace_bytes(int64_t n_det, int64_t nt) { (void)nt; return vt_layout(nullptr, n_det).bytes; }

// the per-image table of a batch call from its host arrays (det_row_host NULL: packed detections); OBB_ERR_BAD_ARG when they are inconsistent
static int vt_fill_imgs(obb::ValTailImgs& im, const int64_t* det_row_host, const int64_t* det_off_host, int64_t bs, const float* img5_host) {
  const int64_t n = det_off_host[bs];
  if (n < 0 || n > 0x7fffffff || det_off_host[0] != 0) return OBB_ERR_BAD_ARG;
  im.bs = (int)bs;
  for (int b = 0; b <= (int)bs; b++) {
    if (b > 0 && det_off_host[b] < det_off_host[b - 1]) return OBB_ERR_BAD_ARG;
    im.det_off[b] = (int)det_off_host[b];
  }
  for (int b = 0; b < (int)bs; b++) {
    const int64_t r = det_row_host ? det_row_host[b] : det_off_host[b];
    if (r < 0 || r > 0x7fffffff - (det_off_host[b + 1] - det_off_host[b])) return OBB_ERR_BAD_ARG;
    im.det_row[b] = (int)r;
  }
  for (int b = 0; img5_host && b < (int)bs; b++) {             // (NULL: the oriented tail, which works in the frame of the rows)
    const float* q = img5_host + (size_t)b * 5;                 // pad_x, pad_y, gain, native width, native height
    if (!(q[2] > 0.f)) return OBB_ERR_BAD_ARG;
    im.pad_x[b] = q[0]; im.pad_y[b] = q[1]; im.gain[b] = q[2]; im.shape_w[b] = q[3]; im.shape_h[b] = q[4];
  }
  return OBB_OK;
}

static int val_tail_batch_impl(const float* det7, const int64_t* det_row_host, const int64_t* det_off_host, int64_t bs, const float* targets, int64_t nt, int64_t tcols,
                               const float* img5_host, const float* iouv, int niou, float* poly10, float* hbb6, float* polyn10,
                               float* hbbn6, float* stats, void* ws, size_t ws_bytes, void* stream, int64_t* done) {
  if (bs < 1 || bs > obb::kValTailMaxBs || nt < 0 || niou < 1 || !det_off_host || !img5_host || !iouv) return OBB_ERR_BAD_ARG;
  if (nt > 0 && (!targets || tcols < 7)) return OBB_ERR_BAD_ARG;
  if (nt > 0x7fffffff) return OBB_ERR_BAD_ARG;
  obb::ValTailImgs im;
  if (vt_fill_imgs(im, det_row_host, det_off_host, bs, img5_host) != OBB_OK) return OBB_ERR_BAD_ARG;
  const int64_t n = det_off_host[bs];
  if (n == 0) { if (done) *done = 0; return OBB_OK; }            // (host-visible memory: nothing to wait for)
  if (!det7 || !stats) return OBB_ERR_BAD_ARG;
  const VtWs w = vt_layout(ws, n);
  if (!obb::ws_ok(ws, ws_bytes, w.bytes)) return OBB_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  obb::k_vt_dets<<<(unsigned)((n + 127) / 128), 128, 0, st>>>(det7, (int)n, im, targets, (int)nt, (int)tcols, iouv, poly10, hbb6, polyn10, hbbn6,
                                                            w.best_label, w.best_iou, w.counter);
  obb::k_vt_stats<float><<<(unsigned)((n + 255) / 256), 256, 0, st>>>(det7, w.best_label, w.best_iou, im, iouv, (int)n, niou, stats, w.counter,
                                                              reinterpret_cast<long long*>(done));
  return hipGetLastError() == hipSuccess ? OBB_OK : OBB_ERR_LAUNCH;
}

int obb_val_tail_batch_f32(const float* det7, const int64_t* det_off_host, int64_t bs, const float* targets, int64_t nt, int64_t tcols,
                           const float* img5_host, const float* iouv, int niou, float* poly10, float* hbb6, float* polyn10,
                           float* hbbn6, float* stats, void* ws, size_t ws_bytes, void* stream) {
  return val_tail_batch_impl(det7, nullptr, det_off_host, bs, targets, nt, tcols, img5_host, iouv, niou, poly10, hbb6, polyn10, hbbn6, stats, ws,
                             ws_bytes, stream, nullptr);
}

int obb_val_tail_batch_polled_f32(const float* det7, const int64_t* det_off_host, int64_t bs, const float* targets, int64_t nt,
                                  int64_t tcols, const float* img5_host, const float* iouv, int niou, float* poly10, float* hbb6,
                                  float* polyn10, float* hbbn6, float* stats, void* ws, size_t ws_bytes, void* stream, int64_t* done) {
  if (!done) return OBB_ERR_BAD_ARG;
  return val_tail_batch_impl(det7, nullptr, det_off_host, bs, targets, nt, tcols, img5_host, iouv, niou, poly10, hbb6, polyn10, hbbn6, stats, ws,
                             ws_bytes, stream, done);
}

int obb_val_tail_batch_rows_f32(const float* det7, const int64_t* det_row_host, const int64_t* det_off_host, int64_t bs, const float* targets,
                                int64_t nt, int64_t tcols, const float* img5_host, const float* iouv, int niou, float* poly10, float* hbb6,
                                float* polyn10, float* hbbn6, float* stats, void* ws, size_t ws_bytes, void* stream, int64_t* done) {
  if (!det_row_host) return OBB_ERR_BAD_ARG;
  return val_tail_batch_impl(det7, det_row_host, det_off_host, bs, targets, nt, tcols, img5_host, iouv, niou, poly10, hbb6, polyn10, hbbn6, stats,
                             ws, ws_bytes, stream, done);
}

struct PbWs { int* best_label; float* best_iou; int* winner; size_t bytes; };
static PbWs pb_layout(void* base, int64_t n, int64_t m) {
  const size_t nn = (size_t)(n > 0 ? n : 0);
  obb::WsCursor c(base);
  PbWs w;
  w.best_label = c.take<int>(nn); w.best_iou = c.take<float>(nn); w.winner = c.take<int>((size_t)(m > 0 ? m : 1));   // (m == 0: one slot is still set)
  w.bytes = c.total();
  return w;
}
size_t obb_process_batch_workspace_bytes(int64_t n, int64_t m) { return pb_layout(nullptr, n, m).bytes; }

int obb_process_batch_f32(const float* det6, int64_t n, const float* lab5, int64_t m, const float* iouv, int niou, uint8_t* correct,
                          void* ws, size_t ws_bytes, void* stream) {
  if (n < 0 || m < 0 || niou < 1 || n > 0x7fffffff || m > 0x7fffffff) return OBB_ERR_BAD_ARG;
  if (n == 0) return OBB_OK;
  if (!det6 || !iouv || !correct || (m > 0 && !lab5)) return OBB_ERR_BAD_ARG;
  const PbWs w = pb_layout(ws, n, m);
  if (!obb::ws_ok(ws, ws_bytes, w.bytes)) return OBB_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(w.winner, 0x7f, (size_t)(m > 0 ? m : 1) * 4, st) != hipSuccess) return OBB_ERR_LAUNCH;
  obb::k_pb_best<<<(unsigned)((n + 127) / 128), 128, 0, st>>>(det6, (int)n, lab5, (int)m, iouv, w.best_label, w.best_iou, w.winner);
  obb::k_pb_correct<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(w.best_label, w.best_iou, w.winner, iouv, (int)n, niou, correct);
  return hipGetLastError() == hipSuccess ? OBB_OK : OBB_ERR_LAUNCH;
}

int obb_process_batch_obb_f32(const float* det7, int64_t n, const float* lab6, int64_t m, const float* iouv, int niou, uint8_t* correct,
                              int32_t* match_label, float* match_iou, void* stream) {
  if (n < 0 || m < 0 || niou < 1 || niou > 16 || n > 0x7fffffff || m > 0x7fffffff) return OBB_ERR_BAD_ARG;
  if (n == 0) return OBB_OK;
  if (!det7 || !iouv || !correct || !match_label || !match_iou || (m > 0 && !lab6)) return OBB_ERR_BAD_ARG;
  obb::ValTailImgs im = {};
  im.bs = 1; im.det_off[1] = (int)n;
  return obb::vo_launch<false, uint8_t>(det7, n, im, lab6, m, 6, iouv, niou, correct, match_label, match_iou, stream);
}

int obb_val_tail_batch_obb_f32(const float* det7, const int64_t* det_row_host, const int64_t* det_off_host, int64_t bs, const float* targets,
                               int64_t nt, int64_t tcols, const float* iouv, int niou, float* stats, int32_t* match_label, float* match_iou,
                               void* stream) {
  if (bs < 1 || bs > obb::kValTailMaxBs || nt < 0 || nt > 0x7fffffff || niou < 1 || niou > 16 || !det_off_host || !iouv) return OBB_ERR_BAD_ARG;
  if (nt > 0 && (!targets || tcols < 7)) return OBB_ERR_BAD_ARG;
  obb::ValTailImgs im;
  if (vt_fill_imgs(im, det_row_host, det_off_host, bs, nullptr) != OBB_OK) return OBB_ERR_BAD_ARG;
  const int64_t n = det_off_host[bs];
  if (n == 0) return OBB_OK;
  if (!det7 || !stats || !match_label || !match_iou) return OBB_ERR_BAD_ARG;
  return obb::vo_launch<true, float>(det7, n, im, targets, nt, tcols, iouv, niou, stats, match_label, match_iou, stream);
}

// the arrays of obb::CmWs: one block each
struct CmLayout { obb::CmWs w; size_t bytes; };
static CmLayout cm_layout(void* base, int64_t n, int64_t nt) {
  const size_t nn = (size_t)(n > 0 ? n : 0), ll = (size_t)(nt > 0 ? nt : 0);
  obb::WsCursor c(base);
  CmLayout l;
  l.w.win = c.take<unsigned long long>(ll);
  l.w.lbox = c.take<float>(4 * ll); l.w.lcls = c.take<int>(ll);
  l.w.dbox = c.take<float>(4 * nn); l.w.dcls = c.take<int>(nn);
  l.w.biou = c.take<float>(nn); l.w.blab = c.take<int>(nn);
  l.bytes = c.total();
  return l;
}
size_t obb_confusion_workspace_bytes(int64_t n_det, int64_t nt) { return cm_layout(nullptr, n_det, nt).bytes; }

int obb_confusion_batch_f32(const float* det7, const int64_t* det_off_host, int64_t bs, const float* targets, int64_t nt, int64_t tcols,
                            const float* img5_host, int nc, float conf_thres, float iou_thres, int64_t* matrix_i64, void* ws,
                            size_t ws_bytes, void* stream) {
  if (bs < 1 || bs > obb::kValTailMaxBs || nt < 0 || nt > 0x7fffffff || nc < 1 || nc > 32767 || !det_off_host || !img5_host || !matrix_i64)
    return OBB_ERR_BAD_ARG;
  if (nt > 0 && (!targets || tcols < 7)) return OBB_ERR_BAD_ARG;
  obb::ValTailImgs im;
  if (vt_fill_imgs(im, nullptr, det_off_host, bs, img5_host) != OBB_OK) return OBB_ERR_BAD_ARG;
  const int64_t n = det_off_host[bs];
  if (n == 0 || nt == 0) return OBB_OK;                          // no image has both detections and labels: nothing is counted
  if (!det7) return OBB_ERR_BAD_ARG;
  const CmLayout l = cm_layout(ws, n, nt);
  if (!obb::ws_ok(ws, ws_bytes, l.bytes)) return OBB_ERR_WORKSPACE;
  obb::k_confusion<true><<<(unsigned)bs, obb::kCmThreads, 0, (hipStream_t)stream>>>(
      det7, im, 0, targets, (int)nt, (int)tcols, nc, conf_thres, iou_thres, reinterpret_cast<unsigned long long*>(matrix_i64), l.w);
  return hipGetLastError() == hipSuccess ? OBB_OK : OBB_ERR_LAUNCH;
}

int obb_confusion_process_batch_f32(const float* det6, int64_t n, const float* lab5, int64_t m, int nc, float conf_thres, float iou_thres,
                                    int64_t* matrix_i64, void* ws, size_t ws_bytes, void* stream) {
  if (n < 0 || m < 0 || n > 0x7fffffff || m > 0x7fffffff || nc < 1 || nc > 32767 || !matrix_i64) return OBB_ERR_BAD_ARG;
  if (n == 0 || m == 0) return OBB_OK;
  if (!det6 || !lab5) return OBB_ERR_BAD_ARG;
  const CmLayout l = cm_layout(ws, n, m);
  if (!obb::ws_ok(ws, ws_bytes, l.bytes)) return OBB_ERR_WORKSPACE;
  obb::ValTailImgs im = {};                                      // (not read by the one-image form)
  obb::k_confusion<false><<<1, obb::kCmThreads, 0, (hipStream_t)stream>>>(
      det6, im, (int)n, lab5, (int)m, 5, nc, conf_thres, iou_thres, reinterpret_cast<unsigned long long*>(matrix_i64), l.w);
  return hipGetLastError() == hipSuccess ? OBB_OK : OBB_ERR_LAUNCH;
}

}  // extern "C"
