// Rotated / quad NMS entry points (C ABI) and nothing else: the single-list and merge drivers are in nms_single.h, the merge's
// device front in tile_merge.h, the fused
// non_max_suppression_obb driver in nmsobb_impl.h (fronts: nmsobb_front.h, nms_head.h), what they share in nms_driver.h.
//
// Replaces, on device tensors:
//   nms_rotated_ext.nms_rotated  (utils/nms_rotated/src/nms_rotated_ext.cpp:25-39 ->
//                                 nms_rotated_cuda, nms_rotated_cuda.cu:71-134)
//   nms_rotated_ext.nms_poly     (nms_rotated_ext.cpp:42-55 -> poly_nms_cuda, poly_nms_cuda.cu:197-261)
//   _poly_nms of the devkit      (DOTA_devkit/poly_nms_gpu/poly_nms_kernel.cu:277-329)
// Everything is stream-ordered on the caller's stream; nothing is copied to the
// host; the caller reads *num_keep when it needs the count.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "dtype_device.h"
#include "nms_driver.h"
#include "nms_head.h"
#include "nms_single.h"
#include "nmsobb_hints.h"
#include "nmsobb_impl.h"
#include "obb_hip.h"
#include "tile_merge.h"
#include "tta_head_plan.h"

using namespace obb;

extern "C" {

size_t obb_nms_workspace_bytes(int64_t n, int64_t nseg, int kind) {
  if (n < 0 || nseg < 1 || kind < 0 || kind > 5) return 0;
  return carve(nullptr, n, nseg, kind_recq(kind), cap_max(nseg), device_cus().cus).total;
}

int obb_nms_rotated_f32(const float* dets5, const float* scores, int64_t n, float iou_thr, int flags, int64_t max_keep,
                        int64_t* keep_out, int64_t* num_keep, void* ws, size_t ws_bytes, void* stream) {
  return run_nms(0, dets5, 5, scores, 1, n, iou_thr, flags, max_keep, keep_out, num_keep, ws, ws_bytes, (hipStream_t)stream);
}

int obb_nms_rotated_f64(const double* dets5, const double* scores, int64_t n, float iou_thr, int flags, int64_t max_keep,
                        int64_t* keep_out, int64_t* num_keep, void* ws, size_t ws_bytes, void* stream) {
  return run_nms_rot64(dets5, scores, n, iou_thr, flags, max_keep, keep_out, num_keep, ws, ws_bytes, (hipStream_t)stream);
}

int obb_nms_poly_f32(const float* polys, int64_t row_stride, int64_t n, float iou_thr, int64_t max_keep, int64_t* keep_out,
                     int64_t* num_keep, void* ws, size_t ws_bytes, void* stream) {
  if (row_stride < 9) return OBB_ERR_BAD_ARG;
  return run_nms(1, polys, (int)row_stride, polys ? polys + 8 : nullptr, (int)row_stride, n, iou_thr, 0, max_keep, keep_out, num_keep,
                 ws, ws_bytes, (hipStream_t)stream);
}


int obb_merge_nms_poly_f64(const double* dets9, int64_t n, const int32_t* order, const int32_t* seg_off, int64_t nseg, double thresh,
                           int64_t* keep_out, int64_t* num_keep, void* ws, size_t ws_bytes, void* stream) {
  return run_merge_nms(2, dets9, 9, n, order, seg_off, nseg, thresh, keep_out, num_keep, ws, ws_bytes, (hipStream_t)stream);
}

int obb_merge_nms_poly_all_f64(const double* dets9, int64_t n, const int32_t* order, const int32_t* seg_off, int64_t nseg, double thresh,
                               int64_t* keep_out, int64_t* num_keep, void* ws, size_t ws_bytes, void* stream) {
  return run_merge_nms(4, dets9, 9, n, order, seg_off, nseg, thresh, keep_out, num_keep, ws, ws_bytes, (hipStream_t)stream);
}

int obb_merge_nms_hbb_f64(const double* dets, int64_t row_stride, int64_t n, const int32_t* order, const int32_t* seg_off, int64_t nseg,
                          double thresh, int64_t* keep_out, int64_t* num_keep, void* ws, size_t ws_bytes, void* stream) {
  if (row_stride < 4 || row_stride > 0x7fffffff) return OBB_ERR_BAD_ARG;
  return run_merge_nms(5, dets, (int)row_stride, n, order, seg_off, nseg, thresh, keep_out, num_keep, ws, ws_bytes, (hipStream_t)stream);
}

// the device front of the merge (tile_merge.h): per-tile NMS outputs in, merged full-image detections out
size_t obb_tile_merge_workspace_bytes(int64_t n, int64_t n_src, int64_t nc) {
  if (n < 0 || n > 0x7fffffffLL || n_src < 1 || n_src > 0x7fffffffLL || nc < 1 || nc > kTmMaxNc || n_src * nc > 0x7fffffffLL) return 0;
  return tm_layout(nullptr, n, n_src * nc, 2, device_cus().cus).bytes;      // (both variants: one record layout, QuadGeom64)
}

int obb_tile_merge_f32(const float* det7, const int64_t* det_off_host, const obb_tile_rec* tiles_host, int64_t ntile, int64_t n_src,
                       int64_t nc, double thresh, int flags, double* out, int64_t* out_count, int32_t* info, void* ws, size_t ws_len,
                       void* stream) {
  return run_tile_merge(det7, det_off_host, tiles_host, ntile, n_src, nc, thresh, flags, out, out_count, info, ws, ws_len, (hipStream_t)stream);
}

// Devkit host-pointer API (DOTA_devkit/poly_nms_gpu/poly_nms.hpp:9-10, poly_nms_kernel.cu:277-329): the rows
// arrive pre-sorted by the caller (poly_nms.pyx:18-21) and are scanned in the given order; keep_out receives
// POSITIONS into that order.  Synchronous; errors are printed like the reference's CUDA_CHECK.
void _poly_nms(int* keep_out_host, int* num_out_host, const float* polys_host, int polys_num, int polys_dim,
               float nms_overlap_thresh, int device_id) {
  if (num_out_host) *num_out_host = 0;
  if (polys_num <= 0 || polys_dim < 8) return;
  int cur = 0;
  if (hipGetDevice(&cur) != hipSuccess) { fprintf(stderr, "_poly_nms: no HIP device\n"); return; }
  if (device_id >= 0 && device_id != cur) hipSetDevice(device_id);
  const size_t n = (size_t)polys_num;
  float *dp = nullptr, *ds = nullptr; int64_t *dk = nullptr, *dn = nullptr; void* ws = nullptr;
  const size_t wsb = obb_nms_workspace_bytes(polys_num, 1, 1);
  float* hs = (float*)malloc(n * 4);
  int64_t* hk = (int64_t*)malloc(n * 8);
  for (size_t i = 0; i < n; i++) hs[i] = (float)(n - i);      // strictly decreasing: keeps the given order (n < 2^24)
  hipError_t e = hipMalloc(&dp, n * polys_dim * 4);
  if (e == hipSuccess) e = hipMalloc(&ds, n * 4);
  if (e == hipSuccess) e = hipMalloc(&dk, n * 8);
  if (e == hipSuccess) e = hipMalloc(&dn, 8);
  if (e == hipSuccess) e = hipMalloc(&ws, wsb);
  if (e == hipSuccess) e = hipMemcpy(dp, polys_host, n * polys_dim * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(ds, hs, n * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    int rc = run_nms(1, dp, polys_dim, ds, 1, polys_num, nms_overlap_thresh, 0, 0, dk, dn, ws, wsb, (hipStream_t)0);
    if (rc) fprintf(stderr, "_poly_nms: launch failed (%d)\n", rc);
    int64_t cnt = 0;
    e = hipMemcpy(&cnt, dn, 8, hipMemcpyDeviceToHost);
    if (e == hipSuccess && cnt > 0) e = hipMemcpy(hk, dk, (size_t)cnt * 8, hipMemcpyDeviceToHost);
    if (e == hipSuccess) {
      for (int64_t i = 0; i < cnt; i++) keep_out_host[i] = (int)hk[i];
      if (num_out_host) *num_out_host = (int)cnt;
    }
  }
  if (e != hipSuccess) fprintf(stderr, "_poly_nms: %s\n", hipGetErrorString(e));
  hipFree(dp); hipFree(ds); hipFree(dk); hipFree(dn); hipFree(ws);
  free(hs); free(hk);
  if (device_id >= 0 && device_id != cur) hipSetDevice(cur);
}

// The reference declares this function with C++ linkage (poly_nms.hpp:9-10: no extern "C"), so a build of its Cython source
// (poly_nms.pyx, `cdef extern from "poly_nms.hpp"`) binds the MANGLED name: the same entry point under that name.
void obb_cxx_poly_nms(int* keep_out_host, int* num_out_host, const float* polys_host, int polys_num, int polys_dim,
                      float nms_overlap_thresh, int device_id) __asm__("_Z9_poly_nmsPiS_PKfiifi");
void obb_cxx_poly_nms(int* keep_out_host, int* num_out_host, const float* polys_host, int polys_num, int polys_dim,
                      float nms_overlap_thresh, int device_id) {
  _poly_nms(keep_out_host, num_out_host, polys_host, polys_num, polys_dim, nms_overlap_thresh, device_id);
}

size_t obb_nms_obb_workspace_bytes(int64_t bs, int64_t cap_img, int64_t nc, int agnostic) {
  if (bs < 1 || cap_img < 1 || nc < 1 || nc > 256) return 0;
  return obb_carve(nullptr, bs, cap_img, agnostic ? 1 : nc, device_cus().cus).total;
}

int obb_non_max_suppression_obb(const void* pred, int dtype, int64_t bs, int64_t A, int64_t no, float conf_thres,
                                float iou_thres, const int32_t* classes_host, int n_classes, int agnostic, int multi_label,
                                int64_t max_det, int64_t max_nms, float max_wh, const float* extra8, int64_t n_extra,
                                int64_t cap_img, int64_t expected_cand, float* out, int out_packed, int64_t* out_count,
                                int64_t* status, void* ws, size_t ws_bytes, void* stream) {
  return obb_non_max_suppression_obb_col(pred, nullptr, dtype, bs, A, no, conf_thres, iou_thres, classes_host, n_classes, agnostic,
                                         multi_label, max_det, max_nms, max_wh, extra8, n_extra, cap_img, expected_cand, out,
                                         out_packed, out_count, status, ws, ws_bytes, stream);
}

int obb_non_max_suppression_obb_col(const void* pred, const void* objcol, int dtype, int64_t bs, int64_t A, int64_t no,
                                    float conf_thres, float iou_thres, const int32_t* classes_host, int n_classes, int agnostic,
                                    int multi_label, int64_t max_det, int64_t max_nms, float max_wh, const float* extra8,
                                    int64_t n_extra, int64_t cap_img, int64_t expected_cand, float* out, int out_packed,
                                    int64_t* out_count, int64_t* status, void* ws, size_t ws_bytes, void* stream) {
  NmsObbCall c = nms_obb_call(dtype, bs, A, no, conf_thres, iou_thres, classes_host, n_classes, agnostic, multi_label, max_det, max_nms,
                              max_wh, extra8, n_extra, cap_img, expected_cand, out, out_packed, out_count, status, ws, ws_bytes, stream);
  c.pred = pred; c.objcol = objcol;
  return run_nms_obb(c);
}

size_t obb_nms_obb_state_bytes(int64_t bs) { return bs < 1 ? 0 : obb_state_bytes(bs); }

int obb_non_max_suppression_obb_st(const void* pred, const void* objcol, int dtype, int64_t bs, int64_t A, int64_t no,
                                   float conf_thres, float iou_thres, const int32_t* classes_host, int n_classes, int agnostic,
                                   int multi_label, int64_t max_det, int64_t max_nms, float max_wh, const float* extra8,
                                   int64_t n_extra, int64_t cap_img, int64_t expected_cand, float* out, int out_packed,
                                   int64_t* out_count, int64_t* status, void* ws, size_t ws_bytes, void* state, size_t state_bytes,
                                   void* stream) {
  if (!state) return OBB_ERR_BAD_ARG;
  NmsObbCall c = nms_obb_call(dtype, bs, A, no, conf_thres, iou_thres, classes_host, n_classes, agnostic, multi_label, max_det, max_nms,
                              max_wh, extra8, n_extra, cap_img, expected_cand, out, out_packed, out_count, status, ws, ws_bytes, stream);
  c.pred = pred; c.objcol = objcol; c.state = state; c.state_bytes = state_bytes;
  return run_nms_obb(c);
}

int obb_non_max_suppression_obb_head(int nl, const void* const* conv_out, int dtype, int64_t bs, int64_t na, int64_t no,
                                     const int64_t* ny, const int64_t* nx, const float* anchors_px_host, const float* strides_host,
                                     float conf_thres, float iou_thres, const int32_t* classes_host, int n_classes, int agnostic,
                                     int multi_label, int64_t max_det, int64_t max_nms, float max_wh, const float* extra8,
                                     int64_t n_extra, int64_t cap_img, int64_t expected_cand, float* out, int out_packed,
                                     int64_t* out_count, int64_t* status, void* ws, size_t ws_bytes, void* state, size_t state_bytes,
                                     void* stream) {
  // the limits of obb_detect_decode_levels and obb_non_max_suppression_obb, checked in host code (nms_head.h) before anything is launched
  HeadFront h;
  int64_t A = 0;
  if (const int rc = head_front_build(nl, conv_out, dtype, bs, na, no, ny, nx, anchors_px_host, strides_host, &h, &A)) return rc;
  NmsObbCall c = nms_obb_call(dtype, bs, A, no, conf_thres, iou_thres, classes_host, n_classes, agnostic, multi_label, max_det, max_nms,
                              max_wh, extra8, n_extra, cap_img, expected_cand, out, out_packed, out_count, status, ws, ws_bytes, stream);
  c.head = &h; c.state = state; c.state_bytes = state_bytes;
  return run_nms_obb(c);
}

int obb_non_max_suppression_obb_tta_head(int npass, const obb_tta_pass* passes_host, int dtype, int64_t bs, int64_t na, int64_t no,
                                         int64_t a_total, float conf_thres, float iou_thres, const int32_t* classes_host, int n_classes,
                                         int agnostic, int multi_label, int64_t max_det, int64_t max_nms, float max_wh, const float* extra8,
                                         int64_t n_extra, int64_t cap_img, int64_t expected_cand, float* out, int out_packed,
                                         int64_t* out_count, int64_t* status, void* ws, size_t ws_size, void* state, size_t state_bytes,
                                         void* stream) {
  // the limits of obb_detect_decode_tta and obb_non_max_suppression_obb_head, checked in host code (tta_head_plan.h) before anything is launched
  HeadFrontTta h;
  if (const int rc = head_tta_build(npass, passes_host, dtype, bs, na, no, a_total, &h, nullptr)) return rc;
  NmsObbCall c = nms_obb_call(dtype, bs, a_total, no, conf_thres, iou_thres, classes_host, n_classes, agnostic, multi_label, max_det, max_nms,
                              max_wh, extra8, n_extra, cap_img, expected_cand, out, out_packed, out_count, status, ws, ws_size, stream);
  c.tta = &h; c.state = state; c.state_bytes = state_bytes;
  return run_nms_obb(c);
}

int obb_profile_enable(int on) {
  g_prof.on = on == 2 ? 2 : (on != 0 ? 1 : 0);
  g_prof.used = 0;
  // the events exist before the first call that records one: creating them lazily put 2 x hipEventCreate per stage into the
  // caller's timed loop (bench.py's first loop ran 9-30 us per step slower than its later ones, depending on the host)
  if (g_prof.on) {
    const int want = 2048 < ProfState::kMax ? 2048 : ProfState::kMax;
    while (g_prof.created < want) {
      if (hipEventCreate(&g_prof.ev0[g_prof.created]) != hipSuccess) return OBB_ERR_INTERNAL;
      if (hipEventCreate(&g_prof.ev1[g_prof.created]) != hipSuccess) { hipEventDestroy(g_prof.ev0[g_prof.created]); return OBB_ERR_INTERNAL; }
      g_prof.created++;
    }
  }
  return OBB_OK;
}

int obb_profile_collect(double* ms_sum, int64_t* count, int n_stages) {
  for (int i = 0; i < n_stages; i++) { ms_sum[i] = 0.0; count[i] = 0; }
  for (int k = 0; k < g_prof.used; k++) {
    float ms = 0.f;
    if (hipEventSynchronize(g_prof.ev1[k]) != hipSuccess) return OBB_ERR_INTERNAL;
    if (hipEventElapsedTime(&ms, g_prof.ev0[k], g_prof.ev1[k]) != hipSuccess) return OBB_ERR_INTERNAL;
    const int id = g_prof.id[k];
    if (id < n_stages) { ms_sum[id] += ms; count[id]++; }
  }
  g_prof.used = 0;
  return OBB_OK;
}

int obb_nms_set_max_grid(int max_workgroups) {
  g_max_grid = max_workgroups > 0 ? max_workgroups : 0;
  return OBB_OK;
}

const char* obb_version(void) { return "obb_hip 0.2 (gfx950)"; }

int obb_device_info(int* cu_count, int* wave_size, char* arch_name, int arch_name_len) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return OBB_ERR_NO_DEVICE;
  hipDeviceProp_t p;
  if (hipGetDeviceProperties(&p, dev) != hipSuccess) return OBB_ERR_NO_DEVICE;
  if (cu_count) *cu_count = p.multiProcessorCount;
  if (wave_size) *wave_size = p.warpSize;
  if (arch_name && arch_name_len > 0) { strncpy(arch_name, p.gcnArchName, arch_name_len - 1); arch_name[arch_name_len - 1] = 0; }
  return OBB_OK;
}

}  // extern "C"

#ifdef OBB_DECODE_TRACE
// (development builds, tools/decode_trace.sh) the stamps of the last k_decode launch; the buffer is cleared
extern "C" int obb_debug_decode_trace(unsigned long long* words) {
  static unsigned long long zero[obb::kDecTraceWgs * 16];
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  if (hipMemcpyFromSymbol(words, HIP_SYMBOL(obb::g_decode_trace), sizeof(obb::g_decode_trace)) != hipSuccess) return -2;
  return hipMemcpyToSymbol(HIP_SYMBOL(obb::g_decode_trace), zero, sizeof(obb::g_decode_trace)) == hipSuccess ? 0 : -3;
}
#endif

#ifdef OBB_SMALL_TRACE
// (development builds, tools/small_trace.sh) the stamps of the last k_nms_small launch; both buffers are cleared
extern "C" int obb_debug_small_trace2(unsigned long long* words) {
  static unsigned long long zero2[2048 * 8];
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  if (hipMemcpyFromSymbol(words, HIP_SYMBOL(obb::g_small_trace2), sizeof(obb::g_small_trace2)) != hipSuccess) return -1;
  return hipMemcpyToSymbol(HIP_SYMBOL(obb::g_small_trace2), zero2, sizeof(obb::g_small_trace2)) == hipSuccess ? 0 : -1;
}
extern "C" int obb_debug_small_trace(unsigned long long* seg_words, unsigned long long* tail_words) {
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  if (hipMemcpyFromSymbol(seg_words, HIP_SYMBOL(obb::g_small_trace), sizeof(obb::g_small_trace)) != hipSuccess) return -2;
  if (hipMemcpyFromSymbol(tail_words, HIP_SYMBOL(obb::g_small_trace_tail), sizeof(obb::g_small_trace_tail)) != hipSuccess) return -3;
  static unsigned long long zero[2048 * 16];
  if (hipMemcpyToSymbol(HIP_SYMBOL(obb::g_small_trace), zero, sizeof(obb::g_small_trace)) != hipSuccess) return -4;
  if (hipMemcpyToSymbol(HIP_SYMBOL(obb::g_small_trace_tail), zero, sizeof(obb::g_small_trace_tail)) != hipSuccess) return -5;
  return 0;
}
#endif
