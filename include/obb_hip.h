/*
 * obb_hip.h -- C ABI of libobb_hip.so, the MI355X (gfx950) oriented-box hot path.
 *
 * Drop-in boundary for hukaixuan19970627/yolov5_obb: every entry point names the
 * reference interface it replaces (file:line, relative to the reference root).
 * Conventions shared by all functions:
 *   - plain C: raw pointers + sizes, no torch / ATen types;
 *   - every pointer is a DEVICE pointer unless its name ends in `_host`;
 *   - buffers are caller-owned; inputs are never modified;
 *   - work is enqueued on `stream` (a hipStream_t passed as void*; NULL = the
 *     default stream) and is stream-ordered: no hidden host synchronisation, no
 *     allocation, no device->host copy.  Scratch memory comes from `ws`
 *     (size from the matching *_workspace_bytes query; 256-byte aligned);
 *   - return value: OBB_OK (0) or a negative OBB_ERR_* code; nothing throws.
 *     The Python host layer turns codes into RuntimeError, mirroring the
 *     reference's AT_ASSERTM / AT_ERROR -> RuntimeError behaviour
 *     (utils/nms_rotated/src/nms_rotated_ext.cpp:29-54).
 *   - floating point: IEEE fp32, no FMA contraction; results are defined by the
 *     CPU oracle in oracle/ (pinned to the reference's own sources).
 */
#ifndef OBB_HIP_H
#define OBB_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OBB_OK 0
#define OBB_ERR_BAD_ARG (-1)
#define OBB_ERR_WORKSPACE (-2)   /* ws (or state) == NULL, not 256-byte aligned, or ws_bytes (state_bytes) too small: answered before any device call */
#define OBB_ERR_LAUNCH (-3)      /* a kernel launch failed (see hipGetLastError) */
#define OBB_ERR_INTERNAL (-4)
#define OBB_ERR_NO_DEVICE (-5)

/* Element type of a tensor handed over as `const void*` with a `dtype` argument (the Detect head's conv outputs, the prediction
 * tensor built from them, the loss gradients): torch.float32, torch.float16 (val.py --half, model.half()) and torch.bfloat16
 * (model.bfloat16(), torch.autocast(dtype=torch.bfloat16)).  Code 2 is RESERVED: it is refused like every other unknown code
 * (OBB_ERR_BAD_ARG before any device call) and will not be given a meaning.  Where an entry's arithmetic "follows the input dtype",
 * bf16 rounds float results to nearest even like c10::BFloat16 (a NaN becomes the quiet NaN 0x7FC0; finite values beyond the bf16
 * range round to inf) -- csrc/bf16_bits.h. */
#define OBB_DTYPE_F32 0
#define OBB_DTYPE_F16 1
#define OBB_DTYPE_BF16 3

/* flags for obb_nms_rotated_* */
#define OBB_NMS_DROP_SMALL 1 /* ignore boxes with min(w,h) < 0.001 (utils/nms_rotated/nms_rotated_wrapper.py:32-39) */

/* Library / device identification: returns OBB_OK and fills the fields when a gfx950-class device is usable. */
const char* obb_version(void);
int obb_device_info(int* cu_count, int* wave_size, char* arch_name, int arch_name_len);
/* The persistent NMS kernel launches one workgroup per CU and its workgroups meet at spin barriers: they must all be
 * resident.  Where that cannot be taken for granted (CU masking, a partition that exposes fewer CUs than it reports, a
 * long kernel of another process holding CUs) a barrier times out and the call reports -1 kept boxes instead of hanging.
 * max_workgroups > 0 caps the grid of the following launches of the CALLING THREAD (thread-local state: the host layer
 * retries an aborted call once with 8 workgroups and restores the default in a finally block; concurrent callers on other
 * threads are not affected, and one call sizes its workspace and its grid from the same value); 0 restores the default
 * (the CU count). */
int obb_nms_set_max_grid(int max_workgroups);

/* Optional per-stage timing with HIP events recorded on the caller's stream (used by bench.py for the roofline
 * object).  Stage ids: 0 decode/filter kernel, 1 per-image sort, 2 candidate prep, 3 NMS steps, 4 output gather of
 * obb_non_max_suppression_obb; 5 sort, 6 prep, 7 NMS steps of obb_nms_*.  obb_profile_collect synchronises the
 * recorded events, returns summed milliseconds and launch counts per stage, and resets the recording.
 * on = 1: every stage (ten event records per fused call: ~30 us of a 0.2 ms step); on = 2: only the NMS kernels (stages 3 and 7,
 * the dominant kernel of a call: two records); 0: off. */
#define OBB_PROF_STAGES 8
int obb_profile_enable(int on);
int obb_profile_collect(double* ms_sum_host, int64_t* count_host, int n_stages);

/* Environment variables read by the library (once per process).  Every build:
 *   OBB_NMS_POLY_STRICT=1   quad NMS: only the proved skip rules (csrc/piou_device.h: the two cone rules); =2: no rule at all, every pair
 *                           is clipped like the reference does (tests/test_nms_gpu.py::test_nms_poly_strict_equals_skip_100k)
 *   OBB_NMS_PHASE_PROF=1    in-kernel phase timers of the single-list NMS (either path), printed to stderr (synchronises; development aid)
 * Read per call (tests switch paths inside one process; nothing but speed depends on them -- the kept list is the same on every path):
 *   OBB_NMS_MK=0 | 1 | 2    single-list rotated NMS of >= 16384 boxes: 0 the persistent kernel (csrc/nms_core.h), 1 the phase kernels
 *                           (csrc/nms_mk.h), 2 = default: the library's choice from what the calling thread's previous calls of the size
 *                           class reported (kept boxes, independent slabs, device time of either path)
 *   OBB_NMS_MK_XLDS=0 | 1   phase kernels: the cross probe on the chunk's table in global memory (0) or on a table of the kept rows in
 *                           every workgroup's LDS (1); default: 1 where the previous call kept <= 6144 boxes
 *   OBB_NMS_SELF_SORT=0|1|2 obb_non_max_suppression_obb* with the small-segment NMS kernel (expected_cand bits 32..60) and out_packed = 0:
 *                           0 = the per-image sort kernel in front of it, 1 = self-sorting segments (csrc/nmsobb_impl.h: SmallSelfSort --
 *                           no sort launch, two launches per call) where the sort kernel would hand out no helper workgroups,
 *                           2 = default: self-sorting segments wherever they are possible
 *   OBB_NMS_SMALL_HELPERS=n small-segment NMS kernel behind the sort kernel: helper workgroups that share large segments (0: none)
 * Read once per process, tests only: OBB_NMS_MK_STEPS (enqueued steps), OBB_NMS_MK_PEND (pending-list capacity): they force the
 * hand-overs to the persistent kernel that tests/test_nms_mk_gpu.py checks.
 * Compile-time diagnostics (-D, csrc/): OBB_SMALL_TRACE, OBB_SORT_TRACE (per-workgroup time stamps printed by the kernels),
 * OBB_NMS_FULL_FENCE (a full fence where the kernels read other workgroups' results: a check for stale reads). */

/* ------------------------------------------------------------------ NMS ------------------------------ */

/* Scratch bytes for n boxes in nseg segments.  kind: 0 = rotated boxes, 1 = quads, 2 = double-precision quads (merge NMS),
 * 3 = double-precision rotated boxes (obb_nms_rotated_f64), 4 = obb_merge_nms_poly_all_f64, 5 = obb_merge_nms_hbb_f64. */
size_t obb_nms_workspace_bytes(int64_t n, int64_t nseg, int kind);

/*
 * Rotated-box NMS.  Replaces nms_rotated_ext.nms_rotated on CUDA tensors
 * (utils/nms_rotated/src/nms_rotated_ext.cpp:25-39 -> nms_rotated_cuda,
 *  utils/nms_rotated/src/nms_rotated_cuda.cu:71-134: sort, N x N/64 mask kernel,
 *  device->host mask copy, host greedy scan).
 *   dets5    [n,5] fp32 contiguous  (cx, cy, w, h, angle in RADIANS)
 *   scores   [n]   fp32
 *   iou_thr  a box is dropped iff an earlier kept box has IoU > iou_thr (strict, cu:60)
 *   max_keep 0 = unlimited; otherwise stop after this many kept boxes (the caller's max_det,
 *            utils/general.py:854-855 truncates the same prefix)
 *   keep_out [n] int64: original indices of kept boxes in descending-score order
 *            (ties: ascending index; NaN scores first -- torch.sort's order)
 *   num_keep [1] int64 (device)
 * Lists of >= 16384 boxes without max_keep: two implementations of the same lazy chunked greedy NMS sit behind this entry -- a chain
 * of ordinary launches, one per phase (no co-residency needed), and one persistent kernel behind spin barriers (see
 * obb_nms_set_max_grid) -- and the library takes the one that was faster for the calling thread's previous calls of the size class
 * (eight pinned words per size class that the device writes and the host reads, once per call, without synchronising: [0] the steps
 * the call needed or -2 "started / handed over", [1] boxes kept, [2] slabs found, [3] steps enqueued -- written by the host --,
 * [4] / [5] 10 ns ticks of the call on the persistent kernel / the phase kernels, [6] / [7] the kept counts those times came with;
 * csrc/nms_plan.h names them).  The persistent kernel is always
 * launched last: it completes whatever the enqueued phases left undone and returns at once otherwise.
 */
int obb_nms_rotated_f32(const float* dets5, const float* scores, int64_t n, float iou_thr, int flags, int64_t max_keep,
                        int64_t* keep_out, int64_t* num_keep, void* ws, size_t ws_bytes, void* stream);

/*
 * The same for float64 tensors: the reference dispatches double to a double-precision instantiation of the kernel
 * (AT_DISPATCH_FLOATING_TYPES, nms_rotated_cuda.cu:96; box_iou_rotated_utils.h:333-360 with T = double).  dets5 / scores
 * are doubles; every IoU is computed in double and compared with the FLOAT threshold of the kernel's signature
 * (nms_rotated_cuda.cu:14,60).  Workspace: obb_nms_workspace_bytes(n, 1, 3).
 */
int obb_nms_rotated_f64(const double* dets5, const double* scores, int64_t n, float iou_thr, int flags, int64_t max_keep,
                        int64_t* keep_out, int64_t* num_keep, void* ws, size_t ws_bytes, void* stream);

/*
 * Quadrilateral NMS.  Replaces nms_rotated_ext.nms_poly (nms_rotated_ext.cpp:42-55 -> poly_nms_cuda,
 * utils/nms_rotated/src/poly_nms_cuda.cu:197-261).  Rows are x1 y1 x2 y2 x3 y3 x4 y4 score (+ ignored extra
 * columns): row_stride >= 9 floats.  Kept set = the reference's greedy scan over devPolyIoU (poly_nms_cuda.cu:26-142).  Pairs whose
 * bounding boxes are disjoint AND whose areas outweigh the rounding noise of the reference's origin-based sum (a bound of
 * 1024 * 2^-24 * M^2 per box, M = its largest |coordinate|) are not clipped.  That bound is backed by search
 * (2.8 * 10^10 skip decisions, none wrong), not by proof, and is only applied inside the envelope the search covered: a quad with
 * every |coordinate| <= 70,000 and a bounding box of at most 600 x 600; any other quad is decided by the two PROVED rules (the two
 * quads' cones, as seen from the coordinate origin, apart by a margin in either order: all 16 terms exactly zero -- csrc/piou_device.h:
 * quad_cone_skip, quad_cone2_skip / quad_cone2_nofuzzy) or clipped like the reference does.
 * OBB_NMS_POLY_STRICT=1 keeps only the proved rules (4.5x the default's time at 30,000 quads), =2 clips every pair.
 */
int obb_nms_poly_f32(const float* polys, int64_t row_stride, int64_t n, float iou_thr, int64_t max_keep, int64_t* keep_out,
                     int64_t* num_keep, void* ws, size_t ws_bytes, void* stream);

/*
 * Tile -> full-image merge NMS in double precision.  Replaces py_cpu_nms_poly_fast
 * (DOTA_devkit/ResultMerge_multi_process.py:62-123; the same function in ResultMerge.py and
 * ResultEnsembleNMS_multi_process.py) for ALL images of a Task1_<class>.txt file in one call: the horizontal-box
 * gate (hbb_ovr > 0, :82-98) followed by DOTA_devkit/polyiou.cpp:108-128 (iou_poly) in IEEE double, a box
 * being dropped unless iou <= thresh (:115; a NaN IoU drops it).
 *   dets9    (n, 9) doubles  x1 y1 .. x4 y4 score  (only the 8 coordinates are read)
 *   order    (n) int32       row indices in processing order, segment after segment: the caller applies the reference's
 *                            `scores.argsort()[::-1]` (:79) per image, so score ties are ordered exactly like numpy's
 *   seg_off  (nseg + 1) int32  segment g = order[seg_off[g] .. seg_off[g+1])
 *   keep_out (n) int64       kept ROW indices of segment g at keep_out[seg_off[g] + k], k < num_keep[g], processing order
 *   num_keep (nseg) int64    (-1 in every entry: the device gave up on an internal barrier)
 * Workspace: obb_nms_workspace_bytes(n, nseg, 2).
 */
int obb_merge_nms_poly_f64(const double* dets9, int64_t n, const int32_t* order, const int32_t* seg_off, int64_t nseg,
                           double thresh, int64_t* keep_out, int64_t* num_keep, void* ws, size_t ws_bytes, void* stream);

/*
 * The other two merge variants of the same file, same conventions (order / seg_off / keep_out / num_keep as above):
 *   obb_merge_nms_poly_all_f64   py_cpu_nms_poly (ResultMerge_multi_process.py:24-60): no horizontal-box gate -- iou_poly of the
 *                                kept box and EVERY remaining candidate.  Workspace: obb_nms_workspace_bytes(n, nseg, 4).
 *   obb_merge_nms_hbb_f64        py_cpu_nms (:125-157; what mergebyrec hands to mergebase): horizontal boxes [x1 y1 x2 y2] in
 *                                columns 0..3 of rows of row_stride doubles, "+ 1" in areas and intersections, numpy double
 *                                arithmetic incl. its NaN rules (np.maximum hands a NaN through; 0 / 0 removes the box).
 *                                Workspace: obb_nms_workspace_bytes(n, nseg, 5).
 */
int obb_merge_nms_poly_all_f64(const double* dets9, int64_t n, const int32_t* order, const int32_t* seg_off, int64_t nseg,
                               double thresh, int64_t* keep_out, int64_t* num_keep, void* ws, size_t ws_bytes, void* stream);
int obb_merge_nms_hbb_f64(const double* dets, int64_t row_stride, int64_t n, const int32_t* order, const int32_t* seg_off,
                          int64_t nseg, double thresh, int64_t* keep_out, int64_t* num_keep, void* ws, size_t ws_bytes, void* stream);

/*
 * In-memory tile -> full-image merge: from the per-tile outputs of non_max_suppression_obb straight to the merged detections of
 * the source images, without the text hand-off of the reference's workflow (val.py:50-66 save_one_json ->
 * tools/TestJson2VocClassTxt.py -> DOTA_devkit/ResultMerge_multi_process.py:183-234).  Per row, in the reference's order:
 * rbox2poly and scale_polys in float32 (the bits of obb_val_postprocess_f32's pred_polyn), with OBB_TILE_MERGE_TEXT_ROUNDING
 * Python's round(x, 1) of the coordinates and round(conf, 5) of the score as the text carries them (csrc/tile_merge_math.h),
 * poly2origpoly (v + left | up) / rate in double; then the merge NMS of obb_merge_nms_poly_f64 (OBB_TILE_MERGE_POLY_ALL:
 * obb_merge_nms_poly_all_f64) per (source image, class).
 *   det7          (n, 7) fp32 device rows [cx cy l s theta conf cls], the tiles back to back, n = det_off_host[ntile]
 *   det_off_host  (ntile + 1) int64 host: tile t owns rows det_off_host[t] .. det_off_host[t + 1]; [0] = 0, ascending
 *   tiles_host    (ntile) obb_tile_rec host: source image in [0, n_src), the tile's origin in the (resized) image, the resize rate
 *                 of its name (> 0), and scale_polys' pad and gain (gain > 0; 0, 0, 1 for a tile fed at the model's size)
 *   thresh        the merge threshold, a Python float (nms_thresh = 0.2 in the reference)
 *   out           (n, 11) doubles, the first sum(out_count) rows written: [8 source-image coordinates, score, cls, src_image],
 *                 source image ascending, class ascending, processing order inside
 *   out_count     (n_src * nc) int64: kept rows of segment src_image * nc + cls
 *   info          (2) int32: [0] != 0: some row's class is not an integer in [0, nc) (it was counted as class 0; the result is
 *                 invalid); [1] != 0: the NMS kernel gave up on an internal barrier (every count is 0)
 * Processing order inside a segment: score descending -- with text rounding the ROUNDED score, so scores that print alike tie --
 * ties in ascending input row (tile order, then the row inside the tile).  numpy's argsort()[::-1] in the reference leaves ties
 * to its sort; where a segment has none, text rounding gives the file pipeline's result bit for bit.  Without it the rows
 * keep the full float32 precision: not the file pipeline's result.
 * All work is plain launches on `stream`; nothing is copied to the host.  1 <= nc <= 256, n, ntile and n_src * nc below 2^31,
 * else OBB_ERR_BAD_ARG before any device call.  Workspace: obb_tile_merge_workspace_bytes(n, n_src, nc).
 */
#define OBB_TILE_MERGE_TEXT_ROUNDING 1
#define OBB_TILE_MERGE_POLY_ALL 2
typedef struct obb_tile_rec {
  int32_t src_image, left, up;
  double rate;
  float pad_x, pad_y, gain;
} obb_tile_rec;
size_t obb_tile_merge_workspace_bytes(int64_t n, int64_t n_src, int64_t nc);
int obb_tile_merge_f32(const float* det7, const int64_t* det_off_host, const obb_tile_rec* tiles_host, int64_t ntile, int64_t n_src,
                       int64_t nc, double thresh, int flags, double* out, int64_t* out_count, int32_t* info, void* ws, size_t ws_len,
                       void* stream);

/*
 * DOTA Task-1 evaluation: the detection x ground-truth part of voc_eval (DOTA_devkit/dota_evaluation_task1.py:168-223)
 * for all detections of a class file in one call.  Per detection, over the ground-truth quads of its own image: the
 * horizontal-box gate with the +1 convention (:181-204), iou_poly(GT, det) of DOTA_devkit/polyiou.cpp in IEEE double for
 * the quads that pass (:206-213), then np.max / np.argmax (:215-218).
 *   dets8   (nd, 8) doubles, in the caller's (confidence-sorted) order      det_img (nd) int32  image index of a detection
 *   gts8    (ng, 8) doubles, the quads of image i at gt_off[i] .. gt_off[i+1]   gt_off (n_img + 1) int32
 *   ovmax   (nd) doubles   -inf: no quad passed the gate (:172); NaN: some IoU was NaN
 *   jmax    (nd) int32     index within the image's list (first maximum; first NaN; -1 with -inf)
 * The sequential TP/FP marking (:225-233) is a first-occurrence pass over (image, jmax) and stays with the caller.
 */
int obb_eval_best_gt_f64(const double* dets8, const int32_t* det_img, int64_t nd, const double* gts8, const int32_t* gt_off,
                         int64_t n_img, double* ovmax, int32_t* jmax, void* stream);

/*
 * In-memory DOTA Task-1 evaluation: the whole of voc_eval (DOTA_devkit/dota_evaluation_task1.py:88-249) for every class in one
 * launch chain -- merged full-image rows and a resident ground-truth set in, per-class AP out (csrc/task1_eval.h; the arithmetic of
 * the curve, of voc_ap and of its np.sum is csrc/voc_ap_math.h, IEEE double in numpy's order).
 *   dets      nd rows of det_stride >= 11 doubles, the layout obb_tile_merge_f32 writes: [x1 y1 .. x4 y4, score, cls, src_image]
 *             (a slice of its `out` is passed as it is); rows are evaluated with the values they carry
 *   gts8      (ng, 8) doubles grouped by segment cls * n_img + img     gt_off (nc * n_img + 1) int32, ascending, [last] = ng
 *   difficult (ng) uint8: a hit on such a record is neither TP nor FP, and npos does not count it
 *   ovthresh  a hit is ovmax > ovthresh (NaN and -inf: no)            flags  OBB_TASK1_EVAL_07_METRIC: the 11-point metric
 *   ap        (nc) doubles; a class without detections evaluates literally, to 0.0      npos (nc) int64
 *   cls_off   (nc + 1) int32: class c owns the sorted positions cls_off[c] .. cls_off[c + 1]
 *   order     (nd) int32 or NULL: the input row at every sorted position
 *   rec, prec (nd) doubles or NULL: the curves, class after class.  npos == 0 gives NaN or inf recalls as numpy does; a NaN is
 *             the canonical quiet NaN (payload and sign are not numpy's), every other value has the reference's bits
 *   info      (2) int32: [0] != 0: some row's class is not an integer in [0, nc) or its image not one in [0, n_img) (the reference
 *             raises KeyError for an unlisted image); such a row is counted in segment 0, nothing is read out of bounds, the result
 *             is invalid.  [1]: reserved, 0
 * Order inside a class: score descending, NaN scores last, -0.0 and +0.0 one value (np.argsort(-confidence)); equal scores in
 * ascending input row (the package's pinned tie rule; the reference leaves ties to numpy's unstable sort).  A record is claimed by
 * the lowest sorted position that hits it (an atomic minimum per record: independent of the order the atomics land in).
 * All work is plain launches on `stream`; nothing is copied to the host, nothing waits.  OBB_ERR_BAD_ARG before any device call
 * for det_stride < 11, nc outside 1..256, a negative count, nd, ng or nc * n_img at or above 2^31, unknown flags or a NULL
 * required pointer (dets with nd > 0; gts8, difficult with ng > 0).  nd == 0: ap = 0, cls_off = 0, npos counted.  The workspace
 * follows the rules of ws / ws_bytes of the other entries (256-byte aligned, at least obb_task1_eval_workspace_bytes, which is 0
 * for arguments the entry refuses; OBB_ERR_WORKSPACE before any device call).
 */
#define OBB_TASK1_EVAL_07_METRIC 1
size_t obb_task1_eval_workspace_bytes(int64_t nd, int64_t ng, int64_t n_img, int64_t nc);
int obb_task1_eval_f64(const double* dets, int64_t det_stride, int64_t nd, const double* gts8, const int32_t* gt_off,
                       const uint8_t* difficult, int64_t ng, int64_t n_img, int64_t nc, double ovthresh, int flags, double* ap,
                       int64_t* npos, int32_t* cls_off, int32_t* order, double* rec, double* prec, int32_t* info, void* ws,
                       size_t ws_extent, void* stream);

/*
 * DOTA Task-2 (horizontal box) evaluation: the same part of DOTA_devkit/dota_evaluation_task2.py's voc_eval (:177-202).
 * Per detection, over the boxes of its own image, in IEEE double and in the reference's expression order:
 *   iw = max(min(gx2, bx2) - max(gx1, bx1) + 1., 0.), ih alike, inters = iw * ih,
 *   uni = (bx2 - bx1 + 1.) * (by2 - by1 + 1.) + (gx2 - gx1 + 1.) * (gy2 - gy1 + 1.) - inters, overlaps = inters / uni
 * with numpy's maximum / minimum (a NaN operand is the result) and no `overlaps > 0` gate, then np.max / np.argmax.
 *   dets4   (nd) rows of det_stride >= 4 doubles, the first four xmin ymin xmax ymax (BB[d, :] of a wider row works)
 *   det_img (nd) int32     image index of a detection; one outside [0, n_img) is treated as an image without boxes
 *   gts4    (ng, 4) doubles, already truncated by the caller (:34-37), image i at gt_off[i] .. gt_off[i+1]
 *   ovmax   (nd) doubles   the first maximum in list order; NaN: some overlap was NaN; -inf: the image has no box.
 *                          A NaN is written as the canonical quiet NaN: payload and sign are not the reference's (numpy's
 *                          0 / 0 on x86 has the sign bit set); every other value has the reference's bits
 *   jmax    (nd) int32     its index within the image's list (the first NaN with NaN; -1 with -inf)
 * No workspace.  Stream-ordered, no synchronisation.  det_stride < 4, a negative count or a NULL required pointer with
 * nd > 0: OBB_ERR_BAD_ARG before any device call; nd == 0: OBB_OK, nothing is launched.
 */
int obb_eval_best_gt_hbb_f64(const double* dets4, int64_t det_stride, const int32_t* det_img, int64_t nd, const double* gts4,
                             const int32_t* gt_off, int64_t n_img, double* ovmax, int32_t* jmax, void* stream);

/*
 * Host-side text I/O of the merge (no device work; csrc/textio.hip).  obb_task1_parse_tiles restates
 * DOTA_devkit/ResultMerge_multi_process.py:186-213 for a whole Task1_<class>.txt buffer: per line
 * `<orig>__<rate>__<x>___<y> score x1 y1 .. x4 y4` -> dets9[line] = [8 source-image coordinates (poly + x|y) / rate,
 * score] (strtod = Python's float()), the position of <orig> in the text, a group id per distinct <orig> in order of
 * first appearance and the first line of every group.  Returns the number of lines, or OBB_ERR_BAD_ARG for anything that
 * is not the plain layout (the Python layer then parses line by line like the reference).
 * obb_task1_format_rows writes `<orig> <round(score, 2)> <round(c, 1)> x 8\n` for the given lines (:218-233) and returns
 * the number of bytes (OBB_ERR_WORKSPACE: out_cap too small; 200 bytes per row + the name suffice for |values| < 1e15;
 * the text equals Python's str(round(..)) for |confidence| < 1e13 and |coordinates| < 1e14, the domain the Python layer checks).
 */
int64_t obb_task1_parse_tiles(const char* text_host, int64_t len, int64_t max_lines, double* dets9_host, int32_t* name_off_host,
                              int32_t* name_len_host, int32_t* group_host, int32_t* group_first_host, int64_t* n_groups_host);
/* The two readers of the Task-1 evaluation (dota_evaluation_task1.py): detections `image score x1 y1 .. x4 y4` (:152-160)
 * -> conf[line], bb8[line][8], position of the image id; ground truth `x1 .. y4 name [difficult]` (:21-53; lines with fewer
 * than 9 fields skipped, difficult = 0 when absent) -> bbox8, position of the class name, the flag.  Same contract as
 * obb_task1_parse_tiles: the number of records, or OBB_ERR_BAD_ARG for a buffer that is not the plain layout. */
int64_t obb_task1_parse_dets(const char* text_host, int64_t len, int64_t max_lines, double* conf_host, double* bb8_host,
                             int32_t* name_off_host, int32_t* name_len_host);
int64_t obb_task1_parse_gt(const char* text_host, int64_t len, int64_t max_lines, double* bbox8_host, int32_t* name_off_host,
                           int32_t* name_len_host, int32_t* difficult_host);
int64_t obb_task1_format_rows(const char* text_host, const int32_t* name_off_host, const int32_t* name_len_host,
                              const double* dets9_host, const int64_t* rows_host, int64_t n_rows, char* out_host, int64_t out_cap);

/* ------------------------------------------------------------------ fused NMS driver ----------------- */

/*
 * The whole of non_max_suppression_obb (utils/general.py:772-862) for a batch, in one stream-ordered call:
 * confidence filter, obj*cls, CSL decode (arg-max over the 180 angle bins -> theta = (idx-90)/180*3.141592),
 * multi-label expansion or best class, class filter, per-image top max_nms by confidence, class offset
 * (xy += cls*max_wh unless agnostic), obb_nms (incl. its min(w,h) < 0.001 filter), max_det truncation.
 *   pred        [bs][A][no] contiguous, no = 5 + nc + 180, rows [cx cy l s obj cls[nc] csl[180]] as produced by
 *               Detect's inference branch (models/yolo.py:67-81); dtype OBB_DTYPE_F32 / OBB_DTYPE_F16 (val.py --half) / OBB_DTYPE_BF16.
 *               The arithmetic follows the input dtype exactly like the reference (conf = obj*cls is rounded to
 *               fp16 for fp16 input and to bf16 for bf16 input, thresholds are compared in that dtype).
 *   classes_host  optional HOST array of allowed class ids (n_classes entries; NULL = all)     (:834-835)
 *   extra8      optional device rows [img, x, y, l, s, theta, conf, cls] appended as candidates: the apriori
 *               `labels` of autolabelling (:807-813), prepared by the host layer; n_extra rows
 *   cap_img     candidate slots reserved per image.  If an image produces more, status[0] receives that count
 *               (> cap_img) and the caller must retry with a larger cap_img (A*nc can never overflow).
 *   expected_cand  what the caller expects, from status[1] of its previous call of this shape (0 = unknown: always valid):
 *               bits 0..31  candidates per image.  Selects the sort: 1 .. OBB_NMS_SORT_LDS_HINT -> the images are sorted in LDS
 *               by a kernel that also builds the NMS records (six launches fewer); larger -> the multi-workgroup sorts of
 *               csrc/segsort.h / csrc/psrs_sort.h.  The in-LDS sort takes at most OBB_NMS_SORT_LDS_MAX candidates of an image:
 *               with a hint in 1 .. OBB_NMS_SORT_LDS_HINT and status[1] (low word) > OBB_NMS_SORT_LDS_MAX after the call, such
 *               images were left EMPTY -- call again with that count as the hint.
 *               bits 32..60 the largest NMS segment (boxes of one class of one image).  1 .. OBB_NMS_SMALL_SEG together with the
 *               in-LDS sort and iou_thres >= 0 selects the one-workgroup-per-segment NMS kernel (csrc/nms_small.h); a call that
 *               meets a larger segment there sets status[0] = -1: NOTHING of its output is valid, call again with the
 *               segment size status[1] reports.  0 or larger: the persistent kernel.
 *               With out_packed = 0 that kernel's (image, class) workgroups also ORDER their class themselves (round 6: no sort
 *               launch; OBB_NMS_SELF_SORT above) and the reported size is the largest class of any image of up to
 *               OBB_NMS_SORT_LDS_MAX candidates; behind the sort kernel an image above OBB_NMS_SORT_LDS_MAX / 2 candidates is
 *               ordered as one list and reported with its whole size.
 *               bit 62      the previous call met boxes with a short side in [0.001, 1) px (status[1] bit 62).  The reference's fp32
 *               clip is ill conditioned for such a box against a partner tens of thousands of pixels away, i.e. across its
 *               cls * max_wh offsets (utils/general.py:849-851), so an image holding one may only keep its per-class NMS segments if
 *               no such pair has IoU > iou_thres.  With the bit set the call checks exactly that (k_tiny_cross: the reference's own
 *               arithmetic on every ill-conditioned cross-class pair; images with at most 64 such boxes and 262,144 box x candidate
 *               combinations: microseconds for the stray sub-pixel box of a trained detector) and keeps the class segments of every
 *               image that passes; without it -- and for an image that fails, is above those bounds, or holds a box whose circle
 *               leaves a 0.95 max_wh window -- the image runs as the reference's single list.  Either way the rows are the reference's.
 *               Apart from the two retry cases the result does not depend on the hint.  The caller's side of all this -- which word to
 *               hand in, which of the retry cases a call ended in, what to keep for the next call of the shape -- is implemented once,
 *               as host code of this library: obb_nms_obb_hints_* below.
 *   out         [bs][max_det][7] fp32 rows [x y l s theta conf cls];  out_count [bs] int64 (-1: device-side abort);
 *               out_packed != 0: the rows of image b start right behind those of image b-1 (row sum(out_count[0..b-1]))
 *               instead of at row b*max_det -- the same buffer size is required, one split instead of bs slices on the host.
 *               out_packed = 0 is the faster form where the small-segment NMS kernel runs (expected_cand, bits 32..60): the rows of an
 *               image do not wait for the counts of the images in front of it, so that kernel writes them itself (csrc/nmsobb_impl.h:
 *               SmallGather) and the call is one launch shorter; obb_val_tail_batch_rows_f32 consumes that layout in place.
 *               status [2] int64: [0] overflow count (see cap_img), or -1 (see expected_cand); [1] largest candidate count of any
 *               image in bits 0..31, largest NMS segment in bits 32..60 (0 where the sort path does not know it), bit 62: an image
 *               held boxes with a sub-pixel short side -- hand these back as expected_cand of the next call of the shape; bit 61
 *               (informational, masked out of the hint): such an image kept its class segments in this call
 *               out_count and status are written with plain 8-byte stores by the last kernel of the call: they may live in
 *               device memory or in pinned host memory (hipHostMalloc) that the caller polls instead of copying back.
 *               What a polled word publishes is the COUNT, nothing else: the kernel that writes out_count[b] / status may still be
 *               storing rows of `out` (of image b and of the images in flight) and reading `ws` at that moment.  `out` is complete and
 *               `ws` is reusable in STREAM ORDER only: a consumer on the call's stream needs nothing more; a consumer on another stream
 *               or on the host records / waits for an event behind the call (or synchronises the stream) before it touches `out` or
 *               hands `ws` to anybody else.  (The bindings of this repository return views of `out` to same-stream consumers and keep
 *               `ws` in a per-stream cache.)
 * Score ties are ordered by ascending (anchor*nc + class): deterministic, where the reference inherits the order
 * of torch's unstable sort.
 * Non-finite inputs (NaN of either sign or payload, +-inf) give what the reference's torch ops give: a row passes the confidence
 * filter iff obj > conf_thres (NaN and -inf fail, +inf passes; conf_thres rounded to the input dtype first); conf = obj * cls in
 * the input dtype (0 * inf = NaN); the best class (multi_label = 0) and the CSL angle bin are the FIRST maximum with every NaN
 * ranked above +inf (torch.max / torch.argmax), so a NaN best confidence drops the row (NaN > conf_thres is false) and a NaN bin is
 * the angle; a box is too small iff min(l, s) < 0.001 with torch.min's NaN propagation (a NaN side keeps the box); NaN / inf
 * coordinates send the image down the single list and reach the NMS unchanged.  The same holds for the _col, _st and _head entries.
 */
#define OBB_NMS_SMALL_SEG 384
#define OBB_NMS_SORT_LDS_HINT 6144
#define OBB_NMS_SORT_LDS_MAX 8192
size_t obb_nms_obb_workspace_bytes(int64_t bs, int64_t cap_img, int64_t nc, int agnostic);
int obb_non_max_suppression_obb(const void* pred, int dtype, int64_t bs, int64_t A, int64_t no, float conf_thres,
                                float iou_thres, const int32_t* classes_host, int n_classes, int agnostic, int multi_label,
                                int64_t max_det, int64_t max_nms, float max_wh, const float* extra8, int64_t n_extra,
                                int64_t cap_img, int64_t expected_cand, float* out, int out_packed, int64_t* out_count,
                                int64_t* status, void* ws, size_t ws_bytes, void* stream);
/* The same call for a `pred` whose producer also stored the objectness column densely: objcol [bs][A] in pred's dtype,
 * objcol[b][i] == pred[b][i][4] bit for bit (obb_detect_decode_col writes it next to z).  The confidence filter
 * (utils/general.py:785 xc = prediction[..., 4] > conf_thres) then reads bs*A elements instead of one 128-byte line of
 * every 400-800-byte row; rows that pass are read from `pred` as before, so the result is the one of the plain call.
 * objcol == NULL is the plain call. */
int obb_non_max_suppression_obb_col(const void* pred, const void* objcol, int dtype, int64_t bs, int64_t A, int64_t no,
                                    float conf_thres, float iou_thres, const int32_t* classes_host, int n_classes, int agnostic,
                                    int multi_label, int64_t max_det, int64_t max_nms, float max_wh, const float* extra8,
                                    int64_t n_extra, int64_t cap_img, int64_t expected_cand, float* out, int out_packed,
                                    int64_t* out_count, int64_t* status, void* ws, size_t ws_bytes, void* stream);

/* The same call with its candidate counters in a buffer of the CALLER's that outlives the call: `state` = obb_nms_obb_state_bytes(bs)
 * bytes of device memory (256-byte aligned), zeroed ONCE by the caller (hipMemset) and then handed to every call with this bs
 * that is ordered on one stream.  Each call finds it zeroed and leaves it zeroed (its last kernel does that), so the call has no
 * reset launch of its own; the filter kernel zeroes the state of the later launches on its way.  At the reference's default
 * thresholds with out_packed = 0 the whole of non_max_suppression_obb is then TWO launches (filter + CSL decode; NMS whose
 * (image, class) workgroups order their own class and write the output rows -- round 6, OBB_NMS_SELF_SORT above; three with the sort
 * kernel between them).  A call that returns an error may leave the buffer dirty: zero it again.  Two calls that are not ordered on one
 * stream need a buffer each.  Everything else as obb_non_max_suppression_obb_col (objcol may be NULL). */
size_t obb_nms_obb_state_bytes(int64_t bs);
int obb_non_max_suppression_obb_st(const void* pred, const void* objcol, int dtype, int64_t bs, int64_t A, int64_t no,
                                   float conf_thres, float iou_thres, const int32_t* classes_host, int n_classes, int agnostic,
                                   int multi_label, int64_t max_det, int64_t max_nms, float max_wh, const float* extra8,
                                   int64_t n_extra, int64_t cap_img, int64_t expected_cand, float* out, int out_packed,
                                   int64_t* out_count, int64_t* status, void* ws, size_t ws_bytes, void* state, size_t state_bytes,
                                   void* stream);

/* The same call fed straight from the Detect head's 1x1-conv outputs instead of `pred`: Detect.forward (models/yolo.py:61-81)
 * followed by non_max_suppression_obb (utils/general.py:772-862) as detect.py and val.py chain them, without the dense prediction
 * tensor z (bs, A, no) and the permuted raw head x in between.
 *   conv_out[l]  level l's conv output (bs, na*no, ny[l], nx[l]), contiguous, dtype OBB_DTYPE_F32 / _F16 / _BF16; nl <= 4, na <=
 *                OBB_LOSS_MAX_ANCHORS, no = 5 + nc + 180 with 1 <= nc <= 256 (the limits of obb_detect_decode_levels and
 *                obb_non_max_suppression_obb)
 *   anchors_px_host HOST [nl][na][2] = Detect.anchors * stride, strides_host HOST [nl]: as obb_detect_decode_levels takes them
 * What is read: per (level, image, anchor) tile of 256 bytes of positions, the objectness line (channel a*no + 4) -- decoded exactly
 * as z[..., 4] and compared with conf_thres in the tensor dtype (:785) -- and, only where some position of the tile passes, the
 * tile's no channel lines, from which the passing rows are decoded with the arithmetic of obb_detect_decode (csrc/detect_math.h)
 * and reduced as the filter kernel of obb_non_max_suppression_obb reduces rows of z.  Every candidate carries the index its row
 * has in z (rows of level l start at sum over the levels before of na*ny*nx, then a*ny*nx + y*nx + x), so the sort keys, the score
 * ties and the kept list are those of the eager chain: the result is bit-identical to obb_detect_decode_levels (z_out) followed by
 * obb_non_max_suppression_obb_st on the same inputs and arguments.
 * Workspace: obb_nms_obb_workspace_bytes(bs, cap_img, nc, agnostic) with A = sum of na*ny[l]*nx[l] -- nothing more.  Output contract,
 * status words, hints and retry cases as obb_non_max_suppression_obb_st; `state` may be NULL (a reset launch zeroes the counters,
 * as in obb_non_max_suppression_obb_col).  Everything before any device call answers OBB_ERR_BAD_ARG for an nl out of range,
 * NULL tables or level pointers, an unknown dtype, nc or na out of range. */
int obb_non_max_suppression_obb_head(int nl, const void* const* conv_out, int dtype, int64_t bs, int64_t na, int64_t no,
                                     const int64_t* ny, const int64_t* nx, const float* anchors_px_host, const float* strides_host,
                                     float conf_thres, float iou_thres, const int32_t* classes_host, int n_classes, int agnostic,
                                     int multi_label, int64_t max_det, int64_t max_nms, float max_wh, const float* extra8,
                                     int64_t n_extra, int64_t cap_img, int64_t expected_cand, float* out, int out_packed,
                                     int64_t* out_count, int64_t* status, void* ws, size_t ws_bytes, void* state, size_t state_bytes,
                                     void* stream);

/* The caller's side of the fused entries (the four above and obb_non_max_suppression_obb_tta_head below), as host code (csrc/nmsobb_hints.h: no device call, no allocation, no state
 * but the struct): the reference implementation of what to do around a call, used by both bindings of this repository.  A caller
 * keeps one obb_nms_obb_hints per input shape (and per thread, device and conf_thres: other batches say nothing about this one's).
 *
 *   obb_nms_obb_hints h;  obb_nms_obb_hints_init(&h);                 once per shape
 *   int64_t cap_img = obb_nms_obb_hints_cap(&h, worst);               per call; worst = A * (multi_label ? nc : 1) + n_extra
 *   for (;;) {
 *     entry(..., cap_img, obb_nms_obb_hints_word(&h), ..., out_count, status, ws sized for cap_img, ...);
 *     ... wait until out_count[0..bs) and status[0..1] are on the host ...
 *     int action = obb_nms_obb_hints_update(&h, &cap_img, worst, out_count, bs, status);
 *     if (action == OBB_HINTS_DONE) break;                            out / out_count are valid; h holds the next call's hints
 *     if (action == OBB_HINTS_RETRY_SMALL_GRID) obb_nms_set_max_grid(8) -- or give up if that was done already
 *   }                                                                 (restore obb_nms_set_max_grid(0) behind the loop)
 *
 * obb_nms_obb_hints_update reads status[1] (bit 62 -> small_boxes, bit 61 -> small_resolved) and then decides, in this order:
 *   status[0] == -1              a segment above OBB_NMS_SMALL_SEG met the small-segment kernel: nothing is valid.  seg = the
 *                                reported segment (at least OBB_NMS_SMALL_SEG + 1), held; OBB_HINTS_RETRY
 *   some out_count[b] < 0        a barrier of the persistent kernel timed out: OBB_HINTS_RETRY_SMALL_GRID, h unchanged otherwise
 *   status[0] > *cap_img         *cap_img = min(worst, max(status[0], 2 * *cap_img)); OBB_HINTS_RETRY (size the workspace again)
 *   a hint in 1 .. OBB_NMS_SORT_LDS_HINT and more than OBB_NMS_SORT_LDS_MAX candidates in an image
 *                                such images were left empty: cand = the reported count, held; OBB_HINTS_RETRY
 *   otherwise                    OBB_HINTS_DONE: cap = *cap_img, cand and seg = what status[1] reports.  A regime that a retry
 *                                of this or an earlier call selected is held for 8 calls -- cand stays above OBB_NMS_SORT_LDS_HINT,
 *                                seg above OBB_NMS_SMALL_SEG -- unless the batch falls 25 % below that limit (a reported segment
 *                                of 0, "not known on this path", does not release it): a stream whose batches hover around a
 *                                limit does not pay the repeat on every other batch.
 * Forcing a hint (cand = 0: the generic sort; seg = 1: the small-segment kernel) is a plain store to the field, with its hold = 0. */
typedef struct obb_nms_obb_hints {
  int64_t cap;                         /* candidate slots per image that sufficed last time (0: none yet)                  */
  int64_t cand, seg;                   /* expected_cand bits 0..31 and 32..60 of the next call                             */
  int64_t hold_cand, hold_seg;         /* calls the larger regime is still held                                            */
  int64_t small_boxes, small_resolved; /* status[1] bits 62 and 61 of the previous call (0 / 1); the first is handed back  */
  int64_t reserved;
} obb_nms_obb_hints;
#define OBB_HINTS_DONE 0
#define OBB_HINTS_RETRY 1
#define OBB_HINTS_RETRY_SMALL_GRID 2
void obb_nms_obb_hints_init(obb_nms_obb_hints* hints_host);
int64_t obb_nms_obb_hints_cap(const obb_nms_obb_hints* hints_host, int64_t worst);
int64_t obb_nms_obb_hints_word(const obb_nms_obb_hints* hints_host);
int obb_nms_obb_hints_update(obb_nms_obb_hints* hints_host, int64_t* cap_img_host, int64_t worst, const int64_t* out_count_host,
                             int64_t bs, const int64_t* status_host);

/* ------------------------------------------------------------------ training loss -------------------- */

/*
 * ComputeLoss of the OBB head (utils/loss.py:90-275): build_targets + box (horizontal CIoU) / objectness / class /
 * CSL-angle losses, forward and backward, for raw head outputs p[i] of shape (bs, na, ny_i, nx_i, no) and the
 * dataloader's target tensor (nt, 7+180) rows [img, cls, cx, cy, l, s, theta, csl x 180] in pixels
 * (utils/datasets.py:637-672) -- or (nt, 7) rows without the labels, see obb_loss_config.csl_radius.  Everything ComputeLoss.__init__ reads from the model (utils/loss.py:93-120) travels
 * in obb_loss_config (host memory, plain C).  obb_loss_config.head_layout = OBB_LOSS_LAYOUT_CONV hands over the 1x1 convs' own
 * outputs (bs, na*no, ny_i, nx_i) instead of the permuted copies, and takes the gradient in that layout (same bits).
 */
#define OBB_LOSS_MAX_LEVELS 8
#define OBB_LOSS_MAX_ANCHORS 8
typedef struct obb_loss_config {
  int32_t nl, na, nc, no, bs;          /* Detect.nl / na / nc / no (= 5 + nc + 180), batch size            */
  int32_t ny[OBB_LOSS_MAX_LEVELS], nx[OBB_LOSS_MAX_LEVELS];     /* p[i].shape[2], p[i].shape[3]             */
  float anchors[OBB_LOSS_MAX_LEVELS][OBB_LOSS_MAX_ANCHORS][2];   /* Detect.anchors (grid units), (l, s)      */
  float stride[OBB_LOSS_MAX_LEVELS];                             /* Detect.stride                            */
  float balance[OBB_LOSS_MAX_LEVELS];                            /* utils/loss.py:114                        */
  float anchor_t;                      /* hyp['anchor_t']                                                   */
  float cp, cn;                        /* smooth_BCE(label_smoothing), utils/loss.py:104                    */
  float cls_pw, theta_pw, obj_pw;      /* BCE pos_weights, utils/loss.py:98-100                             */
  float gain_box, gain_obj, gain_cls, gain_theta;   /* hyp['box'|'obj'|'cls'|'theta'], utils/loss.py:185-188 */
  float gr;                            /* iou ratio, utils/loss.py:116                                      */
  int32_t sort_obj_iou;                /* utils/loss.py:93,156-158                                          */
  float csl_radius;                    /* hyp['csl_radius'] (data/hyps/obb/ yaml files; <= 0: 2.0).  Used only when the target
                                          rows carry no CSL labels (tcols == 7): the 180-bin label is then regenerated on
                                          the device from theta exactly as gaussian_label_cpu rolls its window
                                          (utils/rboxs_utils.py:9-26, utils/datasets.py:639-642) -- SURVEY 8(f) row 3   */
  float fl_gamma;                      /* hyp['fl_gamma']: > 0 wraps the class, angle and objectness BCE in FocalLoss(gamma,
                                          alpha = 0.25) like utils/loss.py:107-110 (35-62); 0: plain BCE                */
  int32_t head_layout;                 /* OBB_LOSS_LAYOUT_*: where obb_loss_forward / _backward find element (b, a, gj, gi, ch) of
                                          p_levels_host[i] and grad_levels_host[i].  A zero-initialised config is the row layout.
                                          Any other value: obb_loss_workspace_bytes answers 0 and the four entries answer
                                          OBB_ERR_BAD_ARG before any device call.  obb_loss_build_targets / _export_targets read
                                          no head tensor: they only check the value.                                          */
} obb_loss_config;
/* (bs, na, ny_i, nx_i, no) contiguous: element at (((b*na + a)*ny_i + gj)*nx_i + gi)*no + ch -- the reference's permuted copy */
#define OBB_LOSS_LAYOUT_ROWS 0
/* (bs, na*no, ny_i, nx_i) contiguous, the 1x1 conv's own output and its gradient: element at
 * ((b*na + a)*no + ch)*ny_i*nx_i + gj*nx_i + gi.  Nothing transposes the head or its gradient (Detect.lazy_train).  loss_out and
 * every gradient element are bit for bit those of OBB_LOSS_LAYOUT_ROWS on the permuted copy of the same data: the kernels keep
 * the row -> thread assignment, the partial sums and the per-cell entry order, only the address of (cell, ch) differs. */
#define OBB_LOSS_LAYOUT_CONV 1

size_t obb_loss_workspace_bytes(const obb_loss_config* cfg, int64_t nt);

/* ComputeLoss.build_targets (utils/loss.py:194-275) into the workspace; counts_out[0..nl) (device, int32) receives
 * the number of matched rows per level and counts_out[OBB_LOSS_MAX_LEVELS] a non-zero flag when a target row names
 * an image or class outside the batch (the reference raises IndexError there).  No host synchronisation.
 * Bad target rows: a row that matches some anchor of some level is bad when its image index (truncated like .long()) is
 * outside [0, bs), its class is negative, or nc > 1 and its class is >= nc.  With nc == 1 the reference never indexes by
 * class (utils/loss.py:163), so any class >= 0 is accepted and the loss is finite.  Negative image or class indices are
 * bad for every nc although torch would wrap them.  A bad row makes loss_out[0] and every gradient NaN. */
int obb_loss_build_targets(const obb_loss_config* cfg, const float* targets, int64_t nt, int64_t tcols, int32_t* counts_out,
                           void* ws, size_t ws_bytes, void* stream);
/* Rows of one level in the reference's order (offset-major, anchor-major, target order), after the caller has read
 * the count n: indices4 [n][4] int64 (b, a, gj, gi); tbox4 [n][4]; anch2 [n][2]; tcls [n] int64; csl180 [n][180]. */
int obb_loss_export_targets(const obb_loss_config* cfg, int64_t nt, int level, int64_t n, int64_t* indices4, float* tbox4,
                            float* anch2, int64_t* tcls, float* csl180, void* ws, size_t ws_bytes, void* stream);

/* ComputeLoss.__call__ forward (utils/loss.py:122-192).  p_levels_host: HOST array of nl device pointers;
 * dtype OBB_DTYPE_F32 / _F16 / _BF16 (arithmetic is fp32 in every case; tobj is rounded to the head dtype as utils/loss.py:155
 * does).  loss_out (device, 5 + nl floats):
 * [0] (lbox+lobj+lcls+ltheta)*bs, [1..4] lbox, lobj, lcls, ltheta (gains applied), [5+i] the un-balanced objectness
 * BCE of level i (what autobalance reads, :180-181).  [0] is NaN when a target row is out of range.
 * Non-finite logits are data: the loss, each item and every gradient element are finite exactly where the reference's are
 * (inf and NaN are not told apart: an infinite objectness logit of a matched cell gives NaN where the reference gives inf).
 * A NaN box logit of a matched cell reaches lbox and, through the cell's objectness target iou.detach().clamp(0) (torch's
 * clamp propagates NaN, argsort under sort_obj_iou ranks it last), lobj and the gradients of the cell's channels 0..4.
 * The workspace keeps the matched rows and (round 5) a dense copy of every anchor row's objectness logit for obb_loss_backward
 * (which then reads 4 contiguous bytes per row instead of one 128-byte line of each 800-byte row): pass the same buffer, untouched.
 * cfg->head_layout = OBB_LOSS_LAYOUT_CONV: p_levels_host[i] is the conv output (bs, na*no, ny_i, nx_i); the objectness logits of an
 * anchor are then one contiguous plane, so no dense copy is kept and the workspace is smaller by that column.  In both layouts
 * every p_levels_host[i] (and grad_levels_host[i] below) must be 16-byte aligned: the kernels use 16-byte accesses from the base. */
int obb_loss_forward(const obb_loss_config* cfg, const void* const* p_levels_host, int dtype, const float* targets, int64_t nt,
                     int64_t tcols, float* loss_out, void* ws, size_t ws_bytes, void* stream);
/* Gradient of loss_out[0] with respect to every p[i], times *grad_scale (device scalar: the incoming dL/dloss, e.g.
 * the GradScaler factor).  grad_levels_host: HOST array of nl device pointers, same shapes / dtype / layout as p (16-byte
 * aligned); every element is written (no prior zero-fill needed).  cfg, p, targets and ws as obb_loss_forward left them.
 * OBB_LOSS_LAYOUT_CONV: the gradient is the conv output's, (bs, na*no, ny_i, nx_i) contiguous -- one linear stream of zeros with
 * the objectness gradient in the planes of channel 4 (k_loss_bwd_dense_conv), then the rows of the matched cells, one strided
 * store per channel.
 * Kernel resources of the conv-layout instantiations (gfx950, -Rpass-analysis=kernel-resource-usage; VGPR for f32 / f16 / bf16;
 * none uses scratch or spills; DESIGN.md 4.8 has the row layout's beside them):
 *   k_loss_dense_fwd<T, 1>      VGPR 40 / 40 / 40     SGPR 72             LDS 32 B   scratch 0
 *   k_loss_entries_fwd<T, 1>    VGPR 94 / 92 / 94     SGPR 103            LDS 0      scratch 0
 *   k_loss_entries_bwd<T, 1>    VGPR 150 / 150 / 150  SGPR 104            LDS 0      scratch 0
 *   k_loss_bwd_dense_conv<T>    VGPR 66 / 70 / 70     SGPR 82 / 98 / 98   LDS 0      scratch 0 */
int obb_loss_backward(const obb_loss_config* cfg, const void* const* p_levels_host, int dtype, const float* targets, int64_t nt,
                      int64_t tcols, const float* grad_scale, void* const* grad_levels_host, void* ws, size_t ws_bytes,
                      void* stream);

/* ------------------------------------------------------------------ Detect head / CSL / box utils ----- */

/*
 * Detect.forward, inference branch, for ONE level (models/yolo.py:61-79): conv_out is the 1x1-conv output
 * (bs, na*no, ny, nx), contiguous, dtype OBB_DTYPE_F32 / _F16 / _BF16.  Writes (either pointer may be NULL)
 *   x_perm_out  (bs, na, ny, nx, no)  the raw head, what `x[i].view(bs,na,no,ny,nx).permute(0,1,3,4,2).contiguous()` returns (:65)
 *   z_out       rows [a_offset, a_offset + na*ny*nx) of every image of the concatenated prediction tensor
 *               (bs, a_total, no): sigmoid, xy = (y*2-0.5+grid)*stride, wh = (y*2)^2*anchor_grid (:71-79),
 *               arithmetic and rounding steps in the tensor dtype exactly as the reference's in-place branch.
 *   anchors_px_host  HOST array [na][2] = Detect.anchors[i] * stride[i] (anchor_grid, :90-91)
 */
int obb_detect_decode(const void* conv_out, int dtype, int64_t bs, int64_t na, int64_t no, int64_t ny, int64_t nx,
                      const float* anchors_px_host, float stride, void* x_perm_out, void* z_out, int64_t a_total,
                      int64_t a_offset, void* stream);
/* obb_detect_decode that also writes objcol_out [bs][a_total] (same dtype) = z[..., 4] of the level's rows: the column the
 * confidence filter of obb_non_max_suppression_obb_col reads.  Any of x_perm_out / z_out / objcol_out may be NULL. */
int obb_detect_decode_col(const void* conv_out, int dtype, int64_t bs, int64_t na, int64_t no, int64_t ny, int64_t nx,
                          const float* anchors_px_host, float stride, void* x_perm_out, void* z_out, int64_t a_total,
                          int64_t a_offset, void* objcol_out, void* stream);

/* The whole inference branch of Detect.forward (models/yolo.py:61-79: the loop over the nl levels and the torch.cat) in ONE
 * launch: conv_out[l] is level l's conv output (bs, na*no, ny[l], nx[l]); x_perm_out[l] its permuted raw head (the array or
 * any entry may be NULL); the levels' rows follow each other in z_out / objcol_out (bs, a_total, ...) in level order, like
 * torch.cat(z, 1).  anchors_px_host HOST [nl][na][2], strides_host HOST [nl].  nl <= 4.  Same bytes as nl calls of
 * obb_detect_decode_col with a_offset = the rows of the levels before. */
int obb_detect_decode_levels(int nl, const void* const* conv_out, int dtype, int64_t bs, int64_t na, int64_t no, const int64_t* ny,
                             const int64_t* nx, const float* anchors_px_host, const float* strides_host, void* const* x_perm_out,
                             void* z_out, int64_t a_total, void* objcol_out, void* stream);

/* Augmented inference (models/yolo.py:149-209: _forward_augment, _descale_pred, _clip_augmented) behind the conv outputs of its
 * passes, in ONE launch: every pass is decoded like obb_detect_decode_levels, its box channels 0..3 are de-scaled and de-flipped,
 * and the rows land where torch.cat(_clip_augmented(y), 1) puts them -- pass after pass, level after level -- in z_out
 * (bs, a_total, no), written once.  objcol_out (bs, a_total) or NULL receives z[..., 4] once more, bit-identical (the column of
 * obb_non_max_suppression_obb_col).  The permuted raw heads are not written (train_out is None under augmentation).
 *   A pass lists only the levels that SURVIVE the clip (the caller drops a clipped level by not listing it: its conv output is
 *   never read); a clip that does not fall on a level boundary cannot be expressed -- use the eager chain there.
 *   conv_out[l] (bs, na*no, ny[l], nx[l]) contiguous, dtype as below; anchors_px[l][a] = Detect.anchors * stride of that level;
 *   scale  the pass's image scale (> 0, finite); flip 0 (none), 2 (up-down) or 3 (left-right), the dims of torch.flip;
 *   img_h, img_w  the UN-scaled input size the de-flip mirrors at.
 * Arithmetic per element, in the tensor dtype with the reference's rounding points: the decode as in obb_detect_decode, rounded;
 * `/= scale` as torch evaluates it for a Python float -- a multiplication with (float)(1.0 / scale), the reciprocal taken once in
 * double and then rounded to fp32 -- rounded
 * (scale == 1 is the identity); flip 3: channel 0 = img_w - x, flip 2: channel 1 = img_h - y, in fp32, rounded.  Channels >= 4
 * are the plain decode.  The result is bit-identical to the eager chain on the same device.
 * Host structs, no workspace.  OBB_ERR_BAD_ARG before any device call for: npass outside 1..OBB_TTA_MAX_PASSES, a pass's nl outside
 * 1..OBB_DETECT_MAX_LEVELS, a flip other than 0 / 2 / 3, a scale <= 0 or not finite, an image size < 1, a NULL z_out / passes /
 * listed conv_out, na > OBB_LOSS_MAX_ANCHORS, no outside 6..441, an unknown dtype, a_total smaller than the rows listed. */
#define OBB_TTA_MAX_PASSES 4
#define OBB_DETECT_MAX_LEVELS 4
typedef struct obb_tta_pass {
  int32_t nl;                                                             /* surviving levels of this pass                  */
  int32_t flip;                                                           /* 0, 2 (up-down) or 3 (left-right)               */
  double scale;                                                           /* the Python float, unrounded                    */
  int32_t img_h, img_w;                                                   /* the un-scaled input                            */
  const void* conv_out[OBB_DETECT_MAX_LEVELS];                            /* DEVICE pointers                                */
  int64_t ny[OBB_DETECT_MAX_LEVELS], nx[OBB_DETECT_MAX_LEVELS];
  float stride[OBB_DETECT_MAX_LEVELS];
  float anchors_px[OBB_DETECT_MAX_LEVELS][OBB_LOSS_MAX_ANCHORS][2];       /* pixels: Detect.anchors[l] * stride[l]          */
} obb_tta_pass;
int obb_detect_decode_tta(int npass, const obb_tta_pass* passes_host, int dtype, int64_t bs, int64_t na, int64_t no, void* z_out,
                          int64_t a_total, void* objcol_out, void* stream);

/* Augmented inference followed by non_max_suppression_obb, fed straight from the passes' conv outputs: obb_detect_decode_tta and
 * obb_non_max_suppression_obb_st as val.py --augment / detect.py --augment chain them, without the dense prediction tensor z
 * (bs, a_total, no) in between -- obb_non_max_suppression_obb_head over (pass, level) entries.
 *   passes_host  as for obb_detect_decode_tta: every pass lists only the levels that SURVIVE the clip, in order; at most
 *                OBB_TTA_MAX_PASSES * OBB_DETECT_MAX_LEVELS = 16 entries.  a_total: the rows of torch.cat(_clip_augmented(y), 1).
 * What is read: per (entry, image, anchor) tile of 256 bytes of positions, the objectness line (channel a*no + 4; the de-scale does
 * not touch it) -- decoded exactly as z[..., 4] and compared with conf_thres in the tensor dtype -- and, only where some position of
 * the tile passes, the tile's no channel lines.  The passing rows are decoded with the arithmetic of obb_detect_decode, their box
 * channels 0..3 de-scaled with (float)(1.0 / scale) and de-flipped with the rounding points of obb_detect_decode_tta
 * (csrc/detect_math.h), and reduced as the filter kernel of obb_non_max_suppression_obb reduces rows of z.  The channel lines of an
 * entry are loaded 16 or 8 bytes at a time when its conv output and its planes (ny*nx elements) lie on such boundaries, element-wise
 * otherwise -- chosen per entry.  Every candidate carries the row it has in the concatenated z (an entry starts at the rows of the
 * entries before it, then a*ny*nx + y*nx + x), so the sort keys, the score ties and the kept list are those of the eager chain: the
 * result is bit-identical to obb_detect_decode_tta (z_out) followed by obb_non_max_suppression_obb_st on the same inputs and arguments.
 * Workspace: ws_size = obb_nms_obb_workspace_bytes(bs, cap_img, nc, agnostic) bytes with A = a_total -- nothing more; ws / ws_size
 * follow the rules of ws / ws_bytes of the other entries (256-byte aligned, OBB_ERR_WORKSPACE before any device call).  Output
 * contract, status words, hints and retry cases as obb_non_max_suppression_obb_st; `state` may be NULL (as in
 * obb_non_max_suppression_obb_head).
 * OBB_ERR_BAD_ARG before any device call (host code, csrc/tta_head_plan.h) for: npass outside 1..OBB_TTA_MAX_PASSES, a pass's nl
 * outside 1..OBB_DETECT_MAX_LEVELS, a flip other than 0 / 2 / 3, a scale <= 0 or not finite, an image size < 1, NULL passes or a NULL
 * listed conv_out, na outside 1..OBB_LOSS_MAX_ANCHORS, nc = no - 185 outside 1..256, an unknown dtype, bs * na > 65535, a_total
 * smaller than the rows listed, a_total * nc past the 32-bit row field of the sort key, more tiles than the grid holds. */
int obb_non_max_suppression_obb_tta_head(int npass, const obb_tta_pass* passes_host, int dtype, int64_t bs, int64_t na, int64_t no,
                                         int64_t a_total, float conf_thres, float iou_thres, const int32_t* classes_host, int n_classes,
                                         int agnostic, int multi_label, int64_t max_det, int64_t max_nms, float max_wh, const float* extra8,
                                         int64_t n_extra, int64_t cap_img, int64_t expected_cand, float* out, int out_packed,
                                         int64_t* out_count, int64_t* status, void* ws, size_t ws_size, void* state, size_t state_bytes,
                                         void* stream);

/* gaussian_label_cpu (utils/rboxs_utils.py:9-26) for n angles at once: out [n][num_class] fp32, evaluated in double. */
int obb_csl_encode_f32(const float* labels, int64_t n, int num_class, double u, double sig, float* out, void* stream);

/* rbox2poly (utils/rboxs_utils.py:106-145) and poly2hbb of the result (:147-181): rows [cx cy l s theta ...] with
 * row_stride >= 5 floats -> poly8 [n][8] and/or hbb4 [n][4] = [xc yc w h] (either may be NULL). */
int obb_rbox2poly_f32(const float* rboxes, int64_t n, int64_t row_stride, float* poly8, float* hbb4, void* stream);

/* ------------------------------------------------------------------ post-NMS tail of val.py --------- */

/* val.py:226-236 for the detections of one image (n,7) [x y l s theta conf cls] in one kernel: pred_poly (n,10),
 * pred_hbb (n,6) in model-input space, pred_polyn (n,10) / pred_hbbn (n,6) in native image space
 * (scale_polys, utils/general.py:636-650: (x - pad_x) / gain, (y - pad_y) / gain).  Any output may be NULL. */
int obb_val_postprocess_f32(const float* det7, int64_t n, float pad_x, float pad_y, float gain, float* poly10, float* hbb6,
                            float* polyn10, float* hbbn6, void* stream);

/* The same tail for ALL images of a batch in two launches (val.py:209-250 is a per-image loop): det7 = the packed (N,7)
 * detections of the batch, image b's rows at [det_off_host[b], det_off_host[b+1]) (bs + 1 host integers, det_off_host[0] = 0,
 * bs <= 64); targets = the batch's labels on the device, (nt, tcols >= 7) rows [img cls cx cy l s theta ...] in pixels of the
 * letterboxed frame (the collate format); img5_host = bs x {pad_x, pad_y, gain, native width, native height} (shapes[si] of
 * val.py).  Label boxes go through rbox2poly -> poly2hbb -> xywh2xyxy -> scale_coords in the reference's order (val.py:238-241).
 * Outputs (device): the four packed arrays of obb_val_postprocess_f32 (any may be NULL) and stats (N, niou + 2) floats: the
 * correct row of process_batch as 0 / 1, then conf, then cls -- val.py:250's tuple in one array, one copy per batch. */
size_t obb_val_tail_batch_workspace_bytes(int64_t n_det, int64_t nt);
int obb_val_tail_batch_f32(const float* det7, const int64_t* det_off_host, int64_t bs, const float* targets, int64_t nt, int64_t tcols,
                           const float* img5_host, const float* iouv, int niou, float* poly10, float* hbb6, float* polyn10,
                           float* hbbn6, float* stats, void* ws, size_t ws_bytes, void* stream);
/* The same, for a caller that does not want to copy `stats` back and wait for the stream: `stats` and `done` point into PINNED
 * HOST memory (hipHostMalloc: the device writes through the same pointers); `done` receives n (the number of detections) once
 * every row of `stats` is visible to the host -- the caller sets it to a negative value before the call and polls it. */
int obb_val_tail_batch_polled_f32(const float* det7, const int64_t* det_off_host, int64_t bs, const float* targets, int64_t nt,
                                  int64_t tcols, const float* img5_host, const float* iouv, int niou, float* poly10, float* hbb6,
                                  float* polyn10, float* hbbn6, float* stats, void* ws, size_t ws_bytes, void* stream, int64_t* done);
/* The same for detections that are NOT packed: image b's rows are det7[det_row_host[b] .. det_row_host[b] + det_off_host[b+1] -
 * det_off_host[b]) (bs host integers, rows of 7 floats from det7) -- the layout obb_non_max_suppression_obb writes with
 * out_packed = 0 (det_row_host[b] = b * max_det), consumed where it lies.  Every OUTPUT stays packed by det_off_host.  done may be
 * NULL (then the caller waits for the stream), else as above. */
int obb_val_tail_batch_rows_f32(const float* det7, const int64_t* det_row_host, const int64_t* det_off_host, int64_t bs, const float* targets,
                                int64_t nt, int64_t tcols, const float* img5_host, const float* iouv, int niou, float* poly10, float* hbb6,
                                float* polyn10, float* hbbn6, float* stats, void* ws, size_t ws_bytes, void* stream, int64_t* done);

/* process_batch (val.py:69-90): detections (n,6) [x1 y1 x2 y2 conf cls], labels (m,5) [cls x1 y1 x2 y2], iouv (niou) on the
 * device -> correct (n, niou) bytes (0/1).  No device->host round trip (the reference sorts the matches with numpy). */
size_t obb_process_batch_workspace_bytes(int64_t n, int64_t m);
int obb_process_batch_f32(const float* det6, int64_t n, const float* lab5, int64_t m, const float* iouv, int niou, uint8_t* correct,
                          void* ws, size_t ws_bytes, void* stream);

/* process_batch with the ROTATED IoU -- the oriented-box mAP, which val.py can only reach offline through DOTA_devkit:
 * val.py:69-90 with box_iou(labels, detections) replaced by single_box_iou_rotated<float>(label [cx cy l s theta], detection
 * [cx cy l s theta]), the label FIRST: iou[l][d] is the value obb_rotated_iou_pairs_f32(a5 = label, b5 = detection) returns, bit
 * for bit.  Both boxes are taken in the letterboxed frame as the rows carry them (the rotated IoU is invariant under scale_polys'
 * uniform gain and shift: no pad, gain or clip is applied, and none of its rounding).  A pair is a candidate iff the classes are
 * equal as floats and iou >= iouv[0] (NON-strict, unlike the NMS; a NaN IoU is never a candidate); a detection keeps its candidate
 * of highest IoU, equal IoUs to the lower label row; a label keeps the lowest-indexed detection of its image that kept it;
 * correct[d][k] = won && iou >= iouv[k].  The exact clip is skipped only for pairs PROVED to lie below iouv[0], which needs
 * iouv[0] > 0; with iouv[0] <= 0 every pair of equal class is clipped.
 *   obb_process_batch_obb_f32   one image: det7 (n,7) [cx cy l s theta conf cls], lab6 (m,6) [cls cx cy l s theta] -> correct
 *                               (n, niou) bytes 0 / 1
 *   obb_val_tail_batch_obb_f32  all images of a batch (bs <= 64) on the inputs of obb_val_tail_batch_rows_f32: det7 packed by
 *                               det_off_host (det_row_host NULL) or at det_row_host[b]; targets (nt, tcols >= 7) -> stats
 *                               (N, niou + 2) rows [correct as 0 / 1, conf, cls], packed by det_off_host
 *   match_label [n] int32       the row of lab6 / targets the detection kept, or -1 -- set whether or not it won the label
 *   match_iou   [n] float       that label's IoU, or -1.  Both arrays are REQUIRED: they are the state between the two launches
 *                               (there is no workspace), and what an angle-error statistic needs.
 * iouv: niou (1..16) device floats.  Stream-ordered, no synchronisation; the argument checks (bs outside 1..64, niou outside
 * 1..16, tcols < 7, a NULL required pointer, inconsistent offsets) answer OBB_ERR_BAD_ARG before any device call and leave the
 * outputs untouched.  n == 0: OBB_OK, no launch.  m == 0 / nt == 0: correct all 0, match_label -1, match_iou -1. */
int obb_process_batch_obb_f32(const float* det7, int64_t n, const float* lab6, int64_t m, const float* iouv, int niou, uint8_t* correct,
                              int32_t* match_label, float* match_iou, void* stream);
int obb_val_tail_batch_obb_f32(const float* det7, const int64_t* det_row_host, const int64_t* det_off_host, int64_t bs, const float* targets,
                               int64_t nt, int64_t tcols, const float* iouv, int niou, float* stats, int32_t* match_label, float* match_iou,
                               void* stream);

/* ConfusionMatrix.process_batch (utils/metrics.py:117-163) on the device, one launch per batch, one workgroup per image.
 * Per image: detections with conf > conf_thres (strict; NaN fails) against the labels; a pair is a candidate iff box_iou >
 * iou_thres (strict, float32; both thresholds are taken as float32, as torch compares a float32 tensor with a Python scalar).
 * TIE RULE (the reference's numpy argsort leaves equal IoUs in an unspecified order; pinned here to the reference's own lines with
 * every argsort stable): each kept detection chooses its candidate label of highest IoU, ties to the HIGHER label index; each
 * label keeps, among the detections that chose it, the one of highest IoU, ties to the HIGHER detection index (indices = positions
 * in the image's own lists).  Then, as the reference: a label with a winner d adds 1 to matrix[cls_d][cls_l] whether or not the
 * classes agree, a label without one to matrix[nc][cls_l]; a kept detection that won no label adds 1 to matrix[cls_d][nc], but
 * only in an image with at least one match.  Only images with at least one detection row AND one label take part (val.py:217-246).
 *   matrix_i64  (nc + 1)^2 + 1 device int64, row-major [predicted][true]; ACCUMULATED into, never zeroed by the call.  The last
 *               element counts the cells that could not be taken because a class, truncated like .int(), lies outside [0, nc)
 *               (the reference raises IndexError or wraps a negative index); such a row still takes part in the matching.
 *   1 <= nc <= 32767.  An LDS histogram per workgroup when (nc + 1)^2 <= 12100 (nc <= 109), global atomics per count above.
 *   Per-image counts up to 32767 are the contract (the reference's astype(np.int16) wrap above that is not reproduced).
 * obb_confusion_batch_f32 takes the inputs of obb_val_tail_batch_f32 (bs <= 64, packed det7, targets, img5_host) and computes
 * the same boxes (pred_hbbn, the label boxes), so both run back to back on the same arrays.  obb_confusion_process_batch_f32 is
 * the reference's per-image signature on boxes already computed: det6 (n,6) [x1 y1 x2 y2 conf cls], lab5 (m,5) [cls x1 y1 x2 y2].
 * Stream-ordered, no synchronisation; the argument checks answer before any device call; no detections or no labels: OBB_OK,
 * no launch.  The workspace (obb_confusion_workspace_bytes of the call's n and nt / m) is linear in both. */
size_t obb_confusion_workspace_bytes(int64_t n_det, int64_t nt);
int obb_confusion_batch_f32(const float* det7, const int64_t* det_off_host, int64_t bs, const float* targets, int64_t nt, int64_t tcols,
                            const float* img5_host, int nc, float conf_thres, float iou_thres, int64_t* matrix_i64, void* ws,
                            size_t ws_bytes, void* stream);
int obb_confusion_process_batch_f32(const float* det6, int64_t n, const float* lab5, int64_t m, int nc, float conf_thres, float iou_thres,
                                    int64_t* matrix_i64, void* ws, size_t ws_bytes, void* stream);

/* ap_per_class (utils/metrics.py:21-114, compute_ap method 'interp') over statistics that stay on the device.  stats = n rows
 * [correct x niou as 0 / 1, conf, cls] with row_stride >= niou + 2 floats -- the rows obb_val_tail_batch_f32 writes; target_cls =
 * the class of every label (m floats).  Class ids are integers 0 .. nc_max - 1, nc_max <= 256; 1 <= niou <= 16; n, m < 2^31 - 1.
 * ORDER: conf descending, ties by ascending row index (np.argsort(-conf, kind='stable')) -- this library's rule: the
 * reference's order among ties is whatever numpy's introsort leaves.  All arithmetic is double, in numpy's operation order.
 * Outputs (device), dense by class id -- the host keeps the classes with counts[0][c] > 0 (np.unique(target_cls)):
 *   ap      [nc_max][niou]
 *   prf     [nc_max][5]        p, r, f1, tp, fp at the best F1 index
 *   counts  [2][nc_max]        labels per class, predictions per class
 *   info    [4]                best F1 index (first argmax of the class-mean F1 over px), true positives at IoU column 0,
 *                              1 when a class value of either array is not an integer in [0, nc_max), 1 when a conf is NaN
 *                              (the results are then unspecified)
 *   curves  [3][nc_max][1000]  p, r, f1 over px = linspace(0, 1, 1000); may be NULL
 * A class with labels and no predictions keeps zero rows; a predicted class without labels is ignored.  Stream-ordered, no
 * synchronisation; the argument checks answer before any device call.  The workspace is linear in n. */
size_t obb_ap_per_class_workspace_bytes(int64_t n, int niou, int nc_max);
int obb_ap_per_class_f32(const float* stats, int64_t row_stride, int64_t n, int niou, const float* target_cls, int64_t m, int nc_max,
                         double* ap, double* prf, int32_t* counts, int32_t* info, double* curves, void* ws, size_t ws_bytes,
                         void* stream);

/*
 * Merge of the validation statistics of several ranks into GLOBAL IMAGE ORDER (csrc/stats_merge.h): sharded validation gives
 * every rank the rows of its own images, image after image; ap_per_class orders equal confidences by ascending row index of the
 * rows in image order, so the ranks' rows must be interleaved image by image, not concatenated rank by rank.
 *   src                  one device buffer of `world` runs: run r starts at row r * run_stride and holds rows_per_run_host[r]
 *                        (<= run_stride) rows of src_stride >= width floats, the images of the run back to back
 *   counts, img_id       (world, max_images_per_run) int32 / int64 device, rank-major: rows and global id of the j-th image of run r
 *                        at [r * max_images_per_run + j], j < images_per_run_host[r] (<= max_images_per_run); the padding is not read
 *   n_images_total       ids are 0 .. n_images_total - 1; an id no run supplies is an image with no rows
 *   dst                  dst_rows rows of dst_stride >= width floats: image 0's rows, image 1's rows, ...; the first `width` floats
 *                        of the first info[1] rows are written and NOTHING else (not the gap of a wider stride, not a row behind)
 *   counts_out           (n_images_total) int32 device or NULL: rows of every image, by id
 *   info                 (4) int32 device.  [1] the total number of rows.  [0] != 0: the call copied NOTHING, dst is as it was:
 *                        bit 0 an id outside [0, n_images_total); bit 1 an id supplied twice ([2] is one such id); bit 2 the counts
 *                        of a run do not add up to rows_per_run_host[r], or one is negative ([3] is one such run); bit 3 the
 *                        total exceeds dst_rows
 * The same entry merges the rows and the oriented-box rows (width niou + 2) and, with the per-image LABEL counts, target_cls
 * (width 1).  Plain launches on `stream`, nothing is read back; the copy runs one wave per image with its lanes along the
 * image's contiguous floats.  Before any device call: OBB_ERR_BAD_ARG for a NULL info / host array (src, counts, img_id, dst when
 * there is something to read or write), world < 1, width < 1, a stride < width, a run longer than run_stride, more images in a run
 * than max_images_per_run, n_images_total or the rows of all runs >= 2^31 - 1; OBB_ERR_WORKSPACE for a NULL, misaligned or short
 * ws (obb_stats_merge_workspace_bytes(n_images_total), linear in it).
 */
size_t obb_stats_merge_workspace_bytes(int64_t n_images_total);
int obb_stats_merge_f32(const float* src, int64_t src_stride, int64_t run_stride, const int64_t* rows_per_run_host, const int32_t* counts,
                        const int64_t* img_id, int64_t max_images_per_run, const int64_t* images_per_run_host, int64_t world,
                        int64_t n_images_total, int64_t width, float* dst, int64_t dst_stride, int64_t dst_rows, int32_t* counts_out,
                        int32_t* info, void* ws, size_t ws_cap, void* stream);

/* ------------------------------------------------------------------ pairwise IoU --------------------- */

/* out[i] = IoU(a5[i], b5[i]); the device function behind the NMS
 * (single_box_iou_rotated<float>, utils/nms_rotated/src/box_iou_rotated_utils.h:333-360). */
int obb_rotated_iou_pairs_f32(const float* a5, const float* b5, int64_t n, float* out, void* stream);
/* out[i*k + j] = IoU(a5[i], b5[j]).  One workgroup per 64 x 64 tile, the row tiles on the grid's y axis: n <= 65535 * 64 =
 * 4,194,240 rows (k is not limited by the grid); a larger n returns OBB_ERR_BAD_ARG and launches nothing -- split the rows. */
int obb_rotated_iou_matrix_f32(const float* a5, int64_t n, const float* b5, int64_t k, float* out, void* stream);
/* out[i*k + j] = quad IoU of rows (first 8 floats used) -- devPolyIoU, utils/nms_rotated/src/poly_nms_cuda.cu:122-142.
 * Entries the two proved cone rules of csrc/piou_device.h vouch for are written as the exact +0 the clip would return. */
int obb_quad_iou_matrix_f32(const float* a, int64_t a_stride, int64_t n, const float* b, int64_t b_stride, int64_t k,
                            float* out, void* stream);
/* Dense IoU matrix of rboxes through RotBox2Poly + devPolyIoU: the overlaps_kernel of
 * DOTA_devkit/poly_nms_gpu/poly_overlaps_kernel.cu:280-353 on device pointers. */
int obb_rbox_overlaps_f32(const float* boxes5, int64_t n, const float* query5, int64_t k, float* out, void* stream);

/* ------------------------------------------------------------------ devkit host-pointer API ---------- */

/* Same symbols, argument order and host-pointer convention as the reference's devkit
 * (DOTA_devkit/poly_nms_gpu/poly_nms.hpp:9-10, poly_overlaps.hpp:1); synchronous.  The reference declares the two
 * functions with C++ linkage: the library also exports them under the mangled names a build of the reference's Cython
 * sources binds (_Z9_poly_nmsPiS_PKfiifi, _Z9_overlapsPfPKfS1_iii).  tests/test_devkit_binding.py calls both spellings through
 * ctypes, and oracle/ref_shim_devkit.cpp -- a translation unit that includes the reference's own poly_nms.hpp / poly_overlaps.hpp
 * -- is linked against this library by oracle/Makefile and driven like poly_nms.pyx:9-24 / poly_overlaps.pyx:7-12. */
void _poly_nms(int* keep_out_host, int* num_out_host, const float* polys_host, int polys_num, int polys_dim,
               float nms_overlap_thresh, int device_id);
void _overlaps(float* overlaps_host, const float* boxes_host, const float* query_boxes_host, int n, int k, int device_id);

#ifdef __cplusplus
}
#endif
#endif /* OBB_HIP_H */
