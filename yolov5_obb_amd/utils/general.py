"""Mirror of the OBB part of the reference's ``utils/general.py``: ``non_max_suppression_obb``
(utils/general.py:772-862), backed by ONE call into libobb_hip.so for the whole batch
(``obb_non_max_suppression_obb``, include/obb_hip.h) instead of a per-image loop of small ATen
kernels, host syncs and a device->host mask copy.
"""
import ctypes as C
import threading
import time

import torch

from .. import _lib
from ..lazy import LazyTensor

pi = 3.141592  # utils/general.py:34 (truncated on purpose: it is the constant the labels were encoded with)

_MAX_WH = 4096      # utils/general.py:793
_PENDING = -(1 << 62)
_POLL_SECONDS = 2e-3  # busy-poll this long (a bs16 step is ~0.2 ms), then yield the GIL between polls, then give up polling
_POLL_GIVE_UP = 1.0   # ... after this many seconds: fall back to a stream synchronise
_MAX_NMS = 30000    # utils/general.py:794
_CSL = 180          # utils/general.py:784
_ws_memo = {}       # (device index, bs, cap, nc, agnostic, grid capped) -> workspace bytes (a ctypes call saved per batch)
_meta_memo = {}     # (device index, bs, thread) -> the int64 buffer the counters are read back from
_SEG_SMALL = 384    # include/obb_hip.h OBB_NMS_SMALL_SEG: the one-workgroup-per-segment kernel of csrc/nms_small.h takes segments up to this size
_HINTS_DONE, _HINTS_RETRY, _HINTS_RETRY_SMALL_GRID = 0, 1, 2   # include/obb_hip.h OBB_HINTS_*: what obb_nms_obb_hints_update answers
_MAX_SHAPES = 512   # thread churn or a swept threshold must not grow a thread's hints without bound
_tls = threading.local()   # .hints: (device, A, nc, multi_label, conf_thres) -> _lib.NmsObbHints of the calling thread: what its earlier
                           # calls of that shape learned (include/obb_hip.h: obb_nms_obb_hints); other threads' batches say nothing about it


def _hints_of(key, make=True):
    hints = getattr(_tls, "hints", None)
    if hints is None:
        hints = _tls.hints = {}
    h = hints.get(key)
    if h is None and make:
        if len(hints) >= _MAX_SHAPES:         # hints only: forgetting them costs the next call of every shape one repeated call at most
            hints.clear()
        h = hints[key] = _lib.NmsObbHints()
        _lib.lib().obb_nms_obb_hints_init(C.byref(h))
    return h


def _key(device, A, nc, multi, conf_thres):
    idx = torch.device(device).index
    return (torch.cuda.current_device() if idx is None else idx, int(A), int(nc), bool(multi), float(conf_thres))


def hints_clear():
    """Forget what the calling thread's earlier calls learned about their shapes (tests, tools)."""
    _tls.hints = {}
    ext = _lib.compiled()
    if ext is not None:
        ext.hints_clear()


def hint_get(device, A, nc, multi_label, conf_thres):
    """The hint state of a shape on the active binding (the fields of obb_nms_obb_hints, include/obb_hip.h):
    dict(cap=, cand=, seg=, hold_cand=, hold_seg=, small_boxes=, small_resolved=) or None."""
    key = _key(device, A, nc, multi_label, conf_thres)
    ext = _lib.compiled()
    if ext is not None:
        return ext.hint_get(*key)
    h = _hints_of(key, make=False)
    if h is None:
        return None
    return {"cap": h.cap, "cand": h.cand, "seg": h.seg, "hold_cand": h.hold_cand, "hold_seg": h.hold_seg,
            "small_boxes": bool(h.small_boxes), "small_resolved": bool(h.small_resolved)}


def hint_set(device, A, nc, multi_label, conf_thres, cand=None, seg=None):
    """Force the hints of the next call of a shape (cand = 0: the generic sort; seg = 1: the small-segment kernel)."""
    key = _key(device, A, nc, multi_label, conf_thres)
    ext = _lib.compiled()
    if ext is not None:
        ext.hint_set(*key, -1 if cand is None else int(cand), -1 if seg is None else int(seg))
        return
    h = _hints_of(key)
    if cand is not None:
        h.cand, h.hold_cand = int(cand), 0
    if seg is not None:
        h.seg, h.hold_seg = int(seg), 0


def _label_rows(labels, bs, nc, device):
    """Apriori labels for autolabelling (utils/general.py:807-813) as candidate rows [img, x, y, l, s, theta, conf, cls]:
    obj = 1, one-hot class = 1 -> conf = 1; the CSL part of such a row is all zeros -> arg-max bin 0 -> theta = -90/180*pi."""
    rows = []
    theta0 = torch.tensor((0 - 90) / 180, dtype=torch.float32).mul(pi).item()
    for b in range(bs):
        if b < len(labels) and len(labels[b]):
            lb = labels[b].to(device=device, dtype=torch.float32)
            r = torch.zeros((lb.shape[0], 8), device=device, dtype=torch.float32)
            r[:, 0] = b
            r[:, 1:5] = lb[:, 1:5]
            r[:, 5] = theta0
            r[:, 6] = 1.0
            r[:, 7] = lb[:, 0].long().float()
            rows.append(r)
    return torch.cat(rows, 0).contiguous() if rows else None


def _objectness_column(prediction, pred):
    """The dense copy of prediction[..., 4] that this package's Detect hangs on its output (models/yolo.py), or None.
    Only trusted for the very tensor object Detect returned, unchanged since: same object (the attribute lives on it), same
    version counter (any in-place write through the tensor or a view of it bumps it), same geometry."""
    tag = getattr(prediction, "_obb_objcol", None)
    if tag is None or pred is not prediction:
        return None
    col, version = tag
    try:
        current = prediction._version      # inference tensors (torch.inference_mode) track no version: nothing to trust
    except RuntimeError:
        return None
    if (version != current or not isinstance(col, torch.Tensor) or col.shape != prediction.shape[:2]
            or col.dtype != prediction.dtype or col.device != prediction.device or not col.is_contiguous()):
        return None
    return col


def non_max_suppression_obb(prediction, conf_thres=0.25, iou_thres=0.45, classes=None, agnostic=False, multi_label=False,
                            labels=(), max_det=1500):
    """Runs Non-Maximum Suppression (NMS) on inference results_obb (utils/general.py:772-862).

    Args:
        prediction (tensor): (b, n_all_anchors, [cx cy l s obj num_cls theta_cls]), fp32, fp16 or bf16, on the GPU
        agnostic (bool): True = NMS will be applied between elements of different categories
        labels : () or per-image apriori labels (n, [cls x y l s]) for autolabelling
    Returns:
        list of detections, len=batch_size, on (n,7) tensor per image [xylsθ, conf, cls] θ ∈ [-pi/2, pi/2)
    """
    head = None
    if isinstance(prediction, LazyTensor):
        # Detect.lazy_nms / lazy_tta: never touched -> the fused entry on the conv outputs; materialised -> the real tensor, plain path
        head = prediction.payload
        if head is None:
            prediction = prediction.materialize()
        else:
            head.check()
    _lib.require_cuda(prediction, "prediction")
    if prediction.dim() != 3:
        raise RuntimeError(f"prediction must be (bs, anchors, no), got {tuple(prediction.shape)}")
    nc = prediction.shape[2] - 5 - _CSL  # number of classes
    # Checks (same asserts as the reference, :789-790)
    assert 0 <= conf_thres <= 1, f'Invalid Confidence threshold {conf_thres}, valid values are between 0.0 and 1.0'
    assert 0 <= iou_thres <= 1, f'Invalid IoU {iou_thres}, valid values are between 0.0 and 1.0'
    if nc < 1 or nc > 256:
        raise RuntimeError(f"non_max_suppression_obb: 1 <= nc <= 256 supported, got nc = {nc}")
    dtype = _lib.dtype_code(prediction, "non_max_suppression_obb")
    pred = prediction.contiguous()
    bs, A, no = pred.shape
    dev = pred.device
    col = _objectness_column(prediction, pred) if head is None else None
    multi = bool(multi_label) and nc > 1
    if bs == 0:
        return []
    if A == 0:
        return [torch.zeros((0, 7), device=dev)] * bs

    extra = _label_rows(labels, bs, nc, dev) if labels else None
    ext = _lib.compiled()
    if ext is not None:
        # the compiled binding (csrc/torch_ext/nms_rotated_ext.cpp): the call loop of _run_fused below, in C++
        cl = None
        if classes is not None:
            cl = [int(c) for c in (classes if isinstance(classes, (list, tuple)) else list(classes))]
        if head is not None and getattr(head, "tta", False):       # models/yolo.py LazyTtaHead: the passes of augmented inference
            convs, scales, flips, apx, strd = (list(v) for v in zip(*head.pass_lists()))
            return ext.non_max_suppression_obb_tta_head(convs, scales, flips, apx, strd, head.img_h, head.img_w, head.na, head.a_total,
                                                        float(conf_thres), float(iou_thres), cl, bool(agnostic), multi, extra, int(max_det))
        if head is not None:
            return ext.non_max_suppression_obb_head(head.convs, head.anchor_px, head.strides, float(conf_thres), float(iou_thres), cl,
                                                    bool(agnostic), multi, extra, int(max_det))
        return ext.non_max_suppression_obb(pred, float(conf_thres), float(iou_thres), cl, bool(agnostic), multi, extra, int(max_det), col)
    n_extra = 0 if extra is None else extra.shape[0]
    cls_arr = None
    if classes is not None:
        cl = [int(c) for c in (classes if isinstance(classes, (list, tuple)) else list(classes))]
        cls_arr = (C.c_int32 * max(1, len(cl)))(*cl)
        n_cls = len(cl)
        if n_cls == 0:
            return [torch.zeros((0, 7), device=dev)] * bs
    else:
        n_cls = 0

    L = _lib.lib()
    max_det = int(max_det)
    cls_p = C.cast(cls_arr, C.c_void_p) if cls_arr is not None else C.c_void_p(0)
    agn = int(bool(agnostic))
    if head is None:
        def launch(cap, hint_word, out, counts, status, ws, st):
            return L.obb_non_max_suppression_obb_col(
                _lib.ptr(pred), _lib.ptr(col), dtype, bs, A, no, float(conf_thres), float(iou_thres), cls_p, n_cls, agn, int(multi),
                max_det, _MAX_NMS, float(_MAX_WH), _lib.ptr(extra), n_extra, cap, hint_word, out, 1, counts, status, _lib.ptr(ws), ws.numel(), C.c_void_p(st))
    elif getattr(head, "tta", False):
        passes = head.passes()
        passes_p = C.cast(passes, C.c_void_p)

        def launch(cap, hint_word, out, counts, status, ws, st):
            return L.obb_non_max_suppression_obb_tta_head(
                len(passes), passes_p, dtype, bs, head.na, no, A, float(conf_thres), float(iou_thres), cls_p, n_cls,
                agn, int(multi), max_det, _MAX_NMS, float(_MAX_WH), _lib.ptr(extra), n_extra, cap, hint_word, out, 1, counts, status,
                _lib.ptr(ws), ws.numel(), None, 0, C.c_void_p(st))
    else:
        nl = head.nl
        conv_arr = (C.c_void_p * nl)(*[c.data_ptr() for c in head.convs])
        ny_arr = (C.c_int64 * nl)(*[c.shape[2] for c in head.convs])
        nx_arr = (C.c_int64 * nl)(*[c.shape[3] for c in head.convs])
        px_arr = (C.c_float * len(head.anchor_px))(*head.anchor_px)
        st_arr = (C.c_float * nl)(*head.strides)

        def launch(cap, hint_word, out, counts, status, ws, st):
            return L.obb_non_max_suppression_obb_head(
                nl, conv_arr, dtype, bs, head.na, no, ny_arr, nx_arr, px_arr, st_arr, float(conf_thres), float(iou_thres), cls_p, n_cls,
                agn, int(multi), max_det, _MAX_NMS, float(_MAX_WH), _lib.ptr(extra), n_extra, cap, hint_word, out, 1, counts, status,
                _lib.ptr(ws), ws.numel(), None, 0, C.c_void_p(st))
    return _run_fused(launch, dev, bs, A, nc, multi, conf_thres, n_extra, agn, max_det)


def _run_fused(launch, dev, bs, A, nc, multi, conf_thres, n_extra, agn, max_det):
    """The ctypes binding's call loop around one fused entry (launch: obb_non_max_suppression_obb_col, _head or _tta_head): workspace,
    polled counters, and the shape's hints and retries as the library decides them (include/obb_hip.h: obb_nms_obb_hints_*)."""
    L = _lib.lib()
    worst = A * (nc if multi else 1) + n_extra
    h = _hints_of((dev.index, A, nc, multi, float(conf_thres)))          # (_key of a tensor's device, spelled out)
    hints = C.addressof(h)
    cap = C.c_int64(L.obb_nms_obb_hints_cap(hints, worst))               # obb_nms_obb_hints_update may raise it: in / out
    cap_p = C.addressof(cap)                                              # (plain addresses: the cheapest arguments ctypes takes)
    out = torch.empty((bs * max_det, 7), dtype=torch.float32, device=dev)   # packed: image b's rows follow image b-1's
    mkey = (dev.index, bs, threading.get_ident())
    meta = _meta_memo.get(mkey)                                       # counts[bs] + status[2]: read back before returning,
    if meta is None:                                                  # never handed out -> one buffer per (device, bs, thread)
        # Pinned host memory the last kernel writes straight into (the device reaches it through the same pointer), polled
        # by this thread: no copy kernel, no wake-up of a blocked stream wait.  (Device memory + one blocking copy: 0.254 ms
        # per bs16 step; pinned memory + stream synchronise: 0.282 ms.)
        meta = torch.empty(bs + 2, dtype=torch.int64).pin_memory()
        _meta_memo[mkey] = meta = (meta, meta.numpy())
    meta, meta_np = meta
    counts_p = meta.data_ptr()
    status_p = counts_p + 8 * bs
    capped = False                # obb_nms_set_max_grid is per calling thread (thread_local in the library): no other thread sees it
    try:
        while True:
            meta_np.fill(_PENDING)
            with _lib.guard(dev):
                st = _lib.stream_handle(dev)
                wkey = (dev.index, bs, cap.value, nc, agn, capped)    # (the library sizes the workspace from the current device's CUs and the calling thread's grid cap)
                nbytes = _ws_memo.get(wkey)
                if nbytes is None:
                    nbytes = _ws_memo[wkey] = L.obb_nms_obb_workspace_bytes(bs, cap.value, nc, agn)
                ws = _lib.workspace(nbytes, dev, st)
                rc = launch(cap.value, L.obb_nms_obb_hints_word(hints), _lib.ptr(out), counts_p, status_p, ws, st)
            _lib.check(rc, "obb_non_max_suppression_obb")
            t_poll = time.perf_counter()                              # every entry is one aligned 8-byte store of the last kernel
            while meta_np.min() == _PENDING:
                waited = time.perf_counter() - t_poll
                if waited > _POLL_GIVE_UP:                            # something is badly wrong, or a very long call
                    _lib.stream_sync(dev)
                    break
                if waited > _POLL_SECONDS:                            # the stream still holds earlier work (the model's forward):
                    time.sleep(0)                                     # let other Python threads (DataLoader, pin-memory) run
            action = L.obb_nms_obb_hints_update(hints, cap_p, worst, counts_p, bs, status_p)
            if action == _HINTS_DONE:
                break
            if action == _HINTS_RETRY_SMALL_GRID:                     # a team barrier of the NMS kernel timed out
                if capped:
                    _lib.checked_count(int(meta_np[:bs].min()), "obb_non_max_suppression_obb")
                capped = True
                L.obb_nms_set_max_grid(8)                             # once more with a grid that is resident under any CU mask
    finally:
        if capped:
            L.obb_nms_set_max_grid(0)
    counts = meta_np[:bs].tolist()
    return list(out.narrow(0, 0, sum(counts)).split_with_sizes(counts))     # one call instead of bs slicing ops
