"""Mirror of the per-image tail of the reference's ``val.py``: what runs for every image right
after ``non_max_suppression_obb`` -- ``rbox2poly`` -> ``poly2hbb`` -> ``xywh2xyxy`` -> ``scale_polys`` (val.py:226-236) and
``process_batch`` (val.py:69-90) -- as two fused launches of libobb_hip.so instead of ~15 small ATen kernels and a
``.cpu().numpy()`` round trip per image."""
import threading

import torch

from . import _lib, stats_merge
from .tail_batch import MAX_BS, TailBatch, as_f32, box_arrays, split_rows


def val_postprocess(pred, ratio_pad=None, img1_shape=None, img0_shape=None):
    """pred (n,7) [x y l s theta conf cls] (CUDA) -> pred_poly (n,10), pred_hbb (n,6), pred_polyn (n,10), pred_hbbn (n,6).

    ratio_pad = ((h_ratio, w_ratio), (pad_w, pad_h)) as val.py passes it (shapes[si][1]); when None it is derived from the
    two shapes exactly like utils/general.py:639-641."""
    _lib.require_cuda(pred, "pred")
    if pred.dim() != 2 or pred.shape[1] != 7:
        raise RuntimeError(f"val_postprocess: pred must be (n,7), got {tuple(pred.shape)}")
    if ratio_pad is None:
        gain = min(img1_shape[0] / img0_shape[0], img1_shape[1] / img0_shape[1])
        pad = (img1_shape[1] - img0_shape[1] * gain) / 2, (img1_shape[0] - img0_shape[0] * gain) / 2
    else:
        gain, pad = ratio_pad[0][0], ratio_pad[1]
    p = pred.to(torch.float32).contiguous()
    n, dev = p.shape[0], p.device
    poly = torch.empty((n, 10), dtype=torch.float32, device=dev)
    hbb = torch.empty((n, 6), dtype=torch.float32, device=dev)
    polyn = torch.empty((n, 10), dtype=torch.float32, device=dev)
    hbbn = torch.empty((n, 6), dtype=torch.float32, device=dev)
    with _lib.guard(dev):
        rc = _lib.lib().obb_val_postprocess_f32(_lib.ptr(p), n, float(pad[0]), float(pad[1]), float(gain), _lib.ptr(poly), _lib.ptr(hbb),
                                                _lib.ptr(polyn), _lib.ptr(hbbn), _lib.stream_ptr(dev))
    _lib.check(rc, "obb_val_postprocess_f32")
    return poly, hbb, polyn, hbbn


def process_batch(detections, labels, iouv):
    """Return correct predictions matrix (val.py:69-90).  Both sets of boxes are in (x1, y1, x2, y2) format.
    Arguments:
        detections (Array[N, 6]), x1, y1, x2, y2, conf, class
        labels (Array[M, 5]), class, x1, y1, x2, y2
    Returns:
        correct (Array[N, 10]), for 10 IoU levels
    """
    _lib.require_cuda(detections, "detections")
    dev = detections.device
    det = detections.to(torch.float32).contiguous()
    lab = labels.to(device=dev, dtype=torch.float32).contiguous()
    iv = iouv.to(device=dev, dtype=torch.float32).contiguous()
    n, m, niou = det.shape[0], lab.shape[0], iv.shape[0]
    correct = torch.zeros((n, niou), dtype=torch.bool, device=dev)
    if n == 0:
        return correct
    L = _lib.lib()
    with _lib.guard(dev):
        ws = torch.empty(L.obb_process_batch_workspace_bytes(n, m), dtype=torch.uint8, device=dev)
        out = correct.view(torch.uint8)
        rc = L.obb_process_batch_f32(_lib.ptr(det), n, _lib.ptr(lab) if m else 0, m, _lib.ptr(iv), niou, _lib.ptr(out), _lib.ptr(ws),
                                     ws.numel(), _lib.stream_ptr(dev))
    _lib.check(rc, "obb_process_batch_f32")
    return correct


def process_batch_obb(pred, labels, iouv, return_match=False):
    """process_batch (val.py:69-90) with the ROTATED IoU: the oriented-box `correct` matrix of one image.
    Arguments:
        pred (Array[N, 7]), cx, cy, l, s, theta, conf, class -- the rows non_max_suppression_obb returns
        labels (Array[M, 6]), class, cx, cy, l, s, theta -- in the same (letterboxed) frame
    Returns:
        correct (Array[N, niou]) bool; with return_match also match_label (N) int32 -- the label row each detection kept,
        -1 for none, whether or not it won that label -- and match_iou (N) float32, that label's IoU or -1.
    iou[l, d] is ops.rotated_iou_pairs(label, detection) bit for bit; the rules are process_batch's (include/obb_hip.h)."""
    _lib.require_cuda(pred, "pred")
    if pred.dim() != 2 or pred.shape[1] != 7:
        raise RuntimeError(f"process_batch_obb: pred must be (n,7), got {tuple(pred.shape)}")
    if labels.dim() != 2 or labels.shape[1] != 6:
        raise RuntimeError(f"process_batch_obb: labels must be (m,6), got {tuple(labels.shape)}")
    dev = pred.device
    det = as_f32(pred, dev)
    lab = as_f32(labels, dev)
    iv = as_f32(iouv, dev)
    n, m, niou = det.shape[0], lab.shape[0], iv.shape[0]
    correct = torch.zeros((n, niou), dtype=torch.bool, device=dev)
    match_label = torch.full((n,), -1, dtype=torch.int32, device=dev)
    match_iou = torch.full((n,), -1.0, dtype=torch.float32, device=dev)
    if n:
        with _lib.guard(dev):
            rc = _lib.lib().obb_process_batch_obb_f32(_lib.ptr(det), n, _lib.ptr(lab) if m else 0, m, _lib.ptr(iv), niou,
                                                      _lib.ptr(correct.view(torch.uint8)), _lib.ptr(match_label), _lib.ptr(match_iou),
                                                      _lib.stream_ptr(dev))
        _lib.check(rc, "obb_process_batch_obb_f32")
    return (correct, match_label, match_iou) if return_match else correct


_pin_cache = {}


def _pinned_rows(n, cols):
    """A pinned (n, cols) float32 view of a cached host buffer (per thread; grown geometrically)."""
    key = (threading.get_ident(), cols)
    buf = _pin_cache.get(key)
    if buf is None or buf.shape[0] < n:
        buf = torch.empty((max(1024, 2 * n), cols), dtype=torch.float32).pin_memory()
        _pin_cache[key] = buf
    return buf[:n]


def val_tail_batch(preds, targets, shapes, iouv, want_boxes=False):
    """The tail of val.py:209-250 for ALL images of a batch: two launches, and the statistics land in pinned host memory
    that this thread polls (no copy kernel, no blocked stream wait; the host side of this function is most of its time, so it
    avoids every torch call it can).

    preds    list of (n_i, 7) CUDA tensors [x y l s theta conf cls], the output of non_max_suppression_obb (consecutive views
             of its packed buffer are used in place; anything else is concatenated)
    targets  (nt, >= 7) labels of the batch [img cls cx cy l s theta ...] in pixels of the letterboxed frame
    shapes   per image (shape (h, w), ratio_pad ((gain, gain), (pad_x, pad_y))) as LoadImagesAndLabels yields them
    Returns  stats: per image (correct bool (n_i, niou), conf (n_i), cls (n_i)) on the HOST -- what val.py:250 appends -- and,
             with want_boxes, the packed device arrays (pred_poly, pred_hbb, pred_polyn, pred_hbbn) + the offsets."""
    if len(preds) == 0:
        return ([], None) if want_boxes else []
    ext = _lib.compiled()
    if ext is not None:          # the compiled binding builds the per-image tuples in C++ (csrc/torch_ext/nms_rotated_ext.cpp)
        return ext.val_tail_batch(list(preds), targets, shapes, iouv, bool(want_boxes))
    _lib.require_cuda(preds[0], "pred")
    dev = preds[0].device
    tb = TailBatch(preds, targets, dev)
    if not tb.in_place:
        _lib.require_cuda_preds(preds)
    n, niou = tb.n, iouv.shape[0]
    iv = as_f32(iouv, dev)
    host = _pinned_rows(n, niou + 2)                             # the kernels write the rows straight into it
    boxes = box_arrays(n, dev) if want_boxes else None
    if n:
        L = _lib.lib()
        with _lib.guard(dev):
            st = _lib.stream_handle(dev)
            ws = _lib.workspace(L.obb_val_tail_batch_workspace_bytes(n, tb.nt), dev, st)
            flag, flag_np = _lib.pinned_count(dev)
            for ch in tb.chunks(shapes):                         # (one call for any batch size val.py uses)
                if tb.bs > MAX_BS:                               # a chunk of several: the flag is armed again for each
                    flag_np[0] = _lib._PENDING
                rc = L.obb_val_tail_batch_polled_f32(
                    ch.part(tb.packed, 7), ch.doff, ch.k, ch.tg_ptr, ch.ntk, ch.tcols, ch.img5, iv.data_ptr(), niou, *ch.box_parts(boxes),
                    ch.part(host, niou + 2), ws.data_ptr(), ws.numel(), st, flag.data_ptr())
                _lib.check(rc, "obb_val_tail_batch_f32")
                _lib.wait_count(flag_np, dev)                    # every row of this chunk is in `host`
    # (the pinned buffer is reused by the next batch.  Copy and compare through numpy, single-threaded: a torch CPU op on these
    #  ~44k elements fans out to the whole intra-op pool -- 128 OpenMP workers on the GPU boxes -- whose spinning uses up the
    #  container's CPU quota: the kernel then parks the process for the rest of the 100 ms period, profiles/r5_host_stall.md)
    out = split_rows(host.numpy().copy(), niou, tb.counts)
    return (out, (boxes, tb.offs)) if want_boxes else out


def _obb_tail_launch(L, tb, iv, niou, rows, row0, match_label, match_iou, st):
    """obb_val_tail_batch_obb_f32 on every chunk of the batch: the stats rows go to rows[row0 + d], the match arrays to [d],
    d = the packed row of the detection."""
    for ch in tb.chunks():
        rc = L.obb_val_tail_batch_obb_f32(
            ch.part(tb.packed, 7), None, ch.doff, ch.k, ch.tg_ptr, ch.ntk, ch.tcols, iv.data_ptr(), niou,
            ch.part(rows, niou + 2, row0), ch.part(match_label, 1), ch.part(match_iou, 1), st)
        _lib.check(rc, "obb_val_tail_batch_obb_f32")
        if ch.rows is not None and ch.ntk:                       # rows of the chunk's label list -> rows of `targets`
            ml = match_label[ch.lo:ch.hi]
            ml.copy_(torch.where(ml >= 0, ch.rows.to(torch.int32)[ml.clamp(min=0).long()], ml))


def val_tail_batch_obb(preds, targets, iouv, return_match=False):
    """The oriented-box statistics of ALL images of a batch, what val.py:250 would append if process_batch compared rotated
    boxes: per image (correct bool (n_i, niou), conf (n_i), cls (n_i)) on the HOST, like val_tail_batch.  Two launches.

    preds    list of (n_i, 7) CUDA tensors [x y l s theta conf cls], the output of non_max_suppression_obb
    targets  (nt, >= 7) labels of the batch [img cls cx cy l s theta ...] in pixels of the letterboxed frame
    No shapes: both boxes stay in the letterboxed frame (the rotated IoU does not change under scale_polys).  With return_match
    also, per image, (match_label int32: the row of `targets` each detection kept or -1, match_iou float32) on the device."""
    if len(preds) == 0:
        return ([], []) if return_match else []
    _lib.require_cuda(preds[0], "pred")
    dev = preds[0].device
    tb = TailBatch(preds, targets, dev)
    if not tb.in_place:
        _lib.require_cuda_preds(preds)
    n, niou = tb.n, int(iouv.shape[0])
    iv = as_f32(iouv, dev)
    rows = torch.empty((n, niou + 2), dtype=torch.float32, device=dev)
    match_label = torch.full((n,), -1, dtype=torch.int32, device=dev)
    match_iou = torch.full((n,), -1.0, dtype=torch.float32, device=dev)
    if n:
        with _lib.guard(dev):
            _obb_tail_launch(_lib.lib(), tb, iv, niou, rows, 0, match_label, match_iou, _lib.stream_handle(dev))
    out = split_rows(rows.cpu().numpy(), niou, tb.counts)
    return (out, list(zip(match_label.split(tb.counts), match_iou.split(tb.counts)))) if return_match else out


class ValStats:
    """The statistics of a whole validation run in DEVICE memory: what val.py:250 appends per image and :269 concatenates, as
    one (n, niou + 2) array of rows [correct x niou as 0 / 1, conf, cls] (the rows obb_val_tail_batch_f32 writes, in the order
    of the images) plus the class of every label -- the inputs of utils.metrics.ap_per_class, which then runs on them where
    they lie.  Nothing is copied to the host and nothing waits for the stream until ap_per_class() / cpu() is called.

    Beside the rows, three values per image seen, on the device too: its rows, its labels and a global image id (`image_ids=` of
    add_batch; a running index by default).  They are what puts the statistics of several ranks back in image order: merged()
    for accumulators on one device, all_gather() across the ranks of a process group (stats_merge.py)."""

    def __init__(self, niou=10, device=None, capacity=1 << 16, obb=False):
        self.niou = int(niou)
        self.obb = bool(obb)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("ValStats: device must be a CUDA/HIP device (no CPU path, by design)")
        self.n, self.m = 0, 0
        self._rows = torch.empty((max(1, int(capacity)), self.niou + 2), dtype=torch.float32, device=self.device)
        self._tcls = torch.empty(max(1, int(capacity) // 8), dtype=torch.float32, device=self.device)
        self._result = [None, None]            # of _metrics(obb=False / True)
        # obb=True: the same rows with process_batch on the ROTATED boxes (obb_val_tail_batch_obb_f32), row for row beside the others
        self._rows_obb = torch.empty_like(self._rows) if self.obb else None
        self._match = None
        self.k = 0                             # images seen
        self._img_rows = torch.empty(1024, dtype=torch.int32, device=self.device)
        self._img_labels = torch.empty(1024, dtype=torch.int32, device=self.device)
        self._img_ids = torch.empty(1024, dtype=torch.int64, device=self.device)
        self._arange = {}                      # batch size -> (1, bs) float32 0 .. bs - 1 on the device
        self._merge_info, self._merge_error = None, None
        self.supplied = None                   # merged() / all_gather(): the images their parts held between them

    @property
    def rows(self):
        """(n, niou + 2) float32 on the device."""
        return self._rows[:self.n]

    @property
    def target_cls(self):
        """(m) float32 on the device: the class of every label seen, images without detections included (val.py:213-215)."""
        return self._tcls[:self.m]

    @staticmethod
    def _grown(buf, used, need):
        """buf with room for `need` leading entries (grown geometrically; the first `used` are kept)."""
        if need <= buf.shape[0]:
            return buf
        new = torch.empty((max(need, 2 * buf.shape[0]),) + tuple(buf.shape[1:]), dtype=buf.dtype, device=buf.device)
        new[:used] = buf[:used]
        return new

    def _note_images(self, tb, image_ids):
        """Rows, labels and id of every image of the batch, behind the ones already held.  Nothing waits: the row counts and the
        ids are on the host already (one pinned array, one asynchronous copy), the label counts are a compare-and-sum over the
        image column of `targets` on the stream (an image index outside the batch counts nowhere and indexes nothing)."""
        bs, k = tb.bs, self.k
        if bs == 0:
            return
        ids = range(k, k + bs) if image_ids is None else [int(i) for i in image_ids]
        if len(ids) != bs:
            raise RuntimeError(f"ValStats: {len(ids)} image ids for a batch of {bs} images")
        host = torch.tensor(tb.counts + list(ids), dtype=torch.int64).pin_memory()
        both = host.to(self.device, non_blocking=True)
        self._img_rows = self._grown(self._img_rows, k, k + bs)
        self._img_labels = self._grown(self._img_labels, k, k + bs)
        self._img_ids = self._grown(self._img_ids, k, k + bs)
        self._img_rows[k:k + bs] = both[:bs]
        self._img_ids[k:k + bs] = both[bs:]
        if tb.nt:
            ar = self._arange.get(bs)
            if ar is None:
                ar = self._arange[bs] = torch.arange(bs, dtype=torch.float32, device=self.device)[None, :]
            self._img_labels[k:k + bs] = (tb.tg[:, 0:1] == ar).sum(0)
        else:
            self._img_labels[k:k + bs] = 0
        self.k += bs

    def add_batch(self, preds, targets, shapes, iouv, want_boxes=False, confusion=None, image_ids=None):
        """The inputs of val_tail_batch; the rows go straight behind the ones already held.  Returns None, or with want_boxes
        the packed device arrays (pred_poly, pred_hbb, pred_polyn, pred_hbbn) and the per-image offsets.
        confusion: a utils.metrics.ConfusionMatrix -- val.py:245-246 with plots=True: its launch runs right behind the tail's
        two, on the same packed detections and targets.
        image_ids: the global id of every image of the batch (a sharded run: its index in the whole image list); default: the
        running index 0, 1, 2, ... of the images this accumulator has seen.  Images without detections, without labels or with
        neither are recorded too.  (merged() / all_gather() take the labels of an image to be consecutive rows of `targets`, the
        images ascending, as collate_fn yields them.)"""
        dev = self.device
        if int(iouv.shape[0]) != self.niou:
            raise RuntimeError(f"ValStats: iouv has {int(iouv.shape[0])} levels, this accumulator {self.niou}")
        for p in preds:
            if p.device != dev:
                _lib.require_cuda(p, "pred")
                raise RuntimeError(f"ValStats: pred on {p.device}, the accumulator on {dev}")
        tb = TailBatch(preds, targets, dev)
        n, nt = tb.n, tb.nt
        self._result = [None, None]
        self._note_images(tb, image_ids)
        if nt:
            self._tcls = self._grown(self._tcls, self.m, self.m + nt)
            self._tcls[self.m:self.m + nt] = tb.tg[:, 1]
            self.m += nt
        boxes = box_arrays(n, dev) if want_boxes else None
        if n == 0:
            return (boxes, tb.offs) if want_boxes else None
        iv = as_f32(iouv, dev)
        self._rows = self._grown(self._rows, self.n, self.n + n)
        if self.obb:
            self._rows_obb = self._grown(self._rows_obb, self.n, self.n + n)
        L = _lib.lib()
        with _lib.guard(dev):
            st = _lib.stream_handle(dev)
            ws = _lib.workspace(L.obb_val_tail_batch_workspace_bytes(n, nt), dev, st)
            for ch in tb.chunks(shapes):
                rc = L.obb_val_tail_batch_f32(
                    ch.part(tb.packed, 7), ch.doff, ch.k, ch.tg_ptr, ch.ntk, ch.tcols, ch.img5, iv.data_ptr(), self.niou,
                    *ch.box_parts(boxes), ch.part(self._rows, self.niou + 2, self.n), ws.data_ptr(), ws.numel(), st)
                _lib.check(rc, "obb_val_tail_batch_f32")
                if confusion is not None:
                    confusion._launch(L, tb, ch, st)
            if self.obb:                                         # (the match arrays of the last batch stay readable: last_match)
                self._match = (torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.float32, device=dev))
                _obb_tail_launch(L, tb, iv, self.niou, self._rows_obb, self.n, self._match[0], self._match[1], st)
        self.n += n
        return (boxes, tb.offs) if want_boxes else None

    def _metrics(self, obb=False):
        """(the 7-tuple of ap_per_class, info) over `rows`, or over `rows_obb`; kept until the next batch."""
        self._check_merge()
        rows = self.rows_obb if obb else self.rows
        if self._result[obb] is None:
            from .utils import metrics
            self._result[obb] = metrics.ap_from_rows(rows, self.target_cls, self.niou)
        return self._result[obb]

    def _cpu(self, rows):
        self._check_merge()
        arr = rows.cpu().numpy()
        return arr[:, :self.niou] > 0.5, arr[:, self.niou].copy(), arr[:, self.niou + 1].copy(), self.target_cls.cpu().numpy()

    def ap_per_class(self):
        """utils.metrics.ap_per_class over everything added so far (the 7-tuple of numpy arrays)."""
        return self._metrics()[0]

    @property
    def any_tp(self):
        """val.py:270's guard `stats[0].any()`: a true positive at the first IoU level."""
        return self._metrics()[1][1] > 0

    def cpu(self):
        """(correct bool (n, niou), conf (n), pcls (n), tcls (m)) numpy arrays: the four arrays of val.py:269."""
        return self._cpu(self.rows)

    # ---- per image: rows, labels, global id -- and the merge of several accumulators in id order
    @property
    def img_rows(self):
        """(k) int32 on the device: the detection rows of every image seen, in the order they were added."""
        return self._img_rows[:self.k]

    @property
    def img_labels(self):
        """(k) int32 on the device: the labels of every image seen."""
        return self._img_labels[:self.k]

    @property
    def img_ids(self):
        """(k) int64 on the device: the global id of every image seen."""
        return self._img_ids[:self.k]

    def _shard(self):
        return stats_merge.Shard(self.rows, self._rows_obb[:self.n] if self.obb else None, self.target_cls, self.img_rows, self.img_labels,
                                 self.img_ids)

    @classmethod
    def _of_merged(cls, mg, niou, obb, device):
        out = cls(niou=niou, device=device, capacity=1, obb=obb)
        out._rows, out._rows_obb, out._tcls = mg.rows, mg.rows_obb, mg.tcls
        out.n, out.m, out.k = mg.totals
        out._img_rows, out._img_labels = mg.img_rows, mg.img_labels
        out._img_ids = torch.arange(out.k, dtype=torch.int64, device=out.device)
        out._merge_info = mg.info
        out.supplied = mg.supplied             # images the merged parts held between them (k counts the ids no part held too)
        return out

    def _check_merge(self):
        """The info words of the merge that made this accumulator, read where the caller synchronises anyway."""
        if self._merge_info is not None:
            self._merge_error = stats_merge.describe(self._merge_info.cpu())
            self._merge_info = None
        if self._merge_error:
            raise RuntimeError(f"ValStats: {self._merge_error}")

    @classmethod
    def merged(cls, parts, n_images_total=None, merge=None):
        """parts: accumulators on ONE device (virtual ranks, or shards gathered there) whose image ids are distinct -> a new
        ValStats whose rows, rows_obb, target_cls, per-image counts and ids are those of a single accumulator that was fed every
        image in ascending id order (ids no part holds, below n_images_total, are images without rows and labels).
        n_images_total: default the number of images the parts hold.  Three calls of obb_stats_merge_f32, nothing waits; an id
        held twice, an id outside [0, n_images_total) or counts that do not add up raise RuntimeError at the next
        ap_per_class() / cpu(), where the host waits for the device anyway."""
        parts = list(parts)
        if not parts:
            raise RuntimeError("ValStats.merged: no accumulators")
        p0 = parts[0]
        for p in parts:
            if p.device != p0.device or p.niou != p0.niou or p.obb != p0.obb:
                raise RuntimeError("ValStats.merged: the accumulators must share device, niou and obb")
            p._check_merge()
        with _lib.guard(p0.device):
            mg = stats_merge.merge_parts([p._shard() for p in parts], p0.niou + 2, p0.obb, n_images_total, merge)
        return cls._of_merged(mg, p0.niou, p0.obb, p0.device)

    def all_gather(self, group=None, n_images_total=None, merge=None):
        """The one exchange of a sharded run (stats_merge.exchange): the totals of every rank, then the padded rows -- RCCL
        gathers device buffers, any other backend stages through the host, once per run -- then merged() on every rank: each
        rank returns the ValStats of the whole run.  Without a process group: merged([self])."""
        self._check_merge()
        with _lib.guard(self.device):
            mg = stats_merge.exchange(self._shard(), self.niou + 2, self.obb, group, n_images_total, merge)
        return self._of_merged(mg, self.niou, self.obb, self.device)

    # ---- obb=True: the oriented-box statistics, accessor for accessor
    def _need_obb(self):
        if not self.obb:
            raise RuntimeError("ValStats: the oriented-box statistics need ValStats(obb=True)")

    @property
    def rows_obb(self):
        """(n, niou + 2) float32 on the device: `rows` with `correct` from the rotated IoU (conf and cls are the same)."""
        self._need_obb()
        return self._rows_obb[:self.n]

    @property
    def last_match(self):
        """(match_label int32, match_iou float32) of the last batch added, by packed detection row (None before any)."""
        self._need_obb()
        return self._match

    def ap_per_class_obb(self):
        """utils.metrics.ap_per_class over the oriented-box rows: the OBB mAP@0.5 and mAP@0.5:0.95 of everything added so far."""
        return self._metrics(True)[0]

    @property
    def any_tp_obb(self):
        return self._metrics(True)[1][1] > 0

    def cpu_obb(self):
        """cpu() of the oriented-box rows."""
        return self._cpu(self.rows_obb)
