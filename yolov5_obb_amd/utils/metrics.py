"""Mirror of the reference's ``utils/metrics.py::ap_per_class`` (:21-114) on the device: one call of
``obb_ap_per_class_f32`` (csrc/metrics.hip) over statistics that may never have left device memory (``val.ValStats``).

ONE deliberate difference: the order among equal confidences.  The reference sorts with ``np.argsort(-conf)``, an unstable
introsort, so tied rows land in an unspecified order and its AP moves with it (by up to 8e-3 on 5,000 rows with two-decimal
confidences).  Here ties are broken by ASCENDING ROW INDEX -- ``np.argsort(-conf, kind='stable')`` -- like every score sort
of this package.  Everything else is numpy's arithmetic in double, operation for operation.

``ConfusionMatrix`` (:117-163 of the reference) is the other class of that file that lives here: one launch of
``obb_confusion_batch_f32`` per batch (csrc/head.hip: k_confusion) into counters that stay on the device.  Its deliberate
difference is of the same kind: the reference orders equal IoUs with ``matches[:, 2].argsort()[::-1]``, numpy's unstable
sort; here every argsort is stable (the rule is written out on the class).

Opt-in: ``dropin.install()`` does not replace the reference's function or class."""
import numpy as np
import torch

from .. import _lib
from ..tail_batch import TailBatch

NC_MAX = 256      # include/obb_hip.h: class ids are integers 0 .. 255
MAX_NIOU = 16


def ap_from_rows(rows, target_cls, niou):
    """rows (n, >= niou + 2) float32 CUDA with unit column stride [correct x niou as 0 / 1, conf, cls] -- the rows
    obb_val_tail_batch_f32 writes -- and target_cls (m) float32 CUDA -> (the 7-tuple of ap_per_class, info) with info =
    (best F1 index, true positives at IoU column 0).  One launch chain, one copy back."""
    dev = rows.device
    n, m = int(rows.shape[0]), int(target_cls.shape[0])
    if not 1 <= niou <= MAX_NIOU:
        raise RuntimeError(f"ap_per_class: 1 <= niou <= {MAX_NIOU}, got {niou}")
    if m == 0:                                                     # no labels, no classes: the reference's shapes, no launch
        z = np.zeros(0)
        tp0 = int((rows[:, 0] > 0.5).sum()) if n else 0
        return (z, z.copy(), z.copy(), z.copy(), z.copy(), np.zeros((0, niou)), np.zeros(0, dtype=np.int32)), (0, tp0)
    if n and (rows.dtype != torch.float32 or rows.stride(1) != 1 or rows.shape[1] < niou + 2):
        raise RuntimeError("ap_per_class: rows must be float32 (n, >= niou + 2) with contiguous rows")
    tc = target_cls if target_cls.dtype == torch.float32 and target_cls.is_contiguous() else target_cls.float().contiguous()
    L = _lib.lib()
    n_ap, n_prf, n_cnt = NC_MAX * niou, NC_MAX * 5, NC_MAX          # (counts: 2 x 256 int32 = 256 doubles; info: 4 int32 = 2)
    with _lib.guard(dev):
        out = torch.empty(n_ap + n_prf + n_cnt + 2, dtype=torch.float64, device=dev)      # one buffer, one copy back
        ap_d, prf_d, cnt_d, info_d = out[:n_ap], out[n_ap:n_ap + n_prf], out[n_ap + n_prf:n_ap + n_prf + n_cnt], out[n_ap + n_prf + n_cnt:]
        st = _lib.stream_handle(dev)
        ws = _lib.workspace(L.obb_ap_per_class_workspace_bytes(n, niou, NC_MAX), dev, st)
        rc = L.obb_ap_per_class_f32(_lib.ptr(rows) if n else None, int(rows.stride(0)) if n else niou + 2, n, niou, _lib.ptr(tc), m, NC_MAX,
                                    _lib.ptr(ap_d), _lib.ptr(prf_d), _lib.ptr(cnt_d), _lib.ptr(info_d), None, _lib.ptr(ws), ws.numel(),
                                    _lib.stream_ptr(dev))
        _lib.check(rc, "obb_ap_per_class_f32")
        host = out.cpu().numpy()
    ap = host[:n_ap].reshape(NC_MAX, niou)
    prf = host[n_ap:n_ap + n_prf].reshape(NC_MAX, 5)
    counts = host[n_ap + n_prf:n_ap + n_prf + n_cnt].view(np.int32).reshape(2, NC_MAX)
    info = host[n_ap + n_prf + n_cnt:].view(np.int32)
    if info[2]:
        raise RuntimeError(f"ap_per_class: a class value (pred_cls or target_cls) is not an integer in [0, {NC_MAX})")
    if info[3]:
        raise RuntimeError("ap_per_class: conf holds NaN (the order of such rows is unspecified)")
    keep = np.flatnonzero(counts[0] > 0)                            # np.unique(target_cls)
    res = (prf[keep, 3].copy(), prf[keep, 4].copy(), prf[keep, 0].copy(), prf[keep, 1].copy(), prf[keep, 2].copy(), ap[keep].copy(),
           keep.astype(np.int32))
    return res, (int(info[0]), int(info[1]))


def _to_dev(x, dev, dtype=torch.float32):
    if isinstance(x, torch.Tensor):
        return x.to(device=dev, dtype=dtype)
    return torch.as_tensor(np.asarray(x), device=dev).to(dtype)


def ap_per_class(tp, conf, pred_cls, target_cls, plot=False, save_dir='.', names=(), eps=1e-16):
    """ Compute the average precision, given the recall and precision curves (utils/metrics.py:21).
    # Arguments
        tp:  True positives (n x niou), conf (n), pred_cls (n), target_cls (m): CUDA tensors or numpy arrays (numpy arrays are
             copied to the current device); conf is taken as float32, what the validation path produces
    # Returns
        tp, fp, p, r, f1 (nc,) float64, ap (nc, niou) float64, unique_classes (nc,) int32 -- numpy arrays, as the reference's
    Equal confidences are ordered by ascending row index (see the module docstring)."""
    if plot:
        raise NotImplementedError("ap_per_class: plots are not part of this package; call the reference's function for them")
    if eps != 1e-16:
        raise RuntimeError("ap_per_class: eps is fixed at 1e-16 (the reference's default)")
    dev = next((x.device for x in (tp, conf, pred_cls, target_cls) if isinstance(x, torch.Tensor) and x.is_cuda), None)
    if dev is None:
        if any(isinstance(x, torch.Tensor) for x in (tp, conf, pred_cls)):
            _lib.require_cuda(tp if isinstance(tp, torch.Tensor) else conf, "tp")
        dev = torch.device("cuda", torch.cuda.current_device())
    tp = _to_dev(tp, dev)
    if tp.dim() != 2:
        raise RuntimeError(f"ap_per_class: tp must be (n, niou), got {tuple(tp.shape)}")
    n, niou = tp.shape
    conf, pred_cls = _to_dev(conf, dev).reshape(-1), _to_dev(pred_cls, dev).reshape(-1)
    if conf.shape[0] != n or pred_cls.shape[0] != n:
        raise RuntimeError("ap_per_class: tp, conf and pred_cls must have the same number of rows")
    rows = torch.cat((tp, conf[:, None], pred_cls[:, None]), 1)
    return ap_from_rows(rows, _to_dev(target_cls, dev).reshape(-1), niou)[0]


class ConfusionMatrix:
    """The reference's ConfusionMatrix (utils/metrics.py:117-163) with the counters in device memory: process_batch / add_batch
    launch one kernel and return; nothing is copied and nothing waits until `.matrix` is read.

    Per image: detections with conf > self.conf against the labels, a pair is a candidate iff box_iou > self.iou_thres (both
    strict, in float32).  TIES, where the reference's numpy sort leaves the order unspecified, are pinned to the reference's own
    lines with every argsort stable: a detection chooses its candidate label of highest IoU, ties to the HIGHER label index;
    a label keeps, among the detections that chose it, the one of highest IoU, ties to the HIGHER detection index.  The fill is
    the reference's, quirks included: the winner's cell is taken whether or not the classes agree, an unmatched label counts in
    the background row, an unmatched kept detection in the background column -- but only in an image with at least one match.
    A class outside [0, nc) touches no cell and makes the next read of `.matrix` raise (the reference raises IndexError, or
    wraps a negative index silently).  Per-image counts up to 32767 (the reference's int16 wrap above is not reproduced)."""

    def __init__(self, nc, conf=0.25, iou_thres=0.45, device=None):
        self.nc = int(nc)  # number of classes
        self.conf = conf
        self.iou_thres = iou_thres
        if self.nc < 1:
            raise RuntimeError(f"ConfusionMatrix: nc must be >= 1, got {nc}")
        self.device = None if device is None else torch.device(device)
        if self.device is not None and self.device.type != "cuda":
            raise RuntimeError("ConfusionMatrix: device must be a CUDA/HIP device (no CPU path, by design)")
        self._mat = None                   # (nc + 1)^2 + 1 int64 on the device, made at the first batch; the last one counts bad classes

    def _counters(self, dev):
        if self._mat is None:
            if self.device is None:
                self.device = dev
            self._mat = torch.zeros((self.nc + 1) ** 2 + 1, dtype=torch.int64, device=self.device)
        if dev != self._mat.device:
            raise RuntimeError(f"ConfusionMatrix: input on {dev}, the counters on {self._mat.device}")
        return self._mat

    def process_batch(self, detections, labels):
        """
        Arguments:
            detections (Array[N, 6]), x1, y1, x2, y2, conf, class   (CUDA)
            labels (Array[M, 5]), class, x1, y1, x2, y2             (moved to the detections' device when they are elsewhere)
        Returns:
            None, updates confusion matrix accordingly (asynchronously)
        """
        _lib.require_cuda(detections, "detections")
        dev = detections.device
        if detections.dim() != 2 or detections.shape[1] != 6 or labels.dim() != 2 or labels.shape[1] != 5:
            raise RuntimeError(f"ConfusionMatrix: detections (n, 6) and labels (m, 5), got {tuple(detections.shape)} and {tuple(labels.shape)}")
        mat = self._counters(dev)
        n, m = int(detections.shape[0]), int(labels.shape[0])
        if n == 0 or m == 0:
            return
        det = detections.to(torch.float32).contiguous()
        lab = labels.to(device=dev, dtype=torch.float32).contiguous()
        L = _lib.lib()
        with _lib.guard(dev):
            st = _lib.stream_handle(dev)
            ws = _lib.workspace(L.obb_confusion_workspace_bytes(n, m), dev, st)
            rc = L.obb_confusion_process_batch_f32(_lib.ptr(det), n, _lib.ptr(lab), m, self.nc, float(self.conf), float(self.iou_thres),
                                                   _lib.ptr(mat), _lib.ptr(ws), ws.numel(), st)
        _lib.check(rc, "obb_confusion_process_batch_f32")

    def _launch(self, L, tb, ch, st):
        """One obb_confusion_batch_f32 on a chunk (tail_batch.Chunk, with its img5) of the batch tb: <= 64 images."""
        mat = self._counters(tb.device)
        if ch.ntk == 0:
            return
        ws = _lib.workspace(L.obb_confusion_workspace_bytes(ch.hi - ch.lo, ch.ntk), tb.device, st)
        rc = L.obb_confusion_batch_f32(ch.part(tb.packed, 7), ch.doff, ch.k, ch.tg_ptr, ch.ntk, ch.tcols, ch.img5, self.nc,
                                       float(self.conf), float(self.iou_thres), _lib.ptr(mat), _lib.ptr(ws), ws.numel(), st)
        _lib.check(rc, "obb_confusion_batch_f32")

    def add_batch(self, preds, targets, shapes):
        """process_batch for ALL images of a batch in one launch, from the arguments of val.val_tail_batch: preds list of (n_i, 7)
        CUDA tensors [x y l s theta conf cls] (consecutive views of non_max_suppression_obb's packed buffer are used in place),
        targets (nt, >= 7) [img cls cx cy l s theta ...], shapes per image ((h, w), ((gain, gain), (pad_x, pad_y))).  The boxes
        are those of val.py:226-243 (pred_hbbn, labels_hbbn); images without detections or without labels add nothing."""
        if len(preds) == 0:
            return
        _lib.require_cuda(preds[0], "pred")
        dev = preds[0].device
        self._counters(dev)
        tb = TailBatch(preds, targets, dev)
        if tb.n == 0 or tb.nt == 0:
            return
        if not tb.in_place:
            _lib.require_cuda_preds(preds)
        L = _lib.lib()
        with _lib.guard(dev):
            st = _lib.stream_handle(dev)
            for ch in tb.chunks(shapes):
                self._launch(L, tb, ch, st)

    def all_reduce(self, group=None, device=None):
        """Sum the counters over the ranks of a process group (the cells AND the counter of classes out of range): after it every
        rank holds the matrix of the whole run.  RCCL reduces the device array in place; any other backend stages it through the
        host.  device: where the counters are made when this rank has not seen a batch.  No process group: nothing to do."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
            return
        if self._mat is None:
            dev = self.device if self.device is not None else device
            if dev is None:
                raise RuntimeError("ConfusionMatrix.all_reduce: no batch was added on this rank; pass device=")
            dev = torch.device(dev)
            self._counters(dev if dev.index is not None else torch.device("cuda", torch.cuda.current_device()))
        if dist.get_backend(group) == "nccl":
            dist.all_reduce(self._mat, group=group)
        else:
            host = self._mat.cpu()
            dist.all_reduce(host, group=group)
            self._mat.copy_(host)

    @property
    def matrix(self):
        """(nc + 1, nc + 1) float64 numpy array [predicted][true], as the reference's attribute.  The one place that waits for
        the device; raises RuntimeError when a class outside [0, nc) was met."""
        cells = (self.nc + 1) ** 2
        if self._mat is None:
            return np.zeros((self.nc + 1, self.nc + 1))
        torch.cuda.synchronize(self._mat.device)
        host = self._mat.cpu().numpy()
        if host[cells]:
            raise RuntimeError(f"ConfusionMatrix: {int(host[cells])} cells were not counted: a detection or label class outside [0, {self.nc})")
        return host[:cells].reshape(self.nc + 1, self.nc + 1).astype(np.float64)

    def tp_fp(self):
        matrix = self.matrix
        tp = matrix.diagonal()  # true positives
        fp = matrix.sum(1) - tp  # false positives
        return tp[:-1], fp[:-1]  # remove background class

    def plot(self, normalize=True, save_dir='', names=()):
        raise NotImplementedError("ConfusionMatrix.plot: plots are not part of this package; assign this object's .matrix to the "
                                  "reference's ConfusionMatrix and call its plot()")

    def print(self):
        matrix = self.matrix
        for i in range(self.nc + 1):
            print(' '.join(map(str, matrix[i])))
