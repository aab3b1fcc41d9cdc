"""Mirror of the reference's ``utils/metrics.py::ap_per_class`` (:21-114) on the device: one call of
``obb_ap_per_class_f32`` (csrc/metrics.hip) over statistics that may never have left device memory (``val.ValStats``).

ONE deliberate difference: the order among equal confidences.  The reference sorts with ``np.argsort(-conf)``, an unstable
introsort, so tied rows land in an unspecified order and its AP moves with it (by up to 8e-3 on 5,000 rows with two-decimal
confidences).  Here ties are broken by ASCENDING ROW INDEX -- ``np.argsort(-conf, kind='stable')`` -- like every score sort
of this package.  Everything else is numpy's arithmetic in double, operation for operation.

Opt-in: ``dropin.install()`` does not replace the reference's function."""
import numpy as np
import torch

from .. import _lib

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
