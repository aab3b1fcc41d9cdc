"""DOTA Task-2 (horizontal box) evaluation with the det x GT overlaps on the GPU: the interface of the reference's
DOTA_devkit/dota_evaluation_task2.py (`parse_gt`, `voc_ap`, `voc_eval`, `evaluate` = its main loop), same file formats.

The reference walks the confidence-sorted detections one by one with five numpy calls each (:177-202).  Here the
(ovmax, jmax) of all detections of a class file are one device call (`obb_eval_best_gt_hbb_f64`); reading the files,
`np.argsort(-confidence)`, the first-occurrence TP pass and the AP integration are the Task-1 mirror's, on the host in double.
GPU only.
"""
import numpy as np
import torch

from .. import _lib
from . import dota_evaluation_task1 as _task1
from .dota_evaluation_task1 import voc_ap  # noqa: F401  (:47-78, the same function as Task 1's)


def parse_gt(filename):
    """:19-46.  `x1 y1 x2 y2 x3 y3 x4 y4 name [difficult]` per line; the box is int(float()) of columns 0, 1, 4, 5."""
    objects = []
    with open(filename, 'r') as f:
        for line in f:
            tok = line.strip().split(' ')
            if len(tok) < 9:
                continue
            obj = {'name': tok[8]}
            if len(tok) == 9:
                obj['difficult'] = 0
            elif len(tok) == 10:
                obj['difficult'] = int(tok[9])
            obj['bbox'] = [int(float(tok[0])), int(float(tok[1])), int(float(tok[4])), int(float(tok[5]))]
            obj['area'] = (obj['bbox'][2] - obj['bbox'][0]) * (obj['bbox'][3] - obj['bbox'][1])
            objects.append(obj)
    return objects


def load_gt(annopath, imagenames, classname):
    """(gts (k, 4) float64 truncated toward zero, difficult (k,) bool, gt_off) of one class over the listed images.  From the
    Task-1 reader's exact doubles when every file is the plain layout and the four columns are finite (np.trunc of a finite
    double is float(int())); through parse_gt otherwise, which raises on a non-finite value like the reference's int()."""
    fast = _task1.load_gt(annopath, imagenames, classname)
    if fast is not None and np.isfinite(fast[0][:, [0, 1, 4, 5]]).all():
        return np.trunc(fast[0][:, [0, 1, 4, 5]]) + 0.0, fast[1], fast[2]     # (+ 0.0: int() has no negative zero)
    gts, gt_off, difficult = [], [0], []
    for imagename in imagenames:
        objs = [o for o in parse_gt(annopath.format(imagename)) if o['name'] == classname]
        gts.extend(o['bbox'] for o in objs)
        difficult.extend(bool(o['difficult']) for o in objs)
        gt_off.append(len(gts))
    return (np.array(gts, dtype=np.float64).reshape(-1, 4), np.array(difficult, dtype=np.bool_),
            np.array(gt_off, dtype=np.int64))


def read_detections(detfile):
    """`image score xmin ymin xmax ymax [more]` per line (:151-161) -> (image ids, confidence (n,), BB (n, >= 4))."""
    return _task1.read_detections_text(detfile, lambda ncols: ncols >= 6)


def best_gt(dets, det_img, gts4, gt_off):
    """(ovmax, jmax) per detection over the boxes of its image (include/obb_hip.h: obb_eval_best_gt_hbb_f64).  dets: rows of
    at least four doubles, xmin ymin xmax ymax first."""
    if not torch.cuda.is_available():
        raise RuntimeError("yolov5_obb_amd Task-2 evaluation needs a HIP device (no CPU fallback)")
    dev = torch.device("cuda", torch.cuda.current_device())
    dets = np.ascontiguousarray(dets, dtype=np.float64)
    if dets.ndim != 2 or dets.shape[1] < 4:
        raise IndexError(f"detections need at least four columns after the score, got an array of shape {dets.shape}")
    nd = len(dets)
    d_det = torch.from_numpy(dets).to(dev)
    d_img = torch.from_numpy(np.ascontiguousarray(det_img, dtype=np.int32)).to(dev)
    d_gt = torch.from_numpy(np.ascontiguousarray(gts4, dtype=np.float64).reshape(-1, 4)).to(dev)
    d_off = torch.from_numpy(np.ascontiguousarray(gt_off, dtype=np.int32)).to(dev)
    ov = torch.empty(nd, dtype=torch.float64, device=dev)
    jm = torch.empty(nd, dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().obb_eval_best_gt_hbb_f64(_lib.ptr(d_det), dets.shape[1], _lib.ptr(d_img), nd, _lib.ptr(d_gt),
                                                   _lib.ptr(d_off), len(gt_off) - 1, _lib.ptr(ov), _lib.ptr(jm),
                                                   _lib.stream_ptr(dev)), "obb_eval_best_gt_hbb_f64")
    return ov.cpu().numpy(), jm.cpu().numpy()


def voc_eval(detpath, annopath, imagesetfile, classname, ovthresh=0.5, use_07_metric=False):
    """:80-231.  rec, prec, ap of one class."""
    with open(imagesetfile, 'r') as f:
        imagenames = [x.strip() for x in f.readlines()]
    index = {imagename: i for i, imagename in enumerate(imagenames)}   # a name listed twice: the last record wins, as in the reference's dict
    gts, difficult, gt_off = load_gt(annopath, imagenames, classname)
    npos = int((~difficult).sum())                       # :145 adds per listed name, duplicates included

    image_ids, confidence, BB = read_detections(detpath.format(classname))
    sorted_ind = np.argsort(-confidence)                 # :164
    BB = BB[sorted_ind, :]
    det_img = np.array([index[image_ids[x]] for x in sorted_ind], dtype=np.int32)   # KeyError for an unlisted image, as :178

    ovmax, jmax = best_gt(BB, det_img, gts, gt_off)
    return _task1.pr_curve(ovmax, jmax, det_img, gt_off, difficult, npos, ovthresh, use_07_metric)


def evaluate(detpath, annopath, imagesetfile, classnames, ovthresh=0.5, use_07_metric=True):
    """The loop of main() (:245-268): per-class AP and their sum over len(classnames); no class is skipped (a missing result
    file raises, as there)."""
    classaps = []
    mean_ap = 0
    for classname in classnames:
        _, _, ap = voc_eval(detpath, annopath, imagesetfile, classname, ovthresh=ovthresh, use_07_metric=use_07_metric)
        mean_ap = mean_ap + ap
        classaps.append(ap)
    mean_ap = mean_ap / len(classnames)
    return mean_ap, 100 * np.array(classaps)
