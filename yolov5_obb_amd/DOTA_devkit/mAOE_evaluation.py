"""Mean angle-orientation error (the reference's DOTA_devkit/mAOE_evaluation.py): `parse_gt`, `aoe_eval`, `evaluate` = its
main loop, same file formats.

The det x GT part of aoe_eval (:113-161) -- the horizontal-box gate, `polyiou.iou_poly(GT, det)` for the survivors, np.max /
np.argmax -- is the Task-1 evaluation's, so it is the same device call (`dota_evaluation_task1.best_gt`).  What follows is
O(hits) and elementwise and stays on the host in numpy: `poly2rbox_single_v3` of a hit and of its ground truth
(dota_poly2rbox.poly2rbox_v3, bit-identical rows) and `abs(angle difference) * 57.32`.  Unlike voc_eval there is no difficult
filter and no once-only claim: every detection above the threshold contributes.  The angles are not wrapped: differences
near 180 degrees are the reference's behaviour.  GPU only.
"""
import numpy as np

from . import dota_evaluation_task1 as _task1
from .dota_evaluation_task1 import parse_gt  # noqa: F401  (:14-45 reads what Task 1's parse_gt reads)
from .dota_poly2rbox import poly2rbox_v3


def aoe_eval(detpath, annopath, imagesetfile, classname, ovthresh=0.5):
    """:48-171.  The angle errors (degrees, by the reference's factor 57.32) of the detections of one class whose best
    ground truth overlaps them by more than ovthresh, in confidence order."""
    with open(imagesetfile, 'r') as f:
        imagenames = [x.strip() for x in f.readlines()]
    index = {imagename: i for i, imagename in enumerate(imagenames)}
    fast = _task1.load_gt(annopath, imagenames, classname)
    if fast is not None:
        gts, gt_off = fast[0], fast[2]
    else:
        gts, gt_off = [], [0]
        for imagename in imagenames:
            gts.extend(o['bbox'] for o in parse_gt(annopath.format(imagename)) if o['name'] == classname)
            gt_off.append(len(gts))
        gts, gt_off = np.array(gts, dtype=np.float64).reshape(-1, 8), np.array(gt_off, dtype=np.int64)

    image_ids, confidence, BB = _task1.read_detections(detpath.format(classname))
    sorted_ind = np.argsort(-confidence)                 # :103
    BB = BB[sorted_ind, :]
    det_img = np.array([index[image_ids[x]] for x in sorted_ind], dtype=np.int32)

    ovmax, jmax = _task1.best_gt(BB, det_img, gts, gt_off)
    h = np.nonzero(ovmax > ovthresh)[0]                  # NaN and -inf: no contribution (:160)
    if len(h) == 0:
        return []
    angle_gt = poly2rbox_v3(gts[gt_off[det_img[h]] + jmax[h]])[:, 4]
    angle_bb = poly2rbox_v3(BB[h])[:, 4]
    return (np.abs(angle_bb - angle_gt) * 57.32).tolist()


def evaluate(detpath, annopath, imagesetfile, classnames, ovthresh=0.7):
    """The loop of main() (:191-209): the mean error per class (added up in list order) and the mean of those.  A class
    without a contributing detection raises ZeroDivisionError, as there."""
    class_means = []
    for classname in classnames:
        angle_dif_list = aoe_eval(detpath, annopath, imagesetfile, classname, ovthresh=ovthresh)
        angle_dif = 0.0
        for item in angle_dif_list:
            angle_dif = angle_dif + item
        class_means.append(angle_dif / len(angle_dif_list))
    total = 0.0
    for m in class_means:
        total = total + m
    return total / len(class_means), class_means
