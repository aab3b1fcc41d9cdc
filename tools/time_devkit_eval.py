"""Task-2 voc_eval and mAOE aoe_eval of this package beside the reference formulation on the same files:
    python tools/time_devkit_eval.py [out.md]
The set: tests.golden.gen_golden.eval_inputs(1000, 14, 5) -- 1000 images, about 12,600 ground-truth quads and 20,000 detections
in two classes -- as Task-1 files for aoe_eval and through tests.devkit_eval_cases.to_task2 for voc_eval.  The reference
formulation is restated below from the devkit's description of itself: files read line by line, then one Python iteration per
detection with numpy calls on the boxes of its image (Task 2), or the horizontal-box gate plus one polygon-IoU call per surviving
box (mAOE; the SWIG polyiou module is not built here, the CPU oracle's double-precision quad IoU stands in for it).
Method: whole calls, host clock; the package's calls end in a device-to-host copy, i.e. synchronised.  Every shape is warmed up
once, then three runs, the two sides alternating inside a run and the ratio taken inside the run.  The C entry alone is timed
with device events around the call (median of 20): launch plus kernel, not a kernel-trace figure.  Outputs of the two sides are
compared before anything is timed.  Needs a GPU."""
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import oracle
from tests import devkit_eval_cases as DC
from tests.golden.gen_golden import EVAL_CLASSES, eval_inputs, eval_write
from yolov5_obb_amd import _lib
from yolov5_obb_amd.DOTA_devkit import dota_evaluation_task2 as T2
from yolov5_obb_amd.DOTA_devkit import mAOE_evaluation as MA
from yolov5_obb_amd.DOTA_devkit.dota_poly2rbox import poly2rbox_single_v3

SET = (1000, 14, 5)
RUNS = 3


def read_class(annopath, imagesetfile, classname, task2):
    with open(imagesetfile) as f:
        imagenames = [x.strip() for x in f.readlines()]
    recs, npos = {}, 0
    for imagename in imagenames:
        objs = [o for o in (T2.parse_gt if task2 else MA.parse_gt)(annopath.format(imagename)) if o['name'] == classname]
        difficult = np.array([o['difficult'] for o in objs]).astype(bool)
        npos += int(sum(~difficult))
        recs[imagename] = {'bbox': np.array([o['bbox'] for o in objs]), 'difficult': difficult, 'det': [False] * len(objs)}
    return recs, npos


def read_dets(detfile):
    with open(detfile) as f:
        rows = [x.strip().split(' ') for x in f.readlines()]
    ids = [x[0] for x in rows]
    conf = np.array([float(x[1]) for x in rows])
    BB = np.array([[float(z) for z in x[2:]] for x in rows])
    order = np.argsort(-conf)
    return [ids[i] for i in order], BB[order, :]


def hbb_overlaps(BBGT, bb):
    iw = np.maximum(np.minimum(BBGT[:, 2], bb[2]) - np.maximum(BBGT[:, 0], bb[0]) + 1., 0.)
    ih = np.maximum(np.minimum(BBGT[:, 3], bb[3]) - np.maximum(BBGT[:, 1], bb[1]) + 1., 0.)
    inters = iw * ih
    return inters / ((bb[2] - bb[0] + 1.) * (bb[3] - bb[1] + 1.) + (BBGT[:, 2] - BBGT[:, 0] + 1.) * (BBGT[:, 3] - BBGT[:, 1] + 1.) - inters)


def loop_voc_eval(detpath, annopath, imagesetfile, classname, ovthresh=0.5, use_07_metric=False):
    """Task-2 voc_eval, one iteration per detection."""
    recs, npos = read_class(annopath, imagesetfile, classname, True)
    ids, BB = read_dets(detpath.format(classname))
    nd = len(ids)
    tp, fp = np.zeros(nd), np.zeros(nd)
    for d in range(nd):
        R = recs[ids[d]]
        BBGT = R['bbox'].astype(float)
        ovmax = -np.inf
        if BBGT.size > 0:
            overlaps = hbb_overlaps(BBGT, BB[d, :].astype(float))
            ovmax, jmax = np.max(overlaps), np.argmax(overlaps)
        if ovmax > ovthresh:
            if not R['difficult'][jmax]:
                if not R['det'][jmax]:
                    tp[d] = 1.
                    R['det'][jmax] = 1
                else:
                    fp[d] = 1.
        else:
            fp[d] = 1.
    fp, tp = np.cumsum(fp), np.cumsum(tp)
    rec = tp / float(npos)
    prec = tp / np.maximum(tp + fp, np.finfo(np.float64).eps)
    return rec, prec, T2.voc_ap(rec, prec, use_07_metric)


def loop_aoe_eval(detpath, annopath, imagesetfile, classname, ovthresh=0.5):
    """mAOE aoe_eval, one iteration per detection, one polygon-IoU call per ground truth that passes the horizontal-box gate."""
    piou = oracle.lib().oracle_piou_f64
    recs, _ = read_class(annopath, imagesetfile, classname, False)
    ids, BB = read_dets(detpath.format(classname))
    out = []
    for d in range(len(ids)):
        BBGT = recs[ids[d]]['bbox'].astype(float)
        bb = BB[d, :].astype(float)
        if BBGT.size == 0:
            continue
        hull = np.stack([BBGT[:, 0::2].min(1), BBGT[:, 1::2].min(1), BBGT[:, 0::2].max(1), BBGT[:, 1::2].max(1)], 1)
        keep = BBGT[hbb_overlaps(hull, [bb[0::2].min(), bb[1::2].min(), bb[0::2].max(), bb[1::2].max()]) > 0, :]
        if len(keep) > 0:
            overlaps = [piou(np.ascontiguousarray(g), bb) for g in keep]
            if np.max(overlaps) > ovthresh:
                out.append(abs(poly2rbox_single_v3(bb)[-1] - poly2rbox_single_v3(keep[np.argmax(overlaps)])[-1]) * 57.32)
    return out


def entry_call_us(detpath, annopath, imagesetfile, classname, dev):
    """obb_eval_best_gt_hbb_f64 alone on the class's arrays: device events around the call (launch + kernel), median of 20 after
    3 warm-up calls."""
    with open(imagesetfile) as f:
        imagenames = [x.strip() for x in f.readlines()]
    index = {n: i for i, n in enumerate(imagenames)}
    gts, _, gt_off = T2.load_gt(annopath, imagenames, classname)
    ids, conf, BB = T2.read_detections(detpath.format(classname))
    order = np.argsort(-conf)
    d_det = torch.from_numpy(np.ascontiguousarray(BB[order])).to(dev)
    d_img = torch.from_numpy(np.array([index[ids[i]] for i in order], dtype=np.int32)).to(dev)
    d_gt, d_off = torch.from_numpy(gts).to(dev), torch.from_numpy(gt_off.astype(np.int32)).to(dev)
    ov, jm = torch.empty(len(order), dtype=torch.float64, device=dev), torch.empty(len(order), dtype=torch.int32, device=dev)

    def call():
        rc = _lib.lib().obb_eval_best_gt_hbb_f64(_lib.ptr(d_det), BB.shape[1], _lib.ptr(d_img), len(order), _lib.ptr(d_gt), _lib.ptr(d_off),
                                                 len(gt_off) - 1, _lib.ptr(ov), _lib.ptr(jm), _lib.stream_ptr(dev))
        assert rc == 0, rc
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    ts = []
    for _ in range(20):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); call(); b.record(); b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return float(np.median(ts)), len(order), int(gt_off[-1])


def timed(fn, *args, **kw):
    t0 = time.perf_counter()
    r = fn(*args, **kw)
    return time.perf_counter() - t0, r


def main():
    assert torch.cuda.is_available(), "time_devkit_eval.py needs a GPU"
    dev = torch.device("cuda:0")
    oracle.build(with_ref=False)
    gt1, det1 = eval_inputs(*SET)
    gt2, det2 = DC.to_task2(gt1, det1)
    rows = [f"# Task-2 voc_eval and mAOE aoe_eval: this package beside the per-detection loop\n",
            f"Device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; numpy {np.__version__}; {os.cpu_count()} host CPUs visible.",
            f"Set: eval_inputs{SET}: {len(gt1)} images, {sum(len(v) for v in gt1.values()) - len(gt1)} ground-truth boxes, "
            f"{sum(len(v) for v in det1.values())} detections.  Whole calls (files in, result out), host clock, one warm-up call, "
            f"{RUNS} runs with the two sides alternating; the ratio is loop / package inside a run.  Outputs compared first: equal.\n",
            "| call | class | detections | run | package ms | loop ms | loop / package |", "|---|---|---|---|---|---|---|"]
    with np.errstate(all='ignore'), tempfile.TemporaryDirectory() as td:
        p1 = eval_write(os.path.join(td, 't1'), gt1, det1)
        p2 = DC.task2_write(os.path.join(td, 't2'), gt2, det2)
        for cls in EVAL_CLASSES:
            a, b = T2.voc_eval(*p2, cls, ovthresh=0.5, use_07_metric=True), loop_voc_eval(*p2, cls, ovthresh=0.5, use_07_metric=True)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2], "voc_eval differs from the loop"
            for run in range(RUNS):
                tp, _ = timed(T2.voc_eval, *p2, cls, ovthresh=0.5, use_07_metric=True)
                tl, _ = timed(loop_voc_eval, *p2, cls, ovthresh=0.5, use_07_metric=True)
                rows.append(f"| Task-2 voc_eval | {cls} | {len(det2[cls])} | {run + 1} | {tp * 1e3:.1f} | {tl * 1e3:.1f} | {tl / tp:.1f} |")
                print(rows[-1], flush=True)
        for cls in EVAL_CLASSES:
            a, b = MA.aoe_eval(*p1, cls, ovthresh=0.7), loop_aoe_eval(*p1, cls, ovthresh=0.7)
            assert len(a) == len(b) and np.allclose(a, b, rtol=0, atol=1e-9), "aoe_eval differs from the loop"
            for run in range(RUNS):
                tp, _ = timed(MA.aoe_eval, *p1, cls, ovthresh=0.7)
                tl, _ = timed(loop_aoe_eval, *p1, cls, ovthresh=0.7)
                rows.append(f"| mAOE aoe_eval (0.7, {len(a)} hits) | {cls} | {len(det1[cls])} | {run + 1} | {tp * 1e3:.1f} | {tl * 1e3:.1f} | {tl / tp:.1f} |")
                print(rows[-1], flush=True)
        rows.append("\nobb_eval_best_gt_hbb_f64 alone (device events around the call: launch plus kernel, no kernel trace was taken; 3 warm-up calls, median of 20):\n")
        rows += ["| class | detections | boxes | event-timed call us |", "|---|---|---|---|"]
        for cls in EVAL_CLASSES:
            us, nd, ng = entry_call_us(*p2, cls, dev)
            rows.append(f"| {cls} | {nd} | {ng} | {us:.1f} |")
            print(rows[-1], flush=True)
    text = '\n'.join(rows) + '\n'
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
