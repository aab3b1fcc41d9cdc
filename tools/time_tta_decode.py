"""Augmented-inference decode timing: the eager chain against the one fused launch (profiles/tta_decode.md).
    python tools/time_tta_decode.py [--bs 1,16] [--windows 7] [--iters 10]

A 1024^2 image at scales 1 / 0.83 / 0.67 (inputs 1024, 864, 704), nc 18, fp16: synthetic conv outputs of the three passes.
  chain   what Model._forward_augment runs behind the backbone today: three eager Detect forwards (each writes z and the permuted
          raw head), then the reference's torch ops -- `/= scale`, the de-flip, the row-count clip, torch.cat;
  fused   ONE obb_detect_decode_tta launch on the surviving levels (models.yolo.forward_augment with Detect.fused_tta).
Both are timed with events on the stream, in windows of `iters` calls that rotate over enough input sets that more than 256 MB
pass between two uses of the same bytes; the figure is the median window.  The NMS is timed on each result: the chain's tensor
has lost the objectness column, the fused one carries it.  One JSON line at the end."""
import argparse
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn as nn

from tests import synth
from yolov5_obb_amd.models.yolo import Detect, _augment_chain, _decode_tta, tta_plan
from yolov5_obb_amd.utils.general import non_max_suppression_obb

ap = argparse.ArgumentParser()
ap.add_argument("--bs", default="1,16")
ap.add_argument("--windows", type=int, default=7)
ap.add_argument("--iters", type=int, default=10)
args = ap.parse_args()
assert args.windows >= 5

dev = torch.device("cuda:0")
NC, NA, DT = 18, 3, torch.float16
NO = NC + 185
IMG = (1024, 1024)
SCALES, FLIPS = (1, 0.83, 0.67), (None, 3, None)
MAPS = [[(n, n) for n in (128, 64, 32)], [(n, n) for n in (108, 54, 27)], [(n, n) for n in (88, 44, 22)]]
PASSES = list(zip(SCALES, FLIPS))
plan = tta_plan(MAPS, NA, 3)
assert plan.on_boundary and plan.a_total == 114627

det = Detect(nc=NC, anchors=synth.DEFAULT_ANCHORS, ch=(1, 1, 1))
det.stride = torch.tensor(synth.DEFAULT_STRIDES)
det.anchors /= det.stride.view(-1, 1, 1)
det.m = nn.ModuleList(nn.Identity() for _ in range(3))                 # the passes are handed their conv outputs
det = det.to(dev).to(DT).eval()

esz = 2
rows_all = [sum(NA * a * b for a, b in m) for m in MAPS]
rows_kept = [p.rows for p in plan.passes]
conv_all = sum(rows_all) * NO * esz
conv_kept = sum(rows_kept) * NO * esz
result = plan.a_total * NO * esz
# per image: what the chain moves (conv read, z and x written, the two strided read-modify-writes at 64-byte granularity, cat read
# + write) and what has to move (surviving conv outputs read once, the result and its column written once)
chain_bytes = conv_all + 2 * conv_all + 2 * 64 * (sum(rows_all) + rows_all[1]) + 2 * result
fused_bytes = conv_kept + result + plan.a_total * esz


def make_set(bs, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    out = []
    for m in MAPS:
        cs = []
        for ny, nx in m:
            c = torch.randn(bs, NA * NO, ny, nx, generator=g, device=dev, dtype=DT) * 2
            c.view(bs, NA, NO, ny, nx)[:, :, 4] -= 7           # few anchors above the confidence threshold, as in a real image
            cs.append(c)
        out.append(cs)
    return out


def chain(convs):
    y = [det(list(cs))[0] for cs in convs]
    return _augment_chain(y, PASSES, IMG[0], IMG[1], 3)


def fused(convs):
    return _decode_tta(det, convs, plan, SCALES, FLIPS, IMG[0], IMG[1])


def median_ms(fn, sets, windows, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    k, ms = 0, []
    for w in range(windows + 1):                                # (the first window warms up)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(iters):
            fn(sets[k % len(sets)])
            k += 1
        e1.record()
        torch.cuda.synchronize()
        if w:
            ms.append(e0.elapsed_time(e1) / iters)
    return statistics.median(ms), min(ms), max(ms)


res = {"what": "tta_decode", "image": IMG[0], "nc": NC, "dtype": "fp16", "a_total": plan.a_total,
       "chain_bytes_per_image": chain_bytes, "fused_bytes_per_image": fused_bytes,
       "predicted_ratio": round(chain_bytes / fused_bytes, 2), "windows": args.windows, "iters": args.iters}
kw = dict(conf_thres=0.25, iou_thres=0.4, multi_label=True)
with torch.no_grad():
    for bs in [int(b) for b in args.bs.split(",")]:
        nsets = max(2, math.ceil((256 << 20) / (conv_all * bs)) + 1)
        sets = [make_set(bs, 100 + i) for i in range(nsets)]
        zc, zf = chain(sets[0]), fused(sets[0])
        same = torch.equal(zc.view(torch.int16), zf.view(torch.int16))
        # interleaved: chain, fused, chain, fused -- a drift of the clocks meets both
        c1, f1 = median_ms(chain, sets, args.windows, args.iters), median_ms(fused, sets, args.windows, args.iters)
        c2, f2 = median_ms(chain, sets, args.windows, args.iters), median_ms(fused, sets, args.windows, args.iters)
        c_ms, f_ms = (c1[0] + c2[0]) / 2, (f1[0] + f2[0]) / 2
        nms_c = median_ms(lambda z: non_max_suppression_obb(z, **kw), [zc], args.windows, args.iters)
        nms_f = median_ms(lambda z: non_max_suppression_obb(z, **kw), [zf], args.windows, args.iters)
        res[f"bs{bs}"] = {"sets": nsets, "bit_equal": same, "chain_ms": round(c_ms, 4), "fused_ms": round(f_ms, 4),
                          "ratio": round(c_ms / f_ms, 2), "chain_ms_runs": [round(c1[0], 4), round(c2[0], 4)],
                          "fused_ms_runs": [round(f1[0], 4), round(f2[0], 4)],
                          "chain_window_min_max": [round(min(c1[1], c2[1]), 4), round(max(c1[2], c2[2]), 4)],
                          "fused_window_min_max": [round(min(f1[1], f2[1]), 4), round(max(f1[2], f2[2]), 4)],
                          "fused_GBps": round(fused_bytes * bs / f_ms / 1e6), "chain_GBps": round(chain_bytes * bs / c_ms / 1e6),
                          "nms_ms_no_column": round(nms_c[0], 4), "nms_ms_column": round(nms_f[0], 4),
                          "detections": int(sum(len(t) for t in non_max_suppression_obb(zf, **kw)))}
        print(f"bs {bs}: chain {c_ms:.3f} ms, fused {f_ms:.3f} ms ({c_ms / f_ms:.2f}x), NMS {nms_c[0]:.3f} -> {nms_f[0]:.3f} ms, "
              f"bit-equal {same}", flush=True)
        del sets, zc, zf
        torch.cuda.empty_cache()
print(json.dumps(res))
