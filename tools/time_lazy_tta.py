"""Augmented inference behind the conv outputs: the eager chain against the lazy call (profiles/lazy_tta.md).
    python tools/time_lazy_tta.py [--bs 1,16] [--windows 7] [--iters 10] [--runs 3]

The workload of tools/time_tta_decode.py: a 1024^2 image at scales 1 / 0.83 / 0.67 (inputs 1024, 864, 704), nc 18, fp16, synthetic
conv outputs of the three passes (tests/synth.py s_head: planted objects on a background whose objectness logit is N(-6, 1.5));
the NMS arguments of bench.py's TTA object: conf 0.01, iou 0.4, multi-label, max_det 1500.
  (a) chain   what Detect.fused_tta runs today: ONE obb_detect_decode_tta launch that writes z (bs, 114627, 203) and its objectness
              column, then non_max_suppression_obb on that tensor;
  (b) lazy    Detect.lazy_tta: non_max_suppression_obb on the lazy output -- obb_non_max_suppression_obb_tta_head reads the conv
              outputs, z is never written.
Both are timed from the host with the call's own completion (non_max_suppression_obb returns when its counters are on the host),
in windows of `iters` calls that rotate over enough input sets that more than 256 MB pass between two uses of the same bytes; the
figure of a run is the median window, and a run interleaves (a) and (b).  `--runs` runs in this process; the ratio is taken inside
each run (the machines of a pool differ by several per cent).  The front kernel alone: OBB_PROFILE-style stage timers of the library
(obb_profile_enable / obb_profile_collect, stage 0 = the filter kernel).  One JSON line at the end."""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn as nn

from tests import synth
from yolov5_obb_amd import _lib
from yolov5_obb_amd.models.yolo import Detect, _decode_tta, _lazy_tta_output, tta_plan
from yolov5_obb_amd.utils.general import non_max_suppression_obb

ap = argparse.ArgumentParser()
ap.add_argument("--bs", default="1,16")
ap.add_argument("--windows", type=int, default=7)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--runs", type=int, default=3)
args = ap.parse_args()
assert args.windows >= 5 and args.runs >= 1

dev = torch.device("cuda:0")
NC, NA, DT = 18, 3, torch.float16
NO = NC + 185
IMG = (1024, 1024)
SCALES, FLIPS = (1, 0.83, 0.67), (None, 3, None)
SIZES = [(128, 64, 32), (108, 54, 27), (88, 44, 22)]
MAPS = [[(n, n) for n in s] for s in SIZES]
plan = tta_plan(MAPS, NA, 3)
assert plan.on_boundary and plan.a_total == 114627
KW = dict(conf_thres=0.01, iou_thres=0.4, multi_label=True, max_det=1500)

det = Detect(nc=NC, anchors=synth.DEFAULT_ANCHORS, ch=(1, 1, 1))
det.stride = torch.tensor(synth.DEFAULT_STRIDES)
det.anchors /= det.stride.view(-1, 1, 1)
det.m = nn.ModuleList(nn.Identity() for _ in range(3))
det = det.to(dev).to(DT).eval()

esz = 2
conv_kept = plan.a_total * NO * esz                                    # the surviving conv outputs, read once
conv_all = sum(NA * n * n for s in SIZES for n in s) * NO * esz


def make_set(bs, seed):
    return [[c.to(dev) for c in synth.s_head(bs, NC, s, seed=seed + 7 * k, n_obj=120, dtype=DT)] for k, s in enumerate(SIZES)]


def chain(convs):
    return non_max_suppression_obb(_decode_tta(det, convs, plan, SCALES, FLIPS, IMG[0], IMG[1]), **KW)


def lazy(convs):
    return non_max_suppression_obb(_lazy_tta_output(det, convs, plan, SCALES, FLIPS, IMG[0], IMG[1]), **KW)


def median_ms(fn, sets, windows, iters):
    k, ms = 0, []
    for w in range(windows + 1):                                       # (the first window warms up)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn(sets[k % len(sets)])
            k += 1
        torch.cuda.synchronize()
        if w:
            ms.append((time.perf_counter() - t0) * 1e3 / iters)
    return statistics.median(ms), min(ms), max(ms)


def front_ms(fn, sets, iters):
    """Mean time of the filter kernel (stage 0 of the library's stage timers) over `iters` calls."""
    L = _lib.lib()
    for s in sets[:2]:
        fn(s)
    L.obb_profile_enable(1)
    for i in range(iters):
        fn(sets[i % len(sets)])
    torch.cuda.synchronize()
    ms, cnt = (C.c_double * 8)(), (C.c_int64 * 8)()
    L.obb_profile_collect(ms, cnt, 8)
    L.obb_profile_enable(0)
    return round(ms[0] / cnt[0], 4) if cnt[0] else None


res = {"what": "lazy_tta", "image": IMG[0], "nc": NC, "dtype": "fp16", "a_total": plan.a_total, "kw": KW,
       "conv_kept_bytes_per_image": conv_kept, "z_bytes_per_image": conv_kept, "windows": args.windows, "iters": args.iters, "runs": args.runs}
with torch.no_grad():
    for bs in [int(b) for b in args.bs.split(",")]:
        nsets = max(2, math.ceil((256 << 20) / (conv_all * bs)) + 1)
        sets = [make_set(bs, 100 + i) for i in range(nsets)]
        a, b = chain(sets[0]), lazy(sets[0])
        same = len(a) == len(b) and all(torch.equal(p, q) for p, q in zip(a, b))
        z = _decode_tta(det, sets[0], plan, SCALES, FLIPS, IMG[0], IMG[1])
        cand = int((((z[..., 5:5 + NC] * z[..., 4:5]) > KW["conf_thres"]) & (z[..., 4:5] > KW["conf_thres"])).sum())
        rows = int((z[..., 4] > KW["conf_thres"]).sum())
        del z
        runs = []
        for r in range(args.runs):
            c1, l1 = median_ms(chain, sets, args.windows, args.iters), median_ms(lazy, sets, args.windows, args.iters)
            c2, l2 = median_ms(chain, sets, args.windows, args.iters), median_ms(lazy, sets, args.windows, args.iters)
            c_ms, l_ms = (c1[0] + c2[0]) / 2, (l1[0] + l2[0]) / 2
            runs.append({"chain_ms": round(c_ms, 4), "lazy_ms": round(l_ms, 4), "ratio": round(c_ms / l_ms, 3),
                         "chain_window_min_max": [round(min(c1[1], c2[1]), 4), round(max(c1[2], c2[2]), 4)],
                         "lazy_window_min_max": [round(min(l1[1], l2[1]), 4), round(max(l1[2], l2[2]), 4)]})
            print(f"bs {bs} run {r}: chain {c_ms:.3f} ms, lazy {l_ms:.3f} ms ({c_ms / l_ms:.3f}x)", flush=True)
        ratios = [x["ratio"] for x in runs]
        res[f"bs{bs}"] = {"sets": nsets, "results_equal": same, "rows_passing_obj": rows, "candidates": cand,
                          "detections": int(sum(len(t) for t in a)), "runs": runs, "ratio_median": statistics.median(ratios),
                          "ratio_min_max": [min(ratios), max(ratios)],
                          "front_ms_chain_k_decode": front_ms(chain, sets, 2 * args.iters),
                          "front_ms_lazy_k_decode_head_tta": front_ms(lazy, sets, 2 * args.iters)}
        print(f"bs {bs}: ratio median {res[f'bs{bs}']['ratio_median']}, results equal {same}, candidates {cand}", flush=True)
        del sets
        torch.cuda.empty_cache()
print(json.dumps(res))
