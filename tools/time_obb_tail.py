"""Oriented-box validation tail timing (profiles/obb_tail.md).
    python tools/time_obb_tail.py [--windows 7] [--iters 10]

A val-shaped batch: 16 images, 150 .. 1500 detections and 60 .. 400 labels each, 3 classes, the detections jittered copies of
their labels (tests/valtail_cases.py).  Three paths on the same arrays:
  fused  obb_val_tail_batch_obb_f32: two launches, the rows [correct, conf, cls] and the match arrays stay on the device;
  hbb    obb_val_tail_batch_f32 without the box outputs: the horizontal tail the loop runs today (two launches);
  user   what gives the oriented `correct` without the fused tail: per image ops.rotated_iou_matrix(labels, detections) -- n x m
         pairs, the clip for every pair its reject does not prove disjoint -- and val.py:80-89 on the matrix (torch.where, one
         .cpu().numpy() round trip, numpy's argsort and two np.unique, the result back to the device).
Timed with events on the stream (the host time of `user` lies between them), in windows of `iters` calls, the median window;
fused / hbb / user interleaved twice so that a drift of the clocks meets all three.  Ratios are taken inside the run: the
machines of a pool differ by several per cent.  One JSON line at the end."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from tests import valtail_cases as VC
from yolov5_obb_amd import _lib, ops

ap = argparse.ArgumentParser()
ap.add_argument("--windows", type=int, default=7)
ap.add_argument("--iters", type=int, default=10)
args = ap.parse_args()
assert args.windows >= 5

dev = torch.device("cuda:0")
NIOU = 10
IMAGES = [(1500, 400, 3, 0, 0), (1200, 300, 3, 0, 0), (900, 350, 3, 0, 0), (700, 200, 3, 0, 0), (1500, 250, 3, 0, 0), (400, 120, 3, 0, 0),
          (300, 60, 3, 0, 0), (1000, 380, 3, 0, 0), (150, 90, 3, 0, 0), (800, 220, 3, 0, 0), (1300, 330, 3, 0, 0), (600, 180, 3, 0, 0),
          (1100, 270, 3, 0, 0), (500, 140, 3, 0, 0), (1400, 390, 3, 0, 0), (950, 240, 3, 0, 0)]
preds, targets, shapes = VC.make_batch(7, IMAGES)
bs = len(preds)
counts = [p.shape[0] for p in preds]
offs = np.cumsum([0] + counts).astype(np.int64)
n, nt = int(offs[-1]), int(targets.shape[0])
det = torch.cat(preds, 0).to(dev)
tg = targets.to(dev).contiguous()
iouv = VC.IOUV.to(dev)
img_dets = [det[offs[b]:offs[b + 1]] for b in range(bs)]
img_labs = [tg[tg[:, 0] == b][:, 1:7].contiguous() for b in range(bs)]

L = _lib.lib()
st = _lib.stream_ptr(dev)
doff = C.cast((C.c_int64 * (bs + 1))(*offs.tolist()), C.c_void_p)
flat = []
for shape, ratio_pad in shapes:
    flat += (ratio_pad[1][0], ratio_pad[1][1], ratio_pad[0][0], shape[1], shape[0])
img5 = C.cast((C.c_float * (5 * bs))(*flat), C.c_void_p)
stats_o = torch.zeros((n, NIOU + 2), device=dev)
stats_h = torch.zeros((n, NIOU + 2), device=dev)
match_label = torch.zeros(n, dtype=torch.int32, device=dev)
match_iou = torch.zeros(n, device=dev)
ws = torch.empty(L.obb_val_tail_batch_workspace_bytes(n, nt), dtype=torch.uint8, device=dev)
null = C.c_void_p(0)


def fused():
    rc = L.obb_val_tail_batch_obb_f32(_lib.ptr(det), null, doff, bs, _lib.ptr(tg), nt, tg.shape[1], _lib.ptr(iouv), NIOU, _lib.ptr(stats_o),
                                      _lib.ptr(match_label), _lib.ptr(match_iou), st)
    assert rc == 0


def hbb():
    rc = L.obb_val_tail_batch_f32(_lib.ptr(det), doff, bs, _lib.ptr(tg), nt, tg.shape[1], img5, _lib.ptr(iouv), NIOU, null, null, null, null,
                                  _lib.ptr(stats_h), _lib.ptr(ws), ws.numel(), st)
    assert rc == 0


def user_image(d, lab):
    """val.py:78-90 with iou = rotated_iou_matrix(labels, detections)."""
    correct = torch.zeros(d.shape[0], NIOU, dtype=torch.bool, device=dev)
    iou = ops.rotated_iou_matrix(lab[:, 1:6], d[:, :5])
    x = torch.where((iou >= iouv[0]) & (lab[:, 0:1] == d[:, 6]))
    if x[0].shape[0]:
        matches = torch.cat((torch.stack(x, 1), iou[x[0], x[1]][:, None]), 1).cpu().numpy()
        if x[0].shape[0] > 1:
            matches = matches[matches[:, 2].argsort()[::-1]]
            matches = matches[np.unique(matches[:, 1], return_index=True)[1]]
            matches = matches[np.unique(matches[:, 0], return_index=True)[1]]
        matches = torch.Tensor(matches).to(dev)
        correct[matches[:, 1].long()] = matches[:, 2:3] >= iouv
    return correct


def user():
    return [user_image(d, lab) for d, lab in zip(img_dets, img_labs)]


def median_ms(fn, windows, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for w in range(windows + 1):                                # (the first window warms up)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        if w:
            ms.append(e0.elapsed_time(e1) / iters)
    return statistics.median(ms), min(ms), max(ms)


fused()
hbb()
torch.cuda.synchronize()
got = stats_o[:, :NIOU] > 0.5
want = torch.cat(user(), 0)
same_rows = int((got == want).all(1).sum())
f1, h1, u1 = (median_ms(f, args.windows, args.iters) for f in (fused, hbb, user))
f2, h2, u2 = (median_ms(f, args.windows, args.iters) for f in (fused, hbb, user))
f_ms, h_ms, u_ms = (f1[0] + f2[0]) / 2, (h1[0] + h2[0]) / 2, (u1[0] + u2[0]) / 2
res = {"what": "obb_tail", "bs": bs, "detections": n, "labels": nt, "windows": args.windows, "iters": args.iters,
       "rows_equal_to_user": same_rows, "obb_correct_rows": int(got.any(1).sum()), "hbb_correct_rows": int((stats_h[:, :NIOU] > 0.5).any(1).sum()),
       "fused_ms": round(f_ms, 4), "hbb_ms": round(h_ms, 4), "user_ms": round(u_ms, 4),
       "fused_ms_runs": [round(f1[0], 4), round(f2[0], 4)], "hbb_ms_runs": [round(h1[0], 4), round(h2[0], 4)],
       "user_ms_runs": [round(u1[0], 4), round(u2[0], 4)],
       "fused_window_min_max": [round(min(f1[1], f2[1]), 4), round(max(f1[2], f2[2]), 4)],
       "user_window_min_max": [round(min(u1[1], u2[1]), 4), round(max(u1[2], u2[2]), 4)],
       "user_over_fused": round(u_ms / f_ms, 2), "fused_over_hbb": round(f_ms / h_ms, 2)}
print(f"bs {bs}, {n} detections, {nt} labels: fused {f_ms:.4f} ms, hbb {h_ms:.4f} ms ({f_ms / h_ms:.2f}x), user {u_ms:.3f} ms "
      f"({u_ms / f_ms:.1f}x of fused); rows equal to the user's {same_rows} / {n}", flush=True)
print(json.dumps(res))
