#!/usr/bin/env python3
"""Detect -> non_max_suppression_obb per batch, eager (coupled, what bench.py's detect_nms_chain times) against Detect.lazy_nms (the
fused entry on the conv outputs, obb_non_max_suppression_obb_head), on bench.py's chain workload: tests/synth.py
s_head(16, 16, (128, 64, 32), seed=2000, n_obj=120) fp16, iou .45, multi_label, max_det 1500.  Prints one JSON line: ms per batch of
both chains, the front kernel's ms (library stage 0: k_decode, or k_decode_head on the lazy chain), and whether the detections are
identical.

usage: python tools/time_lazy_chain.py [--conf 0.25] [--steps 50] [--warmup 10]
       python tools/time_lazy_chain.py --pmc-run            (a few lazy calls only: the process to run under rocprofv3 --pmc)
       python tools/time_lazy_chain.py --pmc-csv DIR        (FETCH_SIZE of k_decode_head from rocprofv3's counter_collection.csv
                                                            under DIR, against the conv-output bytes)
"""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BS, NC, SIZES, NA = 16, 16, (128, 64, 32), 3
CONV_BYTES = BS * NA * (5 + NC + 180) * sum(n * n for n in SIZES) * 2


def setup(dev):
    import torch
    from tests import synth
    from yolov5_obb_amd.models.yolo import Detect
    det = Detect(nc=NC, anchors=synth.DEFAULT_ANCHORS, ch=(8, 8, 8))
    det.stride = torch.tensor(synth.DEFAULT_STRIDES)
    det.anchors /= det.stride.view(-1, 1, 1)
    det = det.to(dev).half().eval()
    det.m = torch.nn.ModuleList([torch.nn.Identity() for _ in range(3)])      # the conv outputs are the input
    heads = [h.to(dev) for h in synth.s_head(BS, NC, SIZES, seed=2000, n_obj=120, dtype=torch.float16)]
    return det, heads


def chain(det, heads, lazy, kw):
    import torch
    from yolov5_obb_amd.utils.general import non_max_suppression_obb
    det.lazy_nms = lazy
    with torch.no_grad():
        z, _ = det(list(heads))
        return non_max_suppression_obb(z, **kw)


def collect(L):
    ms, cnt = (C.c_double * 8)(), (C.c_int64 * 8)()
    assert L.obb_profile_collect(C.cast(ms, C.c_void_p), C.cast(cnt, C.c_void_p), 8) == 0
    return list(ms), list(cnt)


def timed(det, heads, lazy, kw, steps, warmup):
    import torch
    from yolov5_obb_amd import _lib
    L = _lib.lib()
    for _ in range(warmup):
        out = chain(det, heads, lazy, kw)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        out = chain(det, heads, lazy, kw)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    collect(L)                                                   # (drop anything recorded before)
    L.obb_profile_enable(1)                                      # stage events: a separate pass, they cost time themselves
    for _ in range(min(steps, 20)):
        chain(det, heads, lazy, kw)
    torch.cuda.synchronize()
    pm, pc = collect(L)
    L.obb_profile_enable(0)
    return ms, pm[0] / max(1, pc[0]), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--conf", type=float, default=0.25)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--pmc-run", action="store_true")
    ap.add_argument("--pmc-csv", default=None)
    a = ap.parse_args()
    if a.pmc_csv:
        vals = []
        for path in glob.glob(os.path.join(a.pmc_csv, "**", "*counter_collection.csv"), recursive=True):
            for r in csv.DictReader(open(path)):
                if "k_decode_head" in r.get("Kernel_Name", "") and r.get("Counter_Name") == "FETCH_SIZE":
                    vals.append(float(r["Counter_Value"]))
        # FETCH_SIZE is in KB and tallies wide (128-byte) coalesced requests at half their size on gfx950 (tools/pmc_json.py)
        fetch = [2 * v * 1024 for v in vals]
        res = {"kernel": "k_decode_head<__half>", "dispatches": len(vals), "conv_output_bytes": CONV_BYTES,
               "fetch_bytes_per_dispatch": [round(v) for v in fetch],
               "fetch_over_conv_bytes": [round(v / CONV_BYTES, 4) for v in fetch]}
        print(json.dumps(res))
        return
    import torch
    dev = torch.device("cuda:0")
    det, heads = setup(dev)
    kw = dict(conf_thres=a.conf, iou_thres=0.45, multi_label=True, max_det=1500)
    if a.pmc_run:
        for _ in range(3):
            chain(det, heads, True, kw)
        torch.cuda.synchronize()
        return
    det.couple_nms = True
    ms_e, dec_e, out_e = timed(det, heads, False, kw, a.steps, a.warmup)
    ms_l, dec_l, out_l = timed(det, heads, True, kw, a.steps, a.warmup)
    same = len(out_e) == len(out_l) and all(torch.equal(p, q) for p, q in zip(out_e, out_l))
    print(json.dumps({"workload": f"s_head(16, 16, (128, 64, 32), seed=2000, n_obj=120) fp16, conf {a.conf}, iou .45, multi_label, "
                                  "max_det 1500, per batch of 16",
                      "ms_eager_coupled": round(ms_e, 4), "ms_lazy": round(ms_l, 4),
                      "front_kernel_ms_eager_k_decode": round(dec_e, 4), "front_kernel_ms_lazy_k_decode_head": round(dec_l, 4),
                      "conv_output_bytes": CONV_BYTES, "front_GBs_if_conv_read_once": round(CONV_BYTES / (dec_l * 1e-3) / 1e9, 1),
                      "detections": sum(int(o.shape[0]) for o in out_l), "same_detections": bool(same)}))


if __name__ == "__main__":
    main()
