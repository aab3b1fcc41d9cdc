"""Device ConfusionMatrix (obb_confusion_batch_f32, one launch) beside the val.py tail (obb_val_tail_batch_f32, two launches) on
the same inputs: python tools/time_confusion.py [out.json]
Two shapes: the bench's batch (tests/confusion_cases.py::timing_batch: 16 images, ~300 detections and ~50 labels each, 16
classes -- the input of tests/golden/gen_confusion_cases.py REF --time, which times the reference's per-image calls on the CPU)
and the dense batch of tests/test_valtail_dense_gpu.py (5 images, up to 1000 detections against 1500 labels).  Device events
around the call, warmed up, median of 15."""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from tests import confusion_cases as CC
from tests import valtail_cases as VC
from yolov5_obb_amd import _lib

NC, NIOU = 16, 10


def median_ms(fn, warm, reps):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def main():
    assert torch.cuda.is_available(), "time_confusion.py needs a GPU"
    dev = torch.device("cuda:0")
    L = _lib.lib()
    bench = CC.timing_batch()
    dense = VC.make_batch(*VC.CASES["dense"])
    out = {"cases": []}
    for name, (preds, targets, shapes) in (("bench batch", (bench["preds"], bench["targets"], bench["shapes"])), ("dense", dense)):
        counts = [p.shape[0] for p in preds]
        n, nt, bs = sum(counts), int(targets.shape[0]), len(preds)
        det = torch.cat(preds, 0).to(dev).contiguous()
        tg = targets.to(dev).contiguous()
        doff = (C.c_int64 * (bs + 1))(*np.concatenate(([0], np.cumsum(counts))).tolist())
        flat = []
        for shape, ratio_pad in shapes:
            flat += (ratio_pad[1][0], ratio_pad[1][1], ratio_pad[0][0], shape[1], shape[0])
        img5 = (C.c_float * len(flat))(*flat)
        iouv = torch.linspace(0.5, 0.95, NIOU, device=dev)
        stats = torch.empty((n, NIOU + 2), dtype=torch.float32, device=dev)
        mat = torch.zeros((NC + 1) ** 2 + 1, dtype=torch.int64, device=dev)
        ws_t = torch.empty(L.obb_val_tail_batch_workspace_bytes(n, nt), dtype=torch.uint8, device=dev)
        ws_c = torch.empty(L.obb_confusion_workspace_bytes(n, nt), dtype=torch.uint8, device=dev)
        st = _lib.stream_ptr(dev)
        doffp, img5p = C.cast(doff, C.c_void_p), C.cast(img5, C.c_void_p)

        def tail():
            rc = L.obb_val_tail_batch_f32(_lib.ptr(det), doffp, bs, _lib.ptr(tg), nt, int(tg.shape[1]), img5p, _lib.ptr(iouv), NIOU, None, None,
                                          None, None, _lib.ptr(stats), _lib.ptr(ws_t), ws_t.numel(), st)
            assert rc == 0, rc

        def confusion():
            rc = L.obb_confusion_batch_f32(_lib.ptr(det), doffp, bs, _lib.ptr(tg), nt, int(tg.shape[1]), img5p, NC, 0.25, 0.45, _lib.ptr(mat),
                                           _lib.ptr(ws_c), ws_c.numel(), st)
            assert rc == 0, rc
        t_med, t_lo, t_hi = median_ms(tail, 3, 15)
        c_med, c_lo, c_hi = median_ms(confusion, 3, 15)
        case = {"shape": name, "images": bs, "detections": n, "labels": nt, "most_detections": max(counts),
                "most_labels": int(torch.bincount(targets[:, 0].long()).max()), "classes": NC,
                "val_tail_ms_median": t_med, "val_tail_ms_min": t_lo, "val_tail_ms_max": t_hi,
                "confusion_ms_median": c_med, "confusion_ms_min": c_lo, "confusion_ms_max": c_hi}
        out["cases"].append(case)
        print(f"{name}: {bs} images, {n} detections, {nt} labels: obb_val_tail_batch_f32 {t_med * 1e3:.1f} us (min {t_lo * 1e3:.1f}, max "
              f"{t_hi * 1e3:.1f}); obb_confusion_batch_f32 {c_med * 1e3:.1f} us (min {c_lo * 1e3:.1f}, max {c_hi * 1e3:.1f})")
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
