"""Device ap_per_class (obb_ap_per_class_f32) at validation scale: python tools/time_metrics.py [out.json]
n = 200,000 and 4,000,000 rows, 16 classes, 10 IoU levels (tests/ap_cases.py::timing_inputs, the inputs of
tests/golden/gen_ap_cases.py REF --time, which times the reference's numpy function on the CPU).  Device events around the call,
warmed up, median of the repeats; the stats bytes it must read (n * (niou + 2) * 4) over that time, as a fraction of the copy
rate measured here (a device-to-device copy of 1 GiB counts its bytes once read, once written)."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from tests import ap_cases
from yolov5_obb_amd import _lib
from yolov5_obb_amd.utils import metrics

NIOU, NC = 10, 16


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
    assert torch.cuda.is_available(), "time_metrics.py needs a GPU"
    dev = torch.device("cuda:0")
    L = _lib.lib()
    src = torch.empty(1 << 28, dtype=torch.float32, device=dev).normal_()
    dst = torch.empty_like(src)
    copy_ms = median_ms(lambda: dst.copy_(src), 3, 15)[0]
    copy_rate = 2 * src.numel() * 4 / (copy_ms * 1e-3)                    # bytes / s, read + write
    del src, dst
    out = {"copy_GBps": copy_rate / 1e9, "cases": []}
    print(f"device copy: {copy_rate / 1e9:.0f} GB/s (read + write)")
    for n in (200_000, 4_000_000):
        tp, conf, pcls, tcls = ap_cases.timing_inputs(n, NC, NIOU)
        rows = torch.from_numpy(np.concatenate((tp.astype(np.float32), conf[:, None], pcls[:, None]), 1)).to(dev)
        tc = torch.from_numpy(tcls).to(dev)
        res = torch.empty(metrics.NC_MAX * (NIOU + 5 + 1) + 2, dtype=torch.float64, device=dev)
        o1, o2, o3 = metrics.NC_MAX * NIOU, metrics.NC_MAX * (NIOU + 5), metrics.NC_MAX * (NIOU + 6)
        ws = torch.empty(L.obb_ap_per_class_workspace_bytes(n, NIOU, metrics.NC_MAX), dtype=torch.uint8, device=dev)
        st = _lib.stream_ptr(dev)

        def call():
            rc = L.obb_ap_per_class_f32(_lib.ptr(rows), NIOU + 2, n, NIOU, _lib.ptr(tc), len(tcls), metrics.NC_MAX, _lib.ptr(res[:o1]),
                                        _lib.ptr(res[o1:o2]), _lib.ptr(res[o2:o3]), _lib.ptr(res[o3:]), None, _lib.ptr(ws), ws.numel(), st)
            assert rc == 0, rc
        med, lo, hi = median_ms(call, 3, 15)
        stats_bytes = n * (NIOU + 2) * 4
        rate = stats_bytes / (med * 1e-3)
        ap = res[:o1].cpu().numpy().reshape(-1, NIOU)[:NC]
        case = {"n": n, "classes": NC, "niou": NIOU, "device_ms_median": med, "device_ms_min": lo, "device_ms_max": hi,
                "stats_bytes": stats_bytes, "stats_GBps": rate / 1e9, "fraction_of_copy_rate": rate / copy_rate,
                "workspace_MiB": ws.numel() / 2 ** 20, "mAP50": float(ap[:, 0].mean())}
        out["cases"].append(case)
        print(f"n = {n}: obb_ap_per_class_f32 {med:.3f} ms (min {lo:.3f}, max {hi:.3f}); stats {stats_bytes / 1e6:.1f} MB -> "
              f"{rate / 1e9:.1f} GB/s = {100 * rate / copy_rate:.2f} % of the copy rate; workspace {ws.numel() / 2 ** 20:.0f} MiB; mAP@0.5 {ap[:, 0].mean():.6f}")
        del rows, ws
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
