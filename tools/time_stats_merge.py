"""End-of-run cost of multi-rank validation metrics at DOTA-val size: python tools/time_stats_merge.py [out.json]
One process, W = 8 virtual ranks (strided split), 5,297 images with 100 .. 500 detection rows and 0 .. 60 labels each, 16 classes,
10 IoU levels.  Two routes over the same statistics, timed in the same run (wall clock around a device synchronise, warmed up,
median of the repeats):

  device   val.ValStats.merged(parts) + ap_per_class(): three obb_stats_merge_f32 calls and one obb_ap_per_class_f32, the rows
           never leave the device (between processes the exchange adds one all-gather of the same bytes)
  host     the route val_sharded.run takes without device_metrics: the per-image (correct, conf, pcls, tcls) tuples, already on
           the host, through shard.gather_results into image order -- the tuples of the seven other ranks pickled and unpickled
           as gather_object does -- then np.concatenate and ap_per_class on the CPU.  The CPU metric here is the host build of
           csrc/ap_math.h (tests/native/host_ap_math.cpp), compiled C++ that stands in for the reference's numpy function, which
           is slower: the ratio errs in the host route's favour.

Both routes must agree on AP (to 1e-12, the bound of tests/test_ap_math_host.py for the host build); the tool checks it."""
import ctypes as C
import json
import os
import pickle
import subprocess
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from yolov5_obb_amd import val as V
from yolov5_obb_amd.utils import shard

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NIOU, NC, WORLD, IMAGES, NC_MAX = 10, 16, 8, 5297, 256


def image(i):
    """(rows (c, NIOU + 2) float32, tcls (l) float32) of image i: correct falls with the IoU level, two-decimal confidences (ties)."""
    rng = np.random.RandomState(i)
    c, l = int(rng.randint(100, 501)), int(rng.randint(0, 61))
    level = rng.randint(0, NIOU + 1, size=c) * (rng.rand(c) < 0.4)
    rows = np.zeros((c, NIOU + 2), dtype=np.float32)
    rows[:, :NIOU] = np.arange(NIOU)[None, :] < level[:, None]
    rows[:, NIOU] = np.round(rng.rand(c), 2)
    rows[:, NIOU + 1] = rng.randint(0, NC, size=c)
    return rows, rng.randint(0, NC, size=l).astype(np.float32)


def accumulator(dev, ids, per_image):
    """A ValStats holding the images `ids` as add_batch would have left them."""
    vs = V.ValStats(niou=NIOU, device=dev, capacity=1)
    rows = np.concatenate([per_image[i][0] for i in ids], 0)
    tcls = np.concatenate([per_image[i][1] for i in ids], 0)
    vs._rows, vs.n = torch.from_numpy(rows).to(dev), len(rows)
    vs._tcls, vs.m = torch.from_numpy(tcls).to(dev), len(tcls)
    vs._img_rows = torch.tensor([len(per_image[i][0]) for i in ids], dtype=torch.int32, device=dev)
    vs._img_labels = torch.tensor([len(per_image[i][1]) for i in ids], dtype=torch.int32, device=dev)
    vs._img_ids, vs.k = torch.tensor(list(ids), dtype=torch.int64, device=dev), len(ids)
    return vs


def host_metric():
    d = tempfile.mkdtemp()
    out = os.path.join(d, "libhostap.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", f"-I{ROOT}/yolov5_obb_amd/csrc",
                    f"{ROOT}/tests/native/host_ap_math.cpp", "-o", out, "-lm"], check=True)
    L = C.CDLL(out)
    f32, f64 = (np.ctypeslib.ndpointer(dtype=t, flags="C_CONTIGUOUS") for t in (np.float32, np.float64))
    i32, u8 = (np.ctypeslib.ndpointer(dtype=t, flags="C_CONTIGUOUS") for t in (np.int32, np.uint8))
    L.hc_ap_per_class.argtypes = [u8, f32, f32, C.c_long, C.c_int, f32, C.c_long, C.c_int, f64, f64, i32, i32]
    L.hc_ap_per_class.restype = C.c_int

    def ap_per_class(tp, conf, pcls, tcls):
        ap, prf = np.zeros((NC_MAX, tp.shape[1])), np.zeros((NC_MAX, 5))
        counts, info = np.zeros((2, NC_MAX), np.int32), np.zeros(4, np.int32)
        assert L.hc_ap_per_class(np.ascontiguousarray(tp, dtype=np.uint8), conf, pcls, len(conf), tp.shape[1], tcls, len(tcls), NC_MAX, ap, prf,
                                 counts, info) == 0
        return ap[np.flatnonzero(counts[0] > 0)]
    return ap_per_class


def median_s(fn, warm, reps):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def main():
    assert torch.cuda.is_available(), "time_stats_merge.py needs a GPU"
    dev = torch.device("cuda:0")
    per_image = [image(i) for i in range(IMAGES)]
    parts = [accumulator(dev, list(range(r, IMAGES, WORLD)), per_image) for r in range(WORLD)]
    tuples = [[(torch.from_numpy(per_image[i][0][:, :NIOU] > 0.5), torch.from_numpy(per_image[i][0][:, NIOU].copy()),
                torch.from_numpy(per_image[i][0][:, NIOU + 1].copy()), per_image[i][1].tolist()) for i in range(r, IMAGES, WORLD)] for r in range(WORLD)]
    metric = host_metric()
    res = {}

    def device_route():
        mg = V.ValStats.merged(parts)
        res["device"] = mg.ap_per_class()[5]

    def host_route():
        full = [None] * IMAGES
        for r in range(WORLD):
            idx = list(range(r, IMAGES, WORLD))
            payload = (idx, tuples[r])
            if r:                                                  # what gather_object does to another rank's share
                payload = pickle.loads(pickle.dumps(payload))
            for i, t in zip(*payload):
                full[i] = t
        full = shard.gather_results(list(range(IMAGES)), full, IMAGES)
        cols = [np.concatenate([np.asarray(x) for x in col], 0) for col in zip(*full)]
        res["host"] = metric(cols[0], cols[1].astype(np.float32), cols[2].astype(np.float32), cols[3].astype(np.float32))

    dm = median_s(device_route, 2, 7)
    hm = median_s(host_route, 1, 5)
    assert np.array_equal(res["device"], res["host"]) or np.abs(res["device"] - res["host"]).max() <= 1e-12, "the routes disagree on AP"
    n, m = sum(p.n for p in parts), sum(p.m for p in parts)
    out = {"world": WORLD, "images": IMAGES, "rows": n, "labels": m, "device_s_median": dm[0], "device_s_min": dm[1], "device_s_max": dm[2],
           "host_s_median": hm[0], "host_s_min": hm[1], "host_s_max": hm[2], "host_over_device": hm[0] / dm[0],
           "mAP50": float(res["device"][:, 0].mean())}
    print(f"{IMAGES} images, {n} rows, {m} labels, {WORLD} virtual ranks: merged + ap_per_class {dm[0] * 1e3:.2f} ms (min {dm[1] * 1e3:.2f}, max "
          f"{dm[2] * 1e3:.2f}); host route {hm[0] * 1e3:.1f} ms (min {hm[1] * 1e3:.1f}, max {hm[2] * 1e3:.1f}); host / device = {hm[0] / dm[0]:.1f}; "
          f"mAP@0.5 {out['mAP50']:.6f}")
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
