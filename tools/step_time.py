"""The headline step (bench.py's tensors: four rotated (16, 64512, 201) fp16 tensors) timed in windows of 200 calls, plus a
checksum of the outputs (development aid; A/B switches are read from the environment by the library).
    python tools/step_time.py [windows] [--dtype fp16,bf16] [--nc 16]
With several dtypes the windows alternate between them (one window of each in turn), so the columns are back to back."""
import argparse
import os, sys, time, hashlib
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from tests import synth
from yolov5_obb_amd.utils.general import non_max_suppression_obb
DTYPES = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
ap = argparse.ArgumentParser()
ap.add_argument("windows", nargs="?", type=int, default=5)
ap.add_argument("--dtype", default="fp16", help="comma list of fp32 / fp16 / bf16")
ap.add_argument("--nc", type=int, default=16)
args = ap.parse_args()
names = args.dtype.split(",")
dev = torch.device("cuda:0")
bs, A, nc = int(os.environ.get("BS", "16")), 64512, args.nc
kw = dict(conf_thres=0.25, iou_thres=0.45, multi_label=True, max_det=1500)
# one set of fp16 tensors (bench.py's), cast: every dtype sees the same scene
base = [synth.s_pred(bs, A, nc, seed=1000 + r, n_obj=120, fg_frac=0.03, device=dev, dtype=torch.float16) for r in range(4)]
preds = {k: [p.to(DTYPES[k]) for p in base] for k in names}
torch.cuda.synchronize()
sha, out = {}, {}
for k in names:
    h = hashlib.sha256()
    for p in preds[k]:
        for _ in range(3):
            out[k] = non_max_suppression_obb(p, **kw)
        for o in out[k]:
            h.update(o.cpu().numpy().tobytes())
    sha[k] = h.hexdigest()[:16]
    t_spin = time.perf_counter()
    i = 0
    while time.perf_counter() - t_spin < 0.4:
        out[k] = non_max_suppression_obb(preds[k][i % 4], **kw); i += 1
    torch.cuda.synchronize()
ws = {k: [] for k in names}
for w in range(args.windows):
    for k in names:
        t0 = time.perf_counter()
        for i in range(200):
            out[k] = non_max_suppression_obb(preds[k][i % 4], **kw)
        torch.cuda.synchronize()
        ws[k].append((time.perf_counter() - t0) / 200 * 1e3)
for k in names:
    print(f"{k + ' ' if len(names) > 1 else ''}step median {np.median(ws[k]):.4f} ms  windows {[round(w, 4) for w in ws[k]]}  rows {sum(int(o.shape[0]) for o in out[k])}  sha {sha[k]}  "
          f"[HELPERS={os.environ.get('OBB_NMS_SMALL_HELPERS', '-')} BS={bs} nc={nc}]", flush=True)
