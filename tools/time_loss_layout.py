"""Training-head timing: the eager permute copy against Detect.lazy_train (profiles/loss_layout.md).
    python tools/time_loss_layout.py [--steps 200] [--repeats 3] [--dtypes fp16,fp32] [--nts 50,1500] [--profile]

The project's training shape: bs 16, 1024^2, nc 16 (no 201), three levels of 128 / 64 / 32 cells, synthetic conv outputs.
  eager   conv outputs -> view / permute / contiguous (what Detect.forward does in training mode) -> ComputeLoss -> backward down
          to the gradient AT the conv outputs (autograd transposes the gradient back): what runs without the switch;
  lazy    the same with the permuted views (Detect.lazy_train): ComputeLoss reads the conv layout, the gradient is written in it.
Each leg is timed with device events around `steps` steps after a warm-up, the legs alternating, `repeats` times each; the figure
is the median repeat and the spread is max - min over a leg's own repeats.  The result of the two legs is compared bit for bit
first.  --profile runs a few steps of every configuration and nothing else: for `rocprofv3 --kernel-trace --stats -- python ...`.
One JSON line at the end."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from tests import synth
from yolov5_obb_amd.utils.loss import ComputeLoss

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--dtypes", default="fp16,fp32")
ap.add_argument("--nts", default="50,1500")
ap.add_argument("--profile", action="store_true")
args = ap.parse_args()
assert args.profile or (args.steps >= 200 and args.repeats >= 3)

dev = torch.device("cuda:0")
BS, NC, NA, IMG = 16, 16, 3, 1024
NO = NC + 185
GRIDS = [int(IMG / s) for s in synth.DEFAULT_STRIDES]
DT = {"fp16": torch.float16, "fp32": torch.float32}
ROWS = sum(BS * NA * n * n for n in GRIDS)

cl = ComputeLoss(synth.FakeModel(NC, synth.scaled_hyp(NC, IMG), dev))


def heads_of(convs, copy):
    v = [c.view(BS, NA, NO, c.shape[2], c.shape[3]).permute(0, 1, 3, 4, 2) for c in convs]
    return [x.contiguous() for x in v] if copy else v


def step(convs, t, copy):
    loss, _ = cl(heads_of(convs, copy), t)
    return loss, torch.autograd.grad(loss, convs)


def timed(convs, t, copy, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(args.warmup):
        step(convs, t, copy)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(steps):
        step(convs, t, copy)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


res = {"what": "loss_layout", "bs": BS, "image": IMG, "nc": NC, "rows": ROWS, "steps": args.steps, "repeats": args.repeats, "configs": {}}
for name in args.dtypes.split(","):
    dtype = DT[name]
    esz = torch.empty((), dtype=dtype).element_size()
    g = torch.Generator(device=dev).manual_seed(3)
    convs = [(torch.randn(BS, NA * NO, n, n, generator=g, device=dev, dtype=dtype)).requires_grad_(True) for n in GRIDS]
    for nt in [int(x) for x in args.nts.split(",")]:
        _, t = synth.s_loss(BS, NC, nt, seed=7, imgsz=IMG, sizes=[1, 1, 1])      # (only the targets: the logits are made on the device)
        t = t.to(dev)
        _, _, indices, _, _ = cl.build_targets(heads_of(convs, False), t)
        entries = sum(int(i[0].shape[0]) for i in indices)
        if args.profile:
            for copy in (True, False):
                for _ in range(5):
                    step(convs, t, copy)
            torch.cuda.synchronize()
            continue
        (le, ge), (lz, gz) = step(convs, t, True), step(convs, t, False)
        same = torch.equal(le, lz) and all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(ge, gz))
        del ge, gz
        eager, lazy = [], []
        for _ in range(args.repeats):                    # alternating: a drift of the clocks meets both legs
            eager.append(timed(convs, t, True, args.steps))
            lazy.append(timed(convs, t, False, args.steps))
        me, mz = statistics.median(eager), statistics.median(lazy)
        spread = max(eager) - min(eager)
        cfg = {"entries": entries, "bit_equal": same, "eager_ms": round(me, 4), "lazy_ms": round(mz, 4), "saved_ms": round(me - mz, 4),
               "eager_runs": [round(x, 4) for x in eager], "lazy_runs": [round(x, 4) for x in lazy], "eager_spread_ms": round(spread, 4),
               "lazy_not_slower": bool(mz <= me + spread),
               # bytes from shapes: each transposing copy reads and writes the heads once; an entry's row is read by the entry
               # kernels of the forward and the backward and written once (one element per 128-byte line in the conv layout)
               "copy_bytes": 4 * ROWS * NO * esz, "entry_row_bytes": 3 * entries * NO * esz, "entry_lines_conv": 3 * entries * NO}
        res["configs"][f"{name}_nt{nt}"] = cfg
        print(f"{name} nt {nt}: entries {entries}, eager {me:.3f} ms (spread {spread:.3f}), lazy {mz:.3f} ms, saved {me - mz:.3f} ms, "
              f"bit-equal {same}", flush=True)
    del convs
    torch.cuda.empty_cache()
print(json.dumps(res))
