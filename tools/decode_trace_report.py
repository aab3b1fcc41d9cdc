"""Per-workgroup timeline of k_decode on the bench batch, from the stamps a -DOBB_DECODE_TRACE library keeps (tools/decode_trace.sh).

Prints a markdown report: for cold (four tensors rotated, as bench.py does) and warm (one tensor) input, with and without the dense
objectness column, the median and the slowest workgroup's time in every interval of the kernel's chain, and the spread of n_rows."""
import ctypes as C, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from tests import synth
from yolov5_obb_amd import _lib
from yolov5_obb_amd.utils.general import non_max_suppression_obb

WGS, WORDS = 2048, 16
CALLS = int(os.environ.get("CALLS", "6"))      # traced calls per case (after the warm-up that settles the shape's hints)
dev = torch.device("cuda:0")
assert _lib.compiled() is not None, "the compiled binding is the bench's path (caller-kept counters)"
L = C.CDLL(_lib.LIB_PATH)
preds = [synth.s_pred(16, 64512, 16, seed=1000 + r, n_obj=120, fg_frac=0.03, device=dev, dtype=torch.float16) for r in range(4)]
kw = dict(conf_thres=0.25, iou_thres=0.45, multi_label=True, max_det=1500)
us = lambda x: x / 100.0                       # wall_clock64: 100 MHz

# (name, first stamp, last stamp) -- stamp words: 1 entry, 2 first barrier, 3 / 4 objectness used by the first / last wave,
# 5 list built, 6 / 7 rows reduced by the first / last wave, 8 slot atomic returned, 9 exit.  (The objectness loads and the zeroing
# stores are issued in front of the first barrier: `entry -> first barrier` holds what the barrier waits of them.)
INTERVALS = [("entry -> first barrier", 1, 2), ("first barrier -> objectness, first wave", 2, 3),
             ("first barrier -> objectness, last wave", 2, 4), ("objectness, last wave -> list built", 4, 5),
             ("list built -> rows reduced, first wave", 5, 6), ("list built -> rows reduced, last wave", 5, 7),
             ("rows, last wave -> slot atomic returned", 7, 8), ("slot atomic -> exit (write_out)", 8, 9), ("entry -> exit", 1, 9)]


def read_trace():
    w = np.zeros(WGS * WORDS, dtype=np.uint64)
    rc = L.obb_debug_decode_trace(w.ctypes.data_as(C.c_void_p))
    assert rc == 0, rc
    w = w.reshape(WGS, WORDS).astype(np.int64)
    return w[w[:, 0] == 1]


def tag_objcol(p):
    p._obb_objcol = (p[..., 4].contiguous(), p._version)


def case(title, tensors):
    for i in range(8):
        non_max_suppression_obb(tensors[i % len(tensors)], **kw)
    torch.cuda.synchronize()
    read_trace()
    runs = []
    for i in range(CALLS):
        non_max_suppression_obb(tensors[i % len(tensors)], **kw)
        torch.cuda.synchronize()
        runs.append(read_trace())
    print(f"\n## {title}\n")
    span = sorted(us(r[:, 9].max() - r[:, 1].min()) for r in runs)
    skew = sorted(us(r[:, 1].max() - r[:, 1].min()) for r in runs)
    print(f"{len(runs[-1])} workgroups; kernel span (first entry -> last exit) over {CALLS} calls: median {span[len(span) // 2]:.1f} us "
          f"(min {span[0]:.1f}, max {span[-1]:.1f}); entry skew median {skew[len(skew) // 2]:.1f} us\n")
    print("| interval | median workgroup, us | slowest workgroup, us |\n|---|---|---|")
    for name, a, b in INTERVALS:
        med = sorted(float(np.median(us(r[:, b] - r[:, a]))) for r in runs)
        mx = sorted(float(us((r[:, b] - r[:, a]).max())) for r in runs)
        print(f"| {name} | {med[len(med) // 2]:.1f} | {mx[len(mx) // 2]:.1f} |")
    r = runs[-1]
    nr, st = np.sort(r[:, 10]), np.sort(r[:, 11])
    print(f"\nn_rows per workgroup (last call): min {nr[0]} median {nr[len(nr) // 2]} p90 {nr[int(len(nr) * .9)]} max {nr[-1]}, sum {nr.sum()}; "
          f"candidates: median {st[len(st) // 2]} max {st[-1]}, sum {st.sum()}")


print(f"# k_decode stamps, bench batch (16, 64512, 201) fp16, library {os.path.basename(_lib.LIB_PATH)}")
case("cold (four tensors rotated), strided objectness", preds)
case("warm (one tensor), strided objectness", preds[:1])
for p in preds:
    tag_objcol(p)
case("cold (four tensors rotated), dense objectness column", preds)
case("warm (one tensor), dense objectness column", preds[:1])
