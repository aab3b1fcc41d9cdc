"""Every *_workspace_bytes query of libobb_hip.so over a fixed grid of arguments, one line per query, and a SHA-256 digest of the
lines: python tools/ws_sizes.py [--lib path/to/libobb_hip.so] [--against earlier_output.txt]
The queries need no device.  Two digests: the five queries whose answers a refactor must not change (NMS, fused NMS and its
state, loss, AP) and the three of the val.py tail (head.hip).  Every point is asked with obb_nms_set_max_grid at 0 and at 8 (the
NMS sizes depend on the calling thread's grid cap).  --against prints the largest difference to the lines of an earlier run."""
import argparse
import ctypes as C
import hashlib
import itertools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HEAD = ("obb_val_tail_batch_workspace_bytes", "obb_process_batch_workspace_bytes", "obb_confusion_workspace_bytes")


def loss_configs():
    from tests import loss_cases as LC
    from yolov5_obb_amd.utils.loss import _LossConfig
    for name, (case, _) in LC.FIXTURE.items():      # the configurations of tests/golden/loss_configs.npz
        case = case or LC.nc1_class3_inputs()[0]
        c = _LossConfig()
        c.nl, c.na, c.nc, c.no, c.bs = case.nl, case.na, case.nc, case.no, case.bs
        for i, (ny, nx) in enumerate(case.sizes):
            c.ny[i], c.nx[i] = ny, nx
        yield name, c


def lines(L):
    i64, sz = C.c_int64, C.c_size_t
    for f, argt in (("obb_nms_workspace_bytes", (i64, i64, C.c_int)), ("obb_nms_obb_workspace_bytes", (i64, i64, i64, C.c_int)),
                    ("obb_nms_obb_state_bytes", (i64,)), ("obb_loss_workspace_bytes", (C.c_void_p, i64)),
                    ("obb_ap_per_class_workspace_bytes", (i64, C.c_int, C.c_int))) + tuple((h, (i64, i64)) for h in HEAD):
        getattr(L, f).restype, getattr(L, f).argtypes = sz, argt
    L.obb_nms_set_max_grid.argtypes = (C.c_int,)
    cfgs = list(loss_configs())
    for grid in (0, 8):
        L.obb_nms_set_max_grid(grid)
        q = lambda f, *a: f"{f} {' '.join(map(str, a))} grid={grid} -> {getattr(L, f)(*a)}"
        for n, nseg, kind in itertools.product((0, 1, 63, 64, 65, 8191, 8192, 16384, 32768, 100000), (1, 3, 64, 65), range(6)):
            yield q("obb_nms_workspace_bytes", n, nseg, kind)
        for bs, cap, nc, agn in itertools.product((1, 2, 16), (1, 64, 65, 4096), (1, 15, 256), (0, 1)):
            yield q("obb_nms_obb_workspace_bytes", bs, cap, nc, agn)
        for bs in (1, 2, 16):
            yield q("obb_nms_obb_state_bytes", bs)
        for (name, c), nt in itertools.product(cfgs, (0, 1, 205, 1024)):
            yield f"obb_loss_workspace_bytes {name} {nt} grid={grid} -> {L.obb_loss_workspace_bytes(C.byref(c), nt)}"
        for n, niou, nc_max in itertools.product((0, 1, 1023, 100000), (1, 10), (1, 16, 256)):
            yield q("obb_ap_per_class_workspace_bytes", n, niou, nc_max)
        for f, (n, nt) in itertools.product(HEAD, ((0, 0), (0, 1), (1, 0), (1, 1), (9, 5), (300, 40), (1000, 1500), (4800, 800), (100000, 3))):
            yield q(f, n, nt)
    L.obb_nms_set_max_grid(0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=os.path.join(ROOT, "yolov5_obb_amd", "libobb_hip.so"))
    ap.add_argument("--against")
    a = ap.parse_args()
    out = list(lines(C.CDLL(a.lib)))
    print("\n".join(out))
    for what, part in (("exact", [s for s in out if not s.startswith(HEAD)]), ("head", [s for s in out if s.startswith(HEAD)])):
        print(f"digest {what} ({len(part)} lines): {hashlib.sha256(chr(10).join(part).encode()).hexdigest()}")
    if a.against:
        size = lambda s: (s.split(" -> ")[0], int(s.split(" -> ")[1]))
        old = dict(size(s) for s in open(a.against).read().splitlines() if " -> " in s)
        diffs = [(size(s)[1] - old[size(s)[0]], s) for s in out]
        for what, part in (("exact", [d for d in diffs if not d[1].startswith(HEAD)]), ("head", [d for d in diffs if d[1].startswith(HEAD)])):
            print(f"{what}: largest increase {max(part)[0]} ({max(part)[1]}), largest decrease {-min(part)[0]} ({min(part)[1]})")


if __name__ == "__main__":
    main()
