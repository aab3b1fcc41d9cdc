"""GPU: the zeroing contract of the fused driver with caller-kept counters (obb_non_max_suppression_obb_st and the _head entry with
`state`): the call's first kernel zeroes the state of the later launches that the call's OWN path reads (csrc/nms_plan.h:
zero_bar / zero_alive) and nothing else, so no call may depend on what an earlier call of another path left in the workspace.

One workspace and one state block serve a sequence of calls that alternates between the small-segment path (which reads neither the
persistent kernel's barrier block nor the alive bitmap) and the two paths that take the persistent kernel (in-LDS sort: both blocks;
un-hinted radix sort: the barrier block).  Before every call after the first the test overwrites the WHOLE workspace -- so the
barrier and alive regions wherever the call's carve puts them -- with 0xA5.  Every call must give the oracle's rows and must not
report the abort status (out_count = -1)."""
import ctypes as C

import pytest
import torch

from oracle import pyref
from tests import synth

pytestmark = pytest.mark.gpu

MAX_DET = 300
SMALL = 6144 | (1 << 32)            # in-LDS regime, largest segment "1": the small-segment kernel
PERSIST_LDS = 6144 | (1000 << 32)   # in-LDS sort, a segment above the small-segment kernel's 384: the persistent kernel
UNHINTED = 0                        # radix sort + the persistent kernel


def vp(x):
    return C.c_void_p(int(x)) if x else C.c_void_p(0)


class Buffers:
    def __init__(self, dev, L, shapes):
        # shapes: (bs, cap_img, nc, agnostic) of every call of the sequence: one workspace that is large enough for each
        self.L, self.dev = L, dev
        self.ws_bytes = max(int(L.obb_nms_obb_workspace_bytes(bs, cap, nc, agn)) for bs, cap, nc, agn in shapes)
        self.ws = torch.zeros(self.ws_bytes, dtype=torch.uint8, device=dev)
        bs = max(s[0] for s in shapes)
        self.state_bytes = {b: int(L.obb_nms_obb_state_bytes(b)) for b in set(s[0] for s in shapes)}
        self.state = torch.zeros(max(self.state_bytes.values()), dtype=torch.uint8, device=dev)      # zero once: every call leaves it zero
        self.out = torch.empty(bs * MAX_DET * 7, dtype=torch.float32, device=dev)
        self.count = torch.empty(bs, dtype=torch.int64, device=dev)
        self.status = torch.empty(2, dtype=torch.int64, device=dev)

    def poison(self):
        self.ws.fill_(0xA5)

    def results(self, bs, ref, what):
        torch.cuda.synchronize()
        count, status = self.count[:bs].cpu().tolist(), self.status.cpu().tolist()
        assert -1 not in count, (what, "abort status", count)
        assert status[0] == 0 and count == [int(r.shape[0]) for r in ref], (what, status, count)
        out = self.out.cpu().reshape(-1, 7)
        for b, r in enumerate(ref):
            assert out[b * MAX_DET:b * MAX_DET + len(r)].numpy().tobytes() == r.float().numpy().tobytes(), (what, "image", b)


def _tail(kw, cap_img, hint):
    from yolov5_obb_amd.utils import general
    return (kw["conf_thres"], kw["iou_thres"], None, 0, int(kw["agnostic"]), 1, MAX_DET, general._MAX_NMS, float(general._MAX_WH), None, 0,
            cap_img, hint)


def test_state_across_paths_pred(dev, oracle_lib):
    from yolov5_obb_amd import _lib
    L = _lib.lib()
    kw = dict(conf_thres=0.25, iou_thres=0.45, agnostic=False, multi_label=True, max_det=MAX_DET)
    bs, A = 2, 3000
    small = synth.s_pred(bs, A, 16, seed=8100, n_obj=12, fg_frac=0.04, dtype=torch.float16)
    big = synth.s_pred(bs, A, 2, seed=8101, n_obj=300, fg_frac=0.5, dtype=torch.float16)       # nc = 2: > 384 candidates in a class
    cls = big[..., 5:7].float() * big[..., 4:5].float()
    assert int(((cls > 0.25) & (big[..., 4:5] > 0.25)).sum(1).max()) > 384
    ref = {id(p): pyref.non_max_suppression_obb(p.clone(), **kw) for p in (small, big)}
    dsmall, dbig = small.to(dev), big.to(dev)
    cap = {16: min(A * 16, 65536), 2: A * 2}
    B = Buffers(dev, L, [(bs, cap[16], 16, 0), (bs, cap[2], 2, 0)])
    st = torch.cuda.current_stream(dev).cuda_stream
    seq = [("small", dsmall, small, SMALL), ("persistent, in-LDS sort", dbig, big, PERSIST_LDS), ("small again", dsmall, small, SMALL),
           ("persistent, un-hinted", dbig, big, UNHINTED), ("small, third", dsmall, small, SMALL)]
    for i, (what, d, host, hint) in enumerate(seq):
        if i:
            B.poison()
        no = d.shape[2]
        nc = no - 185
        col = d[..., 4].contiguous() if i % 2 else None                                          # with and without the objectness column
        rc = L.obb_non_max_suppression_obb_st(vp(d.data_ptr()), vp(col.data_ptr() if col is not None else 0), 1, bs, A, no,
                                              *_tail(kw, cap[nc], hint), vp(B.out.data_ptr()), 0, vp(B.count.data_ptr()),
                                              vp(B.status.data_ptr()), vp(B.ws.data_ptr()), B.ws_bytes, vp(B.state.data_ptr()),
                                              B.state_bytes[bs], vp(st))
        assert rc == 0, (what, rc)
        B.results(bs, ref[id(host)], what)
        # the largest segment a hinted call reports says which NMS kernel can have taken it (the un-hinted radix path reports none)
        seg = (int(B.status.cpu()[1]) >> 32) & 0x1fffffff
        if hint != UNHINTED:
            assert (0 < seg <= 384) == (nc == 16), (what, seg)


def test_state_across_paths_head(dev, oracle_lib):
    """The same through k_decode_head (what Detect.lazy_nms calls): one small head, class segments on the small-segment kernel against
    the agnostic call of the same head (one list per image: the persistent kernel)."""
    from tests import head_cases as HC
    from yolov5_obb_amd import _lib
    L = _lib.lib()
    case = HC.BY_NAME["nl3_na3_nc16_straddle"]
    convs = HC.convs(case, torch.float16)
    bs, nc, na, nl = case.bs, case.nc, case.na, case.nl
    no, A = case.no, case.a_total
    d = [c.to(dev) for c in convs]
    arr = (C.c_void_p * nl)(*[c.data_ptr() for c in d])
    ny = (C.c_int64 * nl)(*[c.shape[2] for c in d]); nx = (C.c_int64 * nl)(*[c.shape[3] for c in d])
    apx = HC.anchors_px(case).reshape(-1)
    px = (C.c_float * len(apx))(*[float(v) for v in apx]); sta = (C.c_float * nl)(*[float(s) for s in HC.strides(case)])
    st = torch.cuda.current_stream(dev).cuda_stream
    # z as the library's own Detect decode writes it: the tensor the _head entry is defined by (include/obb_hip.h)
    zd = torch.empty((bs, A, no), dtype=torch.float16, device=dev)
    assert L.obb_detect_decode_levels(nl, arr, 1, bs, na, no, ny, nx, px, sta, None, vp(zd.data_ptr()), A, None, vp(st)) == 0
    z = zd.cpu()
    refs = {}
    for agn in (0, 1):
        kw = dict(conf_thres=0.25, iou_thres=0.45, agnostic=bool(agn), multi_label=True, max_det=MAX_DET)
        refs[agn] = (kw, pyref.non_max_suppression_obb(z.clone(), **kw))
    assert sum(r.shape[0] for r in refs[0][1]) > 0
    cap_img = min(A * nc, 65536)
    B = Buffers(dev, L, [(bs, cap_img, nc, 0), (bs, cap_img, nc, 1)])
    for i, (what, agn, hint) in enumerate([("small", 0, SMALL), ("persistent, in-LDS sort", 1, PERSIST_LDS), ("small again", 0, SMALL),
                                           ("persistent, un-hinted", 1, UNHINTED), ("small, third", 0, SMALL)]):
        if i:
            B.poison()
        kw, ref = refs[agn]
        rc = L.obb_non_max_suppression_obb_head(nl, arr, 1, bs, na, no, ny, nx, px, sta, *_tail(kw, cap_img, hint), vp(B.out.data_ptr()), 0,
                                                vp(B.count.data_ptr()), vp(B.status.data_ptr()), vp(B.ws.data_ptr()), B.ws_bytes,
                                                vp(B.state.data_ptr()), B.state_bytes[bs], vp(st))
        assert rc == 0, (what, rc)
        B.results(bs, ref, what)
