"""GPU: the memory contract of obb_non_max_suppression_obb_tta_head, called through the raw C ABI with the harness of
tests/abi_contract.py as tests/test_abi_contract_gpu.py calls its neighbours: an exact-size poisoned workspace between canaries,
a short / NULL / misaligned `ws` refused before any device call, a capped grid.  Shape nc3_128 of tests/test_tta_decode_gpu.py, fp16.

(The table of tests/test_abi_contract_gpu.py is tied to the header's `ws_bytes` parameters by a host test of that module; this
entry names the same argument `ws_size` and has its table here.)

The oracle is the eager chain on the same device: obb_detect_decode_tta, then non_max_suppression_obb of that tensor."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import abi_contract as AC
from tests import lazy_tta_cases as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE, MAX_DET, SEED = "nc3_128", 300, 11
vp = C.c_void_p
_memo = {}


def L_():
    from yolov5_obb_amd import _lib
    return _lib.lib()


def setup(dev):
    """Conv outputs (host), the plan, the eager z and the eager NMS of it -- once."""
    if "s" not in _memo:
        det = TC.make_detect(CASE, dev, torch.float16)
        convs = TC.heads(CASE, dev, torch.float16, SEED)
        ze, plan = TC.eager(det, convs, CASE, TC.SCALES, TC.FLIPS[0])
        from yolov5_obb_amd.utils.general import non_max_suppression_obb
        kw = dict(TC.KW, max_det=MAX_DET)
        ref = [r.cpu() for r in non_max_suppression_obb(ze, **kw)]
        obj = ze[..., 4:5]
        nc = ze.shape[2] - 185
        most = int((((ze[..., 5:5 + nc] * obj) > kw["conf_thres"]) & (obj > kw["conf_thres"])).sum((1, 2)).max())
        anchor_px, strides = det._host_tables()
        _memo["s"] = dict(det=det, convs=[[c.cpu() for c in cs] for cs in convs], plan=plan, ref=ref, most=most,
                          anchor_px=[list(a) for a in anchor_px], strides=list(strides), kw=kw)
    return _memo["s"]


def tta_case(dev, packed, with_state, cap=None):
    from yolov5_obb_amd import _lib
    from yolov5_obb_amd.models.yolo import _tta_passes
    from yolov5_obb_amd.utils import general
    s = setup(dev)
    nc, _, _, img, bs, _ = TC.CASES[CASE]
    plan, kw, ref = s["plan"], s["kw"], s["ref"]
    no, na = nc + 185, 3
    inputs = {f"conv{k}_{lv}": s["convs"][k][lv].numpy() for k, p in enumerate(plan.passes) for lv in p.levels}
    cap_img = int(cap if cap is not None else min(plan.a_total * nc, 65536))
    name = f"tta_head-{'packed' if packed else 'rows'}-{'state' if with_state else 'nostate'}"

    class At:                                                          # what _tta_passes reads of a conv output, at its address in the arena
        def __init__(self, ptr, t):
            self.ptr, self.shape = ptr, t.shape

        def data_ptr(self):
            return self.ptr

    def call(L, P, ws, wsb, st, mark):
        at = [[At(P.get(f"conv{k}_{lv}", 0), c) for lv, c in enumerate(cs)] for k, cs in enumerate(s["convs"])]
        arr = _tta_passes(at, plan, TC.SCALES, TC.FLIPS[0], img[0], img[1], na, s["anchor_px"], s["strides"])
        return L.obb_non_max_suppression_obb_tta_head(
            len(arr), C.cast(arr, vp), _lib.DTYPE_CODES[torch.float16], bs, na, no, plan.a_total, kw["conf_thres"], kw["iou_thres"], None, 0, 0, 1,
            MAX_DET, general._MAX_NMS, float(general._MAX_WH), None, 0, cap_img, 0, vp(P["out"]), packed, vp(P["out_count"]), vp(P["status"]),
            vp(ws), wsb, vp(P["state"]), state_bytes(L) if P["state"] else 0, vp(st))

    def state_bytes(L):
        return L.obb_nms_obb_state_bytes(bs)

    def verify(O):
        count, status = O("out_count", np.int64), O("status", np.int64)
        assert int(status[1] & 0xffffffff) == s["most"], (name, int(status[1] & 0xffffffff), s["most"])
        assert int(status[0]) == 0 and count.tolist() == [int(r.shape[0]) for r in ref], (name, status.tolist(), count.tolist())
        assert sum(count.tolist()) > bs, name
        out = O("out", np.float32).reshape(bs * MAX_DET, 7)
        rows, at = [], 0
        for b, r in enumerate(ref):
            lo = at if packed else b * MAX_DET
            rows.append(out[lo:lo + len(r)].copy())
            at += len(r)
            assert rows[-1].tobytes() == r.float().numpy().tobytes(), (name, "image", b)
        return [count, status] + rows

    return AC.Case(name, ["obb_non_max_suppression_obb_tta_head"], inputs, dict(out=bs * MAX_DET * 7 * 4, out_count=bs * 8, status=16),
                   lambda L: L.obb_nms_obb_workspace_bytes(bs, cap_img, nc, 0), call, verify, state_bytes=state_bytes if with_state else None)


def test_the_entry_is_the_only_one_that_names_its_workspace_size_ws_size():
    """Host: the functions of include/obb_hip.h with a `size_t ws_size` parameter are exactly the entry this module calls."""
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "obb_hip.h")).read(), flags=re.S)
    found = [m.group(1) for m in re.finditer(r"\b(\w+)\s*\(([^;{}()]*)\)\s*;", text) if re.search(r"\bsize_t\s+ws_size\b", m.group(2))]
    assert found == ["obb_non_max_suppression_obb_tta_head"]


@pytest.mark.gpu
@pytest.mark.parametrize("packed,with_state", [(1, True), (0, False)], ids=["packed_state", "rows_nostate"])
def test_exact_poisoned_workspace_between_canaries(dev, packed, with_state):
    case = tta_case(dev, packed, with_state)
    donor = tta_case(dev, 1 - packed, not with_state)
    AC.run_poisons(L_(), dev, case, donor)


@pytest.mark.gpu
@pytest.mark.parametrize("ws_mode", ["short", "null", "+8", "+128"])
def test_a_short_missing_or_misaligned_workspace_is_refused_before_anything_is_written(dev, ws_mode):
    AC.run_refused(L_(), dev, tta_case(dev, 1, True), ws_mode)


@pytest.mark.gpu
def test_query_and_call_under_a_capped_grid(dev):
    AC.run_capped(L_(), dev, tta_case(dev, 1, True))
