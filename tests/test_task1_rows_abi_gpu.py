"""GPU: the memory contract of obb_task1_eval_f64, called through the raw C ABI with the harness of tests/abi_contract.py as
tests/test_tile_merge_abi_gpu.py calls its neighbour: an exact-size poisoned workspace between canaries, a short / NULL /
misaligned `ws` refused before anything is written, a side stream, nd == 0, and every OBB_ERR_BAD_ARG case answered before a
device call (those run without a GPU).

(The table of tests/test_abi_contract_gpu.py is tied to the header's `ws_bytes` parameters and the one of
tests/test_tile_merge_abi_gpu.py to `ws_len`, each by a host test of its module, and `ws_size` / `ws_cap` are taken; this entry names the same argument `ws_extent`
and has its table here.)

The oracle is the restatement of voc_eval with the pinned tie rule (tests/task1_rows_cases.expected_class)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import abi_contract as AC
from tests import task1_rows_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def vp(x):
    return C.c_void_p(int(x)) if x else C.c_void_p(0)


def L_():
    from yolov5_obb_amd import _lib
    return _lib.lib()


def scene(name):
    """(rows, bbox8 grouped by segment, gt_off, difficult, n_img, nc) and the expected outputs of both metrics."""
    def make():
        if name == "hand":
            rows, bbox8, cls, img, diff, n_img, classnames = RC.hand_made()
        else:
            gt_lines, det = RC.tie_free_set(name)
            imagenames, classnames = list(gt_lines), list(RC.CLASSES[name])
            rows = RC.rows_of(det, imagenames, classnames, seed=3)
            bbox8, cls, img, diff = RC.parse_gt_lines(gt_lines, imagenames, classnames)
            n_img = len(imagenames)
        nc = len(classnames)
        seg = cls * n_img + img
        by_seg = np.argsort(seg, kind="stable")
        gt_off = np.zeros(nc * n_img + 1, dtype=np.int32)
        gt_off[1:] = np.cumsum(np.bincount(seg, minlength=nc * n_img))
        want = dict(ap={1: [], 0: []}, npos=[], cls_off=[0], order=[], rec=[], prec=[])
        for c in range(nc):
            mine = np.flatnonzero(rows[:, 9] == c)
            want["npos"].append(int(((cls == c) & (diff == 0)).sum()))
            want["cls_off"].append(want["cls_off"][-1] + len(mine))
            if len(mine) == 0:
                want["ap"][1].append(0.0); want["ap"][0].append(0.0)   # evaluated literally: voc_ap of empty curves
                continue
            rec, prec, ap1, ap0, sorted_ind = RC.expected_class(rows, c, bbox8, cls, img, diff)
            want["ap"][1].append(ap1); want["ap"][0].append(ap0)
            want["order"].append(mine[sorted_ind]); want["rec"].append(rec); want["prec"].append(prec)
        for k in ("order", "rec", "prec"):
            want[k] = np.concatenate(want[k])
        return rows, np.ascontiguousarray(bbox8[by_seg]), gt_off, (diff[by_seg] != 0).astype(np.uint8), n_img, nc, want
    return RC.memo(("abi", name), make)


def eval_case(name, flags, nd=None):
    rows, gts8, gt_off, difficult, n_img, nc, want = scene(name)
    n = len(rows) if nd is None else nd
    ng = len(gts8)

    def call(L, P, ws, wsb, st, mark):
        return L.obb_task1_eval_f64(vp(P["dets"]), 11, n, vp(P["gts8"]), vp(P["gt_off"]), vp(P["difficult"]), ng, n_img, nc, 0.5, flags,
                                    vp(P["ap"]), vp(P["npos"]), vp(P["cls_off"]), vp(P["order"]), vp(P["rec"]), vp(P["prec"]), vp(P["info"]),
                                    vp(ws), wsb, vp(st))

    def verify(O):
        info, ap, npos, cls_off = O("info", np.int32), O("ap", np.float64), O("npos", np.int64), O("cls_off", np.int32)
        order, rec, prec = O("order", np.int32), O("rec", np.float64), O("prec", np.float64)
        assert info.tolist() == [0, 0], (name, info.tolist())
        assert npos.tolist() == want["npos"], name
        if n == 0:
            assert ap.tolist() == [0.0] * nc and cls_off.tolist() == [0] * (nc + 1)
            for buf in (order, rec, prec):
                assert (buf.view(np.uint8) == AC.FILL).all(), "nd == 0 writes no row"
            return [info, ap, npos, cls_off]
        assert cls_off.tolist() == want["cls_off"], name
        assert order.tolist() == want["order"].tolist(), name
        assert RC.same(rec, want["rec"]) and RC.same(prec, want["prec"]), name
        assert RC.same(ap, np.array(want["ap"][flags & 1], dtype=np.float64)), (name, ap, want["ap"][flags & 1])
        return [info, ap, npos, cls_off, order, rec, prec]

    return AC.Case(f"task1_eval-{name}-flags{flags}-nd{n}", ["obb_task1_eval_f64"], dict(dets=rows, gts8=gts8, gt_off=gt_off, difficult=difficult),
                   dict(ap=nc * 8, npos=nc * 8, cls_off=(nc + 1) * 4, order=len(rows) * 4, rec=len(rows) * 8, prec=len(rows) * 8, info=8),
                   lambda L: L.obb_task1_eval_workspace_bytes(n, ng, n_img, nc), call, verify, index_inputs=("dets",))


def test_the_entry_is_the_only_one_that_names_its_workspace_size_ws_extent():
    """Host: the functions of include/obb_hip.h with a `size_t ws_extent` parameter are exactly the entry this module calls."""
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "obb_hip.h")).read(), flags=re.S)
    found = [m.group(1) for m in re.finditer(r"\b(\w+)\s*\(([^;{}()]*)\)\s*;", text) if re.search(r"\bsize_t\s+ws_extent\b", m.group(2))]
    assert found == ["obb_task1_eval_f64"]


def test_every_bad_argument_is_answered_before_a_device_call():
    """Host: OBB_ERR_BAD_ARG = -1 with pointers that are never followed (no GPU needed), and a size query of 0 for the same."""
    L = L_()
    p = 4096                                                     # non-NULL, never dereferenced

    def call(det_stride=11, nd=5, ng=3, n_img=2, nc=2, flags=1, **null):
        a = {k: (0 if null.get(k) else p) for k in ("dets", "gts8", "gt_off", "difficult", "ap", "npos", "cls_off", "info")}
        return L.obb_task1_eval_f64(vp(a["dets"]), det_stride, nd, vp(a["gts8"]), vp(a["gt_off"]), vp(a["difficult"]), ng, n_img, nc, 0.5, flags,
                                    vp(a["ap"]), vp(a["npos"]), vp(a["cls_off"]), vp(0), vp(0), vp(0), vp(a["info"]), vp(p), 1 << 30, vp(0))
    bad = [dict(det_stride=10), dict(det_stride=0), dict(nc=0), dict(nc=257), dict(nc=-1), dict(nd=-1), dict(ng=-1), dict(n_img=-1),
           dict(nd=2 ** 31), dict(ng=2 ** 31), dict(nc=256, n_img=2 ** 23), dict(n_img=2 ** 31), dict(flags=2), dict(flags=-1),
           dict(dets=True), dict(gts8=True), dict(gt_off=True), dict(difficult=True), dict(ap=True), dict(npos=True), dict(cls_off=True),
           dict(info=True)]
    for kw in bad:
        assert call(**kw) == -1, kw
    for nd, ng, n_img, nc in ((-1, 0, 1, 1), (0, -1, 1, 1), (0, 0, -1, 1), (0, 0, 1, 0), (0, 0, 1, 257), (2 ** 31, 0, 1, 1), (0, 2 ** 31, 1, 1),
                              (0, 0, 2 ** 23, 256)):
        assert L.obb_task1_eval_workspace_bytes(nd, ng, n_img, nc) == 0, (nd, ng, n_img, nc)
    assert L.obb_task1_eval_workspace_bytes(0, 0, 0, 1) > 0 and L.obb_task1_eval_workspace_bytes(2 ** 31 - 1, 2 ** 31 - 1, 2 ** 23 - 1, 256) > 0
    # a workspace that is short, NULL or misaligned is the next answer, still before any device call
    a = [vp(p), 11, 5, vp(p), vp(p), vp(p), 3, 2, 2, 0.5, 1, vp(p), vp(p), vp(p), vp(0), vp(0), vp(0), vp(p)]
    need = L.obb_task1_eval_workspace_bytes(5, 3, 2, 2)
    assert L.obb_task1_eval_f64(*a, vp(0), need, vp(0)) == -2
    assert L.obb_task1_eval_f64(*a, vp(p), need - 1, vp(0)) == -2
    assert L.obb_task1_eval_f64(*a, vp(p + 128), need, vp(0)) == -2


@pytest.mark.gpu
@pytest.mark.parametrize("name,flags,donor", [("hand", 1, "wide"), ("hand", 0, "wide"), ("wide", 0, "hand"), ("wide", 1, "hand")])
def test_exact_poisoned_workspace_between_canaries(dev, oracle_lib, name, flags, donor):
    AC.run_poisons(L_(), dev, eval_case(name, flags), eval_case(donor, 1))


@pytest.mark.gpu
@pytest.mark.parametrize("ws_mode", ["short", "null", "+8", "+128"])
def test_a_short_missing_or_misaligned_workspace_is_refused_before_anything_is_written(dev, oracle_lib, ws_mode):
    AC.run_refused(L_(), dev, eval_case("hand", 1), ws_mode)


@pytest.mark.gpu
def test_no_detection_writes_zero_aps_and_counts_the_records(dev, oracle_lib):
    AC.run_poisons(L_(), dev, eval_case("hand", 1, nd=0), eval_case("wide", 1))


@pytest.mark.gpu
def test_all_work_is_enqueued_on_the_callers_stream(dev, oracle_lib):
    from tests.test_abi_contract_gpu import DELAY_ITERS, _seed_matrix
    res, pending = AC.run_on_side_stream(L_(), dev, eval_case("wide", 0), DELAY_ITERS, _seed_matrix(dev))
    assert pending, "the delay had drained before the ABI call returned: the run proves nothing"
