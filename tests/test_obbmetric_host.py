"""Host: the oriented-box process_batch -- the pinned rule restated on an IoU matrix (tests/obbmetric_cases.py::rule) against
the outputs frozen from the reference's val.process_batch with the rotated IoU (tests/golden/obbmetric_cases.npz), the two C-ABI
entries in header, library and binding table, and their argument checks (which answer before any device call).  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import obbmetric_cases as OC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("obb_process_batch_obb_f32", "obb_val_tail_batch_obb_f32")


@pytest.mark.parametrize("name", OC.NAMES)
def test_restated_rule_reproduces_every_golden_row(name, oracle_lib):
    if name in OC.SINGLE:
        pred, labels, want = OC.load(name)
        assert (pred.shape[0], labels.shape[0]) == OC.SINGLE[name][:2]
        got = OC.rule(OC.riou(labels, pred), labels[:, 0].numpy(), pred[:, 6].numpy(), OC.IOUV.numpy())[0]
    else:
        preds, targets, want = OC.load(name)
        assert [(p.shape[0], int((targets[:, 0] == b).sum())) for b, p in enumerate(preds)] == [im[:2] for im in OC.BATCH[name]]
        got = OC.rule_batch(preds, targets, OC.IOUV.numpy())[0]
    assert got.shape == tuple(want.shape) and np.array_equal(got, want.numpy())
    assert name == "n1_m1" or (int(want[:, 0].sum()) >= 3 and not bool(want.all()))


def test_golden_inputs_keep_the_distance_the_exact_comparison_needs(oracle_lib):
    """No IoU of an equal-class pair within 1e-5 of a level, no best / second-best pair closer than 1e-5 (the generator's refusal)."""
    iouv = OC.IOUV.numpy().astype(np.float64)
    images = []
    for name in OC.NAMES:
        if name in OC.SINGLE:
            pred, labels, _ = OC.load(name)
            images.append((pred, labels))
        else:
            preds, targets, _ = OC.load(name)
            images += [(p, OC.labels_of(targets, b)[0]) for b, p in enumerate(preds)]
    for pred, labels in images:
        if pred.shape[0] == 0 or labels.shape[0] == 0:
            continue
        iou = OC.riou(labels, pred).astype(np.float64)
        same = labels[:, 0:1].numpy() == pred[:, 6].numpy()[None, :]
        assert np.abs(iou[same][:, None] - iouv[None, :]).min() >= 1e-5
        cand = np.sort(np.where(same & (iou >= iouv[0]), iou, -np.inf), axis=0)
        if cand.shape[0] >= 2:
            two = cand[-2] > -np.inf
            assert (cand[-1][two] - cand[-2][two] >= 1e-5).all()


def test_the_batch_case_reaches_the_paths_it_is_named_for(oracle_lib):
    preds, targets, _ = OC.load("bs5")
    n = [p.shape[0] for p in preds]
    m = [int((targets[:, 0] == b).sum()) for b in range(5)]
    assert n[0] == 0 and m[0] > 0 and n[1] > 0 and m[1] == 0
    assert n[1] < 128 < n[1] + n[2] + n[3] and n[1] + n[2] < 128           # two image boundaries inside the first 128 detections
    assert m[3] > 512                                                        # more labels than one LDS tile
    lab4, _ = OC.labels_of(targets, 4)
    iou = OC.riou(lab4, preds[4][:1])[:, 0]
    assert int(((lab4[:, 0] == preds[4][0, 6]).numpy() & (iou >= 0.5)).sum()) >= 100      # one lane fills its wave's queue


def test_header_library_and_binding_table_carry_both_entries():
    from yolov5_obb_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "obb_hip.h")).read(), flags=re.S)
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    L = C.CDLL(_lib.LIB_PATH)
    for e in ENTRIES:
        decl = re.search(r"\bint\s+" + e + r"\s*\(([^;]*)\)\s*;", text)
        assert decl, f"{e} is not declared in include/obb_hip.h"
        assert "ws_bytes" not in decl.group(1) and "match_label" in decl.group(1) and "match_iou" in decl.group(1)
        assert hasattr(L, e), f"{e} is not exported by the library"
        assert e in _lib.SIGNATURES


def test_argument_checks_answer_before_any_device_call():
    """OBB_ERR_BAD_ARG = -1 with nothing launched (callable without a GPU); n == 0 is OBB_OK with nothing launched either."""
    from yolov5_obb_amd import _lib
    L = _lib.lib()
    buf = (C.c_float * 64)()
    p, null = C.cast(buf, C.c_void_p), C.c_void_p(0)
    off = lambda *v: C.cast((C.c_int64 * len(v))(*v), C.c_void_p)           # noqa: E731
    pb = L.obb_process_batch_obb_f32
    assert pb(p, 0, p, 3, p, 10, p, p, p, null) == 0                        # no detections
    assert pb(null, 0, null, 0, null, 10, null, null, null, null) == 0
    for args in ((p, -1, p, 3, p, 10, p, p, p), (p, 4, p, -1, p, 10, p, p, p), (p, 4, p, 3, p, 0, p, p, p), (p, 4, p, 3, p, 17, p, p, p),
                 (null, 4, p, 3, p, 10, p, p, p), (p, 4, null, 3, p, 10, p, p, p), (p, 4, p, 3, null, 10, p, p, p),
                 (p, 4, p, 3, p, 10, null, p, p), (p, 4, p, 3, p, 10, p, null, p), (p, 4, p, 3, p, 10, p, p, null),
                 (p, 1 << 31, p, 3, p, 10, p, p, p)):
        assert pb(*args, null) == -1, args[1:6:2]
    vt = L.obb_val_tail_batch_obb_f32
    assert vt(p, null, off(0, 0, 0), 2, p, 3, 7, p, 10, p, p, p, null) == 0         # no detections in the batch
    for args in ((p, null, off(0, 4), 0, p, 3, 7, p, 10, p, p, p), (p, null, off(*range(66)), 65, p, 3, 7, p, 10, p, p, p),
                 (p, null, off(0, 4), 1, p, 3, 7, p, 0, p, p, p), (p, null, off(0, 4), 1, p, 3, 7, p, 17, p, p, p),
                 (p, null, off(0, 4), 1, p, 3, 6, p, 10, p, p, p), (p, null, off(0, 4), 1, null, 3, 7, p, 10, p, p, p),
                 (p, null, off(0, 4), 1, p, -1, 7, p, 10, p, p, p), (p, null, null, 1, p, 3, 7, p, 10, p, p, p),
                 (p, null, off(0, 4), 1, p, 3, 7, null, 10, p, p, p), (null, null, off(0, 4), 1, p, 3, 7, p, 10, p, p, p),
                 (p, null, off(0, 4), 1, p, 3, 7, p, 10, null, p, p), (p, null, off(0, 4), 1, p, 3, 7, p, 10, p, null, p),
                 (p, null, off(0, 4), 1, p, 3, 7, p, 10, p, p, null), (p, null, off(1, 4), 1, p, 3, 7, p, 10, p, p, p),
                 (p, null, off(0, 4, 2), 2, p, 3, 7, p, 10, p, p, p), (p, off(-1), off(0, 4), 1, p, 3, 7, p, 10, p, p, p)):
        assert vt(*args, null) == -1, args[3:9]
    assert all(v == 0.0 for v in buf)


def test_python_entries_refuse_cpu_tensors_and_wrong_shapes():
    from yolov5_obb_amd import val as V, val_sharded
    with pytest.raises(RuntimeError):
        V.process_batch_obb(torch.zeros(3, 7), torch.zeros(2, 6), OC.IOUV)
    with pytest.raises(RuntimeError):
        V.val_tail_batch_obb([torch.zeros(3, 7)], torch.zeros(2, 7), OC.IOUV)
    with pytest.raises(RuntimeError, match="obb_metrics needs device_metrics"):
        val_sharded.run(lambda im: (im,), [], device="cpu", obb_metrics=True, nms=lambda *a, **k: [], half=False)
