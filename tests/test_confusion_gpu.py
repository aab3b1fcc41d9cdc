"""GPU: the device ConfusionMatrix (csrc/head.hip: k_confusion behind obb_confusion_batch_f32 / obb_confusion_process_batch_f32,
utils.metrics.ConfusionMatrix, ValStats.add_batch(confusion=), val_sharded.run(confusion_matrix=)) against the reference's own
ConfusionMatrix.process_batch with every argsort stable (tests/golden/confusion_cases.npz), integer for integer.

Every case of tests/confusion_cases.py goes through three paths that must give the same cells:
  * the whole-batch C entry on (det7, targets, shapes), in chunks of 64 images;
  * the per-image C entry, fed image by image with val_postprocess's pred_hbbn and the label boxes (the device's hull, then
    pad / gain / clip in float32 on the host, IEEE-exact like vt_label_box);
  * the Python object's add_batch on consecutive views of one packed buffer.
The cases hold: exact ties and their permutations, the threshold and filter edges, the participation rule, 1 / 511 / 512 / 513 /
1025 labels (the LDS tile; winner slots in LDS or in the workspace), 1 .. 1025 kept detections (waves, 256, the workgroup's 1024
threads), 1 / 2 / 64 / 65 images, nc = 1 .. 110 (109 | 110: the LDS histogram's cut-over)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import confusion_cases as CC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "confusion_cases.npz"))


def _img5(shapes):
    flat = []
    for shape, ratio_pad in shapes:
        flat += (ratio_pad[1][0], ratio_pad[1][1], ratio_pad[0][0], shape[1], shape[0])
    return (C.c_float * len(flat))(*flat)


def _new_matrix(dev, nc, fill=0):
    return torch.full(((nc + 1) ** 2 + 1,), fill, dtype=torch.int64, device=dev)


def cabi_batch(dev, case, mat=None):
    """obb_confusion_batch_f32 over the case in chunks of <= 64 images -> the (nc + 1)^2 + 1 counters (a device tensor)."""
    from yolov5_obb_amd import _lib
    L = _lib.lib()
    nc = case["nc"]
    mat = _new_matrix(dev, nc) if mat is None else mat
    preds, targets = case["preds"], case["targets"]
    for b0 in range(0, len(preds), 64):
        b1 = min(len(preds), b0 + 64)
        counts = [p.shape[0] for p in preds[b0:b1]]
        doff = (C.c_int64 * (b1 - b0 + 1))(*np.concatenate(([0], np.cumsum(counts))).tolist())
        n = sum(counts)
        det = torch.cat(preds[b0:b1], 0).to(dev).contiguous() if n else None
        sel = (targets[:, 0] >= b0) & (targets[:, 0] < b1)
        tg = targets[sel].clone()
        tg[:, 0] -= b0
        tg = tg.to(dev).contiguous()
        nt = int(tg.shape[0])
        img5 = _img5(case["shapes"][b0:b1])
        ws = torch.empty(L.obb_confusion_workspace_bytes(n, nt), dtype=torch.uint8, device=dev)
        rc = L.obb_confusion_batch_f32(_lib.ptr(det), C.cast(doff, C.c_void_p), b1 - b0, _lib.ptr(tg) if nt else None, nt, 9,
                                       C.cast(img5, C.c_void_p), nc, case["conf"], case["iou_thres"], _lib.ptr(mat), _lib.ptr(ws),
                                       ws.numel(), _lib.stream_ptr(dev))
        assert rc == 0, rc
    return mat


def device_boxes(dev, case, b):
    """(pred_hbbn (n, 6), labels_hbbn (m, 5)) of image b with the device's bits, on the device."""
    from yolov5_obb_amd.val import val_postprocess
    (h, w), ratio_pad = case["shapes"][b]
    hbbn = val_postprocess(case["preds"][b].to(dev), ratio_pad=ratio_pad)[3]
    lab = CC.labels_of(case["targets"], b)
    lab7 = torch.cat((lab[:, 2:7], torch.zeros_like(lab[:, :1]), lab[:, 1:2]), 1).to(dev)
    tb = val_postprocess(lab7, ratio_pad=((1.0, 1.0), (0.0, 0.0)))[1][:, :4].cpu()
    f = lambda v: torch.tensor(v, dtype=torch.float32)
    tb[:, [0, 2]] -= f(ratio_pad[1][0]); tb[:, [1, 3]] -= f(ratio_pad[1][1])
    tb /= f(ratio_pad[0][0])
    tb[:, [0, 2]] = tb[:, [0, 2]].clamp(0, float(w)); tb[:, [1, 3]] = tb[:, [1, 3]].clamp(0, float(h))
    return hbbn, torch.cat((lab[:, 1:2], tb), 1).to(dev)


def cabi_per_image(dev, case):
    """obb_confusion_process_batch_f32 image by image -> (bs, nc + 1, nc + 1) int64 on the host."""
    from yolov5_obb_amd import _lib
    L = _lib.lib()
    nc = case["nc"]
    out = np.zeros((len(case["preds"]), nc + 1, nc + 1), dtype=np.int64)
    for b in range(len(case["preds"])):
        if not CC.takes_part(case, b):
            continue
        det, lab = device_boxes(dev, case, b)
        mat = _new_matrix(dev, nc)
        ws = torch.empty(L.obb_confusion_workspace_bytes(det.shape[0], lab.shape[0]), dtype=torch.uint8, device=dev)
        rc = L.obb_confusion_process_batch_f32(_lib.ptr(det), det.shape[0], _lib.ptr(lab), lab.shape[0], nc, case["conf"],
                                               case["iou_thres"], _lib.ptr(mat), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev))
        assert rc == 0, rc
        host = mat.cpu().numpy()
        assert host[-1] == 0
        out[b] = host[:-1].reshape(nc + 1, nc + 1)
    return out


def packed_views(dev, preds):
    packed = torch.cat(preds, 0).to(dev)
    return list(packed.split([p.shape[0] for p in preds]))


def _cells(mat, nc):
    host = mat.cpu().numpy()
    return host[:-1].reshape(nc + 1, nc + 1), int(host[-1])


@pytest.mark.parametrize("name", CC.NAMES)
def test_case_matches_the_reference_through_every_entry(dev, golden, name):
    from yolov5_obb_amd.utils.metrics import ConfusionMatrix
    case = CC.build(name)
    nc, want = case["nc"], golden[name].astype(np.int64)
    got, oor = _cells(cabi_batch(dev, case), nc)
    diff = int(np.abs(got - want.sum(0)).sum())
    print(name, "counts", int(want.sum()), "batch entry differs by", diff)
    assert oor == 0 and diff == 0, (name, "obb_confusion_batch_f32")
    per = cabi_per_image(dev, case)
    assert np.array_equal(per, want), (name, "obb_confusion_process_batch_f32", np.flatnonzero(np.abs(per - want).sum((1, 2))).tolist())
    cm = ConfusionMatrix(nc, conf=case["conf"], iou_thres=case["iou_thres"])
    cm.add_batch(packed_views(dev, case["preds"]) if sum(p.shape[0] for p in case["preds"]) else [p.to(dev) for p in case["preds"]],
                 case["targets"].to(dev), case["shapes"])
    m = cm.matrix
    assert m.dtype == np.float64 and m.shape == (nc + 1, nc + 1) and np.array_equal(m, want.sum(0).astype(np.float64)), (name, "add_batch")


def test_process_batch_of_the_object_and_labels_on_the_host(dev, golden):
    from yolov5_obb_amd.utils.metrics import ConfusionMatrix
    case = CC.build("tie_grid")
    cm = ConfusionMatrix(case["nc"], device=dev)
    for b in range(len(case["preds"])):
        det, lab = device_boxes(dev, case, b)
        cm.process_batch(det, lab.cpu())                        # labels on the host are moved, as val.process_batch does
    cm.process_batch(det[:0], lab)                              # no detections, no labels: nothing
    cm.process_batch(det, lab[:0])
    assert np.array_equal(cm.matrix, golden["tie_grid"].sum(0))
    tp, fp = cm.tp_fp()
    assert np.array_equal(tp, cm.matrix.diagonal()[:-1]) and np.array_equal(fp, cm.matrix.sum(1)[:-1] - tp)


def test_calls_accumulate_and_a_second_matrix_on_another_stream_is_its_own(dev, golden):
    from yolov5_obb_amd.utils.metrics import ConfusionMatrix
    a, b = CC.build("nc16"), CC.build("det_257")
    assert a["nc"] == b["nc"] == 16
    mat = cabi_batch(dev, a)
    cabi_batch(dev, b, mat)                                     # the call never zeroes the counters
    want = (golden["nc16"].sum(0) + golden["det_257"].sum(0)).astype(np.int64)
    assert np.array_equal(_cells(mat, 16)[0], want)
    pre = _new_matrix(dev, 16, fill=7)                          # nor does it assume zeros
    assert np.array_equal(_cells(cabi_batch(dev, a, pre), 16)[0], golden["nc16"].sum(0) + 7)
    cm1, cm2 = ConfusionMatrix(16), ConfusionMatrix(16)
    side = torch.cuda.Stream(dev)
    views_a, views_b = packed_views(dev, a["preds"]), packed_views(dev, b["preds"])
    tg_a, tg_b = a["targets"].to(dev), b["targets"].to(dev)
    torch.cuda.synchronize(dev)
    cm1.add_batch(views_a, tg_a, a["shapes"])
    with torch.cuda.stream(side):
        cm2.add_batch(views_b, tg_b, b["shapes"])
    cm1.add_batch(views_b, tg_b, b["shapes"])
    assert np.array_equal(cm1.matrix, want) and np.array_equal(cm2.matrix, golden["det_257"].sum(0))


def test_out_of_range_classes_touch_no_cell_and_raise_on_read(dev):
    """A detection of class nc on a label of class -1, beside a pair in range: one cell, the counter at 1, RuntimeError."""
    from yolov5_obb_amd.utils.metrics import ConfusionMatrix
    B, B2 = CC.BOX, CC._shift(CC.BOX, 200)
    case = CC._exact([([(-1, *B), (1, *B2)], [(*B, 0.9, 3), (*B2, 0.9, 1)])], nc=3)
    pre = _new_matrix(dev, 3, fill=5)
    pre[-1] = 0
    cells, oor = _cells(cabi_batch(dev, case, pre), 3)
    want = np.full((4, 4), 5, dtype=np.int64)
    want[1, 1] += 1
    assert np.array_equal(cells, want) and oor == 1
    per = ConfusionMatrix(3)
    det, lab = device_boxes(dev, case, 0)
    per.process_batch(det, lab)
    cm = ConfusionMatrix(3)
    cm.add_batch([p.to(dev) for p in case["preds"]], case["targets"].to(dev), case["shapes"])
    for obj in (per, cm):
        with pytest.raises(RuntimeError, match="outside"):
            obj.matrix
    # unmatched rows with a class out of range: the background cells are not taken either
    case = CC._exact([([(5, *B), (1, *B2)], [(*CC._shift(B, 400), 0.9, -1), (*B2, 0.9, 1)])], nc=3)
    cells, oor = _cells(cabi_batch(dev, case), 3)
    want = np.zeros((4, 4), dtype=np.int64)
    want[1, 1] = 1
    assert np.array_equal(cells, want) and oor == 2


def test_valstats_and_val_sharded_pass_the_matrix_through(dev, golden):
    """Three batches: the statistics rows are bit-identical with and without the argument; the matrix is the goldens' sum."""
    from yolov5_obb_amd import val as V, val_sharded
    from yolov5_obb_amd.utils.metrics import ConfusionMatrix
    names = ["bs2", "det_65", "lab_513"]
    cases = [CC.build(n) for n in names]
    assert all(c["nc"] == 16 for c in cases)
    want = sum(golden[n].sum(0) for n in names).astype(np.float64)
    iouv = torch.linspace(0.5, 0.95, 10, device=dev)
    plain, with_cm, cm = V.ValStats(device=dev), V.ValStats(device=dev), ConfusionMatrix(16)
    for c in cases:
        plain.add_batch(packed_views(dev, c["preds"]), c["targets"].to(dev), c["shapes"], iouv)
        with_cm.add_batch(packed_views(dev, c["preds"]), c["targets"].to(dev), c["shapes"], iouv, confusion=cm)
    assert torch.equal(plain.rows, with_cm.rows) and torch.equal(plain.target_cls, with_cm.target_cls)
    assert np.array_equal(cm.matrix, want)
    # val_sharded.run: a stand-in model, and an NMS stand-in that hands out the cases' detections
    loader = list((torch.zeros(len(c["preds"]), 3, 32, 32, dtype=torch.uint8), c["targets"], [""] * len(c["preds"]), c["shapes"])
                     for c in cases)
    queue = []

    def nms(out, *a, **k):
        if not queue:
            queue.extend(cases)
        return packed_views(dev, queue.pop(0)["preds"])
    model = lambda im: (im,)
    base = val_sharded.run(model, loader, device=dev, nms=nms, device_metrics=True, half=False)
    cm2 = ConfusionMatrix(16)
    res = val_sharded.run(model, loader, device=dev, nms=nms, device_metrics=True, half=False, confusion_matrix=cm2)
    assert "confusion_matrix" not in base and res["confusion_matrix"] is cm2
    assert torch.equal(base["val_stats"].rows, res["val_stats"].rows) and torch.equal(base["val_stats"].rows, plain.rows)
    assert np.array_equal(cm2.matrix, want)
    with pytest.raises(RuntimeError):
        val_sharded.run(model, loader, device=dev, nms=nms, confusion_matrix=ConfusionMatrix(16))      # needs device_metrics=True
