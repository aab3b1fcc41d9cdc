"""Freezes outputs of the reference's OWN ConfusionMatrix.process_batch (utils/metrics.py:117-163) on the seeded batches of
tests/confusion_cases.py -> tests/golden/confusion_cases.npz.  Needs a checkout of the reference (hukaixuan19970627/yolov5_obb):
    python tests/golden/gen_confusion_cases.py REF                 write the golden file
    python tests/golden/gen_confusion_cases.py REF --find-seeds    print, per random case, the first seed that meets the conditions
    python tests/golden/gen_confusion_cases.py REF --default-sort  the tie cases whose matrix differs under numpy's default sort
    python tests/golden/gen_confusion_cases.py REF --time          seconds of the reference's per-image calls on the bench's batch
Per image the boxes are built as val.py:226-243 builds them, with the reference's own rbox2poly, poly2hbb, xywh2xyxy,
scale_polys and scale_coords, on CPU float32 tensors; only images with detections and labels are processed (val.py:217-246).

STABLE SORTS.  The reference calls the ndarray.argsort METHOD (`matches[:, 2].argsort()[::-1]`), so wrapping np.argsort does
nothing.  For the duration of every call torch.Tensor.numpy returns a view of an ndarray subclass whose argsort forces
kind='stable'; slices and fancy indexing keep the subclass, so both sorts of the function are stable.

Only outputs are stored: name -> (images, nc + 1, nc + 1) int32, zeros for an image that takes no part.
Every stored RANDOM case must meet (else its seed in tests/confusion_cases.py::SEEDS is changed):
 (a) no IoU of a (label, kept detection) pair within 1e-4 of iou_thres;
 (b) no kept detection whose two best candidate labels, and no label whose two best candidate detections, differ by less than
     1e-4 in IoU (host and device sinf / cosf may differ in the last bits; no case may hinge on that);
 (c) the summed matrix has a non-zero cell in the diagonal, the background row, the background column and off the diagonal
     (nc = 1 has no cell off the diagonal and is exempt from that one).
The exact cases (theta = 0, integer boxes, integer pads, gain 1 or 1/2) are exempt from (a) and (b) by construction."""
import importlib.util
import os
import sys
import time
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import confusion_cases as CC  # noqa: E402


def load_reference():
    dirs = [a for a in sys.argv[1:] if not a.startswith("--")]
    if len(dirs) != 1:
        sys.exit(__doc__)
    ref = os.path.abspath(dirs[0])

    def stub(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
    for name in ("cv2", "torchvision", "seaborn"):            # imported at the top of utils/general.py, not used here
        if importlib.util.find_spec(name) is None:
            stub(name, setNumThreads=lambda n: None)
            if name == "torchvision":
                stub("torchvision.ops")
    stub("utils.nms_rotated", obb_nms=None)                  # utils/general.py:35 imports the compiled NMS; not needed here
    sys.path.insert(0, ref)
    import utils.general as G
    import utils.metrics as M
    import utils.rboxs_utils as R
    return G, R, M


class _StableArray(np.ndarray):
    def argsort(self, axis=-1, kind=None, order=None):
        return np.asarray(self).argsort(axis=axis, kind="stable", order=order)


class stable_sorts:
    """with stable_sorts(): every ndarray.argsort on arrays that come out of Tensor.numpy() is stable."""

    def __enter__(self):
        self.orig = torch.Tensor.numpy
        orig = self.orig
        torch.Tensor.numpy = lambda t, *a, **k: orig(t, *a, **k).view(_StableArray)

    def __exit__(self, *exc):
        torch.Tensor.numpy = self.orig


def image_boxes(G, R, case, b):
    """(pred_hbbn (n, 6), labels_hbbn (m, 5)) of image b, val.py:226-243."""
    pred = case["preds"][b].clone()
    labels = CC.labels_of(case["targets"], b)[:, 1:7].clone()
    shape, ratio_pad = case["shapes"][b]
    pred_poly = torch.cat((R.rbox2poly(pred[:, :5]), pred[:, -2:]), dim=1)
    pred_polyn = pred_poly.clone()
    G.scale_polys(None, pred_polyn[:, :8], shape, ratio_pad)
    pred_hbbn = torch.cat((G.xywh2xyxy(R.poly2hbb(pred_polyn[:, :8])), pred_polyn[:, -2:]), dim=1)
    tbox = G.xywh2xyxy(R.poly2hbb(R.rbox2poly(labels[:, 1:6])))
    G.scale_coords(None, tbox, shape, ratio_pad)
    return pred_hbbn, torch.cat((labels[:, 0:1], tbox), 1)


def run_case(G, R, M, case, stable=True):
    """(per-image matrices (bs, nc + 1, nc + 1) int32, the violated conditions (a) (b) as strings)."""
    nc = case["nc"]
    out = np.zeros((len(case["preds"]), nc + 1, nc + 1), dtype=np.int32)
    bad = set()
    for b in range(len(case["preds"])):
        if not CC.takes_part(case, b):
            continue
        det, lab = image_boxes(G, R, case, b)
        cm = M.ConfusionMatrix(nc, conf=case["conf"], iou_thres=case["iou_thres"])
        if stable:
            with stable_sorts():
                cm.process_batch(det, lab)
        else:
            cm.process_batch(det, lab)
        assert np.array_equal(cm.matrix, np.round(cm.matrix))
        out[b] = cm.matrix.astype(np.int32)
        kept = det[det[:, 4] > case["conf"]]
        if kept.shape[0]:
            iou = M.box_iou(lab[:, 1:], kept[:, :4]).numpy().astype(np.float64)
            thr = float(np.float32(case["iou_thres"]))
            if (np.abs(iou - thr) < 1e-4).any():
                bad.add("a")
            cand = np.where(iou > thr, iou, -1.0)
            for axis in (0, 1):
                if cand.shape[axis] >= 2:
                    top = np.sort(cand, axis=axis)
                    a, s = (top[-1], top[-2]) if axis == 0 else (top[:, -1], top[:, -2])
                    if ((s > 0) & (a - s < 1e-4)).any():
                        bad.add("b")
    return out, sorted(bad)


def condition_c(total, nc):
    core = total[:nc, :nc]
    need = {"diagonal": np.trace(core) > 0, "background row": total[nc, :nc].sum() > 0, "background column": total[:nc, nc].sum() > 0}
    if nc > 1:
        need["off the diagonal"] = core.sum() - np.trace(core) > 0
    return [k for k, v in need.items() if not v]


def main():
    G, R, M = load_reference()
    if "--time" in sys.argv:
        case = CC.timing_batch()
        boxes = [image_boxes(G, R, case, b) for b in range(16)]
        ts = []
        for _ in range(5):
            cm = M.ConfusionMatrix(16)
            t0 = time.perf_counter()
            for det, lab in boxes:
                cm.process_batch(det, lab)
            ts.append(time.perf_counter() - t0)
        print(f"reference ConfusionMatrix.process_batch, 16 images of ~300 detections x ~50 labels, CPU tensors: "
              f"median {sorted(ts)[2] * 1e3:.2f} ms per batch of {['%.2f' % (t * 1e3) for t in ts]} ms")
        return
    if "--default-sort" in sys.argv:
        for name in CC.TIE_NAMES:
            a = run_case(G, R, M, CC.build(name))[0]
            b = run_case(G, R, M, CC.build(name), stable=False)[0]
            print(f"{name}: {'DIFFERS' if not np.array_equal(a, b) else 'same'} ({int(np.abs(a - b).sum())} counts)")
        return
    if "--find-seeds" in sys.argv:
        for name in CC.RANDOM_NAMES:
            for seed in range(200):
                case = CC.build(name, seed=seed)
                out, bad = run_case(G, R, M, case)
                if not bad and not condition_c(out.sum(0), case["nc"]):
                    print(name, seed)
                    break
            else:
                print(name, "NO SEED")
        return
    store = {}
    for name in CC.NAMES:
        case = CC.build(name)
        out, bad = run_case(G, R, M, case)
        if name in CC.RANDOM:
            assert not bad, (name, bad)
            assert not condition_c(out.sum(0), case["nc"]), (name, condition_c(out.sum(0), case["nc"]))
        store[name] = out
    np.savez_compressed(os.path.join(HERE, "confusion_cases.npz"), **store)
    print(f"wrote tests/golden/confusion_cases.npz: {len(store)} cases")


if __name__ == "__main__":
    main()
