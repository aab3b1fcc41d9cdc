"""Freezes the reference's OWN process_batch (val.py:69-90) with the rotated IoU in place of box_iou, on the seeded cases of
tests/obbmetric_cases.py -> tests/golden/obbmetric_cases.npz.  Needs a checkout of the reference where
tests/golden/gen_golden.py expects it, and the oracle built with its reference shims (oracle/_ref):

    python tests/golden/gen_obbmetric_cases.py

The reference's val.py is imported with the stubs of gen_golden.py; for every image `val.box_iou` is replaced by a closure that
returns oracle.riou_matrix(labels[:, 1:6], pred[:, :5]) -- iou[l, d] = single_box_iou_rotated<float>(label, detection), boxes in
the letterboxed frame -- and V.process_batch runs as it stands on (n, 6) / (m, 5) arrays that carry the classes.  An image
without labels keeps all-zero rows (val.py:238 `if nl:`), an image without detections has none.

The npz holds inputs and `correct` only: iouv; per single case NAME_pred (n, 7), NAME_labels (m, 6), NAME_correct (n, 10); per
batch NAME_pred (N, 7) packed, NAME_off (bs + 1), NAME_targets (nt, 7), NAME_correct (N, 10).

A case is REFUSED, and redrawn with the next seed, when in any image
 (a) the IoU of a pair of equal class lies within 1e-5 of a level of iouv, or
 (b) the best and the second-best candidate IoU of a detection differ by less than 1e-5
(double sin / cos of two maths libraries differ in the last bit of 2 IoUs in 200k; 1e-5 is about 80 such ulps and
SURVEY's scalar tolerance): on the stored inputs a device result has to equal the reference exactly, on every row."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
import oracle                                  # noqa: E402
from tests import obbmetric_cases as OC        # noqa: E402
from tests.golden import gen_golden            # noqa: E402

SEED0 = {"n1_m1": 100, "n70_m9": 200, "n300_m40": 300, "bs5": 400}


def reference_correct(V, pred, labels, iouv):
    """V.process_batch with the rotated IoU of (labels (m, 6), pred (n, 7)); also the IoU matrix it used."""
    iou = oracle.riou_matrix(labels[:, 1:6].numpy(), pred[:, :5].numpy())
    orig = V.box_iou
    V.box_iou = lambda a, b: torch.from_numpy(iou)
    try:
        det6 = torch.cat((torch.zeros(pred.shape[0], 4), pred[:, 5:7]), 1)
        lab5 = torch.cat((labels[:, 0:1], torch.zeros(labels.shape[0], 4)), 1)
        correct = V.process_batch(det6, lab5, iouv)
    finally:
        V.box_iou = orig
    return correct, iou


def refused(iou, labels, pred, iouv):
    """The conditions (a), (b) an image violates."""
    same = labels[:, 0:1].numpy() == pred[:, 6].numpy()[None, :]
    bad = set()
    v = iou.astype(np.float64)
    if (np.abs(v[same][:, None] - iouv.numpy().astype(np.float64)[None, :]) < 1e-5).any():
        bad.add("a")
    cand = np.where(same & (iou >= iouv.numpy()[0]), v, -np.inf)
    if cand.shape[0] >= 2:
        top = np.sort(cand, axis=0)
        two = top[-2] > -np.inf                                    # detections with a second candidate
        if (top[-1][two] - top[-2][two] < 1e-5).any():
            bad.add("b")
    return bad


def image(V, pred, labels, iouv):
    if pred.shape[0] == 0 or labels.shape[0] == 0:
        return torch.zeros(pred.shape[0], iouv.shape[0], dtype=torch.bool), set()
    correct, iou = reference_correct(V, pred, labels, iouv)
    return correct, refused(iou, labels, pred, iouv)


def main():
    here = os.getcwd()
    gen_golden.load_reference()
    import val as V                                              # the reference's val.py
    os.chdir(here)
    iouv = OC.IOUV
    store = {"iouv": iouv.numpy()}
    for name in OC.NAMES:
        for seed in range(SEED0[name], SEED0[name] + 100):
            if name in OC.SINGLE:
                pred, labels = OC.build_single(name, seed)
                correct, bad = image(V, pred, labels, iouv)
                case = {f"{name}_pred": pred.numpy(), f"{name}_labels": labels.numpy(), f"{name}_correct": correct.numpy()}
            else:
                preds, targets = OC.build_batch(name, seed)
                res = [image(V, p, OC.labels_of(targets, b)[0], iouv) for b, p in enumerate(preds)]
                bad = set().union(*[r[1] for r in res])
                off = np.cumsum([0] + [p.shape[0] for p in preds]).astype(np.int64)
                correct = torch.cat([r[0] for r in res], 0)
                case = {f"{name}_pred": torch.cat(preds, 0).numpy(), f"{name}_off": off, f"{name}_targets": targets.numpy(),
                        f"{name}_correct": correct.numpy()}
            if not bad:
                break
            print(f"{name}: seed {seed} refused ({sorted(bad)}), redrawn")
        assert not bad, (name, "no seed in range meets the conditions")
        assert name == "n1_m1" or int(correct.any(1).sum()) >= 3, (name, "too few matches to test anything")
        print(f"{name}: seed {seed}, {correct.shape[0]} detections, {int(correct[:, 0].sum())} correct at {float(iouv[0]):.2f}, "
              f"{int(correct[:, -1].sum())} at {float(iouv[-1]):.2f}")
        store.update(case)
    np.savez_compressed(OC.GOLDEN, **store)
    print(f"wrote {os.path.relpath(OC.GOLDEN, ROOT)}: {len(OC.NAMES)} cases, {os.path.getsize(OC.GOLDEN)} bytes")


if __name__ == "__main__":
    main()
