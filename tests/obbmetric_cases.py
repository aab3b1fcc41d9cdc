"""Inputs of the oriented-box process_batch tests (tests/test_obbmetric_host.py, tests/test_obbmetric_gpu.py) and of their
generator (tests/golden/gen_obbmetric_cases.py): the seeded builders, the stored golden file, and the pinned rule restated on a
given IoU matrix.

Detections are rows [cx cy l s theta conf cls] with descending confidences; an image's labels [cls cx cy l s theta] are jittered
copies of a subset of its detections plus distractors drawn apart from them, 2-3 classes.  A batch carries its labels as
`targets` rows [img cls cx cy l s theta]."""
import os

import numpy as np
import torch

IOUV = torch.linspace(0.5, 0.95, 10)
JIT = torch.tensor([1.5, 1.5, 2.0, 1.0, 0.02])      # cx cy l s theta
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "obbmetric_cases.npz")

# one image: name -> (n detections, m labels, classes)
SINGLE = {"n1_m1": (1, 1, 1), "n70_m9": (70, 9, 2), "n300_m40": (300, 40, 3)}
# the batch: per image (n detections, m labels, classes, near-duplicate labels on detection 0).  Image 0 has no detections,
# image 1 no labels; the boundaries 40 | 100 lie inside the first 128-detection workgroup, 230 inside the second; image 3 has
# more labels than one LDS tile (512) holds; the first detection of image 4 sits on 150 labels of its own class, which fill the
# queue of its wave (64 entries) twice before the tile ends.
BATCH = {"bs5": [(0, 12, 2, 0), (40, 0, 2, 0), (60, 25, 3, 0), (130, 600, 2, 0), (50, 160, 2, 150)]}
NAMES = list(SINGLE) + list(BATCH)


def make_image(g, n_det, n_lab, n_cls, ndup=0):
    """(detections (n_det, 7), labels (n_lab, 6)) of one image from the generator g."""
    d = torch.zeros(n_det, 7)
    d[:, :2] = torch.rand(n_det, 2, generator=g) * 900 + 50
    d[:, 2] = torch.rand(n_det, generator=g) * 60 + 12
    d[:, 3] = torch.rand(n_det, generator=g) * 20 + 6
    d[:, 4] = (torch.rand(n_det, generator=g) * 2 - 1) * 1.55
    d[:, 5] = torch.sort(torch.rand(n_det, generator=g), descending=True)[0]
    d[:, 6] = torch.randint(0, n_cls, (n_det,), generator=g).float()
    lab = torch.zeros(n_lab, 6)
    lab[:, 0] = torch.randint(0, n_cls, (n_lab,), generator=g).float()
    lab[:, 1:3] = torch.rand(n_lab, 2, generator=g) * 900 + 50
    lab[:, 3] = torch.rand(n_lab, generator=g) * 60 + 12
    lab[:, 4] = torch.rand(n_lab, generator=g) * 20 + 6
    lab[:, 5] = (torch.rand(n_lab, generator=g) * 2 - 1) * 1.55
    if n_det and n_lab:
        # three quarters of the remaining labels (all of them when there are few): jittered copies of distinct detections
        free = n_lab - ndup
        k = min(n_det, free if free <= 4 else 3 * free // 4)
        src = torch.randperm(n_det, generator=g)[:k]
        rows = ndup + torch.randperm(free, generator=g)[:k]
        lab[rows, 1:6] = d[src, :5] + (torch.rand(k, 5, generator=g) * 2 - 1) * JIT
        lab[rows, 0] = d[src, 6]
        if ndup:                                                 # detection 0 under `ndup` labels of its class
            lab[:ndup, 1:6] = d[0, :5] + (torch.rand(ndup, 5, generator=g) * 2 - 1) * JIT * 1.5
            lab[:ndup, 0] = d[0, 6]
    return d, lab


def build_single(name, seed):
    n, m, nc = SINGLE[name]
    return make_image(torch.Generator().manual_seed(seed), n, m, nc)


def build_batch(name, seed):
    """(preds: list of (n_i, 7), targets (nt, 7))."""
    g = torch.Generator().manual_seed(seed)
    preds, tgs = [], []
    for b, (n, m, nc, ndup) in enumerate(BATCH[name]):
        d, lab = make_image(g, n, m, nc, ndup)
        preds.append(d)
        tgs.append(torch.cat((torch.full((m, 1), float(b)), lab), 1))
    return preds, torch.cat(tgs, 0)


def labels_of(targets, b):
    """The (m_b, 6) labels of image b and their rows in `targets`."""
    rows = torch.nonzero(targets[:, 0] == b)[:, 0]
    return targets[rows, 1:7], rows


def load(name):
    """The stored case: single -> (pred, labels, correct); batch -> (preds list, targets, correct of the packed rows)."""
    G = np.load(GOLDEN)
    pred, correct = torch.from_numpy(G[f"{name}_pred"]), torch.from_numpy(G[f"{name}_correct"])
    if name in SINGLE:
        return pred, torch.from_numpy(G[f"{name}_labels"]), correct
    off = G[f"{name}_off"].tolist()
    return [pred[off[b]:off[b + 1]] for b in range(len(off) - 1)], torch.from_numpy(G[f"{name}_targets"]), correct


def riou(labels6, pred7):
    """The oracle's iou[l, d] = single_box_iou_rotated<float>(label, detection) as a float32 array (m, n)."""
    import oracle
    return oracle.riou_matrix(labels6[:, 1:6].numpy(), pred7[:, :5].numpy())


def rule(iou, lab_cls, det_cls, iouv):
    """The pinned rule on a given IoU matrix iou[l, d] (numpy float32): a pair is a candidate iff the classes are equal and
    iou >= iouv[0] (NaN never); a detection keeps its candidate of highest IoU, the lower label index among equals; a label
    keeps the lowest-indexed detection that kept it.  -> (correct (n, niou) bool, match_label (n) int32, match_iou (n) float32)."""
    iou = np.asarray(iou, dtype=np.float32)
    iouv = np.asarray(iouv, dtype=np.float32)
    m, n = iou.shape
    correct = np.zeros((n, len(iouv)), dtype=bool)
    match_label, match_iou = np.full(n, -1, dtype=np.int32), np.full(n, -1, dtype=np.float32)
    if n == 0 or m == 0:
        return correct, match_label, match_iou
    with np.errstate(invalid="ignore"):
        ok = (np.asarray(lab_cls, dtype=np.float32)[:, None] == np.asarray(det_cls, dtype=np.float32)[None, :]) & (iou >= iouv[0])
    taken = set()
    for d in range(n):
        cand = np.nonzero(ok[:, d])[0]
        if len(cand) == 0:
            continue
        best = cand[np.argmax(iou[cand, d])]                     # argmax: the first maximum, i.e. the lowest label index
        match_label[d], match_iou[d] = best, iou[best, d]
        if int(best) not in taken:
            taken.add(int(best))
            correct[d] = iou[best, d] >= iouv
    return correct, match_label, match_iou


def rule_batch(preds, targets, iouv, iou_of=riou):
    """The rule per image on the packed rows of a batch: match_label holds rows of `targets`."""
    out = []
    for b, p in enumerate(preds):
        lab, rows = labels_of(targets, b)
        n, m = p.shape[0], lab.shape[0]
        iou = iou_of(lab, p) if n and m else np.zeros((m, n), dtype=np.float32)
        c, ml, mi = rule(iou, lab[:, 0].numpy(), p[:, 6].numpy(), iouv)
        if m:
            ml = np.where(ml >= 0, rows.numpy().astype(np.int32)[np.maximum(ml, 0)], -1).astype(np.int32)
        out.append((c, ml, mi))
    return (np.concatenate([o[0] for o in out], 0), np.concatenate([o[1] for o in out]), np.concatenate([o[2] for o in out]))
