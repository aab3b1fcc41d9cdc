"""Host: the oracle's side of the dense val.py-tail tests -- process_batch's pinned tie rule (oracle/pyref.py, ties="first"),
val_label_boxes, and the coverage the shared cases of tests/valtail_cases.py must keep reaching.  No GPU."""
import os

import numpy as np
import pytest
import torch

from oracle import pyref
from tests import valtail_cases as VC

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "reference_outputs.npz"))


def rule_model(det, labels, iouv):
    """The kernels' documented rule (csrc/head.hip: k_pb_best / k_pb_correct), restated without any sort: a detection keeps the
    FIRST label in label order among those of its class with the highest IoU >= iouv[0]; a label keeps the LOWEST-indexed
    detection that chose it."""
    n, m = det.shape[0], labels.shape[0]
    correct = torch.zeros(n, iouv.shape[0], dtype=torch.bool)
    if n == 0 or m == 0:
        return correct
    iou = pyref.box_iou(labels[:, 1:], det[:, :4])
    ok = (iou >= iouv[0]) & (labels[:, 0:1] == det[:, 5])
    masked = torch.where(ok, iou, torch.full_like(iou, -1.0))
    best = masked.max(0)[0]
    first = ((masked == best) & ok).int().argmax(0)              # argmax of 0 / 1: the first maximum
    taken = set()
    for d in range(n):
        if best[d] >= iouv[0] and int(first[d]) not in taken:
            taken.add(int(first[d]))
            correct[d] = best[d] >= iouv
    return correct


def test_pinned_tie_rule_equals_the_reference_on_its_tie_free_fixtures():
    from tests.golden.gen_golden import VALPOST_CASES, valpost_inputs
    for name, (n, m, seed) in VALPOST_CASES.items():
        det, labels, iouv = valpost_inputs(n, m, seed)
        pinned = pyref.process_batch(det, labels, iouv, ties="first")
        assert torch.equal(pinned, pyref.process_batch(det, labels, iouv)), name
        assert np.array_equal(pinned.numpy(), G[f"pb_{name}"]), name
        assert torch.equal(pinned, rule_model(det, labels, iouv)), name


def _tie_case(n=600, groups=40, singles=30, seed=3):
    """Axis-aligned labels on a grid, far apart (a detection overlaps its own label only): `singles` + `groups` distinct boxes,
    then exact copies of the first `groups` of them appended at the end.  Detections: jittered copies, integer coordinates."""
    g = torch.Generator().manual_seed(seed)
    k = groups + singles
    cx = (torch.arange(k) % 10).float() * 100 + 50
    cy = (torch.arange(k) // 10).float() * 100 + 50
    w = torch.randint(10, 30, (k,), generator=g).float() * 2
    h = torch.randint(5, 20, (k,), generator=g).float() * 2
    box = torch.stack((cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2), 1)
    labels = torch.cat((torch.zeros(k, 1), box), 1)
    labels = torch.cat((labels, labels[:groups]), 0)             # label groups + j duplicates label j
    src = torch.randint(0, k, (n,), generator=g)
    det = torch.cat((box[src] + torch.randint(-3, 4, (n, 4), generator=g).float(), torch.sort(torch.rand(n, generator=g), descending=True)[0][:, None],
                     torch.zeros(n, 1)), 1)
    return det, labels, src, k


def test_pinned_tie_rule_on_duplicate_labels_one_winner_per_group_the_lowest_index():
    groups = 40
    det, labels, src, k = _tie_case(groups=groups)
    iouv = VC.IOUV
    got = pyref.process_batch(det, labels, iouv, ties="first")
    for _ in range(3):                                           # (ties=None on this input is implementation-defined: not asserted)
        assert torch.equal(pyref.process_batch(det.clone(), labels.clone(), iouv, ties="first"), got)
    iou = pyref.box_iou(labels[:, 1:], det[:, :4])
    assert int((iou[:k] > 0).sum(0).max()) == 1, "the grid keeps the distinct boxes apart"
    tied = 0
    for j in range(k):
        cand = torch.nonzero((src == j) & (iou[j] >= iouv[0]))[:, 0]           # the detections that can match box j (and its copy)
        rows = torch.nonzero(got.any(1) & (src == j))[:, 0]
        if len(cand) == 0:
            assert len(rows) == 0
            continue
        # ONE winner for the box, duplicated or not: every candidate keeps the first copy, the second copy stays unmatched
        assert rows.tolist() == [int(cand.min())], (j, rows.tolist(), cand.tolist())
        assert torch.equal(got[rows[0]], iou[j, rows[0]] >= iouv)
        tied += len(cand) if j < groups else 0
    assert tied >= 100
    assert int(got.any(1).sum()) <= k
    assert torch.equal(got, rule_model(det, labels, iouv))


def test_val_label_boxes_chain():
    """rbox2poly -> poly2hbb -> xywh2xyxy -> minus pad -> over gain -> clip (val.py:238-243, utils/general.py:621-633)."""
    t = torch.tensor([[3, 2, 100.0, 60.0, 40.0, 10.0, 0.0, 9, 9],          # axis-aligned: by hand
                      [3, 5, 10.0, 500.0, 40.0, 10.0, 0.0, 9, 9],          # left of the frame after the pad: clipped to 0
                      [3, 1, 990.0, 700.0, 60.0, 20.0, 0.0, 9, 9]])        # beyond the native width and height: clipped
    got = pyref.val_label_boxes(t, 0.5, (4.0, 10.0), (1300, 1900))
    want = torch.tensor([[2, 152.0, 90.0, 232.0, 110.0], [5, 0.0, 970.0, 52.0, 990.0], [1, 1900.0, 1300.0, 1900.0, 1300.0]])
    assert got.dtype == torch.float32 and torch.equal(got, want)
    assert torch.equal(pyref.val_label_boxes(t, 0.5, (4.0, 10.0), (1300, 1900), dtype=torch.float64), want.double())
    assert pyref.val_label_boxes(t[:0], 0.5, (4.0, 10.0), (1300, 1900)).shape == (0, 5)
    # rotated rows: float32 against float64, and against the detection chain (scale_polys first, hull second: the same box up
    # to rounding where nothing is clipped)
    g = torch.Generator().manual_seed(5)
    _, lab = VC.make_image(g, 0, 0, 400)
    gain, pad, hw = 0.7314, (12.0, 3.5), (5000, 5000)
    b32 = pyref.val_label_boxes(lab, gain, pad, hw)
    b64 = pyref.val_label_boxes(lab, gain, pad, hw, dtype=torch.float64)
    assert torch.allclose(b32.double(), b64, rtol=1e-6, atol=2e-4)
    as_det = torch.cat((lab[:, 2:7], torch.zeros(400, 1), lab[:, 1:2]), 1)
    assert torch.allclose(b32[:, 1:], pyref.val_postprocess(as_det, gain, pad)[3][:, :4], rtol=1e-6, atol=2e-4)
    small = pyref.val_label_boxes(lab, gain, pad, (700, 900))
    assert float(small[:, [1, 3]].max()) == 900.0 and float(small[:, [2, 4]].max()) == 700.0 and float(small[:, 1:].min()) >= 0.0


# what each shared case must exercise (the reference chain in float32 on the host; the GPU tests assert the same on the device's boxes)
@pytest.mark.parametrize("name", list(VC.CASES))
def test_shared_cases_reach_the_mechanisms_they_are_named_for(name):
    seed, images = VC.CASES[name]
    preds, targets, shapes = VC.make_batch(seed, images)
    chain = VC.oracle_chain(preds, targets, shapes)
    rows = sum(int(c.any(1).sum()) for _, _, c in chain)
    cov = [VC.coverage(boxes[3], lab) for boxes, lab, _ in chain]
    chosen, tied = max(c[0] for c in cov), sum(c[1] for c in cov)
    if name.startswith("lds_"):
        assert rows >= 40
    elif name == "two_images_one_block":
        assert rows >= 50
    elif name == "dense":
        assert chosen >= 130 and tied >= 100
    elif name == "straddle":
        assert chosen >= 65
    for (boxes, lab, correct) in chain:                          # the pinned oracle is the sort-free rule on every row
        assert torch.equal(correct, rule_model(boxes[3], lab, VC.IOUV))
