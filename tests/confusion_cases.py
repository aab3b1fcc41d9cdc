"""Seeded inputs of ConfusionMatrix for tests/golden/confusion_cases.npz (written by tests/golden/gen_confusion_cases.py from the
reference's own ConfusionMatrix.process_batch with every argsort stable) -- the golden file stores outputs only, one
(nc + 1, nc + 1) matrix per image of every case; the inputs are rebuilt here.

build(name) -> dict(preds, targets, shapes, nc, conf, iou_thres): a batch in the format of val.val_tail_batch --
  preds    list of (n_i, 7) float32 [x y l s theta conf cls]
  targets  (nt, 9) float32 [img cls cx cy l s theta + two spare columns]
  shapes   per image ((h, w), ((gain, gain), (pad_x, pad_y)))

EXACT cases (tie_*, thr_*, conf_*, nan_*, one_candidate, part_*): theta = 0, integer corner coordinates, integer pads, gain 1 or
2 -- every number of the chain and every IoU is exact in float32 on the host and on the device, so equal IoUs ARE equal.
RANDOM cases (lab_*, det_*, bs*, nc*): rotated boxes, fractional gains and pads; the generator checks that no decision hinges on
the last bits of sinf / cosf (its conditions (a) (b)) and that the summed matrix is non-trivial (c); SEEDS holds the seeds that
had to move for it."""
import numpy as np
import torch

CONF, IOU = 0.25, 0.45
ULP_BELOW_HALF = float(np.nextafter(np.float32(0.5), np.float32(0)))


def _labels(b, rows):
    """rows of (cls, x1, y1, x2, y2) -> targets rows [img cls cx cy l s 0 0 0] (axis-aligned; l along x)."""
    t = torch.zeros(len(rows), 9)
    for i, (c, x1, y1, x2, y2) in enumerate(rows):
        t[i] = torch.tensor([b, c, (x1 + x2) / 2, (y1 + y2) / 2, x2 - x1, y2 - y1, 0, 0, 0], dtype=torch.float32)
    return t


def _dets(rows):
    """rows of (x1, y1, x2, y2, conf, cls) -> (n, 7) [cx cy l s 0 conf cls]."""
    d = torch.zeros(len(rows), 7)
    for i, (x1, y1, x2, y2, cf, c) in enumerate(rows):
        d[i] = torch.tensor([(x1 + x2) / 2, (y1 + y2) / 2, x2 - x1, y2 - y1, 0, cf, c], dtype=torch.float32)
    return d


UNIT = ((600, 800), ((1.0, 1.0), (0.0, 0.0)))
HALF = ((1200, 1600), ((0.5, 0.5), (8.0, 6.0)))          # native = (letterboxed - pad) * 2: exact
BOX = (100, 100, 120, 110)                               # 20 x 10, even sides: the centre is an integer


def _shift(box, dx):
    return (box[0] + dx, box[1], box[2] + dx, box[3])


def _exact(images, nc=3, conf=CONF, iou_thres=IOU, shapes=None):
    """images: list of (label rows, detection rows)."""
    preds = [_dets(d) for _, d in images]
    tg = [_labels(b, l) for b, (l, _) in enumerate(images)]
    return dict(preds=preds, targets=torch.cat(tg, 0) if tg else torch.zeros(0, 9), nc=nc, conf=conf, iou_thres=iou_thres,
                shapes=shapes or [UNIT if b % 2 == 0 else HALF for b in range(len(images))])


def _tie_grid(seed, n_lab, n_det, nc=4, cell=8, span=6):
    """Boxes on a coarse integer grid (corners multiples of `cell`, sides 2 or 3 cells): dozens of equal IoUs per image."""
    rng = np.random.RandomState(seed)

    def boxes(k):
        x1 = rng.randint(0, span, k) * cell + 40
        y1 = rng.randint(0, span, k) * cell + 40
        return x1, y1, x1 + rng.randint(2, 4, k) * cell, y1 + rng.randint(2, 4, k) * cell
    lx1, ly1, lx2, ly2 = boxes(n_lab)
    dx1, dy1, dx2, dy2 = boxes(n_det)
    lab = [(int(rng.randint(nc)), int(a), int(b), int(c), int(d)) for a, b, c, d in zip(lx1, ly1, lx2, ly2)]
    det = [(int(a), int(b), int(c), int(d), float(np.float32(0.2 + 0.8 * rng.rand())), int(rng.randint(nc)))
           for a, b, c, d in zip(dx1, dy1, dx2, dy2)]
    return lab, det


def _exact_cases():
    B, B2 = BOX, _shift(BOX, 200)
    det_half = (100, 100, 120, 105)                      # inside BOX, half its area: IoU = 100 / 200 = 0.5 exactly
    det_55 = (100, 100, 111, 110)                        # 110 / 200 = 0.55
    c = {}
    # ---- ties (the expected cells follow from csrc/confusion_math.h's two rules; the golden file is the reference's answer)
    c["tie_two_labels_same_class"] = _exact([([(1, *B), (1, *B)], [(*B, 0.9, 1)])])
    c["tie_two_labels_other_class"] = _exact([([(0, *B), (2, *B)], [(*B, 0.9, 0)])])          # the HIGHER label: cell [0][2]
    c["tie_two_labels_other_class_perm"] = _exact([([(2, *B), (0, *B)], [(*B, 0.9, 0)])])     # rows swapped: cell [0][0]
    c["tie_two_dets"] = _exact([([(0, *B)], [(*B, 0.9, 0), (*B, 0.8, 1)])])                   # the HIGHER detection: [1][0], loser [0][nc]
    c["tie_two_dets_perm"] = _exact([([(0, *B)], [(*B, 0.8, 1), (*B, 0.9, 0)])])
    c["tie_3x3"] = _exact([([(k, *B) for k in range(3)], [(*B, 0.9 - 0.1 * k, k) for k in range(3)])])
    c["tie_3x3_perm"] = _exact([([(k, *B) for k in (1, 2, 0)], [(*B, 0.9 - 0.1 * i, k) for i, k in enumerate((2, 0, 1))])])
    # two 3 x 3 blocks and a mixed pair in one image, in the doubled frame as well
    blk = ([(k % 3, *(B if k < 3 else B2)) for k in range(6)], [(*(B if k % 2 else B2), 0.9, (k + 1) % 3) for k in range(6)])
    c["tie_blocks_two_frames"] = _exact([blk, blk])
    # 6 x 6 identical boxes = 36 equal candidates, and grids: past the 16 entries below which numpy's default sort is an insertion sort
    c["tie_6x6"] = _exact([([(k % 3, *B) for k in range(6)], [(*B, 0.9, (k + 1) % 3) for k in range(6)])])
    c["tie_grid"] = _exact([_tie_grid(1, 40, 60), _tie_grid(2, 25, 80), _tie_grid(3, 60, 30)], nc=4)
    g = _tie_grid(1, 40, 60)
    c["tie_grid_perm"] = _exact([(g[0][::-1], g[1][::-1])], nc=4)
    # ---- threshold and filter edges
    c["thr_equal"] = _exact([([(1, *B)], [(*det_half, 0.9, 1)])], iou_thres=0.5)              # 0.5 > 0.5 fails: no match at all
    c["thr_one_ulp_above"] = _exact([([(1, *B)], [(*det_half, 0.9, 1)])], iou_thres=ULP_BELOW_HALF)
    # float32(0.55) > 0.55: the comparison is made in float32 (threshold rounded), where 110 / 200 == float32(0.55) fails
    c["thr_rounded_to_f32"] = _exact([([(1, *B)], [(*det_55, 0.9, 1)])], iou_thres=0.55)
    c["conf_equal"] = _exact([([(1, *B), (2, *B2)], [(*B, 0.25, 1), (*B2, float(np.nextafter(np.float32(0.25), np.float32(1))), 2)])])
    nan = float("nan")
    c["nan_conf_and_box"] = _exact([([(1, *B), (2, *B2), (0, *_shift(B, 400))],
                                     [(*B, nan, 1), (*B2, 0.9, 2), (nan, 100, nan, 110, 0.9, 0), (*_shift(B, 400), 0.8, 1)])])
    c["one_candidate"] = _exact([([(1, *B), (2, *B2)], [(*B, 0.9, 0), (*_shift(B, 400), 0.9, 2)])])
    # ---- which images take part (val.py:217-246)
    c["part_rules"] = _exact([
        ([(1, *B), (2, *B2)], []),                                                 # labels, no detections: adds nothing
        ([], [(*B, 0.9, 1)]),                                                      # detections, no labels: adds nothing
        ([(1, *B), (2, *B2)], [(*B, 0.2, 1), (*B2, 0.1, 2)]),                      # none above conf: labels -> background row
        ([(1, *B), (0, *B2)], [(*_shift(B, 400), 0.9, 1), (*det_half, 0.9, 2)]),   # none above IoU: background row, detections NOT counted
        ([], []),                                                                  # both empty
        ([(1, *B), (2, *B2)], [(*B, 0.9, 1), (*_shift(B, 400), 0.9, 0)]),          # an ordinary image
    ])
    c["part_no_detections_in_batch"] = _exact([([(1, *B)], []), ([(2, *B2), (0, *B)], [])])
    return c


# ---- random cases: name -> (seed, nc, [(kept detections, dropped detections, labels), ...])
_ORD = (60, 15, 30)                                      # an ordinary image, added so that the sum meets condition (c)
RANDOM = {}
for _m in (1, 511, 512, 513):
    RANDOM[f"lab_{_m}"] = (0, 16, [(100, 20, _m), _ORD])
RANDOM["lab_1025_det_1000"] = (0, 16, [(1000, 0, 1025), _ORD])          # the largest: two label tiles plus one
for _n in (1, 63, 64, 65, 255, 256, 257, 1000, 1023, 1024, 1025):       # waves, 256 and the workgroup's 1024 threads
    RANDOM[f"det_{_n}"] = (0, 16, [(_n, 9, 40), _ORD])
RANDOM["bs1"] = (0, 16, [_ORD])
RANDOM["bs2"] = (0, 16, [_ORD, (7, 2, 5)])
RANDOM["bs64"] = (0, 3, [(5 + b % 4, b % 3, 3 + b % 5) for b in range(64)])       # image boundaries inside every wave of the packed rows
RANDOM["bs65"] = (0, 3, [(5 + b % 4, b % 3, 3 + b % 5) for b in range(65)])
for _nc in (1, 2, 16, 80, 109, 110):                                   # 109 | 110: the LDS histogram's cut-over
    RANDOM[f"nc{_nc}"] = (0, _nc, [_ORD, (40, 5, 50)])
SEEDS = {"lab_1025_det_1000": 2, "det_1000": 1}          # moved off 0 by gen_confusion_cases.py REF --find-seeds
for _k, _s in SEEDS.items():
    RANDOM[_k] = (_s,) + RANDOM[_k][1:]

JIT = np.array([1.5, 1.5, 2.0, 1.0, 0.02], dtype=np.float32)            # cx cy l s theta


def _random_image(rng, b, kept, dropped, n_lab, nc):
    t = np.zeros((n_lab, 9), dtype=np.float32)
    t[:, 0] = b
    t[:, 1] = rng.randint(nc, size=n_lab)
    t[:, 2:4] = rng.rand(n_lab, 2) * 900 + 50
    t[:, 4] = rng.rand(n_lab) * 60 + 12
    t[:, 5] = rng.rand(n_lab) * 20 + 6
    t[:, 6] = (rng.rand(n_lab) * 2 - 1) * 1.55
    n = kept + dropped
    d = np.zeros((n, 7), dtype=np.float32)
    src = rng.randint(n_lab, size=n)
    d[:, :5] = t[src, 2:7] + (rng.rand(n, 5).astype(np.float32) * 2 - 1) * JIT
    d[:, 6] = t[src, 1]
    stray = rng.rand(n) < 0.2                                           # a fifth lie somewhere else: the background column
    d[stray, :2] = (rng.rand(int(stray.sum()), 2) * 900 + 50).astype(np.float32)
    flip = rng.rand(n) < 0.2                                            # a fifth carry another class: off the diagonal
    d[flip, 6] = rng.randint(nc, size=int(flip.sum()))
    conf = np.concatenate((0.3 + 0.69 * rng.rand(kept), 0.24 * rng.rand(dropped))).astype(np.float32)
    d[:, 5] = conf[rng.permutation(n)]
    return torch.from_numpy(d), torch.from_numpy(t)


def _random(seed, nc, images):
    rng = np.random.RandomState(seed)
    preds, tgs, shapes = [], [], []
    for b, (kept, dropped, n_lab) in enumerate(images):
        d, t = _random_image(rng, b, kept, dropped, n_lab, nc)
        preds.append(d)
        tgs.append(t)
        gain = float(np.float32(0.6 + 0.4 * rng.rand()))
        shapes.append(((int(960 / gain) + b, int(940 / gain) - b), ((gain, gain), (4.0 + b % 3, 9.5 + 0.25 * b))))
    return dict(preds=preds, targets=torch.cat(tgs, 0), shapes=shapes, nc=nc, conf=CONF, iou_thres=IOU)


_EXACT = _exact_cases()
EXACT_NAMES = list(_EXACT)
RANDOM_NAMES = list(RANDOM)
NAMES = EXACT_NAMES + RANDOM_NAMES
TIE_NAMES = [k for k in EXACT_NAMES if k.startswith("tie_")]
_cache = {}


def build(name, seed=None):
    """The case's batch (cached and shared: treat it as read-only)."""
    if name in _EXACT:
        return _EXACT[name]
    if seed is not None:
        return _random(seed, *RANDOM[name][1:])
    if name not in _cache:
        _cache[name] = _random(*RANDOM[name])
    return _cache[name]


def labels_of(targets, b):
    return targets[targets[:, 0] == b]


def takes_part(case, b):
    """val.py:217-246: at least one detection row and at least one label."""
    return case["preds"][b].shape[0] > 0 and int((case["targets"][:, 0] == b).sum()) > 0


def host_boxes(case, b):
    """(pred_hbbn (n, 6), labels_hbbn (m, 5)) of image b through the restated chain of oracle/pyref.py, float32 on the host."""
    from oracle import pyref
    (h, w), ((gain, _), pad) = case["shapes"][b]
    det = pyref.val_postprocess(case["preds"][b].clone(), gain, pad)[3]
    return det, pyref.val_label_boxes(labels_of(case["targets"], b), gain, pad, (h, w))


def timing_batch(seed=0):
    """The shape of bench.py's validation batch: 16 images, about 300 detections and about 50 labels each, 16 classes (the input
    of tools/time_confusion.py and of gen_confusion_cases.py REF --time)."""
    return _random(seed, 16, [(240 + 8 * (b % 5), 60, 44 + b % 13) for b in range(16)])
