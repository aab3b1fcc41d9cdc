"""Inputs of the dense val.py-tail tests (tests/test_valtail_dense_gpu.py on the GPU, tests/test_valtail_oracle_host.py on the
host): one generator, the named cases, the oracle's side of the comparison and the coverage figures each case must reach.

An image is (n_det, n_lab, n_cls, hot, dup):
  hot > 0  three quarters of the detections are jittered copies of the first `hot` labels (then shuffled): many detections
           whose best label is the same one -- the prefix scan of k_vt_stats then needs more than one 64-entry trip
  dup > 0  the last `dup` labels are exact copies of the first `dup`: exact IoU ties
Labels are [img cls cx cy l s theta + two spare columns]; detections are label rows jittered by JIT and carry their label's
class; confidences descend, as non_max_suppression_obb returns them."""
import torch

from oracle import pyref

IOUV = torch.linspace(0.5, 0.95, 10)
JIT = torch.tensor([1.5, 1.5, 2.0, 1.0, 0.02])      # cx cy l s theta

# name -> (seed, [image, ...])
CASES = {
    # one image, one workgroup of k_vt_dets, on either side of its `nl <= kVtLabLds` (512) switch
    "lds_511": (11, [(128, 511, 2, 0, 0)]),
    "lds_512": (12, [(128, 512, 2, 0, 0)]),
    "lds_513": (13, [(128, 513, 2, 0, 0)]),
    # 128 detections = one workgroup over two images: 600 labels in its range, each image under 512
    "two_images_one_block": (20, [(60, 300, 2, 0, 0), (68, 300, 2, 0, 0)]),
    # max_det detections against DOTA-tile label counts; a hot image; no detections; no labels; duplicate labels
    "dense": (30, [(1000, 1500, 3, 0, 0), (700, 40, 1, 3, 0), (0, 20, 2, 0, 0), (129, 0, 2, 0, 0), (300, 600, 1, 0, 150)]),
    # image boundaries inside waves and workgroups of both kernels (128- and 256-thread blocks)
    "straddle": (40, [(100, 30, 2, 2, 0), (200, 3, 1, 1, 0), (1, 1, 1, 0, 0), (0, 0, 1, 0, 0), (127, 90, 2, 3, 0), (128, 10, 2, 1, 0),
                      (129, 700, 2, 0, 0), (257, 5, 1, 1, 0)]),
}


def make_image(g, b, n_det, n_lab, n_cls=2, hot=0, dup=0, axis=False, integer=False):
    """(detections (n_det, 7) [x y l s theta conf cls], labels (n_lab, 9)) of image b.  axis: theta = 0 everywhere;
    integer: every box coordinate rounded to an integer AFTER the jitter (exact arithmetic, exact ties)."""
    t = torch.zeros(n_lab, 9)
    t[:, 0] = b
    t[:, 1] = torch.randint(0, n_cls, (n_lab,), generator=g).float()
    t[:, 2:4] = torch.rand(n_lab, 2, generator=g) * 900 + 50
    t[:, 4] = torch.rand(n_lab, generator=g) * 60 + 12
    t[:, 5] = torch.rand(n_lab, generator=g) * 20 + 6
    t[:, 6] = 0.0 if axis else (torch.rand(n_lab, generator=g) * 2 - 1) * 1.55
    if integer:
        t[:, 2:4] = t[:, 2:4].round()
        t[:, 4:6] = (t[:, 4:6] / 2).round() * 2                  # even sides: the half extents are integers as well
    if dup:
        t[n_lab - dup:, 1:7] = t[:dup, 1:7]
    d = torch.zeros(n_det, 7)
    if n_det and n_lab:
        src = torch.randint(0, n_lab, (n_det,), generator=g)
        if hot:
            k = 3 * n_det // 4
            src[:k] = torch.randint(0, hot, (k,), generator=g)
            src = src[torch.randperm(n_det, generator=g)]
        d[:, :5] = t[src, 2:7] + (torch.rand(n_det, 5, generator=g) * 2 - 1) * JIT
        d[:, 6] = t[src, 1]
    elif n_det:
        d[:, :2] = torch.rand(n_det, 2, generator=g) * 900 + 50
        d[:, 2] = torch.rand(n_det, generator=g) * 60 + 12
        d[:, 3] = torch.rand(n_det, generator=g) * 20 + 6
        d[:, 4] = (torch.rand(n_det, generator=g) * 2 - 1) * 1.55
        d[:, 6] = torch.randint(0, n_cls, (n_det,), generator=g).float()
    if axis:
        d[:, 4] = 0.0
    if integer:
        d[:, :4] = d[:, :4].round()
        d[:, 2:4] = (d[:, 2:4] / 2).round().clamp(min=1) * 2
    d[:, 5] = torch.sort(torch.rand(n_det, generator=g), descending=True)[0]
    return d, t


def make_batch(seed, images, axis=False, integer=False, unit_frame=False):
    """preds (list of (n_i, 7)), targets (nt, 9), shapes [((h, w), ((gain, gain), (pad_x, pad_y)))]: gains in [0.6, 1.0], a
    pad and a native shape of its own for every image (the shape a little under the labels' extent: some labels are clipped).
    unit_frame: gain 1, pad 0 (with integer boxes every number in the chain is then exact)."""
    g = torch.Generator().manual_seed(seed)
    preds, tgs, shapes = [], [], []
    for b, im in enumerate(images):
        d, t = make_image(g, b, *im, axis=axis, integer=integer)
        preds.append(d)
        tgs.append(t)
        gain = 0.6 + 0.4 * float(torch.rand(1, generator=g))
        if unit_frame:
            shapes.append(((1100 + b, 1300 - b), ((1.0, 1.0), (0.0, 0.0))))
        else:
            shapes.append(((int(960 / gain) + b, int(940 / gain) - b), ((gain, gain), (4.0 + b % 3, 9.5 + 0.25 * b))))
    return preds, torch.cat(tgs, 0), shapes


def labels_of(targets, b):
    return targets[targets[:, 0] == b]


def oracle_correct(det_boxes6, labels_hbbn, iouv=IOUV):
    """val.py:238-248 for one image with the pinned tie rule: zeros when the image has no labels."""
    if labels_hbbn.shape[0] == 0:
        return torch.zeros(det_boxes6.shape[0], iouv.shape[0], dtype=torch.bool)
    return pyref.process_batch(det_boxes6, labels_hbbn, iouv, ties="first")


def oracle_chain(preds, targets, shapes, dtype=torch.float32):
    """The whole tail on the host: per image (the four box arrays of val_postprocess, labels_hbbn, correct)."""
    out = []
    for b, p in enumerate(preds):
        (h, w), ((gain, _), pad) = shapes[b]
        boxes = pyref.val_postprocess(p.to(dtype), gain, pad)
        lab = pyref.val_label_boxes(labels_of(targets, b), gain, pad, (h, w), dtype=dtype)
        out.append((boxes, lab, oracle_correct(boxes[3], lab, IOUV.to(dtype))))
    return out


def coverage(det_boxes6, labels_hbbn, thr=0.5):
    """What one image's boxes exercise: (most detections that chose the same best label, detections whose best IoU is reached
    by two or more labels)."""
    if det_boxes6.shape[0] == 0 or labels_hbbn.shape[0] == 0:
        return 0, 0
    iou = pyref.box_iou(labels_hbbn[:, 1:], det_boxes6[:, :4])
    ok = (iou >= thr) & (labels_hbbn[:, 0:1] == det_boxes6[:, 5])
    iou = torch.where(ok, iou, torch.full_like(iou, -1.0))
    best, arg = iou.max(0)
    hit = best >= thr
    chosen = int(torch.bincount(arg[hit], minlength=1).max()) if hit.any() else 0
    tied = int((((iou == best) & ok).sum(0) >= 2).sum())
    return chosen, tied
