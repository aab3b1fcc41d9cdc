"""Inputs shared by tests/golden/gen_devkit_eval_cases.py (which freezes the reference's outputs on them in
tests/golden/devkit_eval_cases.npz) and tests/test_devkit_eval_host.py / test_devkit_eval_gpu.py.  Everything is seeded."""
import os

import numpy as np

from tests.golden.gen_golden import EVAL_CASES, EVAL_CLASSES, eval_inputs

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "devkit_eval_cases.npz")
AOE_THRESHOLDS = (0.5, 0.7)
MAX_REDRAWS = 20


def golden():
    return np.load(GOLDEN)


def _hull(vals):
    xs, ys = vals[0::2], vals[1::2]
    return min(xs), min(ys), max(xs), max(ys)


def task2_quad(x1, y1, x2, y2):
    """Task-2 ground-truth layout: the axis-aligned quad x1 y1 x2 y1 x2 y2 x1 y2 (parse_gt reads columns 0, 1, 4, 5)."""
    return f"{x1!r} {y1!r} {x2!r} {y1!r} {x2!r} {y2!r} {x1!r} {y2!r}"


# by hand, in an image of their own per class: truncation toward zero of fractional and negative coordinates, a duplicated box, a
# box whose column 4 is column 0 - 1 after truncation with a detection of xmax = xmin - 1 on it (both areas 0, inters 0: NaN),
# an image without ground truth of the class, repeated scores
HAND_GT = {
    "H0000": ["-3.7 -2.2 10.9 -2.2 10.9 8.6 -3.7 8.6 {c} 0",
              "-0.4 -0.9 0.7 -0.9 0.7 12.5 -0.4 12.5 {c}",
              "20.5 20.5 40.5 20.5 40.5 35.5 20.5 35.5 {c} 0",
              "20.5 20.5 40.5 20.5 40.5 35.5 20.5 35.5 {c} 0",
              "50.2 60.0 49.9 60.0 49.9 70.0 50.2 70.0 {c} 0",
              "80.9 80.1 99.2 80.1 99.2 95.8 80.9 95.8 {c} 1"],
    "H0001": ["5.0 5.0 30.0 5.0 30.0 25.0 5.0 25.0 harbor 0"],
}
HAND_DET = ["H0000 0.9 50.0 60.0 49.0 70.0",            # on the zero-area box: overlaps NaN
            "H0000 0.8 -3.0 -2.0 10.0 8.0",             # the truncated first box exactly (floor would give -4 -3)
            "H0000 0.8 -4.0 -3.0 10.0 8.0",
            "H0000 0.7 20.0 20.0 40.0 35.0",            # the duplicated box: the first index wins
            "H0000 0.7 21.0 20.0 40.0 35.0",            # ... claimed already
            "H0000 0.7 0.0 0.0 0.0 12.0",
            "H0000 0.50 80.0 80.0 99.0 95.0",           # a difficult box
            "H0001 0.50 5.0 5.0 30.0 25.0",             # no ground truth of this class in the image
            "H0000 0.3 500.0 500.0 510.0 520.0"]


def to_task2(gt1, det1):
    """A Task-1 set (eval_inputs) with every quad replaced by its horizontal hull: ground truth in Task-2 layout, detections as
    `image score xmin ymin xmax ymax`."""
    gt, det = {}, {}
    for image, lines in gt1.items():
        out = []
        for line in lines:
            tok = line.split(' ')
            if len(tok) < 9:
                out.append(line)
                continue
            out.append(task2_quad(*_hull([float(v) for v in tok[:8]])) + ' ' + ' '.join(tok[8:]))
        gt[image] = out
    for c, lines in det1.items():
        out = []
        for line in lines:
            tok = line.split(' ')
            out.append(' '.join(tok[:2]) + ' ' + ' '.join(repr(v) for v in _hull([float(v) for v in tok[2:]])))
        det[c] = out
    return gt, det


def task2_inputs(name, redraw=0):
    """{image -> Task-2 labelTxt lines}, {class -> Task2_<class>.txt lines} of case `name`: the Task-1 set of EVAL_CASES through
    to_task2, plus the rows above.  `redraw` moves the seed (the generator's refusal rule)."""
    n_img, n_gt, seed = EVAL_CASES[name]
    gt, det = to_task2(*eval_inputs(n_img, n_gt, seed + 1000 * redraw))
    gt["H0000"] = [line.format(c=c) for c in EVAL_CLASSES for line in HAND_GT["H0000"]]
    gt["H0001"] = list(HAND_GT["H0001"])
    for c in EVAL_CLASSES:
        det[c] = det[c][:len(det[c]) // 2] + HAND_DET + det[c][len(det[c]) // 2:]
    return gt, det


def task2_write(root, gt, det):
    """The set on disk the way the devkit expects it; (detpath, annopath, imagesetfile)."""
    os.makedirs(os.path.join(root, 'labelTxt')); os.makedirs(os.path.join(root, 'res'))
    for image, lines in gt.items():
        with open(os.path.join(root, 'labelTxt', image + '.txt'), 'w') as f:
            f.write('\n'.join(lines) + '\n')
    with open(os.path.join(root, 'imgnamefile.txt'), 'w') as f:
        f.write('\n'.join(gt) + '\n')
    for c, lines in det.items():
        with open(os.path.join(root, 'res', f'Task2_{c}.txt'), 'w') as f:
            f.write('\n'.join(lines) + '\n')
    return os.path.join(root, 'res', 'Task2_{:s}.txt'), os.path.join(root, 'labelTxt', '{:s}.txt'), os.path.join(root, 'imgnamefile.txt')


def rbox_quads():
    """About 200 quads for the dota_poly2rbox functions: rotated rectangles, exact 45-degree quads with integer corners in
    every corner order, axis-aligned boxes, squares, near-squares around the 1.15 edge ratio, a segment and a point."""
    rng = np.random.RandomState(11)
    quads = []

    def rect(cx, cy, w, h, t):
        c, s = np.cos(t), np.sin(t)
        q = []
        for sx, sy in ((1, 1), (1, -1), (-1, -1), (-1, 1)):
            q += [cx + sx * w / 2 * c - sy * h / 2 * s, cy + sx * w / 2 * s + sy * h / 2 * c]
        return q
    for _ in range(90):
        quads.append(rect(rng.rand() * 800, rng.rand() * 800, rng.rand() * 90 + 4, rng.rand() * 40 + 4, (rng.rand() - 0.5) * 2 * np.pi))
    for _ in range(30):                                              # near-square: both sides of the ratio branch
        w = rng.rand() * 50 + 10
        quads.append(rect(rng.rand() * 800, rng.rand() * 800, w, w * (1 + rng.rand() * 0.3), (rng.rand() - 0.5) * 2 * np.pi))
    for a, b in ((5, 2), (3, 3), (7, 1), (2, 9), (4, 4)):            # 45 degrees, integer corners
        base = [(10, 20), (10 + a, 20 + a), (10 + a - b, 20 + a + b), (10 - b, 20 + b)]
        for pts in (base, base[::-1]):
            for r in range(4):
                quads.append([float(v) for p in pts[r:] + pts[:r] for v in p])
    for w, h in ((10, 4), (4, 10), (6, 6), (1, 1), (115, 100), (23, 20)):   # axis-aligned, both directions, every start
        base = [(3, 5), (3 + w, 5), (3 + w, 5 + h), (3, 5 + h)]
        for pts in (base, base[::-1]):
            for r in range(4):
                quads.append([float(v) for p in pts[r:] + pts[:r] for v in p])
    quads.append([7.0, 7.0] * 4)                                     # a point
    quads.append([1.0, 2.0, 9.0, 6.0, 1.0, 2.0, 9.0, 6.0])           # a segment walked twice
    quads.append([-12.5, -3.25, 40.75, -3.25, 40.75, 18.5, -12.5, 18.5])
    return np.array(quads, dtype=np.float64)


OBB2HBB_FILES = {
    "Task1_plane.txt": "P0001 0.50 10.5 20.25 30.0 18.0 33.5 40.0 12.0 44.75\n"
                       "P0001 0.9 100.0 100.0 200.0 100.0 200.0 150.0 100.0 150.0\n"
                       "P0002 1e-05 -3.5 7.0 2.25 -8.0 9.0 1.0 4.0 12.5\n"
                       "P0002 0.123456789 1e3 2e3 1.5e3 2e3 1.5e3 2.5e3 1e3 2.5e3",
    "merged_small-vehicle.txt": "img_a 0.3  1.0 2.0 3.0 4.0 5.0 6.0 7.0 8.0\n"
                                "img_b 0.70 0.1 0.2 0.30000000000000004 0.4 100000000000000000000.0 6 7 1e-7\n",
}


def chain_tile_lines():
    from tests.golden.gen_golden import merge_input_lines
    return merge_input_lines(3, 25, 7, False)
