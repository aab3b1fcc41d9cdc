"""Inputs of the in-memory Task-1 evaluation tests (yolov5_obb_amd.DOTA_devkit.dota_evaluation_task1.evaluate_rows), shared by
the generator of the frozen reference results (tests/golden/gen_task1_rows_golden.py) and the GPU tests: everything is
regenerated from seeds, only the reference's outputs are stored.

TIE-FREE sets: eval_inputs(...) of tests/golden/gen_golden.py with every score replaced by a distinct value (printed with repr,
so the text carries the double exactly).  Without ties np.argsort(-confidence) has one answer and the reference's voc_eval is
defined; its rec / prec / AP are frozen in tests/golden/task1_rows_reference.npz.
  a      (5, 30)    the small set
  b      (2, 700)   images with hundreds of records: several 64-lane rounds of k_eval_best_gt
  wide   3 classes, > 2100 detections (past the 2048-row LDS block of the bitonic sort, class segments that straddle a
         1024-row scan tile): the 'ship' records are relabelled 'harbor', so 'ship' has detections and no ground truth
         (npos = 0: NaN recalls) and 'harbor' has ground truth and no detection (skipped, as a class without a result file)."""
import numpy as np

from tests.golden.gen_golden import EVAL_CLASSES, eval_inputs

TIE_FREE = {'a': (5, 30, 0), 'b': (2, 700, 1), 'wide': (16, 120, 5)}
CLASSES = {'a': EVAL_CLASSES, 'b': EVAL_CLASSES, 'wide': ('plane', 'ship', 'harbor')}
_memo = {}


def memo(key, make):
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


def tie_free_set(name):
    """(gt: image -> labelTxt lines, det: class -> Task1 lines) with distinct scores over the whole set."""
    def make():
        gt, det = eval_inputs(*TIE_FREE[name])
        total = sum(len(v) for v in det.values())
        scores = (np.random.RandomState(100 + TIE_FREE[name][2]).permutation(total) + 1.0) / (total + 1.0)
        k = 0
        out = {}
        for c, lines in det.items():
            new = []
            for line in lines:
                tok = line.split(' ')
                tok[1] = repr(float(scores[k]))
                k += 1
                new.append(' '.join(tok))
            out[c] = new
        if name == 'wide':
            def relabel(line):
                tok = line.split(' ')
                if len(tok) >= 9 and tok[8] == 'ship':
                    tok[8] = 'harbor'
                return ' '.join(tok)
            gt = {im: [relabel(ln) for ln in lines] for im, lines in gt.items()}
        return gt, out
    return memo(('set', name), make)


def rows_of(det, imagenames, classnames, seed=None):
    """The (n, 11) float64 rows [8 coordinates, score, cls, image] of a det dict; seed: a seeded shuffle of the rows (classes
    and images interleaved), None: class after class in file order."""
    index = {n: i for i, n in enumerate(imagenames)}
    rows = []
    for ci, c in enumerate(classnames):
        for line in det.get(c, []):
            tok = line.split(' ')
            rows.append([float(v) for v in tok[2:10]] + [float(tok[1]), float(ci), float(index[tok[0]])])
    rows = np.array(rows, dtype=np.float64).reshape(-1, 11)
    if seed is not None:
        rows = rows[np.random.RandomState(seed).permutation(len(rows))]
    return rows


def parse_gt_lines(gt, imagenames, classnames):
    """(bbox8 (k, 8), cls (k,), img (k,), difficult (k,)) of the records whose name is in classnames (parse_gt's rules: lines
    with fewer than 9 tokens are skipped, 9 tokens: not difficult)."""
    cidx = {c: i for i, c in enumerate(classnames)}
    bbox, cls, img, diff = [], [], [], []
    for i, name in enumerate(imagenames):
        for line in gt[name]:
            tok = line.strip().split(' ')
            if len(tok) < 9 or tok[8] not in cidx:
                continue
            bbox.append([float(v) for v in tok[:8]]); cls.append(cidx[tok[8]]); img.append(i)
            diff.append(int(tok[9]) if len(tok) == 10 else 0)
    return np.array(bbox, dtype=np.float64).reshape(-1, 8), np.array(cls, dtype=np.int64), np.array(img, dtype=np.int64), np.array(diff, dtype=np.int64)


def voc_ap(rec, prec, use_07_metric):
    """dota_evaluation_task1.py:54-86, restated (the statements of the package's own voc_ap)."""
    with np.errstate(all='ignore'):
        if use_07_metric:
            ap = 0.
            for t in np.arange(0., 1.1, 0.1):
                p = 0 if np.sum(rec >= t) == 0 else np.max(prec[rec >= t])
                ap = ap + p / 11.
            return ap
        mrec = np.concatenate(([0.], rec, [1.]))
        mpre = np.concatenate(([0.], prec, [0.]))
        for i in range(mpre.size - 1, 0, -1):
            mpre[i - 1] = np.maximum(mpre[i - 1], mpre[i])
        i = np.where(mrec[1:] != mrec[:-1])[0]
        return np.sum((mrec[i + 1] - mrec[i]) * mpre[i + 1])


def expected_class(rows, cls_index, bbox8, gcls, gimg, gdiff, ovthresh=0.5):
    """The statements of voc_eval (:131-249) for one class on rows / records held in arrays, with the package's pinned tie rule
    np.argsort(-confidence, kind='stable') and oracle.pyref.task1_best_gt per detection: (rec, prec, ap07, ap, sorted_ind into
    the class's rows in input order)."""
    from oracle import pyref
    mine = rows[rows[:, 9] == cls_index]
    recs = {}
    for im in np.unique(gimg[gcls == cls_index]):
        sel = (gcls == cls_index) & (gimg == im)
        recs[int(im)] = {'bbox': bbox8[sel], 'difficult': gdiff[sel].astype(bool), 'det': [False] * int(sel.sum())}
    npos = int(sum((~r['difficult']).sum() for r in recs.values()))
    sorted_ind = np.argsort(-mine[:, 8], kind='stable')
    nd = len(mine)
    tp, fp = np.zeros(nd), np.zeros(nd)
    none = {'bbox': np.zeros((0, 8)), 'difficult': np.zeros(0, dtype=bool), 'det': []}
    for d, r in enumerate(sorted_ind):
        R = recs.get(int(mine[r, 10]), none)
        ovmax, jmax = pyref.task1_best_gt(mine[r, :8].copy(), R['bbox'])
        if ovmax > ovthresh:
            if not R['difficult'][jmax]:
                if not R['det'][jmax]:
                    tp[d] = 1.
                    R['det'][jmax] = 1
                else:
                    fp[d] = 1.
        else:
            fp[d] = 1.
    fp, tp = np.cumsum(fp), np.cumsum(tp)
    with np.errstate(all='ignore'):
        rec = tp / float(npos)
        prec = tp / np.maximum(tp + fp, np.finfo(np.float64).eps)
    return rec, prec, voc_ap(rec, prec, True), voc_ap(rec, prec, False), sorted_ind


def same(a, b):
    """exact equality of doubles, any NaN equal to any NaN (the payload of a device NaN is not numpy's)"""
    a, b = np.atleast_1d(np.asarray(a, dtype=np.float64)), np.atleast_1d(np.asarray(b, dtype=np.float64))
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and a[~na].tobytes() == b[~nb].tobytes())


def hand_made():
    """The claim rule on a hand-made set, one class of interest ('x') and a second one ('y'):
      image 0   one easy record; five detections on it (two with equal scores, 0.9: the lower row takes it), and a detection
                far from everything whose score ties with the fourth one on the record
      image 1   one difficult record with a detection on it (neither TP nor FP), one easy record of class y
      image 2   130 records of class x in a grid (several 64-lane rounds); detections on records 0, 64 and 129, one with a
                NaN score on record 100 (last position), one far from everything
      image 3   no record at all; one detection
    Returns (rows (n, 11), bbox8, cls, img, difficult, n_img, classnames)."""
    def box(cx, cy, w=40., h=16.):
        return [cx - w / 2, cy - h / 2, cx + w / 2, cy - h / 2, cx + w / 2, cy + h / 2, cx - w / 2, cy + h / 2]
    bbox, cls, img, diff, rows = [], [], [], [], []
    bbox.append(box(100, 100)); cls.append(0); img.append(0); diff.append(0)
    for k, s in enumerate([0.6, 0.9, 0.8, 0.7, 0.9]):
        rows.append(box(100 + k, 100.5) + [s, 0., 0.])
    rows.append(box(900, 900) + [0.7, 0., 0.])
    bbox.append(box(300, 300)); cls.append(0); img.append(1); diff.append(1)
    bbox.append(box(300, 300)); cls.append(1); img.append(1); diff.append(0)
    rows.append(box(301, 300) + [0.95, 0., 1.])
    rows.append(box(301, 300) + [0.5, 1., 1.])
    for k in range(130):
        bbox.append(box(60 * (k % 13) + 50, 40 * (k // 13) + 50)); cls.append(0); img.append(2); diff.append(0)
    for k, s in ((0, 0.85), (64, 0.75), (129, 0.65), (100, float('nan'))):
        rows.append(box(60 * (k % 13) + 51, 40 * (k // 13) + 50) + [s, 0., 2.])
    rows.append(box(5000, 5000) + [0.99, 0., 2.])
    rows.append(box(64 * 13 + 51, 50) + [0.3, 0., 2.])               # a second claim on nothing: next to the grid
    rows.append(box(100, 100) + [0.4, 0., 3.])
    return (np.array(rows, dtype=np.float64), np.array(bbox, dtype=np.float64), np.array(cls), np.array(img), np.array(diff), 4, ('x', 'y'))
