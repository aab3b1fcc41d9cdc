"""Generate tests/golden/devkit_eval_cases.npz from the REFERENCE ITSELF (run in the build container only):

    python tests/golden/gen_devkit_eval_cases.py

What is frozen, all from the reference's own DOTA_devkit files imported in place (numpy's removed aliases np.bool / np.float
set, matplotlib stubbed, the SWIG module polyiou backed by the reference's polyiou.cpp compiled into oracle/_ref, as
gen_golden.py section H / I does):
  * dota_evaluation_task2.voc_eval (rec, prec, both APs) on the Task-2 sets of tests/devkit_eval_cases.task2_inputs;
  * mAOE_evaluation.aoe_eval (the contributing detections and their angle errors) on the Task-1 sets of EVAL_CASES at
    ovthresh 0.5 and 0.7;
  * dota_poly2rbox.poly2rbox_single / _v2 / _v3 / rbox2poly_single / get_best_begin_point_single on rbox_quads();
  * results_obb2hbb.OBB2HBB on OBB2HBB_FILES;
  * the chain ResultMerge (polygon NMS) -> OBB2HBB -> Task-2 voc_eval on chain_tile_lines(), with its ground-truth text.
Refusals: a Task-2 case with an equal-image pair whose overlap is within 1e-9 of ovthresh is redrawn (another seed, at most
MAX_REDRAWS times, the count is stored); an mAOE case fails when a contributing box has its edge ratio within 1e-4 of 1.15, in
the near-square branch ||a1| - |a2|| < 1e-6, or a pre-wrap angle within 1e-9 of -pi/4 or 3pi/4.
"""
import contextlib
import ctypes as C
import io
import os
import sys
import tempfile
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, ROOT)

import oracle                                                      # noqa: E402
from tests import devkit_eval_cases as DC                          # noqa: E402
from tests.golden.gen_golden import EVAL_CASES, EVAL_CLASSES, eval_inputs, eval_write   # noqa: E402


def load_reference():
    oracle.build(with_ref=True)
    np.bool = bool
    np.float = float
    pol = C.CDLL(os.path.join(ROOT, 'oracle/_ref/libref_polyiou.so'))
    f64p = np.ctypeslib.ndpointer(np.float64, flags='C')
    pol.ref_iou_poly.restype = C.c_double
    pol.ref_iou_poly.argtypes = [f64p, f64p]
    stubp = types.ModuleType('polyiou')
    stubp.VectorDouble = lambda v: np.ascontiguousarray(v, dtype=np.float64)
    stubp.iou_poly = lambda p, q: pol.ref_iou_poly(p, q)
    sys.modules['polyiou'] = stubp
    sys.modules['DOTA_devkit.polyiou'] = stubp
    sys.modules.setdefault('shapely', types.ModuleType('shapely'))
    sys.modules['shapely.geometry'] = types.ModuleType('shapely.geometry')
    sys.modules.setdefault('matplotlib', types.ModuleType('matplotlib'))
    sys.modules.setdefault('matplotlib.pyplot', types.ModuleType('matplotlib.pyplot'))
    sys.path.insert(0, os.path.join(REF, 'DOTA_devkit'))            # mAOE_evaluation imports dota_poly2rbox by its bare name
    sys.path.insert(0, REF)
    import DOTA_devkit
    DOTA_devkit.polyiou = stubp
    import dota_evaluation_task2 as T2
    import dota_poly2rbox as RP
    import mAOE_evaluation as MA
    import results_obb2hbb as OH
    import DOTA_devkit.ResultMerge_multi_process as RM
    return T2, RP, MA, OH, RM


def quiet(fn, *args, **kw):
    with contextlib.redirect_stdout(io.StringIO()), warnings.catch_warnings(), np.errstate(all='ignore'):
        warnings.simplefilter('ignore')
        return fn(*args, **kw)


def task2_near_threshold(gt, det, ovthresh):
    """True when some detection x same-image, same-class box overlap is within 1e-9 of ovthresh."""
    for c in EVAL_CLASSES:
        boxes = {}
        for image, lines in gt.items():
            rows = [ln.split(' ') for ln in lines]
            boxes[image] = np.array([[int(float(t[0])), int(float(t[1])), int(float(t[4])), int(float(t[5]))]
                                     for t in rows if len(t) >= 9 and t[8] == c], dtype=np.float64).reshape(-1, 4)
        for line in det[c]:
            tok = line.split(' ')
            g, b = boxes[tok[0]], [float(v) for v in tok[2:6]]
            if not len(g):
                continue
            with np.errstate(all='ignore'):
                iw = np.maximum(np.minimum(g[:, 2], b[2]) - np.maximum(g[:, 0], b[0]) + 1., 0.)
                ih = np.maximum(np.minimum(g[:, 3], b[3]) - np.maximum(g[:, 1], b[1]) + 1., 0.)
                ov = iw * ih / ((b[2] - b[0] + 1.) * (b[3] - b[1] + 1.) + (g[:, 2] - g[:, 0] + 1.) * (g[:, 3] - g[:, 1] + 1.) - iw * ih)
            if (np.abs(ov - ovthresh) < 1e-9).any():
                return True
    return False


def aoe_refuse(RP, polys, what):
    """The refusal rules of the module docstring on the quads that went through poly2rbox_single_v3.  The edge lengths are the
    reference's own (width, height of its poly2rbox_single_v3: the longer and the shorter edge in both branches), the wrap is its
    norm_angle, the two edge angles are numpy's arctan2 of the float32 corner differences; nothing of this package is used."""
    with np.errstate(all='ignore'):
        wh = np.array([RP.poly2rbox_single_v3(p)[2:4] for p in polys])
        ratio = wh[:, 0] / wh[:, 1]
    p32 = polys.astype(np.float32)
    edge1 = np.hypot((p32[:, 0] - p32[:, 2]).astype(np.float64), (p32[:, 1] - p32[:, 3]).astype(np.float64))
    edge2 = np.hypot((p32[:, 2] - p32[:, 4]).astype(np.float64), (p32[:, 3] - p32[:, 5]).astype(np.float64))
    a1 = np.arctan2((p32[:, 3] - p32[:, 1]).astype(np.float64), (p32[:, 2] - p32[:, 0]).astype(np.float64))
    a2 = np.arctan2((p32[:, 7] - p32[:, 1]).astype(np.float64), (p32[:, 6] - p32[:, 0]).astype(np.float64))
    assert not (np.abs(ratio - 1.15) < 1e-4).any(), what + ": edge ratio at 1.15"
    sq = ratio < 1.15
    assert not (np.abs(np.abs(RP.norm_angle(a1[sq])) - np.abs(RP.norm_angle(a2[sq]))) < 1e-6).any(), what + ": near-square tie"
    used = np.concatenate([a1[sq], a2[sq], np.where(edge1 > edge2, a1, a2)[~sq]])
    for bound in (-np.pi / 4, 3 * np.pi / 4):
        assert not (np.abs(used - bound) < 1e-9).any(), what + ": angle at a wrap boundary"
    return int(sq.sum())


def main():
    T2, RP, MA, OH, RM = load_reference()
    out = {}

    # ------------------------------------------------------------------ Task 2
    for name in EVAL_CASES:
        for redraw in range(DC.MAX_REDRAWS + 1):
            gt, det = DC.task2_inputs(name, redraw)
            if not task2_near_threshold(gt, det, 0.5):
                break
        else:
            raise SystemExit(f"task2 {name}: no case within {DC.MAX_REDRAWS} redraws")
        out[f'task2_{name}_redraw'] = np.array(redraw)
        with tempfile.TemporaryDirectory() as td:
            detpath, annopath, imagesetfile = DC.task2_write(td, gt, det)
            for cls in EVAL_CLASSES:
                for m07 in (True, False):
                    rec, prec, ap = quiet(T2.voc_eval, detpath, annopath, imagesetfile, cls, ovthresh=0.5, use_07_metric=m07)
                    out[f'task2_{name}_{cls}_ap{int(m07)}'] = np.array(ap)
                out[f'task2_{name}_{cls}_rec'] = rec
                out[f'task2_{name}_{cls}_prec'] = prec
                print(f"task2 {name} {cls}: redraw {redraw} nd {len(rec)} ap07 {float(out[f'task2_{name}_{cls}_ap1']):.4f} "
                      f"ap {ap:.4f} nan in prec {int(np.isnan(prec).sum())}")
            if name == 'a':                                          # parse_gt on the hand-made image: truncation toward zero
                objs = T2.parse_gt(annopath.format('H0000'))
                out['task2_parse_gt_bbox'] = np.array([o['bbox'] for o in objs], dtype=np.int64)
                out['task2_parse_gt_difficult'] = np.array([o['difficult'] for o in objs], dtype=np.int64)
                out['task2_parse_gt_area'] = np.array([o['area'] for o in objs], dtype=np.int64)
                out['task2_parse_gt_name'] = np.array([o['name'] for o in objs])

    # voc_ap on fixed curves
    rng = np.random.RandomState(4)
    for k, n in enumerate((1, 7, 200)):
        tp = (rng.rand(n) < 0.6).astype(np.float64)
        rec = np.cumsum(tp) / max(tp.sum() + 3, 1)
        prec = np.cumsum(tp) / np.arange(1, n + 1)
        out[f'vocap_{k}_rec'], out[f'vocap_{k}_prec'] = rec, prec
        out[f'vocap_{k}_ap'] = np.array([T2.voc_ap(rec, prec, True), T2.voc_ap(rec, prec, False)])

    # ------------------------------------------------------------------ mAOE on the Task-1 sets
    calls = []
    v3 = RP.poly2rbox_single_v3

    def recording_v3(poly):
        calls.append(np.array(poly[:8], dtype=np.float64))
        return v3(poly)
    MA.poly2rbox_single_v3 = recording_v3
    n_calls = n_square = 0
    for name, cfg in EVAL_CASES.items():
        gt, det = eval_inputs(*cfg)
        with tempfile.TemporaryDirectory() as td:
            detpath, annopath, imagesetfile = eval_write(td, gt, det)
            for thr in DC.AOE_THRESHOLDS:
                for cls in EVAL_CLASSES:
                    del calls[:]
                    difs = quiet(MA.aoe_eval, detpath, annopath, imagesetfile, cls, ovthresh=thr)
                    assert len(calls) == 2 * len(difs) and len(difs) > 0
                    polys = np.array(calls)
                    n_square += aoe_refuse(RP, polys, f"aoe {name} {cls} {thr}")
                    n_calls += len(polys)
                    # the contributing detections as positions in confidence order (the reference returns only the errors)
                    conf = np.array([float(x.split(' ')[1]) for x in det[cls]])
                    BB = np.array([[float(v) for v in x.split(' ')[2:]] for x in det[cls]])[np.argsort(-conf)]
                    hits, at = [], 0
                    for bb in polys[1::2]:
                        while not np.array_equal(BB[at], bb):
                            at += 1
                        hits.append(at)
                        at += 1
                    key = f'aoe_{name}_{cls}_{thr}'
                    out[key + '_hits'] = np.array(hits, dtype=np.int32)
                    out[key + '_gt'] = polys[0::2]
                    out[key + '_dif'] = np.array(difs, dtype=np.float64)
                    print(f"aoe {name} {cls} {thr}: {len(difs)} hits, mean {np.mean(difs):.2f} max {np.max(difs):.1f}")
    MA.poly2rbox_single_v3 = v3
    print(f"aoe: {n_calls} poly2rbox_single_v3 calls, {n_square} in the ratio < 1.15 branch")

    # ------------------------------------------------------------------ dota_poly2rbox on fixed quads
    quads = DC.rbox_quads()
    r1 = np.array([quiet(RP.poly2rbox_single, q) for q in quads])
    out['rbox_v1'] = r1
    out['rbox_v2'] = np.array([quiet(RP.poly2rbox_single_v2, q) for q in quads])
    out['rbox_v3'] = np.array([quiet(RP.poly2rbox_single_v3, q) for q in quads])
    out['rbox_back'] = np.array([quiet(RP.rbox2poly_single, r) for r in r1])
    out['rbox_begin'] = np.array([RP.get_best_begin_point_single(q) for q in quads])
    assert out['rbox_back'].dtype == np.float32 and out['rbox_begin'].dtype == np.float64
    print(f"poly2rbox: {len(quads)} quads")

    # ------------------------------------------------------------------ OBB2HBB
    with tempfile.TemporaryDirectory() as td:
        os.makedirs(os.path.join(td, 'src'))
        for fn, text in DC.OBB2HBB_FILES.items():
            with open(os.path.join(td, 'src', fn), 'w') as f:
                f.write(text)
        OH.OBB2HBB(os.path.join(td, 'src'), os.path.join(td, 'dst'))
        assert sorted(os.listdir(os.path.join(td, 'dst'))) == ['Task2_plane.txt', 'Task2_small-vehicle.txt']
        for fn in os.listdir(os.path.join(td, 'dst')):
            out['obb2hbb_' + fn] = np.array(open(os.path.join(td, 'dst', fn)).read())

    # ------------------------------------------------------------------ chain: merge -> OBB2HBB -> Task-2 voc_eval
    lines = DC.chain_tile_lines()
    with tempfile.TemporaryDirectory() as td:
        for d in ('src', 'merged', 'labelTxt'):
            os.makedirs(os.path.join(td, d))
        with open(os.path.join(td, 'src', 'Task1_plane.txt'), 'w') as f:
            f.write('\n'.join(lines) + '\n')
        RM.mergebase(os.path.join(td, 'src'), os.path.join(td, 'merged'), RM.py_cpu_nms_poly_fast)
        merged = open(os.path.join(td, 'merged', 'Task1_plane.txt')).read().splitlines()
        OH.OBB2HBB(os.path.join(td, 'merged'), os.path.join(td, 'hbb'))
        rng = np.random.RandomState(5)
        gt = {}
        for i, line in enumerate(merged):                            # ground truth: every other merged box, jittered, Task-2 layout
            tok = line.split(' ')
            gt.setdefault(tok[0], [])
            if i % 2 == 0:
                x1, y1, x2, y2 = DC._hull([float(v) for v in tok[2:]])
                j = np.round(rng.randn(4) * 3, 1)
                gt[tok[0]].append(DC.task2_quad(float(x1 + j[0]), float(y1 + j[1]), float(x2 + j[2]), float(y2 + j[3])) + f" plane {int(i % 5 == 0)}")
        for image, rows in gt.items():
            with open(os.path.join(td, 'labelTxt', image + '.txt'), 'w') as f:
                f.write('\n'.join(rows) + '\n')
        with open(os.path.join(td, 'imgnamefile.txt'), 'w') as f:
            f.write('\n'.join(gt) + '\n')
        args = (os.path.join(td, 'hbb', 'Task2_{:s}.txt'), os.path.join(td, 'labelTxt', '{:s}.txt'), os.path.join(td, 'imgnamefile.txt'), 'plane')
        rec, prec, ap1 = quiet(T2.voc_eval, *args, ovthresh=0.5, use_07_metric=True)
        _, _, ap0 = quiet(T2.voc_eval, *args, ovthresh=0.5, use_07_metric=False)
        out['chain_gt_images'] = np.array(list(gt))
        out['chain_gt_text'] = np.array(['\n'.join(rows) for rows in gt.values()])
        out['chain_hbb_text'] = np.array(open(os.path.join(td, 'hbb', 'Task2_plane.txt')).read())
        out['chain_rec'], out['chain_prec'], out['chain_ap'] = rec, prec, np.array([ap1, ap0])
        print(f"chain: {len(lines)} tile lines -> {len(merged)} merged, ap07 {ap1:.4f} ap {ap0:.4f}")

    path = os.path.join(HERE, 'devkit_eval_cases.npz')
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB, {len(out)} arrays)")


if __name__ == '__main__':
    main()
