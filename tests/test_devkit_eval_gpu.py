"""GPU parity of the Task-2 / mAOE chain against values frozen from the reference's own DOTA_devkit files
(tests/golden/gen_devkit_eval_cases.py -> tests/golden/devkit_eval_cases.npz).

A. Task-2 voc_eval / evaluate (dota_evaluation_task2.py over obb_eval_best_gt_hbb_f64): rec, prec and both APs, exact.
B. obb_eval_best_gt_hbb_f64 per detection against a numpy restatement of the reference's :183-202: list lengths 0, 1, 63, 64, 65
   (the lane-serial path of k_eval_best_gt_hbb ends at 64 boxes), 130 and 900 (the wave-cooperative path, ragged last round),
   ties, the NaN pair, non-finite detections, row strides 4 / 5 / 10, more than one pass of the capped grid, a side stream.
   ovmax is compared by its bits; a NaN by being NaN (numpy's 0 / 0 and the device's differ in the sign bit of the NaN, which
   neither IEEE 754 nor numpy defines).
C. mAOE aoe_eval / evaluate: the contributing detections and their order, every angle error within 1e-9 degrees of the frozen
   value and bit-identical to the formula evaluated here.
D. The chain ResultMerge.mergebypoly -> OBB2HBB -> Task-2 voc_eval.
"""
import os

import numpy as np
import pytest
import torch

from tests import devkit_eval_cases as DC
from tests.golden.gen_golden import EVAL_CASES, EVAL_CLASSES, eval_inputs, eval_write

pytestmark = pytest.mark.gpu

G = DC.golden()


# ---- A. Task-2 voc_eval ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(EVAL_CASES))
def test_task2_voc_eval_equals_the_reference_devkit(dev, tmp_path, name):
    from yolov5_obb_amd.DOTA_devkit import dota_evaluation_task2 as T2
    gt, det = DC.task2_inputs(name, int(G[f"task2_{name}_redraw"]))
    detpath, annopath, imagesetfile = DC.task2_write(str(tmp_path / "set"), gt, det)
    aps = []
    for cls in EVAL_CLASSES:
        for m07 in (True, False):
            rec, prec, ap = T2.voc_eval(detpath, annopath, imagesetfile, cls, ovthresh=0.5, use_07_metric=m07)
            assert ap == float(G[f"task2_{name}_{cls}_ap{int(m07)}"]), (cls, m07)
            assert np.array_equal(rec, G[f"task2_{name}_{cls}_rec"]) and np.array_equal(prec, G[f"task2_{name}_{cls}_prec"]), (cls, m07)
        aps.append(float(G[f"task2_{name}_{cls}_ap1"]))
    mean_ap, classaps = T2.evaluate(detpath, annopath, imagesetfile, list(EVAL_CLASSES))
    assert mean_ap == (0 + aps[0] + aps[1]) / 2 and np.array_equal(classaps, 100 * np.array(aps))
    with pytest.raises(FileNotFoundError):                                    # main() skips nothing
        T2.evaluate(detpath, annopath, imagesetfile, list(EVAL_CLASSES) + ['harbor'])


# ---- B. the kernel per detection ------------------------------------------------------------------------------------------
def np_best_gt_hbb(bb, BBGT):
    """dota_evaluation_task2.py:180-202 for one detection: (ovmax, jmax); (-inf, -1) for an image without boxes."""
    ovmax, jmax = -np.inf, -1
    if BBGT.size > 0:
        ixmin = np.maximum(BBGT[:, 0], bb[0])
        iymin = np.maximum(BBGT[:, 1], bb[1])
        ixmax = np.minimum(BBGT[:, 2], bb[2])
        iymax = np.minimum(BBGT[:, 3], bb[3])
        iw = np.maximum(ixmax - ixmin + 1., 0.)
        ih = np.maximum(iymax - iymin + 1., 0.)
        inters = iw * ih
        uni = ((bb[2] - bb[0] + 1.) * (bb[3] - bb[1] + 1.) + (BBGT[:, 2] - BBGT[:, 0] + 1.) * (BBGT[:, 3] - BBGT[:, 1] + 1.) - inters)
        overlaps = inters / uni
        ovmax = np.max(overlaps)
        jmax = int(np.argmax(overlaps))
    return ovmax, jmax


LIST_LENGTHS = [0, 1, 63, 64, 65, 130, 900, 0, 200]
_BASE = []


def hbb_base():
    """(dets (n, 4), det_img, gts (m, 4), gt_off, want_ov, want_j): truncated boxes in images of LIST_LENGTHS boxes, detections
    shuffled, with the numpy restatement's answers.  Computed once, never modified."""
    if _BASE:
        return _BASE[0]
    rng = np.random.RandomState(9)

    def boxes(n, extent):
        x, y = rng.rand(n) * extent - 20, rng.rand(n) * extent - 20
        return np.stack([x, y, x + rng.rand(n) * 60 + 1, y + rng.rand(n) * 40 + 1], 1)
    gts, off, dets, dimg = [], [0], [], []
    for im, ng in enumerate(LIST_LENGTHS):
        extent = 30 * np.sqrt(ng) + 60
        g = np.trunc(boxes(ng, extent)) + 0.0
        nd = 30 + ng // 4
        d = boxes(nd, extent)
        if ng > 10:
            g[5] = g[2]                                                   # a duplicated box: the first index wins
            g[ng - 1] = g[ng - 2]                                         # ... also at the end of the list (the ragged last round)
            g[7] = [50., 60., 49., 70.]                                   # zero area: with the detection below 0 / 0
            src = rng.randint(0, ng, nd // 2)
            d[:nd // 2] = g[src] + np.round(rng.randn(nd // 2, 4) * 2, 1)
            d[0] = g[2]; d[1] = g[ng - 1]; d[2] = [50., 60., 49., 70.]
            d[3] = [np.nan, 0., 10., 10.]                                 # every overlap NaN: the first index
            d[4] = [-np.inf, -np.inf, np.inf, np.inf]                     # inf / inf
            d[5] = [1e6, 1e6, 1e6 + 5, 1e6 + 5]                           # far from everything: overlap 0 with all, index 0
            d[6] = [0., 0., np.inf, 10.]
        gts.append(g); off.append(off[-1] + ng)
        dets.append(d); dimg += [im] * nd
    gts, dets, dimg = np.concatenate(gts), np.concatenate(dets), np.array(dimg, dtype=np.int32)
    perm = rng.permutation(len(dets))
    dets, dimg, off = np.ascontiguousarray(dets[perm]), dimg[perm], np.array(off)
    with np.errstate(all='ignore'):
        want = [np_best_gt_hbb(dets[d], gts[off[dimg[d]]:off[dimg[d] + 1]]) for d in range(len(dets))]
    ov, jm = np.array([w[0] for w in want]), np.array([w[1] for w in want], dtype=np.int32)
    assert np.isnan(ov).sum() >= 10 and (ov == -np.inf).sum() == 60 and (jm[np.isnan(ov)] > 0).any() and (jm[np.isnan(ov)] == 0).any()
    assert (ov == 1.0).sum() >= 10 and (ov > 0.5).sum() > 100
    _BASE.append((dets, dimg, gts, off, ov, jm))
    return _BASE[0]


def _assert_same(ov, jm, want_ov, want_j):
    nan = np.isnan(want_ov)
    assert np.array_equal(np.isnan(ov), nan), "NaN positions"
    assert np.array_equal(ov[~nan].view(np.uint64), want_ov[~nan].view(np.uint64)), np.argwhere(ov[~nan] != want_ov[~nan])[:5]
    assert np.array_equal(jm, want_j), np.argwhere(jm != want_j)[:5]


@pytest.mark.parametrize("stride", [4, 5, 10])
def test_best_gt_hbb_equals_numpy_per_detection(dev, stride):
    """Row strides 4 (a Task-2 file), 10 (a Task-1 style row, read as double2) and 5 (rows that are not 16-byte aligned)."""
    from yolov5_obb_amd.DOTA_devkit.dota_evaluation_task2 import best_gt
    dets, dimg, gts, off, want_ov, want_j = hbb_base()
    wide = np.full((len(dets), stride), 12345.0)
    wide[:, :4] = dets
    ov, jm = best_gt(wide, dimg, gts, off)
    assert ov.dtype == np.float64 and jm.dtype == np.int32 and ov.shape == jm.shape == (len(dets),)
    _assert_same(ov, jm, want_ov, want_j)


def test_best_gt_hbb_on_views_and_empty_inputs(dev):
    """An unaligned ground-truth pointer (a view 8 bytes into a buffer) takes the scalar loads; no detections: no launch; no
    ground truth at all: -inf, -1 everywhere; an image index outside the table counts as an image without boxes."""
    from yolov5_obb_amd import _lib
    from yolov5_obb_amd.DOTA_devkit.dota_evaluation_task2 import best_gt
    dets, dimg, gts, off, want_ov, want_j = hbb_base()
    nd = len(dets)
    d_det, d_img, d_off = torch.from_numpy(dets).to(dev), torch.from_numpy(dimg).to(dev), torch.from_numpy(off.astype(np.int32)).to(dev)
    buf = torch.zeros(gts.size + 1, dtype=torch.float64, device=dev)
    buf[1:] = torch.from_numpy(gts).to(dev).reshape(-1)
    assert buf[1:].data_ptr() % 16 == 8
    ov, jm = torch.full((nd,), 7.0, dtype=torch.float64, device=dev), torch.full((nd,), 7, dtype=torch.int32, device=dev)
    rc = _lib.lib().obb_eval_best_gt_hbb_f64(_lib.ptr(d_det), 4, _lib.ptr(d_img), nd, _lib.ptr(buf[1:]), _lib.ptr(d_off), len(off) - 1,
                                             _lib.ptr(ov), _lib.ptr(jm), _lib.stream_ptr(dev))
    assert rc == 0
    _assert_same(ov.cpu().numpy(), jm.cpu().numpy(), want_ov, want_j)
    ov0, jm0 = best_gt(np.zeros((0, 4)), np.zeros(0, np.int32), gts, off)
    assert ov0.shape == (0,) and jm0.shape == (0,)
    ov1, jm1 = best_gt(dets[:70], dimg[:70], np.zeros((0, 4)), np.zeros(len(off), dtype=np.int64))
    assert (ov1 == -np.inf).all() and (jm1 == -1).all()
    out_of_table = np.where(np.arange(70) % 2 == 0, np.int32(len(off) - 1), np.int32(-1)).astype(np.int32)
    ov2, jm2 = best_gt(dets[:70], out_of_table, gts, off)
    assert (ov2 == -np.inf).all() and (jm2 == -1).all()


def test_best_gt_hbb_beyond_one_grid_pass(dev):
    """k_eval_best_gt_hbb runs at most 4096 one-wave workgroups = 262144 detections per pass of its grid-stride loop: two full
    passes and a third whose only workgroup has three live lanes.  The base detections cycled in shuffled order: every copy
    gets the answer of its base detection."""
    from yolov5_obb_amd.DOTA_devkit.dota_evaluation_task2 import best_gt
    dets, dimg, gts, off, want_ov, want_j = hbb_base()
    nd = 2 * 4096 * 64 + 3
    src = np.random.RandomState(1).permutation(np.arange(nd) % len(dets))
    ov, jm = best_gt(dets[src], dimg[src], gts, off)
    assert ov.shape == (nd,)
    _assert_same(ov, jm, want_ov[src], want_j[src])


def test_best_gt_hbb_on_a_side_stream(dev):
    from yolov5_obb_amd.DOTA_devkit.dota_evaluation_task2 import best_gt
    dets, dimg, gts, off, want_ov, want_j = hbb_base()
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        ov, jm = best_gt(dets, dimg, gts, off)
    side.synchronize()
    _assert_same(ov, jm, want_ov, want_j)


# ---- C. mAOE --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(EVAL_CASES))
def test_aoe_eval_equals_the_reference_devkit(dev, tmp_path, name):
    """Tolerance 1e-9 degrees: both sides are double; the only freedom between machines is libm's arctan2, about 1 ulp of pi
    (4.4e-16 rad) per angle; two angles and fewer than 10 roundings, times 57.32, stay below 1e-12; the factor 1e3 left is
    margin, and 1e6 below the smallest non-zero difference of the fixtures."""
    from yolov5_obb_amd.DOTA_devkit import mAOE_evaluation as MA
    from yolov5_obb_amd.DOTA_devkit.dota_poly2rbox import poly2rbox_single_v3
    gt, det = eval_inputs(*EVAL_CASES[name])
    detpath, annopath, imagesetfile = eval_write(str(tmp_path / "set"), gt, det)
    for thr in DC.AOE_THRESHOLDS:
        means = []
        for cls in EVAL_CLASSES:
            key = f"aoe_{name}_{cls}_{thr}"
            got = MA.aoe_eval(detpath, annopath, imagesetfile, cls, ovthresh=thr)
            want, hits = G[key + "_dif"], G[key + "_hits"]
            assert isinstance(got, list) and all(type(x) is float for x in got)
            # the contributing detections and their order: the errors computed here for the frozen (detection, ground truth) pairs
            conf = np.array([float(x.split(' ')[1]) for x in det[cls]])
            BB = np.array([[float(v) for v in x.split(' ')[2:]] for x in det[cls]])[np.argsort(-conf)]
            mine = [abs(poly2rbox_single_v3(BB[h])[-1] - poly2rbox_single_v3(g)[-1]) * 57.32 for h, g in zip(hits, G[key + "_gt"])]
            assert len(got) == len(want) == len(mine), (key, len(got), len(want))
            assert got == mine, (key, [i for i in range(len(got)) if got[i] != mine[i]][:5])          # bit for bit
            err = np.abs(np.array(got) - want)
            print(f" [{key}: {len(got)} hits, max |error| {err.max():.3e} deg]", end="")
            assert (err <= 1e-9).all(), (key, err.max())
            m = 0.0
            for x in got:
                m = m + x
            means.append(m / len(got))
        maoe, per_class = MA.evaluate(detpath, annopath, imagesetfile, list(EVAL_CLASSES), ovthresh=thr)
        assert per_class == means and maoe == (0.0 + means[0] + means[1]) / 2
    with pytest.raises(ZeroDivisionError):                                    # a class without a hit, as main()
        MA.evaluate(detpath, annopath, imagesetfile, list(EVAL_CLASSES), ovthresh=1.5)


# ---- D. the chain ---------------------------------------------------------------------------------------------------------
def test_chain_merge_obb2hbb_task2(dev, tmp_path):
    from yolov5_obb_amd.DOTA_devkit import ResultMerge_multi_process as RM
    from yolov5_obb_amd.DOTA_devkit import dota_evaluation_task2 as T2
    from yolov5_obb_amd.DOTA_devkit import results_obb2hbb as OH
    for d in ("src", "labelTxt"):
        os.makedirs(tmp_path / d)
    (tmp_path / "src" / "Task1_plane.txt").write_text('\n'.join(DC.chain_tile_lines()) + '\n')
    RM.mergebypoly(str(tmp_path / "src"), str(tmp_path / "merged"))
    OH.OBB2HBB(str(tmp_path / "merged"), str(tmp_path / "hbb"))
    assert (tmp_path / "hbb" / "Task2_plane.txt").read_text() == str(G["chain_hbb_text"])
    images = G["chain_gt_images"].tolist()
    for image, text in zip(images, G["chain_gt_text"].tolist()):
        (tmp_path / "labelTxt" / (image + ".txt")).write_text(text + '\n')
    (tmp_path / "imgnamefile.txt").write_text('\n'.join(images) + '\n')
    args = (str(tmp_path / "hbb" / "Task2_{:s}.txt"), str(tmp_path / "labelTxt" / "{:s}.txt"), str(tmp_path / "imgnamefile.txt"), "plane")
    rec, prec, ap1 = T2.voc_eval(*args, ovthresh=0.5, use_07_metric=True)
    _, _, ap0 = T2.voc_eval(*args, ovthresh=0.5, use_07_metric=False)
    assert np.array_equal(rec, G["chain_rec"]) and np.array_equal(prec, G["chain_prec"]) and [ap1, ap0] == G["chain_ap"].tolist()
    assert 0.1 < ap1 < 0.9
