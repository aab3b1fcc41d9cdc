"""CPU: the host parts of the Task-2 / mAOE chain against values frozen from the reference's own DOTA_devkit files
(tests/golden/gen_devkit_eval_cases.py -> tests/golden/devkit_eval_cases.npz): dota_poly2rbox (scalar and array forms),
results_obb2hbb.OBB2HBB (bytes), Task-2 parse_gt / truncation / voc_ap, and the argument refusals of
obb_eval_best_gt_hbb_f64, which answer before any device call."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import devkit_eval_cases as DC
from tests.golden.gen_golden import EVAL_CLASSES

G = DC.golden()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _same(got, want, what):
    """Same dtype, same bits (NaN == NaN)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    assert np.array_equal(got, want, equal_nan=True), (what, np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))[:5])


# ---- dota_poly2rbox: the frozen values come from the same numpy and the same formula: exact ------------------------------
def test_poly2rbox_scalar_forms_equal_the_reference():
    from yolov5_obb_amd.DOTA_devkit import dota_poly2rbox as P
    quads = DC.rbox_quads()
    assert 190 <= len(quads) <= 230
    with np.errstate(all='ignore'):
        v1 = [P.poly2rbox_single(q) for q in quads]
        v2 = [P.poly2rbox_single_v2(q) for q in quads]
        v3 = [P.poly2rbox_single_v3(q) for q in quads]
        back = [P.rbox2poly_single(r) for r in v1]
    begin = [P.get_best_begin_point_single(q) for q in quads]
    assert all(isinstance(r, np.ndarray) and r.dtype == np.float64 and r.shape == (5,) for r in v1)
    assert all(isinstance(r, tuple) and len(r) == 5 and all(type(x) is float for x in r) for r in v2 + v3)
    _same(np.array(v1), G['rbox_v1'], 'poly2rbox_single')
    _same(np.array(v2), G['rbox_v2'], 'poly2rbox_single_v2')
    _same(np.array(v3), G['rbox_v3'], 'poly2rbox_single_v3')
    _same(np.array(back), G['rbox_back'], 'rbox2poly_single')
    _same(np.array(begin), G['rbox_begin'], 'get_best_begin_point_single')
    # the fixtures reach what they are for: both ratio branches, the exact lower wrap boundary, a NaN ratio
    assert np.isclose(G['rbox_v3'][:, 4], 3 * np.pi / 4).sum() + np.isclose(G['rbox_v3'][:, 4], -np.pi / 4).sum() >= 4
    assert (G['rbox_v2'][:, 4] != G['rbox_v3'][:, 4]).sum() >= 5 and (G['rbox_v1'][:, 4] != G['rbox_v2'][:, 4]).sum() >= 1


def test_poly2rbox_array_forms_equal_the_scalar_ones_bit_for_bit():
    from yolov5_obb_amd.DOTA_devkit import dota_poly2rbox as P
    quads = DC.rbox_quads()
    for fn, key in ((P.poly2rbox, 'rbox_v1'), (P.poly2rbox_v2, 'rbox_v2'), (P.poly2rbox_v3, 'rbox_v3')):
        got = fn(quads)
        assert got.dtype == np.float64 and got.shape == (len(quads), 5)
        ok = (_bits(got) == _bits(G[key])) | (np.isnan(got) & np.isnan(G[key]))
        assert ok.all(), (key, np.argwhere(~ok)[:5])
    wide = np.concatenate([quads, np.full((len(quads), 2), 9.0)], 1)          # rows with more columns: poly[:8]
    assert np.array_equal(P.poly2rbox_v3(wide), P.poly2rbox_v3(quads), equal_nan=True)
    assert P.poly2rbox_v3(np.zeros((0, 8))).shape == (0, 5)
    assert P.norm_angle(-np.pi / 4) == -np.pi / 4 and P.norm_angle(np.pi) == 0.0
    assert P.cal_line_length((0, 0), (3, 4)) == 5.0


# ---- results_obb2hbb ------------------------------------------------------------------------------------------------------
def test_obb2hbb_writes_the_reference_bytes(tmp_path):
    from yolov5_obb_amd.DOTA_devkit import results_obb2hbb as OH
    src, dst = tmp_path / "src" / "deep", tmp_path / "dst"
    os.makedirs(src)
    for fn, text in DC.OBB2HBB_FILES.items():
        (src / fn).write_text(text)
    os.makedirs(dst)
    (dst / "stale.txt").write_text("gone")                                    # dstpath is removed and recreated
    OH.OBB2HBB(str(tmp_path / "src"), str(dst))
    assert sorted(os.listdir(dst)) == ['Task2_plane.txt', 'Task2_small-vehicle.txt']
    for fn in os.listdir(dst):
        got = (dst / fn).read_bytes()
        assert got == str(G['obb2hbb_' + fn]).encode(), fn
        assert not got.endswith(b'\n')
    plane = (dst / 'Task2_plane.txt').read_text().split('\n')
    assert plane[0].split(' ')[1] == '0.50' and plane[2].split(' ')[1] == '1e-05'      # the score token is copied
    assert OH.custombasename('/a/b/Task1_plane.txt') == 'Task1_plane'
    assert sorted(os.path.basename(f) for f in OH.GetFileFromThisRootDir(str(tmp_path / "src"), ext=['txt'])) == sorted(DC.OBB2HBB_FILES)
    assert OH.GetFileFromThisRootDir(str(tmp_path / "src"), ext=['xml']) == []


# ---- Task 2: parse_gt, truncation, voc_ap ---------------------------------------------------------------------------------
def test_task2_parse_gt_truncates_toward_zero(tmp_path):
    from yolov5_obb_amd.DOTA_devkit import dota_evaluation_task2 as T2
    gt, det = DC.task2_inputs('a', int(G['task2_a_redraw']))
    _, annopath, _ = DC.task2_write(str(tmp_path / "set"), gt, det)
    objs = T2.parse_gt(annopath.format('H0000'))
    assert [o['bbox'] for o in objs] == G['task2_parse_gt_bbox'].tolist()
    assert [o['difficult'] for o in objs] == G['task2_parse_gt_difficult'].tolist()
    assert [o['area'] for o in objs] == G['task2_parse_gt_area'].tolist()
    assert [o['name'] for o in objs] == G['task2_parse_gt_name'].tolist()
    assert all(type(v) is int for o in objs for v in o['bbox'])
    assert objs[0]['bbox'] == [-3, -2, 10, 8] and objs[1]['bbox'] == [0, 0, 0, 12]      # not floor
    assert objs[4]['bbox'][2] == objs[4]['bbox'][0] - 1                                  # the zero-area box of the NaN pair


def test_task2_load_gt_is_parse_gt_as_arrays(tmp_path):
    """The array reader (np.trunc of the exact doubles) gives what parse_gt's records give, per class; a non-finite coordinate
    goes through parse_gt and raises like int() in the reference."""
    from yolov5_obb_amd.DOTA_devkit import dota_evaluation_task2 as T2
    gt, det = DC.task2_inputs('c', int(G['task2_c_redraw']))
    _, annopath, imagesetfile = DC.task2_write(str(tmp_path / "set"), gt, det)
    images = list(gt)
    for cls in EVAL_CLASSES:
        boxes, difficult, off = T2.load_gt(annopath, images, cls)
        want = [[o for o in T2.parse_gt(annopath.format(im)) if o['name'] == cls] for im in images]
        assert boxes.dtype == np.float64 and boxes.shape == (sum(len(w) for w in want), 4)
        assert not np.signbit(boxes[boxes == 0]).any()
        assert off.tolist() == np.concatenate([[0], np.cumsum([len(w) for w in want])]).tolist()
        assert boxes.tolist() == [[float(v) for v in o['bbox']] for w in want for o in w]
        assert difficult.tolist() == [bool(o['difficult']) for w in want for o in w]
    assert T2.load_gt(annopath, ['H0001'], 'plane')[0].shape == (0, 4)
    for bad, err in (("nan", ValueError), ("inf", OverflowError), ("1e999", OverflowError)):
        with open(annopath.format('H0001'), 'w') as f:
            f.write(f"1.0 2.0 3.0 2.0 {bad} 9.0 1.0 9.0 plane 0\n")
        with pytest.raises(err):
            T2.load_gt(annopath, ['H0001'], 'plane')


def test_task2_read_detections_takes_four_or_more_columns(tmp_path):
    from yolov5_obb_amd.DOTA_devkit import dota_evaluation_task2 as T2
    p = tmp_path / "Task2_x.txt"
    p.write_text("P1 0.50 1.5 2.0 3.0 4.25\nP2 0.1 -1.0 0.0 1e2 7\n")
    ids, conf, bb = T2.read_detections(str(p))
    assert list(ids) == ['P1', 'P2'] and conf.tolist() == [0.5, 0.1] and bb.tolist() == [[1.5, 2.0, 3.0, 4.25], [-1.0, 0.0, 100.0, 7.0]]
    p.write_text("P1 0.50 1 2 3 4 5 6 7 8\n")                                  # a Task-1 row: BB[d, :4] is what the overlap reads
    assert T2.read_detections(str(p))[2].shape == (1, 8)
    p.write_text("P1 0.5 1 2 nan 4\n")                                        # not plain: line by line, float('nan')
    assert np.isnan(T2.read_detections(str(p))[2][0, 2])


def test_task2_voc_ap_equals_the_reference():
    from yolov5_obb_amd.DOTA_devkit import dota_evaluation_task2 as T2
    for k in range(3):
        rec, prec = G[f'vocap_{k}_rec'], G[f'vocap_{k}_prec']
        assert [T2.voc_ap(rec, prec, True), T2.voc_ap(rec, prec, False)] == G[f'vocap_{k}_ap'].tolist()


def test_task2_refuses_to_run_without_a_device(monkeypatch):
    import torch
    from yolov5_obb_amd.DOTA_devkit import dota_evaluation_task2 as T2
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="HIP device"):
        T2.best_gt(np.zeros((1, 4)), np.zeros(1, np.int32), np.zeros((1, 4)), np.array([0, 1]))


# ---- the C entry's argument checks ----------------------------------------------------------------------------------------
def test_best_gt_hbb_argument_checks_answer_before_any_device_call():
    """OBB_ERR_BAD_ARG = -1 for det_stride < 4, a negative count and a NULL required pointer with nd > 0; nd == 0 is OBB_OK with
    nothing launched: callable without a GPU."""
    from yolov5_obb_amd import _lib
    L = _lib.lib()
    null = C.c_void_p(0)
    buf = (C.c_double * 8)()
    p = C.cast(buf, C.c_void_p)
    assert L.obb_eval_best_gt_hbb_f64(p, 3, p, 1, p, p, 1, p, p, null) == -1            # det_stride < 4
    assert L.obb_eval_best_gt_hbb_f64(p, 4, p, -1, p, p, 1, p, p, null) == -1           # negative nd
    assert L.obb_eval_best_gt_hbb_f64(p, 4, p, 1, p, p, -1, p, p, null) == -1           # negative n_img
    for k in (0, 2, 5, 7, 8):                                                           # dets4, det_img, gt_off, ovmax, jmax
        args = [p, 4, p, 1, p, p, 1, p, p, null]
        args[k] = null
        assert L.obb_eval_best_gt_hbb_f64(*args) == -1, k
    assert L.obb_eval_best_gt_hbb_f64(null, 4, null, 0, null, null, 0, null, null, null) == 0
    assert L.obb_eval_best_gt_hbb_f64(null, 3, null, 0, null, null, 0, null, null, null) == -1
