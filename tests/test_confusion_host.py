"""CPU: the PRODUCT's ConfusionMatrix rules (yolov5_obb_amd/csrc/confusion_math.h: the IoU, the strict compares, the tie
compare and the winner key) compiled with g++ behind a serial driver (tests/native/host_confusion.cpp) and compared, integer for
integer, with every golden case (tests/golden/confusion_cases.npz: the reference's own ConfusionMatrix.process_batch with every
argsort stable).  The boxes come from the restated chain of oracle/pyref.py; the random cases are chosen so that no decision
hinges on the last bits of a box (gen_confusion_cases.py, conditions (a) (b)), the exact cases have no rounding at all.

Also: a flipped tie rule, or one keyed on the lower index, passes every random case and fails the permuted tie cases (so the
tie cases mean something); the three C-ABI entries answer argument errors before any device call; the Python object refuses
CPU tensors."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import confusion_cases as CC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_host_confusion(out):
    """tests/native/host_confusion.cpp -> the shared library `out`, loaded with hc_confusion's signature set."""
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", f"-I{ROOT}/yolov5_obb_amd/csrc",
                    f"{ROOT}/tests/native/host_confusion.cpp", "-o", str(out), "-lm"], check=True)
    L = C.CDLL(str(out))
    f32 = np.ctypeslib.ndpointer(dtype=np.float32, flags="C_CONTIGUOUS")
    i64 = np.ctypeslib.ndpointer(dtype=np.int64, flags="C_CONTIGUOUS")
    L.hc_confusion.argtypes = [f32, C.c_long, f32, C.c_long, C.c_int, C.c_float, C.c_float, i64, C.c_int]
    L.hc_confusion.restype = C.c_int
    return L


@pytest.fixture(scope="module")
def hc(tmp_path_factory):
    return build_host_confusion(tmp_path_factory.mktemp("hc") / "libhostconfusion.so")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "confusion_cases.npz"))


def host_matrices(L, case, flip=0):
    """Per-image (bs, nc + 1, nc + 1) matrices of a case and the out-of-range count."""
    nc = case["nc"]
    out = np.zeros((len(case["preds"]), nc + 1, nc + 1), dtype=np.int64)
    oor = 0
    for b in range(len(case["preds"])):
        if not CC.takes_part(case, b):
            continue
        det, lab = CC.host_boxes(case, b)
        mat = np.zeros((nc + 1) ** 2 + 1, dtype=np.int64)
        rc = L.hc_confusion(np.ascontiguousarray(det.numpy()), det.shape[0], np.ascontiguousarray(lab.numpy()), lab.shape[0], nc,
                            case["conf"], case["iou_thres"], mat, flip)
        assert rc == 0
        out[b] = mat[:-1].reshape(nc + 1, nc + 1)
        oor += int(mat[-1])
    return out, oor


def test_every_case_has_a_golden_matrix_per_image(golden):
    assert sorted(golden.files) == sorted(CC.NAMES)
    for name in CC.NAMES:
        case = CC.build(name)
        assert golden[name].shape == (len(case["preds"]), case["nc"] + 1, case["nc"] + 1), name


@pytest.mark.parametrize("name", CC.NAMES)
def test_host_rules_match_the_reference(hc, golden, name):
    got, oor = host_matrices(hc, CC.build(name))
    assert oor == 0 and np.array_equal(got, golden[name]), (name, int(np.abs(got - golden[name]).sum()))


def test_the_pinned_cells_of_the_small_tie_cases(golden):
    """The cells the two rules of csrc/confusion_math.h give, written out: the golden file must hold exactly these."""
    nc = 3
    want = {
        "tie_two_labels_other_class": {(0, 2): 1, (nc, 0): 1},              # the HIGHER label index takes the detection
        "tie_two_labels_other_class_perm": {(0, 0): 1, (nc, 2): 1},
        "tie_two_dets": {(1, 0): 1, (0, nc): 1},                            # the HIGHER detection index wins; the loser: background column
        "tie_two_dets_perm": {(0, 0): 1, (1, nc): 1},
        "tie_3x3": {(2, 2): 1, (nc, 0): 1, (nc, 1): 1, (0, nc): 1, (1, nc): 1},
        "tie_3x3_perm": {(1, 0): 1, (nc, 1): 1, (nc, 2): 1, (2, nc): 1, (0, nc): 1},
        "thr_equal": {(nc, 1): 1},                                          # no match: the detection is NOT counted
        "thr_one_ulp_above": {(1, 1): 1},
        "thr_rounded_to_f32": {(nc, 1): 1},
        "conf_equal": {(nc, 1): 1, (2, 2): 1},
    }
    for name, cells in want.items():
        m = np.zeros((nc + 1, nc + 1), dtype=np.int64)
        for rc, v in cells.items():
            m[rc] = v
        assert np.array_equal(golden[name].sum(0), m), name


@pytest.mark.parametrize("flip", [1, 2])
def test_a_flipped_tie_rule_fails_tie_cases_and_passes_the_random_ones(hc, golden, flip):
    """flip 1: the LOWER label index on ties; flip 2: the LOWER detection index (the rule of val.process_batch)."""
    failed = [n for n in CC.TIE_NAMES if not np.array_equal(host_matrices(hc, CC.build(n), flip)[0], golden[n])]
    small = ("tie_two_labels_other_class", "tie_two_labels_other_class_perm") if flip == 1 else ("tie_two_dets", "tie_two_dets_perm")
    assert set(small) <= set(failed) and "tie_grid" in failed and "tie_3x3" in failed and "tie_3x3_perm" in failed, failed
    for name in ("bs2", "nc16", "det_257", "lab_513"):
        assert np.array_equal(host_matrices(hc, CC.build(name), flip)[0], golden[name]), name


def test_out_of_range_classes_touch_no_cell(hc):
    det = np.array([[0, 0, 10, 10, .9, 3], [50, 50, 60, 60, .9, 1], [80, 80, 90, 90, .9, -1]], dtype=np.float32)
    lab = np.array([[-1, 0, 0, 10, 10], [1, 50, 50, 60, 60], [3, 200, 200, 210, 210]], dtype=np.float32)
    mat = np.zeros(17, dtype=np.int64)
    hc.hc_confusion(det, 3, lab, 3, 3, 0.25, 0.45, mat, 0)
    want = np.zeros(17, dtype=np.int64)
    want[1 * 4 + 1] = 1                      # the pair in range
    want[16] = 3                             # (det class 3, label class -1), the unmatched label of class 3, the unmatched detection of class -1
    assert np.array_equal(mat, want)


def test_argument_checks_answer_before_any_device_call():
    """OBB_ERR_BAD_ARG = -1, OBB_ERR_WORKSPACE = -2, nothing is launched: callable without a GPU."""
    from yolov5_obb_amd import _lib
    L = _lib.lib()
    null, p = C.c_void_p(0), C.c_void_p(4096)                    # (p: a non-null pointer that no check dereferences)
    off = (C.c_int64 * 3)(0, 4, 9)
    offv = C.cast(off, C.c_void_p)
    img = (C.c_float * 10)(0, 0, 1, 640, 640, 0, 0, 1, 640, 640)
    imgv = C.cast(img, C.c_void_p)
    need = L.obb_confusion_workspace_bytes(9, 5)
    assert need >= 9 * 28 + 5 * 28 and L.obb_confusion_workspace_bytes(0, 0) > 0

    def batch(det=p, doff=offv, bs=2, tg=p, nt=5, tcols=7, im=imgv, nc=16, mat=p, ws=p, wsb=need):
        return L.obb_confusion_batch_f32(det, doff, bs, tg, nt, tcols, im, nc, 0.25, 0.45, mat, ws, wsb, null)
    for kw in (dict(bs=0), dict(bs=65), dict(nc=0), dict(nt=-1), dict(doff=null), dict(im=null), dict(mat=null), dict(det=null),
               dict(tg=null), dict(tcols=6)):
        assert batch(**kw) == -1, kw
    assert batch(ws=null) == -2 and batch(wsb=need - 1) == -2
    assert batch(nt=0, tg=null, ws=null, wsb=0) == 0             # no labels: OBB_OK, no launch
    zero = (C.c_int64 * 3)(0, 0, 0)
    assert batch(doff=C.cast(zero, C.c_void_p), det=null, ws=null, wsb=0) == 0      # no detections: OBB_OK, no launch
    bad = (C.c_int64 * 3)(0, 5, 4)
    assert batch(doff=C.cast(bad, C.c_void_p)) == -1             # offsets that decrease
    img[2] = 0.0
    assert batch() == -1                                         # a gain of 0
    img[2] = 1.0

    def one(det=p, n=9, lab=p, m=5, nc=16, mat=p, ws=p, wsb=need):
        return L.obb_confusion_process_batch_f32(det, n, lab, m, nc, 0.25, 0.45, mat, ws, wsb, null)
    for kw in (dict(n=-1), dict(m=-1), dict(nc=0), dict(mat=null), dict(det=null), dict(lab=null)):
        assert one(**kw) == -1, kw
    assert one(ws=null) == -2 and one(wsb=need - 1) == -2
    assert one(n=0, det=null, ws=null, wsb=0) == 0 and one(m=0, lab=null, ws=null, wsb=0) == 0


def test_confusion_matrix_refuses_cpu_tensors():
    from yolov5_obb_amd.utils.metrics import ConfusionMatrix
    with pytest.raises(RuntimeError):
        ConfusionMatrix(3, device="cpu")
    cm = ConfusionMatrix(3)                                      # (no device is touched before the first batch)
    with pytest.raises(RuntimeError):
        cm.process_batch(torch.zeros(2, 6), torch.zeros(1, 5))
    with pytest.raises(RuntimeError):
        cm.add_batch([torch.zeros(2, 7)], torch.zeros(1, 9), [CC.UNIT])
    with pytest.raises(NotImplementedError):
        cm.plot()
    assert np.array_equal(cm.matrix, np.zeros((4, 4))) and cm.matrix.dtype == np.float64
    tp, fp = cm.tp_fp()
    assert tp.shape == (3,) and fp.shape == (3,)
