"""GPU: the row reads of the filter kernel (csrc/nmsobb_front.h: k_decode, dec_load_quad) against oracle/pyref.py, bit for bit and in
the same order.  Every load of a row is unconditional -- a lane that wants nothing reads an element of its row and drops it -- so
the cases are the ones where "which element, of which row" can go wrong: a partial 16-row chunk, one row short of and one over a
chunk, a row count that is no multiple of a workgroup's rows, more than one workgroup; rows that start on odd element offsets
(no odd); the class group fetched on demand (nc = 33); the three dtypes, with and without the dense objectness column, multi-label
and best-class; a tensor whose first and last rows pass and that lies between poisoned elements; NaN and inf in the angle bins and
in a class score of a passing row."""
import pytest
import torch

from oracle import pyref
from tests import synth

pytestmark = pytest.mark.gpu

KW = dict(conf_thres=0.25, iou_thres=0.45, max_det=300)
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}


def _stage_counts(L):
    import ctypes as C
    ms = (C.c_double * 8)()
    cnt = (C.c_int64 * 8)()
    assert L.obb_profile_collect(C.cast(ms, C.c_void_p), C.cast(cnt, C.c_void_p), 8) == 0
    return list(cnt)


def _pred(A, nc, dtype, seed):
    # few objects and few rows on them: every image keeps far fewer than 384 candidates per class (the small-segment kernel's limit)
    return synth.s_pred(2, A, nc, seed=seed, n_obj=6, fg_frac=0.5 if A < 100 else 0.04, dtype=dtype)


def _cmp(got, ref, what):
    assert len(got) == len(ref), what
    for b, (g, r) in enumerate(zip(got, ref)):
        assert g.shape == r.shape and torch.equal(g.cpu(), r), (what, "image", b, tuple(g.shape), tuple(r.shape))


def _run(dev, pred_dev, ref_multi, ref_best, what, nc, expect_small=True, kw=KW):
    """Both label modes, with and without the objectness column; the third call of a shape runs on the hints of the second.
    kw: the thresholds and max_det the references were made with."""
    from yolov5_obb_amd import _lib
    from yolov5_obb_amd.utils import general
    L = _lib.lib()
    A = pred_dev.shape[1]
    for multi, ref in ((True, ref_multi), (False, ref_best)):
        for col in (False, True):
            p = pred_dev.clone() if col else pred_dev
            if col:
                p._obb_objcol = (p[..., 4].contiguous(), p._version)
            general.hints_clear()
            for rep in range(3):
                L.obb_profile_enable(1)
                try:
                    got = general.non_max_suppression_obb(p, multi_label=multi, **kw)
                finally:
                    cnt = _stage_counts(L)
                    L.obb_profile_enable(0)
                _cmp(got, ref, (what, "multi_label", multi, "objcol", col, "call", rep))
            if nc > 1 and expect_small:
                # the small-segment kernel (the shape's hint says which kernel the third call took); its segments sort themselves, with
                # no sort launch in front, when every class can have a full segment of the image's candidate slots (csrc/nms_plan.h)
                seg = general.hint_get(dev, A, nc, multi and nc > 1, kw["conf_thres"])["seg"]
                slots = -(-(A * (nc if multi else 1)) // 64) * 64
                assert 0 < seg <= general._SEG_SMALL and cnt[0] > 0, (what, multi, col, seg, cnt)
                assert (cnt[1] == 0) == (nc * general._SEG_SMALL <= slots), (what, multi, col, slots, cnt)
            elif nc == 1:
                assert cnt[0] > 0 and cnt[1] > 0, (what, multi, col, cnt)       # one class: no class segments, the sort runs


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("nc", [1, 16, 33])
@pytest.mark.parametrize("A", [15, 16, 17, 1000, 2049])
def test_rows_equal_the_oracle(dev, oracle_lib, A, nc, dt):
    pred = _pred(A, nc, DTYPES[dt], seed=7000 + A + nc)
    pred[:, -1, 4] = 0.9                                   # the last row of every image passes
    pred[:, -1, 5] = 0.8
    ref_multi = pyref.non_max_suppression_obb(pred.clone(), multi_label=True, **KW)
    ref_best = pyref.non_max_suppression_obb(pred.clone(), multi_label=False, **KW)
    assert sum(r.shape[0] for r in ref_multi) >= 2
    _run(dev, pred.to(dev), ref_multi, ref_best, (A, nc, dt), nc)


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("nc", [16, 33])
@pytest.mark.parametrize("lead", [64, 65])
def test_a_tensor_between_poisoned_elements(dev, oracle_lib, lead, nc, dt):
    """The tensor is an exact-size view inside a larger buffer of NaNs: `lead` elements in front (65: a base address that is only
    element-aligned), NaNs behind its last element.  The first and the last row pass.  A NaN read as an angle bin or a class score
    would win the arg-max or drop the row."""
    dtype = DTYPES[dt]
    A = 1000
    pred = _pred(A, nc, dtype, seed=7100 + nc)
    for b, r in ((0, 0), (-1, -1)):
        pred[b, r, 4] = 0.9
        pred[b, r, 5 + nc - 1] = 0.8                        # the last class, next to the first angle bin
        pred[b, r, 5 + nc:] = 0.1
        pred[b, r, -1] = 0.7                                # the arg-max is the row's LAST element
    ref_multi = pyref.non_max_suppression_obb(pred.clone(), multi_label=True, **KW)
    ref_best = pyref.non_max_suppression_obb(pred.clone(), multi_label=False, **KW)
    assert ref_multi[0].shape[0] > 0 and ref_multi[-1].shape[0] > 0
    n = pred.numel()
    buf = torch.full((lead + n + 4096,), float("nan"), dtype=dtype, device=dev)
    buf[lead:lead + n] = pred.reshape(-1).to(dev)
    view = buf[lead:lead + n].view(pred.shape)
    assert view.is_contiguous() and view.data_ptr() == buf.data_ptr() + lead * buf.element_size()
    _run(dev, view, ref_multi, ref_best, ("between NaNs", lead, nc, dt), nc)
    assert bool(torch.isnan(buf[:lead]).all()) and bool(torch.isnan(buf[lead + n:]).all())


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("bad", ["nan", "inf"])
def test_nan_and_inf_in_bins_and_class_scores(dev, oracle_lib, bad, dt):
    """torch.max ranks a NaN as the maximum and takes the first of several; a NaN confidence fails `> conf_thres`; an inf is an
    ordinary largest value.  Planted on passing rows at both ends of the bins and in a class score."""
    nc, A = 16, 1000
    v = float(bad)
    pred = _pred(A, nc, DTYPES[dt], seed=7200)
    rows = [3, 500, 999]
    for r in rows:
        pred[:, r, 4] = 0.9
        pred[:, r, 5:5 + nc] = 0.02
        pred[:, r, 5 + 2] = 0.8
    pred[0, 3, 5 + nc + 179] = v                            # the last bin ...
    pred[0, 3, 5 + nc + 40] = v                             # ... and an earlier one: the first wins
    pred[0, 500, 5 + nc] = v                                # the first bin
    pred[1, 3, 5 + 7] = v                                   # a class score: conf = obj * v
    pred[1, 999, 5 + nc + 90] = v
    pred[1, 999, 5 + 2] = v
    ref_multi = pyref.non_max_suppression_obb(pred.clone(), multi_label=True, **KW)
    ref_best = pyref.non_max_suppression_obb(pred.clone(), multi_label=False, **KW)
    assert sum(r.shape[0] for r in ref_multi) >= 4
    # (which NMS kernel takes an image with an inf confidence is not this test's subject)
    _run(dev, pred.to(dev), ref_multi, ref_best, (bad, dt), nc, expect_small=False)
