"""GPU: the fused non_max_suppression_obb on bfloat16 predictions -- decoded z through the ctypes path and the compiled binding,
and the lazy entry that reads bf16 conv outputs (obb_non_max_suppression_obb_head) -- against the restated reference run on
the same bf16 tensor on the CPU (oracle/pyref.py, written against x.dtype).  Rows, order and values are exact, as
tests/test_nmsobb_gpu.py::_cmp asks of fp16.

bf16 is the harsher input for the sort paths: a confidence has 8 significand bits (128 values per octave), so with
conf_thres = 0.001 and multi_label most candidates share their confidence with others (image 0 of the (2, 3000, 15) case below:
3038 candidates, 805 distinct confidences) and the pinned tie order (ascending anchor * nc + class) decides the kept list; decoded
centres above 512 px sit on a 4-pixel lattice, so exact duplicate boxes are common."""
import pytest
import torch

from oracle import pyref
from tests import head_cases as H
from tests import synth
from tests.test_lazy_nms_gpu import binding  # noqa: F401  (compiled and ctypes bindings)
from tests.test_nmsobb_gpu import _cmp
from tests.test_nonfinite_gpu import Z_KWS, _cmp as _cmp_nan, _plant_z

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16


def _nms(pred, **kw):
    from yolov5_obb_amd.utils.general import non_max_suppression_obb
    return non_max_suppression_obb(pred, **kw)


CASES = {
    "conf25_best_class": ((2, 3000, 15), dict(conf_thres=0.25, iou_thres=0.45, multi_label=False, max_det=300)),
    "conf001_multi_ties": ((2, 3000, 15), dict(conf_thres=0.001, iou_thres=0.45, multi_label=True, max_det=300)),
    "nc2_conf05_multi": ((3, 4000, 2), dict(conf_thres=0.05, iou_thres=0.45, multi_label=True, max_det=300)),
    "agnostic": ((2, 3000, 15), dict(conf_thres=0.1, iou_thres=0.45, multi_label=True, agnostic=True, max_det=300)),
    "classes": ((2, 3000, 15), dict(conf_thres=0.1, iou_thres=0.45, multi_label=True, classes=[1, 4, 9], max_det=300)),
}
_REF = {}


def _case(name):
    """(bf16 prediction on the CPU, reference rows): computed once, shared by both bindings, never modified."""
    if name not in _REF:
        (bs, A, nc), kw = CASES[name]
        pred = synth.s_pred(bs, A, nc, seed=700 + A + nc).to(BF16)
        _REF[name] = (pred, pyref.non_max_suppression_obb(pred.clone(), **kw))
    return _REF[name]


@pytest.mark.parametrize("name", list(CASES))
def test_bf16_prediction_vs_pyref(dev, oracle_lib, binding, name):
    from yolov5_obb_amd.utils import general
    pred, ref = _case(name)
    kw = CASES[name][1]
    assert sum(int(r.shape[0]) for r in ref) > 20
    if name == "conf001_multi_ties":
        assert all(int(r.shape[0]) == kw["max_det"] for r in ref)         # both images are cut at max_det
        x = pred[0].float()
        conf = (pred[0, :, 5:20] * pred[0, :, 4:5]).float()               # the product in bf16, as utils/general.py:820
        cand = conf[(x[:, 4:5] > 0.001).expand_as(conf) & (conf > 0.001)]
        assert cand.numel() > 3 * cand.unique().numel()                   # ties dominate: over three candidates per confidence
    general.hints_clear()
    p = pred.to(dev)
    for rep in range(2):                                                  # un-hinted, then on the first call's hints
        _cmp(_nms(p, **kw), ref)


def test_bf16_threshold_is_compared_in_bf16(dev, oracle_lib, binding):
    """conf_thres = 0.2515 rounds UP to bf16 0.251953125 (the scalar is cast to the tensor dtype, utils/general.py:785): a row at
    exactly 0.251953125 fails `>` although it is above the float 0.2515.  Objectness and obj * cls at 0.25, 0.251953125 and
    0.25390625; boxes sit apart, so the NMS keeps every candidate."""
    nc, A = 4, 64
    ci = 5 + nc
    edges = (0.25, 0.251953125, 0.25390625)
    assert all(float(torch.tensor(e, dtype=BF16)) == e for e in edges) and float(torch.tensor(0.2515, dtype=BF16)) == edges[1]
    pred = torch.zeros(1, A, ci + 180, dtype=BF16)
    i = torch.arange(A)
    pred[0, :, 0] = (50 + 80 * (i % 8)).to(BF16)
    pred[0, :, 1] = (50 + 80 * (i // 8)).to(BF16)
    pred[0, :, 2], pred[0, :, 3] = 30.0, 20.0
    pred[0, :, 4] = -1.0
    pred[0, :, ci:] = torch.linspace(-0.9, -0.1, 180).to(BF16)
    r = 0
    for e in edges:                                                       # objectness at the edge, cls = 1
        pred[0, r, 4], pred[0, r, 5 + r % nc] = e, 1.0
        r += 1
    for e in edges:                                                       # cls at the edge, objectness = 1
        pred[0, r, 4], pred[0, r, 5 + r % nc] = 1.0, e
        r += 1
    for e in edges:                                                       # objectness 0.5, cls = 2 x the edge: the product is the edge
        pred[0, r, 4], pred[0, r, 5 + r % nc] = 0.5, 2 * e
        r += 1
    for multi in (True, False):
        kw = dict(conf_thres=0.2515, iou_thres=0.45, multi_label=multi, max_det=300)
        ref = pyref.non_max_suppression_obb(pred.clone(), **kw)
        confs = sorted(ref[0][:, 5].tolist())
        # of the nine rows only the three whose confidence is 0.25390625 pass: 0.251953125 > bf16(0.2515) is false
        assert confs == [edges[2]] * 3, confs
        _cmp(_nms(pred.to(dev), **kw), ref)
        # the same rows against the float threshold 0.25 pass at 0.251953125 too
        kw25 = dict(kw, conf_thres=0.25)
        ref25 = pyref.non_max_suppression_obb(pred.clone(), **kw25)
        assert sorted(ref25[0][:, 5].tolist()) == [edges[1]] * 3 + [edges[2]] * 3
        _cmp(_nms(pred.to(dev), **kw25), ref25)


@pytest.mark.parametrize("multi", [True, False])
@pytest.mark.parametrize("nc", [2, 40])
def test_bf16_nonfinite_rows_vs_pyref(dev, oracle_lib, binding, nc, multi):
    """The planted rows of tests/test_nonfinite_gpu.py (NaN of both signs, +-inf, -0 in objectness, class, CSL and box columns),
    cast to bf16 -- a signalling pattern becomes a quiet NaN on the way, every other special value survives the cast."""
    pred = _plant_z(synth.s_pred(2, 3000, nc, seed=500 + nc, fg_frac=0.03), nc, seed=nc).to(BF16)
    assert bool(torch.isnan(pred.float()).any()) and bool(torch.isinf(pred.float()).any())
    p = pred.to(dev)
    for kw in Z_KWS:
        kw = dict(kw, multi_label=multi, max_det=300)
        ref = pyref.non_max_suppression_obb(pred.clone(), **kw)
        assert sum(int(r.shape[0]) for r in ref) > 20
        _cmp_nan(_nms(p, **kw), ref)


# ------------------------------------------------------------------ the lazy entry on bf16 conv outputs
def _detect(case, dev):
    from yolov5_obb_amd.models.yolo import Detect
    det = Detect(nc=case.nc, anchors=H.detect_anchor_arg(case), ch=(8,) * case.nl)
    det.stride = torch.tensor(H.strides(case))
    det.anchors /= det.stride.view(-1, 1, 1)
    det = det.to(dev).bfloat16().eval()
    det.m = torch.nn.ModuleList([torch.nn.Identity() for _ in range(case.nl)])
    return det


def _run(det, heads, lazy, **kw):
    det.lazy_nms = lazy
    try:
        with torch.no_grad():
            z, _ = det(list(heads))
            out = _nms(z, **kw)
    finally:
        det.lazy_nms = False
    return z, out


@pytest.mark.parametrize("multi_label", [True, False], ids=["multi_label", "best_class"])
@pytest.mark.parametrize("name", H.NAMES)
def test_bf16_lazy_head_equals_eager_and_pyref(dev, oracle_lib, binding, name, multi_label):
    """obb_non_max_suppression_obb_head on bf16 conv outputs == obb_detect_decode_levels followed by the NMS on z, on the same
    device, bit for bit (Detect.lazy_nms = True against False, end to end); and the eager rows are the reference's on that z."""
    from yolov5_obb_amd.utils import general
    case = H.BY_NAME[name]
    det = _detect(case, dev)
    heads = [c.to(BF16).to(dev) for c in H.convs(case, torch.float32)]
    kw = dict(multi_label=multi_label, **H.KW)
    z, eager = _run(det, heads, False, **kw)
    assert z.dtype == BF16
    ref = pyref.non_max_suppression_obb(z.cpu().clone(), **kw)
    _cmp(eager, ref)
    assert sum(int(r.shape[0]) for r in ref) >= H.coverage_floor(case)[0]
    general.hints_clear()
    for rep in range(2):
        zl, lazy = _run(det, heads, True, **kw)
        assert type(zl).__name__ == "LazyTensor" and zl.dtype == BF16 and not zl.is_materialized(), "the fused entry did not run"
        assert len(lazy) == len(eager) and all(torch.equal(a, b) for a, b in zip(lazy, eager)), rep
