"""GPU: Detect.lazy_tta -- forward_augment's lazy output and the fused NMS that reads the passes' conv outputs
(obb_non_max_suppression_obb_tta_head, k_decode_head<T, true>) against the eager chain on the same device: _decode_tta
(Detect.fused_tta) followed by non_max_suppression_obb on that tensor.  torch.equal per image, no tolerance, both bindings.

The conv outputs are fed through identity Detect.m (tests/lazy_tta_cases.py).  Before anything is compared the eager tensors are
held to preconditions without which an agreement would say little: every listed (pass, level) entry has a row that passes both
thresholds, every pass contributes a kept detection (one of them from a flipped pass), and the NMS suppresses something."""
import pytest
import torch

from tests import lazy_tta_cases as TC
from tests.lazy_tta_cases import CASES, DTYPES, FLIPS, KW, SCALES
from tests.test_tta_decode_gpu import StandIn, bits

pytestmark = pytest.mark.gpu

SEED = TC.SEED


@pytest.fixture(params=["compiled", "ctypes"])
def binding(request, monkeypatch):
    from yolov5_obb_amd import _lib
    ext = _lib.compiled()
    assert ext is not None, "nms_rotated_ext_c.so is not built"
    if request.param == "ctypes":
        monkeypatch.setattr(_lib, "_ext", None)
        monkeypatch.setattr(_lib, "_ext_tried", True)
    return request.param


def nms(z, **kw):
    from yolov5_obb_amd.utils.general import non_max_suppression_obb
    with torch.no_grad():
        return non_max_suppression_obb(z, **kw)


def run_case(dev, case, dt, scales, flips, seed, kw=KW, check=True):
    det = TC.make_detect(case, dev, DTYPES[dt])
    convs = TC.heads(case, dev, DTYPES[dt], seed)
    ze, plan = TC.eager(det, convs, case, scales, flips)
    want = nms(ze, **kw)
    if check:
        print("candidates %d, kept %d, kept per pass %s" % TC.preconditions(ze, plan, want, flips, kw["conf_thres"], det.na, CASES[case][5]))
    with torch.no_grad():
        z = TC.augment(det, convs, case, scales, flips, lazy_tta=True)
    assert type(z).__name__ == "LazyTensor" and z.shape == ze.shape and z.dtype == ze.dtype and z.device == ze.device
    got = nms(z, **kw)
    assert not z.is_materialized(), "the fused entry did not run"
    TC.same(got, want)
    return det, convs, z, ze, want


@pytest.mark.parametrize("flips", FLIPS, ids=["lr_mid", "ud_first_lr_last"])
@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("dt", list(DTYPES))
def test_lazy_equals_fused_then_nms(dev, binding, dt, case, flips):
    run_case(dev, case, dt, SCALES, flips, SEED[case])


@pytest.mark.parametrize("dt", list(DTYPES))
def test_scale_whose_two_reciprocals_differ(dev, binding, dt):
    """s = 0.85: float(1 / s) taken in double and 1.0f / float(s) differ by one ulp (tests/test_tta_decode_gpu.py)."""
    s = 0.85
    assert float(torch.tensor(1 / s)) != float(torch.tensor(1.0) / torch.tensor(s))
    case, scales, flips, seed = TC.IDENTITY_CASES[-1]
    assert scales == (1, s, s)
    run_case(dev, case, dt, scales, flips, seed)


LABELS = [torch.tensor([[2, 40.0, 50.0, 30.0, 12.0], [0, 90.0, 30.0, 12.0, 9.0]]), torch.tensor([[1, 60.0, 70.0, 25.0, 10.0]])]


@pytest.mark.parametrize("kw", [
    dict(conf_thres=0.001, iou_thres=0.45, multi_label=True, max_det=300),
    dict(conf_thres=0.25, iou_thres=0.45, multi_label=False, max_det=300),
    dict(conf_thres=0.25, iou_thres=0.2, multi_label=True, agnostic=True, max_det=300),
    dict(conf_thres=0.25, iou_thres=0.45, multi_label=True, classes=[0, 2], max_det=300),
    dict(conf_thres=0.25, iou_thres=0.45, multi_label=True, labels=LABELS, max_det=300),
    dict(conf_thres=0.25, iou_thres=0.45, multi_label=True, max_det=7),
], ids=["conf0.001", "best_class", "agnostic", "classes", "labels", "max_det"])
def test_arguments(dev, binding, kw):
    _, _, _, _, want = run_case(dev, "nc3_128", "fp16", SCALES, FLIPS[0], SEED["nc3_128"], kw=kw, check=False)
    assert sum(int(o.shape[0]) for o in want) > 0
    if kw["max_det"] == 7:                                            # smaller than the kept count: the cut is what is compared
        full = nms(TC.eager(TC.make_detect("nc3_128", dev, torch.float16), TC.heads("nc3_128", dev, torch.float16, SEED["nc3_128"]),
                            "nc3_128", SCALES, FLIPS[0])[0], **dict(kw, max_det=300))
        assert all(int(f.shape[0]) > 7 and int(w.shape[0]) == 7 for f, w in zip(full, want))


def test_materialised_output_is_the_fused_tensor(dev):
    case = "nc3_128"
    det = TC.make_detect(case, dev, torch.float16)
    convs = TC.heads(case, dev, torch.float16, 3)
    ze, _ = TC.eager(det, convs, case, SCALES, FLIPS[1])
    with torch.no_grad():
        z = TC.augment(det, convs, case, SCALES, FLIPS[1], lazy_tta=True)
        assert type(z).__name__ == "LazyTensor" and not z.is_materialized() and type(z.payload).__name__ == "LazyTtaHead"
        box = z[..., :4].clone()
    assert z.is_materialized() and z.payload is None
    assert torch.equal(bits(box), bits(ze[..., :4])) and torch.equal(bits(z.materialize()), bits(ze))
    TC.same(nms(z, **KW), nms(ze, **KW))                              # a materialised output takes the plain path
    assert "_collect" not in vars(det) and "lazy_tta" not in vars(det)


def test_inplace_edit_of_a_conv_output_raises(dev, binding):
    case = "nc3_128"
    det = TC.make_detect(case, dev, torch.float16)
    convs = TC.heads(case, dev, torch.float16, 4)
    with torch.no_grad():
        z = TC.augment(det, convs, case, SCALES, FLIPS[0], lazy_tta=True)
        convs[1][0].mul_(2.0)
        with pytest.raises(RuntimeError, match="modified in place"):
            nms(z, **KW)
        with pytest.raises(RuntimeError, match="modified in place"):
            z.materialize()
        with pytest.raises(RuntimeError, match="modified in place"):
            z + 1


def test_fallbacks_return_plain_tensors(dev):
    """inference mode, grad enabled: what forward_augment returns today with the flags it is given -- lazy_tta alone: the chain of
    torch ops on the eager passes; with fused_tta: the fused tensor.  Same bits either way."""
    case = "nc3_128"
    det = TC.make_detect(case, dev, torch.float16)
    convs = TC.heads(case, dev, torch.float16, 5)
    ze, _ = TC.eager(det, convs, case, SCALES, FLIPS[0])
    for flags in (dict(lazy_tta=True), dict(lazy_tta=True, fused_tta=True), dict(lazy_tta=True, lazy_nms=True)):
        with torch.inference_mode():
            z = TC.augment(det, convs, case, SCALES, FLIPS[0], **flags)
            assert type(z) is torch.Tensor and torch.equal(bits(z), bits(ze)), flags
        with torch.enable_grad():
            z = TC.augment(det, convs, case, SCALES, FLIPS[0], **flags)
        assert type(z) is torch.Tensor and torch.equal(bits(z), bits(ze)), flags
    with torch.no_grad():                                             # the flag off: fused_tta still wins over lazy_nms
        z = TC.augment(det, convs, case, SCALES, FLIPS[0], fused_tta=True, lazy_nms=True)
    assert type(z) is torch.Tensor and torch.equal(bits(z), bits(ze))


def test_off_boundary_plan_falls_back(dev):
    """Ceil-mode pools on 136 x 136 (tests/test_tta_decode_gpu.py): the first pass's cut splits a level, the chain runs."""
    from yolov5_obb_amd.models.yolo import forward_augment
    model = StandIn(ceil_mode=True).to(dev).half().eval()
    det = model.model[-1]
    x = torch.rand(1, 3, 136, 136, generator=torch.Generator().manual_seed(3)).to(dev).half()
    with torch.no_grad():
        want, _ = forward_augment(model, x)
        det.lazy_tta = True
        try:
            got, none = forward_augment(model, x)
        finally:
            del det.lazy_tta
    assert none is None and type(got) is torch.Tensor and got.shape == want.shape and torch.equal(bits(got), bits(want))
    assert "_collect" not in vars(det)


def test_forward_augment_of_a_model_with_convs(dev, binding):
    """The whole path behind real 1x1 convs and pools (on the level boundary): lazy equals fused_tta + NMS."""
    from yolov5_obb_amd.models.yolo import forward_augment
    model = StandIn().to(dev).half().eval()
    det = model.model[-1]
    x = torch.rand(2, 3, 128, 128, generator=torch.Generator().manual_seed(2)).to(dev).half()
    kw = dict(KW, conf_thres=0.05)
    with torch.no_grad():
        det.fused_tta = True
        try:
            ze, _ = forward_augment(model, x)
        finally:
            del det.fused_tta
        det.lazy_tta = True
        try:
            z, _ = forward_augment(model, x)
        finally:
            del det.lazy_tta
    want, got = nms(ze, **kw), nms(z, **kw)
    assert type(z).__name__ == "LazyTensor" and not z.is_materialized()
    TC.same(got, want)
    assert sum(int(o.shape[0]) for o in want) > 0


def test_repeated_lazy_calls_are_identical(dev, binding):
    """Two lazy calls in a row on one stream give the eager result: the caller-kept state is left zeroed by every call."""
    case = "nc3_128"
    det = TC.make_detect(case, dev, torch.float16)
    convs = TC.heads(case, dev, torch.float16, SEED[case])
    want = nms(TC.eager(det, convs, case, SCALES, FLIPS[0])[0], **KW)
    for _ in range(2):
        with torch.no_grad():
            z = TC.augment(det, convs, case, SCALES, FLIPS[0], lazy_tta=True)
        got = nms(z, **KW)
        assert not z.is_materialized()
        TC.same(got, want)
    assert "_collect" not in vars(det)


def test_side_stream(dev, binding):
    case = "nc3_128"
    det = TC.make_detect(case, dev, torch.float16)
    convs = TC.heads(case, dev, torch.float16, SEED[case])
    want = nms(TC.eager(det, convs, case, SCALES, FLIPS[0])[0], **KW)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side), torch.no_grad():
        z = TC.augment(det, convs, case, SCALES, FLIPS[0], lazy_tta=True)
        got = [o.cpu() for o in nms(z, **KW)]                         # reads on that stream
    side.synchronize()
    assert not z.is_materialized()
    TC.same(got, [w.cpu() for w in want])
