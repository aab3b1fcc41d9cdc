"""GPU: Detect.lazy_nms -- the lazy Detect outputs and the fused NMS that reads the conv outputs (obb_non_max_suppression_obb_head)
against the eager chain (Detect decode -> non_max_suppression_obb), bit for bit, on both bindings.  The conv outputs are fed
through identity Detect.m, as tests/test_e2e_gpu.py and bench.py do."""
import pytest
import torch

from tests import synth

pytestmark = pytest.mark.gpu

P6_ANCHORS, P6_STRIDES = synth.P6_ANCHORS, synth.P6_STRIDES


@pytest.fixture(params=["compiled", "ctypes"])
def binding(request, monkeypatch):
    from yolov5_obb_amd import _lib
    ext = _lib.compiled()
    assert ext is not None, "nms_rotated_ext_c.so is not built"
    if request.param == "ctypes":
        monkeypatch.setattr(_lib, "_ext", None)
        monkeypatch.setattr(_lib, "_ext_tried", True)
    return request.param


def _detect(nc, nl, dev, dtype):
    from yolov5_obb_amd.models.yolo import Detect
    anchors, strides = (synth.DEFAULT_ANCHORS, synth.DEFAULT_STRIDES) if nl == 3 else (P6_ANCHORS, P6_STRIDES)
    det = Detect(nc=nc, anchors=anchors, ch=(8,) * nl)
    det.stride = torch.tensor(strides)
    det.anchors /= det.stride.view(-1, 1, 1)
    det = det.to(dev).to(dtype).eval()
    det.m = torch.nn.ModuleList([torch.nn.Identity() for _ in range(nl)])
    return det


def _heads(bs, nc, shapes, seed, dev, dtype, na=3, k=None):
    """Conv outputs (bs, na*no, ny, nx): background like synth.s_head (objectness logit ~ N(-6, 1.5), class / angle ~ N(-4, .)),
    plus k confident cells per image and level with a class and a CSL bump; several of them share a class, some a position."""
    g = torch.Generator().manual_seed(seed)
    no = 5 + nc + 180
    out = []
    for ny, nx in shapes:
        x = torch.randn(bs, na, ny, nx, no, generator=g) * 0.5
        x[..., 4] = torch.randn(bs, na, ny, nx, generator=g) * 1.5 - 6.0
        x[..., 5:] -= 4.0
        kk = k if k is not None else max(3, ny * nx // 12)
        for b in range(bs):
            a = torch.randint(0, na, (kk,), generator=g)
            yy, xx = torch.randint(0, ny, (kk,), generator=g), torch.randint(0, nx, (kk,), generator=g)
            cls, ang = torch.randint(0, nc, (kk,), generator=g), torch.randint(0, 180, (kk,), generator=g)
            x[b, a, yy, xx, 4] = 1.0 + 3.0 * torch.rand(kk, generator=g)
            x[b, a, yy, xx, 5 + cls] = 1.5 + 2.0 * torch.rand(kk, generator=g)
            x[b, a, yy, xx, 5 + nc + ang] = 4.0
            x[b, a, yy, xx, 5 + nc + (ang + 1) % 180] = 4.0          # two equal bins: the first maximum decides
        out.append(x.permute(0, 1, 4, 2, 3).contiguous().view(bs, na * no, ny, nx).to(dtype).to(dev))
    return out


def _run(det, heads, lazy, couple=True, **kw):
    from yolov5_obb_amd.utils.general import non_max_suppression_obb
    det.lazy_nms, det.couple_nms = lazy, couple
    try:
        with torch.no_grad():
            z, x = det(list(heads))
            out = non_max_suppression_obb(z, **kw)
    finally:
        det.lazy_nms, det.couple_nms = False, True
    return z, x, out


def _same(a, b):
    assert len(a) == len(b)
    for i, (p, q) in enumerate(zip(a, b)):
        assert p.shape == q.shape and torch.equal(p, q), (i, p.shape, q.shape)


def _check(det, heads, **kw):
    _, _, eager = _run(det, heads, False, couple=True, **kw)
    _, _, plain = _run(det, heads, False, couple=False, **kw)
    z, _, lazy = _run(det, heads, True, **kw)
    assert not z.is_materialized(), "the fused entry did not run"
    _same(lazy, eager)
    _same(lazy, plain)
    return lazy


KW = dict(conf_thres=0.25, iou_thres=0.45, multi_label=True, max_det=300)


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("nc", [1, 2, 15, 16, 33])
def test_lazy_equals_eager_dtypes_and_classes(dev, binding, dtype, nc):
    det = _detect(nc, 3, dev, dtype)
    heads = _heads(3, nc, [(32, 32), (16, 16), (8, 8)], seed=nc, dev=dev, dtype=dtype)
    out = _check(det, heads, **KW)
    assert sum(int(o.shape[0]) for o in out) > 0


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("nl,shapes,bs", [
    (4, [(64, 64), (32, 32), (16, 16), (8, 8)], 1),                 # P6
    (3, [(13, 13), (7, 7), (5, 5)], 3),                             # odd sizes: element-wise tile loads
    (3, [(128, 80), (64, 40), (32, 20)], 3),                        # letterboxed, non-square
    (3, [(64, 64), (32, 32), (16, 16)], 16),
])
def test_lazy_equals_eager_shapes(dev, binding, dtype, nl, shapes, bs):
    det = _detect(16, nl, dev, dtype)
    heads = _heads(bs, 16, shapes, seed=7 + nl + bs, dev=dev, dtype=dtype)
    _check(det, heads, **KW)


@pytest.mark.parametrize("kw", [
    dict(conf_thres=0.001, iou_thres=0.45, multi_label=True, max_det=300),
    dict(conf_thres=0.6, iou_thres=0.2, multi_label=True, max_det=1500),
    dict(conf_thres=0.25, iou_thres=0.45, multi_label=False, max_det=1500),
    dict(conf_thres=0.25, iou_thres=0.2, multi_label=True, agnostic=True, max_det=300),
    dict(conf_thres=0.25, iou_thres=0.45, multi_label=True, classes=[0, 3, 7], max_det=300),
    dict(conf_thres=0.001, iou_thres=0.45, multi_label=False, classes=[1], max_det=1500),
])
def test_lazy_equals_eager_arguments(dev, binding, kw):
    det = _detect(15, 3, dev, torch.float16)
    heads = _heads(3, 15, [(40, 40), (20, 20), (10, 10)], seed=11, dev=dev, dtype=torch.float16)
    _check(det, heads, **kw)


def test_lazy_equals_eager_with_label_rows(dev, binding):
    det = _detect(15, 3, dev, torch.float32)
    heads = _heads(2, 15, [(32, 32), (16, 16), (8, 8)], seed=5, dev=dev, dtype=torch.float32)
    labels = [torch.tensor([[3, 100.0, 120.0, 40.0, 20.0], [7, 30.0, 40.0, 12.0, 9.0]]), torch.tensor([[1, 60.0, 70.0, 25.0, 10.0]])]
    _check(det, heads, labels=labels, **KW)


@pytest.mark.parametrize("conf", [0.25, 0.001])
def test_bench_workload(dev, binding, conf):
    """bench.py's chain: s_head seed 2000, bs 16, nc 16, 1024^2 (levels 128 / 64 / 32), fp16, multi-label, max_det 1500.  At conf
    0.001 the candidates overflow the first cap_img and the large segments send the call through its retries."""
    from yolov5_obb_amd.utils.general import hints_clear
    det = _detect(16, 3, dev, torch.float16)
    heads = [h.to(dev) for h in synth.s_head(16, 16, (128, 64, 32), seed=2000, n_obj=120, dtype=torch.float16)]
    kw = dict(conf_thres=conf, iou_thres=0.45, multi_label=True, max_det=1500)
    hints_clear()
    out = _check(det, heads, **kw)
    hints_clear()
    z, _, first = _run(det, heads, True, **kw)                       # a lazy call on a fresh memo: its own retries
    assert not z.is_materialized()
    _same(first, out)
    assert sum(int(o.shape[0]) for o in out) > 16 * 50


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_materialised_outputs_equal_eager(dev, dtype):
    det = _detect(15, 3, dev, dtype)
    heads = _heads(2, 15, [(24, 40), (12, 20), (6, 10)], seed=3, dev=dev, dtype=dtype)
    det.lazy_nms = True
    try:
        with torch.no_grad():
            z, x = det(list(heads))
    finally:
        det.lazy_nms = False
    with torch.no_grad():
        ze, xe = det(list(heads))
    assert type(z).__name__ == "LazyTensor" and z.shape == ze.shape and z.dtype == ze.dtype and z.device == ze.device
    assert torch.equal(z.materialize(), ze) and z.is_materialized()
    for xi, xei in zip(x, xe):
        assert not xi.is_materialized()
        r = xi.materialize()
        assert r.shape == xei.shape == (2, 3, xei.shape[2], xei.shape[3], 20 + 180) and r.is_contiguous() and torch.equal(r, xei)


def test_inplace_edit_of_z_takes_the_eager_path(dev, binding):
    det = _detect(15, 3, dev, torch.float16)
    heads = _heads(2, 15, [(32, 32), (16, 16), (8, 8)], seed=9, dev=dev, dtype=torch.float16)
    from yolov5_obb_amd.utils.general import non_max_suppression_obb
    det.lazy_nms = True
    try:
        with torch.no_grad():
            z, _ = det(list(heads))
            z[..., 4] = 0
            out = non_max_suppression_obb(z, **KW)
    finally:
        det.lazy_nms = False
    assert type(z).__name__ == "LazyTensor" and z.is_materialized()
    assert all(o.shape[0] == 0 for o in out)


def test_tta_sequence_equals_eager(dev, binding):
    """Model._forward_augment / _descale_pred (models/yolo.py of the reference): in-place descale of xy / wh, a flip, then
    torch.cat of three outputs."""
    from yolov5_obb_amd.utils.general import non_max_suppression_obb
    det = _detect(15, 3, dev, torch.float32)
    heads = [_heads(1, 15, [(32, 32), (16, 16), (8, 8)], seed=20 + i, dev=dev, dtype=torch.float32) for i in range(3)]

    def tta(lazy):
        det.lazy_nms = lazy
        ys = []
        try:
            with torch.no_grad():
                for i, (s, f) in enumerate(((1.0, None), (0.83, 3), (0.67, None))):
                    p, _ = det(list(heads[i]))
                    p[..., :4] /= s                                   # de-scale
                    if f == 3:
                        p[..., 0] = 256 - p[..., 0]                   # de-flip lr
                    ys.append(p)
                y = torch.cat(ys, 1)
        finally:
            det.lazy_nms = False
        return non_max_suppression_obb(y, **KW)
    _same(tta(True), tta(False))


def test_inplace_edit_of_a_conv_output_raises(dev, binding):
    from yolov5_obb_amd.utils.general import non_max_suppression_obb
    det = _detect(15, 3, dev, torch.float16)
    heads = _heads(1, 15, [(16, 16), (8, 8), (4, 4)], seed=4, dev=dev, dtype=torch.float16)
    det.lazy_nms = True
    try:
        with torch.no_grad():
            z, x = det(list(heads))
            heads[1].mul_(2.0)
            with pytest.raises(RuntimeError, match="modified in place"):
                non_max_suppression_obb(z, **KW)
            with pytest.raises(RuntimeError, match="modified in place"):
                z.materialize()
            with pytest.raises(RuntimeError, match="modified in place"):
                x[0] + 1
    finally:
        det.lazy_nms = False


def test_fallbacks_return_plain_tensors(dev):
    det = _detect(15, 3, dev, torch.float16)
    heads = _heads(1, 15, [(16, 16), (8, 8), (4, 4)], seed=2, dev=dev, dtype=torch.float16)
    with torch.no_grad():
        ze, _ = det(list(heads))
        z, _ = det(list(heads))                                     # lazy_nms off (the default)
    assert type(z) is torch.Tensor and torch.equal(z, ze)
    det.lazy_nms = True
    try:
        with torch.enable_grad():
            z, _ = det(list(heads))                                 # grad enabled
        assert type(z) is torch.Tensor and torch.equal(z, ze)
        with torch.inference_mode():
            z, _ = det([h.clone() for h in heads])                  # inference mode
        assert type(z) is torch.Tensor and torch.equal(z.clone(), ze)
    finally:
        det.lazy_nms = False
    # nl > 4: five levels
    from yolov5_obb_amd.models.yolo import Detect
    a5 = P6_ANCHORS + [[900, 900, 1000, 800, 1100, 1200]]
    d5 = Detect(nc=15, anchors=a5, ch=(8,) * 5)
    d5.stride = torch.tensor(P6_STRIDES + [128.0])
    d5.anchors /= d5.stride.view(-1, 1, 1)
    d5 = d5.to(dev).half().eval()
    d5.m = torch.nn.ModuleList([torch.nn.Identity() for _ in range(5)])
    h5 = _heads(1, 15, [(32, 32), (16, 16), (8, 8), (4, 4), (2, 2)], seed=6, dev=dev, dtype=torch.float16)
    with torch.no_grad():
        ze5, _ = d5(list(h5))
        d5.lazy_nms = True
        z5, _ = d5(list(h5))
    assert type(z5) is torch.Tensor and torch.equal(z5, ze5)


def test_repeated_lazy_calls_are_identical(dev, binding):
    """Ten lazy calls in a row on one stream: the caller-kept state is left zeroed by every call."""
    det = _detect(16, 3, dev, torch.float16)
    heads = _heads(4, 16, [(64, 64), (32, 32), (16, 16)], seed=1, dev=dev, dtype=torch.float16)
    _, _, ref = _run(det, heads, False, **KW)
    for _ in range(10):
        z, _, out = _run(det, heads, True, **KW)
        assert not z.is_materialized()
        _same(out, ref)
