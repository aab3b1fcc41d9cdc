"""CPU: the lazy Detect output (yolov5_obb_amd/lazy.py) with a CPU materialiser, the C entry it feeds
(obb_non_max_suppression_obb_head) and the Detect.lazy_nms switch -- no GPU needed."""
import ctypes
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lazy(calls, shape=(2, 5, 7), dtype=torch.float32):
    from yolov5_obb_amd.lazy import LazyTensor
    base = torch.arange(torch.Size(shape).numel(), dtype=torch.float32).view(shape).to(dtype)

    def make():
        calls.append(1)
        return base.clone()
    return LazyTensor(shape, dtype, torch.device("cpu"), make, payload="record"), base


def test_metadata_without_materialising():
    calls = []
    z, _ = _lazy(calls, dtype=torch.float16)
    assert z.shape == (2, 5, 7) and z.dtype == torch.float16 and z.device.type == "cpu" and z.dim() == 3
    assert z.is_contiguous() and z.contiguous() is z
    assert not z.is_materialized() and z.payload == "record" and calls == []


def test_first_op_materialises_exactly_once():
    calls = []
    z, base = _lazy(calls)
    assert torch.equal(z[..., :4], base[..., :4])
    assert calls == [1] and z.is_materialized() and z.payload is None
    assert torch.equal(z + 1, base + 1) and float(z.sum()) == float(base.sum())
    assert calls == [1]


def test_inplace_views_cat_clone_equal_the_materialised_tensor():
    calls = []
    z, base = _lazy(calls)
    ref = base.clone()
    z[..., :4] /= 2.0                                   # Model._descale_pred: p[..., :4] /= scale
    ref[..., :4] /= 2.0
    w = z
    w *= 3.0                                            # in place on the wrapper: the caller keeps the wrapper
    ref *= 3.0
    assert w is z and type(z).__name__ == "LazyTensor"
    assert torch.equal(z.materialize(), ref)
    v = z[:, 1:3]
    assert torch.equal(v, ref[:, 1:3]) and type(v) is torch.Tensor
    c = torch.cat((z, z[:, :2]), 1)                     # TTA: torch.cat(y, 1)
    assert type(c) is torch.Tensor and torch.equal(c, torch.cat((ref, ref[:, :2]), 1))
    cl = z.clone()
    assert type(cl) is torch.Tensor and torch.equal(cl, ref)
    assert calls == [1]


def test_materialises_under_inference_mode():
    calls = []
    z, base = _lazy(calls)
    with torch.inference_mode():
        assert torch.equal(z * 2, base * 2)
    assert calls == [1]


def test_library_exports_the_head_entry():
    from yolov5_obb_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    L = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(L, "obb_non_max_suppression_obb_head")
    assert "obb_non_max_suppression_obb_head" in _lib.SIGNATURES
    text = open(os.path.join(ROOT, "include", "obb_hip.h")).read()
    assert "int obb_non_max_suppression_obb_head(" in text


def test_head_entry_checks_its_arguments_before_any_device_call():
    """OBB_ERR_BAD_ARG (-1) for nl out of range, NULL tables or level pointers, unknown dtype, nc or na out of range."""
    import ctypes as C
    from yolov5_obb_amd import _lib
    L = _lib.lib()
    null = C.c_void_p(0)
    n8 = (C.c_int64 * 4)(8, 8, 8, 8)
    ptrs = (C.c_void_p * 4)(256, 512, 768, 1024)
    nulls = (C.c_void_p * 4)(256, 0, 768, 1024)
    px = (C.c_float * 64)(*([4.0] * 64))
    st = (C.c_float * 4)(8.0, 16.0, 32.0, 64.0)
    no16 = 5 + 16 + 180

    def call(nl=3, conv=ptrs, dtype=1, na=3, no=no16, ny=n8, nx=n8, anchors=px, strides=st):
        return L.obb_non_max_suppression_obb_head(nl, conv, dtype, 2, na, no, ny, nx, anchors, strides, 0.25, 0.45, null, 0, 0, 1,
                                                  300, 30000, 4096.0, null, 0, 1024, 0, null, 0, null, null, null, 0, null, 0, null)
    cases = [dict(nl=0), dict(nl=5), dict(conv=null), dict(conv=nulls), dict(dtype=7), dict(na=0), dict(na=9),
             dict(no=5 + 180), dict(no=5 + 257 + 180), dict(ny=null), dict(nx=null), dict(anchors=null), dict(strides=null)]
    for kw in cases:
        assert call(**kw) == -1, kw


def test_detect_lazy_nms_exists_and_is_off_by_default():
    from yolov5_obb_amd.models.yolo import Detect
    assert Detect.lazy_nms is False
    from tests import synth
    det = Detect(nc=4, anchors=synth.DEFAULT_ANCHORS, ch=(8, 8, 8))
    assert det.lazy_nms is False
