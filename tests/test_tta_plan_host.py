"""CPU: the row plan of fused augmented inference (yolov5_obb_amd.models.yolo.tta_plan), the package's scale_img against the
reference's, and the argument refusals of obb_detect_decode_tta (answered before any device call: no GPU needed)."""
import ctypes as C
import math
import os
import sys

import pytest
import torch

REF = "/root/reference"


def _maps(h, w, strides):
    return [(h // s, w // s) for s in strides]


def test_plan_1024_known_answer():
    """1024^2 at scales 1 / 0.83 / 0.67 (inputs 1024, 864, 704), strides 8 / 16 / 32, na 3."""
    from yolov5_obb_amd.models.yolo import tta_plan
    plan = tta_plan([_maps(1024, 1024, (8, 16, 32)), _maps(864, 864, (8, 16, 32)), _maps(704, 704, (8, 16, 32))], 3, 3)
    assert [p.rows for p in plan.passes] == [61440, 45927, 7260]
    assert plan.a_total == 114627 and plan.on_boundary
    assert [p.levels for p in plan.passes] == [(0, 1), (0, 1, 2), (1, 2)]          # pass 0 drops its last level, pass 2 its first
    assert plan.passes[0].offsets == (0, 3 * 128 * 128)
    assert plan.passes[1].offsets == (61440, 61440 + 3 * 108 * 108, 61440 + 3 * (108 * 108 + 54 * 54))
    assert plan.passes[2].offsets == (61440 + 45927, 61440 + 45927 + 3 * 44 * 44)
    assert (plan.passes[0].lo, plan.passes[0].hi) == (0, 61440)
    assert (plan.passes[2].lo, plan.passes[2].hi) == (3 * 88 * 88, 3 * (88 * 88 + 44 * 44 + 22 * 22))


def test_plan_four_levels():
    from yolov5_obb_amd.models.yolo import tta_plan
    shapes = _maps(128, 128, (8, 16, 32, 64))                # 16 / 8 / 4 / 2 in every pass (gs = 64 pads 0.83 and 0.67 back to 128)
    plan = tta_plan([shapes, shapes, shapes], 3, 4)
    A = 3 * (256 + 64 + 16 + 4)
    assert plan.on_boundary
    assert [p.levels for p in plan.passes] == [(0, 1, 2), (0, 1, 2, 3), (1, 2, 3)]
    assert [p.rows for p in plan.passes] == [A - 12, A, A - 768]
    assert plan.a_total == 3 * A - 12 - 768
    assert plan.passes[2].offsets == (2 * A - 12, 2 * A - 12 + 192, 2 * A - 12 + 192 + 48)


def test_plan_reports_a_cut_off_the_level_boundary():
    """Maps 17 / 9 / 5 (a ceil-mode backbone on 136^2): A = 3 * 395 = 1185, 1185 // 21 = 56 rows is not the last level's 75."""
    from yolov5_obb_amd.models.yolo import tta_plan
    shapes = [(17, 17), (9, 9), (5, 5)]
    plan = tta_plan([shapes, shapes, shapes], 3, 3)
    assert not plan.on_boundary
    assert plan.passes[0].rows == 1185 - 56 and plan.passes[2].rows == 1185 - 56 * 16
    assert plan.a_total == 3 * 1185 - 56 - 56 * 16


def test_plan_matches_the_slices_it_stands_for():
    """The kept ranges are those of y[0][:, :-i] / y[-1][:, i:] on tensors of the passes' row counts."""
    from yolov5_obb_amd.models.yolo import tta_plan
    for per_pass, na, nl in (([_maps(160, 96, (8, 16, 32)), _maps(160, 96, (8, 16, 32)), _maps(128, 96, (8, 16, 32))], 3, 3),
                             ([[(17, 17), (9, 9), (5, 5)]] * 3, 3, 3), ([[(4, 4), (2, 2)]] * 2, 2, 2)):
        plan = tta_plan(per_pass, na, nl)
        y = [torch.arange(na * sum(a * b for a, b in s)) for s in per_pass]
        g = sum(4 ** k for k in range(nl))
        i = y[0].shape[0] // g
        y[0] = y[0][:-i]
        i = (y[-1].shape[0] // g) * 4 ** (nl - 1)
        y[-1] = y[-1][i:]
        for t, p in zip(y, plan.passes):
            assert t.tolist() == list(range(p.lo, p.hi)) and p.rows == len(t)
        assert plan.a_total == sum(len(t) for t in y)


def _reference_scale_img():
    """The reference's own scale_img, compiled from its file on its own (utils/torch_utils.py imports cv2, thop, ... at module
    level; the function needs math, torch and F only)."""
    import ast
    import torch.nn.functional as F
    path = os.path.join(REF, "utils", "torch_utils.py")
    tree = ast.parse(open(path).read(), path)
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "scale_img"]
    ns = {"math": math, "torch": torch, "F": F}
    exec(compile(ast.Module(body=fn, type_ignores=[]), path, "exec"), ns)
    return ns["scale_img"]


@pytest.mark.skipif(not os.path.exists(os.path.join(REF, "utils", "torch_utils.py")), reason="needs the reference checkout")
def test_scale_img_equals_the_reference():
    """Ratios 1 / 0.83 / 0.67 on 128 x 128 and 160 x 96 CPU batches, bit for bit."""
    from yolov5_obb_amd.models.yolo import scale_img
    ref_scale_img = _reference_scale_img()
    g = torch.Generator().manual_seed(5)
    for h, w in ((128, 128), (160, 96)):
        img = torch.rand(2, 3, h, w, generator=g)
        for ratio in (1, 0.83, 0.67):
            for gs in (32, 64):
                got, want = scale_img(img, ratio, gs=gs), ref_scale_img(img, ratio, gs=gs)
                assert got.shape == want.shape and torch.equal(got, want), (h, w, ratio, gs)
                assert ratio == 1 or (got.shape[2] % gs == 0 and got.shape[3] % gs == 0)
            assert torch.equal(scale_img(img, ratio, same_shape=True), ref_scale_img(img, ratio, same_shape=True))
        assert scale_img(img, 1) is img


def _pass(nl=1, flip=0, scale=1.0, img=(64, 64), conv=16, ny=8, nx=8):
    from yolov5_obb_amd import _lib
    t = _lib.TtaPass()
    t.nl, t.flip, t.scale, t.img_h, t.img_w = nl, flip, scale, img[0], img[1]
    for j in range(_lib.DETECT_MAX_LEVELS):
        t.conv_out[j], t.ny[j], t.nx[j], t.stride[j] = conv, ny, nx, 8.0
    return t


def test_struct_layout_matches_the_header():
    """obb_tta_pass: 2 x 4 bytes, a double, 2 x 4 bytes, 4 pointers, 2 x 4 int64, 4 floats, 4 x 8 x 2 floats."""
    from yolov5_obb_amd import _lib
    assert C.sizeof(_lib.TtaPass) == 24 + 32 + 64 + 16 + 256
    assert _lib.TtaPass.conv_out.offset == 24 and _lib.TtaPass.anchors_px.offset == 136


def test_tta_argument_refusals_answer_before_any_device_call():
    """Every refusal include/obb_hip.h lists for obb_detect_decode_tta is OBB_ERR_BAD_ARG; the device pointers are never valid
    (NULL, or the address 16), so nothing here can have reached a device."""
    from yolov5_obb_amd import _lib
    L = _lib.lib()
    fake = C.c_void_p(16)
    null = C.c_void_p(0)

    def call(passes, npass=None, dtype=1, bs=1, na=3, no=21, z=fake, a_total=10 ** 6):
        arr = (_lib.TtaPass * max(1, len(passes)))(*passes)
        return L.obb_detect_decode_tta(len(passes) if npass is None else npass, C.cast(arr, C.c_void_p), dtype, bs, na, no, z, a_total,
                                       null, null)

    ok = _pass()
    assert call([ok], npass=0) == -1 and call([ok] * 5, npass=5) == -1 and call([ok], npass=-1) == -1      # npass out of range
    assert L.obb_detect_decode_tta(1, null, 1, 1, 3, 21, fake, 10, null, null) == -1                        # no pass table
    assert call([_pass(nl=0)]) == -1 and call([_pass(nl=5)]) == -1                                         # nl out of range
    for flip in (1, 4, -1):
        assert call([_pass(flip=flip)]) == -1                                                              # flip not in {0, 2, 3}
    for scale in (0.0, -0.5, math.inf, math.nan):
        assert call([_pass(scale=scale)]) == -1                                                            # scale <= 0 or not finite
    assert call([ok], z=null) == -1                                                                        # NULL z_out
    assert call([ok], na=9) == -1 and call([ok], na=0) == -1                                               # na > OBB_LOSS_MAX_ANCHORS
    for dtype in (2, 4, -1):
        assert call([ok], dtype=dtype) == -1                                                               # unknown dtype
    assert call([ok], a_total=3 * 64 - 1) == -1                                                            # fewer rows than listed
    assert call([ok, _pass(nl=2)], a_total=3 * 64 * 3 - 1) == -1
    assert call([_pass(conv=0)]) == -1                                                                     # a listed level without data
    assert call([_pass(ny=0)]) == -1 and call([_pass(img=(0, 64))]) == -1
    assert call([ok, _pass(flip=7)]) == -1                                                                 # ... in a later pass too
