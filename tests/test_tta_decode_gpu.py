"""GPU: fused augmented inference (obb_detect_decode_tta, models.yolo.forward_augment) against the chain it replaces, on raw bits.

The oracle is the eager path on the same device: this package's Detect per pass (its public forward, the 1x1 convs replaced by
identities so that the test hands it the conv outputs), then the reference's tail restated with plain torch ops -- the in-place
`/=` with the Python float, `img - p[..., k]`, the row-count clip, torch.cat.  The decode arithmetic is shared and the tail's
rounding points are torch's own, so there is no tolerance: tensors are compared as int16 / int32.
The conv outputs are seeded N(0, 1) * 2 tensors (bs, na * no, ny, nx); no backbone is needed.
"""
import pytest
import torch
import torch.nn as nn

from tests import synth

pytestmark = pytest.mark.gpu

SCALES = (1, 0.83, 0.67)
FLIPS = ((None, 3, None), (2, None, 3))
# name -> (nc, anchors, strides, (img_h, img_w), bs, maps per pass)
CASES = {
    # HW = 256 takes the vector path, HW = 9 (and every entry behind an odd row offset) the element-wise one; two images
    "nc3_128": (3, synth.DEFAULT_ANCHORS, synth.DEFAULT_STRIDES, (128, 128), 2,
                [[(16, 16), (8, 8), (4, 4)], [(16, 16), (8, 8), (4, 4)], [(12, 12), (6, 6), (3, 3)]]),
    # non-square: 160 x 96 scales to 160 x 96 (0.83) and 128 x 96 (0.67) at gs = 32
    "nc16_160x96": (16, synth.DEFAULT_ANCHORS, synth.DEFAULT_STRIDES, (160, 96), 1,
                    [[(20, 12), (10, 6), (5, 3)], [(20, 12), (10, 6), (5, 3)], [(16, 12), (8, 6), (4, 3)]]),
    # four levels at strides 8 .. 64: gs = 64 pads every pass of a 128 x 128 input back to 128
    "nl4_128": (3, synth.P6_ANCHORS, synth.P6_STRIDES, (128, 128), 1, [[(16, 16), (8, 8), (4, 4), (2, 2)]] * 3),
}
DTYPES = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}


def bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def make_detect(case, dev, dtype):
    from yolov5_obb_amd.models.yolo import Detect
    nc, anchors, strides = CASES[case][:3]
    det = Detect(nc=nc, anchors=anchors, ch=(1,) * len(anchors))
    det.stride = torch.tensor(strides)
    det.anchors /= det.stride.view(-1, 1, 1)
    det.m = nn.ModuleList(nn.Identity() for _ in anchors)          # forward() is handed the conv outputs
    return det.to(dev).to(dtype).eval()


def make_convs(case, dev, dtype, seed=0):
    nc, anchors, _, _, bs, maps = CASES[case]
    g = torch.Generator().manual_seed(seed)
    no, na = nc + 185, len(anchors[0]) // 2
    return [[(torch.randn(bs, na * no, ny, nx, generator=g) * 2).to(dtype).to(dev) for ny, nx in level] for level in maps]


def chain(det, convs, scales, flips, img):
    """The parent's augmented inference on the same conv outputs: eager Detect, then the reference's torch ops."""
    y = []
    for cs, s, f in zip(convs, scales, flips):
        p = det(list(cs))[0]
        p[..., :4] /= s
        if f == 2:
            p[..., 1] = img[0] - p[..., 1]
        elif f == 3:
            p[..., 0] = img[1] - p[..., 0]
        y.append(p)
    g = sum(4 ** k for k in range(det.nl))
    i = y[0].shape[1] // g
    y[0] = y[0][:, :-i]
    i = (y[-1].shape[1] // g) * 4 ** (det.nl - 1)
    y[-1] = y[-1][:, i:]
    return torch.cat(y, 1)


def fused(det, convs, scales, flips, img):
    from yolov5_obb_amd.models.yolo import _decode_tta, tta_plan
    plan = tta_plan([[tuple(c.shape[2:]) for c in cs] for cs in convs], det.na, det.nl)
    assert plan.on_boundary
    return _decode_tta(det, convs, plan, scales, flips, img[0], img[1]), plan


_memo = {}


def both(case, dt, flips, dev):
    """(oracle, fused z, plan) of a case, computed once and shared (read-only) by the tests."""
    key = (case, dt, flips)
    if key not in _memo:
        det = make_detect(case, dev, DTYPES[dt])
        convs = make_convs(case, dev, DTYPES[dt])
        img = CASES[case][3]
        with torch.no_grad():
            want = chain(det, convs, SCALES, flips, img)
            got, plan = fused(det, convs, SCALES, flips, img)
        _memo[key] = (want, got, plan)
    return _memo[key]


@pytest.mark.parametrize("flips", FLIPS, ids=["lr_mid", "ud_first_lr_last"])
@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("dt", list(DTYPES))
def test_fused_equals_the_chain_bit_for_bit(dev, dt, case, flips):
    want, got, plan = both(case, dt, flips, dev)
    assert got.shape == want.shape == (CASES[case][4], plan.a_total, CASES[case][0] + 185) and got.dtype == want.dtype
    assert torch.equal(bits(got), bits(want)), (bits(got) != bits(want)).nonzero()[:8].tolist()
    col, version = got._obb_objcol
    assert version == got._version and col.shape == got.shape[:2] and col.is_contiguous()
    assert torch.equal(bits(col), bits(got[..., 4]))


def test_division_formula_is_pinned(dev):
    """`p[..., :4] /= 0.83` on the device: a true division and a multiplication with the reciprocal give different bits on this
    input (else the input could not tell them apart), and the fused output carries the bits of torch's in-place op."""
    case, s = "nc3_128", 0.83
    det = make_detect(case, dev, torch.float32)
    convs = make_convs(case, dev, torch.float32)
    with torch.no_grad():
        p = det(list(convs[1]))[0][..., :4].contiguous()
        divided = p / torch.tensor(s, device=dev)                               # a device divisor: an element-wise division
        times_py = p * (1 / s)                                                  # the reciprocal taken in double by Python
        inv32 = float(torch.tensor(1.0) / torch.tensor(s))                      # ... and in fp32 (IEEE, on the host)
        times_f32 = p * inv32
        inplace = p.clone()
        inplace /= s
    assert not torch.equal(bits(divided), bits(times_py)), "the input cannot tell a division from a multiplication: enlarge it"
    matched = [n for n, t in (("divide", divided), ("multiply by double 1/s", times_py), ("multiply by fp32 1/s", times_f32))
               if torch.equal(bits(t), bits(inplace))]
    print("torch's in-place `/= 0.83` equals:", matched)
    want, got, plan = both(case, "fp32", FLIPS[0], dev)
    lo = plan.passes[1].offsets[0]
    assert torch.equal(bits(got[:, lo:lo + plan.passes[1].rows, 1:4]), bits(inplace[..., 1:4]))      # (channel 0 is de-flipped)
    assert torch.equal(bits(got), bits(want))


@pytest.mark.parametrize("dt", list(DTYPES))
def test_scale_whose_two_reciprocals_differ(dev, dt):
    """0.83 and 0.67 cannot tell WHICH reciprocal torch multiplies with: float(1 / s) taken in double and 1.0f / float(s) are the
    same float for both.  For s = 0.85 they differ by one ulp (1.1764706 / 1.1764705), and the fused output still equals the chain
    (torch takes the reciprocal in double and rounds it to fp32; a kernel that takes it in fp32 fails here in fp32)."""
    s = 0.85
    assert float(torch.tensor(1 / s)) != float(torch.tensor(1.0) / torch.tensor(s))
    case = "nc3_128"
    det = make_detect(case, dev, DTYPES[dt])
    convs = make_convs(case, dev, DTYPES[dt], seed=4)
    scales, flips = (1, s, s), (None, 2, 3)
    with torch.no_grad():
        want = chain(det, convs, scales, flips, CASES[case][3])
        got, _ = fused(det, convs, scales, flips, CASES[case][3])
        if dt == "fp32":
            p = det(list(convs[1]))[0][..., :4].contiguous()
            inplace = p.clone()
            inplace /= s
            which = [n for n, t in (("double 1/s", p * (1 / s)), ("fp32 1/s", p * float(torch.tensor(1.0) / torch.tensor(s))))
                     if torch.equal(bits(t), bits(inplace))]
            print("torch's in-place `/= 0.85` equals the multiplication with:", which)
    assert torch.equal(bits(got), bits(want)), (bits(got) != bits(want)).nonzero()[:8].tolist()


def test_nms_agrees_and_reads_the_column(dev):
    from yolov5_obb_amd.utils.general import _objectness_column, non_max_suppression_obb
    want, got, _ = both("nc16_160x96", "fp16", FLIPS[0], dev)
    kw = dict(conf_thres=0.25, iou_thres=0.4, multi_label=True)
    a, b = non_max_suppression_obb(want, **kw), non_max_suppression_obb(got, **kw)
    assert not hasattr(want, "_obb_objcol") and _objectness_column(got, got) is got._obb_objcol[0]
    assert len(a) == len(b) and sum(len(t) for t in a) > 0
    for ta, tb in zip(a, b):
        assert torch.equal(ta, tb)
    # an in-place edit of a fused tensor (a fresh one: the shared tensors stay as they are): the column is stale and is ignored
    det = make_detect("nc16_160x96", dev, torch.float16)
    with torch.no_grad():
        edited, _ = fused(det, make_convs("nc16_160x96", dev, torch.float16), SCALES, FLIPS[0], CASES["nc16_160x96"][3])
    assert torch.equal(bits(edited), bits(got)) and _objectness_column(edited, edited) is not None
    edited[:, ::3, 4] = 0
    assert _objectness_column(edited, edited) is None
    plain = edited.clone()
    c, d = non_max_suppression_obb(edited, **kw), non_max_suppression_obb(plain, **kw)
    assert len(c) == len(d) and all(torch.equal(tc, td) for tc, td in zip(c, d))
    assert any(not torch.equal(tb, tc) for tb, tc in zip(b, c))     # (the edit was one the NMS sees)


class StandIn(nn.Module):
    """A model as forward_augment sees one: strided average pools and 1x1 convs for the stride-8 / 16 / 32 maps, this package's
    Detect, `_forward_once`, `stride` and `inplace`."""

    def __init__(self, nc=3, ceil_mode=False, seed=1):
        from yolov5_obb_amd.models.yolo import Detect
        super().__init__()
        torch.manual_seed(seed)
        ch = (4, 6, 8)
        self.pools = nn.ModuleList(nn.AvgPool2d(s, s, ceil_mode=ceil_mode) for s in (8, 16, 32))
        self.convs = nn.ModuleList(nn.Conv2d(3, c, 1) for c in ch)
        det = Detect(nc=nc, anchors=synth.DEFAULT_ANCHORS, ch=ch)
        det.stride = torch.tensor(synth.DEFAULT_STRIDES)
        det.anchors /= det.stride.view(-1, 1, 1)
        for m in det.m:                                             # spread the logits: objectness on both sides of the threshold
            nn.init.normal_(m.weight, std=1.0)
        self.model = nn.ModuleList([det])
        self.stride = det.stride
        self.inplace = True

    def _forward_once(self, x):
        return self.model[-1]([conv(pool(x)) for pool, conv in zip(self.pools, self.convs)])


def _augment(model, x, fused_tta):
    from yolov5_obb_amd.models.yolo import forward_augment
    model.model[-1].fused_tta = fused_tta
    return forward_augment(model, x)


def test_forward_augment_fused_equals_unfused(dev, monkeypatch):
    from yolov5_obb_amd.models.yolo import tta_plan
    model = StandIn().to(dev).half().eval()
    x = torch.rand(2, 3, 128, 128, generator=torch.Generator().manual_seed(2)).to(dev).half()
    a_total = tta_plan([[(16, 16), (8, 8), (4, 4)]] * 2 + [[(12, 12), (6, 6), (3, 3)]], 3, 3).a_total
    cats = []
    real_cat = torch.cat
    monkeypatch.setattr(torch, "cat", lambda *a, **k: (cats.append(1), real_cat(*a, **k))[1])
    with torch.no_grad():
        want, none_a = _augment(model, x, False)
        n_chain = len(cats)
        got, none_b = _augment(model, x, True)
    assert none_a is None and none_b is None and n_chain >= 1 and len(cats) == n_chain       # no torch.cat in the fused run
    assert got.shape == want.shape == (2, a_total, 188) and torch.equal(bits(got), bits(want))
    # written once, in its final place: one allocation of exactly a_total rows, with the column on it
    assert got.is_contiguous() and got.storage_offset() == 0 and got.untyped_storage().nbytes() == got.numel() * 2
    assert torch.equal(bits(got._obb_objcol[0]), bits(got[..., 4])) and not hasattr(want, "_obb_objcol")
    assert "_collect" not in vars(model.model[-1])                  # the head is back in its normal mode
    with torch.inference_mode():
        got_i, none_c = _augment(model, x, True)
    assert none_c is None and torch.equal(bits(got_i), bits(want)) and not hasattr(got_i, "_obb_objcol")
    model.model[-1].lazy_nms = True                                 # fused_tta wins over lazy_nms
    with torch.no_grad():
        got_l, _ = _augment(model, x, True)
    assert type(got_l) is torch.Tensor and torch.equal(bits(got_l), bits(want))


def test_forward_augment_falls_back_off_the_level_boundary(dev):
    """Ceil-mode pools on 136 x 136: maps 17 / 9 / 5, the first pass's cut (56 rows) splits its last level (75): the chain runs."""
    model = StandIn(ceil_mode=True).to(dev).half().eval()
    x = torch.rand(1, 3, 136, 136, generator=torch.Generator().manual_seed(3)).to(dev).half()
    with torch.no_grad():
        want, _ = _augment(model, x, False)
        got, none = _augment(model, x, True)
    assert none is None and got.shape == want.shape and got.shape[1] == 1185 - 56 + 3 * 336 + 3 * (36 + 9)
    assert torch.equal(bits(got), bits(want))


def test_side_stream(dev):
    case, dt = "nc3_128", "fp16"
    want, got, _ = both(case, dt, FLIPS[0], dev)
    det = make_detect(case, dev, DTYPES[dt])
    convs = make_convs(case, dev, DTYPES[dt])
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side), torch.no_grad():
        z, _ = fused(det, convs, SCALES, FLIPS[0], CASES[case][3])
        host = z.cpu()                                              # a read on that stream
        col = z._obb_objcol[0].cpu()
    side.synchronize()
    assert torch.equal(bits(host), bits(got.cpu())) and torch.equal(bits(col), bits(got[..., 4].cpu()))
