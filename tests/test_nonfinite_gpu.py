"""GPU: NaN, inf and threshold-edge inputs through the Detect decode, the fused non_max_suppression_obb (decoded z and lazy head)
and the single-list obb_nms, against the restated reference (oracle/pyref.py, oracle.nms_rotated).

What the reference does with such values (utils/general.py:785-835, nms_rotated_wrapper.py:32): torch.max / torch.argmax rank a
NaN of either sign as the maximum (first one wins), so a row whose best class confidence is NaN is dropped (NaN > conf_thres is
false) and a NaN angle bin is the arg-max; torch.min propagates NaN, so a box with one NaN side is never "too small"; a Python
threshold is cast to the tensor dtype before the > comparison.  Special values are written by bit pattern (both NaN signs and a
signalling-pattern NaN) so that no conversion on the way can change them.

Comparison rule: row counts equal, NaN positions equal (any NaN pattern counts as the same NaN), every other value bit-equal, in
the oracle's row order (equal confidences: ascending anchor * nc + class, as tests/test_nms_ties_gpu.py pins it)."""
import os

import numpy as np
import pytest
import torch

import oracle
from oracle import pyref
from tests import synth
from tests.test_lazy_nms_gpu import _detect, _heads, binding  # noqa: F401  (binding: compiled and ctypes bindings)

pytestmark = pytest.mark.gpu

SPECIAL = {  # name: (fp32 bits, fp16 bits)
    "qnan": (0x7FC00000, 0x7E00),
    "nqnan": (0xFFC00000, 0xFE00),
    "snan": (0x7F800001, 0x7C01),
    "inf": (0x7F800000, 0x7C00),
    "ninf": (0xFF800000, 0xFC00),
    "nzero": (0x80000000, 0x8000),
}
NANS = ("qnan", "nqnan", "snan")
NONFINITE = NANS + ("inf", "ninf")
CANON_NAN = 0x7FC00000


def _ibits(dtype, name):
    b = SPECIAL[name][0 if dtype == torch.float32 else 1]
    return int(np.array(b, np.uint32).view(np.int32)) if dtype == torch.float32 else int(np.array(b, np.uint16).view(np.int16))


def _ints(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _put(t, idx, name):
    """t[idx] = the special value `name`, written as its bit pattern."""
    _ints(t)[idx] = _ibits(t.dtype, name)


def _canon(t):
    """(n, 7) output rows as int32 bits of their float32 values, every NaN as one pattern."""
    t = t.detach().cpu().float().contiguous()
    bits = t.view(torch.int32).clone()
    bits[torch.isnan(t)] = CANON_NAN
    return bits


def _cmp(got, ref):
    assert len(got) == len(ref)
    for b, (g, r) in enumerate(zip(got, ref)):
        g, r = _canon(g), _canon(r)
        assert g.shape == r.shape, (b, g.shape, r.shape)
        bad = (g != r).any(1).nonzero()
        assert bad.numel() == 0, (b, int(bad[0]), g[bad[0]].view(torch.float32).tolist(), r[bad[0]].view(torch.float32).tolist())


def _nms(pred, **kw):
    from yolov5_obb_amd.utils.general import non_max_suppression_obb
    return non_max_suppression_obb(pred, **kw)


# ------------------------------------------------------------------------------------------------------ decoded z (user input)
def _plant_z(pred, nc, seed):
    """Special values in passing rows of every image: each listed case gets its own row (objectness 0.9, one strong class)."""
    bs, A, no = pred.shape
    ci = 5 + nc
    g = torch.Generator().manual_seed(seed)
    for b in range(bs):
        rows = iter(torch.randperm(A, generator=g).tolist())

        def row(cls_val=0.95):
            r = next(rows)
            pred[b, r, 4] = 0.9
            pred[b, r, 5:ci] = 0.05
            pred[b, r, 5 + int(torch.randint(0, nc, (1,), generator=g))] = cls_val
            return r

        for col in range(5):                                       # x, y, l, s, obj
            for name in NONFINITE:
                _put(pred, (b, row(), col), name)
        for name in NONFINITE:                                     # a class: the strong one, and another one
            r = row()
            _put(pred, (b, r, 5 + int(pred[b, r, 5:ci].float().argmax())), name)
            _put(pred, (b, row(), 5 + (b + 1) % nc), name)
        for k in (0, 175, 179):                                    # CSL bins (first, inside the last register group, last)
            for name in NONFINITE:
                _put(pred, (b, row(), ci + k), name)
        for name in NANS:                                          # whole-NaN CSL rows: the first bin wins
            _put(pred, (b, row(), slice(ci, no)), name)
        for name in ("qnan", "nqnan"):                             # two NaN bins: the first wins
            r = row()
            _put(pred, (b, r, ci + 40), name)
            _put(pred, (b, r, ci + 20), "qnan" if name == "nqnan" else "nqnan")
        r = row(0.8)                                               # obj = +inf with some class 0: 0 * inf = NaN
        _put(pred, (b, r, 4), "inf")
        pred[b, r, 5 + (b % nc)] = 0.0
        r = row(0.8)                                               # obj = +inf, all classes > 0: conf = inf
        _put(pred, (b, r, 4), "inf")
        pred[b, row(), 2] = -5.0                                   # negative and -0 sizes: too small
        pred[b, row(), 3] = -0.5
        _put(pred, (b, row(), 2), "nzero")
        _put(pred, (b, row(), 3), "nzero")
        for name in ("qnan", "nqnan"):                             # one NaN side: torch.min is NaN, the box is kept
            r = row()
            pred[b, r, 2] = 0.0005
            _put(pred, (b, r, 3), name)
            r = row()
            _put(pred, (b, r, 2), name)
            pred[b, r, 3] = 0.0005
        r = row()                                                  # circles leaving the class window (kImgWide)
        pred[b, r, 0] = -3000.0
        r = row()
        pred[b, r, 2] = 9000.0
    return pred


Z_KWS = [
    dict(conf_thres=0.25, iou_thres=0.45),
    dict(conf_thres=0.25, iou_thres=0.45, agnostic=True),
    dict(conf_thres=0.1, iou_thres=0.45, classes=[0, 1, 5, 39]),
    dict(conf_thres=0.25, iou_thres=0.0),
    dict(conf_thres=0.25, iou_thres=1.0),
]


@pytest.mark.parametrize("multi", [True, False])
@pytest.mark.parametrize("nc", [1, 2, 16, 40])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_z_nonfinite_vs_pyref(dev, oracle_lib, binding, dtype, nc, multi):
    """nc 40 puts classes both in the two register groups and in the on-demand fetch of k_decode (kDecClsRegs)."""
    pred = _plant_z(synth.s_pred(2, 3000, nc, seed=500 + nc, fg_frac=0.03, dtype=dtype), nc, seed=nc)
    for kw in Z_KWS:
        kw = dict(kw, multi_label=multi, max_det=300)
        ref = pyref.non_max_suppression_obb(pred.clone(), **kw)
        assert sum(int(r.shape[0]) for r in ref) > 20
        _cmp(_nms(pred.to(dev), **kw), ref)


def test_z_nonfinite_bs16_full_size(dev, oracle_lib):
    """One batch at the flagship size: bs 16 x 64512 anchors, fp16."""
    nc = 16
    pred = torch.cat([synth.s_pred(1, 64512, nc, seed=600 + b, dtype=torch.float16) for b in range(16)])
    pred = _plant_z(pred, nc, seed=7)
    for multi in (True, False):
        kw = dict(conf_thres=0.25, iou_thres=0.45, multi_label=multi, max_det=300)
        ref = pyref.non_max_suppression_obb(pred.clone(), **kw)
        _cmp(_nms(pred.to(dev), **kw), ref)


# ------------------------------------------------------------------------------------------------------------ threshold edges
def _step(v, dtype, up):
    """The neighbour of the dtype value v (a 0-d tensor of that dtype) one ulp up or down."""
    t = v.clone().reshape(1)
    i = _ints(t)
    if float(t) == 0.0:
        i[0] = 1 if up else -(2 ** 31) + 1 if dtype == torch.float32 else -(2 ** 15) + 1
    elif (float(t) > 0) == up:
        i[0] += 1
    else:
        i[0] -= 1
    return t[0]


@pytest.mark.parametrize("multi", [True, False])
@pytest.mark.parametrize("conf", [0.25, 0.001, 0.3, 0.45, 0.0, 1.0])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_threshold_edges_vs_pyref(dev, oracle_lib, dtype, conf, multi):
    """obj and obj * cls equal to conf_thres as stored in the dtype, one ulp below and above (only the value above passes);
    first-maximum ties between classes, CSL bins and +0 / -0.  Boxes sit apart, so NMS keeps every candidate."""
    nc, A = 4, 256
    ci = 5 + nc
    pred = torch.zeros(1, A, ci + 180, dtype=dtype)
    i = torch.arange(A)
    pred[0, :, 0] = (50 + 80 * (i % 16)).to(dtype)
    pred[0, :, 1] = (50 + 80 * (i // 16)).to(dtype)
    pred[0, :, 2], pred[0, :, 3] = 30.0, 20.0
    pred[0, :, 4] = -1.0                                            # every row not listed below fails the objectness filter
    pred[0, :, 5:ci] = 0.0
    pred[0, :, ci:] = torch.linspace(-0.9, -0.1, 180).to(dtype)     # CSL arg-max: the last bin unless a row says otherwise
    t = torch.tensor(conf, dtype=dtype)
    edges = [_step(t, dtype, False), t, _step(t, dtype, True)]
    half = [(e.float() * 0.5).to(dtype) for e in edges]
    obj_pass = torch.tensor(float("inf") if conf == 1.0 else 1.0, dtype=dtype)
    r = 0
    for e in edges:                                                 # obj at the edge, cls = 1: conf = obj
        pred[0, r, 4], pred[0, r, 5 + r % nc] = e, 1.0
        r += 1
    for e in edges:                                                 # cls at the edge, obj = 1 (+inf at conf 1.0)
        pred[0, r, 4], pred[0, r, 5 + r % nc] = obj_pass, e
        r += 1
    for e in edges:                                                 # obj = 2 x the edge, cls = 0.5: the product is the edge
        pred[0, r, 4], pred[0, r, 5 + r % nc] = (e.float() * 2).to(dtype), 0.5
        r += 1
    for e in half:                                                  # obj = 0.5 x the edge, cls = 2
        pred[0, r, 4], pred[0, r, 5 + r % nc] = e, 2.0
        r += 1
    big = torch.tensor(1e4, dtype=dtype)
    pred[0, r, 4] = big                                             # equal best classes: the first one
    pred[0, r, 5 + 1] = pred[0, r, 5 + 3] = 0.75
    r += 1
    pred[0, r, 4] = big
    pred[0, r, 5:ci] = 0.5
    r += 1
    pred[0, r, 4], pred[0, r, 5 + 2] = big, 0.6                     # equal CSL bins: the first one
    pred[0, r, ci + 33] = pred[0, r, ci + 150] = 0.9
    r += 1
    for lo, hi in (("nzero", None), (None, "nzero")):               # +0 against -0 in the CSL: equal, the first one wins
        pred[0, r, 4], pred[0, r, 5] = big, 0.6
        pred[0, r, ci:] = -1.0
        pred[0, r, ci + 60] = 0.0
        pred[0, r, ci + 120] = 0.0
        if lo:
            _put(pred, (0, r, ci + 60), lo)
        if hi:
            _put(pred, (0, r, ci + 120), hi)
        r += 1
    if conf == 0.0:                                                 # conf = -0 * obj and +0 * obj: neither passes
        pred[0, r, 4] = 1.0
        _put(pred, (0, r, 5), "nzero")
        r += 1
    for agnostic in (False, True):
        kw = dict(conf_thres=conf, iou_thres=0.45, multi_label=multi, agnostic=agnostic, max_det=300)
        ref = pyref.non_max_suppression_obb(pred.clone(), **kw)
        assert int(ref[0].shape[0]) >= 4
        _cmp(_nms(pred.to(dev), **kw), ref)


# ----------------------------------------------------------------------------------------------- Detect decode of the conv outputs
VEC_SHAPES = [(64, 64), (32, 32), (16, 16)]      # 16-byte aligned maps: vector loads
ODD_SHAPES = [(13, 13), (7, 7), (5, 5)]          # element-wise loads


def _plant_heads(heads, dtype, seed, per=6):
    """Special conv outputs at random positions of every channel kind (box, obj, class, CSL): +-inf, both NaN signs, a
    signalling-pattern NaN, +-65504 (the fp16 maximum) and logits in (-104, -87), where the fp32 sigmoid is subnormal."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for h in heads:
        h = h.cpu().clone()
        bs, C, ny, nx = h.shape
        flat = h.view(-1)
        n = flat.numel()
        for name in NONFINITE:
            idx = torch.randint(0, n, (per * bs,), generator=g)
            _put(flat, idx, name)
        for v in (65504.0, -65504.0):
            flat[torch.randint(0, n, (per * bs,), generator=g)] = v
        idx = torch.randint(0, n, (4 * per * bs,), generator=g)
        flat[idx] = (-104.0 + 17.0 * torch.rand(idx.numel(), generator=g)).to(dtype)
        out.append(h)
    return out


def _plant_passing(heads, nc, seed, na=3, per=8):
    """A third of the positions above the objectness threshold, and special values in the channels of passing positions: box,
    objectness, one class, CSL bins 0 / 175 / 179 / any."""
    g = torch.Generator().manual_seed(seed)
    no = 5 + nc + 180
    out = []
    for h in heads:
        bs, C, ny, nx = h.shape
        v = h.view(bs, na, no, ny, nx)
        m = torch.rand(bs, na, ny, nx, generator=g) < 0.3
        v[:, :, 4][m] = (1.0 + torch.rand(int(m.sum()), generator=g)).to(h.dtype)
        cells = m.nonzero()
        for name in NONFINITE + ("max", "nmax"):
            pick = cells[torch.randint(0, cells.shape[0], (per * bs,), generator=g)]
            for k, (b, a, y, x) in enumerate(pick.tolist()):
                ch = [k % 5, 5 + k % nc, 5 + nc, 5 + nc + 175, 5 + nc + 179, 5 + nc + (7 * k) % 180][k % 6]
                if name in ("max", "nmax"):
                    v[b, a, ch, y, x] = 65504.0 if name == "max" else -65504.0
                else:
                    _put(v, (b, a, ch, y, x), name)
        out.append(h)
    return out


def _torch_decode(det, raw):
    """The reference's own op sequence on the GPU (models/yolo.py:71-79), as tests/test_head_gpu.py::test_detect_inference_fp16."""
    zs = []
    for i, r in enumerate(raw):
        grid, ag = det._make_grid(r.shape[3], r.shape[2], i)
        y = r.sigmoid()
        y[..., 0:2] = (y[..., 0:2] * 2 - 0.5 + grid) * det.stride[i]
        y[..., 2:4] = (y[..., 2:4] * 2) ** 2 * ag
        zs.append(y.view(r.shape[0], -1, det.no))
    return torch.cat(zs, 1)


def _close(z, ref):
    """NaN and inf positions equal (infs of the same sign); elsewhere tests/test_head_gpu.py's rule for the dtype."""
    assert z.dtype == ref.dtype and z.shape == ref.shape
    half = z.dtype == torch.float16
    z, ref = z.float(), ref.float()
    assert torch.equal(torch.isnan(z), torch.isnan(ref)), int((torch.isnan(z) != torch.isnan(ref)).sum())
    inf = torch.isinf(z) | torch.isinf(ref)
    assert torch.equal(z[inf], ref[inf])
    ok = ~(torch.isnan(ref) | inf)
    d, r = (z[ok] - ref[ok]).abs(), ref[ok].abs()
    if half:
        ulp = torch.clamp(r * 2 ** -10, min=2.0 ** -24)
        assert (d <= ulp * 1.01).all(), (d / ulp).max()
    else:
        assert (d <= 1e-6 + 2e-6 * r).all(), d.max()


def _same_bits(a, b):
    assert a.shape == b.shape and a.dtype == b.dtype
    assert torch.equal(_ints(a.contiguous()), _ints(b.contiguous()))


@pytest.mark.parametrize("shapes", [VEC_SHAPES, ODD_SHAPES], ids=["vector", "elementwise"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_detect_decode_nonfinite(dev, dtype, shapes):
    """Fused-levels launch, per-level launches and a lazy materialize() against torch's op sequence; the permuted raw heads
    are copies, bit for bit (NaN payloads included)."""
    nc, bs = 16, 2
    det = _detect(nc, 3, dev, dtype)
    heads = [h.to(dev) for h in _plant_heads(_heads(bs, nc, shapes, seed=11, dev="cpu", dtype=dtype), dtype, seed=12)]
    with torch.no_grad():
        raw = [h.view(bs, det.na, det.no, h.shape[2], h.shape[3]).permute(0, 1, 3, 4, 2).contiguous() for h in heads]
        ref = _torch_decode(det, raw)
        assert torch.isnan(ref).any()
        for fused in (True, False):
            det.fused_levels = fused
            try:
                z, xs = det(list(heads))
            finally:
                det.fused_levels = True
            _close(z, ref)
            for a, b in zip(xs, raw):
                _same_bits(a, b)
        det.lazy_nms = True
        try:
            z, xs = det(list(heads))
        finally:
            det.lazy_nms = False
        assert not z.is_materialized()
        _close(z.materialize(), ref)
        for a, b in zip(xs, raw):
            _same_bits(a.materialize() if hasattr(a, "materialize") else a, b)


# ---------------------------------------------------------------------------------------------------------------- lazy head
def _run(det, heads, lazy, couple, **kw):
    det.lazy_nms, det.couple_nms = lazy, couple
    try:
        with torch.no_grad():
            z, _ = det(list(heads))
            out = _nms(z, **kw)
    finally:
        det.lazy_nms, det.couple_nms = False, True
    return z, out


@pytest.mark.parametrize("kw", [
    dict(conf_thres=0.25, iou_thres=0.45, multi_label=True, max_det=300),
    dict(conf_thres=0.25, iou_thres=0.45, multi_label=False, max_det=1500),
    dict(conf_thres=0.001, iou_thres=0.2, multi_label=False, agnostic=True, max_det=300),
    dict(conf_thres=0.1, iou_thres=0.45, multi_label=True, classes=[0, 3, 7], max_det=300),
], ids=["multi", "best", "best_agnostic", "classes"])
@pytest.mark.parametrize("shapes", [VEC_SHAPES, ODD_SHAPES], ids=["vector", "elementwise"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_lazy_head_nonfinite(dev, oracle_lib, binding, dtype, shapes, kw):
    """The fused NMS that reads the conv outputs (k_decode_head) == the eager chain (k_decode on z, with and without the
    objectness column) == the reference chain run on the eager z."""
    nc, bs = 16, 2
    det = _detect(nc, 3, dev, dtype)
    heads = _plant_passing(_heads(bs, nc, shapes, seed=21, dev="cpu", dtype=dtype), nc, seed=22)
    heads = [h.to(dev) for h in _plant_heads(heads, dtype, seed=23)]
    z_eager, eager = _run(det, heads, False, True, **kw)
    _, plain = _run(det, heads, False, False, **kw)
    z, lazy = _run(det, heads, True, True, **kw)
    assert not z.is_materialized(), "the fused entry did not run"
    _cmp(lazy, eager)
    _cmp(plain, eager)
    ref = pyref.non_max_suppression_obb(z_eager.cpu(), **kw)
    assert sum(int(r.shape[0]) for r in ref) >= 5
    _cmp(eager, ref)


# ------------------------------------------------------------------------------------------------------ single-list obb_nms
def _ref_obb_nms(dets, scores, thr):
    """nms_rotated_wrapper.py:32-39 in the tensor's dtype (numpy's min propagates NaN like torch.min), oracle NMS."""
    d, s = dets.numpy(), scores.numpy()
    ok = ~(d[:, 2:4].min(1) < (np.float32(0.001) if d.dtype == np.float32 else 0.001))
    idx = np.nonzero(ok)[0]
    return idx[oracle.nms_rotated(d[ok], s[ok], thr, threads=min(os.cpu_count() or 1, 32))]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("n", [3000, 24000], ids=["small", "indexed"])
def test_obb_nms_one_nan_side(dev, oracle_lib, dtype, n):
    """(l, s) = (0.0005, NaN) and (NaN, 0.0005) among ordinary boxes: torch.min is NaN, so neither box is dropped;
    (0.0005, 30) is.  n = 24000 takes the indexed cross phase (tests/test_nms_gpu.py::test_index_path_with_degenerate_boxes)."""
    from yolov5_obb_amd.utils.nms_rotated import obb_nms
    dets, scores = synth.s_uniform(n, 31, extent=2048.0) if n > 8192 else synth.s_clustered(n, 50, 31)
    dets, scores = dets.to(dtype), synth.tie_free(scores).to(dtype)
    g = torch.Generator().manual_seed(32)
    pick = torch.randperm(n, generator=g)
    def nan_side(idx, col, name):
        if dtype == torch.float32:
            _put(dets, (idx, col), name)
        else:
            dets[idx, col] = float("nan") if name == "qnan" else -float("nan")

    for k, name in enumerate(("qnan", "nqnan")):
        a, b = pick[40 * k:40 * k + 20], pick[40 * k + 20:40 * k + 40]
        dets[a, 2] = 0.0005
        nan_side(a, 3, name)
        nan_side(b, 2, name)
        dets[b, 3] = 0.0005
    dets[pick[100:120], 2] = 0.0005                                  # finite and too small: dropped
    ref = _ref_obb_nms(dets, scores, 0.4)
    if dtype == torch.float32 and n < 8192:
        assert np.array_equal(pyref.obb_nms(dets, scores, 0.4).numpy(), ref)
    assert np.isin(pick[:80].numpy(), ref).any() and not np.isin(pick[100:120].numpy(), ref).any()
    for _ in range(2):
        _, inds = obb_nms(dets.to(dev), scores.to(dev), 0.4)
        assert np.array_equal(inds.cpu().numpy(), ref), (len(ref), int(inds.numel()))
