"""GPU parity of the Detect inference decode, the CSL encode and rbox2poly / poly2hbb kernels (csrc/head.hip)
against the CPU oracle (oracle/pyref.py, pinned to the reference's models/yolo.py and utils/rboxs_utils.py) and
against the fixtures frozen from the reference itself (tests/golden).

Tolerances: the permuted raw head is a copy -> bit-exact.  Decoded values go through sigmoid/exp, whose last bit
differs between libm implementations: fp32 within 2e-6 relative (north_star: 1e-5), fp16 within one fp16 ulp."""
import os

import numpy as np
import pytest
import torch

from oracle import pyref
from tests import synth

pytestmark = pytest.mark.gpu
G = np.load(os.path.join(os.path.dirname(__file__), "golden", "reference_outputs.npz"))


def make_detect(nc, ch, dev, dtype=torch.float32, seed=0):
    from yolov5_obb_amd.models.yolo import Detect
    torch.manual_seed(seed)
    det = Detect(nc=nc, anchors=synth.DEFAULT_ANCHORS, ch=ch)
    det.stride = torch.tensor(synth.DEFAULT_STRIDES)
    det.anchors /= det.stride.view(-1, 1, 1)
    return det.to(dev).to(dtype).eval()


@pytest.mark.parametrize("nc,sizes,bs", [(3, (16, 8, 4), 2), (16, (40, 20, 10), 3), (15, (13, 7, 5), 1), (18, (128, 64, 32), 2)])
def test_detect_inference_matches_oracle_fp32(dev, nc, sizes, bs):
    ch = (8, 16, 32)
    det = make_detect(nc, ch, dev)
    feats = [torch.randn(bs, c, s, s + (i % 2)) for i, (c, s) in enumerate(zip(ch, sizes))]     # non-square maps too
    with torch.no_grad():
        z, xs = det([f.to(dev) for f in feats])
        convs = [det.m[i](feats[i].to(dev)) for i in range(3)]
    raw = [c.view(bs, det.na, det.no, c.shape[2], c.shape[3]).permute(0, 1, 3, 4, 2).contiguous() for c in convs]
    for a, b in zip(xs, raw):
        assert torch.equal(a, b)                                  # the permuted raw head is bit-exact
    ref = pyref.detect_decode([r.cpu() for r in raw], det.anchors.cpu(), det.stride)
    assert z.shape == ref.shape
    assert torch.allclose(z.cpu(), ref, rtol=2e-6, atol=1e-6), (z.cpu() - ref).abs().max()


def test_detect_golden_fixture_from_reference_module(dev):
    raw = [torch.from_numpy(G[f"detect_raw{i}"]) for i in range(3)]
    from yolov5_obb_amd import _lib
    import ctypes as C
    bs, na, _, _, no = raw[0].shape
    a_total = sum(r.shape[1] * r.shape[2] * r.shape[3] for r in raw)
    z = torch.empty((bs, a_total, no), device=dev)
    off = 0
    for i, r in enumerate(raw):
        conv = r.permute(0, 1, 4, 2, 3).contiguous().view(bs, na * no, r.shape[2], r.shape[3]).to(dev)   # back to the conv layout
        px = (synth.grid_anchors()[i] * synth.DEFAULT_STRIDES[i]).reshape(-1).tolist()
        arr = (C.c_float * len(px))(*px)
        xp = torch.empty(r.shape, device=dev)
        rc = _lib.lib().obb_detect_decode(_lib.ptr(conv), 0, bs, na, no, r.shape[2], r.shape[3], C.cast(arr, C.c_void_p),
                                          synth.DEFAULT_STRIDES[i], _lib.ptr(xp), _lib.ptr(z), a_total, off, _lib.stream_ptr(dev))
        assert rc == 0
        assert torch.equal(xp.cpu(), r)
        off += na * r.shape[2] * r.shape[3]
    assert np.allclose(z.cpu().numpy(), G["detect_z"], rtol=2e-6, atol=1e-6)


def test_detect_inference_fp16(dev):
    det = make_detect(16, (8, 16, 32), dev, torch.float16)
    feats = [torch.randn(2, c, s, s).half() for c, s in zip((8, 16, 32), (32, 16, 8))]
    with torch.no_grad():
        z, xs = det([f.to(dev) for f in feats])
        convs = [det.m[i](feats[i].to(dev)) for i in range(3)]
        raw = [c.view(2, det.na, det.no, c.shape[2], c.shape[3]).permute(0, 1, 3, 4, 2).contiguous() for c in convs]
        # the reference's own op sequence on the GPU in fp16 (models/yolo.py:71-79)
        zs = []
        for i, r in enumerate(raw):
            grid, ag = det._make_grid(r.shape[3], r.shape[2], i)
            y = r.sigmoid()
            y[..., 0:2] = (y[..., 0:2] * 2 - 0.5 + grid) * det.stride[i]
            y[..., 2:4] = (y[..., 2:4] * 2) ** 2 * ag
            zs.append(y.view(2, -1, det.no))
        ref = torch.cat(zs, 1)
    for a, b in zip(xs, raw):
        assert torch.equal(a, b)
    assert z.dtype == torch.float16
    d = (z.float() - ref.float()).abs()
    ulp = torch.maximum(ref.float().abs() * 2 ** -10, torch.tensor(2.0 ** -24, device=dev))
    assert (d <= ulp * 1.01).all(), (d / ulp).max()
    assert (d == 0).float().mean() > 0.98


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("nc,sizes,bs", [(16, (40, 20, 10), 3), (15, (13, 7, 5), 1), (15, (128, 64, 32), 2)])
def test_detect_all_levels_in_one_launch_same_bytes(dev, dtype, nc, sizes, bs):
    """obb_detect_decode_levels (the default of Detect.forward) writes the same z, objectness column and permuted heads as one
    obb_detect_decode_col call per level -- vector and element-wise paths (13 x 14 maps are not 16-byte aligned), both dtypes."""
    ch = (8, 16, 32)
    det = make_detect(nc, ch, dev, dtype)
    feats = [torch.randn(bs, c, s, s + (i % 2)).to(dtype).to(dev) for i, (c, s) in enumerate(zip(ch, sizes))]
    outs = []
    with torch.no_grad():
        for fused in (True, False):
            det.fused_levels = fused
            z, xs = det(list(feats))
            outs.append((z, z._obb_objcol[0], xs))
    (z1, c1, x1), (z0, c0, x0) = outs
    assert torch.equal(z1, z0) and torch.equal(c1, c0) and torch.equal(c1, z1[..., 4])
    assert all(torch.equal(a, b) for a, b in zip(x1, x0))


def test_detect_rejects_cpu_inference_but_trains_on_cpu():
    from yolov5_obb_amd.models.yolo import Detect
    det = Detect(nc=3, anchors=synth.DEFAULT_ANCHORS, ch=(4, 4, 4))
    det.stride = torch.tensor(synth.DEFAULT_STRIDES)
    out = det([torch.zeros(1, 4, 8, 8), torch.zeros(1, 4, 4, 4), torch.zeros(1, 4, 2, 2)])     # training branch: plain torch
    assert [tuple(o.shape) for o in out] == [(1, 3, 8, 8, 188), (1, 3, 4, 4, 188), (1, 3, 2, 2, 188)]
    det.eval()
    with pytest.raises(RuntimeError):
        det([torch.zeros(1, 4, 8, 8), torch.zeros(1, 4, 4, 4), torch.zeros(1, 4, 2, 2)])


def test_csl_encode_matches_numpy_reference(dev):
    from yolov5_obb_amd.utils.rboxs_utils import csl_encode, gaussian_label_cpu
    ang = np.concatenate([G["csl_angles"], np.random.default_rng(0).uniform(0, 180, 500), [179.999, 0.0, 90.0, 180.0, 200.0, -5.0, 400.0]])
    for sig in (2.0, 4.0, 6.0):
        got = csl_encode(torch.from_numpy(ang.astype(np.float32)).to(dev), 180, 0.0, sig).cpu().numpy()
        ref = np.stack([pyref.gaussian_label(float(np.float32(a)), 180, 0, sig) for a in ang]).astype(np.float32)
        assert got.shape == ref.shape
        assert np.allclose(got, ref, rtol=1e-6, atol=1e-30), np.abs(got - ref).max()
        assert np.array_equal(got.argmax(1), ref.argmax(1))
        mine = np.stack([gaussian_label_cpu(float(np.float32(a)), 180, 0, sig) for a in ang]).astype(np.float32)
        assert np.array_equal(mine, ref)
    g37 = csl_encode(torch.from_numpy(G["csl_angles"].astype(np.float32)).to(dev), 180, 0.0, 2.0).cpu().numpy()
    ref37 = np.stack([pyref.gaussian_label(float(np.float32(a)), 180, 0, 2.0) for a in G["csl_angles"]])
    assert np.allclose(g37, ref37.astype(np.float32), rtol=1e-6, atol=1e-30)


def test_rbox2poly_and_hbb_match_reference(dev):
    from yolov5_obb_amd.utils.rboxs_utils import rbox2poly, poly2hbb, rbox2hbb
    rb = synth.s_uniform(300, 21)[0]
    poly = rbox2poly(rb.to(dev))
    assert np.allclose(poly.cpu().numpy(), G["rbox2poly_ref"], rtol=1e-6, atol=1e-4)
    hbb = rbox2hbb(rb.to(dev))
    assert np.allclose(hbb.cpu().numpy(), G["poly2hbb_ref"], rtol=1e-6, atol=1e-4)
    assert torch.allclose(poly2hbb(poly), hbb, rtol=0, atol=0)
    big = synth.s_clustered(100000, 300, 1)[0]
    p2 = rbox2poly(big.to(dev)).cpu()
    assert torch.allclose(p2, pyref.rbox2poly(big), rtol=1e-6, atol=2e-4)
    assert rbox2poly(torch.zeros(0, 5, device=dev)).shape == (0, 8)


def _csl_labels(n):
    """Every integer label from -(n + 2) to n + 2, the float32 neighbours of each and the half-way points: int(n/2 - label)
    steps at every one of them, and |n/2 - label| crosses n (the window is then left unrolled) at -n/2 and 3n/2."""
    i = np.arange(-(n + 2), n + 3, dtype=np.float32)
    lab = np.concatenate([i, np.nextafter(i, np.float32(-np.inf)), np.nextafter(i, np.float32(np.inf)), i + np.float32(0.5),
                          np.float32([n, -n, n + 0.5, -(n + 0.5), 1.5 * n, -0.5 * n, 1.5 * n + 1, -0.5 * n - 1])])
    return lab.astype(np.float32)


@pytest.mark.parametrize("sig", [0.5, 6.0])
@pytest.mark.parametrize("u", [0.0, 0.5, -3.0])
@pytest.mark.parametrize("num_class", [1, 2, 90, 181])
def test_csl_encode_window_sizes_offsets_and_widths(dev, num_class, u, sig):
    """obb_csl_encode_f32 away from num_class = 180, u = 0: odd window sizes (n / 2 is no integer), a window of one bin, a shifted
    and a narrow Gaussian, labels on and next to every integer and beyond +-num_class."""
    from yolov5_obb_amd.utils.rboxs_utils import csl_encode
    lab = _csl_labels(num_class)
    got = csl_encode(torch.from_numpy(lab).to(dev), num_class, u, sig).cpu().numpy()
    ref = np.stack([pyref.gaussian_label(float(a), num_class, u, sig) for a in lab]).astype(np.float32)
    assert got.shape == ref.shape == (len(lab), num_class)
    assert np.allclose(got, ref, rtol=1e-6, atol=1e-30), np.abs(got - ref).max()
    assert np.array_equal(got.argmax(1), ref.argmax(1))


def _poly_f64(rb):
    """utils/rboxs_utils.py:106-145 and :147-181 in float64 on the float32 inputs."""
    x, y, w, h, th = (rb[:, k].astype(np.float64) for k in range(5))
    c, s = np.cos(th), np.sin(th)
    v1x, v1y, v2x, v2y = w / 2 * c, -w / 2 * s, -h / 2 * s, -h / 2 * c
    poly = np.stack([x + v1x + v2x, y + v1y + v2y, x + v1x - v2x, y + v1y - v2y, x - v1x - v2x, y - v1y - v2y, x - v1x + v2x, y - v1y + v2y], 1)
    px, py = poly[:, 0::2], poly[:, 1::2]
    hbb = np.stack([(px.max(1) + px.min(1)) / 2, (py.max(1) + py.min(1)) / 2, px.max(1) - px.min(1), py.max(1) - py.min(1)], 1)
    return poly, hbb


@pytest.mark.parametrize("want", ["poly", "hbb"])
@pytest.mark.parametrize("n", [1, 257, 3001])
def test_rbox2poly_row_stride_and_single_outputs(dev, n, want):
    """obb_rbox2poly_f32 through the C ABI on (n, 7) rows (row_stride = 7: the NMS output [x y l s theta conf cls]) with only one
    of the two outputs requested; |theta| up to 4 pi, sides from 1e-3 to 4096.  The output sits between guard bytes.

    Each formula is compared with its float64 evaluation under the file's tolerance: the polygon (utils/rboxs_utils.py:106-145)
    on the boxes, the hull (:147-181) on the float32 polygon it is computed from, as the reference computes it.  The hull of the
    float64 polygon is no reference for that tolerance: a hull extent is the difference of two float32 corners of magnitude up
    to 3000 (half an ulp each: 1.2e-4), measured 1.20 x (1e-4 + 1e-6 |ref|) on a 4096 x 1e-3 box; it is held to twice the
    polygon's tolerance instead."""
    import ctypes as C
    from yolov5_obb_amd import _lib
    rng = np.random.default_rng(100 + n)
    rb = np.zeros((n, 7), np.float32)
    rb[:, 0:2] = rng.uniform(0.0, 1024.0, (n, 2))
    rb[:, 2:4] = np.exp(rng.uniform(np.log(1e-3), np.log(4096.0), (n, 2)))
    rb[:, 4] = rng.uniform(-4 * np.pi, 4 * np.pi, n)
    rb[:, 5:7] = rng.uniform(1e6, 2e6, (n, 2))                       # a kernel reading columns 5, 6 as the next row's x, y shows
    rb[0, 2:5] = (4096.0, 1e-3, 4 * np.pi)
    poly_ref, hbb_ref = _poly_f64(rb)
    width, guard, fill = (8, 64, 0x5A) if want == "poly" else (4, 64, 0x5A)
    raw = torch.full(((2 * guard + n * width) * 4,), fill, dtype=torch.uint8, device=dev)
    out = raw[guard * 4:(guard + n * width) * 4].view(torch.float32)
    d = torch.from_numpy(rb).to(dev)
    with torch.cuda.device(dev):
        rc = _lib.lib().obb_rbox2poly_f32(_lib.ptr(d), n, 7, _lib.ptr(out) if want == "poly" else None, _lib.ptr(out) if want == "hbb" else None,
                                          _lib.stream_ptr(dev))
    assert rc == 0
    torch.cuda.synchronize(dev)
    assert bool((raw[:guard * 4] == fill).all()) and bool((raw[(guard + n * width) * 4:] == fill).all())
    got = out.view(n, width).cpu().numpy().astype(np.float64)
    if want == "poly":
        ref = poly_ref
    else:
        poly = torch.empty((n, 8), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            assert _lib.lib().obb_rbox2poly_f32(_lib.ptr(d), n, 7, _lib.ptr(poly), None, _lib.stream_ptr(dev)) == 0
        p = poly.cpu().numpy().astype(np.float64)
        assert np.allclose(p, poly_ref, rtol=1e-6, atol=1e-4)
        px, py = p[:, 0::2], p[:, 1::2]
        ref = np.stack([(px.max(1) + px.min(1)) / 2, (py.max(1) + py.min(1)) / 2, px.max(1) - px.min(1), py.max(1) - py.min(1)], 1)
        bound = 2.0 * (1e-4 + 1e-6 * np.abs(poly_ref).max(1, keepdims=True))
        assert (np.abs(got - hbb_ref) <= bound).all(), (np.abs(got - hbb_ref) / bound).max()
    err = np.abs(got - ref) / (1e-4 + 1e-6 * np.abs(ref))
    print(f"rbox2poly {want} n={n}: max |got - ref| / (1e-4 + 1e-6 |ref|) = {err.max():.3f}")
    assert np.allclose(got, ref, rtol=1e-6, atol=1e-4), err.max()
    with torch.cuda.device(dev):                                     # neither output: an error, nothing is launched
        assert _lib.lib().obb_rbox2poly_f32(_lib.ptr(d), n, 7, None, None, _lib.stream_ptr(dev)) == -1
        assert _lib.lib().obb_rbox2poly_f32(_lib.ptr(d), n, 4, _lib.ptr(out), None, _lib.stream_ptr(dev)) == -1
