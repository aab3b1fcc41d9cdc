"""GPU: the three Detect decode entries (obb_detect_decode, obb_detect_decode_col, obb_detect_decode_levels), Detect.forward and
the lazy NMS entry (Detect.lazy_nms -> obb_non_max_suppression_obb_head) across the head configurations of tests/head_cases.py:
nl 1..4, na 1..8, nc 1..256, maps from 1 x 1 up, both dtypes.

The reference is independent of the kernels: tests/head_cases.py:decode_ref, numpy float64 from the formula of the reference's
models/yolo.py:71-79 (tests/test_head_configs_host.py ties it to the oracle, to torch's own fp16 op chain and to the reference's
Detect), and oracle/pyref.py for the NMS.  Tolerances are those of tests/test_head_gpu.py: the permuted raw head is a copy
(bit-exact); decoded fp32 values within 1e-6 + 2e-6 |ref|, fp16 values within one fp16 ulp; the objectness column is
z[..., 4] bit for bit; NMS rows are torch.equal."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import pyref
from tests import head_cases as H

pytestmark = pytest.mark.gpu

DTYPES = [pytest.param(torch.float32, id="fp32"), pytest.param(torch.float16, id="fp16")]
OBB_OK, OBB_ERR_BAD_ARG = 0, -1
SENTINEL = 0x5A                      # every guard byte
GUARD = 64                           # guard elements in front of and behind every output (a multiple of 16 bytes)
EXTRA_ROWS = 8                       # a_total - the levels' sum (8 rows are a multiple of 16 bytes for every no: alignment is kept)


@pytest.fixture(params=["compiled", "ctypes"])
def binding(request, monkeypatch):
    from yolov5_obb_amd import _lib
    ext = _lib.compiled()
    assert ext is not None, "nms_rotated_ext_c.so is not built"
    if request.param == "ctypes":
        monkeypatch.setattr(_lib, "_ext", None)
        monkeypatch.setattr(_lib, "_ext_tried", True)
    return request.param


def _code(dtype):
    return 0 if dtype == torch.float32 else 1


def _detect(case, dev, dtype):
    from yolov5_obb_amd.models.yolo import Detect
    det = Detect(nc=case.nc, anchors=H.detect_anchor_arg(case), ch=(8,) * case.nl)
    det.stride = torch.tensor(H.strides(case))
    det.anchors /= det.stride.view(-1, 1, 1)
    det = det.to(dev).to(dtype).eval()
    det.m = torch.nn.ModuleList([torch.nn.Identity() for _ in range(case.nl)])
    return det


def _heads(case, dev, dtype):
    return [c.to(dev) for c in H.convs(case, dtype)]


def _farr(v):
    v = [float(x) for x in np.asarray(v, np.float32).reshape(-1)]
    return (C.c_float * len(v))(*v)


class Buf:
    """An output of `numel` elements inside a larger device buffer filled with the sentinel; `shift` elements off the 16-byte
    alignment torch's allocator gives (GUARD elements are a multiple of 16 bytes)."""

    def __init__(self, numel, dtype, dev, shift=0):
        self.esz = torch.empty(0, dtype=dtype).element_size()
        self.lo = (GUARD + shift) * self.esz
        self.n = numel * self.esz
        self.raw = torch.full((self.lo + self.n + GUARD * self.esz,), SENTINEL, dtype=torch.uint8, device=dev)
        self.t = self.raw[self.lo:self.lo + self.n].view(dtype)
        assert self.raw.data_ptr() % 16 == 0 and self.t.data_ptr() == self.raw.data_ptr() + self.lo

    def guards_intact(self):
        return bool((self.raw[:self.lo] == SENTINEL).all()) and bool((self.raw[self.lo + self.n:] == SENTINEL).all())

    def untouched(self):
        return bool((self.raw == SENTINEL).all())


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def decode_levels(case, heads, dtype, xps, z, a_total, col, nl=None, sizes=None, anchors=None, na=None, no=None):
    """obb_detect_decode_levels on raw pointers (any output may be None)."""
    from yolov5_obb_amd import _lib
    dev = heads[0].device
    nl = case.nl if nl is None else nl
    sizes = case.sizes if sizes is None else sizes
    with torch.cuda.device(dev):
        return _lib.lib().obb_detect_decode_levels(
            nl, (C.c_void_p * max(nl, 1))(*[h.data_ptr() for h in heads[:max(nl, 1)]]), _code(dtype), heads[0].shape[0],
            case.na if na is None else na, case.no if no is None else no,
            (C.c_int64 * len(sizes))(*[s[0] for s in sizes]), (C.c_int64 * len(sizes))(*[s[1] for s in sizes]),
            _farr(H.anchors_px(case) if anchors is None else anchors), _farr(H.strides(case)),
            (C.c_void_p * max(nl, 1))(*[(x.data_ptr() if x is not None else None) for x in xps[:max(nl, 1)]]) if xps is not None else None,
            _ptr(z), a_total, _ptr(col), _lib.stream_ptr(dev))


def decode_one(case, heads, dtype, l, xp, z, a_total, a_off, col, entry="col"):
    """obb_detect_decode_col (or obb_detect_decode, which has no column output) for level l."""
    from yolov5_obb_amd import _lib
    dev = heads[0].device
    ny, nx = case.sizes[l]
    L = _lib.lib()
    args = (_ptr(heads[l]), _code(dtype), heads[l].shape[0], case.na, case.no, ny, nx, C.cast(_farr(H.anchors_px(case)[l]), C.c_void_p),
            H.strides(case)[l], _ptr(xp), _ptr(z), a_total, a_off)
    with torch.cuda.device(dev):
        if entry == "plain":
            assert col is None
            return L.obb_detect_decode(*args, _lib.stream_ptr(dev))
        return L.obb_detect_decode_col(*args, _ptr(col), _lib.stream_ptr(dev))


def _outputs(case, dtype, dev, a_total=None):
    a_total = case.a_total if a_total is None else a_total
    xps = [torch.empty((case.bs, case.na, ny, nx, case.no), dtype=dtype, device=dev) for ny, nx in case.sizes]
    z = torch.empty((case.bs, a_total, case.no), dtype=dtype, device=dev)
    col = torch.empty((case.bs, a_total), dtype=dtype, device=dev)
    return xps, z, col


GPU_BIT_EQUAL = {}


def check_against_ref(case, dtype, xps, z, col, what):
    """Permuted heads bit-equal; z within the dtype's rule; the column bit-equal to z[..., 4]."""
    zr, xr, _ = H.decode_ref(case, None, dtype)
    if xps is not None:
        for l, (x, r) in enumerate(zip(xps, xr)):
            assert x.shape == r.shape and np.array_equal(x.cpu().numpy().view(np.uint8), r.view(np.uint8)), (what, "x_perm", l)
    zc = z.cpu().numpy()
    assert zc.shape == zr.shape and zc.dtype == zr.dtype
    ok = H.close_fp32(zc, zr) if dtype == torch.float32 else H.close_fp16(zc, zr)
    if not ok.all():
        b, r, c = (int(v) for v in np.argwhere(~ok)[0])
        raise AssertionError((what, f"{int((~ok).sum())} of {ok.size} elements of z out of tolerance; first at image {b} row {r} "
                                    f"channel {c}: got {float(zc[b, r, c])!r}, reference {float(zr[b, r, c])!r}"))
    if dtype == torch.float16:
        same = float((zc == zr).mean())
        GPU_BIT_EQUAL[(case.name, what)] = same
        print(f"{case.name} {what}: {same * 100:.4f} % of {zc.size} fp16 elements bit-equal to the float64 model")
        assert same > 0.98, (what, same)
    if col is not None:
        assert torch.equal(col, z[..., 4]), (what, "objectness column")


# ------------------------------------------------------------------ a. decode parity
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", H.NAMES)
def test_decode_entries_match_the_formula(dev, name, dtype):
    case = H.BY_NAME[name]
    heads = _heads(case, dev, dtype)
    # all levels in one launch
    xps, z, col = _outputs(case, dtype, dev)
    assert decode_levels(case, heads, dtype, xps, z, case.a_total, col) == OBB_OK
    check_against_ref(case, dtype, xps, z, col, "levels")
    # one launch per level, with and without the column
    for entry in ("col", "plain"):
        xps1, z1, col1 = _outputs(case, dtype, dev)
        off = 0
        for l, n in enumerate(case.level_rows):
            assert decode_one(case, heads, dtype, l, xps1[l], z1, case.a_total, off, col1 if entry == "col" else None, entry) == OBB_OK
            off += n
        check_against_ref(case, dtype, xps1, z1, col1 if entry == "col" else None, entry)
        assert torch.equal(z1, z) and all(torch.equal(a, b) for a, b in zip(xps1, xps)), entry
        assert entry == "plain" or torch.equal(col1, col)


@pytest.mark.parametrize("fused", [True, False], ids=["fused_levels", "per_level"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", H.NAMES)
def test_detect_forward_matches_the_formula(dev, name, dtype, fused):
    case = H.BY_NAME[name]
    det = _detect(case, dev, dtype)
    det.fused_levels = fused
    with torch.no_grad():
        z, xs = det(_heads(case, dev, dtype))
    assert type(z) is torch.Tensor and z.shape == (case.bs, case.a_total, case.no) and z.dtype == dtype
    check_against_ref(case, dtype, xs, z, z._obb_objcol[0], "forward")


# ------------------------------------------------------------------ b. only the bytes they own
MODES = ["all", "z", "xperm", "objcol", "none"]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", H.NAMES)
def test_entries_write_only_their_bytes(dev, name, dtype, mode):
    """Every output sits in a larger buffer of sentinel bytes, a_total is 8 rows more than the levels fill: guard bytes and the
    rows past the levels' sum keep the sentinel, for every partial-output mode of LazyHead.decode; what is written equals the
    plain call bit for bit."""
    case = H.BY_NAME[name]
    heads = _heads(case, dev, dtype)
    xps0, z0, col0 = _outputs(case, dtype, dev)
    assert decode_levels(case, heads, dtype, xps0, z0, case.a_total, col0) == OBB_OK
    a_total, rows, no, lx = case.a_total + EXTRA_ROWS, case.a_total, case.no, case.nl // 2
    for entry in ("levels", "col"):
        bz, bc = Buf(case.bs * a_total * no, dtype, dev), Buf(case.bs * a_total, dtype, dev)
        bx = [Buf(case.bs * n * no, dtype, dev) for n in case.level_rows]
        want_z, want_c = mode in ("all", "z"), mode in ("all", "objcol")
        want_x = [mode == "all" or (mode == "xperm" and l == lx) for l in range(case.nl)]
        if entry == "levels":
            rc = decode_levels(case, heads, dtype, [b.t if w else None for b, w in zip(bx, want_x)] if any(want_x) else None,
                               bz.t if want_z else None, a_total, bc.t if want_c else None)
            assert rc == OBB_OK
        else:
            off = 0
            for l, n in enumerate(case.level_rows):
                assert decode_one(case, heads, dtype, l, bx[l].t if want_x[l] else None, bz.t if want_z else None, a_total, off,
                                  bc.t if want_c else None) == OBB_OK
                off += n
        torch.cuda.synchronize(dev)
        for l in range(case.nl):
            if want_x[l]:
                assert bx[l].guards_intact() and torch.equal(bx[l].t.view(xps0[l].shape), xps0[l]), (entry, "x_perm", l)
            else:
                assert bx[l].untouched(), (entry, "x_perm", l)
        if want_z:
            zt = bz.t.view(case.bs, a_total, no)
            assert bz.guards_intact() and torch.equal(zt[:, :rows], z0), entry
            assert bool((zt[:, rows:].contiguous().view(torch.uint8) == SENTINEL).all()), (entry, "rows of z past the levels' sum")
        else:
            assert bz.untouched(), (entry, "z")
        if want_c:
            ct = bc.t.view(case.bs, a_total)
            assert bc.guards_intact() and torch.equal(ct[:, :rows], col0), entry
            assert bool((ct[:, rows:].contiguous().view(torch.uint8) == SENTINEL).all()), (entry, "column past the levels' sum")
        else:
            assert bc.untouched(), (entry, "objcol")


# ------------------------------------------------------------------ c. the element-wise path on vector-eligible maps
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", H.NAMES)
def test_misaligned_outputs_take_the_elementwise_path_same_bits(dev, name, dtype):
    """z one element off the 16-byte alignment; and every level placed behind one odd row (a_offset * no is then no multiple of
    16 bytes unless no itself is): obb_detect_decode_col must write the same bits as the aligned calls."""
    case = H.BY_NAME[name]
    heads = _heads(case, dev, dtype)
    xps0, z0, col0 = _outputs(case, dtype, dev)
    assert decode_levels(case, heads, dtype, xps0, z0, case.a_total, col0) == OBB_OK
    no = case.no
    # (1) z and the permuted heads one element off
    bz, bc = Buf(case.bs * case.a_total * no, dtype, dev, shift=1), Buf(case.bs * case.a_total, dtype, dev, shift=1)
    bx = [Buf(case.bs * n * no, dtype, dev, shift=1) for n in case.level_rows]
    assert bz.t.data_ptr() % 16 != 0
    off = 0
    for l, n in enumerate(case.level_rows):
        assert decode_one(case, heads, dtype, l, bx[l].t, bz.t, case.a_total, off, bc.t) == OBB_OK
        off += n
    torch.cuda.synchronize(dev)
    assert bz.guards_intact() and torch.equal(bz.t.view(z0.shape), z0)
    assert bc.guards_intact() and torch.equal(bc.t.view(col0.shape), col0)
    for l in range(case.nl):
        assert bx[l].guards_intact() and torch.equal(bx[l].t.view(xps0[l].shape), xps0[l]), l
    # (2) every level on its own behind one row of another size: a_offset = 1
    lo = 0
    for l, n in enumerate(case.level_rows):
        a_total = 1 + n
        bz, bc = Buf(case.bs * a_total * no, dtype, dev), Buf(case.bs * a_total, dtype, dev)
        assert decode_one(case, heads, dtype, l, None, bz.t, a_total, 1, bc.t) == OBB_OK
        torch.cuda.synchronize(dev)
        zt, ct = bz.t.view(case.bs, a_total, no), bc.t.view(case.bs, a_total)
        assert bz.guards_intact() and bc.guards_intact()
        assert torch.equal(zt[:, 1:], z0[:, lo:lo + n]) and torch.equal(ct[:, 1:], col0[:, lo:lo + n]), l
        assert bool((zt[:, :1].contiguous().view(torch.uint8) == SENTINEL).all()) and bool((ct[:, :1].contiguous().view(torch.uint8) == SENTINEL).all())
        lo += n


# ------------------------------------------------------------------ d. argument checks
def test_bad_arguments_are_rejected_before_any_launch(dev):
    """Each call below must return OBB_ERR_BAD_ARG; the buffers are large enough for the nearest valid call."""
    from yolov5_obb_amd import _lib
    L = _lib.lib()
    case = H.BY_NAME["nl2_na2_nc71"]
    heads = _heads(case, dev, torch.float32)
    xps, z, col = _outputs(case, torch.float32, dev)
    ny, nx = case.sizes[0]
    apx, st = C.cast(_farr(H.anchors_px(case)[0]), C.c_void_p), _lib.stream_ptr(dev)

    def one(dtype=0, bs=case.bs, na=case.na, no=case.no, a_total=case.a_total, a_off=0, zz=z):
        return L.obb_detect_decode_col(_ptr(heads[0]), dtype, bs, na, no, ny, nx, apx, 8.0, None, _ptr(zz), a_total, a_off, None, st)

    def plain(**kw):
        kw = dict(dict(dtype=0, bs=case.bs, na=case.na, no=case.no, a_total=case.a_total, a_off=0), **kw)
        return L.obb_detect_decode(_ptr(heads[0]), kw["dtype"], kw["bs"], kw["na"], kw["no"], ny, nx, apx, 8.0, None, _ptr(z),
                                   kw["a_total"], kw["a_off"], st)

    def lev(nl=case.nl, dtype=0, bs=case.bs, na=case.na, no=case.no, a_total=case.a_total):
        k = 5
        sizes = (list(case.sizes) * k)[:k]
        ptrs = (C.c_void_p * k)(*([h.data_ptr() for h in heads] * k)[:k])
        return L.obb_detect_decode_levels(nl, ptrs, dtype, bs, na, no, (C.c_int64 * k)(*[s[0] for s in sizes]),
                                          (C.c_int64 * k)(*[s[1] for s in sizes]), _farr(np.ones((k, 8, 2))), _farr([8.0] * k),
                                          None, _ptr(z), a_total, _ptr(col), st)

    assert one() == OBB_OK and plain() == OBB_OK and lev() == OBB_OK                       # the valid calls
    for f in (one, plain, lev):
        assert f(no=5) == OBB_ERR_BAD_ARG and f(no=442) == OBB_ERR_BAD_ARG, f.__name__
        assert f(na=9) == OBB_ERR_BAD_ARG and f(na=0) == OBB_ERR_BAD_ARG, f.__name__
        assert f(dtype=2) == OBB_ERR_BAD_ARG and f(dtype=-1) == OBB_ERR_BAD_ARG, f.__name__
        assert f(bs=8192, na=8) == OBB_ERR_BAD_ARG, f.__name__                             # bs * na = 65536
        assert f(bs=0) == OBB_ERR_BAD_ARG, f.__name__
    assert lev(nl=0) == OBB_ERR_BAD_ARG and lev(nl=5) == OBB_ERR_BAD_ARG
    n0 = case.level_rows[0]
    assert one(a_total=n0, a_off=1) == OBB_ERR_BAD_ARG and plain(a_total=n0, a_off=1) == OBB_ERR_BAD_ARG      # a_offset + na*HW > a_total
    assert one(a_total=n0 - 1) == OBB_ERR_BAD_ARG and one(a_off=-1) == OBB_ERR_BAD_ARG
    assert lev(a_total=case.a_total - 1) == OBB_ERR_BAD_ARG                                # the levels' sum > a_total
    torch.cuda.synchronize(dev)


@pytest.mark.parametrize("dtype", DTYPES)
def test_smallest_no_through_the_raw_abi(dev, dtype):
    """no = 6 (below anything Detect builds: 5 + nc + 180) decodes by the same formula."""
    rng = np.random.default_rng(77)
    na, no, sizes, bs = 3, 6, [(5, 8), (3, 3)], 2
    case = H.Case("raw_no6", 2, na, 1, tuple(sizes), bs)
    apx, st = H.anchors_px(case), H.strides(case)
    cv = [torch.from_numpy(np.clip(rng.normal(0.0, 4.0, (bs, na * no, ny, nx)), -12.0, 12.0)).to(dtype) for ny, nx in sizes]
    zr, xr, _ = H.decode_formula([c.numpy() for c in cv], na, no, apx, st, dtype == torch.float16)
    heads = [c.to(dev) for c in cv]
    rows = [na * ny * nx for ny, nx in sizes]
    for entry in ("levels", "col"):
        xps = [torch.empty((bs, na, ny, nx, no), dtype=dtype, device=dev) for ny, nx in sizes]
        z = torch.empty((bs, sum(rows), no), dtype=dtype, device=dev)
        col = torch.empty((bs, sum(rows)), dtype=dtype, device=dev)
        if entry == "levels":
            assert decode_levels(case, heads, dtype, xps, z, sum(rows), col, no=no) == OBB_OK
        else:
            from yolov5_obb_amd import _lib
            off = 0
            for l, (ny, nx) in enumerate(sizes):
                rc = _lib.lib().obb_detect_decode_col(_ptr(heads[l]), _code(dtype), bs, na, no, ny, nx, C.cast(_farr(apx[l]), C.c_void_p), st[l],
                                                      _ptr(xps[l]), _ptr(z), sum(rows), off, _ptr(col), _lib.stream_ptr(dev))
                assert rc == OBB_OK
                off += rows[l]
        for x, r in zip(xps, xr):
            assert np.array_equal(x.cpu().numpy().view(np.uint8), r.view(np.uint8)), entry
        zc = z.cpu().numpy()
        assert (H.close_fp32(zc, zr) if dtype == torch.float32 else H.close_fp16(zc, zr)).all(), entry
        assert torch.equal(col, z[..., 4]), entry


# ------------------------------------------------------------------ e. NMS on these heads
def _exact(got, ref, what=""):
    assert len(got) == len(ref), what
    for b, (g, r) in enumerate(zip(got, ref)):
        g = g.cpu()
        assert g.shape == r.shape, (what, b, tuple(g.shape), tuple(r.shape))
        if not torch.equal(g, r):
            k = int((g != r).any(1).nonzero()[0])
            raise AssertionError((what, f"image {b}: first differing row {k} of {len(r)}", g[k].tolist(), r[k].tolist()))


def _run(det, heads, lazy, **kw):
    from yolov5_obb_amd.utils.general import non_max_suppression_obb
    det.lazy_nms = lazy
    try:
        with torch.no_grad():
            z, _ = det(list(heads))
            out = non_max_suppression_obb(z, **kw)
    finally:
        det.lazy_nms = False
    return z, out


def _eager_and_lazy_equal_the_oracle(case, dev, dtype, **kw):
    from yolov5_obb_amd.utils import general
    det = _detect(case, dev, dtype)
    heads = _heads(case, dev, dtype)
    z, eager = _run(det, heads, False, **kw)
    ref = pyref.non_max_suppression_obb(z.cpu().clone(), **kw)
    _exact(eager, ref, "eager")
    general.hints_clear()
    for rep in range(3):
        zl, lazy = _run(det, heads, True, **kw)
        assert type(zl).__name__ == "LazyTensor" and not zl.is_materialized(), "the fused entry did not run"
        _exact(lazy, ref, ("lazy", rep))
    return ref


@pytest.mark.parametrize("multi_label", [True, False], ids=["multi_label", "best_class"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", H.NAMES)
def test_nms_eager_and_lazy_equal_the_oracle(dev, oracle_lib, binding, name, dtype, multi_label):
    case = H.BY_NAME[name]
    ref = _eager_and_lazy_equal_the_oracle(case, dev, dtype, multi_label=multi_label, **H.KW)
    assert sum(int(r.shape[0]) for r in ref) >= H.coverage_floor(case)[0]


@pytest.mark.parametrize("kw", [dict(agnostic=True), dict(classes=[0, 3, 7, 17])], ids=["agnostic", "classes"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_nms_arguments_at_eight_anchors(dev, oracle_lib, binding, dtype, kw):
    case = H.BY_NAME["nl4_na8_nc18_p6"]
    ref = _eager_and_lazy_equal_the_oracle(case, dev, dtype, multi_label=True, **H.KW, **kw)
    assert sum(int(r.shape[0]) for r in ref) >= 20
