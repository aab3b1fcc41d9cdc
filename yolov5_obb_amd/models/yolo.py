"""Mirror of the OBB ``Detect`` head of the reference's ``models/yolo.py`` (:33-92).

Only the head is mirrored: ``Model`` / ``parse_model`` / the CSP backbone stay the reference's PyTorch code (they run on
PyTorch-ROCm unchanged).  This class keeps the reference's constructor, attributes (``nc no nl na anchors m grid
anchor_grid stride inplace onnx_dynamic``), parameter names and return values, so checkpoints and ``parse_model`` can use it
in place of the reference's ``Detect``.  In inference mode on the GPU the per-level chain
``view -> permute -> contiguous -> sigmoid -> 2 slice updates -> cat`` is ONE pass of ``obb_detect_decode_col``
(libobb_hip.so, csrc/head.hip) per level.

Coupling with the NMS (the next stage of val.py / detect.py): the same pass stores the objectness column ``z[..., 4]`` once
more as a dense (bs, A) tensor and hangs it on the returned ``z`` (``z._obb_objcol = (column, z._version)``).
``utils.general.non_max_suppression_obb`` reads its confidence filter from that column -- 2 bytes per anchor instead of one
128-byte line of every 400-byte row -- when it is handed this very tensor object, unmodified (same ``_version``); any other
tensor (a clone, a cast, the TTA concatenation, an in-place edit) takes the plain path.  The results are identical.

Augmented inference (``Model._forward_augment``, :149-209): ``forward_augment`` below.  With ``Detect.fused_tta`` the three passes'
conv outputs are decoded, de-scaled, de-flipped and laid out like ``torch.cat(_clip_augmented(y), 1)`` by ONE launch of
``obb_detect_decode_tta``, and the result keeps its objectness column (the concatenation of the eager chain loses it).  With
``Detect.lazy_tta`` nothing is launched at all: the result is a ``LazyTensor`` that ``non_max_suppression_obb`` reads straight from
the passes' conv outputs (``obb_non_max_suppression_obb_tta_head``); any other use materialises the ``fused_tta`` tensor.
"""
import collections
import ctypes as C
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _lib
from ..lazy import LazyTensor

_LAZY_MAX_LEVELS = 4         # include/obb_hip.h obb_non_max_suppression_obb_head: nl <= 4
_LAZY_MAX_ANCHORS = 8        # ... na <= OBB_LOSS_MAX_ANCHORS


class Detect(nn.Module):
    stride = None  # strides computed during build
    onnx_dynamic = False  # ONNX export parameter
    # host copy of anchors * stride as plain Python lists (picklable; absent in checkpoints written by the reference: the
    # class default makes such modules work without a cast first)
    _anchor_px = None
    # inference on CPU tensors: this package has no CPU path.  yolov5_obb_amd.dropin.install() points this at the
    # reference's own Detect.forward (models/yolo.py:50-81), so that `detect.py --device cpu` keeps running its code.
    _cpu_forward = None
    # store z[..., 4] densely next to z for the confidence filter of non_max_suppression_obb (module docstring)
    couple_nms = True
    fused_levels = True      # all levels decoded by one launch (obb_detect_decode_levels); False: one launch per level
    # return z and x as lazy tensors (yolov5_obb_amd/lazy.py) that non_max_suppression_obb reads straight from the conv outputs
    # (obb_non_max_suppression_obb_head): nothing of size (bs, A, no) is written unless something else touches them
    lazy_nms = False
    # augmented inference (forward_augment below, Model._forward_augment under dropin.install()): the three passes' surviving
    # levels decoded, de-scaled, de-flipped and concatenated by ONE launch of obb_detect_decode_tta.  Opt-in like lazy_nms.
    fused_tta = False
    # training mode on the GPU: return the permuted heads as VIEWS of the conv outputs (same shape, dtype and values, no
    # transposing copy).  ComputeLoss reads them where they lie and writes the gradient straight into the conv layout
    # (OBB_LOSS_LAYOUT_CONV); any other consumer sees ordinary strided tensors.  Opt-in like lazy_nms.
    lazy_train = False
    # augmented inference without the dense prediction tensor: forward_augment returns a lazy z (yolov5_obb_amd/lazy.py) that
    # non_max_suppression_obb reads straight from the passes' conv outputs (obb_non_max_suppression_obb_tta_head); any other use
    # materialises exactly the fused_tta tensor.  Needs neither fused_tta nor lazy_nms.  Opt-in.
    lazy_tta = False
    _collect = False        # set by forward_augment around its passes: forward() returns the conv outputs

    def __init__(self, nc=80, anchors=(), ch=(), inplace=True):  # detection layer
        super().__init__()
        self.nc = nc  # number of classes
        self.no = nc + 5 + 180  # number of outputs per anchor (models/yolo.py:40)
        self.nl = len(anchors)  # number of detection layers
        self.na = len(anchors[0]) // 2  # number of anchors
        self.grid = [torch.zeros(1)] * self.nl  # init grid
        self.anchor_grid = [torch.zeros(1)] * self.nl  # init anchor grid
        self.register_buffer('anchors', torch.tensor(anchors).float().view(self.nl, -1, 2))  # shape(nl,na,2)
        self.m = nn.ModuleList(nn.Conv2d(x, self.no * self.na, 1) for x in ch)  # output conv
        self.inplace = inplace  # use in-place ops (e.g. slice assignment)

    @staticmethod
    def _tensor_key(t):
        """(version, storage address) of a tensor; inference tensors track no version counter: None = "cannot be cached"."""
        try:
            return (t._version, t.data_ptr())
        except RuntimeError:
            return None

    def _host_tables(self):
        # The reference reads anchors / stride on every call (models/yolo.py:90-91), so an in-place update after the first
        # inference (autoanchor's `m.anchors[:] = ...`, check_anchor_order) is picked up there; the host copy here is keyed
        # on the tensors' version counters and storage, like ComputeLoss._refresh_host_tables.
        stride_t = torch.as_tensor(self.stride)
        key = (self._tensor_key(self.anchors), self._tensor_key(stride_t))
        # (a tensor without a version counter -- created under torch.inference_mode() -- can change unnoticed: the small host table
        #  is then rebuilt on every call, as the reference re-reads the anchors on every call)
        if self._anchor_px is None or None in key or self._anchor_px[2] != key:
            st = [float(s) for s in stride_t.float().cpu().tolist()]
            an = self.anchors.detach().float().cpu()
            px = [(an[i] * st[i]).reshape(-1).tolist() for i in range(self.nl)]      # anchor_grid values (:90-91)
            self._anchor_px = (px, st, key)
        px, st = self._anchor_px[0], self._anchor_px[1]
        return [(C.c_float * len(p))(*p) for p in px], st      # ctypes arrays are built per call: they do not pickle

    def _apply(self, fn):  # anchors / stride may change (Model._apply, autoanchor): drop the host cache
        self._anchor_px = None
        return super()._apply(fn)

    def forward(self, x):
        """
        Args:
            x (list[P3_in,...]): torch.Size(b, c_i, h_i, w_i)
        Return：
            if train:
                x (list[P3_out,...]): torch.Size(b, self.na, h_i, w_i, self.no)
            else:
                inference (tensor): (b, n_all_anchors, self.no)
                x (list[P3_out,...]): torch.Size(b, self.na, h_i, w_i, self.no)
        """
        if self.training:
            for i in range(self.nl):
                x[i] = self.m[i](x[i])  # conv
                bs, _, ny, nx = x[i].shape
                x[i] = x[i].view(bs, self.na, self.no, ny, nx).permute(0, 1, 3, 4, 2)
                if not (self.lazy_train and x[i].is_cuda):
                    x[i] = x[i].contiguous()
            return x

        if not x[0].is_cuda:
            if type(self)._cpu_forward is None:
                raise RuntimeError("Detect (inference): yolov5_obb_amd is compiled for MI355X only (no CPU path, by design); "
                                   "under yolov5_obb_amd.dropin.install() CPU tensors run the reference's own Detect.forward")
            return type(self)._cpu_forward(self, x)
        convs = [self.m[i](x[i]).contiguous() for i in range(self.nl)]
        if self._collect:      # forward_augment: the conv outputs of this pass, nothing launched here
            return convs
        return self._decode(convs, x)

    def _decode(self, convs, x, allow_lazy=True):
        """The inference branch behind the 1x1 convs: (z, x) with x[i] replaced by the permuted raw heads."""
        c0 = convs[0]
        code = _lib.dtype_code(c0, "Detect (inference)")       # fp32 / fp16 / bf16: the decode runs in the conv outputs' dtype
        anchor_px, strides = self._host_tables()
        bs = c0.shape[0]
        shapes = [(c.shape[2], c.shape[3]) for c in convs]
        a_total = sum(self.na * ny * nx for ny, nx in shapes)
        if allow_lazy and self._lazy_possible(convs):
            for i, (ny, nx) in enumerate(shapes):
                if self.onnx_dynamic or self.grid[i].shape[2:4] != (ny, nx):
                    self.grid[i], self.anchor_grid[i] = self._make_grid(nx, ny, i)
            return _lazy_outputs(convs, code, self.na, self.no, anchor_px, strides, a_total, x)
        z = torch.empty((bs, a_total, self.no), dtype=c0.dtype, device=c0.device)
        col = torch.empty((bs, a_total), dtype=c0.dtype, device=c0.device) if self.couple_nms else None
        L = _lib.lib()
        for i, (ny, nx) in enumerate(shapes):
            if self.onnx_dynamic or self.grid[i].shape[2:4] != (ny, nx):
                self.grid[i], self.anchor_grid[i] = self._make_grid(nx, ny, i)      # kept for attribute compatibility
        xps = [torch.empty((bs, self.na, ny, nx, self.no), dtype=c0.dtype, device=c0.device) for ny, nx in shapes]
        with torch.cuda.device(c0.device):
            st = _lib.stream_ptr(c0.device)
            if self.nl <= 4 and self.fused_levels:
                # the loop over the levels and the torch.cat of models/yolo.py:61-79 as ONE launch
                nl = self.nl
                rc = L.obb_detect_decode_levels(nl, (C.c_void_p * nl)(*[c.data_ptr() for c in convs]), code, bs, self.na, self.no,
                                                (C.c_int64 * nl)(*[s[0] for s in shapes]), (C.c_int64 * nl)(*[s[1] for s in shapes]),
                                                (C.c_float * (nl * self.na * 2))(*[v for a in anchor_px for v in a]),
                                                (C.c_float * nl)(*strides[:nl]), (C.c_void_p * nl)(*[t.data_ptr() for t in xps]),
                                                _lib.ptr(z), a_total, _lib.ptr(col), st)
                _lib.check(rc, "obb_detect_decode_levels")
            else:
                off = 0
                for i in range(self.nl):
                    ny, nx = shapes[i]
                    rc = L.obb_detect_decode_col(_lib.ptr(convs[i]), code, bs, self.na, self.no, ny, nx, C.cast(anchor_px[i], C.c_void_p),
                                                 strides[i], _lib.ptr(xps[i]), _lib.ptr(z), a_total, off, _lib.ptr(col), st)
                    _lib.check(rc, "obb_detect_decode_col")
                    off += self.na * ny * nx
        for i in range(self.nl):
            x[i] = xps[i]
        if col is not None and not torch.is_inference(z):
            # read by utils.general.non_max_suppression_obb (module docstring).  Under torch.inference_mode() tensors carry no
            # version counter, so "unchanged since Detect wrote it" cannot be checked: the column is not attached and the NMS
            # scans z[..., 4] itself (same results).
            z._obb_objcol = (col, z._version)
        return z, x

    def _lazy_possible(self, convs):
        """lazy_nms applies: eval mode on the GPU (checked by the caller), grad disabled, version counters present (not under
        torch.inference_mode(), like couple_nms), and the limits of obb_non_max_suppression_obb_head."""
        return self.lazy_nms and self._lazy_conditions(convs)

    def _lazy_conditions(self, convs):
        """What a lazy output needs whichever flag asks for it (lazy_nms, lazy_tta)."""
        return (not torch.is_grad_enabled() and not torch.is_inference_mode_enabled()
                and not any(torch.is_inference(c) for c in convs) and 1 <= self.nl <= _LAZY_MAX_LEVELS
                and 1 <= self.na <= _LAZY_MAX_ANCHORS and 1 <= self.nc <= 256)

    def _make_grid(self, nx=20, ny=20, i=0):  # models/yolo.py:83-92
        d = self.anchors[i].device
        yv, xv = torch.meshgrid([torch.arange(ny, device=d), torch.arange(nx, device=d)], indexing='ij')
        grid = torch.stack((xv, yv), 2).expand((1, self.na, ny, nx, 2)).float()
        anchor_grid = (self.anchors[i].clone() * self.stride[i]).view((1, self.na, 1, 1, 2)).expand((1, self.na, ny, nx, 2)).float()
        return grid, anchor_grid


class LazyHead:
    """What a lazy Detect output keeps: the conv outputs with the version counters they had at forward time, and the host
    anchor / stride tables.  The values the outputs stand for were fixed at forward time: once a conv output has been
    modified in place they are gone, and any use of the outputs raises."""

    def __init__(self, convs, code, na, no, anchor_px, strides):
        self.convs = convs
        self.versions = [c._version for c in convs]
        self.code, self.na, self.no = code, na, no
        self.nl = len(convs)
        self.anchor_px = [float(v) for a in anchor_px for v in a]       # [nl][na][2] flattened
        self.strides = [float(s) for s in strides[:self.nl]]

    def check(self):
        if [c._version for c in self.convs] != self.versions:
            raise RuntimeError("Detect (lazy_nms): a conv output was modified in place after forward(); the prediction it stood "
                               "for is gone -- keep the conv outputs unchanged until the outputs are used, or set lazy_nms = False")

    def decode(self, z=None, level=None, xp=None):
        """Run the Detect decode into z (all levels) or into the permuted raw head xp of one level (obb_detect_decode_levels /
        obb_detect_decode_col with only that output non-NULL)."""
        self.check()
        L = _lib.lib()
        c0 = self.convs[0]
        bs, nl, na = c0.shape[0], self.nl, self.na
        with torch.cuda.device(c0.device):
            st = _lib.stream_ptr(c0.device)
            if z is not None:
                rc = L.obb_detect_decode_levels(nl, (C.c_void_p * nl)(*[c.data_ptr() for c in self.convs]), self.code, bs, na, self.no,
                                                (C.c_int64 * nl)(*[c.shape[2] for c in self.convs]),
                                                (C.c_int64 * nl)(*[c.shape[3] for c in self.convs]),
                                                (C.c_float * len(self.anchor_px))(*self.anchor_px), (C.c_float * nl)(*self.strides),
                                                None, _lib.ptr(z), z.shape[1], None, st)
                _lib.check(rc, "obb_detect_decode_levels")
            else:
                c = self.convs[level]
                px = (C.c_float * (2 * na))(*self.anchor_px[2 * na * level:2 * na * (level + 1)])
                rc = L.obb_detect_decode_col(_lib.ptr(c), self.code, bs, na, self.no, c.shape[2], c.shape[3], C.cast(px, C.c_void_p),
                                             self.strides[level], _lib.ptr(xp), None, 0, 0, None, st)
                _lib.check(rc, "obb_detect_decode_col")


def _lazy_outputs(convs, code, na, no, anchor_px, strides, a_total, x):
    """(lazy z, [lazy x_i]) of Detect.forward's inference branch; nothing is launched here."""
    head = LazyHead(convs, code, na, no, anchor_px, strides)
    c0 = convs[0]
    bs, dt, dev = c0.shape[0], c0.dtype, c0.device

    def make_z():
        z = torch.empty((bs, a_total, no), dtype=dt, device=dev)
        head.decode(z=z)
        return z

    def make_x(i):
        def run():
            c = convs[i]
            xp = torch.empty((bs, na, c.shape[2], c.shape[3], no), dtype=dt, device=dev)
            head.decode(level=i, xp=xp)
            return xp
        return run

    z = LazyTensor((bs, a_total, no), dt, dev, make_z, payload=head)
    for i, c in enumerate(convs):
        x[i] = LazyTensor((bs, na, c.shape[2], c.shape[3], no), dt, dev, make_x(i))
    return z, x


# ---------------------------------------------------------------------------------------------------------------------------
# Augmented inference (models/yolo.py:149-209 of the reference: _forward_augment, _descale_pred, _clip_augmented)

TtaPassPlan = collections.namedtuple("TtaPassPlan", "levels offsets rows lo hi")
TtaPlan = collections.namedtuple("TtaPlan", "passes a_total on_boundary")


def _clip_rows(totals, nl):
    """The row range [lo, hi) every pass keeps of its `totals[k]` rows (the row-count rule of tta_plan's docstring)."""
    g = sum(4 ** k for k in range(nl))
    lo, hi = [0] * len(totals), list(totals)
    cut = hi[0] // g
    hi[0] = hi[0] - cut if cut else 0                      # a slice [:-0] keeps nothing
    cut = ((hi[-1] - lo[-1]) // g) * 4 ** (nl - 1)
    lo[-1] = min(lo[-1] + cut, hi[-1])
    return lo, hi


def tta_plan(level_shapes_per_pass, na, nl):
    """Where the rows of every pass land in torch.cat(_clip_augmented(y), 1).  Pure Python.

    level_shapes_per_pass: per pass, the (ny, nx) of its nl levels.  The reference clips by ROW COUNT (models/yolo.py:200-209):
    with g = sum(4**k for k < nl), the first pass loses its last (A0 // g) * 1 rows and the last pass its first
    (A_last // g) * 4**(nl - 1) rows -- whole levels exactly when the levels' areas are in the ratio 4:1.

    Returns TtaPlan(passes, a_total, on_boundary); per pass TtaPassPlan(levels, offsets, rows, lo, hi): the kept row range
    [lo, hi) of the pass's own rows, `rows` = hi - lo, the levels that lie inside it and the output row each of them starts at.
    on_boundary is False when a cut splits a level (`levels` then lists only the whole ones: the plan cannot be decoded level-wise).
    """
    rows = [[na * ny * nx for ny, nx in shapes] for shapes in level_shapes_per_pass]
    lo, hi = _clip_rows([sum(r) for r in rows], nl)
    passes, out, on_boundary = [], 0, True
    for r, a, b in zip(rows, lo, hi):
        edges = [sum(r[:k]) for k in range(len(r) + 1)]
        if b > a and not (a in edges and b in edges):
            on_boundary = False
        levels, offsets = [], []
        for k in range(len(r)):
            if r[k] and edges[k] >= a and edges[k + 1] <= b:
                levels.append(k)
                offsets.append(out + edges[k] - a)
        passes.append(TtaPassPlan(tuple(levels), tuple(offsets), b - a, a, b))
        out += b - a
    return TtaPlan(passes, out, on_boundary)


def scale_img(img, ratio=1.0, same_shape=False, gs=32):
    """An image batch (bs, c, h, w) resized by `ratio` (bilinear, align_corners=False) and padded with 0.447 up to the next
    multiple of gs of the scaled size -- or back to (h, w) with same_shape.  Ratio 1 returns the batch itself.  Same values as
    the reference's utils.torch_utils.scale_img."""
    if ratio == 1.0:
        return img
    h, w = img.shape[2:]
    nh, nw = int(h * ratio), int(w * ratio)
    out = F.interpolate(img, size=(nh, nw), mode="bilinear", align_corners=False)
    ph, pw = (h, w) if same_shape else (math.ceil(h * ratio / gs) * gs, math.ceil(w * ratio / gs) * gs)
    return F.pad(out, [0, pw - nw, 0, ph - nh], value=0.447)


_scale_img = scale_img       # (forward_augment has a parameter of that name)


def _tta_passes(convs_per_pass, plan, scales, flips, img_h, img_w, na, anchor_px, strides):
    """The obb_tta_pass array of the plan's surviving levels (a pass that keeps no level is not listed)."""
    listed = [(k, p) for k, p in enumerate(plan.passes) if p.levels]
    arr = (_lib.TtaPass * len(listed))()
    for t, (k, p) in zip(arr, listed):
        t.nl, t.flip, t.scale, t.img_h, t.img_w = len(p.levels), int(flips[k] or 0), float(scales[k]), int(img_h), int(img_w)
        for j, lv in enumerate(p.levels):
            c = convs_per_pass[k][lv]
            t.conv_out[j], t.ny[j], t.nx[j], t.stride[j] = c.data_ptr(), c.shape[2], c.shape[3], strides[lv]
            for a in range(na):
                t.anchors_px[j][a][0], t.anchors_px[j][a][1] = anchor_px[lv][2 * a], anchor_px[lv][2 * a + 1]
    return arr


def _decode_tta(det, convs_per_pass, plan, scales, flips, img_h, img_w, tables=None):
    """One obb_detect_decode_tta launch for the plan's surviving levels -> z (bs, a_total, no) with the objectness column.
    tables: (anchor_px, strides) read earlier (a lazy output's), or None for the head's current ones."""
    c0 = convs_per_pass[0][0]
    code = _lib.dtype_code(c0, "forward_augment")
    anchor_px, strides = tables or det._host_tables()
    bs, na = c0.shape[0], det.na
    arr = _tta_passes(convs_per_pass, plan, scales, flips, img_h, img_w, na, anchor_px, strides)
    z = torch.empty((bs, plan.a_total, det.no), dtype=c0.dtype, device=c0.device)
    col = torch.empty((bs, plan.a_total), dtype=c0.dtype, device=c0.device) if det.couple_nms else None
    with torch.cuda.device(c0.device):
        rc = _lib.lib().obb_detect_decode_tta(len(arr), C.cast(arr, C.c_void_p), code, bs, na, det.no, _lib.ptr(z), plan.a_total,
                                              _lib.ptr(col), _lib.stream_ptr(c0.device))
    _lib.check(rc, "obb_detect_decode_tta")
    if col is not None and not torch.is_inference(z):      # as in Detect.forward: no version counter, no column
        z._obb_objcol = (col, z._version)
    return z


class LazyTtaHead:
    """What a lazy forward_augment output keeps (Detect.lazy_tta): the passes' conv outputs with the version counters they had
    when the passes ran, the plan, the passes' scales and flips, the image size and the host anchor / stride tables.  Like
    LazyHead, the values the output stands for were fixed then: an in-place edit of a conv output makes any use raise."""
    tta = True

    def __init__(self, det, convs_per_pass, plan, scales, flips, img_h, img_w):
        anchor_px, strides = det._host_tables()
        self.det = det
        self.convs = convs_per_pass
        self.versions = [[c._version for c in cs] for cs in convs_per_pass]
        self.plan, self.scales, self.flips = plan, [float(s) for s in scales], [int(f or 0) for f in flips]
        self.img_h, self.img_w = int(img_h), int(img_w)
        self.code = _lib.dtype_code(convs_per_pass[0][0], "forward_augment")
        self.na, self.no, self.a_total = det.na, det.no, plan.a_total
        self.anchor_px = [list(a) for a in anchor_px]           # [level][na * 2], pixels
        self.strides = [float(s) for s in strides]
        self.listed = [k for k, p in enumerate(plan.passes) if p.levels]

    def check(self):
        if [[c._version for c in cs] for cs in self.convs] != self.versions:
            raise RuntimeError("forward_augment (lazy_tta): a conv output was modified in place after the passes ran; the prediction "
                               "it stood for is gone -- keep the conv outputs unchanged until the output is used, or set lazy_tta = False")

    def passes(self):
        """The obb_tta_pass array of obb_non_max_suppression_obb_tta_head / obb_detect_decode_tta."""
        return _tta_passes(self.convs, self.plan, self.scales, self.flips, self.img_h, self.img_w, self.na, self.anchor_px, self.strides)

    def pass_lists(self):
        """The same as plain lists for the compiled binding: per listed pass its surviving convs, scale, flip, anchors
        [nl][na][2] flattened and strides [nl]."""
        out = []
        for k in self.listed:
            lv = self.plan.passes[k].levels
            out.append(([self.convs[k][i] for i in lv], self.scales[k], self.flips[k], [v for i in lv for v in self.anchor_px[i]],
                        [self.strides[i] for i in lv]))
        return out

    def decode(self):
        """The fused_tta tensor (the materialiser of the lazy output)."""
        self.check()
        return _decode_tta(self.det, self.convs, self.plan, self.scales, self.flips, self.img_h, self.img_w,
                           tables=(self.anchor_px, self.strides))


def _lazy_tta_output(det, convs_per_pass, plan, scales, flips, img_h, img_w):
    """The lazy z of forward_augment; nothing is launched here."""
    head = LazyTtaHead(det, convs_per_pass, plan, scales, flips, img_h, img_w)
    c0 = convs_per_pass[0][0]
    return LazyTensor((c0.shape[0], plan.a_total, det.no), c0.dtype, c0.device, head.decode, payload=head)


def forward_augment(model, x, scales=(1, 0.83, 0.67), flips=(None, 3, None), scale_img=None):
    """Model._forward_augment of the reference for a model whose head is this package's Detect: (z, None).

    With Detect.fused_tta on GPU tensors the passes run with the head collecting its conv outputs, and ONE launch decodes,
    de-scales, de-flips and concatenates them (obb_detect_decode_tta): z is written once, in place, with the objectness column
    attached.  fused_tta wins over lazy_nms here.  With Detect.lazy_tta (and grad disabled, outside torch.inference_mode()) the same
    passes are collected and z is a LazyTensor that launches nothing: non_max_suppression_obb reads the conv outputs
    (obb_non_max_suppression_obb_tta_head), any other use materialises the fused_tta tensor.  Otherwise -- both flags off, CPU
    tensors, nl > 4, a flip other than None / 2 / 3, or a clip that does not fall on a level boundary (tta_plan) -- the reference's chain of torch ops on the eager passes; the
    values are the same.  scale_img: the reference's utils.torch_utils.scale_img, or None for this module's.
    """
    det = model.model[-1]
    resize = scale_img or _scale_img
    gs = int(torch.as_tensor(model.stride).max())
    img_h, img_w = x.shape[-2:]
    passes = list(zip(scales, flips))

    def run(si, fi):
        return model._forward_once(resize(x.flip(fi) if fi else x, si, gs=gs))

    level_wise = (x.is_cuda and not det.training and det.nl <= _lib.DETECT_MAX_LEVELS
                  and det.na <= _lib.MAX_ANCHORS and 1 <= len(passes) <= _lib.TTA_MAX_PASSES and all(fi in (None, 0, 2, 3) for _, fi in passes)
                  and all(si > 0 and math.isfinite(si) for si, _ in passes))
    fused = getattr(det, "fused_tta", False) and level_wise
    lazy = getattr(det, "lazy_tta", False) and level_wise and det._lazy_conditions(())
    if fused or lazy:
        det._collect = True
        try:
            convs = [run(si, fi) for si, fi in passes]
        finally:
            del det._collect
        plan = tta_plan([[tuple(c.shape[2:]) for c in cs] for cs in convs], det.na, det.nl)
        if plan.on_boundary and plan.a_total > 0:
            if lazy and det._lazy_conditions([c for cs in convs for c in cs]):
                return _lazy_tta_output(det, convs, plan, [s for s, _ in passes], [f for _, f in passes], img_h, img_w), None
            if fused:
                return _decode_tta(det, convs, plan, [s for s, _ in passes], [f for _, f in passes], img_h, img_w), None
        y = [det._decode(cs, list(cs), allow_lazy=False)[0] for cs in convs]     # the cut splits a level (or lazy_tta alone cannot apply): the chain, eagerly
    else:
        y = [run(si, fi)[0] for si, fi in passes]
    return _augment_chain(y, passes, img_h, img_w, det.nl, getattr(model, "inplace", True)), None


def _augment_chain(y, passes, img_h, img_w, nl, inplace=True):
    """_descale_pred, _clip_augmented and the torch.cat of the reference on the passes' predictions (torch ops)."""
    out = []
    for p, (si, fi) in zip(y, passes):
        if not inplace:
            p = p.clone()
        p[..., :4] /= si
        if fi == 2:
            p[..., 1] = img_h - p[..., 1]
        elif fi == 3:
            p[..., 0] = img_w - p[..., 0]
        out.append(p)
    lo, hi = _clip_rows([p.shape[1] for p in out], nl)
    return torch.cat([p[:, a:b] for p, a, b in zip(out, lo, hi)], 1)
