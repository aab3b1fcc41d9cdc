"""ComputeLoss on the conv layout (obb_loss_config.head_layout = OBB_LOSS_LAYOUT_CONV, Detect.lazy_train): the loss reads the
1x1 convs' outputs (bs, na*no, ny, nx) where they lie and writes the gradient in the same layout.

The kernels keep the row -> thread assignment, the partial sums and the per-cell entry order of the row layout, so there is no
tolerance here: loss_out and every gradient element are compared BIT FOR BIT with the row layout on the permuted copy of the
same data (NaN equal to NaN), at the C ABI, through ComputeLoss, through Detect and under autocast + GradScaler.  The frozen
reference values (tests/golden/loss_configs.npz) go through the lazy path with the comparison of tests/test_loss_configs_gpu.py.
The memory contract of include/obb_hip.h is held with the harness of tests/abi_contract.py."""
import ctypes as C
import dataclasses
import itertools

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import abi_contract as AC
from tests import loss_cases as LC
from tests import synth

gpu = pytest.mark.gpu
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
# grids: a plane shorter than a 16-byte vector (1x1, 2x2), an odd plane that misaligns every later plane in fp16 (3x5), the ordinary case
SHAPES = {
    "nl1_na1_nc1": LC._c("lay_nl1", 1, 1, 1, [(3, 5)], 2, 50, seed=501),
    "nl3_na3_nc2": LC._c("lay_nl3", 3, 3, 2, [(8, 8), (3, 5), (1, 1)], 2, 50, seed=502),
    "nl4_na3_nc16": LC._c("lay_nl4", 4, 3, 16, [(8, 8), (3, 5), (2, 2), (1, 1)], 2, 50, seed=503),
}
OPTIONS = list(itertools.product((False, True), (0.0, 1.5), (187, 7)))          # sort_obj_iou, fl_gamma, target columns


def L_():
    from yolov5_obb_amd import _lib
    return _lib.lib()


def dense(x):
    """A copy with the strides of a freshly allocated tensor (contiguous() keeps odd strides on dimensions of size 1)."""
    return x.clone(memory_format=torch.contiguous_format)


def to_conv(x):
    """(bs, na, ny, nx, no) -> the conv output it is the permuted view of, (bs, na*no, ny, nx) contiguous."""
    bs, na, ny, nx, no = x.shape
    return dense(x.permute(0, 1, 4, 2, 3).reshape(bs, na * no, ny, nx))


def view_of(c, na):
    bs, ch, ny, nx = c.shape
    return c.view(bs, na, ch // na, ny, nx).permute(0, 1, 3, 4, 2)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(dense(a).view(torch.uint8), dense(b).view(torch.uint8))


_memo = {}


def inputs(shape, nt):
    """(case, fp32 rows-layout logits, (nt, 187) targets): nt = 50 is 40 random rows and the first 10 of them again, so that
    several targets land in one (image, anchor, cell) -- exact duplicates included.  Shared, never modified."""
    if (shape, nt) not in _memo:
        case = dataclasses.replace(SHAPES[shape], nt=nt)
        p, t = LC.random_inputs(dataclasses.replace(case, nt=min(nt, 40)))
        if nt > 40:
            t = torch.cat([t, t[:nt - 40]])
        assert t.shape == (nt, 187)
        _memo[shape, nt] = case, p, t
    return _memo[shape, nt]


def compute_loss(case, dev, sort=False, gamma=0.0):
    from yolov5_obb_amd.utils.loss import ComputeLoss
    ag, _, st = LC.head(case)
    hyp = LC.hyp_of(case)
    hyp["fl_gamma"] = gamma
    cl = ComputeLoss(synth.FakeModel(case.nc, hyp, dev, anchors=ag, strides=st))
    cl.sort_obj_iou = sort
    return cl


def abi_step(cfg, layout, heads, tg, dev, fill):
    """obb_loss_forward + obb_loss_backward on a poisoned workspace of exactly the queried size, the gradient buffers pre-filled
    with the byte `fill` -> (the 5 + nl floats of loss_out, the gradients in the layout of `heads`)."""
    from yolov5_obb_amd import _lib
    L = L_()
    cfg.head_layout = layout
    nl, nt, tcols = cfg.nl, int(tg.shape[0]), int(tg.shape[1])
    need = L.obb_loss_workspace_bytes(C.byref(cfg), nt)
    assert need > 0
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=dev)
    out = torch.full((5 + nl,), float("nan"), dtype=torch.float32, device=dev)
    grads = [torch.empty(h.shape, dtype=h.dtype, device=dev) for h in heads]
    for g in grads:
        g.view(torch.uint8).fill_(fill)
    gscale = torch.tensor([1.75], dtype=torch.float32, device=dev)
    parr = (C.c_void_p * nl)(*[h.data_ptr() for h in heads])
    garr = (C.c_void_p * nl)(*[g.data_ptr() for g in grads])
    code, st = _lib.DTYPE_CODES[heads[0].dtype], _lib.stream_ptr(dev)
    tptr = _lib.ptr(tg if nt else None)
    assert L.obb_loss_forward(C.byref(cfg), parr, code, tptr, nt, tcols, _lib.ptr(out), _lib.ptr(ws), need, st) == 0
    assert L.obb_loss_backward(C.byref(cfg), parr, code, tptr, nt, tcols, _lib.ptr(gscale), garr, _lib.ptr(ws), need, st) == 0
    torch.cuda.synchronize(dev)
    return out, grads


def untouched(g, fill):
    """Number of elements of g that still hold the pre-fill pattern."""
    word = {4: torch.int32, 2: torch.int16}[g.element_size()]
    pat = int.from_bytes(bytes([fill]) * g.element_size(), "little", signed=False)
    pat -= (1 << (8 * g.element_size())) if pat >= 1 << (8 * g.element_size() - 1) else 0
    return int((g.view(word) == pat).sum())


def compare_layouts(case, p, t, dtype, dev, sort, gamma, tcols):
    cl = compute_loss(case, dev, sort, gamma)
    cfg = cl._config(p)
    cfg.sort_obj_iou = int(sort)
    rows = [dense(x.to(device=dev, dtype=dtype)) for x in p]
    convs = [to_conv(x) for x in rows]
    tg = t[:, :tcols].contiguous().to(dev)
    out0, g0 = abi_step(cfg, 0, rows, tg, dev, 0x5A)
    out1, g1 = abi_step(cfg, 1, convs, tg, dev, 0xC3)
    what = (case.name, dtype, case.nt, sort, gamma, tcols)
    assert same_bits(out0, out1), (what, out0.tolist(), out1.tolist())
    for i, (a, b) in enumerate(zip(g0, g1)):
        assert untouched(b, 0xC3) == 0 and untouched(a, 0x5A) == 0, (what, i, "elements were not written")
        assert same_bits(a, view_of(b, case.na)), (what, "gradient of level", i)
    return out1, g1


# ---------------------------------------------------------------------------------------------------- C ABI, bitwise
@gpu
@pytest.mark.parametrize("nt", [0, 1, 50])
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_conv_layout_is_the_row_layout_bit_for_bit(dev, shape, dt, nt):
    case, p, t = inputs(shape, nt)
    if nt == 50:        # several entries in one cell: the owner / prev chain is walked
        cl = compute_loss(case, dev)
        _, _, indices, _, _ = cl.build_targets([x.to(dev) for x in p], t.to(dev))
        cells = torch.stack(indices[0], 1)
        assert cells.shape[0] > torch.unique(cells, dim=0).shape[0]
    finite = 0
    for sort, gamma, tcols in OPTIONS:
        out, grads = compare_layouts(case, p, t, DTYPES[dt], dev, sort, gamma, tcols)
        finite += bool(torch.isfinite(out).all())
        if nt == 50:      # matched cells: box gradients, not only the dense objectness planes
            assert bool((view_of(grads[0], case.na)[..., :4] != 0).any())
    assert finite == len(OPTIONS)


@gpu
@pytest.mark.parametrize("dt", list(DTYPES))
def test_an_image_index_outside_the_batch_is_nan_in_both_layouts(dev, dt):
    case, p, t = inputs("nl3_na3_nc2", 50)
    t = t.clone()
    t[5:15, 0] = float(case.bs)
    out, grads = compare_layouts(case, p, t, DTYPES[dt], dev, False, 0.0, 187)
    assert bool(torch.isnan(out[0]))
    for g in grads:       # the objectness planes are NaN, the untouched channels of unmatched cells stay zero
        assert bool(torch.isnan(view_of(g, case.na)[..., 4]).all())


# ---------------------------------------------------------------------------------------------------- frozen reference values
def lazy_heads(p, dev, dtype=torch.float32):
    convs = [to_conv(x.to(device=dev, dtype=dtype)).requires_grad_(True) for x in p]
    return convs, [view_of(c, x.shape[1]) for c, x in zip(convs, p)]


@gpu
@pytest.mark.parametrize("name", list(LC.FIXTURE))
def test_golden_reference_config_through_the_lazy_path(dev, name):
    """tests/test_loss_configs_gpu.py:test_golden_reference_config with the heads handed over as views of conv outputs."""
    from tests.test_loss_configs_gpu import _loss, fixture
    g = fixture()
    case, p, t = LC.fixture_inputs(name)
    cl = _loss(case, dev)
    tg = t[:, :7].contiguous() if case.csl7 else t
    convs, pg = lazy_heads(p, dev)
    loss, items = cl(pg, tg.to(dev))
    assert loss.grad_fn.cfg.head_layout == 1
    loss.backward()
    assert np.allclose(loss.detach().cpu().numpy(), g[f"{name}_loss"], rtol=1e-5, atol=1e-6)
    assert np.allclose(items.cpu().numpy(), g[f"{name}_items"], rtol=1e-5, atol=1e-6)
    tcls, tbox, indices, anch, tcsl = cl.build_targets(pg, tg.to(dev))
    for i in range(case.nl):
        assert np.array_equal(torch.stack(indices[i], 1).cpu().numpy(), g[f"{name}_idx{i}"]), i
        assert np.array_equal(tbox[i].cpu().numpy(), g[f"{name}_tbox{i}"]), i
        gs = LC.group_sums(view_of(convs[i].grad, case.na).double().cpu(), case.nc)
        ref = g[f"{name}_gradsum{i}"]
        assert np.all(np.abs(gs - ref) <= 1e-4 * np.abs(ref[:, 1:2]) + 1e-9), (i, gs, ref)


# ---------------------------------------------------------------------------------------------------- module level
NC, CH = 2, 8
GRIDS = (8, 4, 2)


class Model(nn.Module):
    """The least ComputeLoss reads from a model (utils/loss.py:93-120) around a real Detect."""

    def __init__(self, dev, dtype=torch.float32):
        super().__init__()
        from yolov5_obb_amd.models.yolo import Detect
        torch.manual_seed(11)
        det = Detect(nc=NC, anchors=synth.DEFAULT_ANCHORS, ch=(CH,) * 3)
        det.stride = torch.tensor(synth.DEFAULT_STRIDES)
        det.anchors /= det.stride.view(-1, 1, 1)
        self.model = nn.ModuleList([nn.Identity(), det])
        self.hyp = synth.scaled_hyp(NC, 64, 3)
        self.to(dev).to(dtype).train()

    @property
    def det(self):
        return self.model[-1]


def module_inputs(dev, dtype=torch.float32):
    g = torch.Generator().manual_seed(5)
    feats = [torch.randn(2, CH, n, n, generator=g).to(device=dev, dtype=dtype) for n in GRIDS]
    _, t = synth.s_loss(2, NC, 24, seed=9, imgsz=64, sizes=list(GRIDS), anchors=synth.DEFAULT_ANCHORS)
    return feats, torch.cat([t, t[:6]]).to(dev)


def step(model, cl, feats, t, lazy, scaler=None, autocast=False):
    """One forward + backward -> everything the comparisons need."""
    det = model.det
    det.lazy_train = lazy
    r = dict(convs=[], arrived=[None] * 3, returned=[None] * 3)

    def keep(_module, _inputs, out):
        out.retain_grad()
        r["convs"].append(out)
    hooks = [m.register_forward_hook(keep) for m in det.m]
    try:
        with torch.autocast("cuda", dtype=torch.float16, enabled=autocast):
            x = det([f.clone() for f in feats])
            for i in range(3):
                r["convs"][i].register_hook(lambda g, i=i: r["arrived"].__setitem__(i, g))
                x[i].register_hook(lambda g, i=i: r["returned"].__setitem__(i, g))
            loss, items = cl(x, t)
        r.update(x=x, loss=loss, items=items, saved=loss.grad_fn.saved_tensors[1:], layout=loss.grad_fn.cfg.head_layout)
        (scaler.scale(loss) if scaler else loss).backward()
    finally:
        for h in hooks:
            h.remove()
        det.lazy_train = False
    r["grads"] = [c.grad for c in r["convs"]]
    return r


def check_lazy_against_eager(e, z):
    assert (e["layout"], z["layout"]) == (0, 1)
    assert same_bits(e["loss"].detach(), z["loss"].detach()) and same_bits(e["items"], z["items"])
    assert bool(torch.isfinite(z["loss"]).all())
    for i in range(3):
        ce, cz = e["convs"][i], z["convs"][i]
        assert e["x"][i].shape == z["x"][i].shape == (2, 3, GRIDS[i], GRIDS[i], NC + 185) and e["x"][i].dtype == z["x"][i].dtype
        assert same_bits(e["x"][i].detach(), z["x"][i].detach())
        # the lazy outputs and what the Function saved ARE the conv outputs; the eager ones are copies
        assert z["x"][i].data_ptr() == cz.data_ptr() and not z["x"][i].is_contiguous()
        assert z["saved"][i].data_ptr() == cz.data_ptr() and z["saved"][i].stride() == z["x"][i].stride()
        assert e["x"][i].data_ptr() != ce.data_ptr() and e["saved"][i].data_ptr() != ce.data_ptr()
        # the gradient that arrives at the conv output is contiguous and is the buffer the backward allocated and returned
        assert same_bits(e["grads"][i], z["grads"][i])
        assert bool((z["grads"][i] != 0).any())
        assert z["arrived"][i].is_contiguous() and z["arrived"][i].shape == cz.shape
        assert z["arrived"][i].data_ptr() == z["returned"][i].data_ptr() and z["returned"][i].stride() == z["x"][i].stride()
        assert e["arrived"][i].data_ptr() != e["returned"][i].data_ptr()


@gpu
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_detect_lazy_train_against_eager(dev, dt):
    from yolov5_obb_amd.models.yolo import Detect
    from yolov5_obb_amd.utils.loss import ComputeLoss
    assert Detect.lazy_train is False
    model = Model(dev, DTYPES[dt])
    cl = ComputeLoss(model)
    feats, t = module_inputs(dev, DTYPES[dt])
    check_lazy_against_eager(step(model, cl, feats, t, False), step(model, cl, feats, t, True))


@gpu
def test_autocast_and_grad_scaler_step(dev):
    from yolov5_obb_amd.utils.loss import ComputeLoss
    model = Model(dev)
    cl = ComputeLoss(model)
    feats, t = module_inputs(dev)
    runs = [step(model, cl, feats, t, lazy, torch.amp.GradScaler("cuda", init_scale=1024.0), autocast=True) for lazy in (False, True)]
    assert all(c.dtype == torch.float16 for r in runs for c in r["convs"])
    check_lazy_against_eager(*runs)


# ---------------------------------------------------------------------------------------------------- fallbacks
def _eager_reference(case, p, t, dev, dtype):
    cl = compute_loss(case, dev)
    convs = [to_conv(x.to(device=dev, dtype=dtype)).requires_grad_(True) for x in p]
    loss, items = cl([view_of(c, case.na).contiguous() for c in convs], t.to(dev))
    assert loss.grad_fn.cfg.head_layout == 0
    loss.backward()
    return cl, loss.detach(), items, [c.grad for c in convs]


@gpu
@pytest.mark.parametrize("kind", ["one_level_contiguous", "channels_last", "sliced_base"])
def test_what_is_not_a_conv_view_falls_back_to_the_row_layout(dev, kind):
    from yolov5_obb_amd.utils.loss import is_conv_view
    case, p, t = inputs("nl3_na3_nc2", 50)
    dtype = torch.float16
    cl, loss_e, items_e, grads_e = _eager_reference(case, p, t, dev, dtype)
    convs = [to_conv(x.to(device=dev, dtype=dtype)) for x in p]
    if kind == "channels_last":
        leaves = [c.contiguous(memory_format=torch.channels_last).requires_grad_(True) for c in convs]
        heads = [view_of(c, case.na) for c in leaves]
        assert not any(is_conv_view(h) for h in heads[:2])
    elif kind == "sliced_base":          # every level starts one fp16 element behind a 16-byte boundary
        leaves = [torch.cat([c.new_zeros(1), c.reshape(-1)]).requires_grad_(True) for c in convs]
        heads = [view_of(l[1:].view(c.shape), case.na) for l, c in zip(leaves, convs)]
        assert all(h.data_ptr() % 16 == 2 and not is_conv_view(h) for h in heads)
    else:
        leaves = [c.clone().requires_grad_(True) for c in convs]
        heads = [view_of(c, case.na) for c in leaves]
        assert all(is_conv_view(h) for h in heads)
        heads[1] = heads[1].contiguous()
    loss, items = cl(heads, t.to(dev))
    assert loss.grad_fn.cfg.head_layout == 0
    loss.backward()
    assert same_bits(loss.detach(), loss_e) and same_bits(items, items_e)
    for i, (leaf, ge) in enumerate(zip(leaves, grads_e)):
        got = leaf.grad[1:].view(ge.shape) if kind == "sliced_base" else leaf.grad
        assert same_bits(got, ge), (kind, i)


# ---------------------------------------------------------------------------------------------------- memory contract
def contract_case(dev, shape, half):
    """obb_loss_forward + obb_loss_backward with head_layout = 1 as a case of tests/abi_contract.py; verify() holds the outputs,
    bit for bit, to the row layout's on the permuted copy."""
    vp = lambda x: C.c_void_p(int(x)) if x else C.c_void_p(0)
    case, p, t = inputs(shape, 50)
    dtype = torch.float16 if half else torch.float32
    cl = compute_loss(case, dev)
    cfg0 = cl._config(p)
    rows = [dense(x.to(device=dev, dtype=dtype)) for x in p]
    tg = t.to(dev)
    gscale = np.full(1, 1.75, dtype=np.float32)                 # abi_step's
    out0, g0 = abi_step(cfg0, 0, rows, tg, dev, 0x5A)
    want = [out0.cpu().numpy()] + [to_conv(g).cpu().numpy() for g in g0]
    cfg = cl._config(p)
    cfg.head_layout = 1
    nl, nt = case.nl, case.nt
    ph = [to_conv(x).cpu() for x in rows]
    inputs_ = {f"p{i}": x.numpy() for i, x in enumerate(ph)}
    inputs_.update(targets=t.numpy(), grad_scale=gscale)
    outs = dict(loss=(5 + nl) * 4)
    outs.update({f"g{i}": x.numel() * x.element_size() for i, x in enumerate(ph)})

    def call(L, P, ws, wsb, st, mark):
        parr = (C.c_void_p * nl)(*[P[f"p{i}"] for i in range(nl)])
        garr = (C.c_void_p * nl)(*[P[f"g{i}"] for i in range(nl)])
        rc = L.obb_loss_forward(C.byref(cfg), parr, int(half), vp(P["targets"]), nt, 187, vp(P["loss"]), vp(ws), wsb, vp(st))
        mark()
        if rc:
            return rc
        return L.obb_loss_backward(C.byref(cfg), parr, int(half), vp(P["targets"]), nt, 187, vp(P["grad_scale"]), garr, vp(ws), wsb, vp(st))

    def verify(O):
        got = [O("loss", np.float32)] + [O(f"g{i}", np.float16 if half else np.float32).reshape(tuple(x.shape)) for i, x in enumerate(ph)]
        assert AC.same_arrays(got, want), (shape, half)
        return got
    return AC.Case(f"obb_loss_forward+backward-conv-{shape}-{'f16' if half else 'f32'}", ["obb_loss_forward", "obb_loss_backward"], inputs_, outs,
                   lambda L: L.obb_loss_workspace_bytes(C.byref(cfg), nt), call, verify, index_inputs=("targets",))


CONTRACT = [("nl3_na3_nc2", True), ("nl4_na3_nc16", False)]
CONTRACT_IDS = [f"{s}-{'f16' if h else 'f32'}" for s, h in CONTRACT]


@gpu
@pytest.mark.parametrize("k", range(2), ids=CONTRACT_IDS)
def test_conv_layout_on_an_exact_poisoned_workspace_between_canaries(dev, k):
    AC.run_poisons(L_(), dev, contract_case(dev, *CONTRACT[k]), contract_case(dev, *CONTRACT[1 - k]))


@gpu
@pytest.mark.parametrize("ws_mode", ["short", "null", "+8", "+128"])
@pytest.mark.parametrize("k", range(2), ids=CONTRACT_IDS)
def test_conv_layout_refuses_a_short_missing_or_misaligned_workspace(dev, k, ws_mode):
    AC.run_refused(L_(), dev, contract_case(dev, *CONTRACT[k]), ws_mode)


@gpu
@pytest.mark.parametrize("k", range(2), ids=CONTRACT_IDS)
def test_conv_layout_under_a_capped_grid(dev, k):
    AC.run_capped(L_(), dev, contract_case(dev, *CONTRACT[k]))


@gpu
@pytest.mark.parametrize("k", range(2), ids=CONTRACT_IDS)
def test_conv_layout_enqueues_on_the_callers_stream(dev, k):
    from tests import test_abi_contract_gpu as TA
    _, pending = AC.run_on_side_stream(L_(), dev, contract_case(dev, *CONTRACT[k]), TA.DELAY_ITERS, TA._seed_matrix(dev))
    assert pending, "the delay had drained before the ABI call returned: the run proves nothing"
