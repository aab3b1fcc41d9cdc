"""ComputeLoss (csrc/loss.hip) against the oracle (oracle/pyref.py) across the head configurations its C ABI accepts:
nl 1-8, na 1-8, nc 1-256 (every 64-channel chunk of a row), non-square, odd and 1x1 grids, a level of one row, last 64-row
regions that end in a partial 16-byte vector (the scalar tail of k_loss_bwd_dense), bs 1 / 3 / 16, fp32 and fp16,
sort_obj_iou, focal loss, label smoothing, (nt, 7) targets and autobalance.  The cases live in tests/loss_cases.py.

Each case checks build_targets (indices, tbox, anchors, classes bit-exact; the CSL rows bit-exact when they are stored, within
one float ulp when regenerated from theta), the loss scalars (rtol 1e-5; fp16 as test_fp16_heads) and every element of every
gradient tensor per channel group (tests/test_loss_gpu.py:check_grads).  The gradient tensors are not pre-filled: the blocks
the caching allocator hands to the backward were filled with NaN just before, so an element the kernels skip fails."""
import os

import numpy as np
import pytest
import torch

from oracle import pyref
from tests import loss_cases as LC
from tests import synth
from tests.test_loss_gpu import ACHIEVED, check_grads

FIX = None


def fixture():
    global FIX
    if FIX is None:
        FIX = np.load(os.path.join(os.path.dirname(__file__), "golden", "loss_configs.npz"))
    return FIX


def _loss(case, dev, sort_obj_iou=None):
    from yolov5_obb_amd.utils.loss import ComputeLoss
    ag, _, st = LC.head(case)
    cl = ComputeLoss(synth.FakeModel(case.nc, LC.hyp_of(case), dev, anchors=ag, strides=st), autobalance=case.autobalance)
    if LC.balance_of(case):
        cl.balance = list(LC.balance_of(case))
    cl.sort_obj_iou = case.sort_obj_iou if sort_obj_iou is None else sort_obj_iou
    return cl


def _poison(like):
    """Fill, then free, blocks of the gradients' sizes: the backward's torch.empty_like gets them back from the cache."""
    junk = [torch.full_like(x, float("nan")) for x in like]
    del junk


def _compare_targets(cl, case, p, t, tg, dev):
    spec = LC.spec_of(case)
    ref = pyref.build_targets(spec, p, t)
    tcls, tbox, indices, anch, tcsl = cl.build_targets([x.to(dev) for x in p], tg.to(dev))
    for i in range(case.nl):
        r = ref[i]
        assert np.array_equal(torch.stack(indices[i], 1).cpu().numpy(), torch.stack((r['b'], r['a'], r['gj'], r['gi']), 1).numpy()), i
        assert np.array_equal(tbox[i].cpu().numpy(), r['tbox'].numpy()), i
        assert np.array_equal(anch[i].cpu().numpy(), r['anch'].numpy()), i
        assert np.array_equal(tcls[i].cpu().numpy(), r['tcls'].numpy()), i
        if case.csl7:       # regenerated on the device from theta: exp in double, stored as float, vs numpy's exp
            np.testing.assert_array_max_ulp(tcsl[i].cpu().numpy(), r['csl'].numpy(), maxulp=1)
        else:
            assert np.array_equal(tcsl[i].cpu().numpy(), r['csl'].numpy()), i
    return ref


def run_case(case, p, t, dev, sort_obj_iou=None):
    sort = case.sort_obj_iou if sort_obj_iou is None else sort_obj_iou
    dtype = torch.float16 if case.half else torch.float32
    spec = LC.spec_of(case)
    cl = _loss(case, dev, sort)
    tg = t[:, :7].contiguous() if case.csl7 else t
    _compare_targets(cl, case, p, t, tg, dev)
    pc = [x.clone().to(dtype).float().requires_grad_(True) for x in p]          # the oracle sees the dtype-rounded logits
    lo, io = pyref.compute_loss(spec, pc, t.clone(), sort_obj_iou=sort, autobalance=case.autobalance)
    lo.backward()
    pg = [x.clone().to(device=dev, dtype=dtype).requires_grad_(True) for x in p]
    lg, ig = cl(pg, tg.to(dev))
    _poison(pg)
    lg.backward()
    assert lg.shape == (1,) and ig.shape == (4,)
    if case.half:       # as test_fp16_heads: tobj is rounded to fp16 (utils/loss.py:155), gradients are stored in fp16
        assert np.allclose(lg.detach().cpu().numpy(), lo.detach().numpy(), rtol=2e-3), (lg, lo)
        assert np.allclose(ig.cpu().numpy(), io.numpy(), rtol=2e-3, atol=1e-5), (ig, io)
        assert all(x.grad.dtype == torch.float16 for x in pg)
        check_grads(pg, pc, grtol=2e-3, atol=1e-7)
    else:
        assert np.allclose(lg.detach().cpu().numpy(), lo.detach().numpy(), rtol=1e-5, atol=1e-6), (lg, lo)
        assert np.allclose(ig.cpu().numpy(), io.numpy(), rtol=1e-5, atol=1e-6), (ig, io)
        ref = np.concatenate([lo.detach().numpy().ravel(), io.numpy().ravel()])
        got = np.concatenate([lg.detach().cpu().numpy().ravel(), ig.cpu().numpy().ravel()])
        ok = np.abs(ref) > 1e-3
        if ok.any():
            ACHIEVED["scalar_rel"] = max(ACHIEVED["scalar_rel"], float(np.max(np.abs(got[ok] - ref[ok]) / np.abs(ref[ok]))))
        check_grads(pg, pc)
    if case.autobalance:      # (the reference keeps its 5-entry default list at nl = 4; only the first nl entries are used)
        assert len(cl.balance) == case.nl and cl.balance[1] == 1.0
        assert np.allclose(np.asarray(cl.balance, np.float64), np.asarray(spec.balance[:case.nl], np.float64), rtol=1e-6), (cl.balance, spec.balance)
    return lg


def test_case_table_covers_every_axis():
    """CPU: the case table reaches every value the issue of this module lists (no GPU needed)."""
    C = LC.CASES
    assert {k.nl for k in C} >= {1, 2, 3, 4, 5, 8}
    assert {k.na for k in C} >= {1, 2, 3, 4, 8}
    assert {k.nc for k in C} >= {1, 2, 7, 8, 71, 72, 135, 136, 199, 200, 256}
    assert {k.bs for k in C} >= {1, 3, 16}
    shapes = [s for k in C for s in k.sizes]
    assert any(ny > nx > 1 for ny, nx in shapes) and any(nx > ny > 1 for ny, nx in shapes)
    assert any(ny % 2 and nx % 2 and ny > 1 for ny, nx in shapes) and (1, 1) in shapes
    assert any(k.rows(i) == 1 for k in C for i in range(k.nl))
    for half in (False, True):
        assert any(k.tail(i) for k in C if k.half == half for i in range(k.nl)), half
    assert 0.25 <= sum(k.half for k in C) / len(C) <= 0.45
    assert any(k.sort_obj_iou for k in C) and any(k.csl7 for k in C) and any(k.autobalance and k.nl == 4 for k in C)
    assert any(k.hyp.get('fl_gamma') for k in C) and any(k.hyp.get('label_smoothing') for k in C)
    assert 40 <= 2 * len(C) <= 60


@pytest.mark.gpu
@pytest.mark.parametrize("name", [k.name for k in LC.CASES])
def test_random_targets(dev, name):
    case = LC.BY_NAME[name]
    p, t = LC.random_inputs(case)
    run_case(case, p, t, dev)


@pytest.mark.gpu
@pytest.mark.parametrize("name", [k.name for k in LC.CASES])
def test_planted_edge_targets(dev, name):
    """Targets on the cell-boundary and ratio edges of build_targets, degenerate and NaN sizes, theta where the CSL roll
    changes, the last image and class, and a crowd with exact duplicates in one cell (tests/loss_cases.py:planted_targets).
    sort_obj_iou is flipped against the random-target case of the same configuration, so both settings see the crowd."""
    case = LC.BY_NAME[name]
    p, _ = LC.random_inputs(case)
    run_case(case, p, LC.planted_targets(case), dev, sort_obj_iou=not case.sort_obj_iou)


@pytest.mark.gpu
@pytest.mark.parametrize("sort", [False, True])
@pytest.mark.parametrize("half", [False, True])
def test_duplicate_rows_reach_the_tie_rule(dev, sort, half):
    """Exact duplicate target rows give exactly equal CIoU: the winner of the cell's objectness target (last writer, or the
    largest score with ties to the later row under sort_obj_iou) must not change the loss or any gradient."""
    case = LC._c("dups", 3, 3, 16, [(12, 8), (6, 4), (3, 2)], 2, 30, half=half, seed=91)
    p, t = LC.random_inputs(case)
    t = torch.cat([t, t[:10], t[:10], t[5:15]])
    run_case(case, p, t, dev, sort_obj_iou=sort)


@pytest.mark.gpu
def test_nc1_class_beyond_nc_is_finite(dev):
    """nc = 1 with targets of class 0 and class 3: the reference skips the class term (utils/loss.py:163) and never indexes
    by class, so its loss is finite.  Regression: bt_eval flagged cls >= nc for every nc, which made the loss NaN."""
    case, p, t = LC.nc1_class3_inputs()
    lg = run_case(case, p, t, dev)
    assert torch.isfinite(lg).all()


@pytest.mark.gpu
def test_negative_class_stays_bad_at_nc1(dev):
    """A negative class (or image) index is a bad row for every nc (include/obb_hip.h), although torch would wrap it."""
    case, p, t = LC.nc1_class3_inputs()
    t = t.clone()
    t[:, 1] = -1.0
    cl = _loss(case, dev)
    pg = [x.clone().to(dev).requires_grad_(True) for x in p]
    loss, _ = cl(pg, t.to(dev))
    assert torch.isnan(loss).all()
    with pytest.raises(IndexError):
        cl.build_targets([x.to(dev) for x in p], t.to(dev))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(LC.FIXTURE))
def test_golden_reference_config(dev, name):
    """The configurations frozen from the reference's own utils/loss.py (tests/golden/gen_loss_configs.py)."""
    g = fixture()
    case, p, t = LC.fixture_inputs(name)
    cl = _loss(case, dev)
    tg = t[:, :7].contiguous() if case.csl7 else t
    pg = [x.clone().to(dev).requires_grad_(True) for x in p]
    loss, items = cl(pg, tg.to(dev))
    loss.backward()
    assert np.allclose(loss.detach().cpu().numpy(), g[f"{name}_loss"], rtol=1e-5, atol=1e-6)
    assert np.allclose(items.cpu().numpy(), g[f"{name}_items"], rtol=1e-5, atol=1e-6)
    tcls, tbox, indices, anch, tcsl = cl.build_targets(pg, tg.to(dev))
    for i in range(case.nl):
        assert np.array_equal(torch.stack(indices[i], 1).cpu().numpy(), g[f"{name}_idx{i}"]), i
        assert np.array_equal(tbox[i].cpu().numpy(), g[f"{name}_tbox{i}"]), i
        gs = LC.group_sums(pg[i].grad.double().cpu(), case.nc)
        ref = g[f"{name}_gradsum{i}"]
        assert np.all(np.abs(gs - ref) <= 1e-4 * np.abs(ref[:, 1:2]) + 1e-9), (i, gs, ref)
