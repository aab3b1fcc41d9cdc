"""CPU: what makes tests/test_loss_regimes_gpu.py trustworthy.  The GPU module compares the kernels with the fp32 oracle
(oracle/pyref.py) at 1e-5 of each channel group's largest gradient, on logits far outside N(0,1) (tests/loss_regimes.py).  That
is only a fair bar where the fp32 oracle itself is close to the true value, so every finite case is ADMITTED here first: the
oracle runs in fp32 and in fp64 on the same (dtype-rounded) logits and, per channel group,

    E_ref = max|g32 - g64| / max|g64|  <=  2e-6          (a fifth of the 1e-5 contract)

Measured (seeds 3, 4, 5; emitted by test_zz_report_e_ref): E_ref <= 7.4e-7 in every group of every case.  Size logits
saturated LOW do not pass (one box-gradient element 1e-2 of the group's maximum off: fp32 gives exactly 0 where fp64 gives
4.5e-6, two edge terms of the CIoU gradient of order 1e6 cancel when w = h = 0), which is why `degenerate_box` carries an exempt set, pinned here to exactly its 16 planted
elements.  The oracle's non-finite pattern of every `nonfinite` case is pinned too, so that a torch upgrade that changes it is
noticed here and not on the GPU."""
import warnings

import pytest
import torch

from tests import loss_regimes as LR
from tests.loss_cases import groups


E_REF = {}          # case id -> {group: E_ref}, emitted by test_zz_report_e_ref


@pytest.mark.parametrize("cid", [c.id for c in LR.FINITE_CASES])
def test_finite_cases_are_admitted(cid):
    ref = LR.reference(LR.FINITE_BY_ID[cid])
    E_REF[cid] = ref.e_ref
    print(f"E_ref {cid}: " + ", ".join(f"{k} {v:.1e}" for k, v in ref.e_ref.items()))
    assert all(torch.isfinite(g).all() for g in ref.g32 + ref.g64) and torch.isfinite(ref.l32) and torch.isfinite(ref.l64)
    for k, v in ref.e_ref.items():
        assert v <= LR.E_REF_MAX, (cid, k, v)
    # every level has matched cells and, at nc > 1, every group a gradient: the group maxima above are not vacuous
    for i, g in enumerate(ref.g64):
        for k, sl in groups(ref.reg.nc).items():
            assert (g[..., sl].abs().max() > 0) == (k != "cls" or ref.reg.nc > 1), (cid, i, k)


@pytest.mark.parametrize("regime", list(LR.FINITE))
@pytest.mark.parametrize("seed", [4, 5])
def test_admission_holds_on_other_seeds(regime, seed):
    """The margin under 2e-6 is not a property of seed 3."""
    for gamma in (0.0, 1.5):
        reg = LR.FINITE[regime](seed, hyp_over=dict(fl_gamma=gamma))
        _, _, g32 = LR.oracle_run(reg, reg.p)
        _, _, g64 = LR.oracle_run(reg, reg.p, f64=True)
        e = LR.group_errors(g32, g64, reg.nc, skip=LR.exempt_masks(reg, reg.p))
        E_REF[f"{regime}-f32-g{gamma}-seed{seed}"] = e
        print(f"E_ref {regime} seed {seed} gamma {gamma}: " + ", ".join(f"{k} {v:.1e}" for k, v in e.items()))
        assert max(e.values()) <= LR.E_REF_MAX, (regime, seed, gamma, e)


def test_regimes_are_what_they_claim():
    tr, sa = LR.trained(), LR.saturated()
    for reg in (tr, sa):
        for x, cells in zip(reg.p, reg.cells):
            assert len(cells) > 0
            assert x[..., 2:4].min() >= -2.0                             # no size logit saturated low
    bg = tr.p[0][..., 4].clone()
    b, a, gj, gi = tr.cells[0].T
    on = bg[b, a, gj, gi]
    bg[b, a, gj, gi] = float("nan")
    assert -6.2 < bg[~bg.isnan()].mean() < -5.8 and 1.5 < on.mean() < 2.5
    assert tr.p[0].abs().max() < 17.0
    for x in sa.p:
        frac = (x.abs() >= LR.SAT_LO).float().mean().item()
        assert 0.045 < frac < 0.055, frac
        assert x.abs().max() <= LR.SAT_HI and (x[..., 2:4] > LR.SAT_LO).any() and (x[..., 4] < -LR.SAT_LO).any()


@pytest.mark.parametrize("dtype", list(LR.DTYPES))
def test_degenerate_box_exempt_set_is_the_16_planted_elements(dtype):
    reg = LR.degenerate_box()
    p = LR.rounded(reg.p, LR.DTYPES[dtype])
    masks = LR.exempt_masks(reg, p)
    want = [torch.zeros_like(m) for m in masks]
    assert len(reg.planted) == 4 and len(set(reg.planted)) == 4
    for lv, b, a, gj, gi in reg.planted:
        want[lv][b, a, gj, gi, 0:4] = True
    assert sum(int(m.sum()) for m in masks) == 16
    assert all(torch.equal(m, w) for m, w in zip(masks, want))
    wh = torch.stack([p[lv][b, a, gj, gi, 2:4] for lv, b, a, gj, gi in reg.planted])
    low = wh <= -LR.SAT_LO
    assert low.tolist() == [[True, False], [False, True], [True, True], [True, True]]
    # why the set exists: outside it the fp32 oracle is admitted, inside it fp32 and fp64 disagree (recorded, not asserted)
    _, _, g32 = LR.oracle_run(reg, p)
    _, _, g64 = LR.oracle_run(reg, p, f64=True)
    scale = g64[0][..., 0:4].abs().max().item()
    worst = ((g32[0].double() - g64[0]).abs() * masks[0]).max().item() / scale
    print(f"degenerate_box {dtype}: largest |g32 - g64| / max|g64| inside the exempt set {worst:.1e}")
    assert torch.isfinite(g32[0][masks[0]]).all() and torch.isfinite(g64[0][masks[0]]).all()


def _pattern(reg, p, f64):
    loss, items, grads = LR.oracle_run(reg, p, f64=f64)
    return bool(torch.isfinite(loss).all()), torch.isfinite(items).tolist(), [torch.isfinite(g) for g in grads]


@pytest.mark.parametrize("cid,position,vn,value,dtype", LR.nonfinite_cases(), ids=[c[0] for c in LR.nonfinite_cases()])
def test_oracle_nonfinite_pattern_is_pinned(cid, position, vn, value, dtype):
    """isfinite of the loss, of the four items and of every gradient element, in fp32 and in fp64, against the table in
    tests/loss_regimes.py::nonfinite_expectation."""
    reg = LR.nonfinite_base()
    p, idx = LR.planted(reg, position, value, dtype)
    bad_items, bad_ch = LR.nonfinite_expectation(position, vn)
    want_items = [k not in bad_items for k in range(4)]
    want_masks = [torch.ones(x.shape, dtype=torch.bool) for x in p]
    for ch in bad_ch:
        want_masks[idx[0]][idx[1:5] + (idx[5] if ch < 0 else ch,)] = False
    for f64 in (False, True):
        loss_ok, items_ok, masks = _pattern(reg, p, f64)
        assert items_ok == want_items, (cid, f64, items_ok)
        assert loss_ok == all(want_items), (cid, f64)
        for i, (m, w) in enumerate(zip(masks, want_masks)):
            assert torch.equal(m, w), (cid, f64, i, (m != w).nonzero().tolist())


def test_the_two_results_the_gpu_module_rests_on():
    """A NaN size logit at a matched cell: items [nan, nan, finite, finite] and five NaN gradient elements on that level (the
    cell's channels 0..4: the objectness target iou.detach().clamp(0) propagates the NaN).  +inf background objectness: loss
    inf with every gradient finite."""
    reg = LR.nonfinite_base()
    p, idx = LR.planted(reg, "matched_wh", float("nan"))
    loss, items, grads = LR.oracle_run(reg, p)
    assert torch.isnan(loss).all() and torch.isnan(items).tolist() == [True, True, False, False]
    assert torch.isfinite(items[2:]).all()
    bad = torch.isnan(grads[0]).nonzero().tolist()
    assert bad == [list(idx[1:5]) + [ch] for ch in range(5)]
    assert all(torch.isfinite(g).all() for g in grads[1:])
    p, idx = LR.planted(reg, "bg_obj", float("inf"))
    loss, items, grads = LR.oracle_run(reg, p)
    assert torch.isinf(loss).all() and loss.item() > 0 and torch.isinf(items[1])
    assert all(torch.isfinite(g).all() for g in grads)


def test_zz_report_e_ref():
    """Not a check of its own: E_ref of every case admitted in this run, in the warnings summary."""
    lines = [f"{cid}: " + ", ".join(f"{k} {v:.1e}" for k, v in e.items()) for cid, e in E_REF.items()]
    worst = max((v for e in E_REF.values() for v in e.values()), default=0.0)
    warnings.warn(UserWarning(f"E_ref = max|g32 - g64| / max|g64| per channel group (admission limit {LR.E_REF_MAX:.0e}, worst "
                              f"{worst:.1e}):\n  " + "\n  ".join(lines)))
