"""Logit regimes for the ComputeLoss tests beyond N(0,1): a trained head (background objectness around -6, class and CSL
logits strongly negative with peaks on the targets, size logits that never saturate low), the same head with 5 % of its logits
saturated at +-U(17, 90), four matched cells whose size logits are saturated LOW (a degenerate predicted box), and one
non-finite or largest-finite value planted into a small trained head.  Shared by tests/test_loss_regimes_host.py and
tests/test_loss_regimes_gpu.py; nothing here touches a GPU.

Every case starts from synth.s_loss, so the targets and the build_targets rows are the ones the other loss tests use; only the
logits are transformed (z is the N(0,1) logit s_loss drew for the element):

  trained         xy 2z; wh 0.5 + 1.5z with anything below -2 reflected to its negative ((2 sigmoid)^2 has to reach 0.25..4, a
                  trained head never saturates a size logit low); objectness -6 + 1.5z on the background and 2 + 2z on matched
                  cells; class -4 + 1.5z, +3 on the target class of a matched cell; CSL -5 + 2z, +2 on the bins where the label
                  of a target of the cell exceeds 0.5
  saturated       trained, then 5 % of the objectness, class, CSL and xy logits replaced by +-U(17, 90) and 5 % of the wh
                  logits by +U(17, 90) (high side only)
  degenerate_box  saturated, then four matched cells of level 0 get wh logits <= -17: one w only, one h only, two both
  nonfinite       trained at sizes (8, 4, 2) with ONE planted value (tests plant it after rounding the head to its dtype)
"""
from dataclasses import dataclass, field

import torch

from oracle import pyref
from tests import synth
from tests.loss_cases import groups

BS, NA, NC, NT = 2, 3, 16, 60
SIZES, SIZES_NONFINITE = (32, 16, 8), (8, 4, 2)
SEED = 3
SAT_LO, SAT_HI, SAT_FRAC = 17.0, 90.0, 0.05
TINY_BOX = 1e-3            # grid units: a decoded pw or ph below this makes the cell's box gradients exempt (degenerate_box)
DEGENERATE_WH = ((-17.0, None), (None, -20.0), (-30.0, -17.0), (-60.0, -88.0))     # (w logit, h logit) of the planted cells


@dataclass
class Regime:
    name: str
    nc: int
    hyp: dict
    p: list                     # float32 logits per level, (bs, na, ny, nx, 5 + nc + 180)
    t: torch.Tensor             # (nt, 187) targets
    cells: list                 # per level: (m, 4) int64 rows (b, a, gj, gi) of the matched cells, unique, in first-seen order
    planted: list = field(default_factory=list)       # degenerate_box: [(level, b, a, gj, gi)]

    @property
    def spec(self):
        return pyref.LossSpec(self.hyp, synth.grid_anchors(), torch.tensor(synth.DEFAULT_STRIDES), self.nc)


def _unique_rows(rows):
    seen, out = set(), []
    for r in rows.tolist():
        if tuple(r) not in seen:
            seen.add(tuple(r))
            out.append(r)
    return torch.tensor(out, dtype=torch.long).view(-1, 4)


def trained(seed=SEED, nc=NC, sizes=SIZES, hyp_over=None, crowd=False):
    """crowd: 30 targets moved into one cell, as tests/test_loss_gpu.py::test_sort_obj_iou does."""
    imgsz = 8 * sizes[0]
    hyp = synth.scaled_hyp(nc, imgsz)
    hyp.update(hyp_over or {})
    z, t = synth.s_loss(BS, nc, NT, seed, imgsz=imgsz, sizes=list(sizes))
    if crowd:
        t = t.clone()
        t[:30, 0] = 1
        t[:30, 2:4] = torch.tensor([40.2, 200.1]) * (imgsz / 256.0)
    reg = Regime("trained", nc, hyp, [], t, [])
    bt = pyref.build_targets(reg.spec, z, t)
    ci = 5 + nc
    for zi, r in zip(z, bt):
        x = torch.empty_like(zi)
        x[..., 0:2] = 2.0 * zi[..., 0:2]
        wh = 0.5 + 1.5 * zi[..., 2:4]
        x[..., 2:4] = torch.where(wh < -2.0, -wh, wh)
        x[..., 4] = -6.0 + 1.5 * zi[..., 4]
        x[..., 5:ci] = -4.0 + 1.5 * zi[..., 5:ci]
        x[..., ci:] = -5.0 + 2.0 * zi[..., ci:]
        b, a, gj, gi = r['b'], r['a'], r['gj'], r['gi']
        if b.numel():
            x[b, a, gj, gi, 4] = 2.0 + 2.0 * zi[b, a, gj, gi, 4]
            # assignments, not increments: a cell matched by several rows gets each bump once
            if nc > 1:
                x[b, a, gj, gi, 5 + r['tcls']] = -4.0 + 1.5 * zi[b, a, gj, gi, 5 + r['tcls']] + 3.0
            n_, k_ = (r['csl'] > 0.5).nonzero(as_tuple=True)
            x[b[n_], a[n_], gj[n_], gi[n_], ci + k_] = -5.0 + 2.0 * zi[b[n_], a[n_], gj[n_], gi[n_], ci + k_] + 2.0
        reg.p.append(x)
        reg.cells.append(_unique_rows(torch.stack((b, a, gj, gi), 1)))
    return reg


def saturated(seed=SEED, **kw):
    reg = trained(seed, **kw)
    reg.name = "saturated"
    g = torch.Generator().manual_seed(7000 + seed)
    for x in reg.p:
        pick = torch.rand(x.shape, generator=g) < SAT_FRAC
        mag = SAT_LO + (SAT_HI - SAT_LO) * torch.rand(x.shape, generator=g)
        sign = torch.where(torch.rand(x.shape, generator=g) < 0.5, -1.0, 1.0)
        sign[..., 2:4] = 1.0                                            # size logits: the high side only
        x[pick] = (sign * mag)[pick]
    return reg


def degenerate_box(seed=SEED, **kw):
    reg = saturated(seed, **kw)
    reg.name = "degenerate_box"
    cells = reg.cells[0]
    assert len(cells) >= 4 * 5
    for k, (w, h) in enumerate(DEGENERATE_WH):
        b, a, gj, gi = cells[5 * k].tolist()                           # spread over the level's matched cells
        if w is not None:
            reg.p[0][b, a, gj, gi, 2] = w
        if h is not None:
            reg.p[0][b, a, gj, gi, 3] = h
        reg.planted.append((0, b, a, gj, gi))
    return reg


FINITE = {"trained": trained, "saturated": saturated, "degenerate_box": degenerate_box}


def rounded(p, dtype):
    """The logits as the head dtype holds them, in float32: what the kernels read and what the oracle is given."""
    return [x.to(dtype).float() for x in p]


def exempt_masks(reg, p):
    """Per level a bool mask of p's shape: box channels 0..3 of the matched cells whose fp32-decoded pw or ph is below
    TINY_BOX grid units.  There the two edge terms of the CIoU gradient (order 1e6 each) cancel, and fp32 and fp64 torch
    disagree by 1e-2 of the group's maximum (fp32: exactly 0); only finiteness is compared."""
    out = []
    anchors = synth.grid_anchors()
    for i, (x, cells) in enumerate(zip(p, reg.cells)):
        m = torch.zeros(x.shape, dtype=torch.bool)
        if len(cells):
            b, a, gj, gi = cells.T
            pwh = (x[b, a, gj, gi, 2:4].float().sigmoid() * 2) ** 2 * anchors[i][a]
            bad = (pwh < TINY_BOX).any(1)
            m[b[bad], a[bad], gj[bad], gi[bad], 0:4] = True
        out.append(m)
    return out


# ----------------------------------------------------------------------------- non-finite plants
POSITIONS = ("bg_obj", "matched_obj", "matched_cls", "matched_csl", "matched_xy", "matched_wh")
VALUES = {"pinf": float("inf"), "ninf": float("-inf"), "nan": float("nan")}


def extreme_values(dtype):
    """+- the largest finite value of a 16-bit head dtype (fp16: 65504)."""
    m = torch.finfo(dtype).max
    return {"pmax": m, "nmax": -m}


_NF = {}


def nonfinite_base():
    if "reg" not in _NF:
        _NF["reg"] = trained(SEED, sizes=SIZES_NONFINITE)
        _NF["reg"].name = "nonfinite"
    return _NF["reg"]


def plant_index(reg, position):
    """(level, b, a, gj, gi, channel) of the planted element: level 0; the first matched cell, or the first cell no target
    row matched."""
    nc = reg.nc
    if position == "bg_obj":
        x = reg.p[0]
        free = torch.ones(x.shape[:4], dtype=torch.bool)
        b, a, gj, gi = reg.cells[0].T
        free[b, a, gj, gi] = False
        return (0, *free.nonzero()[0].tolist(), 4)
    b, a, gj, gi = reg.cells[0][0].tolist()
    if position == "matched_obj":
        ch = 4
    elif position == "matched_cls":
        r = pyref.build_targets(reg.spec, reg.p, reg.t)[0]
        hit = (torch.stack((r['b'], r['a'], r['gj'], r['gi']), 1) == reg.cells[0][0]).all(1).nonzero()[0, 0]
        ch = 5 + int(r['tcls'][hit])
    elif position == "matched_csl":
        ch = 5 + nc + 37
    elif position == "matched_xy":
        ch = 1
    elif position == "matched_wh":
        ch = 2
    else:
        raise KeyError(position)
    return (0, b, a, gj, gi, ch)


def planted(reg, position, value, dtype=torch.float32):
    """The head of `reg` rounded to dtype (as float32) with `value` at plant_index(reg, position), and that index."""
    p = [x.clone() for x in rounded(reg.p, dtype)]
    idx = plant_index(reg, position)
    p[idx[0]][idx[1:]] = value
    return p, idx


# ----------------------------------------------------------------------------- oracle runs and error figures
def oracle_run(reg, p, f64=False, sort_obj_iou=False, scale=1.0):
    """pyref.compute_loss on the given float32 logits (in double when f64) -> (loss, items, [gradient per level])."""
    dt = torch.float64 if f64 else torch.float32
    pc = [x.clone().to(dt).requires_grad_(True) for x in p]
    lo, io = pyref.compute_loss(reg.spec, pc, reg.t.clone(), sort_obj_iou=sort_obj_iou)
    (lo * scale).backward()
    return lo.detach(), io, [x.grad for x in pc]


def group_errors(ga, gb, nc, skip=None):
    """{group: max|ga - gb| / max|gb|} over the levels (the group's maximum taken per level, as check_grads does); elements
    under `skip` (per-level masks) are left out on both sides.  A level whose gb is all zero contributes nothing."""
    out = {k: 0.0 for k in groups(nc)}
    for i, (a, b) in enumerate(zip(ga, gb)):
        a, b = a.double(), b.double()
        if skip is not None:
            a, b = a.masked_fill(skip[i], 0.0), b.masked_fill(skip[i], 0.0)
        for name, sl in groups(nc).items():
            y = b[..., sl]
            scale = y.abs().max().item() if y.numel() else 0.0
            if scale > 0:
                out[name] = max(out[name], (a[..., sl] - y).abs().max().item() / scale)
    return out


# ----------------------------------------------------------------------------- the finite cases of the GPU module
@dataclass
class FiniteCase:
    id: str
    regime: str
    dtype: torch.dtype = torch.float32
    gamma: float = 0.0
    hyp: dict = field(default_factory=dict)
    nc: int = NC
    sort_obj_iou: bool = False        # with 30 targets moved into one cell
    csl7: bool = False                # the kernels get (nt, 7) targets; the oracle keeps the (nt, 187) rows
    scale: float = 1.0                # (loss * scale).backward() on both sides


DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
FINITE_CASES = [FiniteCase(f"{r}-{d}-g{g}", r, dt, g) for r in FINITE for d, dt in DTYPES.items() for g in (0.0, 1.5)]
FINITE_CASES += [
    FiniteCase("saturated-f32-smooth_pw", "saturated", hyp=dict(label_smoothing=0.1, cls_pw=1.7, theta_pw=0.6, obj_pw=2.2)),
    FiniteCase("saturated-f32-sort_obj_iou", "saturated", sort_obj_iou=True),
    FiniteCase("saturated-f32-nc1", "saturated", nc=1),
    FiniteCase("saturated-f32-csl7", "saturated", csl7=True),
    FiniteCase("trained-f16-scale65536", "trained", torch.float16, scale=65536.0),      # GradScaler's initial scale
]
FINITE_BY_ID = {c.id: c for c in FINITE_CASES}
E_REF_MAX = 2e-6          # admission: a fifth of the 1e-5 contract (tests/test_loss_regimes_host.py)
_REF = {}


@dataclass
class Reference:
    reg: Regime
    p: list               # the dtype-rounded logits, float32
    l32: torch.Tensor
    i32: torch.Tensor
    g32: list
    l64: torch.Tensor
    i64: torch.Tensor
    g64: list
    exempt: list          # per-level masks (all False outside degenerate_box)
    e_ref: dict           # per group max|g32 - g64| / max|g64| outside the exempt set


def reference(case):
    """The fp32 and fp64 oracle results of a finite case, computed once per process and left unchanged."""
    if case.id not in _REF:
        hyp = dict(case.hyp)
        hyp["fl_gamma"] = case.gamma
        reg = FINITE[case.regime](SEED, nc=case.nc, hyp_over=hyp, crowd=case.sort_obj_iou)
        p = rounded(reg.p, case.dtype)
        l32, i32, g32 = oracle_run(reg, p, False, case.sort_obj_iou, case.scale)
        l64, i64, g64 = oracle_run(reg, p, True, case.sort_obj_iou, case.scale)
        ex = exempt_masks(reg, p)
        _REF[case.id] = Reference(reg, p, l32, i32, g32, l64, i64, g64, ex, group_errors(g32, g64, reg.nc, skip=ex))
    return _REF[case.id]


# ----------------------------------------------------------------------------- the non-finite cases
def nonfinite_cases():
    """[(id, position, value name, value, head dtype)]: fp32 heads get +-inf and NaN, the 16-bit heads +- their largest finite
    value, at each of the six positions."""
    out = []
    for pos in POSITIONS:
        for vn, v in VALUES.items():
            out.append((f"f32-{pos}-{vn}", pos, vn, v, torch.float32))
        for d in ("f16", "bf16"):
            for vn, v in extreme_values(DTYPES[d]).items():
                out.append((f"{d}-{pos}-{vn}", pos, vn, v, DTYPES[d]))
    return out


def nonfinite_expectation(position, vn):
    """What the reference does with the planted value (pinned against the oracle by tests/test_loss_regimes_host.py):
    (indices of the non-finite loss items among lbox, lobj, lcls, ltheta; channels of the planted cell whose gradient is
    non-finite).  The total loss is non-finite exactly when an item is; no other gradient element is non-finite.
    +-inf in a box logit only saturates the sigmoid; an infinite logit of a BCE term makes that term inf or NaN but its
    gradient (sigmoid - t) stays finite; a NaN box logit reaches lbox, through iou.detach().clamp(0) the objectness target
    of the cell, and with it lobj and the cell's channels 0..4."""
    item = {"bg_obj": 1, "matched_obj": 1, "matched_cls": 2, "matched_csl": 3}
    if vn in ("pmax", "nmax"):
        return (), ()
    if position in item:
        return (item[position],), ((-1,) if vn == "nan" else ())          # -1: the planted channel itself
    return ((0, 1), (0, 1, 2, 3, 4)) if vn == "nan" else ((), ())
