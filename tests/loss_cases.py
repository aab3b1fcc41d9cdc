"""Head configurations and planted targets for the ComputeLoss tests across the shapes the C ABI accepts
(include/obb_hip.h: nl <= 8, na <= 8, 1 <= nc <= 256, any ny, nx, bs).  Shared by tests/test_loss_configs_gpu.py,
tests/test_loss_configs_host.py and tests/golden/gen_loss_configs.py; nothing here touches a GPU."""
import math
from dataclasses import dataclass, field

import numpy as np
import torch

from oracle import pyref
from tests import synth

CSL = 180
ANCHOR_T = 4.0          # hyp['anchor_t'] of synth.HYP_DOTA


@dataclass
class Case:
    name: str
    nl: int
    na: int
    nc: int
    sizes: list          # (ny, nx) per level
    bs: int
    nt: int
    half: bool = False
    sort_obj_iou: bool = False
    csl7: bool = False            # (nt, 7) targets: the CSL rows are regenerated on the device from theta
    hyp: dict = field(default_factory=dict)
    autobalance: bool = False
    seed: int = 0

    @property
    def no(self):
        return 5 + self.nc + CSL

    def rows(self, i):
        ny, nx = self.sizes[i]
        return self.bs * self.na * ny * nx

    def tail(self, i):
        """The last 64-row region of level i ends in a partial 16-byte vector (k_loss_bwd_dense's scalar tail loop)."""
        nr = self.rows(i) % 64 or 64
        return (nr * self.no) % (8 if self.half else 4) != 0


def _c(name, nl, na, nc, sizes, bs, nt, **kw):
    assert len(sizes) == nl, name
    return Case(name, nl, na, nc, [tuple(s) for s in sizes], bs, nt, **kw)


# Pairwise over nl x na x nc x grid x bs x dtype x flags, not the full product.  Large nc goes with small grids (the oracle
# materialises the whole head on the CPU).  nc values are the crossings of no = 5 + nc + 180 over 192 / 256 / 320 / 384
# (the wave's 64-channel chunks) plus 1, 2 and the maximum.
CASES = [
    _c("nl1_na1_nc1", 1, 1, 1, [(20, 13)], 3, 40),
    _c("nl1_na8_nc256", 1, 8, 256, [(5, 7)], 1, 30),
    _c("nl1_na3_nc200_bs16", 1, 3, 200, [(7, 5)], 16, 120, half=True),
    _c("nl1_na2_nc8_sort", 1, 2, 8, [(13, 20)], 16, 150, sort_obj_iou=True),
    _c("nl2_na2_nc2_f16", 2, 2, 2, [(13, 20), (7, 10)], 3, 60, half=True),
    _c("nl2_na4_nc72_sort", 2, 4, 72, [(20, 13), (10, 7)], 1, 50, sort_obj_iou=True),
    _c("nl2_na8_nc199", 2, 8, 199, [(6, 9), (3, 5)], 3, 40, hyp=dict(fl_gamma=1.5)),
    _c("nl2_na3_nc135_f16", 2, 3, 135, [(9, 9), (5, 5)], 1, 40, half=True, hyp=dict(fl_gamma=2.0)),
    _c("nl3_na1_nc7_bs16", 3, 1, 7, [(24, 16), (12, 8), (6, 4)], 16, 200),
    _c("nl3_na3_nc8_f16_focal", 3, 3, 8, [(17, 11), (9, 6), (5, 3)], 3, 80, half=True, hyp=dict(fl_gamma=1.5)),
    _c("nl3_na4_nc135_csl7", 3, 4, 135, [(9, 15), (5, 8), (3, 4)], 3, 60, csl7=True),
    _c("nl3_na8_nc136_1x1", 3, 8, 136, [(8, 8), (4, 4), (1, 1)], 1, 40),
    _c("nl3_na3_nc18_dota2", 3, 3, 18, [(16, 24), (8, 12), (4, 6)], 3, 120, hyp=dict(label_smoothing=0.1)),
    _c("nl3_na2_nc256_f16_sort", 3, 2, 256, [(11, 7), (6, 4), (3, 2)], 3, 50, half=True, sort_obj_iou=True),
    _c("nl3_na3_nc1_smooth", 3, 3, 1, [(15, 9), (8, 5), (4, 3)], 1, 50, hyp=dict(label_smoothing=0.1)),
    _c("nl4_na3_nc199_autobalance", 4, 3, 199, [(12, 20), (6, 10), (3, 5), (2, 3)], 1, 60, autobalance=True),
    _c("nl4_na4_nc200", 4, 4, 200, [(20, 12), (10, 6), (5, 3), (3, 2)], 3, 60),
    _c("nl4_na1_nc71_f16_bs16", 4, 1, 71, [(16, 16), (8, 8), (4, 4), (2, 2)], 16, 150, half=True),
    _c("nl4_na8_nc7_csl7", 4, 8, 7, [(8, 4), (4, 2), (2, 1), (1, 1)], 3, 50, csl7=True, hyp=dict(label_smoothing=0.2)),
    _c("nl4_na2_nc1_f16_autobalance", 4, 2, 1, [(10, 14), (5, 7), (3, 4), (2, 2)], 3, 60, half=True, autobalance=True),
    _c("nl5_na2_nc256", 5, 2, 256, [(8, 12), (4, 6), (2, 3), (1, 2), (1, 1)], 1, 40),
    _c("nl5_na3_nc1", 5, 3, 1, [(13, 13), (7, 7), (4, 4), (2, 2), (1, 1)], 3, 60, sort_obj_iou=True),
    _c("nl5_na4_nc136_bs16_f16", 5, 4, 136, [(6, 4), (3, 2), (2, 1), (1, 1), (1, 1)], 16, 120, half=True, csl7=True),
    _c("nl5_na8_nc72", 5, 8, 72, [(9, 7), (5, 4), (3, 2), (2, 1), (1, 1)], 3, 50, hyp=dict(fl_gamma=2.0, label_smoothing=0.1)),
    _c("nl8_na1_nc2_rows1", 8, 1, 2, [(32, 24), (16, 12), (8, 6), (4, 3), (2, 2), (1, 1), (1, 1), (1, 1)], 1, 80),
    _c("nl8_na8_nc8_f16", 8, 8, 8, [(8, 8), (4, 4), (2, 2), (1, 1), (1, 1), (1, 1), (1, 1), (1, 1)], 3, 60, half=True,
       sort_obj_iou=True),
    _c("nl8_na2_nc71", 8, 2, 71, [(12, 9), (6, 5), (3, 3), (2, 2), (1, 1), (1, 1), (1, 1), (1, 1)], 3, 60, csl7=True),
    _c("nl8_na4_nc200_bs16", 8, 4, 200, [(4, 6), (2, 3), (1, 2), (1, 1), (1, 1), (1, 1), (1, 1), (1, 1)], 16, 80,
       hyp=dict(fl_gamma=1.5)),
]
for _i, _k in enumerate(CASES):
    _k.seed = 1000 + 17 * _i
BY_NAME = {k.name: k for k in CASES}


def head(case):
    """(anchors in grid units (nl, na, 2), anchors in pixels, strides)."""
    apx, st = synth.head_anchors(case.nl, case.na)
    return apx / st.view(-1, 1, 1), apx, st


def balance_of(case):
    """ComputeLoss's own default for nl <= 5 (utils/loss.py:114); nl = 8 needs an explicit list of 8."""
    return None if case.nl <= 5 else [4.0, 1.0, 0.25, 0.06, 0.02, 0.01, 0.005, 0.0025]


def hyp_of(case):
    ny, nx = case.sizes[0]
    h = synth.scaled_hyp(case.nc, int(nx * 8), case.nl)
    h.update(case.hyp)
    return h


def spec_of(case):
    ag, _, st = head(case)
    return pyref.LossSpec(hyp_of(case), ag, st, case.nc, balance=balance_of(case))


def random_inputs(case):
    """Head logits and random targets whose sizes are drawn around the head's own anchors."""
    _, apx, st = head(case)
    imgsz = case.sizes[0][1] * float(st[0])
    p, t = synth.s_loss(case.bs, case.nc, case.nt, case.seed, imgsz=imgsz, sizes=case.sizes, na=case.na, anchors=apx)
    return p, t


def _ratio_sizes(anchor, st, want, inverse):
    """Pixel lengths L (float32) around anchor_t: the oracle's ratio v = r = (L / stride) / anchor (inverse: v = 1 / r), in
    float32 arithmetic, is exactly `want` for one of them, the nearest value below `want` that v can take for another
    (want - 1 ulp where it is reachable), the nearest above for the third.  [(L, v)] in that order."""
    f = np.float32
    a, s = f(anchor), f(st)
    base = f((1.0 / want if inverse else want) * float(a) * float(s))
    Ls = [base]
    lo = hi = base
    for _ in range(256):
        lo, hi = np.nextafter(lo, f(0)), np.nextafter(hi, f(np.inf))
        Ls += [lo, hi]
    vals = []
    for L in Ls:
        r = f(f(L / s) / a)
        vals.append((f(f(1) / r) if inverse else r, L))
    eq = [(v, L) for v, L in vals if v == f(want)]
    below = max((x for x in vals if x[0] < f(want)), key=lambda x: x[0])
    above = min((x for x in vals if x[0] > f(want)), key=lambda x: x[0])
    assert eq, (anchor, st, want, inverse)
    return [(L, v) for v, L in (below, eq[0], above)]


def planted_targets(case, seed=0):
    """(nt, 187) targets that sit on the edges of build_targets (utils/loss.py:229-272) at every level of the case:
    centres at exact cell corners and half cells, 1.0, nx - 1, nx, 0, slightly negative and beyond the grid; (l, s) at
    exactly anchor_t times the anchor and one ulp either side, on both sides of the ratio; l = 0, s = 0 and NaN sizes; the
    last image and the last class; theta at +-pi/2, 0, just above 0 (90 - angle in (-1, 0)) and where |int(90 - angle)| > 180;
    and a crowd of targets in one cell across anchors, with exact duplicates (CIoU ties)."""
    ag, apx, st = head(case)
    rng = np.random.RandomState(seed + case.seed)
    rows = []

    def row(b, c, x, y, l, s, th):
        rows.append([float(b), float(c), float(x), float(y), float(l), float(s), float(th)])

    thetas = [math.pi / 2, -math.pi / 2, 0.0, 0.004, -0.004, 3.5, -3.5, float(np.float32(-pyref.PI)), 1.2, -0.7]
    last_b, last_c = case.bs - 1, case.nc - 1
    for i in range(case.nl):
        ny, nx = case.sizes[i]
        s_ = float(st[i])
        a = int(rng.randint(case.na))
        L, S = float(apx[i, a, 0]), float(apx[i, a, 1])            # ratio 1 to anchor a of this level
        ks = sorted({0, min(1, nx - 1), nx // 2, nx - 1})
        gxs = [0.0, -0.25, -1.5, 1.0, float(np.nextafter(np.float32(1), np.float32(2))), float(nx - 1), float(nx),
               nx + 2.3, float(nx) - 1.5, float(nx) - 0.5] + [k + d for k in ks for d in (0.0, 0.5, 0.25, 0.75)]
        gys = [0.0, -0.25, -1.5, 1.0, float(ny - 1), float(ny), ny + 2.3, float(ny) - 1.5, float(ny) - 0.5, 0.5, 1.5]
        gys += [float(rng.randint(ny)) + d for d in (0.0, 0.5)]
        for j, gx in enumerate(gxs):
            gy = gys[j % len(gys)]
            row(last_b if j % 3 == 0 else rng.randint(case.bs), last_c if j % 4 == 0 else rng.randint(case.nc),
                gx * s_, gy * s_, L, S, thetas[j % len(thetas)])
        for j, gy in enumerate(gys):
            gx = gxs[(3 * j + 1) % len(gxs)]
            row(rng.randint(case.bs), last_c if j % 2 else 0, gx * s_, gy * s_, L, S, thetas[(j + 3) % len(thetas)])
        # ratios exactly at anchor_t and one ulp either side, on l and on s, as r and as 1 / r
        cx, cy = (nx * 0.37 + 0.1) * s_, (ny * 0.61 + 0.1) * s_
        for side in (0, 1):
            for inverse in (False, True):
                for Lx, _ in _ratio_sizes(apx[i, a, side] / s_, s_, ANCHOR_T, inverse):
                    l_, sz = (float(Lx), S) if side == 0 else (L, float(Lx))
                    row(rng.randint(case.bs), rng.randint(case.nc), cx, cy, l_, sz, 0.3)
        # degenerate sizes: filtered by the ratio test (NaN as with torch's NaN-propagating max)
        for l_, sz in ((0.0, S), (L, 0.0), (float('nan'), S), (L, float('nan')), (0.0, 0.0)):
            row(rng.randint(case.bs), rng.randint(case.nc), cx, cy, l_, sz, 0.1)
        # a crowd in one cell across anchors, with exact duplicates; every anchor of the level gets a target of its own size
        gx, gy = (min(2, nx - 1) + 0.3) * s_, (min(2, ny - 1) + 0.7) * s_
        b = rng.randint(case.bs)
        for k in range(case.na):
            for rep in range(2):
                row(b, rng.randint(case.nc), gx, gy, float(apx[i, k, 0]), float(apx[i, k, 1]), 0.2 * k)
        row(b, 0, gx + 0.05 * s_, gy - 0.05 * s_, L * 1.3, S * 0.8, -0.4)
        row(b, 0, gx + 0.05 * s_, gy - 0.05 * s_, L * 1.3, S * 0.8, -0.4)
    t7 = torch.tensor(rows, dtype=torch.float32)
    return with_csl(t7)


def with_csl(t7):
    """(nt, 7) -> (nt, 187): the dataloader's CSL rows from theta, as synth.s_loss makes them (gaussian_label_cpu, radius 2)."""
    ang = t7[:, 6].double().numpy() * 180 / pyref.PI + 90
    csl = np.stack([pyref.gaussian_label(a, CSL, 0, 2.0) for a in ang]) if len(ang) else np.zeros((0, CSL))
    return torch.cat((t7, torch.from_numpy(csl).float()), 1)


def nc1_class3_inputs():
    """nc = 1 with targets of class 0 and of class 3: the reference never indexes by class when nc == 1, so its loss is
    finite (regression: the kernels flagged cls >= nc as a bad row for every nc and returned NaN)."""
    case = _c("nc1_class3", 3, 3, 1, [(16, 12), (8, 6), (4, 3)], 2, 40, seed=77)
    p, t = random_inputs(case)
    t[::2, 1] = 3.0
    t[1::4, 1] = 0.0
    return case, p, t


# The configurations frozen from the reference's own utils/loss.py by tests/golden/gen_loss_configs.py
# (name -> (case, target kind)); "planted" uses planted_targets(case).
FIXTURE = {
    "nl4_na4_nc200": (BY_NAME["nl4_na4_nc200"], "random"),
    "nc1_class3": (None, "nc1_class3"),
    "nl1_na8_nc256": (BY_NAME["nl1_na8_nc256"], "random"),
    "nl1_na1_nc1": (BY_NAME["nl1_na1_nc1"], "random"),
    "nl3_na4_nc135_planted": (BY_NAME["nl3_na4_nc135_csl7"], "planted"),
    "nl5_na2_nc256_planted": (BY_NAME["nl5_na2_nc256"], "planted"),
    "nl2_na8_nc199": (BY_NAME["nl2_na8_nc199"], "random"),
}


def fixture_inputs(name):
    case, kind = FIXTURE[name]
    if kind == "nc1_class3":
        return nc1_class3_inputs()
    p, t = random_inputs(case)
    if kind == "planted":
        t = planted_targets(case)
    return case, p, t


def groups(nc):
    """Channel groups of a prediction row: box 0-3, objectness 4, class 5:5+nc, CSL 5+nc:."""
    return {"box": slice(0, 4), "obj": slice(4, 5), "cls": slice(5, 5 + nc), "csl": slice(5 + nc, None)}


def group_sums(grad, nc):
    """(4, 2) float64: per channel group (box, obj, cls, csl) the sum of the gradient and the sum of its magnitudes."""
    g = grad.double()
    return np.array([[g[..., sl].sum().item(), g[..., sl].abs().sum().item()] for sl in groups(nc).values()])
