"""Head configurations for the Detect decode / lazy NMS tests across the shapes the C ABI accepts (include/obb_hip.h:
obb_detect_decode*, obb_non_max_suppression_obb_head: nl 1..4, na 1..8, nc 1..256).  Shared by tests/test_head_configs_host.py,
tests/test_head_configs_gpu.py and tests/golden/gen_head_configs.py; nothing here touches a GPU.

decode_ref is an independent restatement of the inference branch of the reference's Detect.forward (models/yolo.py:71-79) in
numpy float64, with the fp16 roundings placed where the reference's tensor dtypes force them."""
import functools
from dataclasses import dataclass

import numpy as np
import torch

from tests import synth

CSL = 180
KW = dict(conf_thres=0.25, iou_thres=0.45, max_det=300)      # the NMS arguments of every test on these heads
# Class / angle background logits: multiples of 1 / LATTICE (exact in fp16), nine in ten close to -5 and one in ten anywhere in
# [-12, 12] -- every regime of the sigmoid occurs thousands of times, and the 32 rows per case that the fixture stores in full
# still compress to under 100 KB
LATTICE, WIDE, NARROW = 4.0, 0.1, 0.25


@dataclass(frozen=True)
class Case:
    name: str
    nl: int
    na: int
    nc: int
    sizes: tuple         # (ny, nx) per level
    bs: int
    seed: int = 0

    @property
    def no(self):
        return 5 + self.nc + CSL

    @property
    def level_rows(self):
        return [self.na * ny * nx for ny, nx in self.sizes]

    @property
    def a_total(self):
        return sum(self.level_rows)


def _c(name, nl, na, nc, sizes, bs):
    assert len(sizes) == nl, name
    return name, nl, na, nc, tuple(tuple(s) for s in sizes), bs


# Pairwise over nl x na x nc x maps x bs, not the full product; large nc goes with tiny maps.  What each case is for:
#   1x1            a map smaller than any 16-byte vector
#   nc256_vec      no = 441: maximum LDS (113 KB decode, 115 + 21 KB head front), vector path (HW = 40)
#   nc256_odd      no = 441 on the element-wise store walker, where NT / no = 0
#   nc71 / nc72    no = 256 / 257: either side of the walker's regime change
#   nc6 / nc7      fp32 decode LDS 49,096 / 49,360 bytes: either side of the 48 KB opt-in
#   straddle       HW = 180 (two full 64-position tiles + 52, vector path), 182 (element-wise), 12; nx does not divide 64
#   hw12           no = 218 even, HW = 12: the fp16 decode is vectorised, the fp16 head front (HW % 8 != 0) element-wise
#   p6             four levels, eight anchors, bs 3
#   1x1tail        the last level (HW = 1) takes the all-levels launch off the vector path
#   bs16           grid.y = bs * na with many images
_CASES = [
    _c("nl1_na1_nc1_1x1", 1, 1, 1, [(1, 1)], 2),
    _c("nl1_na8_nc256_vec", 1, 8, 256, [(5, 8)], 1),
    _c("nl1_na8_nc256_odd", 1, 8, 256, [(5, 7)], 2),
    _c("nl2_na2_nc71", 2, 2, 71, [(9, 8), (4, 4)], 2),
    _c("nl2_na2_nc72", 2, 2, 72, [(9, 8), (4, 4)], 2),
    _c("nl2_na4_nc6", 2, 4, 6, [(7, 9), (4, 4)], 2),
    _c("nl2_na4_nc7", 2, 4, 7, [(7, 9), (4, 4)], 2),
    _c("nl3_na3_nc16_straddle", 3, 3, 16, [(9, 20), (13, 14), (3, 4)], 2),
    _c("nl3_na5_nc33_hw12", 3, 5, 33, [(6, 6), (3, 4), (2, 2)], 2),
    _c("nl4_na8_nc18_p6", 4, 8, 18, [(16, 12), (8, 6), (4, 3), (2, 2)], 3),
    _c("nl4_na1_nc200_1x1tail", 4, 1, 200, [(8, 8), (4, 4), (2, 2), (1, 1)], 2),
    _c("nl3_na2_nc2_bs16", 3, 2, 2, [(8, 16), (4, 8), (2, 4)], 16),
]
CASES = [Case(*c, seed=4000 + 13 * i) for i, c in enumerate(_CASES)]
BY_NAME = {k.name: k for k in CASES}
NAMES = [k.name for k in CASES]


def strides(case):
    return [8.0 * 2 ** i for i in range(case.nl)]


def anchors_px(case):
    """(nl, na, 2) float32 anchors in pixels, pairwise distinct over (level, anchor, axis): a swapped or mis-strided table entry
    changes the output.  In grid units (anchor / stride, what Detect.anchors holds) every entry is exact in fp16, so a Detect
    module cast to half keeps the same table.  The P6 case takes the first three anchors of every level from synth.P6_ANCHORS."""
    st = np.asarray(strides(case), np.float32)
    g = np.zeros((case.nl, case.na, 2), np.float32)                # grid units
    for l in range(case.nl):
        for k in range(case.na):
            j = l * 8 + k                      # an odd / even 256th on top: no two entries of the table are equal
            g[l, k] = (1.25 + 0.375 * k + (2 * j + 1) / 256.0, 0.75 + 0.3125 * k + (2 * j + 2) / 256.0)
    if case.nl == 4 and case.na == 8:
        assert st.tolist() == synth.P6_STRIDES
        g[:, :3] = np.asarray(synth.P6_ANCHORS, np.float32).reshape(4, 3, 2) / st[:, None, None]
        for k in range(3, 8):                  # five more per level, from the level's largest anchor, on a 1/32 lattice
            g[:, k, 0] = np.round(g[:, 2, 0] * (1.0 + 0.125 * (k - 2)) * 32.0) / 32.0 + k / 32.0
            g[:, k, 1] = np.round(g[:, 2, 1] * (1.0 - 0.0625 * (k - 2)) * 32.0) / 32.0 + (k + 8) / 32.0
    assert np.array_equal(g.astype(np.float16).astype(np.float32), g), case.name
    a = g * st[:, None, None]
    assert len(set(a.reshape(-1).tolist())) == a.size, case.name
    assert float(a.max()) * 4.0 < 65504.0            # the widest box (y = 1) is finite in fp16
    return a


def detect_anchor_arg(case):
    """Anchors as a model yaml lists them (the constructor argument of Detect): nl lists of na * 2 pixel values."""
    return anchors_px(case).reshape(case.nl, -1).tolist()


# ------------------------------------------------------------------ inputs
def _planted(rng, case, no):
    """One confident cell: the objectness, one to three classes and two equal CSL bins; small boxes (they do not suppress one
    another), and now and then a logit of 12 (the sigmoid rounds to 1 in fp16)."""
    cell = np.empty(no)
    cell[0:2] = np.clip(rng.normal(0.0, 4.0, 2), -12.0, 12.0)
    cell[2:4] = rng.uniform(-2.5, -1.0, 2)
    cell[4] = 12.0 if rng.random() < 0.15 else rng.uniform(0.5, 5.0)
    cell[5:] = np.round(np.clip(rng.normal(-6.0, 2.0, no - 5), -12.0, -1.5) * LATTICE) / LATTICE
    for c in rng.choice(case.nc, size=min(case.nc, int(rng.integers(1, 4))), replace=False):
        cell[5 + c] = 12.0 if rng.random() < 0.15 else rng.uniform(0.5, 4.0)
    ang = int(rng.integers(0, CSL))
    cell[5 + case.nc + ang] = 4.0
    cell[5 + case.nc + (ang + 1) % CSL] = 4.0                    # two equal bins: the first maximum decides
    return cell


@functools.lru_cache(maxsize=None)
def _convs64(name):
    """The conv outputs in float64 as (bs, na, ny, nx, no) per level, before the cast to the tensor dtype."""
    case = BY_NAME[name]
    rng = np.random.default_rng(case.seed)
    bs, na, nc, no = case.bs, case.na, case.nc, case.no
    lv = []
    for ny, nx in case.sizes:
        x = np.empty((bs, na, ny, nx, no))
        x[..., 0:2] = np.clip(rng.normal(0.0, 4.0, (bs, na, ny, nx, 2)), -12.0, 12.0)
        x[..., 2:4] = rng.normal(0.0, 1.5, (bs, na, ny, nx, 2))
        x[..., 4] = np.clip(rng.normal(-6.0, 1.5, (bs, na, ny, nx)), -12.0, -2.0)     # background: below any threshold
        shp = (bs, na, ny, nx, no - 5)
        bg = np.where(rng.random(shp) < WIDE, rng.uniform(-12.0, 12.0, shp), rng.normal(-5.0, NARROW, shp))
        x[..., 5:] = np.round(np.clip(bg, -12.0, 12.0) * LATTICE) / LATTICE
        lv.append(x)
    for b in range(bs):
        used, cells = set(), []

        def free_cell(l, a=None, tries=20):
            ny, nx = case.sizes[l]
            for _ in range(tries):
                key = (l, int(rng.integers(0, na)) if a is None else a, int(rng.integers(0, ny)), int(rng.integers(0, nx)))
                if key not in used:
                    used.add(key)
                    return key
            return None

        for l, (ny, nx) in enumerate(case.sizes):
            for _ in range(int(np.clip(na * ny * nx // 5, 1, 16))):
                key = free_cell(l)
                if key is not None:
                    lv[l][b, key[1], key[2], key[3]] = _planted(rng, case, no)
                    cells.append(key)
        # whole cells copied to another anchor of the level and to another level: the copies decode to other boxes with
        # bit-equal confidences (the tie order is then the row number a_off[l] + a*HW + p)
        for i, (l, a, y, x) in enumerate(cells):
            src = lv[l][b, a, y, x].copy()
            if na >= 2:
                a2 = (a + 1 + i) % na if (a + 1 + i) % na != a else (a + 1) % na
                if i % 2 == 0 and (l, a2, y, x) not in used:      # same position: overlapping boxes with equal confidence,
                    key = (l, a2, y, x)                           # the tie order decides which one survives
                    used.add(key)
                else:
                    key = free_cell(l, a2)
                if key is not None:
                    lv[key[0]][b, key[1], key[2], key[3]] = src
            if case.nl >= 2:
                key = free_cell((l + 1 + i % (case.nl - 1)) % case.nl)
                if key is not None:
                    lv[key[0]][b, key[1], key[2], key[3]] = src
    return tuple(lv)


@functools.lru_cache(maxsize=None)
def _convs(name, half):
    case = BY_NAME[name]
    out = []
    for x, (ny, nx) in zip(_convs64(name), case.sizes):
        t = torch.from_numpy(np.ascontiguousarray(x.transpose(0, 1, 4, 2, 3))).reshape(case.bs, case.na * case.no, ny, nx)
        out.append(t.to(torch.float16 if half else torch.float32).contiguous())
    return tuple(out)


def convs(case, dtype):
    """Seeded CPU conv outputs (bs, na*no, ny, nx) per level.  Cached: treat them as read-only."""
    return list(_convs(case.name, dtype == torch.float16))


# ------------------------------------------------------------------ the reference
def decode_formula(convs_, na, no, anchors, strides_, half):
    """models/yolo.py:71-79 on conv outputs (numpy, (bs, na*no, ny, nx) per level) -> (z, [x_perm], objcol).

    fp32: float64 throughout, rounded once at the end.  fp16: rounded to fp16 where the reference's tensor dtype forces it --
    after the sigmoid (through float32, see below), after * 2, after - 0.5, after the square and at the slice assignment; the
    grid, stride and anchor products are float32 (grid and anchor_grid are float32 tensors)."""
    zs, xps = [], []
    for l, c in enumerate(convs_):
        c = np.asarray(c)
        bs, _, ny, nx = c.shape
        raw = np.ascontiguousarray(c.reshape(bs, na, no, ny, nx).transpose(0, 1, 3, 4, 2))
        xps.append(raw)
        y = 1.0 / (1.0 + np.exp(-raw.astype(np.float64)))
        gy, gx = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
        grid = np.stack((gx, gy), -1)[None, None]                                 # (1, 1, ny, nx, 2)
        ag = np.asarray(anchors[l], np.float32).reshape(1, na, 1, 1, 2)
        if half:
            # a half tensor's sigmoid is computed in float32 and then rounded (torch's elementwise ops on half tensors, on the CPU
            # and on the GPU alike): the float32 step decides the ties of the fp16 rounding
            y = y.astype(np.float32).astype(np.float16)
            t = y[..., 0:4] * np.float16(2.0)                                     # fp16 (numpy rounds every fp16 operation)
            u = t[..., 0:2] - np.float16(0.5)
            xy = ((u.astype(np.float32) + grid.astype(np.float32)) * np.float32(strides_[l])).astype(np.float16)
            q = t[..., 2:4] * t[..., 2:4]
            wh = (q.astype(np.float32) * ag).astype(np.float16)
            assert t.dtype == u.dtype == q.dtype == np.float16
            out = np.concatenate((xy, wh, y[..., 4:]), -1)
        else:
            xy = (y[..., 0:2] * 2.0 - 0.5 + grid) * float(strides_[l])
            wh = (y[..., 2:4] * 2.0) ** 2 * ag.astype(np.float64)
            out = np.concatenate((xy, wh, y[..., 4:]), -1).astype(np.float32)
        zs.append(out.reshape(bs, -1, no))
    z = np.concatenate(zs, 1)
    return z, xps, np.ascontiguousarray(z[..., 4])


@functools.lru_cache(maxsize=None)
def _decode_ref(name, half):
    case = BY_NAME[name]
    cv = [c.numpy() for c in _convs(name, half)]
    return decode_formula(cv, case.na, case.no, anchors_px(case), strides(case), half)


def decode_ref(case, convs_=None, dtype=torch.float32):
    """(z, [x_perm per level], objcol) as numpy arrays of the tensor dtype.  Cached for the case's own convs (read-only)."""
    half = dtype == torch.float16
    if convs_ is None:
        return _decode_ref(case.name, half)
    return decode_formula([c.numpy() for c in convs_], case.na, case.no, anchors_px(case), strides(case), half)


def torch_chain(case, convs_):
    """The reference's op sequence (models/yolo.py:71-79, as tests/test_head_gpu.py::test_detect_inference_fp16 spells it) in
    torch on the CPU, in the dtype of the conv outputs."""
    ap, st = torch.from_numpy(anchors_px(case)), strides(case)
    zs = []
    for l, c in enumerate(convs_):
        bs, _, ny, nx = c.shape
        r = c.view(bs, case.na, case.no, ny, nx).permute(0, 1, 3, 4, 2).contiguous()
        yv, xv = torch.meshgrid([torch.arange(ny), torch.arange(nx)], indexing="ij")
        grid = torch.stack((xv, yv), 2).expand((1, case.na, ny, nx, 2)).float()
        ag = ap[l].view(1, case.na, 1, 1, 2).expand((1, case.na, ny, nx, 2)).float()
        y = r.sigmoid()
        y[..., 0:2] = (y[..., 0:2] * 2 - 0.5 + grid) * torch.tensor(st[l])
        y[..., 2:4] = (y[..., 2:4] * 2) ** 2 * ag
        zs.append(y.view(bs, -1, case.no))
    return torch.cat(zs, 1)


# the project's tolerances for decoded values (tests/test_head_gpu.py)
def close_fp32(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return np.abs(got - ref) <= 1e-6 + 2e-6 * np.abs(ref)


def close_fp16(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return np.abs(got - ref) <= 1.01 * np.maximum(np.abs(ref) * 2.0 ** -10, 2.0 ** -24)


# ------------------------------------------------------------------ fixture digest (tests/golden/head_configs.npz)
GROUPS = ("xy", "wh", "obj", "cls", "csl")
N_SAMPLED = 32


def group_sums(case, z):
    """(nl, 5, 2) float64: per level and channel group (xy, wh, obj, cls, csl) the sum and the sum of magnitudes of z."""
    z = np.asarray(z, np.float64)
    cuts = [(0, 2), (2, 4), (4, 5), (5, 5 + case.nc), (5 + case.nc, case.no)]
    out = np.zeros((case.nl, 5, 2))
    lo = 0
    for l, n in enumerate(case.level_rows):
        for g, (c0, c1) in enumerate(cuts):
            v = z[:, lo:lo + n, c0:c1]
            out[l, g] = v.sum(), np.abs(v).sum()
        lo += n
    return out


def sampled_rows(case):
    """Seeded rows of z.reshape(bs * a_total, no) that the fixture stores in full."""
    n = case.bs * case.a_total
    return np.sort(np.random.default_rng(case.seed + 1).choice(n, size=min(N_SAMPLED, n), replace=False))


# ------------------------------------------------------------------ what the inputs must exercise in the NMS
def row_origin(case):
    """(level, anchor) of every row of z."""
    lvl = np.concatenate([np.full(n, l) for l, n in enumerate(case.level_rows)])
    anc = np.concatenate([np.repeat(np.arange(case.na), ny * nx) for ny, nx in case.sizes])
    return lvl, anc


def nms_coverage(case, z, kept, multi_label):
    """What the reference's NMS on z exercises: (kept rows, confidences tied across two anchors, ... across two levels,
    tie groups with kept members on different levels -- on different anchors for a one-level head).
    z: (bs, A, no) tensor; kept: the list of (n, 7) rows pyref.non_max_suppression_obb returned for it."""
    lvl, anc = row_origin(case)
    nc, thr = case.nc, KW["conf_thres"]
    multi = bool(multi_label) and nc > 1
    n_kept = tie_anchor = tie_level = kept_groups = 0
    for b in range(case.bs):
        x = z[b]
        rows = (x[:, 4] > thr).nonzero().flatten()
        conf = x[rows, 5:5 + nc] * x[rows, 4:5]                                   # in the tensor dtype (utils/general.py:820)
        if multi:
            i, j = (conf > thr).nonzero(as_tuple=False).T
        else:
            v, j = conf.float().max(1)
            i = (v > thr).nonzero().flatten()
            j = j[i]
        src = rows[i].numpy()
        cand = {}
        for r, c, v, box in zip(src, j.tolist(), conf[i, j].float().tolist(), x[src, :4].float().tolist()):
            cand.setdefault(v, []).append((int(lvl[r]), int(anc[r]), tuple(box), float(c)))
        tie_anchor += sum(len({m[1] for m in g}) >= 2 for g in cand.values())
        tie_level += sum(len({m[0] for m in g}) >= 2 for g in cand.values())
        k = kept[b]
        n_kept += int(k.shape[0])
        have = {(tuple(r[:4]), r[5], r[6]) for r in k.float().tolist()}
        for v, g in cand.items():
            alive = [m for m in g if (m[2], v, m[3]) in have]
            kept_groups += len({m[0] if case.nl >= 2 else m[1] for m in alive}) >= 2
    return n_kept, tie_anchor, tie_level, kept_groups


def coverage_floor(case):
    """The conditions on the inputs (checked with the reference alone in tests/test_head_configs_host.py): at least 20 kept rows,
    5 confidences tied across two anchors, 5 across two levels, one tie group kept on both sides.  A head with one anchor
    cannot tie across anchors, one with one level not across levels, and the 1 x 1 head with bs = 2 has two rows in all: every
    one of them has to be kept."""
    return (min(20, case.bs * case.a_total), 5 if case.na >= 2 else 0, 5 if case.nl >= 2 else 0,
            1 if case.nl >= 2 or case.na >= 2 else 0)
