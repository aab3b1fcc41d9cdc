"""Inputs of the score-tie tests (tests/test_nms_ties_gpu.py on the GPU, tests/test_tie_cases_host.py on the host): decoded
Detect outputs whose confidences tie by construction, one named case per sort / merge / cut path of
obb_non_max_suppression_obb, the oracle's side of the comparison and the coverage figures each case must reach.

The contract (include/obb_hip.h): candidates of equal confidence are ordered by ascending anchor * nc + class, label rows
behind every anchor in label order.  oracle/pyref.non_max_suppression_obb is pinned to that order, so device rows and oracle
rows are the same SEQUENCE and every comparison is torch.equal.

Two generators:
  quant_pred    synth.s_pred with the objectness and class columns rounded to multiples of 1/q (q = 8 or 16) before the dtype
                cast: obj * cls is a multiple of 1/q^2 <= 1, exact in fp16 and fp32, so both dtypes tie identically.
  lattice_pred  2 x 2 boxes on an 8 px lattice (no two can touch: NMS keeps every candidate, the output IS the sort order)
                with confidences on five levels; lattice_expected restates the documented order with a stable numpy sort.

Coverage reached (oracle alone, fp32 / fp16 where they differ; `tied` = kept rows whose confidence another kept row of the
image shares, `x-cls` / `same` = adjacent kept rows of equal confidence and different / the same class; asserted with the
bounds of the issue -- tied >= 100, x-cls >= 50 in the non-agnostic cases, same >= 10 -- by tests/test_tie_cases_host.py):

  case                  rows         tied         x-cls        same
  generic               201 / 201    194 / 196    162 / 163    14 / 14
  lds_buckets_network   828 / 830    815 / 819    571 / 571    172 / 175
  one_list_4096         1396 / 1390  1386 / 1379  1266 / 1259  35 / 36
  segsort               1700 / 1691  1692 / 1683  1502 / 1498  102 / 97
  max_nms_cut           1115 / 1123  1115 / 1123  556 / 567    546 / 543
  small_segments        389 / 388    372 / 372    84 / 83      257 / 258
  persistent_merge      631 / 634    606 / 609    425 / 429    127 / 126
  single_list           335 / 335    329 / 328    277 / 275    24 / 25
  agnostic              197 / 197    189 / 191    158 / 159    14 / 14
  labels                232 / 232    225 / 227    192 / 193    15 / 15
  best_class            631 / 628    607 / 602    519 / 512    37 / 40
  classes_filter        347 / 348    322 / 323    250 / 249    27 / 29
  max_det_small         398          398          361          24
  max_det_persistent    302          302          223          69

Candidates per image: generic 532 / 522, lds_buckets_network 1803 / 2406 (class 5 of image 1: above 512), one_list_4096 5460 /
5366, segsort 16028 / 16103, max_nms_cut 40000 (the tie group at confidence 0.375 has 3728 members, 2942 of them inside the
cut at 30000), lattice_lds 3757 / 3756, lattice_small 3157 / 3151, lattice_segsort 13180 / 13113 (every candidate is kept).
max_det 199 and 151 fall between two rows of equal confidence and different class in both images and both dtypes.

Mutants (each of the 17 cases x 2 dtypes, every non-empty image): the reversed tie order (pyref on pred.flip(1)) changes the row
sequence everywhere; so does a stable re-sort of cross-class ties into class order on the 15 class-segmented cases.  On the
quantised cases the reversed order also changes the kept SET (clustered boxes: which of two tied boxes survives), so even the
relaxed compare sees it: blind on 0 of 28 images.  On the three lattice cases the kept set cannot change and the relaxed
compare is blind on 6 of 6 images (per dtype) that the exact compare rejects.

`blind` = images whose rows under the reversed tie order differ from the oracle's while synth.canon_rows -- the relaxed
compare these tests replace -- calls them equal.
"""
import functools

import numpy as np
import torch

from oracle import pyref
from tests import synth

KW = dict(conf_thres=0.25, iou_thres=0.45, multi_label=True, max_det=1500)
LEVELS = (0.5, 0.625, 0.75, 0.875, 1.0)


# --------------------------------------------------------------------------------------------------------------- generators
def quant_pred(bs, A, nc, seed, n_obj, fg_frac, q):
    """synth.s_pred (fp32) with objectness and class scores on the grid k / q."""
    p = synth.s_pred(bs, A, nc, seed=seed, n_obj=n_obj, fg_frac=fg_frac)
    p[..., 4:5 + nc] = (p[..., 4:5 + nc] * q).round() / q
    return p


def plant(pred, b, rows, c, nc, g, n_groups, centre=(512.0, 512.0), spread=400.0, q=16, lo=0.5):
    """rows of image b become members of class c only: n_groups objects of overlapping candidates, objectness on the
    grid k / q in [lo, 1], class score 1 -- heavy ties inside one class segment."""
    cnt = len(rows)
    ctr = torch.tensor(centre) + (torch.rand(n_groups, 2, generator=g) - 0.5) * 2 * spread
    which = torch.randint(0, n_groups, (cnt,), generator=g)
    pred[b, rows, 0:2] = ctr[which] + torch.randn(cnt, 2, generator=g) * 6
    pred[b, rows, 2:4] = torch.tensor([80.0, 28.0]) * (1 + 0.1 * torch.randn(cnt, 2, generator=g))
    k0 = int(round(lo * q))
    pred[b, rows, 4] = torch.randint(k0, q + 1, (cnt,), generator=g).float() / q
    pred[b, rows, 5:5 + nc] = 0.0
    pred[b, rows, 5 + c] = 1.0
    pred[b, rows, 5 + nc:] = 0.02
    pred[b, rows, 5 + nc + torch.randint(0, 180, (n_groups,), generator=g)[which]] = 0.9


def lattice_pred(bs, A, nc, seed, n_cand, second=0.3):
    """Boxes that cannot touch (2 x 2 px on an 8 px lattice of 256 columns), n_cand candidate anchors per image with the
    objectness on LEVELS and one class at score 1; a fraction `second` of them carries a second class at score 1 or 0.5."""
    g = torch.Generator().manual_seed(seed)
    p = torch.zeros(bs, A, 5 + nc + 180)
    i = torch.arange(A)
    p[..., 0] = ((i % 256) * 8 + 4).float()
    p[..., 1] = ((i // 256) * 8 + 4).float()
    p[..., 2:4] = 2.0
    p[..., 5 + nc + 90] = 1.0                                                  # theta = 0
    lev = torch.tensor(LEVELS)
    for b in range(bs):
        rows = torch.randperm(A, generator=g)[:n_cand]
        p[b, rows, 4] = lev[torch.randint(0, len(lev), (n_cand,), generator=g)]
        c1 = torch.randint(0, nc, (n_cand,), generator=g)
        p[b, rows, 5 + c1] = 1.0
        two = torch.rand(n_cand, generator=g) < second
        c2 = torch.randint(0, nc, (n_cand,), generator=g)
        p[b, rows[two], 5 + c2[two]] = torch.where(torch.rand(int(two.sum()), generator=g) < 0.5, 1.0, 0.5)
    return p


def lattice_expected(pred, conf_thres=0.25, multi_label=True, max_det=1500, classes=None, **_):
    """The documented order, restated: candidates in row-major (anchor, class) order, stable sort by descending confidence,
    the max_nms cut, the max_det cut.  Valid where no two candidates interact (lattice_pred, not agnostic ... nor otherwise)."""
    assert multi_label
    out = []
    nc = pred.shape[2] - 185
    for x in pred:
        x = x.float().numpy()
        conf = x[:, 5:5 + nc] * x[:, 4:5]
        ok = (conf > np.float32(conf_thres)) & (x[:, 4:5] > np.float32(conf_thres))
        if classes is not None:
            ok &= np.isin(np.arange(nc), classes)[None, :]
        a, c = np.nonzero(ok)                                                   # row-major: ascending anchor * nc + class
        order = np.argsort(-conf[a, c], kind="stable")[:pyref.MAX_NMS][:max_det]
        a, c = a[order], c[order]
        theta = (x[a, 5 + nc:].argmax(1) - 90).astype(np.float32) / np.float32(180) * np.float32(pyref.PI)
        out.append(torch.from_numpy(np.concatenate([x[a, :4], theta[:, None], conf[a, c][:, None], c[:, None].astype(np.float32)], 1)))
    return out


# -------------------------------------------------------------------------------------------------------------- case builders
def _generic():
    return quant_pred(2, 6000, 16, 7, 60, 0.1, 8)


def _wide():
    return quant_pred(2, 20000, 16, 7, 200, 0.1, 16)


def _buckets_network():
    """image 0: class buckets of a few hundred candidates (rank counting); image 1: 700 candidates of class 5 (a bucket above
    512: the 16-wave network; a segment above 384: the persistent kernel)."""
    p = quant_pred(2, 20000, 16, 11, 200, 0.1, 16)
    plant(p, 1, torch.arange(2000, 2700), 5, 16, torch.Generator().manual_seed(3), 60)
    return p


def _one_list():
    return quant_pred(2, 30000, 40, 92, 300, 0.2, 16)


def _segsort():
    return quant_pred(2, 40000, 16, 21, 300, 0.45, 16)


def _cut():
    """A = 20000, nc = 2, every anchor on one of 200 objects and both classes passing: 40000 candidates on a few dozen
    confidence values, so a tie group of hundreds straddles the max_nms cut."""
    p = quant_pred(1, 20000, 2, 5, 200, 1.0, 8)
    p[..., 4] = p[..., 4].clamp(min=0.625)
    p[..., 5:7] = p[..., 5:7].clamp(min=0.5)
    return p


def _small_segments():
    """Class segments on either side of 128 (above it a segment is split into parts whose bit matrices the last part merges),
    all below 384."""
    nc = 4
    p = quant_pred(2, 20000, nc, 77, 40, 0.01, 16)
    g = torch.Generator().manual_seed(5)
    r0 = 3000
    for img, cls, cnt in ((0, 0, 100), (0, 1, 150), (0, 2, 215), (0, 3, 270), (1, 0, 320), (1, 2, 180), (1, 3, 245)):
        plant(p, img, torch.arange(r0, r0 + cnt), cls, nc, g, max(1, cnt // 12))
        r0 += cnt
    return p


def _persistent():
    return quant_pred(2, 20000, 4, 13, 200, 0.1, 16)


def _single_list():
    """image 0: an oversized box (its circle leaves the class window); image 1: ~300 boxes with a sub-pixel short side (above the
    bound of the cross-class check); image 2: plain class segments."""
    p = quant_pred(3, 6000, 16, 17, 60, 0.1, 8)
    p[0, 500, 2] = 5000.0
    p[0, 500, 4] = 0.875
    g = torch.Generator().manual_seed(5)
    thin = torch.rand(6000, generator=g) < 0.05
    p[1, thin, 3] = torch.rand(int(thin.sum()), generator=g) * 0.6 + 0.3
    p[1, thin, 4] = 1.0
    return p


LABELS = [torch.tensor([[7, 1200., 1200., 30., 10.], [3, 1300., 1200., 30., 10.], [7, 1400., 1200., 30., 10.], [11, 1500., 1200., 30., 10.],
                        [3, 1600., 1200., 30., 10.], [0, 1700., 1200., 30., 10.]]),
          torch.tensor([[15, 1200., 1300., 30., 10.], [15, 1300., 1300., 30., 10.], [2, 1400., 1300., 30., 10.]])]


def _labels():
    """Label rows (confidence 1) and anchors with obj = cls = 1 of the same and of other classes, none touching another box: in
    the oracle's rows the anchors come first (ascending anchor * nc + class), then the labels in label order."""
    p = _generic().clone()
    for b in range(2):
        rows = torch.tensor([5900, 40, 3100, 41, 5000, 2999, 17, 4242])
        cls = torch.tensor([3, 11, 7, 0, 7, 15, 2, 3])
        p[b, rows, 0] = 1200.0 + 100.0 * torch.arange(8)
        p[b, rows, 1] = 1500.0 + 100.0 * b
        p[b, rows, 2], p[b, rows, 3] = 30.0, 10.0
        p[b, rows, 4] = 1.0
        p[b, rows, 5:21] = 0.0
        p[b, rows, 5 + cls] = 1.0
        p[b, rows[:3], 5 + (cls[:3] + 1) % 16] = 1.0                           # multi-label: a second class at confidence 1
    return p


@functools.lru_cache(maxsize=None)
def _lattice(A, nc, n_cand):
    return lattice_pred(2, A, nc, 31 + nc, n_cand)


MAX_DET_SMALL, MAX_DET_PERSISTENT = 199, 151        # inside a tie group of every image (asserted by the host test)

# name -> dict(make, kw, path, segmented (class segments decide: the class-major mutant must be seen), quant (the coverage
# conditions apply), lattice (lattice_expected applies), restated (the reference IS lattice_expected: the oracle's scan of 13000
# boxes that never meet takes 20 s; the two smaller lattices pin lattice_expected to pyref), labels, env)
CASES = {
    "generic": dict(make=_generic, path="generic sort behind hint cand = 0; un-hinted first call"),
    "lds_buckets_network": dict(make=_buckets_network, path="in-LDS sort: rank-counting class buckets + 16-wave network in one batch"),
    "one_list_4096": dict(make=_one_list, env={"OBB_NMS_SELF_SORT": "0"},
                          path="sort kernel, image above 4096 candidates ordered as one list"),
    "segsort": dict(make=_segsort, path="multi-workgroup sort of segsort.h: more than 12288 candidates per image"),
    "max_nms_cut": dict(make=_cut, segmented=False, path="more than max_nms candidates: tie group straddling the cut, single list"),
    "small_segments": dict(make=_small_segments, path="small-segment kernel, segments split into parts above 128"),
    "persistent_merge": dict(make=_persistent, path="class segments above 384: persistent kernel, per-class kept lists merged"),
    "single_list": dict(make=_single_list, path="single-list images: oversized box, sub-pixel boxes"),
    "agnostic": dict(make=_generic, kw=dict(agnostic=True), segmented=False, path="agnostic: one segment per image"),
    "labels": dict(make=_labels, labels=LABELS, path="label rows tied at confidence 1 with anchors"),
    "best_class": dict(make=_wide, kw=dict(multi_label=False), path="multi_label = False"),
    "classes_filter": dict(make=_wide, kw=dict(classes=[0, 2, 3, 5, 8, 9, 12, 15]), path="classes= filter"),
    "max_det_small": dict(make=_wide, kw=dict(max_det=MAX_DET_SMALL), path="max_det inside a tie group, small-segment kernel"),
    "max_det_persistent": dict(make=_persistent, kw=dict(max_det=MAX_DET_PERSISTENT), path="max_det inside a tie group, persistent kernel"),
    "lattice_lds": dict(make=lambda: _lattice(16000, 16, 3000), kw=dict(max_det=30000), lattice=True, quant=False,
                        path="lattice: in-LDS sort + small-segment kernel"),
    "lattice_small": dict(make=lambda: _lattice(16000, 40, 2500), kw=dict(max_det=30000), lattice=True, quant=False,
                          path="lattice: self-sorting small segments"),
    "lattice_segsort": dict(make=lambda: _lattice(40000, 16, 10500), kw=dict(max_det=30000), lattice=True, quant=False, restated=True,
                            path="lattice: multi-workgroup sort"),
}
QUANT = [n for n, c in CASES.items() if c.get("quant", True)]
LATTICE = [n for n, c in CASES.items() if c.get("lattice")]
SEGMENTED = [n for n, c in CASES.items() if c.get("segmented", True)]
MAX_DET = [n for n in CASES if n.startswith("max_det_")]


@functools.lru_cache(maxsize=None)
def _pred32(name):
    return CASES[name]["make"]()


def pred(name, half=False):
    """The case's input on the host (shared: do not write to it)."""
    p = _pred32(name)
    return p.half() if half else p


def kwargs(name, **over):
    kw = dict(KW, **CASES[name].get("kw", {}))
    if CASES[name].get("labels") is not None:
        kw["labels"] = CASES[name]["labels"]
    kw.update(over)
    return kw


@functools.lru_cache(maxsize=None)
def reference(name, half=False, uncut=False):
    """The oracle's rows of a case (computed once, shared: do not write to them).  uncut: without the max_det cut."""
    kw = kwargs(name, **(dict(max_det=pyref.MAX_NMS) if uncut else {}))
    if CASES[name].get("restated"):
        return lattice_expected(pred(name, half), **kw)
    return pyref.non_max_suppression_obb(pred(name, half).clone(), **kw)


def candidate_confs(name, half=False):
    """Per image: the confidences of all candidates (anchors only) in descending order -- what the max_nms cut sees."""
    p, kw = pred(name, half), kwargs(name)
    nc = p.shape[2] - 185
    out = []
    for x in p:
        x = x[x[:, 4] > kw["conf_thres"]]
        conf = (x[:, 5:5 + nc] * x[:, 4:5]).float()
        out.append(torch.sort(conf[conf > kw["conf_thres"]], descending=True)[0])
    return out


def coverage(rows):
    """(tied rows, adjacent equal-confidence pairs of different class, ... of the same class) of one image's kept rows."""
    r = torch.as_tensor(rows)
    if r.shape[0] < 2:
        return 0, 0, 0
    conf, cls = r[:, 5], r[:, 6]
    _, inv, cnt = torch.unique(conf, return_inverse=True, return_counts=True)
    eq = conf[1:] == conf[:-1]
    return int((cnt[inv] > 1).sum()), int((eq & (cls[1:] != cls[:-1])).sum()), int((eq & (cls[1:] == cls[:-1])).sum())


def class_major(rows):
    """Mutant: the oracle's rows with cross-class ties in class order (a stable re-sort by (-conf, cls))."""
    r = torch.as_tensor(rows)
    key = np.lexsort((r[:, 6].numpy(), -r[:, 5].numpy()))
    return r[torch.from_numpy(key)]
