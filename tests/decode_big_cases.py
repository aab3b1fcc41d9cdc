"""Inputs of the filter kernel's large-grid tests (tests/test_decode_rows_per_thread_gpu.py on the GPU,
tests/test_decode_big_cases_host.py on the host): decoded Detect outputs with enough ROWS that the host plan
(csrc/nms_plan.h: plan_nms_obb) hands k_decode two or four rows per thread, and with enough rows times classes that the tie
word `row * nc + class` of a candidate key needs its fourth byte.

The tensors are large in bytes and almost entirely zero: a zero row fails `obj > conf_thres`, so the oracle
(oracle/pyref.py: non_max_suppression_obb) drops it in its first step and the comparison costs what the planted rows cost.
What is planted is chosen from the kernel's row map (csrc/nmsobb_front.h: k_decode, row_of), restated here as wg_rows:

    row = ((q * 32 + (tid >> 4)) * nwg + w) * 16 + (tid & 15),   nwg = ceil(A / (512 G)),   q < G,   row < A

  * the rows at both ends of the image, of the first 16-row chunk and of the first workgroup's share;
  * EVERY row of one workgroup (n_rows = 512 G: at G = 4 the workgroup's LDS row list is exactly full, and its waves flush
    their candidate stage many times);
  * a few rows in every q slot of two further workgroups;
  * image 1: the edge rows and every 7th row of the full workgroup.

G is not restated here: it comes from tests/test_host_index_maps.py (_rows_per_thread), the formula that
tests/test_nms_plan_host.py holds the library's plan to.  The device does not report G.

Reached (oracle alone, per image; `cand` = candidates, `kept` = rows the oracle returns, nothing cut: max_det 4500 is above every
candidate count; asserted within the caps by tests/test_decode_big_cases_host.py):

  case      dtype  planted rows  multi_label cand -> kept    best class cand -> kept   largest class
  g1_top    f16    528           593 -> 551                  407 -> 391                299
  g2_floor  f16    1046          1208 -> 1137                818 -> 790                613
  g2_tail   f32    1047 / 159    1181 / 192 -> 1100 / 177    820 / 123 -> 785 / 114    599   (f16: 1179 -> 1099, bf16: 1176 -> 1105)
  g2_top    f16    1046          1229 -> 1147                837 -> 796                631
  g4_floor  f16    2082          2297 -> 2135                1622 -> 1551              1157
  g4_tail   f32    2083 / 305    2317 / 354 -> 2171 / 334    1616 / 246 -> 1544 / 233  1181  (f16: 2314 -> 2169, bf16: 2306 -> 2212)
  g4_nc33   f16    2083 / 305    2040 / 299 -> 1800 / 266    the same                  65
  tie case  f16    220 / 200     216 / 196 -> 183 / 173 agnostic, 188 / 173 with class keys (10 pairs: 5 of one class)"""
import functools

import numpy as np
import torch

from oracle import pyref
from tests.test_host_index_maps import _rows_per_thread

THREADS = 512
CSL = 180
KW = dict(conf_thres=0.25, iou_thres=0.45, max_det=4500)       # max_det at the candidate cap: no kept row is cut, every planted row shows
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}

# name -> (bs, A, nc, intended G, A % 16, A % (512 G), dtypes)
SHAPES = {
    "g1_top": (1, 491519, 2, 1, 15, 511, ("f16",)),                 # one row short of G = 2: 960 workgroups
    "g2_floor": (1, 491520, 2, 2, 0, 0, ("f16",)),                  # the threshold exactly
    "g2_tail": (2, 245777, 2, 2, 1, 17, ("f32", "f16", "bf16")),    # ragged chunk
    "g2_top": (1, 983039, 2, 2, 15, 1023, ("f16",)),                # one row short of G = 4
    "g4_floor": (1, 983040, 2, 4, 0, 0, ("f16",)),                  # the threshold exactly
    "g4_tail": (2, 491537, 2, 4, 1, 17, ("f32", "f16", "bf16")),    # ragged chunk, full row list
    "g4_nc33": (2, 491537, 33, 4, 1, 17, ("f16",)),                 # class group fetched on demand, small-segment kernel
}
CASES = [(name, dt) for name, s in SHAPES.items() for dt in s[6]]
TIE_SHAPE = (491520, 40)                                            # A * nc = 19,660,800 >= 2^24


def n_workgroups(A, G):
    return (A + THREADS * G - 1) // (THREADS * G)


def wg_rows(A, G, w, q=None):
    """The rows workgroup w of an image reads, in (q, tid) order; q: only that slot of every thread."""
    nwg = n_workgroups(A, G)
    assert 0 <= w < nwg
    tid = np.arange(THREADS, dtype=np.int64)
    out = []
    for qq in (range(G) if q is None else [q]):
        row = ((qq * (THREADS // 16) + (tid >> 4)) * nwg + w) * 16 + (tid & 15)
        out.append(row[row < A])
    return np.concatenate(out)


def edge_rows(A, G):
    return [0, 1, 15, 16, 17, A - 17, A - 16, A - 2, A - 1, THREADS * G - 1, THREADS * G, THREADS * G + 1]


def workgroups_of(A, G):
    """(the workgroup planted in full, the two that get a few rows per q slot): none is the first or the last of the image."""
    nwg = n_workgroups(A, G)
    return nwg // 3, (1, nwg - 2)


def planted_rows(bs, A):
    """Per image: the sorted rows that carry values."""
    G = _rows_per_thread(bs, A)
    full, further = workgroups_of(A, G)
    full_rows = np.sort(wg_rows(A, G, full))
    some = []
    for w in further:
        for q in range(G):
            r = wg_rows(A, G, w, q)
            some += [int(r[0]), int(r[len(r) // 2]), int(r[-1])]
    img0 = np.unique(np.concatenate([edge_rows(A, G), full_rows, some]).astype(np.int64))
    img1 = np.unique(np.concatenate([edge_rows(A, G), full_rows[::7]]).astype(np.int64))
    return [img0 if b == 0 else img1 for b in range(bs)]


def row_values(n, nc, g, keep_plain=None):
    """(n, 5 + nc + 180) fp32 values of n planted rows, the k-th on cell k of a 40 px lattice of 56 columns (30 x 10 boxes with
    2 px of jitter: neighbours cannot suppress each other) -- but every 8th row shares the cell, the size and the angle of the row
    in front of it, so that some pairs do overlap and the NMS has something to suppress.  Objectness in (0.31, 0.98); exactly one
    angle bin at 0.9; nc <= 2: class scores random in (0, 1); nc > 2: class (cell % nc) at 0.9 and the others 0 (at most
    ceil(n / nc) + 1 rows per class).  Rows k % 97 == 13 have no class above the threshold (listed by the filter, yield nothing),
    rows k % 101 == 29 have objectness EQUAL to the threshold (0.25 is exact in the three dtypes: they fail `>`).  keep_plain:
    mask of rows that stay ordinary AND visible: alone in their cell, class 0 above 0.85 where nc <= 2, so each of them is a
    kept row of the oracle in both label modes."""
    R = lambda *s: torch.rand(*s, generator=g)
    k = torch.arange(n)
    plain = torch.zeros(n, dtype=torch.bool) if keep_plain is None else torch.as_tensor(keep_plain)
    dup = (k % 8 == 7) & ~plain & ~plain.roll(1)
    cell = k - dup.long()
    v = torch.zeros(n, 5 + nc + CSL)
    v[:, 0] = 60.0 + 40.0 * (cell % 56).float() + (R(n) - 0.5) * 4
    v[:, 1] = 60.0 + 40.0 * (cell // 56).float() + (R(n) - 0.5) * 4
    size = torch.stack((30.0 + (R(n) - 0.5) * 4, 10.0 + (R(n) - 0.5) * 2), 1)
    bins = torch.randint(0, CSL, (n,), generator=g)
    src = torch.where(dup, k - 1, k)
    v[:, 2:4] = size[src]
    v[k, 5 + nc + bins[src]] = 0.9
    v[:, 4] = 0.31 + 0.67 * R(n)
    if nc <= 2:
        v[:, 5:5 + nc] = R(n, nc) * 0.98 + 0.01
        v[plain, 5] = 0.85 + 0.14 * R(int(plain.sum()))
    else:
        v[k, 5 + cell % nc] = 0.9
    no_class = (k % 97 == 13) & ~plain
    v[no_class, 5:5 + nc] = 0.1
    v[(k % 101 == 29) & ~plain, 4] = KW["conf_thres"]
    return v


def planted(bs, A, nc, dtype, seed):
    """Per image: (rows, values in `dtype`)."""
    G = _rows_per_thread(bs, A)
    edges = np.array(edge_rows(A, G))
    out = []
    for b, rows in enumerate(planted_rows(bs, A)):
        g = torch.Generator().manual_seed(seed + 7919 * b)
        out.append((torch.from_numpy(rows), row_values(len(rows), nc, g, keep_plain=np.isin(rows, edges)).to(dtype)))
    return out


def _fill(bs, A, nc, dtype, rows_vals, device):
    pred = torch.zeros((bs, A, 5 + nc + CSL), dtype=dtype, device=device)
    for b, (rows, vals) in enumerate(rows_vals):
        pred[b, rows.to(device)] = vals.to(device)
    return pred


def build(bs, A, nc, dtype, seed, device="cpu"):
    """pred (bs, A, nc + 185): zeros plus the planted rows (the same bits on any device)."""
    return _fill(bs, A, nc, dtype, planted(bs, A, nc, dtype, seed), device)


def seed_of(name):
    return 9100 + 10 * list(SHAPES).index(name)


def case(name, dt, device="cpu"):
    bs, A, nc = SHAPES[name][:3]
    return build(bs, A, nc, DTYPES[dt], seed_of(name), device)


@functools.lru_cache(maxsize=None)
def reference(name, dt):
    """(multi_label rows, best-class rows) of the oracle on the case's full tensor (computed once, shared: do not write to them)."""
    pred = case(name, dt)
    return (pyref.non_max_suppression_obb(pred, multi_label=True, **KW), pyref.non_max_suppression_obb(pred, multi_label=False, **KW))


def candidate_counts(pred, multi_label=True, conf_thres=KW["conf_thres"]):
    """Per image: the (row, class) pairs with obj > thr and obj * cls > thr in the input dtype (best class: rows whose largest
    obj * cls passes), and the largest class among them."""
    nc = pred.shape[2] - 5 - CSL
    out = []
    for x in pred:
        x = x[x[:, 4] > conf_thres]
        conf = x[:, 5:5 + nc] * x[:, 4:5]
        ok = conf > conf_thres
        if multi_label and nc > 1:
            out.append((int(ok.sum()), int(ok.sum(0).max()) if ok.numel() else 0))
        else:
            best = conf.float().argmax(1)
            passing = ok.any(1)
            out.append((int(passing.sum()), int(torch.bincount(best[passing], minlength=nc).max()) if ok.numel() else 0))
    return out


# ------------------------------------------------------------------------------------------------------------ tie word, byte 3
def tie_pairs(A, nc, seed, n_pairs=10):
    """(r1, c1, r2, c2) with t1 = r1 * nc + c1 < 2^24 <= t2 = r2 * nc + c2 and (t2 & 0xFFFFFF) < (t1 & 0xFFFFFF): a sort that
    looks at three bytes of the tie word puts the SECOND row first.  Even pairs share their class, odd pairs do not."""
    assert A * nc >= 1 << 24
    rng = np.random.default_rng(seed)
    lo2 = -(-(1 << 24) // nc)                             # the first row whose every tie word is >= 2^24
    lo1 = ((A * nc - (1 << 24)) // nc) + 2                # above it: t1 > every t2 - 2^24
    assert lo1 < lo2 - 1 and lo2 < A
    r1 = rng.choice(np.arange(lo1, lo2 - 1), n_pairs, replace=False)
    r2 = rng.choice(np.arange(lo2, A), n_pairs, replace=False)
    c1 = rng.integers(0, nc, n_pairs)
    c2 = np.where(np.arange(n_pairs) % 2 == 0, c1, (c1 + 1 + rng.integers(0, nc - 1, n_pairs)) % nc)
    return [(int(a), int(b), int(c), int(d)) for a, b, c, d in zip(r1, c1, r2, c2)]


def tie_planted(A, nc, dtype, seed, bs=2):
    """Per image (rows, values): 200 ordinary rows each; image 0 also holds the pairs: 60 x 20 boxes at theta = 0 whose centres
    differ by 2 px (IoU 0.94), 120 px from the next pair and 1300 px from the ordinary rows; the two rows of a pair carry the
    same objectness (0.5 + i / 32) and the same class score (0.875), so their confidences are the same bits in any dtype."""
    pairs = tie_pairs(A, nc, seed)
    taken = {r for p in pairs for r in (p[0], p[2])}
    out = []
    for b in range(bs):
        g = torch.Generator().manual_seed(seed + 7919 * b)
        rows = torch.randperm(A, generator=g)[:260].tolist()
        rows = sorted(r for r in rows if r not in taken)[:200]
        vals = row_values(len(rows), nc, g)
        if b == 0:
            pv = torch.zeros(2 * len(pairs), 5 + nc + CSL)
            pr = []
            for i, (r1, c1, r2, c2) in enumerate(pairs):
                for j, (r, c) in enumerate(((r1, c1), (r2, c2))):
                    pv[2 * i + j, :4] = torch.tensor([100.0 + 120.0 * i + 2.0 * j, 1500.0, 60.0, 20.0])
                    pv[2 * i + j, 4] = 0.5 + i / 32.0
                    pv[2 * i + j, 5 + c] = 0.875
                    pv[2 * i + j, 5 + nc + 90] = 0.9
                    pr.append(r)
            order = np.argsort(rows + pr, kind="stable")
            rows = [(rows + pr)[i] for i in order]
            vals = torch.cat((vals, pv), 0)[torch.from_numpy(order)]
        out.append((torch.tensor(rows, dtype=torch.int64), vals.to(dtype)))
    return out, pairs


def tie_case(A, nc, dtype, seed, bs=2, device="cpu"):
    """(pred (bs, A, nc + 185), pairs)."""
    rows_vals, pairs = tie_planted(A, nc, dtype, seed, bs)
    return _fill(bs, A, nc, dtype, rows_vals, device), pairs


TIE_SEED = 9300
TIE_KW = {"agnostic": dict(agnostic=True, multi_label=True), "class_key": dict(agnostic=False, multi_label=True)}


@functools.lru_cache(maxsize=None)
def tie_reference(mode):
    """The oracle's rows of tie_case(*TIE_SHAPE, fp16, TIE_SEED) for both images (image 0 alone is the bs = 1 call's reference)."""
    pred, _ = tie_case(*TIE_SHAPE, torch.float16, TIE_SEED)
    return pyref.non_max_suppression_obb(pred, **KW, **TIE_KW[mode])
