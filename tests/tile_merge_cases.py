"""Scenes for the in-memory tile merge (yolov5_obb_amd/tile_merge.py), built on the CPU: objects planted in SOURCE-image
coordinates, seen by every tile that contains their centre -- so an object in the 200 px overlap of two tiles arrives twice with
the same source coordinates (up to float32), and a share of the sightings is shifted by 0.3 .. 3 px so that the IoUs of such
pairs fall on both sides of the merge threshold 0.2.

A scene: preds (one (n_t, 7) float32 tensor [cx cy l s theta conf cls] per tile, in the MODEL's input frame), tiles
((src_image, left, up, rate, ratio_pad) per tile), nc, names.  Expected results are computed here, on the host, through the
reference's own text: val_postprocess polygons (host_polys), save_one_json's round(x, 1) / round(score, 5) (val.py:60-65), the '%s' line
of tools/TestJson2VocClassTxt.py:45, and pyref.merge_result_lines (mergesingle) per class file.

Scores: distinct multiples of 1e-5 plus at most 0.3e-5, so the rounded scores of a scene are distinct by construction (the
tests assert it per segment); tied scenes are built separately (tie_scene)."""
import math

import numpy as np
import torch

from oracle import pyref

SUB, GAP = 1024, 200
NAMES = ["P0003", "P0011"]
CLASS_NAMES = ["plane", "ship", "harbor"]
_memo = {}


def memo(key, fn):
    """Expected results are computed once and shared (read-only) by every test that needs them."""
    if key not in _memo:
        _memo[key] = fn()
    return _memo[key]


def origins(width, height):
    from yolov5_obb_amd.tile_merge import split_origins
    return split_origins(width, height, SUB, GAP)


def objects(rng, n, cls, width, height):
    """(n, 7) [cx cy l s theta conf cls] in source coordinates"""
    o = np.zeros((n, 7))
    o[:, 0], o[:, 1] = rng.uniform(0, width, n), rng.uniform(0, height, n)
    o[:, 2], o[:, 3] = rng.uniform(20, 120, n), rng.uniform(8, 40, n)
    thin = rng.rand(n) < 0.35                                                 # narrow enough for a 0.3 .. 3 px shift to pass below IoU 0.2
    o[thin, 3] = rng.uniform(1.5, 5, int(thin.sum()))
    o[:, 4] = rng.uniform(-math.pi / 2, math.pi / 2, n)
    o[:, 6] = cls
    return o


def sightings(rng, objs, tile, scores, per_tile=None, shifted=0.5):
    """The rows of one tile: every object whose centre falls inside it, in the model's input frame, a share of them shifted."""
    _, left, up, rate, ratio_pad = tile
    x, y = objs[:, 0] * rate - left, objs[:, 1] * rate - up
    seen = np.flatnonzero((x >= 8) & (x < SUB - 8) & (y >= 8) & (y < SUB - 8))
    if per_tile is not None and len(seen) > per_tile:
        seen = np.sort(rng.choice(seen, per_tile, replace=False))
    r = objs[seen].copy()
    r[:, 0], r[:, 1] = x[seen], y[seen]
    r[:, 2:4] *= rate
    move = rng.rand(len(seen)) < shifted
    d, a = rng.uniform(0.3, 3.0, len(seen)), rng.uniform(0, 2 * math.pi, len(seen))
    r[move, 0] += (d * np.cos(a))[move]
    r[move, 1] += (d * np.sin(a))[move]
    if ratio_pad is not None:
        gain, pad = ratio_pad[0][0], ratio_pad[1]
        r[:, 0], r[:, 1] = r[:, 0] * gain + pad[0], r[:, 1] * gain + pad[1]
        r[:, 2:4] *= gain
    r[:, 5] = [scores.pop() for _ in range(len(seen))]
    return torch.from_numpy(r.astype(np.float32))


def _score_pool(rng, n):
    k = rng.choice(np.arange(5000, 99000), size=n, replace=False)
    return ((k + rng.uniform(-0.3, 0.3, n)) / 1e5).tolist()


def parity_scene():
    """2 source images of 2000 x 1500, nc = 3 with class 1 absent; image 0 also at rate 0.5 (two crops) and 1.5 (one tile); about 40
    rows per tile; the first, the last and one middle tile empty; a ratio_pad on two tiles."""
    rng = np.random.RandomState(5)
    w, h = 2000, 1500
    tiles = [(0, l, u, 1.0, None) for l, u in origins(w, h)]
    tiles += [(0, 0, 0, 0.5, None), (0, 200, 100, 0.5, None), (0, 1648, 824, 1.5, None)]
    tiles += [(1, l, u, 1.0, None) for l, u in origins(w, h)]
    tiles[2] = tiles[2][:4] + (((0.8, 0.8), (12.0, 3.5)),)
    tiles[10] = tiles[10][:4] + (((1.25, 1.25), (0.0, 20.0)),)
    objs = [np.concatenate([objects(rng, 70, 0, w, h), objects(rng, 45, 2, w, h)]) for _ in range(2)]
    scores = _score_pool(rng, 4000)
    empty = {0, 4, len(tiles) - 1}
    preds = [torch.zeros((0, 7)) if t in empty else sightings(rng, objs[tile[0]], tile, scores, per_tile=45) for t, tile in enumerate(tiles)]
    return dict(preds=preds, tiles=tiles, nc=3, n_src=2)


def large_scene():
    """One segment of more than 2048 rows (image 0, class 0: the sort leaves its LDS block), about 5000 rows in all, and a
    segment of exactly one row (image 1, class 2)."""
    rng = np.random.RandomState(9)
    w, h = 2000, 1500
    tiles = [(s, l, u, 1.0, None) for s in range(2) for l, u in origins(w, h)]
    objs = [np.concatenate([objects(rng, 1150, 0, w, h), objects(rng, 330, 1, w, h), objects(rng, 100, 2, w, h)]),
            np.concatenate([objects(rng, 420, 0, w, h), objects(rng, 330, 1, w, h)])]
    scores = _score_pool(rng, 20000)
    preds = [sightings(rng, objs[tile[0]], tile, scores) for tile in tiles]
    one = torch.tensor([[500.0, 400.0, 60.0, 20.0, 0.3, scores.pop(), 2.0]])
    preds[8] = torch.cat([preds[8], one])
    return dict(preds=preds, tiles=tiles, nc=3, n_src=2)


def tie_scene():
    """One image, one class, two tiles that overlap by 200 px.  Pairs of heavily overlapping boxes whose float32 scores DIFFER
    but print alike (round(score, 5)), the higher float in the LATER row -- in the second tile, or further down the same tile: the
    pinned rule keeps the earlier row, the float order would keep the later one.  Plus untied boxes around them."""
    rng = np.random.RandomState(21)
    tiles = [(0, 0, 0, 1.0, None), (0, 824, 0, 1.0, None)]
    a, b = [], []
    for k in range(12):
        cx, cy = 850.0 + 12 * k, 60.0 + 75 * k                                  # inside both tiles
        l, s, th = rng.uniform(40, 60), rng.uniform(15, 30), rng.uniform(-1.5, 1.5)      # (half diagonal < 34: the groups, 75 px apart, stay clear of each other)
        base = np.float32((30000 + 5000 * k) / 1e5)
        lo, hi = base, np.nextafter(np.nextafter(base, np.float32(1)), np.float32(1))
        assert lo != hi and round(float(lo), 5) == round(float(hi), 5)
        if k % 3 == 2:                                                          # both in the first tile, two rows apart
            a += [[cx, cy, l, s, th, lo, 0], [cx - 300, cy, 30, 10, 0.1, 0.01 + k * 1e-3, 0], [cx + 1.0, cy + 0.5, l, s, th, hi, 0]]
        else:                                                                   # one sighting per tile
            a.append([cx, cy, l, s, th, lo, 0])
            b.append([cx - 824 + 1.0, cy + 0.5, l, s, th, hi, 0])
    # a triple: three boxes in a row, equal printed scores, the middle one overlaps both ends, the ends do not overlap each other
    s3 = np.float32(0.77777)
    s3b = np.nextafter(s3, np.float32(1))
    a += [[900.0, 980.0, 60, 20, 0.0, s3, 0], [930.0, 980.0, 60, 20, 0.0, s3b, 0]]
    b += [[960.0 - 824, 980.0, 60, 20, 0.0, np.nextafter(s3b, np.float32(1)), 0]]
    preds = [torch.tensor(np.array(a, dtype=np.float32)), torch.tensor(np.array(b, dtype=np.float32))]
    return dict(preds=preds, tiles=tiles, nc=1, n_src=1)


# ------------------------------------------------------------------------------------------------ the host side
def host_polys(scene):
    """Per tile: pred_polyn (n, 10) float32, the polygon in the tile's frame, from the EXISTING val_postprocess -- the package's
    where a device is visible (what the file pipeline would round and write; it is not under test here), pyref's restatement on
    a machine without one (the CPU test of the scenes' geometry: the two differ by an ulp of float32 here and there)."""
    out = []
    for p, (_, _, _, _, ratio_pad) in zip(scene["preds"], scene["tiles"]):
        gain, pad = (ratio_pad[0][0], ratio_pad[1]) if ratio_pad is not None else (1.0, (0.0, 0.0))
        if not len(p):
            out.append(torch.zeros((0, 10)))
        elif torch.cuda.is_available():
            from yolov5_obb_amd.val import val_postprocess
            out.append(val_postprocess(p.to("cuda:0"), ratio_pad=((gain, gain), pad))[2].cpu())
        else:
            out.append(pyref.val_postprocess(p.clone(), gain, pad)[2])
    return out


def task1_lines(scene, names=NAMES):
    """The Task1_<class>.txt input lines of the scene, per class: save_one_json's rounding, TestJson2VocClassTxt's line."""
    from yolov5_obb_amd.tile_merge import tile_name
    lines = {c: [] for c in range(scene["nc"])}
    for polyn, (src, left, up, rate, _) in zip(host_polys(scene), scene["tiles"]):
        name = tile_name(names[src], rate, left, up)
        for p in polyn.tolist():
            poly, score = [round(x, 1) for x in p[:8]], round(p[-2], 5)
            lines[int(p[-1])].append("%s %s %s %s %s %s %s %s %s %s" % (name, score, *poly))
    return lines


def host_rows(scene, text_rounding):
    """(n, 9) doubles [8 source-image coordinates, score] and the segment of every row, computed on the host from
    pyref.val_postprocess: Python's round on the widened floats when text_rounding, poly2origpoly in double."""
    rows, seg = [], []
    for polyn, (src, left, up, rate, _) in zip(host_polys(scene), scene["tiles"]):
        for p in polyn.tolist():
            xy = [round(x, 1) for x in p[:8]] if text_rounding else p[:8]
            rows.append([float(v + (up if k & 1 else left)) / float(str(rate)) for k, v in enumerate(xy)] + [round(p[8], 5) if text_rounding else p[8]])
            seg.append(src * scene["nc"] + int(p[9]))
    return np.array(rows, dtype=np.float64).reshape(-1, 9), np.array(seg, dtype=np.int64)


def scores_distinct_per_segment(scene, text_rounding=True):
    rows, seg = host_rows(scene, text_rounding)
    return all(len(np.unique(rows[seg == g, 8])) == int((seg == g).sum()) for g in np.unique(seg))


def expected_rows(scene, text_rounding, nms):
    """(m, 11) [rows, cls, src]: per segment ascending, `nms` (a pyref merge function: its own argsort()[::-1], so the segment's
    scores must be distinct) on the host rows."""
    rows, seg = host_rows(scene, text_rounding)
    out = []
    for g in range(scene["n_src"] * scene["nc"]):
        at = np.flatnonzero(seg == g)
        if len(at):
            keep = at[np.asarray(nms(rows[at], 0.2), dtype=np.int64)]
            out.append(np.concatenate([rows[keep], np.full((len(keep), 1), g % scene["nc"]), np.full((len(keep), 1), g // scene["nc"])], 1))
    return np.concatenate(out) if out else np.zeros((0, 11))
