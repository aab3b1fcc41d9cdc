"""GPU: the in-memory tile -> full-image merge (yolov5_obb_amd/tile_merge.py over obb_tile_merge_f32) against the reference's
file pipeline restated on the host (tests/tile_merge_cases.py): val_postprocess polygons, save_one_json's rounding, the Task1
lines of TestJson2VocClassTxt, pyref.merge_result_lines per class file.  Text and row parity: exact (strings; float64 bits)."""
import numpy as np
import pytest
import torch

import oracle
from oracle import pyref
from tests import tile_merge_cases as TC

pytestmark = pytest.mark.gpu


def run(dev, scene, **kw):
    from yolov5_obb_amd.tile_merge import merge_tiles
    rows, counts = merge_tiles([p.to(dev) for p in scene["preds"]], scene["tiles"], scene["nc"], n_src=scene["n_src"], **kw)
    assert rows.dtype == torch.float64 and rows.is_cuda and counts.dtype == np.int64 and counts.shape == (scene["n_src"], scene["nc"])
    assert rows.shape == (int(counts.sum()), 11)
    return rows, counts


def same_rows(got, want, counts, scene):
    got = got.cpu().numpy()
    assert got.shape == want.shape, (got.shape, want.shape)
    assert got.tobytes() == want.tobytes(), ("first differing row", int(np.flatnonzero((got != want).any(1))[0]))
    seg = (want[:, 10] * scene["nc"] + want[:, 9]).astype(np.int64)
    assert counts.reshape(-1).tolist() == np.bincount(seg, minlength=counts.size).tolist()


def files_equal_the_file_pipeline(dev, scene, tmp_path):
    """write_task1's files against mergesingle's lines of the scene's Task1 input, every line and the order, as strings."""
    from yolov5_obb_amd.tile_merge import write_task1
    assert TC.scores_distinct_per_segment(scene), "precondition: no two rounded scores of a segment are equal"
    rows, counts = run(dev, scene)
    paths = write_task1(str(tmp_path), rows, counts, TC.NAMES[:scene["n_src"]], TC.CLASS_NAMES[:scene["nc"]])
    lines = TC.task1_lines(scene)
    want = {TC.CLASS_NAMES[c]: pyref.merge_result_lines(v) for c, v in lines.items() if v}
    assert sorted(p.rsplit("Task1_", 1)[1][:-4] for p in paths) == sorted(want)
    for cname, w in want.items():
        got = (tmp_path / f"Task1_{cname}.txt").read_text().splitlines()
        assert len(got) == len(w) and 0 < len(w) < len(lines[TC.CLASS_NAMES.index(cname)]), (cname, len(got), len(w))
        assert got == w, (cname, "first differing line", next(i for i, (a, b) in enumerate(zip(got, w)) if a != b))
    return rows, counts


def test_parity_with_the_file_pipeline(dev, oracle_lib, tmp_path):
    scene = TC.memo("parity", TC.parity_scene)
    n = [len(p) for p in scene["preds"]]
    assert n[0] == 0 and n[4] == 0 and n[-1] == 0 and sorted(n)[3] >= 10 and 30 <= np.median(n) <= 45 and len(n) == 15
    rows, counts = files_equal_the_file_pipeline(dev, scene, tmp_path)
    assert (counts[:, 1] == 0).all() and (counts[:, [0, 2]] > 0).all(), "class 1 is absent"
    # ... and the rows themselves, bit for bit, against the host's doubles
    same_rows(rows, TC.memo("parity_rows", lambda: TC.expected_rows(scene, True, pyref.merge_nms_poly_fast)), counts, scene)


def test_a_segment_that_leaves_the_sorts_lds_block(dev, oracle_lib, tmp_path):
    scene = TC.memo("large", TC.large_scene)
    _, seg = TC.host_rows(scene, True)
    sizes = np.bincount(seg, minlength=6)
    assert sizes[0] > 2048 and sizes[5] == 1 and 4500 <= sizes.sum() <= 5500, sizes
    rows, counts = files_equal_the_file_pipeline(dev, scene, tmp_path)
    assert counts[1, 2] == 1
    same_rows(rows, TC.memo("large_rows", lambda: TC.expected_rows(scene, True, pyref.merge_nms_poly_fast)), counts, scene)


def test_scores_that_print_alike_are_ordered_by_input_row(dev, oracle_lib):
    """The pinned tie rule: the processing order is np.lexsort((row, -printed score)); the greedy loop is written here."""
    scene = TC.tie_scene()
    rows, _ = TC.host_rows(scene, True)
    score32 = torch.cat(scene["preds"])[:, 5].numpy()
    tied = [np.flatnonzero(rows[:, 8] == v) for v in np.unique(rows[:, 8])]
    tied = [t for t in tied if len(t) > 1]
    assert len(tied) == 13 and all(len(np.unique(score32[t])) == len(t) for t in tied), "the floats differ, the printed scores collide"
    assert all(score32[t[-1]] > score32[t[0]] for t in tied), "the float order is the opposite of the row order"
    order = np.lexsort((np.arange(len(rows)), -rows[:, 8]))
    iou = oracle.piou_matrix(rows[:, :8].copy(), rows[:, :8].copy())
    keep = []
    for i in order:
        if all(iou[k, i] <= 0.2 for k in keep):
            keep.append(i)
    assert all(t[0] in keep and t[1] not in keep for t in tied), "in every tied group the earlier row suppresses the next one"
    assert sum(t[-1] in keep for t in tied if len(t) == 3) == 1, "the triple: its first row drops the middle one, the last one stays"
    want = np.concatenate([rows[keep], np.zeros((len(keep), 2))], 1)
    got, counts = run(dev, scene)
    same_rows(got, want, counts, scene)


def test_without_text_rounding_the_rows_keep_full_precision(dev, oracle_lib):
    scene = TC.memo("parity", TC.parity_scene)
    assert TC.scores_distinct_per_segment(scene, text_rounding=False), "this case needs tie-free float scores"
    want = TC.memo("parity_rows_full", lambda: TC.expected_rows(scene, False, pyref.merge_nms_poly_fast))
    got, counts = run(dev, scene, text_rounding=False)
    same_rows(got, want, counts, scene)
    rounded = TC.memo("parity_rows", lambda: TC.expected_rows(scene, True, pyref.merge_nms_poly_fast))
    assert want.shape != rounded.shape or want.tobytes() != rounded.tobytes(), "not the file pipeline's result"


def test_variant_poly_all(dev, oracle_lib):
    scene = TC.memo("parity", TC.parity_scene)
    want = TC.memo("parity_rows_all", lambda: TC.expected_rows(scene, True, pyref.merge_nms_poly_all))
    got, counts = run(dev, scene, variant="poly_all")
    same_rows(got, want, counts, scene)


@pytest.mark.parametrize("bad", [3.5, 3.0, -1.0, float("nan")])
def test_a_class_that_is_no_integer_below_nc_raises(dev, bad):
    scene = TC.memo("parity", TC.parity_scene)
    preds = [p.clone() for p in scene["preds"]]
    preds[7][5, 6] = bad
    with pytest.raises(RuntimeError, match="class"):
        run(dev, dict(scene, preds=preds))


def test_zero_detections(dev):
    from yolov5_obb_amd.tile_merge import merge_tiles
    scene = TC.memo("parity", TC.parity_scene)
    rows, counts = run(dev, dict(scene, preds=[torch.zeros((0, 7)) for _ in scene["preds"]]))
    assert rows.shape == (0, 11) and not counts.any()
    rows, counts = merge_tiles([], [], 3)
    assert rows.shape == (0, 11) and counts.shape == (1, 3) and not counts.any()
    torch.cuda.synchronize(dev)


def test_more_tiles_than_one_launch_carries(dev, oracle_lib):
    """130 tiles (three k_tm_rows launches of up to 64 tiles), most of them empty, rows in the first, the 64th, the 65th and the last."""
    base = TC.memo("parity", TC.parity_scene)
    take = {0: 1, 63: 2, 64: 3, 129: 5}
    preds = [base["preds"][take[t]] if t in take else torch.zeros((0, 7)) for t in range(130)]
    tiles = [base["tiles"][take[t]] if t in take else (0, 0, 0, 1.0, None) for t in range(130)]
    scene = dict(preds=preds, tiles=tiles, nc=3, n_src=1)
    got, counts = run(dev, scene)
    same_rows(got, TC.expected_rows(scene, True, pyref.merge_nms_poly_fast), counts, scene)


def test_detect_large_equals_merge_tiles_by_hand(dev, oracle_lib):
    """A stand-in model that returns canned predictions per tile, keyed by the tile's top-left pixel: detect_large's result is
    merge_tiles called by hand with split_origins' tiles.  The image is lower than a tile: the crops arrive zero-padded."""
    from tests import synth
    from yolov5_obb_amd.tile_merge import detect_large, merge_tiles, split_origins
    from yolov5_obb_amd.utils.general import non_max_suppression_obb
    nc, width, height = 4, 2500, 900
    tiles = split_origins(width, height)
    assert len(tiles) == 3
    g = torch.Generator().manual_seed(4)
    image = torch.randint(0, 256, (3, height, width), generator=g, dtype=torch.uint8)
    canned = {}
    for k, (left, up) in enumerate(tiles):
        image[:, up, left] = torch.tensor([10 + k, 0, 200], dtype=torch.uint8)
        canned[10 + k] = synth.s_pred(1, 900, nc, seed=30 + k)[0].to(dev)
    seen = []

    def model(x):
        assert x.dtype == torch.float32 and x.shape[1:] == (3, 1024, 1024) and float(x.max()) <= 1.0
        assert not bool(x[:, :, height:, :].any()), "rows below the image are zero padding"
        keys = [int(round(float(v) * 255)) for v in x[:, 0, 0, 0]]
        seen.extend(keys)
        return torch.stack([canned[k] for k in keys]), None

    kw = dict(conf_thres=0.25, iou_thres=0.45)
    rows, counts = detect_large(model, image.to(dev), nc, batch=2, **kw)
    assert seen == [10, 11, 12]
    preds = [non_max_suppression_obb(canned[10 + k][None], **kw)[0] for k in range(3)]
    want_rows, want_counts = merge_tiles(preds, [(0, left, up, 1.0, None) for left, up in tiles], nc)
    assert rows.shape[0] > 10 and torch.equal(rows, want_rows) and np.array_equal(counts, want_counts)
