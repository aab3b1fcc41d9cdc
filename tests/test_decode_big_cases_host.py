"""CPU: the preconditions of the large-grid filter cases (tests/decode_big_cases.py), so that a later edit of the builders cannot
hollow out what tests/test_decode_rows_per_thread_gpu.py reaches on the device:

  * every shape gets the rows-per-thread G it is meant for -- asserted from tests/test_host_index_maps.py: _rows_per_thread, the
    formula tests/test_nms_plan_host.py holds the library's plan to (the device does not report G) -- and has the remainders
    (A % 16, A % (512 G)) and the row total the shape table claims;
  * the planted rows hold one workgroup's complete row set (512 G rows) and touch every q < G of two further workgroups;
  * the oracle keeps some and suppresses some candidates of every image, and stays inside the candidate caps that keep it at
    seconds (4500 per image under multi_label, OBB_NMS_SORT_LDS_HINT = 6144 at most, 384 per (image, class) where nc > 2);
  * the tie case can tell a sort by three bytes of the tie word from a sort by four.

Every case is materialised in full, fp32 (735 MB) included, and the oracle runs on the full tensor; the cases share one
reference per (shape, dtype) with nothing else in this file."""
import numpy as np
import pytest
import torch

import oracle
from oracle import pyref
from tests import decode_big_cases as BC
from tests.test_host_index_maps import _rows_per_thread

SORT_LDS_HINT = 6144     # include/obb_hip.h: OBB_NMS_SORT_LDS_HINT
SMALL_SEG = 384          # include/obb_hip.h: OBB_NMS_SMALL_SEG
MULTI_CAP = 4500


@pytest.mark.parametrize("name", list(BC.SHAPES))
def test_shape_reaches_its_rows_per_thread(name):
    bs, A, nc, G, rem16, rem_wg, _ = BC.SHAPES[name]
    assert _rows_per_thread(bs, A) == G
    assert A % 16 == rem16 and A % (512 * G) == rem_wg
    total = {"g1_top": 491519, "g2_floor": 491520, "g2_tail": 491554, "g2_top": 983039, "g4_floor": 983040, "g4_tail": 983074,
             "g4_nc33": 983074}[name]
    assert bs * A == total
    # the neighbours of the thresholds sit on either side of them
    if name.endswith("_top"):
        assert _rows_per_thread(bs, A + 1) == 2 * G
    if name.endswith("_floor"):
        assert _rows_per_thread(bs, A - 1) == G // 2
    assert A * nc < 1 << 24                                                   # (the tie word's fourth byte is the tie case's subject)


@pytest.mark.parametrize("name", list(BC.SHAPES))
def test_planted_rows_fill_one_workgroup_and_touch_every_slot(name):
    bs, A, nc, G = BC.SHAPES[name][:4]
    nwg = BC.n_workgroups(A, G)
    rows = BC.planted_rows(bs, A)
    assert len(rows) == bs
    full, further = BC.workgroups_of(A, G)
    assert len({0, nwg - 1, full, *further}) == 5
    full_rows = BC.wg_rows(A, G, full)
    assert len(full_rows) == 512 * G == len(set(full_rows.tolist()))          # n_rows = 512 G: at G = 4 the row list is exactly full
    assert np.isin(full_rows, rows[0]).all()
    for w in further:
        for q in range(G):
            assert np.isin(BC.wg_rows(A, G, w, q), rows[0]).any(), (w, q)
    edges = BC.edge_rows(A, G)
    assert len(set(edges)) == 12 and min(edges) == 0 and max(edges) == A - 1
    for b in range(bs):
        assert np.isin(edges, rows[b]).all() and rows[b].min() == 0 and rows[b].max() == A - 1
        assert (np.diff(rows[b]) > 0).all()
    if bs > 1:
        assert np.isin(np.sort(full_rows)[::7], rows[1]).all() and len(rows[1]) < len(rows[0]) // 4
    # the map itself: the workgroups of the image read every row exactly once (a coarse sample of workgroups would not show a
    # repeated row, so all of them -- 15 ms per shape)
    seen = np.zeros(A, dtype=np.int8)
    for w in range(nwg):
        seen[BC.wg_rows(A, G, w)] += 1
    assert (seen == 1).all()


@pytest.mark.parametrize("name,dt", BC.CASES)
def test_oracle_keeps_some_and_stays_inside_the_caps(oracle_lib, name, dt):
    bs, A, nc, G = BC.SHAPES[name][:4]
    pred = BC.case(name, dt)
    assert pred.shape == (bs, A, nc + 185) and pred.dtype == BC.DTYPES[dt]
    thr = BC.KW["conf_thres"]
    for b, (rows, vals) in enumerate(BC.planted(bs, A, nc, BC.DTYPES[dt], BC.seed_of(name))):
        assert torch.equal(pred[b, rows], vals)
        assert int((pred[b, :, 4] != 0).sum()) == len(rows)                   # nothing else is planted
        obj = vals[:, 4].float()
        passing = obj > thr
        at_thr = obj == thr
        assert 2 <= int(at_thr.sum()) <= 32 and bool((obj[~at_thr] > 0.3).all()) and bool((obj < 0.99).all())
        conf = vals[:, 5:5 + nc] * vals[:, 4:5]
        listed_for_nothing = passing & ~(conf > thr).any(1)
        assert int(listed_for_nothing.sum()) >= 2
        assert bool(((vals[:, 5 + nc:] == 0.9).sum(1) == 1).all()) and bool(((vals[:, 5 + nc:] != 0).sum(1) == 1).all())
    ref_multi, ref_best = BC.reference(name, dt)
    edges = BC.edge_rows(A, G)
    for multi, ref in ((True, ref_multi), (False, ref_best)):
        counts = BC.candidate_counts(pred, multi_label=multi)
        for b in range(bs):
            cand, seg = counts[b]
            assert cand < BC.KW["max_det"]                                     # nothing is cut: every kept row is in the reference
            kept = {tuple(r) for r in ref[b][:, :4].tolist()}
            for r in edges:                                                   # a missing edge row would change the rows
                assert tuple(pred[b, r, :4].float().tolist()) in kept, (name, dt, multi, b, r)
            assert 0 < ref[b].shape[0] < cand, (name, dt, multi, b, ref[b].shape[0], cand)
            assert cand <= (MULTI_CAP if multi else SORT_LDS_HINT) and cand <= SORT_LDS_HINT
            if nc > 2:
                assert seg <= SMALL_SEG, (name, dt, multi, b, seg)
    if name == "g4_tail":
        assert BC.candidate_counts(pred)[0][0] > 1024                           # counts_exact's first call overflows its slots


def _ious(vals, i, j):
    box = lambda k: np.array([[float(vals[k, 0]), float(vals[k, 1]), float(vals[k, 2]), float(vals[k, 3]), 0.0]], dtype=np.float32)
    return float(oracle.riou_matrix(box(i), box(j))[0, 0])


def test_tie_case_tells_three_bytes_from_four(oracle_lib):
    A, nc = BC.TIE_SHAPE
    assert A * nc >= 1 << 24 and _rows_per_thread(2, A) == 4 and _rows_per_thread(1, A) == 2
    (planted, pairs) = BC.tie_planted(A, nc, torch.float16, BC.TIE_SEED)
    rows, vals = planted[0]
    assert len(pairs) >= 8 and len(rows) == 200 + 2 * len(pairs) and len(planted[1][0]) == 200
    where = {int(r): i for i, r in enumerate(rows.tolist())}
    thr = BC.KW["conf_thres"]
    centres = []
    for r1, c1, r2, c2 in pairs:
        t1, t2 = r1 * nc + c1, r2 * nc + c2
        assert r1 < r2 and t1 < (1 << 24) <= t2 < (1 << 32) and (t2 & 0xFFFFFF) < (t1 & 0xFFFFFF)
        i, j = where[r1], where[r2]
        assert vals[i, 4].view(torch.int16) == vals[j, 4].view(torch.int16)                       # equal inputs ...
        assert vals[i, 5 + c1].view(torch.int16) == vals[j, 5 + c2].view(torch.int16)
        ci, cj = vals[i, 5 + c1] * vals[i, 4], vals[j, 5 + c2] * vals[j, 4]
        assert ci.view(torch.int16) == cj.view(torch.int16) and float(ci) > thr                   # ... equal confidences
        assert int((vals[i, 5:5 + nc] != 0).sum()) == 1 and int((vals[j, 5:5 + nc] != 0).sum()) == 1
        assert _ious(vals, i, j) > BC.KW["iou_thres"] + 0.3
        assert not torch.equal(vals[i, :4], vals[j, :4])                                          # the kept row says which was first
        centres.append((float(vals[i, 0]), float(vals[i, 1])))
    c = np.array(centres)
    d = np.hypot(*(c[:, None, :] - c[None, :, :]).transpose(2, 0, 1)) + 1e9 * np.eye(len(c))
    assert d.min() >= 100.0                                                                       # pairs far from one another ...
    others = np.array([k for k, r in enumerate(rows.tolist()) if r not in {p for q in pairs for p in (q[0], q[2])}])
    assert float((vals[others, 1].float() + 40).max()) < c[:, 1].min() - 1000                     # ... and from the ordinary rows

    pred, _ = BC.tie_case(A, nc, torch.float16, BC.TIE_SEED)
    ref = BC.tie_reference("agnostic")
    kw = dict(BC.KW, **BC.TIE_KW["agnostic"])
    # the planted rows alone, in row order, are the same list of candidates in the same order
    small = pyref.non_max_suppression_obb(vals[None], **kw)[0]
    assert torch.equal(ref[0], small) and 0 < ref[0].shape[0] < BC.candidate_counts(pred)[0][0]

    def kept_boxes(out):
        return {tuple(r) for r in out[:, :4].tolist()}
    first = {tuple(vals[where[p[0]], :4].float().tolist()) for p in pairs}
    second = {tuple(vals[where[p[2]], :4].float().tolist()) for p in pairs}
    assert first <= kept_boxes(ref[0]) and not (second & kept_boxes(ref[0]))                       # four bytes: every r1, no r2
    # three bytes: the same rows in the order of (tie word & 0xFFFFFF) -- one class per row, so the row order IS the tie order,
    # and the oracle's stable sort by confidence keeps it
    cls = vals[:, 5:5 + nc].float().argmax(1).numpy()
    low = (rows.numpy() * nc + cls) & 0xFFFFFF
    three = pyref.non_max_suppression_obb(vals[torch.from_numpy(np.argsort(low, kind="stable"))][None], **kw)[0]
    assert second & kept_boxes(three)
    assert second <= kept_boxes(three) and not (first & kept_boxes(three))                        # (in fact all of them flip)
    assert not torch.equal(three, ref[0])
    # class-key mode: pairs of one class suppress, pairs of two classes keep both
    refc = BC.tie_reference("class_key")
    keptc = kept_boxes(refc[0])
    for r1, c1, r2, c2 in pairs:
        b1, b2 = tuple(vals[where[r1], :4].float().tolist()), tuple(vals[where[r2], :4].float().tolist())
        assert b1 in keptc and (b2 in keptc) == (c1 != c2)
