"""Host: the score-tie cases of tests/tie_cases.py can fail.  The oracle alone (oracle/pyref.py), never the code under test:
every case ties where its GPU test needs ties (coverage conditions), and two mutants of the oracle -- the opposite tie order, and
cross-class ties in class order -- are rejected by the exact compare on every case, while the relaxed compare that
tests/test_nmsobb_gpu.py used until now (synth.canon_rows) accepts the first of them on the lattice images."""
import numpy as np
import pytest
import torch

from oracle import pyref
from tests import synth
from tests import tie_cases as T

DTYPES = [False, True]     # half?


def _same(a, b):
    return a.shape == b.shape and torch.equal(a, b)


def _reversed(name, half):
    """Mutant: the opposite tie order -- the oracle on the input with the anchor axis reversed."""
    p = T.pred(name, half).flip(1)
    if T.CASES[name].get("restated"):
        return T.lattice_expected(p, **T.kwargs(name))
    return pyref.non_max_suppression_obb(p.clone(), **T.kwargs(name))


@pytest.mark.parametrize("half", DTYPES)
@pytest.mark.parametrize("name", T.QUANT)
def test_quantised_cases_tie_where_they_must(oracle_lib, name, half):
    ref = T.reference(name, half)
    tied, cross, same = (sum(v) for v in zip(*(T.coverage(r) for r in ref)))
    print(f"{name} {'fp16' if half else 'fp32'}: rows {sum(r.shape[0] for r in ref)} tied {tied} x-cls {cross} same {same}")
    assert tied >= 100, (name, tied)
    if not T.kwargs(name).get("agnostic"):
        assert cross >= 50, (name, cross)
    assert same >= 10, (name, same)


@pytest.mark.parametrize("half", DTYPES)
def test_fp16_and_fp32_tie_identically(oracle_lib, half):
    """obj * cls of the quantised inputs is exact in either dtype: the candidates' confidences are the same numbers."""
    for name in ("generic", "lds_buckets_network", "max_nms_cut"):
        a, b = T.candidate_confs(name, False), T.candidate_confs(name, True)
        assert all(torch.equal(x, y) for x, y in zip(a, b)), name


@pytest.mark.parametrize("half", DTYPES)
def test_cut_case_has_a_tie_group_across_max_nms(oracle_lib, half):
    for c in T.candidate_confs("max_nms_cut", half):
        assert len(c) > pyref.MAX_NMS and c[pyref.MAX_NMS - 1] == c[pyref.MAX_NMS]
        inside, group = int((c[:pyref.MAX_NMS] == c[pyref.MAX_NMS]).sum()), int((c == c[pyref.MAX_NMS]).sum())
        print(f"max_nms_cut: tie group of {group} at the cut, {inside} inside")
        assert inside >= 100 and group - inside >= 100


@pytest.mark.parametrize("half", DTYPES)
@pytest.mark.parametrize("name", T.MAX_DET)
def test_max_det_falls_inside_a_tie_group(oracle_lib, name, half):
    md = T.kwargs(name)["max_det"]
    for cut, full in zip(T.reference(name, half), T.reference(name, half, uncut=True)):
        assert full.shape[0] > md and full[md - 1, 5] == full[md, 5] and full[md - 1, 6] != full[md, 6]
        assert torch.equal(cut, full[:md])


@pytest.mark.parametrize("half", DTYPES)
def test_sizes_reach_the_paths_they_are_named_for(oracle_lib, half):
    n = {name: [len(c) for c in T.candidate_confs(name, half)] for name in T.CASES if name != "labels"}
    assert max(n["generic"]) <= 6144 and max(n["lds_buckets_network"]) <= 6144 and max(n["lattice_lds"]) <= 6144
    assert min(n["one_list_4096"]) > 4096 and max(n["one_list_4096"]) <= 6144
    assert min(n["segsort"]) > 12288 and min(n["lattice_segsort"]) > 12288 and max(n["segsort"]) <= pyref.MAX_NMS
    p = T.pred("lds_buckets_network", half)
    nc = 16
    conf = (p[..., 5:5 + nc] * p[..., 4:5]).float()
    per_class = ((conf > 0.25) & (p[..., 4:5] > 0.25)).sum(1)                  # (bs, nc) candidates per class
    assert int(per_class[0].max()) <= 384 and int(per_class[1, 5]) > 512
    for name, lo, hi in (("small_segments", 129, 384), ("persistent_merge", 385, 10 ** 6), ("lattice_lds", 129, 384), ("lattice_small", 1, 128)):
        p = T.pred(name, half)
        nc = p.shape[2] - 185
        conf = (p[..., 5:5 + nc] * p[..., 4:5]).float()
        largest = int(((conf > 0.25) & (p[..., 4:5] > 0.25)).sum(1).max())
        assert lo <= largest <= hi, (name, largest)


@pytest.mark.parametrize("half", DTYPES)
def test_label_rows_follow_every_anchor_in_label_order(oracle_lib, half):
    for b, rows in enumerate(T.reference("labels", half)):
        top = rows[rows[:, 5] == 1.0]
        lb = T.LABELS[b]
        n_anchor = top.shape[0] - len(lb)
        assert n_anchor >= 11                                  # 8 planted anchors, 3 of them with a second class, and the input's own
        assert torch.equal(top[n_anchor:, 6], lb[:, 0]) and torch.equal(top[n_anchor:, :4], lb[:, 1:5])
        assert set(top[:n_anchor, 6].tolist()) & set(lb[:, 0].tolist())           # anchors of the labels' classes among them
        assert torch.equal(rows[:top.shape[0]], top)


@pytest.mark.parametrize("half", DTYPES)
@pytest.mark.parametrize("name", T.LATTICE)
def test_lattice_rows_are_the_documented_order(oracle_lib, name, half):
    """pyref on the lattice equals the restated order (the largest lattice only restates: see tie_cases.CASES)."""
    ref = T.reference(name, half)
    want = T.lattice_expected(T.pred(name, half), **T.kwargs(name))
    assert all(_same(a, b) for a, b in zip(ref, want))
    assert all(r.shape[0] == len(c) for r, c in zip(ref, T.candidate_confs(name, half)))        # every candidate kept


@pytest.mark.parametrize("half", DTYPES)
@pytest.mark.parametrize("name", list(T.CASES))
def test_mutants_are_rejected_by_the_exact_compare(oracle_lib, name, half):
    ref = T.reference(name, half)
    rev = _reversed(name, half)
    blind = 0
    for b, (r, m) in enumerate(zip(ref, rev)):
        if r.shape[0]:
            assert not _same(r, m), (name, b, "the reversed tie order gives the same rows")
            blind += int(r.shape == m.shape and np.array_equal(synth.canon_rows(r), synth.canon_rows(m)))
    print(f"{name} {'fp16' if half else 'fp32'}: relaxed compare blind on {blind} of {len(ref)} images")
    if name in T.SEGMENTED:
        assert all(not torch.equal(T.class_major(r), r) for r in ref if r.shape[0]), (name, "class-major cross-class ties give the same rows")
    if name in T.LATTICE:
        assert blind == len(ref), (name, "the relaxed compare was expected to be blind here")
