"""GPU: the order of equal-confidence candidates on every sort / merge / cut path of the fused non_max_suppression_obb.

include/obb_hip.h: "Score ties are ordered by ascending (anchor*nc + class)", label rows behind every anchor; the result does not
depend on the hints.  oracle/pyref.py is pinned to the same order, so every comparison here is torch.equal on whole rows -- no
tolerance, no set compare.  The inputs (tests/tie_cases.py) tie by construction, in fp32 and fp16 alike; tests/test_tie_cases_host.py
shows with the oracle alone that a kernel with the opposite tie order, or with cross-class ties in class order, fails every one
of them.  Every case runs un-hinted first, then hinted, and checks through the hints and the library's stage counters that the
path it is named for did run."""
import ctypes as C

import pytest
import torch

from oracle import pyref
from tests import tie_cases as T
from tests.test_lazy_nms_gpu import _detect, _heads, _run

pytestmark = pytest.mark.gpu

DTYPES = [pytest.param(False, id="fp32"), pytest.param(True, id="fp16")]


def _exact(got, ref, what=""):
    assert len(got) == len(ref), what
    for b, (g, r) in enumerate(zip(got, ref)):
        g = g.cpu()
        assert g.shape == r.shape, (what, b, tuple(g.shape), tuple(r.shape))
        if not torch.equal(g, r):
            k = int((g != r).any(1).nonzero()[0])
            raise AssertionError((what, f"image {b}: first differing row {k} of {len(r)}", g[k].tolist(), r[k].tolist()))


def _call(p, kw):
    """One call with the stage counters on: (rows, launches per stage -- 0 filter, 1 per-image sort, 3 NMS)."""
    from yolov5_obb_amd import _lib
    from yolov5_obb_amd.utils import general
    L = _lib.lib()
    L.obb_profile_enable(1)
    try:
        got = general.non_max_suppression_obb(p, **kw)
    finally:
        ms, cnt = (C.c_double * 8)(), (C.c_int64 * 8)()
        rc = L.obb_profile_collect(C.cast(ms, C.c_void_p), C.cast(cnt, C.c_void_p), 8)
        L.obb_profile_enable(0)
    assert rc == 0
    return got, list(cnt)


def _hint(dev, name, half):
    from yolov5_obb_amd.utils import general
    p, kw = T.pred(name, half), T.kwargs(name)
    nc = p.shape[2] - 185
    return general.hint_get(dev, p.shape[1], nc, bool(kw["multi_label"]) and nc > 1, kw["conf_thres"])


def _three_calls(dev, name, half, monkeypatch, what="", env=None):
    """hints cleared, then an un-hinted and two hinted calls, each equal to the oracle: (hints after, stage counts of the last).
    env: the case's own environment unless given."""
    from yolov5_obb_amd.utils import general
    for k, v in (T.CASES[name].get("env", {}) if env is None else env).items():
        monkeypatch.setenv(k, v)
    ref, kw = T.reference(name, half), T.kwargs(name)
    p = T.pred(name, half).to(dev)
    general.hints_clear()
    for rep in range(3):
        got, cnt = _call(p, kw)
        _exact(got, ref, (name, what, "call", rep))
    return _hint(dev, name, half), cnt


SEG_SMALL, LDS_HINT = 384, 6144          # include/obb_hip.h: OBB_NMS_SMALL_SEG, OBB_NMS_SORT_LDS_HINT


@pytest.mark.parametrize("half", DTYPES)
def test_generic_sort_and_first_call(dev, oracle_lib, monkeypatch, half):
    from yolov5_obb_amd.utils import general
    _three_calls(dev, "generic", half, monkeypatch)
    p, kw = T.pred("generic", half).to(dev), T.kwargs("generic")
    general.hint_set(dev, p.shape[1], 16, True, kw["conf_thres"], cand=0)            # hint 0: the generic sort
    got, cnt = _call(p, kw)
    _exact(got, T.reference("generic", half), "hint 0")
    assert cnt[1] > 0 and 0 < _hint(dev, "generic", half)["cand"] <= LDS_HINT


@pytest.mark.parametrize("half", DTYPES)
def test_in_lds_sort_buckets_and_network(dev, oracle_lib, monkeypatch, half):
    st, cnt = _three_calls(dev, "lds_buckets_network", half, monkeypatch)
    assert 0 < st["cand"] <= LDS_HINT and cnt[1] > 0                                 # the in-LDS sort kernel ran on the hinted call
    assert st["seg"] > SEG_SMALL                                                     # image 1's class 5: persistent kernel behind it


@pytest.mark.parametrize("half", DTYPES)
def test_image_above_4096_candidates_is_one_list(dev, oracle_lib, monkeypatch, half):
    st, cnt = _three_calls(dev, "one_list_4096", half, monkeypatch)
    assert cnt[1] > 0 and 4096 < st["cand"] <= LDS_HINT and st["seg"] > 4096         # reported with its whole size
    monkeypatch.delenv("OBB_NMS_SELF_SORT")                                          # ... and the library's own choice for this input
    _three_calls(dev, "one_list_4096", half, monkeypatch, "default mode", env={})


@pytest.mark.parametrize("name", ["segsort", "lattice_segsort"])
@pytest.mark.parametrize("half", DTYPES)
def test_multi_workgroup_sort(dev, oracle_lib, monkeypatch, name, half):
    st, _ = _three_calls(dev, name, half, monkeypatch)
    assert st["cand"] > 12288


@pytest.mark.parametrize("half", DTYPES)
def test_tie_group_across_the_max_nms_cut(dev, oracle_lib, monkeypatch, half):
    st, _ = _three_calls(dev, "max_nms_cut", half, monkeypatch)
    assert st["cand"] > pyref.MAX_NMS


@pytest.mark.parametrize("name", ["small_segments", "lattice_lds", "lattice_small"])
@pytest.mark.parametrize("half", DTYPES)
def test_small_segment_kernel_in_every_mode(dev, oracle_lib, monkeypatch, name, half):
    """OBB_NMS_SELF_SORT = 0 (sort kernel in front) / 1 (self-sorting where no helpers run) / 2 and unset (wherever possible) x
    OBB_NMS_SMALL_HELPERS = 0 / unset; segments above 128 are split into parts when helpers run."""
    lo, hi = {"small_segments": (256, SEG_SMALL), "lattice_lds": (128, SEG_SMALL), "lattice_small": (0, 128)}[name]
    for mode in ("0", "1", "2", None):
        for helpers in ("0", None):
            for var, val in (("OBB_NMS_SELF_SORT", mode), ("OBB_NMS_SMALL_HELPERS", helpers)):
                if val is None:
                    monkeypatch.delenv(var, raising=False)
                else:
                    monkeypatch.setenv(var, val)
            st, cnt = _three_calls(dev, name, half, monkeypatch, (mode, helpers))
            assert lo < st["seg"] <= hi, (mode, helpers, st)
            self_ran = cnt[0] > 0 and cnt[1] == 0
            assert self_ran == (mode != "0" and (helpers == "0" or mode in ("2", None))), (mode, helpers, cnt)


@pytest.mark.parametrize("name", ["persistent_merge", "max_det_persistent"])
@pytest.mark.parametrize("half", DTYPES)
def test_persistent_kernel_merges_class_lists_in_global_order(dev, oracle_lib, monkeypatch, name, half):
    st, cnt = _three_calls(dev, name, half, monkeypatch)
    assert st["seg"] > SEG_SMALL and cnt[1] > 0


@pytest.mark.parametrize("name", ["single_list", "agnostic", "labels", "best_class", "classes_filter", "max_det_small"])
@pytest.mark.parametrize("half", DTYPES)
def test_arguments_and_single_list_images(dev, oracle_lib, monkeypatch, name, half):
    st, _ = _three_calls(dev, name, half, monkeypatch)
    if name == "single_list":
        assert st["small_boxes"]                                                     # image 1's sub-pixel boxes were met
    if name == "max_det_small":
        assert 0 < st["seg"] <= SEG_SMALL
    monkeypatch.setenv("OBB_NMS_SELF_SORT", "0")                                     # the same behind the sort kernel
    _three_calls(dev, name, half, monkeypatch, "sort kernel")


def _tied_heads(nc, dtype, seed=3, per_image=40):
    """Conv outputs (host) in which whole cells -- all 5 + nc + 180 channels of one (anchor, y, x) -- of confident level-0 cells are
    copied to other anchors, positions and levels: the copies decode to other boxes with bit-equal confidences."""
    shapes = [(32, 32), (16, 16), (8, 8)]
    heads = _heads(2, nc, shapes, seed, "cpu", dtype, k=60)
    no = 5 + nc + 180
    v = [h.view(2, 3, no, ny, nx) for h, (ny, nx) in zip(heads, shapes)]
    g = torch.Generator().manual_seed(seed)
    for b in range(2):
        src = (v[0][b, :, 4].float() > 1.0).nonzero()[:per_image]
        assert len(src) >= per_image // 2
        for a, y, x in src.tolist():
            cell = v[0][b, a, :, y, x].clone()
            for lvl, (ny, nx) in enumerate(shapes):
                for _ in range(2):
                    a2, y2, x2 = (int(torch.randint(0, hi, (1,), generator=g)) for hi in (3, ny, nx))
                    v[lvl][b, a2, :, y2, x2] = cell
    return heads


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
def test_lazy_head_entry_with_confidences_tied_across_levels(dev, oracle_lib, dtype):
    """Detect.lazy_nms (obb_non_max_suppression_obb_head): the candidates' index is a_off[level] + a*ny*nx + y*nx + x.  Lazy rows
    equal eager rows and the oracle on the decoded tensor, un-hinted and hinted."""
    from yolov5_obb_amd.utils import general
    nc = 16
    det = _detect(nc, 3, dev, dtype)
    heads = [h.to(dev) for h in _tied_heads(nc, dtype)]
    kw = dict(T.KW)
    z, _, eager = _run(det, heads, False, **kw)
    zc = z.cpu()
    ref = pyref.non_max_suppression_obb(zc.clone(), **kw)
    # the input ties across levels: confidences of passing anchors that occur on all three levels
    bounds = [0, 3 * 32 * 32, 3 * 32 * 32 + 3 * 16 * 16, zc.shape[1]]
    for b in range(2):
        conf = (zc[b, :, 5:5 + nc] * zc[b, :, 4:5]).float().amax(1)
        per_level = [set(conf[lo:hi][conf[lo:hi] > 0.25].tolist()) for lo, hi in zip(bounds[:-1], bounds[1:])]
        assert len(per_level[0] & per_level[1] & per_level[2]) >= 10
    assert sum(T.coverage(r)[0] for r in ref) >= 100
    _exact(eager, ref, "eager")
    general.hints_clear()
    for rep in range(3):
        zl, _, lazy = _run(det, heads, True, **kw)
        assert not zl.is_materialized(), "the fused entry did not run"
        _exact(lazy, ref, ("lazy", rep))
