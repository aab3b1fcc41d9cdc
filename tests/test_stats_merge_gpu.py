"""GPU: obb_stats_merge_f32 (csrc/stats_merge.h) and what stands on it -- val.ValStats.merged, the per-image bookkeeping of
ValStats.add_batch -- against numpy permutations and against ONE accumulator that saw every image in id order.  Every comparison
is exact (bit patterns).

Entry level: synthetic floats that name their (image, row, column) (tests/stats_merge_cases.py), dst poisoned between canaries.
ValStats level: one sequence of images (tests/obbmetric_cases.py, batches of 4, images without detections, without labels, with
neither) through one accumulator and through W strided ones.  The tie case: two equal confidences whose order decides AP, which
a rank-major concatenation gets wrong.  The workspace contract with the harness of tests/abi_contract.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import abi_contract as AC
from tests import obbmetric_cases as OC
from tests import stats_merge_cases as SC

pytestmark = pytest.mark.gpu
NIOU = 10
POISON = 0xC3C3C3C3
GUARD = 4096                             # floats of canary in front of and behind dst

_memo = {}


def problem(*key):
    """Problem(world, n_images, width, src_stride, shuffled, seed), built once and left unchanged."""
    if key in _memo:
        return _memo[key]
    P = SC.Problem(*key[:3], src_stride=key[3], shuffled=key[4], seed=key[5])
    if key[1] <= 37 or key == BIG_KEY:                           # (the large ones are used once, but for BIG_KEY)
        _memo[key] = P
    return P


def L_():
    from yolov5_obb_amd import _lib
    return _lib.lib()


def vp(t):
    return C.c_void_p(t.data_ptr()) if t is not None and t.numel() else C.c_void_p(0)


def run_entry(dev, P, dst_stride, spare_rows=5, counts=None, img_id=None, rows_per_run=None, n_images_total=None, dst_rows=None):
    """One call on fresh buffers -> (rc, info (4), dst rows as uint32 (dst_rows, dst_stride), counts_out, both canaries intact, src
    unchanged).  The keyword arguments replace what the Problem holds (the error cases)."""
    L = L_()
    n_img = P.n_images if n_images_total is None else n_images_total
    rows = P.total + spare_rows if dst_rows is None else dst_rows
    src = torch.from_numpy(P.src).to(dev)
    cnt = torch.from_numpy(P.counts if counts is None else counts).to(dev)
    ids = torch.from_numpy(P.img_id if img_id is None else img_id).to(dev)
    buf = torch.full((2 * GUARD + rows * dst_stride,), POISON - (1 << 32), dtype=torch.int32, device=dev).view(torch.float32)
    dst = buf[GUARD:GUARD + rows * dst_stride]
    by_id = torch.full((max(n_img, 1),), -5, dtype=torch.int32, device=dev)
    info = torch.full((4,), -5, dtype=torch.int32, device=dev)
    ws = torch.full((L.obb_stats_merge_workspace_bytes(n_img),), 0xFF, dtype=torch.uint8, device=dev)
    i64 = C.c_int64 * P.world
    rc = L.obb_stats_merge_f32(vp(src), P.src_stride, P.run_stride, i64(*(rows_per_run or P.rows_per_run)), vp(cnt), vp(ids), P.K,
                               i64(*P.images_per_run), P.world, n_img, P.width, vp(dst), dst_stride, rows, vp(by_id), vp(info), vp(ws),
                               ws.numel(), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize(dev)
    bits = buf.view(torch.int32).cpu().numpy().view(np.uint32)
    guards_ok = bool((bits[:GUARD] == POISON).all() and (bits[GUARD + rows * dst_stride:] == POISON).all())
    src_same = SC.same_bits(src.cpu().numpy(), P.src)
    return rc, info.cpu().numpy(), bits[GUARD:GUARD + rows * dst_stride].reshape(rows, dst_stride), by_id.cpu().numpy()[:n_img], guards_ok, src_same


def check_merge(dev, P, dst_stride):
    rc, info, out, by_id, guards_ok, src_same = run_entry(dev, P, dst_stride)
    assert rc == 0 and info.tolist() == [0, P.total, 0, 0], (rc, info.tolist(), P.total)
    assert guards_ok and src_same
    assert np.array_equal(out[:P.total, :P.width], P.want.view(np.uint32)), "dst is not the numpy permutation"
    assert (out[:P.total, P.width:] == POISON).all(), "the gap of a wider dst stride was written"
    assert (out[P.total:] == POISON).all(), "rows behind the total were written"
    assert np.array_equal(by_id, P.count_by_id)


WORLDS = (1, 2, 3, 8)
# (width, src_stride - width, dst_stride - width, shuffled): every width, both strides wider and not, both assignments -- dealt
# round robin over the (world, n_images) grid below, and crossed in full at world 3, 37 images
VARIANTS = [(w, ds, dd, sh) for w in (3, 12, 18) for ds, dd in ((0, 0), (5, 0), (0, 2), (1, 7)) for sh in (False, True)]
GRID = [(world, n) for world in WORLDS for n in sorted({0, 1, world - 1, 37, 4099})]


@pytest.mark.parametrize("k", range(len(GRID)), ids=[f"world{w}-images{n}" for w, n in GRID])
def test_every_world_and_image_count(dev, k):
    """world in {1, 2, 3, 8} x n_images_total in {0, 1, world - 1, 37, 4099}: counts from {0, 0, 1, 2, 65, 300} and one image of
    1500 rows; fewer images than ranks leaves ranks empty."""
    world, n = GRID[k]
    for wi in range(3):                                           # widths 3, 12, 18 at every grid point, the other axes dealt round robin
        w, ds, dd, sh = VARIANTS[8 * wi + (3 * k + 3 * wi) % 8]
        check_merge(dev, problem(world, n, w, w + ds, sh, k), w + dd)


@pytest.mark.parametrize("v", range(len(VARIANTS)), ids=[f"w{w}-src+{ds}-dst+{dd}-{'shuffled' if sh else 'strided'}" for w, ds, dd, sh in VARIANTS])
def test_every_width_stride_and_assignment(dev, v):
    w, ds, dd, sh = VARIANTS[v]
    check_merge(dev, problem(3, 37, w, w + ds, sh, 100 + v), w + dd)


def _refused(dev, P, flag, **kw):
    rc, info, out, _, guards_ok, src_same = run_entry(dev, P, P.width + 1, **kw)
    assert rc == 0 and info[0] & flag, (info.tolist(), flag)
    assert guards_ok and src_same and (out == POISON).all(), "a call that reports an inconsistency must copy nothing"
    return info


def test_inconsistent_inputs_set_info_and_copy_nothing(dev):
    P = problem(3, 37, 12, 12, False, 7)
    r, j = 1, 4
    far, neg, twice, one_more = P.img_id.copy(), P.img_id.copy(), P.img_id.copy(), P.counts.copy()
    far[r, j], neg[r, j], twice[r, j] = 37, -1, P.img_id[0, 2]
    one_more[r, j] += 1
    _refused(dev, P, 1, img_id=far)
    _refused(dev, P, 1, img_id=neg)
    _refused(dev, P, 1, n_images_total=36)                        # (id 36 exists)
    assert int(_refused(dev, P, 2, img_id=twice)[2]) == int(P.img_id[0, 2])
    assert int(_refused(dev, P, 4, counts=one_more)[3]) == r
    short = list(P.rows_per_run)
    short[2] -= 1
    assert int(_refused(dev, P, 4, rows_per_run=short)[3]) == 2
    info = _refused(dev, P, 8, dst_rows=P.total - 1)
    assert int(info[1]) == P.total                                # (the total is reported all the same)


def test_argument_refusals_follow_no_device_pointer(dev):
    """Every refusal with the device pointers src / counts / img_id / dst NULL -- legal for runs without rows and images, so that
    the argument under test is the only thing wrong -- and info poisoned: had anything reached the device, info would be written."""
    L = L_()
    info = torch.full((4,), -5, dtype=torch.int32, device=dev)
    ws = torch.empty(L.obb_stats_merge_workspace_bytes(4) + 256, dtype=torch.uint8, device=dev)
    base = dict(rows=(0, 0), images=(0, 0), src=0, counts=0, img_id=0, dst=0, dst_rows=0, info=info.data_ptr(), ws=ws.data_ptr())
    assert ws.data_ptr() % 256 == 0
    n = 0
    for rc, kw in SC.refusals():
        if set(kw) & {"src", "counts", "img_id", "dst"}:
            continue                                             # (NULL where there is something to read or write: below)
        kw = dict(kw)
        if "ws" in kw:
            kw["ws"] = ws.data_ptr() + (kw["ws"] - 4096) if kw["ws"] else 0
        assert SC.call_refused(L, C, **dict(base, **kw)) == rc, kw
        n += 1
    assert n >= 14
    for name in ("src", "counts", "img_id", "dst"):                # rows, images and a dst capacity, and the pointer to them NULL
        real = dict(base, rows=(5, 8), images=(2, 2), dst_rows=13, src=ws.data_ptr(), counts=ws.data_ptr(), img_id=ws.data_ptr(), dst=ws.data_ptr())
        assert SC.call_refused(L, C, **dict(real, **{name: 0})) == -1, name
    torch.cuda.synchronize(dev)
    assert info.tolist() == [-5] * 4


# ------------------------------------------------------------------------------------------------ ValStats
def _shapes(bs):
    return [((1100, 1100), ((1.0, 1.0), (0.0, 0.0)))] * bs


def _images():
    """13 images (pred (n, 7), labels (m, 6)): the stored batch of tests/obbmetric_cases.py (its image 0 has no detections, image 1
    no labels), three stored single images, an image with neither, and seeded ones of 2-3 classes."""
    def make():
        preds, targets, _ = OC.load("bs5")
        ims = [(p, OC.labels_of(targets, b)[0]) for b, p in enumerate(preds)]
        ims.insert(2, (torch.zeros(0, 7), torch.zeros(0, 6)))
        ims += [OC.load(name)[:2] for name in ("n70_m9", "n1_m1", "n300_m40")]
        g = torch.Generator().manual_seed(11)
        ims += [OC.make_image(g, n, m, nc) for n, m, nc in ((33, 0, 2), (0, 5, 2), (90, 30, 3), (7, 7, 2))]
        return ims
    if "images" not in _memo:
        _memo["images"] = make()
    return _memo["images"]


def _feed(dev, ids, obb=True, bs=4):
    """A ValStats and a ConfusionMatrix fed the images `ids` in that order, in batches of bs, with their ids."""
    from yolov5_obb_amd import val as V
    from yolov5_obb_amd.utils import metrics
    vs, cm = V.ValStats(niou=NIOU, device=dev, capacity=64, obb=obb), metrics.ConfusionMatrix(nc=3, device=dev)
    iouv, ims = OC.IOUV.to(dev), _images()
    for b0 in range(0, len(ids), bs):
        part = ids[b0:b0 + bs]
        preds = [ims[i][0].to(dev) for i in part]
        targets = torch.cat([torch.cat((torch.full((ims[i][1].shape[0], 1), float(b)), ims[i][1]), 1) for b, i in enumerate(part)], 0)
        vs.add_batch(preds, targets.to(dev), _shapes(len(part)), iouv, confusion=cm, image_ids=part)
    return vs, cm


def _single(dev):
    if "single" not in _memo:
        vs, cm = _feed(dev, list(range(len(_images()))))
        _memo["single"] = (vs, cm, vs.ap_per_class(), vs.ap_per_class_obb(), cm._counters(dev).cpu())
    return _memo["single"]


def test_add_batch_keeps_rows_labels_and_id_of_every_image(dev):
    from yolov5_obb_amd import val as V
    vs, _, _, _, _ = _single(dev)
    ims = _images()
    assert vs.k == len(ims) and vs.img_rows.dtype == torch.int32 and vs.img_labels.dtype == torch.int32 and vs.img_ids.dtype == torch.int64
    assert vs.img_rows.tolist() == [p.shape[0] for p, _ in ims] and vs.img_labels.tolist() == [l.shape[0] for _, l in ims]
    assert vs.img_ids.tolist() == list(range(len(ims)))
    assert 0 in vs.img_rows.tolist() and 0 in vs.img_labels.tolist() and (0, 0) in zip(vs.img_rows.tolist(), vs.img_labels.tolist())
    # the default ids are a running index, and the statistics do not depend on the ids
    plain = V.ValStats(niou=NIOU, device=dev, capacity=64)
    iouv = OC.IOUV.to(dev)
    for b0 in (0, 4):
        preds = [ims[i][0].to(dev) for i in range(b0, b0 + 4)]
        targets = torch.cat([torch.cat((torch.full((ims[b0 + b][1].shape[0], 1), float(b)), ims[b0 + b][1]), 1) for b in range(4)], 0)
        plain.add_batch(preds, targets.to(dev), _shapes(4), iouv)
    assert plain.img_ids.tolist() == list(range(8)) and plain.img_rows.tolist() == vs.img_rows.tolist()[:8]
    assert torch.equal(plain.rows, vs.rows[:plain.n]) and torch.equal(plain.target_cls, vs.target_cls[:plain.m])
    with pytest.raises(RuntimeError):
        plain.add_batch(preds, targets.to(dev), _shapes(4), iouv, image_ids=[1, 2])


@pytest.mark.parametrize("world", [2, 3, 8])
def test_merged_equals_one_accumulator(dev, world):
    from yolov5_obb_amd import val as V
    one, _, ap, ap_obb, mat = _single(dev)
    n = len(_images())
    parts = [_feed(dev, list(range(r, n, world))) for r in range(world)]
    mg = V.ValStats.merged([vs for vs, _ in parts])
    assert (mg.n, mg.m, mg.k) == (one.n, one.m, one.k) and mg.supplied == one.k and one.supplied is None
    assert torch.equal(mg.rows, one.rows) and torch.equal(mg.rows_obb, one.rows_obb) and torch.equal(mg.target_cls, one.target_cls)
    assert torch.equal(mg.img_rows, one.img_rows) and torch.equal(mg.img_labels, one.img_labels) and torch.equal(mg.img_ids, one.img_ids)
    got, got_obb = mg.ap_per_class(), mg.ap_per_class_obb()
    assert len(got) == 7 and all(np.array_equal(a, b) for a, b in zip(got, ap))
    assert len(got_obb) == 7 and all(np.array_equal(a, b) for a, b in zip(got_obb, ap_obb))
    assert float(ap[5][:, 0].mean()) > 0.0 and mg.any_tp
    assert torch.equal(sum(cm._counters(dev).cpu() for _, cm in parts), mat) and int(mat.sum()) > 0


def test_merged_reports_an_image_two_parts_hold(dev):
    from yolov5_obb_amd import val as V
    a, b = _feed(dev, [0, 5, 3])[0], _feed(dev, [1, 5])[0]
    mg = V.ValStats.merged([a, b], n_images_total=6)
    with pytest.raises(RuntimeError, match="image 5 produced by two ranks"):
        mg.ap_per_class()
    with pytest.raises(RuntimeError, match="image 5 produced by two ranks"):
        mg.cpu()
    with pytest.raises(RuntimeError, match="outside"):
        V.ValStats.merged([a], n_images_total=4).ap_per_class()


def test_equal_confidences_across_ranks_keep_the_single_process_order(dev):
    """W = 2: image 1 (rank 1) holds a true positive, image 2 (rank 0) a false positive of the same class and exactly the same
    conf.  In image order the true positive comes first; rank-major concatenation puts rank 0's false positive first, and AP drops."""
    from yolov5_obb_amd import val as V
    from yolov5_obb_amd.utils import metrics
    iouv = OC.IOUV.to(dev)
    box = [500.0, 500.0, 100.0, 40.0, 0.0]
    ims = [(torch.zeros(0, 7), torch.tensor([[0.0, 200.0, 200.0, 50.0, 20.0, 0.0]])),                    # image 0: a label nobody finds
           (torch.tensor([box + [0.5, 0.0]]), torch.tensor([[0.0] + box])),                              # image 1: a true positive
           (torch.tensor([box + [0.5, 0.0]]), torch.tensor([[0.0, 900.0, 900.0, 100.0, 40.0, 0.0]]))]    # image 2: a false positive

    def feed(ids):
        vs = V.ValStats(niou=NIOU, device=dev, capacity=8, obb=True)
        for i in ids:                                              # (batches of one)
            p, lab = ims[i]
            vs.add_batch([p.to(dev)], torch.cat((torch.zeros(lab.shape[0], 1), lab), 1).to(dev), _shapes(1), iouv, image_ids=[i])
        return vs
    one, r0, r1 = feed([0, 1, 2]), feed([0, 2]), feed([1])
    assert one.rows[:, 0].tolist() == [1.0, 0.0] and one.rows[:, NIOU].tolist() == [0.5, 0.5] and one.rows[:, NIOU + 1].tolist() == [0.0, 0.0]
    mg = V.ValStats.merged([r0, r1])
    assert torch.equal(mg.rows, one.rows) and torch.equal(mg.rows_obb, one.rows_obb) and torch.equal(mg.target_cls, one.target_cls)
    want, got = one.ap_per_class(), mg.ap_per_class()
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    cat = metrics.ap_from_rows(torch.cat((r0.rows, r1.rows), 0), torch.cat((r0.target_cls, r1.target_cls), 0), NIOU)[0]
    assert not np.array_equal(cat[5], want[5]), "the tie does not decide AP: the case has no teeth"
    assert float(want[5][0, 0]) > float(cat[5][0, 0])


# ------------------------------------------------------------------------------------------------ the workspace contract
def merge_case(key, dst_stride):
    P = problem(*key)
    rows = P.total + 3
    i64 = C.c_int64 * P.world

    def call(L, Pt, ws, wsb, st, mark):
        v = lambda x: C.c_void_p(int(x)) if x else C.c_void_p(0)
        return L.obb_stats_merge_f32(v(Pt["src"]), P.src_stride, P.run_stride, i64(*P.rows_per_run), v(Pt["counts"]), v(Pt["img_id"]), P.K,
                                     i64(*P.images_per_run), P.world, P.n_images, P.width, v(Pt["dst"]), dst_stride, rows, v(Pt["by_id"]),
                                     v(Pt["info"]), v(ws), wsb, v(st))

    def verify(O):
        info, by_id = O("info", np.int32), O("by_id", np.int32)
        out = O("dst", np.uint32).reshape(rows, dst_stride)
        assert info.tolist() == [0, P.total, 0, 0] and np.array_equal(by_id, P.count_by_id)
        assert np.array_equal(out[:P.total, :P.width], P.want.view(np.uint32))
        assert (out[:P.total, P.width:].view(np.uint8) == AC.FILL).all() and (out[P.total:].view(np.uint8) == AC.FILL).all()
        return [info, by_id, out[:P.total, :P.width].copy()]

    return AC.Case(f"stats_merge-{key}", ["obb_stats_merge_f32"], dict(src=P.src, counts=P.counts, img_id=P.img_id),
                   dict(dst=rows * dst_stride * 4, by_id=P.n_images * 4, info=16), lambda L: L.obb_stats_merge_workspace_bytes(P.n_images), call, verify)


BIG_KEY, SMALL_KEY = (8, 4099, 12, 12, True, 3), (3, 37, 18, 19, False, 4)


@pytest.mark.parametrize("key,dst_stride,donor", [(BIG_KEY, 12, SMALL_KEY), (SMALL_KEY, 21, BIG_KEY)])
def test_exact_poisoned_workspace_between_canaries(dev, key, dst_stride, donor):
    AC.run_poisons(L_(), dev, merge_case(key, dst_stride), merge_case(donor, 18))


@pytest.mark.parametrize("ws_mode", ["short", "null", "+8", "+128"])
def test_a_short_missing_or_misaligned_workspace_is_refused_before_anything_is_written(dev, ws_mode):
    AC.run_refused(L_(), dev, merge_case(SMALL_KEY, 21), ws_mode)


def test_all_work_is_enqueued_on_the_callers_stream(dev):
    from tests.test_abi_contract_gpu import DELAY_ITERS, _seed_matrix
    res, pending = AC.run_on_side_stream(L_(), dev, merge_case(BIG_KEY, 12), DELAY_ITERS, _seed_matrix(dev))
    assert pending, "the delay had drained before the ABI call returned: the run proves nothing"
