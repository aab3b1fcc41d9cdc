"""GPU: process_batch with the rotated IoU (csrc/head.hip: k_vo_match + k_vt_stats behind obb_process_batch_obb_f32 /
obb_val_tail_batch_obb_f32; val.process_batch_obb, val.val_tail_batch_obb, ValStats(obb=True), val_sharded.run(obb_metrics=True))
against the outputs frozen from the reference's val.process_batch (tests/golden/obbmetric_cases.npz) and against the pinned rule
restated on the oracle's IoU matrix (tests/obbmetric_cases.py).  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import obbmetric_cases as OC

pytestmark = pytest.mark.gpu
NIOU = 10


def _pb(dev, pred, labels, iouv=OC.IOUV):
    from yolov5_obb_amd.val import process_batch_obb
    c, ml, mi = process_batch_obb(pred.to(dev), labels.to(dev), iouv.to(dev), return_match=True)
    assert c.dtype == torch.bool and ml.dtype == torch.int32 and mi.dtype == torch.float32
    return c.cpu().numpy(), ml.cpu().numpy(), mi.cpu().numpy()


def _pairs_bits(dev, labels5, pred, ml):
    """ops.rotated_iou_pairs(label[match_label[d]], pred[d]) on the device as raw bits; -1.0 where nothing was kept."""
    from yolov5_obb_amd import ops
    want = np.full(len(ml), -1.0, dtype=np.float32)
    hit = np.flatnonzero(ml >= 0)
    if len(hit):
        a = labels5[torch.from_numpy(ml[hit]).long()].to(dev)
        want[hit] = ops.rotated_iou_pairs(a, pred[torch.from_numpy(hit), :5].to(dev)).cpu().numpy()
    return want.view(np.uint32)


def _images():
    """(id, pred, labels, golden correct) of every stored image, the batch's images one by one."""
    out = []
    for name in OC.SINGLE:
        out.append((name,) + OC.load(name))
    preds, targets, correct = OC.load("bs5")
    off = np.cumsum([0] + [p.shape[0] for p in preds])
    for b, p in enumerate(preds):
        out.append((f"bs5_{b}", p, OC.labels_of(targets, b)[0], correct[off[b]:off[b + 1]]))
    return out


@pytest.mark.parametrize("case", _images(), ids=lambda c: c[0])
def test_process_batch_obb_equals_the_reference_and_reports_its_match(dev, case):
    _, pred, labels, want = case
    got, ml, mi = _pb(dev, pred, labels)
    assert got.shape == tuple(want.shape) and np.array_equal(got, want.numpy())
    rc, rl, ri = OC.rule(OC.riou(labels, pred) if len(pred) and len(labels) else np.zeros((len(labels), len(pred))), labels[:, 0].numpy(),
                         pred[:, 6].numpy(), OC.IOUV.numpy())
    assert np.array_equal(ml, rl)
    assert np.array_equal(mi.view(np.uint32), _pairs_bits(dev, labels[:, 1:6], pred, ml))
    assert np.array_equal(mi >= 0.5, ml >= 0) and np.array_equal(mi == -1.0, ml < 0)


def _raw_batch(dev, preds, targets, iouv=OC.IOUV, gaps=False):
    """obb_val_tail_batch_obb_f32 through the raw C ABI: packed, or (gaps) every image's rows at a row of its own between rows of
    NaN that must never be read (det_row_host)."""
    from yolov5_obb_amd import _lib
    L = _lib.lib()
    counts = [p.shape[0] for p in preds]
    off = np.cumsum([0] + counts).astype(np.int64)
    n, bs = int(off[-1]), len(preds)
    if gaps:
        rows, chunks, at = [], [], 0
        for p in preds:
            chunks += [torch.full((3, 7), float("nan")), p]
            rows.append(at + 3)
            at += 3 + p.shape[0]
        det = torch.cat(chunks + [torch.full((2, 7), float("nan"))], 0).to(dev)
        det_row = C.cast((C.c_int64 * bs)(*rows), C.c_void_p)
    else:
        det, det_row = torch.cat(preds, 0).to(dev), C.c_void_p(0)
    tg, iv = targets.to(dev).contiguous(), iouv.to(dev)
    stats = torch.full((n, NIOU + 2), -7.0, device=dev)
    ml = torch.full((n,), -9, dtype=torch.int32, device=dev)
    mi = torch.full((n,), -9.0, device=dev)
    rc = L.obb_val_tail_batch_obb_f32(_lib.ptr(det), det_row, C.cast((C.c_int64 * (bs + 1))(*off.tolist()), C.c_void_p), bs, _lib.ptr(tg),
                                      tg.shape[0], tg.shape[1], _lib.ptr(iv), NIOU, _lib.ptr(stats), _lib.ptr(ml), _lib.ptr(mi),
                                      _lib.stream_ptr(dev))
    assert rc == 0
    torch.cuda.synchronize(dev)
    return stats.cpu().numpy(), ml.cpu().numpy(), mi.cpu().numpy()


def test_val_tail_batch_obb_equals_the_reference_and_the_per_image_entry(dev):
    from yolov5_obb_amd.val import val_tail_batch_obb
    preds, targets, want = OC.load("bs5")
    counts = [p.shape[0] for p in preds]
    tail, match = val_tail_batch_obb([p.to(dev) for p in preds], targets.to(dev), OC.IOUV.to(dev), return_match=True)
    assert len(tail) == 5 and [t[0].shape[0] for t in tail] == counts
    got = torch.cat([t[0] for t in tail], 0)
    assert got.dtype == torch.bool and np.array_equal(got.numpy(), want.numpy())
    for b, p in enumerate(preds):
        assert torch.equal(tail[b][1], p[:, 5]) and torch.equal(tail[b][2], p[:, 6])
    # the per-image entry on every image: the same rows and the same match (label rows counted in `targets`)
    ml = torch.cat([m[0] for m in match]).cpu().numpy()
    mi = torch.cat([m[1] for m in match]).cpu().numpy()
    at = 0
    for b, p in enumerate(preds):
        lab, rows = OC.labels_of(targets, b)
        c1, l1, i1 = _pb(dev, p, lab)
        sl = slice(at, at + p.shape[0])
        assert np.array_equal(c1, got.numpy()[sl])
        assert np.array_equal(np.where(l1 >= 0, rows.numpy()[np.maximum(l1, 0)] if len(rows) else -1, -1), ml[sl])
        assert np.array_equal(i1.view(np.uint32), mi[sl].view(np.uint32))
        at += p.shape[0]
    rc, rl, _ = OC.rule_batch(preds, targets, OC.IOUV.numpy())
    assert np.array_equal(ml, rl) and np.array_equal(rc, want.numpy())
    # the raw entry, packed and with det_row_host: rows [correct as 0 / 1, conf, cls], bit-identical to each other
    packed, gapped = _raw_batch(dev, preds, targets), _raw_batch(dev, preds, targets, gaps=True)
    allp = torch.cat(preds, 0).numpy()
    assert np.array_equal(packed[0][:, :NIOU], want.numpy().astype(np.float32))
    assert np.array_equal(packed[0][:, NIOU], allp[:, 5]) and np.array_equal(packed[0][:, NIOU + 1], allp[:, 6])
    assert np.array_equal(packed[1], ml) and np.array_equal(packed[2].view(np.uint32), mi.view(np.uint32))
    for a, b in zip(packed, gapped):
        assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)
    # the same rows with the labels in another order of rows (the images interleaved): nothing depends on their grouping
    perm = torch.randperm(targets.shape[0], generator=torch.Generator().manual_seed(1))
    mixed = _raw_batch(dev, preds, targets[perm])
    assert np.array_equal(mixed[0], packed[0])
    assert np.array_equal(np.where(mixed[1] >= 0, perm.numpy()[np.maximum(mixed[1], 0)], -1), packed[1])


def test_exact_ties_go_to_the_lower_label_and_the_lower_detection(dev):
    pred, labels, _ = OC.load("n300_m40")
    # every label row twice, the copies in front in reverse order: label j = 40 + (39 - j') ... each detection meets two equal IoUs
    lab2 = torch.cat((labels.flip(0), labels), 0)
    got, ml, mi = _pb(dev, pred, lab2)
    base, bl, bi = _pb(dev, pred, labels)
    assert np.array_equal(got, base) and np.array_equal(mi.view(np.uint32), bi.view(np.uint32))
    assert np.array_equal(ml, np.where(bl >= 0, 39 - bl, -1)) and int((ml >= 0).sum()) >= 30      # the copy in front, never the original
    rc, rl, _ = OC.rule(OC.riou(lab2, pred), lab2[:, 0].numpy(), pred[:, 6].numpy(), OC.IOUV.numpy())
    assert np.array_equal(got, rc) and np.array_equal(ml, rl)
    # every detection three times, back to back in blocks of 300: only the first copy can win a label
    pred3 = torch.cat((pred, pred, pred), 0)
    got3, ml3, mi3 = _pb(dev, pred3, labels)
    assert np.array_equal(got3[:300], base) and not got3[300:].any()
    assert np.array_equal(ml3, np.tile(bl, 3)) and np.array_equal(mi3.view(np.uint32), np.tile(bi, 3).view(np.uint32))
    rc3 = OC.rule(OC.riou(labels, pred3), labels[:, 0].numpy(), pred3[:, 6].numpy(), OC.IOUV.numpy())[0]
    assert np.array_equal(got3, rc3)


@pytest.mark.parametrize("thr0", [0.0, -1.0])
def test_a_first_level_of_zero_or_less_makes_every_pair_of_a_class_a_candidate(dev, thr0):
    pred, labels, _ = OC.load("n70_m9")
    iouv = torch.cat((torch.tensor([thr0]), OC.IOUV[1:]))
    iou = OC.riou(labels, pred)
    same = labels[:, 0:1].numpy() == pred[:, 6].numpy()[None, :]
    assert int((same & (iou == 0)).sum()) > 100, "pairs far apart, IoU exactly 0, are candidates here"
    got, ml, mi = _pb(dev, pred, labels, iouv)
    rc, rl, ri = OC.rule(iou, labels[:, 0].numpy(), pred[:, 6].numpy(), iouv.numpy())
    assert np.array_equal(got, rc) and np.array_equal(ml, rl)
    assert np.array_equal(mi.view(np.uint32), _pairs_bits(dev, labels[:, 1:6], pred, ml))
    assert (ml >= 0).all() and int((mi == 0).sum()) > 20 and not got[mi == 0][:, 1:].any()


def test_non_finite_rows_match_nothing_and_change_nothing_else(dev):
    pred, labels, _ = OC.load("n300_m40")
    base, bl, bi = _pb(dev, pred, labels)
    bad_d = torch.tensor([[float("nan"), 300.0, 40.0, 12.0, 0.3, 0.99, 0.0], [300.0, float("inf"), 40.0, 12.0, 0.3, 0.98, 1.0],
                          [300.0, 300.0, float("inf"), 12.0, 0.3, 0.97, 0.0], [300.0, 300.0, 40.0, 12.0, float("nan"), 0.96, 1.0]])
    bad_l = torch.tensor([[0.0, float("nan"), 300.0, 40.0, 12.0, 0.3], [1.0, 300.0, 300.0, float("inf"), 12.0, 0.3],
                          [0.0, 300.0, -float("inf"), 40.0, 12.0, 0.3], [1.0, 300.0, 300.0, 40.0, 12.0, float("nan")]])
    pred2, lab2 = torch.cat((bad_d, pred), 0), torch.cat((bad_l, labels), 0)       # in front: every index behind them moves
    got, ml, mi = _pb(dev, pred2, lab2)
    assert not got[:4].any() and (ml[:4] == -1).all() and (mi[:4] == -1).all()
    assert not np.isin(ml, [0, 1, 2, 3]).any()
    assert np.array_equal(got[4:], base) and np.array_equal(ml[4:], np.where(bl >= 0, bl + 4, -1))
    assert np.array_equal(mi[4:].view(np.uint32), bi.view(np.uint32))


def test_argument_checks_leave_the_outputs_untouched_and_no_detections_launch_nothing(dev):
    from yolov5_obb_amd import _lib
    L = _lib.lib()
    pred, labels, _ = OC.load("n70_m9")
    det, lab, iv = pred.to(dev), labels.to(dev), OC.IOUV.to(dev)
    tg = torch.cat((torch.zeros(9, 1), labels), 1).to(dev)
    correct = torch.full((70, NIOU), 0xC3, dtype=torch.uint8, device=dev)
    stats = torch.full((70, NIOU + 2), -7.0, device=dev)
    ml = torch.full((70,), -9, dtype=torch.int32, device=dev)
    mi = torch.full((70,), -9.0, device=dev)
    p, st, null = _lib.ptr, _lib.stream_ptr(dev), C.c_void_p(0)
    off = lambda *v: C.cast((C.c_int64 * len(v))(*v), C.c_void_p)           # noqa: E731
    pb, vt = L.obb_process_batch_obb_f32, L.obb_val_tail_batch_obb_f32
    assert pb(p(det), 70, p(lab), 9, p(iv), 0, p(correct), p(ml), p(mi), st) == -1
    assert pb(p(det), 70, p(lab), 9, p(iv), 17, p(correct), p(ml), p(mi), st) == -1
    assert pb(p(det), 70, null, 9, p(iv), NIOU, p(correct), p(ml), p(mi), st) == -1
    assert pb(p(det), 70, p(lab), 9, p(iv), NIOU, p(correct), null, p(mi), st) == -1
    assert pb(p(det), 70, p(lab), 9, p(iv), NIOU, p(correct), p(ml), null, st) == -1
    assert pb(p(det), 0, p(lab), 9, p(iv), NIOU, p(correct), p(ml), p(mi), st) == 0
    assert vt(p(det), null, off(0, 70), 0, p(tg), 9, 7, p(iv), NIOU, p(stats), p(ml), p(mi), st) == -1
    assert vt(p(det), null, off(*range(66)), 65, p(tg), 9, 7, p(iv), NIOU, p(stats), p(ml), p(mi), st) == -1
    assert vt(p(det), null, off(0, 70), 1, p(tg), 9, 6, p(iv), NIOU, p(stats), p(ml), p(mi), st) == -1
    assert vt(p(det), null, off(0, 70), 1, p(tg), 9, 7, p(iv), 17, p(stats), p(ml), p(mi), st) == -1
    assert vt(p(det), null, off(0, 70), 1, p(tg), 9, 7, p(iv), NIOU, null, p(ml), p(mi), st) == -1
    assert vt(p(det), null, off(0, 70), 1, p(tg), 9, 7, p(iv), NIOU, p(stats), null, p(mi), st) == -1
    assert vt(p(det), null, off(0, 70, 60), 2, p(tg), 9, 7, p(iv), NIOU, p(stats), p(ml), p(mi), st) == -1
    assert vt(p(det), null, off(0, 0, 0), 2, p(tg), 9, 7, p(iv), NIOU, p(stats), p(ml), p(mi), st) == 0
    torch.cuda.synchronize(dev)
    assert bool((correct == 0xC3).all()) and bool((stats == -7.0).all()) and bool((ml == -9).all()) and bool((mi == -9.0).all())
    # no labels: zero rows, labels -1, IoUs -1 (m == 0 / nt == 0 with NULL label pointers)
    assert pb(p(det), 70, null, 0, p(iv), NIOU, p(correct), p(ml), p(mi), st) == 0
    assert vt(p(det), null, off(0, 70), 1, null, 0, 0, p(iv), NIOU, p(stats), p(ml), p(mi), st) == 0
    torch.cuda.synchronize(dev)
    assert not bool(correct.any()) and bool((ml == -1).all()) and bool((mi == -1.0).all())
    assert not bool(stats[:, :NIOU].any()) and torch.equal(stats[:, NIOU:].cpu(), pred[:, 5:7])


def _shapes(bs):
    return [((1100, 1100), ((1.0, 1.0), (0.0, 0.0)))] * bs


def test_valstats_obb_rows_and_metrics_beside_unchanged_hbb_ones(dev):
    from yolov5_obb_amd import val as V
    from yolov5_obb_amd.utils import metrics
    iouv = OC.IOUV.to(dev)
    batches = [OC.load("bs5")[:2]]
    p, lab, _ = OC.load("n300_m40")
    batches.append(([p], torch.cat((torch.zeros(40, 1), lab), 1)))
    p, lab, _ = OC.load("n70_m9")
    batches.append(([p, p[:0]], torch.cat((torch.zeros(9, 1), lab), 1)))
    plain, both = V.ValStats(niou=NIOU, device=dev, capacity=64), V.ValStats(niou=NIOU, device=dev, capacity=64, obb=True)
    want = []
    for preds, targets in batches:
        for vs in (plain, both):
            vs.add_batch([q.to(dev) for q in preds], targets.to(dev), _shapes(len(preds)), iouv)
        rc, rl, _ = OC.rule_batch(preds, targets, OC.IOUV.numpy())
        allp = torch.cat(preds, 0).numpy()
        want.append(np.concatenate((rc.astype(np.float32), allp[:, 5:7]), 1))
        assert np.array_equal(both.last_match[0].cpu().numpy(), rl)
    want = np.concatenate(want, 0)
    assert both.n == plain.n == want.shape[0]
    assert np.array_equal(both.rows_obb.cpu().numpy(), want)
    assert torch.equal(both.rows, plain.rows) and torch.equal(both.target_cls, plain.target_cls)
    for a, b in zip(both.ap_per_class(), plain.ap_per_class()):
        assert np.array_equal(a, b)
    ref, info = metrics.ap_from_rows(torch.from_numpy(want).to(dev), both.target_cls, NIOU)
    got = both.ap_per_class_obb()
    assert len(got) == 7 and all(np.array_equal(a, b) for a, b in zip(got, ref))
    assert both.any_tp_obb and info[1] == int(want[:, 0].sum()) and float(got[5][:, 0].mean()) > 0.0
    c, conf, pcls, tcls = both.cpu_obb()
    assert np.array_equal(c, want[:, :NIOU] > 0.5) and np.array_equal(conf, want[:, NIOU]) and np.array_equal(pcls, want[:, NIOU + 1])
    assert np.array_equal(tcls, plain.cpu()[3])
    # the oriented rows differ from the horizontal ones on this input (a hull can agree where the boxes do not)
    assert not np.array_equal(both.rows_obb.cpu().numpy(), both.rows.cpu().numpy())
    with pytest.raises(RuntimeError):
        plain.rows_obb
    with pytest.raises(RuntimeError):
        plain.ap_per_class_obb()


def test_val_sharded_reports_the_oriented_metrics_beside_the_horizontal_ones(dev):
    """The tiny synthetic loader of tests/test_valpost_gpu.py::test_sharded_val_loop_hip_vs_oracle (6 images in batches of 3, a
    stand-in model over seeded predictions); every third label is moved onto a prediction the model will make, so that both
    metrics have something to count."""
    from tests import synth
    from yolov5_obb_amd import val_sharded
    from yolov5_obb_amd.utils import metrics
    from yolov5_obb_amd.utils.general import non_max_suppression_obb

    class Set(torch.utils.data.Dataset):
        def __len__(self):
            return 6

        def __getitem__(self, i):
            g = torch.Generator().manual_seed(70 + i)
            im = torch.randint(0, 256, (3, 64, 64), dtype=torch.uint8, generator=g)
            nl = 12
            lab = torch.zeros(nl, 7)
            lab[:, 1] = torch.randint(0, 15, (nl,), generator=g).float()
            lab[:, 2:4] = torch.rand(nl, 2, generator=g) * 1000
            lab[:, 4] = torch.rand(nl, generator=g) * 120 + 20
            lab[:, 5] = torch.rand(nl, generator=g) * 30 + 8
            lab[:, 6] = (torch.rand(nl, generator=g) - 0.5) * 3.0
            return im, lab, f"i{i}", ((1300, 1400), ((0.7314, 0.7314), (12.0, 3.5)))

        @staticmethod
        def collate_fn(batch):
            im, lab, path, shapes = zip(*batch)
            for k, l in enumerate(lab):
                l[:, 0] = k
            return torch.stack(im, 0), torch.cat(lab, 0), path, shapes

    def model(im):
        key = int(im.float().sum().item()) % 100000
        return (synth.s_pred(im.shape[0], 3000, 15, seed=key % 1000, n_obj=30).to(dev),)
    kw = dict(conf_thres=0.25, iou_thres=0.45, half=False, device=dev, device_metrics=True)
    seen = []
    batches = []
    for im, targets, paths, shapes in torch.utils.data.DataLoader(Set(), batch_size=3, collate_fn=Set.collate_fn):
        out = non_max_suppression_obb(model(im.to(dev).float() / 255)[0], 0.25, 0.45, multi_label=True)     # (what run() hands the model)
        targets = targets.clone()
        for b, o in enumerate(out):                                # labels 0, 3, 6, 9 of the image: a detection of its own, shifted a little
            rows = torch.nonzero(targets[:, 0] == b)[:, 0][::3]
            k = min(len(rows), o.shape[0])
            targets[rows[:k], 2:7] = o[:k, :5].cpu() + torch.tensor([1.0, -1.0, 1.5, 0.5, 0.01])
            targets[rows[:k], 1] = o[:k, 6].cpu()
        batches.append((im, targets, paths, shapes))

    def nms(*a, **k):
        out = non_max_suppression_obb(*a, **k)
        seen.append([o.clone() for o in out])
        return out
    base = val_sharded.run(model, batches, **kw)
    res = val_sharded.run(model, batches, nms=nms, obb_metrics=True, **kw)
    assert "metrics_obb" not in base and base["metrics"] is not None and res["metrics"] is not None and res["metrics_obb"] is not None
    assert all(np.array_equal(a, b) for a, b in zip(base["metrics"], res["metrics"]))
    assert torch.equal(base["val_stats"].rows, res["val_stats"].rows)
    vs = res["val_stats"]
    want = np.concatenate([OC.rule_batch([o.cpu() for o in out], t[:, :7], OC.IOUV.numpy())[0] for out, (_, t, _, _) in zip(seen, batches)], 0)
    assert np.array_equal(vs.rows_obb[:, :NIOU].cpu().numpy() > 0.5, want) and int(want[:, 0].sum()) >= 6
    ref = metrics.ap_from_rows(vs.rows_obb, vs.target_cls, NIOU)[0]
    assert len(res["metrics_obb"]) == 7 and all(np.array_equal(a, b) for a, b in zip(res["metrics_obb"], ref))
    with pytest.raises(RuntimeError):
        val_sharded.run(model, batches, conf_thres=0.25, iou_thres=0.45, half=False, device=dev, obb_metrics=True)
