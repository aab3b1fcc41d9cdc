"""Device ap_per_class (csrc/metrics.hip behind yolov5_obb_amd.utils.metrics.ap_per_class), the device-resident accumulator
val.ValStats and val_sharded.run(device_metrics=True).

The golden file (tests/golden/ap_cases.npz) is the reference's own ap_per_class with np.argsort pinned to kind='stable' --
conf descending, ties by ascending row index, the order this package pins.  unique_classes, tp, fp and the best index are
equal exactly; ap, p, r, f1 within 1e-12 absolute: each is a double in [0, 1] built from exact integer counts by fewer than
~200 roundings (<= 2e-14), so 1e-12 leaves a 50x margin."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import ap_cases, synth, valtail_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-12
KEYS = ("tp", "fp", "p", "r", "f1", "ap", "classes")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "ap_cases.npz"))


def check_against(got, want, what=""):
    """got / want: 7-tuples (tp, fp, p, r, f1, ap, unique_classes)."""
    assert got[6].dtype == np.int32 and np.array_equal(got[6], want[6]), what
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), what
    for g, w, name in zip(got[2:6], want[2:6], KEYS[2:6]):
        assert g.dtype == np.float64 and g.shape == w.shape, (what, name)
        err = np.abs(g - w).max(initial=0.0)
        print(f"{what} {name}: max abs err {err:.3e}")
        assert err <= TOL, (what, name, err)


def identical(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(ap_cases.CASES))
def test_ap_per_class_matches_the_reference_in_stable_order(dev, golden, name):
    from yolov5_obb_amd import val
    from yolov5_obb_amd.utils import metrics
    tp, conf, pcls, tcls = ap_cases.build(name)
    niou = tp.shape[1]
    got_np = metrics.ap_per_class(tp, conf, pcls, tcls, names={})
    got_cu = metrics.ap_per_class(*(torch.from_numpy(x).to(dev) for x in (tp, conf, pcls, tcls)))
    assert identical(got_np, got_cu)
    if len(tcls) == 0:                    # no labels: the reference's empty shapes (its own argmax of an empty mean raises)
        assert [x.shape for x in got_np] == [(0,)] * 5 + [(0, niou), (0,)] and got_np[6].dtype == np.int32
        return
    want = [golden[f"{name}/{k}"] for k in KEYS]
    check_against(got_np, want, name)
    # the best F1 index, through the accumulator's view of the same rows
    rows = torch.from_numpy(np.concatenate((tp.astype(np.float32), conf[:, None], pcls[:, None]), 1)).to(dev)
    res, (best, tp0) = metrics.ap_from_rows(rows, torch.from_numpy(tcls).to(dev), niou)
    assert identical(res, got_np) and best == int(golden[f"{name}/best"]) and tp0 == int(tp[:, 0].sum())
    if len(conf) == 0:
        assert all(not np.any(x) for x in got_np[:6])


@pytest.mark.gpu
def test_row_order_matters_only_inside_groups_of_equal_conf(dev, golden):
    from yolov5_obb_amd.utils import metrics
    # distinct confidences: any shuffle of the rows leaves every output bit-identical
    tp, conf, pcls, tcls = ap_cases.build("n4097_nc5")
    conf = (np.random.RandomState(3).permutation(len(conf)) / np.float32(len(conf))).astype(np.float32)      # 4097 distinct values
    base = metrics.ap_per_class(tp, conf, pcls, tcls)
    assert 0.05 < base[5][:, 0].mean() < 0.999
    order = np.random.RandomState(4).permutation(len(conf))
    assert identical(base, metrics.ap_per_class(tp[order], conf[order], pcls[order], tcls))
    # ties: shuffling inside the groups of equal conf is another stable order -- the golden of the re-indexed input
    tp, conf, pcls, tcls = ap_cases.build("ties_floor100")
    assert len(np.unique(conf)) <= 100
    order = ap_cases.reindex_within_ties(conf, ap_cases.CASES["ties_floor100_reindexed"]["reindex"])
    assert np.array_equal(conf[order], conf) and not np.array_equal(order, np.arange(len(conf)))
    got = metrics.ap_per_class(tp[order], conf, pcls[order], tcls)
    check_against(got, [golden[f"ties_floor100_reindexed/{k}"] for k in KEYS], "reindexed")
    assert np.abs(got[5] - golden["ties_floor100/ap"]).max() > 1e-4          # (and the order inside the groups does matter)


@pytest.mark.gpu
def test_python_layer_rejects_what_the_kernels_cannot_rank(dev):
    from yolov5_obb_amd.utils import metrics
    tp, conf, pcls, tcls = ap_cases.build("n63_nc5")
    bad = conf.copy()
    bad[5] = np.nan
    with pytest.raises(RuntimeError, match="NaN"):
        metrics.ap_per_class(tp, bad, pcls, tcls)
    for arrs in ((tp, conf, np.where(np.arange(63) == 7, 256.0, pcls).astype(np.float32), tcls),
                 (tp, conf, pcls, np.append(tcls, np.float32(1.5))), (tp, conf, pcls, np.append(tcls, np.float32(-1)))):
        with pytest.raises(RuntimeError, match="class"):
            metrics.ap_per_class(*arrs)
    with pytest.raises(NotImplementedError):
        metrics.ap_per_class(tp, conf, pcls, tcls, plot=True)
    with pytest.raises(RuntimeError, match="eps"):
        metrics.ap_per_class(tp, conf, pcls, tcls, eps=1e-9)


def test_c_abi_argument_checks_answer_before_any_device_call():
    """niou / nc_max out of range (OBB_ERR_BAD_ARG = -1) and a short workspace (OBB_ERR_WORKSPACE = -2): nothing is launched,
    callable without a GPU (the pointers are never followed)."""
    from yolov5_obb_amd import _lib
    L = _lib.lib()
    p = C.c_void_p(4096)

    def call(n=100, niou=10, nc_max=16, ws_bytes=None, stride=12, m=10):
        need = L.obb_ap_per_class_workspace_bytes(n, niou, nc_max)
        return L.obb_ap_per_class_f32(p, stride, n, niou, p, m, nc_max, p, p, p, p, None, p, need if ws_bytes is None else ws_bytes, None)
    assert call(niou=0) == -1 and call(niou=17) == -1
    assert call(nc_max=257) == -1 and call(nc_max=0) == -1
    assert call(n=-1) == -1 and call(n=1 << 31) == -1 and call(m=-1) == -1
    assert call(stride=11) == -1                                       # rows shorter than niou + 2
    assert call(ws_bytes=L.obb_ap_per_class_workspace_bytes(100, 10, 16) - 1) == -2
    assert L.obb_ap_per_class_f32(p, 12, 100, 10, p, 10, 16, p, p, p, p, None, None, 1 << 30, None) == -2
    # the workspace is linear in n
    w1, w2 = L.obb_ap_per_class_workspace_bytes(1 << 20, 10, 16), L.obb_ap_per_class_workspace_bytes(1 << 21, 10, 16)
    assert 0 < w1 < w2 <= 2 * w1 and w1 <= (1 << 20) * (12 + 12 * 10) + (8 << 20)


def _tail_rows(preds, targets, shapes, iouv, dev):
    """The (n, niou + 2) rows val_tail_batch returns for a batch, as one host array."""
    from yolov5_obb_amd.val import val_tail_batch
    out = val_tail_batch([p.to(dev) for p in preds], targets.to(dev), shapes, iouv.to(dev))
    rows = [torch.cat((c.float(), s[:, None].float(), k[:, None].float()), 1) for c, s, k in out]
    return torch.cat(rows, 0).numpy() if rows else np.zeros((0, iouv.shape[0] + 2), np.float32)


@pytest.mark.gpu
def test_valstats_holds_the_rows_of_val_tail_batch(dev):
    from yolov5_obb_amd import val
    from yolov5_obb_amd.utils import metrics
    iouv = valtail_cases.IOUV
    vs = val.ValStats(niou=10, device=dev, capacity=64)               # every batch below crosses a capacity boundary
    want_rows, want_tcls = [], []
    for name in ("straddle", "two_images_one_block", "dense"):
        seed, images = valtail_cases.CASES[name]
        preds, targets, shapes = valtail_cases.make_batch(seed, images)
        want_rows.append(_tail_rows(preds, targets, shapes, iouv, dev))
        want_tcls.append(targets[:, 1].numpy())
        vs.add_batch([p.to(dev) for p in preds], targets.to(dev), shapes, iouv.to(dev))
        # earlier rows survive the growth; the new ones are val_tail_batch's bit for bit
        assert vs.rows.shape == (sum(len(r) for r in want_rows), 12)
        assert vs.rows.cpu().numpy().tobytes() == np.concatenate(want_rows, 0).tobytes()
        assert np.array_equal(vs.target_cls.cpu().numpy(), np.concatenate(want_tcls))
    correct, conf, pcls, tcls = vs.cpu()
    assert correct.dtype == bool and correct.shape == (vs.n, 10) and correct[:, 0].any() and vs.any_tp
    assert identical(vs.ap_per_class(), metrics.ap_per_class(correct, conf, pcls, tcls))
    # with the boxes: the same packed arrays val_tail_batch hands out
    seed, images = valtail_cases.CASES["straddle"]
    preds, targets, shapes = valtail_cases.make_batch(seed, images)
    _, (boxes_w, offs_w) = val.val_tail_batch([p.to(dev) for p in preds], targets.to(dev), shapes, iouv.to(dev), want_boxes=True)
    vs2 = val.ValStats(niou=10, device=dev)
    boxes, offs = vs2.add_batch([p.to(dev) for p in preds], targets.to(dev), shapes, iouv.to(dev), want_boxes=True)
    assert list(offs) == list(offs_w) and all(torch.equal(a, b) for a, b in zip(boxes, boxes_w))
    # labels only: classes are counted, nothing matched
    vs3 = val.ValStats(niou=10, device=dev)
    vs3.add_batch([torch.zeros(0, 7, device=dev)], targets[targets[:, 0] == 0].to(dev), shapes[:1], iouv.to(dev))
    res = vs3.ap_per_class()
    assert vs3.n == 0 and vs3.m > 0 and not vs3.any_tp and len(res[6]) > 0 and not res[5].any()


class _Set(torch.utils.data.Dataset):
    """Stand-in data in the format of LoadImagesAndLabels.collate_fn (as tests/test_valpost_gpu.py's loop test).  dets: per image
    the (k, 7) rows a first pass detected -- every third one becomes a label, so that the run has true positives, next to four
    random labels nothing matches; label_cls: one class for every label instead."""

    def __init__(self, dets=None, label_cls=None):
        self.dets, self.label_cls = dets, label_cls

    def __len__(self):
        return 6

    def __getitem__(self, i):
        g = torch.Generator().manual_seed(70 + i)
        im = torch.randint(0, 256, (3, 64, 64), dtype=torch.uint8, generator=g)
        nl = 4
        lab = torch.zeros(nl, 7)
        lab[:, 1] = torch.randint(0, 15, (nl,), generator=g).float()
        lab[:, 2:4] = torch.rand(nl, 2, generator=g) * 1000
        lab[:, 4] = torch.rand(nl, generator=g) * 120 + 20
        lab[:, 5] = torch.rand(nl, generator=g) * 30 + 8
        lab[:, 6] = (torch.rand(nl, generator=g) - 0.5) * 3.0
        if self.dets is not None:
            d = self.dets[i][::3]
            lab = torch.cat((lab, torch.cat((torch.zeros(len(d), 1), d[:, 6:7], d[:, :5]), 1)), 0)
        if self.label_cls is not None:
            lab[:, 1] = self.label_cls
        return im, lab, f"i{i}", ((1300, 1400), ((0.7314, 0.7314), (12.0, 3.5)))

    @staticmethod
    def collate_fn(batch):
        im, lab, path, shapes = zip(*batch)
        for k, l in enumerate(lab):
            l[:, 0] = k
        return torch.stack(im, 0), torch.cat(lab, 0), path, shapes


@pytest.mark.gpu
def test_sharded_val_loop_with_device_metrics(dev):
    from yolov5_obb_amd import val_sharded
    from yolov5_obb_amd.utils import metrics
    from yolov5_obb_amd.utils.general import non_max_suppression_obb
    preds = {}

    def model(im):                                   # per image: seeded by its first two pixel values (exact after / 255)
        out = []
        for b in range(im.shape[0]):
            key = int(round(float(im[b, 0, 0, 0]) * 255)) * 256 + int(round(float(im[b, 0, 0, 1]) * 255))
            if key not in preds:
                preds[key] = synth.s_pred(1, 3000, 15, seed=key % 1000, n_obj=30)
            out.append(preds[key])
        return (torch.cat(out, 0).to(dev),)
    kw = dict(conf_thres=0.25, iou_thres=0.45, half=False, device=dev)
    plain = _Set()
    dets = [non_max_suppression_obb(model(plain[i][0][None].to(dev).float() / 255)[0], 0.25, 0.45, multi_label=True)[0].cpu() for i in range(6)]
    loader = torch.utils.data.DataLoader(_Set(dets), batch_size=3, collate_fn=_Set.collate_fn)
    host = val_sharded.run(model, loader, ap_per_class=metrics.ap_per_class, names={}, **kw)
    devm = val_sharded.run(model, loader, device_metrics=True, **kw)
    assert devm["seen"] == host["seen"] == 6 and devm["stats"] is None
    got = devm["val_stats"].cpu()
    assert len(got[1]) > 20 and got[0][:, 0].sum() >= len(got[1]) // 4
    assert all(np.array_equal(g, h) for g, h in zip(got, host["stats"]))
    assert host["metrics"] is not None and identical(devm["metrics"], host["metrics"])
    assert 0.05 < devm["metrics"][5][:, 0].mean() <= 1.0
    # no label of a predicted class: nothing matches, val.py:270 skips the metrics
    none = val_sharded.run(model, torch.utils.data.DataLoader(_Set(label_cls=200.0), batch_size=3, collate_fn=_Set.collate_fn),
                           device_metrics=True, **kw)
    assert none["metrics"] is None and none["val_stats"].n > 20 and not none["val_stats"].any_tp
    with pytest.raises(RuntimeError):
        val_sharded.run(lambda im: (torch.zeros(im.shape[0], 10, 201),), loader, device_metrics=True, device="cpu", half=False)
