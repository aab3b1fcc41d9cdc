"""GPU: the post-NMS tail of val.py (val.val_tail_batch -> k_vt_dets + k_vt_stats of csrc/head.hip, and val.process_batch) at the
density of the reference workload -- up to max_det = 1000 detections per image against hundreds to thousands of labels --
against the RESTATED REFERENCE (oracle/pyref.py), not against the project's own per-image kernels.  The cases of
tests/valtail_cases.py reach what the small inputs of test_valpost_gpu.py never do:
  * more than kVtLabLds = 512 labels in a workgroup's image range (labels recomputed where they are met), on either side of
    the switch and with two images under 512 each that share a workgroup;
  * the prefix scan of k_vt_stats over more than 64 earlier detections, and waves that straddle two images;
  * exact IoU ties (duplicate labels), where the result is the pinned rule of pyref.process_batch(ties="first").

How `correct` is compared.  The matching is exact comparisons only once the boxes are fixed, but cosf / sinf differ in the last
ulp between the device's libm and the host's, and one ulp in a box flips `iou >= iouv[k]` on a few rows out of thousands.  So the
oracle's process_batch runs on the HOST with the box bits the DEVICE produced (pred_hbbn from want_boxes=True; the label
boxes from val_postprocess on the label rows + pad / gain / clip in float32), and the assertion is torch.equal on every row.
Those device boxes are themselves held to the reference chain (pyref.val_postprocess, pyref.val_label_boxes; rtol=1e-6,
atol=2e-4, the tolerance of test_valpost_gpu.py) in the same tests.  With theta = 0 nothing depends on libm: that case runs the
whole chain on the host and asks for equal bits.

Coverage measured with these generators (the same figures from the host chain and from the device's boxes): correct rows
lds_511/512/513 111/116/113, two_images_one_block 107; dense: 201 detections on one label, 152 tied detections; straddle: 202
detections on one label; ties: 976 tied detections, 158 correct rows."""
import pytest
import torch

from oracle import pyref
from tests import valtail_cases as VC

pytestmark = pytest.mark.gpu

TOL = dict(rtol=1e-6, atol=2e-4)


@pytest.fixture
def ctypes_binding(monkeypatch):
    """Force the fallback binding for the duration of a test (the tests switch back and forth; monkeypatch restores)."""
    from yolov5_obb_amd import _lib
    _lib.compiled()
    monkeypatch.setattr(_lib, "_ext", None)
    monkeypatch.setattr(_lib, "_ext_tried", True)
    return _lib


def _use(lib, binding):
    if binding == "compiled":
        lib._ext_tried = False
        assert lib.compiled() is not None, "nms_rotated_ext_c.so is not built"
    else:
        lib._ext, lib._ext_tried = None, True


def _same(a, b):
    (sa, (ba, oa)), (sb, (bb, ob)) = a, b
    assert list(oa) == list(ob) and len(sa) == len(sb)
    for x, y in zip(sa, sb):
        assert x[0].dtype == torch.bool and all(torch.equal(p, q) for p, q in zip(x, y))
    for p, q in zip(ba, bb):
        assert torch.equal(p, q)


def _tail(lib, dev, preds, targets, shapes):
    """val_tail_batch through both bindings (identical output required); the compiled binding's result, boxes on the host."""
    from yolov5_obb_amd.val import val_tail_batch
    packed = torch.cat(preds, 0).to(dev)
    views = list(packed.split([p.shape[0] for p in preds]))     # consecutive views of one buffer
    tg, iouv = targets.to(dev), VC.IOUV.to(dev)
    out = {}
    for binding in ("compiled", "ctypes"):
        _use(lib, binding)
        out[binding] = val_tail_batch(views, tg, shapes, iouv, want_boxes=True)
    _same(out["compiled"], out["ctypes"])
    stats, (boxes, offs) = out["compiled"]
    return stats, [x.cpu() for x in boxes], list(offs)


def _device_label_boxes(dev, lab, shape_hw, gain, pad):
    """labels_hbbn (m, 5) with the device's bits: the hull from k_val_post (the same vt_rbox2poly / vt_hbb_xyxy the tail uses),
    then scale_coords in float32 on the host (IEEE subtract / divide / clamp, as vt_label_box)."""
    from yolov5_obb_amd.val import val_postprocess
    if lab.shape[0] == 0:
        return torch.zeros(0, 5)
    lab7 = torch.cat((lab[:, 2:7], torch.zeros_like(lab[:, :1]), lab[:, 1:2]), 1).to(dev)
    tb = val_postprocess(lab7, ratio_pad=((1.0, 1.0), (0.0, 0.0)))[1][:, :4].cpu()
    f = lambda v: torch.tensor(v, dtype=torch.float32)
    tb[:, [0, 2]] -= f(pad[0]); tb[:, [1, 3]] -= f(pad[1])
    tb /= f(gain)
    tb[:, [0, 2]] = tb[:, [0, 2]].clamp(0, float(shape_hw[1])); tb[:, [1, 3]] = tb[:, [1, 3]].clamp(0, float(shape_hw[0]))
    return torch.cat((lab[:, 1:2], tb), 1)


def _check(dev, stats, boxes, offs, preds, targets, shapes):
    """Every image against the oracle; returns (correct rows, most detections on one label, tied detections)."""
    rows = chosen = tied = 0
    assert len(stats) == len(preds) and offs[-1] == sum(p.shape[0] for p in preds)
    for b, p in enumerate(preds):
        (h, w), ((gain, _), pad) = shapes[b]
        sl = slice(offs[b], offs[b + 1])
        correct, conf, cls = stats[b]
        assert correct.shape == (p.shape[0], 10) and correct.dtype == torch.bool
        assert torch.equal(conf, p[:, 5]) and torch.equal(cls, p[:, 6])                   # copied through: the same bits
        lab = VC.labels_of(targets, b)
        for got, want in zip(boxes, pyref.val_postprocess(p.clone(), gain, pad)):        # the device's boxes against the reference chain
            assert got[sl].shape == want.shape and torch.allclose(got[sl], want, **TOL), (b, (got[sl] - want).abs().max())
        lab_dev = _device_label_boxes(dev, lab, (h, w), gain, pad)
        lab_ref = pyref.val_label_boxes(lab, gain, pad, (h, w))
        assert torch.allclose(lab_dev, lab_ref, **TOL), (b, (lab_dev - lab_ref).abs().max())
        want = VC.oracle_correct(boxes[3][sl], lab_dev)                                  # exact: identical box bits on both sides
        assert torch.equal(correct, want), (b, int((correct != want).any(1).sum()), "rows differ")
        rows += int(correct.any(1).sum())
        c, t = VC.coverage(boxes[3][sl], lab_dev)
        chosen, tied = max(chosen, c), tied + t
    return rows, chosen, tied


def _case(name):
    seed, images = VC.CASES[name]
    return VC.make_batch(seed, images)


@pytest.mark.parametrize("name", ["lds_511", "lds_512", "lds_513"])
def test_label_staging_on_either_side_of_the_lds_limit(dev, ctypes_binding, name):
    preds, targets, shapes = _case(name)
    rows, _, _ = _check(dev, *_tail(ctypes_binding, dev, preds, targets, shapes), preds, targets, shapes)
    print(name, "correct rows", rows)
    assert rows >= 40


def test_two_images_under_the_limit_in_one_workgroup_take_the_fallback(dev, ctypes_binding):
    preds, targets, shapes = _case("two_images_one_block")
    assert sum(p.shape[0] for p in preds) == 128 and all(0 < (targets[:, 0] == b).sum() < 512 for b in (0, 1)) and len(targets) > 512
    rows, _, _ = _check(dev, *_tail(ctypes_binding, dev, preds, targets, shapes), preds, targets, shapes)
    print("correct rows", rows)
    assert rows >= 50


def test_dense_batch_and_the_rows_layout_of_the_nms(dev, ctypes_binding):
    from yolov5_obb_amd.val import val_tail_batch
    preds, targets, shapes = _case("dense")
    got = _tail(ctypes_binding, dev, preds, targets, shapes)
    rows, chosen, tied = _check(dev, *got, preds, targets, shapes)
    print("correct rows", rows, "most detections on one label", chosen, "tied detections", tied)
    assert chosen >= 130, "some label must be the best label of >= 130 detections: three or more 64-entry scan trips"
    assert tied >= 100
    # the layout non_max_suppression_obb returns: views of a (bs * max_det, 7) buffer, image b at row b * max_det, gaps between
    # them (obb_val_tail_batch_rows_f32's det_row); the gaps hold rows that must never be read
    max_det = 1000
    buf = torch.full((len(preds) * max_det, 7), float("nan"))
    for b, p in enumerate(preds):
        buf[b * max_det:b * max_det + p.shape[0]] = p
    buf = buf.to(dev)
    views = [buf[b * max_det:b * max_det + p.shape[0]] for b, p in enumerate(preds)]
    loose = [p.to(dev).clone() for p in preds]                   # separately allocated tensors: concatenated by the binding
    tg, iouv = targets.to(dev), VC.IOUV.to(dev)
    for binding in ("compiled", "ctypes"):
        _use(ctypes_binding, binding)
        for dets in (views, loose):
            st, (bx, offs) = val_tail_batch(dets, tg, shapes, iouv, want_boxes=True)
            _same((st, (bx, offs)), (got[0], (tuple(x.to(dev) for x in got[1]), got[2])))


def test_image_boundaries_inside_waves_and_workgroups(dev, ctypes_binding):
    preds, targets, shapes = _case("straddle")
    assert [p.shape[0] for p in preds] == [100, 200, 1, 0, 127, 128, 129, 257]
    rows, chosen, _ = _check(dev, *_tail(ctypes_binding, dev, preds, targets, shapes), preds, targets, shapes)
    print("correct rows", rows, "most detections on one label", chosen)
    assert chosen >= 65, "a scan of more than one trip must start inside a wave that straddles two images"


def test_exact_ties_lds_path_fallback_path_and_per_image_kernel_agree_with_the_pinned_oracle(dev, ctypes_binding):
    """Integer boxes, theta = 0, gain 1, pad 0: every IoU is a ratio of small integers, 50 labels are exact copies of others.
    The staged label list of k_vt_dets is filled in arrival order; only the `l < bl` clause makes its choice the first maximum."""
    from yolov5_obb_amd.val import process_batch
    preds, targets, shapes = VC.make_batch(50, [(2000, 200, 1, 0, 50)], axis=True, integer=True, unit_frame=True)
    # Exact copies alone cannot tell the first maximum from the last one (every detection sees both copies alike, and the
    # lowest detection wins either way).  Planted beside the random boxes, 8 times: labels A = [x, x+10] and B = [x+2, x+12]
    # (10 high), detection d0 = A's box, then detection d = [x+1, x+11]: IoU(d, A) = IoU(d, B) = 90 / 110 exactly.  First
    # maximum: d keeps A, which d0 has taken -> d is NOT correct.  Last maximum or arrival order: d keeps B and wins it.
    k = 8
    x0 = 1005.0 + 30.0 * torch.arange(k)
    lab = torch.zeros(2 * k, 9)
    lab[0::2, 2] = x0; lab[1::2, 2] = x0 + 2; lab[:, 3] = 1005.0; lab[:, 4:6] = 10.0
    det = torch.zeros(2 * k, 7)
    det[0::2, 0] = x0; det[1::2, 0] = x0 + 1; det[:, 1] = 1005.0; det[:, 2:4] = 10.0
    det[:, 5] = float(preds[0][:, 5].min()) * torch.linspace(0.9, 0.1, 2 * k)
    preds, targets = [torch.cat((preds[0], det), 0)], torch.cat((targets, lab), 0)
    lds = _tail(ctypes_binding, dev, preds, targets, shapes)
    assert lds[0][0][0][-2 * k:].any(1).tolist() == [True, False] * k
    rows, _, tied = _check(dev, *lds, preds, targets, shapes)
    print("correct rows", rows, "tied detections", tied)
    assert tied >= 500 and rows >= 100
    want = lds[0][0][0]
    for _ in range(5):                                           # (arrival order may change from run to run; the result may not)
        again = _tail(ctypes_binding, dev, preds, targets, shapes)
        assert torch.equal(again[0][0][0], want)
    # 400 labels more of a class no detection has: 600 in range -> every label recomputed where it is met
    pad = VC.make_image(torch.Generator().manual_seed(51), 0, 0, 400, axis=True, integer=True)[1]
    pad[:, 1] = 1.0
    more = torch.cat((targets, pad), 0)
    fb = _tail(ctypes_binding, dev, preds, more, shapes)
    _check(dev, *fb, preds, more, shapes)
    assert torch.equal(fb[0][0][0], want)
    # the per-image kernel on the same boxes
    (h, w), ((gain, _), p) = shapes[0]
    lab_dev = _device_label_boxes(dev, targets, (h, w), gain, p)
    one = process_batch(lds[1][3].to(dev), lab_dev.to(dev), VC.IOUV.to(dev)).cpu()
    assert torch.equal(one, want)
    assert torch.equal(want, pyref.process_batch(lds[1][3], lab_dev, VC.IOUV, ties="first"))


def test_axis_aligned_end_to_end_bit_equal_to_the_host_chain(dev, ctypes_binding):
    """theta = 0: cos = 1 and sin = 0 in every libm and every product of the chain is exact, so the WHOLE tail is computed on the
    host in float32 (pyref.val_postprocess, val_label_boxes, process_batch) with no bits from the device: equal boxes, equal
    `correct`.  The last image holds detections built on the thresholds: IoU exactly 0.5 (>= must count it), 1.0, 0.75, 0.4."""
    seed, images = 60, [(300, 200, 2, 0, 20), (200, 520, 2, 2, 0), (40, 0, 2, 0, 0)]
    preds, targets, shapes = VC.make_batch(seed, images, axis=True)
    b = len(preds)
    lab = torch.zeros(4, 9)
    lab[:, 0] = b
    lab[:, 2] = torch.tensor([100.0, 200.0, 300.0, 400.0]); lab[:, 3] = 100.0; lab[:, 4:6] = 10.0       # four 10 x 10 labels
    det = torch.zeros(4, 7)
    det[:, 0] = lab[:, 2]
    det[:, 1] = torch.tensor([100.0, 97.5, 98.75, 97.0])         # the same box; 10 x 5, 10 x 7.5 and 10 x 4 boxes inside their labels
    det[:, 2] = 10.0
    det[:, 3] = torch.tensor([10.0, 5.0, 7.5, 4.0])
    det[:, 5] = torch.tensor([0.9, 0.8, 0.7, 0.6])
    preds.append(det); targets = torch.cat((targets, lab), 0); shapes.append(((600, 800), ((1.0, 1.0), (0.0, 0.0))))
    stats, boxes, offs = _tail(ctypes_binding, dev, preds, targets, shapes)
    chain = VC.oracle_chain(preds, targets, shapes)
    rows = 0
    for i, (ref_boxes, _, want) in enumerate(chain):
        sl = slice(offs[i], offs[i + 1])
        for got, ref in zip(boxes, ref_boxes):
            assert torch.equal(got[sl], ref), i
        assert torch.equal(stats[i][0], want), i
        assert torch.equal(stats[i][1], preds[i][:, 5]) and torch.equal(stats[i][2], preds[i][:, 6])
        rows += int(want.any(1).sum())
    assert rows >= 150                                           # (189 on the host chain)
    iouv = VC.IOUV
    c = stats[b][0]
    assert c[0].all()                                            # IoU 1.0
    assert c[1].tolist() == [True] + [False] * 9                 # IoU exactly 0.5 = iouv[0]
    assert torch.equal(c[2], torch.tensor(0.75) >= iouv) and int(c[2].sum()) >= 5
    assert not c[3].any()                                        # IoU 0.4


@pytest.mark.parametrize("n,m,n_cls,dup", [(3000, 1500, 3, 0), (3000, 513, 1, 100)])
def test_process_batch_at_density_against_the_pinned_oracle(dev, n, m, n_cls, dup):
    from yolov5_obb_amd.val import process_batch
    g = torch.Generator().manual_seed(70 + dup)
    d, t = VC.make_image(g, 0, n, m, n_cls, 0, dup)
    gain, pad, hw = 0.8125, (6.0, 9.5), (1180, 1150)
    det = pyref.val_postprocess(d, gain, pad)[3]                 # (inputs of this kernel: any boxes do)
    labels = pyref.val_label_boxes(t, gain, pad, hw)
    _, tied = VC.coverage(det, labels)
    want = pyref.process_batch(det, labels, VC.IOUV, ties="first")
    print("correct rows", int(want.any(1).sum()), "tied detections", tied)
    assert (tied >= 500) if dup else (tied == 0)
    assert int(want.any(1).sum()) >= 300
    if not dup:                                                  # tie-free: the reference as written gives the same rows
        assert torch.equal(want, pyref.process_batch(det, labels, VC.IOUV))
    got = process_batch(det.to(dev), labels.to(dev), VC.IOUV.to(dev))
    assert got.dtype == torch.bool and torch.equal(got.cpu(), want)
