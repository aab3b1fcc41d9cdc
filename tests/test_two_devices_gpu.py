"""GPU, two devices in one process: what the library remembers per device.  The dynamic-LDS limit of a kernel is an attribute of
the function ON ONE DEVICE, and the CU count sizes workspaces and grids -- so after device 0 has been used, the first calls on
device 1 must raise the limits there and size everything from that device (csrc/launch_once.h, csrc/nms_driver.h: DeviceCus).
Every call below runs on cuda:0 first and then on cuda:1, and the results must be the same bit for bit:

  * nms_rotated on 500 random boxes (the persistent kernel behind the three-launch sort: k_ps_bucket, k_nms_persist);
  * non_max_suppression_obb three times on one (2, 2048, 187) fp16 prediction, the shape's hints (include/obb_hip.h:
    obb_nms_obb_hints) set so that the first call is un-hinted (radix sort, persistent kernel), the second knows the candidate
    count but no segment size (k_sort_prep_lds, persistent kernel) and the third both (k_nms_small);
  * the lazy-head entry once on conv outputs of 8x8 and 4x4 (k_decode_head).
Skipped with fewer than two devices.  No timing is asserted."""
import pytest
import torch

from tests import synth
from tests.test_lazy_nms_gpu import _heads, _run

pytestmark = pytest.mark.gpu

CONF = 0.2503            # (a threshold no other test uses: the shape's hints start empty on both devices)
KW = dict(conf_thres=CONF, iou_thres=0.45, multi_label=True, max_det=300)


def _detect2(nc, dev, dtype):
    from yolov5_obb_amd.models.yolo import Detect
    det = Detect(nc=nc, anchors=synth.DEFAULT_ANCHORS[:2], ch=(8, 8))
    det.stride = torch.tensor(synth.DEFAULT_STRIDES[:2])
    det.anchors /= det.stride.view(-1, 1, 1)
    det = det.to(dev).to(dtype).eval()
    det.m = torch.nn.ModuleList([torch.nn.Identity() for _ in range(2)])
    return det


def _all_calls(dev, dets, scores, pred, heads):
    """-> the results of every call, on the host."""
    from yolov5_obb_amd.nms_rotated_ext import nms_rotated
    from yolov5_obb_amd.utils import general
    out = [nms_rotated(dets.to(dev), scores.to(dev), 0.4).cpu()]
    p = pred.to(dev)
    shape = (dev, pred.shape[1], 2, True, CONF)
    general.hint_set(*shape, cand=0, seg=0)                          # un-hinted: the radix sort, then the persistent kernel
    out += [r.cpu() for r in general.non_max_suppression_obb(p, **KW)]
    cand = general.hint_get(*shape)["cand"]
    assert 0 < cand <= 6144, "the second call takes the in-LDS sort"
    general.hint_set(*shape, cand=cand, seg=0)                       # hinted, largest segment unknown: k_sort_prep_lds, persistent kernel
    out += [r.cpu() for r in general.non_max_suppression_obb(p, **KW)]
    assert 0 < general.hint_get(*shape)["seg"] <= 384, "the third call takes the small-segment kernel"
    out += [r.cpu() for r in general.non_max_suppression_obb(p, **KW)]   # small-segment: k_nms_small
    det = _detect2(2, dev, torch.float16)
    z, _, lazy = _run(det, [h.to(dev) for h in heads], True, **KW)
    assert not z.is_materialized(), "the fused entry on the conv outputs did not run"
    out += [r.cpu() for r in lazy]
    torch.cuda.synchronize(dev)
    return out


def test_second_device_matches_first():
    if not torch.cuda.is_available() or torch.cuda.device_count() < 2:
        pytest.skip("needs two visible devices")
    dets, scores = synth.s_uniform(500, seed=11)
    scores = synth.tie_free(scores)
    pred = synth.s_pred(2, 2048, 2, seed=12, dtype=torch.float16)
    heads = _heads(2, 2, [(8, 8), (4, 4)], 13, "cpu", torch.float16)
    first = _all_calls(torch.device("cuda:0"), dets, scores, pred, heads)
    second = _all_calls(torch.device("cuda:1"), dets, scores, pred, heads)
    assert len(first) == len(second) == 1 + 3 * 2 + 2
    assert any(r.shape[0] > 0 for r in first[1:]), "the inputs produce detections"
    for i, (a, b) in enumerate(zip(first, second)):
        assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b), (i, a.shape, b.shape)
