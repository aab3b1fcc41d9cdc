"""GPU: two training steps under ``torch.autocast("cuda", dtype=torch.bfloat16)`` -- the 16-bit training mode that needs no
``GradScaler`` -- through the HIP ``ComputeLoss``: the smallest model of tests/test_train_leg_gpu.py (three conv stems + this
package's Detect), plain SGD, no scaler.

Checked: the head outputs are bf16; the loss of the first step equals the oracle's (pyref.compute_loss on the very logits the
head produced, widened to fp32) within the tolerance of tests/test_bf16_loss_gpu.py (four unit roundoffs of bf16, 2^-7); the
gradients at the head outputs are bf16 and finite, every parameter gradient is finite; the weights move and a second step
gives another finite loss."""
import numpy as np
import torch
import pytest

from oracle import pyref
from tests import synth
from tests.test_loss_gpu import check_grads

pytestmark = pytest.mark.gpu

TOL = 2.0 ** -7


class TinyObb(torch.nn.Module):
    """Three conv stems + this package's Detect: what ComputeLoss needs from a model (.hyp, .model[-1])."""

    def __init__(self, nc, hyp):
        super().__init__()
        from yolov5_obb_amd.models.yolo import Detect
        ch = (8, 16, 32)
        self.stems = torch.nn.ModuleList([torch.nn.Conv2d(3, c, 3, stride=s, padding=1) for c, s in zip(ch, (8, 16, 32))])
        det = Detect(nc=nc, anchors=synth.DEFAULT_ANCHORS, ch=ch)
        det.stride = torch.tensor(synth.DEFAULT_STRIDES)
        det.anchors /= det.stride.view(-1, 1, 1)
        self.model = torch.nn.ModuleList([torch.nn.Identity(), det])
        self.hyp = dict(hyp)

    def forward(self, im):
        return self.model[-1]([torch.nn.functional.silu(s(im)) for s in self.stems])


def test_two_bf16_autocast_steps_without_a_gradscaler(dev, oracle_lib):
    from yolov5_obb_amd.utils.loss import ComputeLoss
    nc, imgsz, bs, nt = 16, 256, 4, 60
    hyp = synth.scaled_hyp(nc, imgsz)
    torch.manual_seed(7)
    model = TinyObb(nc, hyp).to(dev).train()
    compute_loss = ComputeLoss(model)
    spec = pyref.LossSpec(hyp, synth.grid_anchors(), torch.tensor(synth.DEFAULT_STRIDES), nc)
    _, targets = synth.s_loss(bs, nc, nt, 11, imgsz=imgsz, sizes=[32, 16, 8])
    im = torch.rand(bs, 3, imgsz, imgsz, generator=torch.Generator().manual_seed(3)).to(dev)
    opt = torch.optim.SGD(model.parameters(), lr=0.01, momentum=0.9)
    params = list(model.parameters())
    before = [p.detach().clone() for p in params]

    with torch.autocast("cuda", dtype=torch.bfloat16):
        pred = model(im)                                                  # list of (bs, na, ny, nx, no), bf16 under autocast
        for p in pred:
            assert p.dtype == torch.bfloat16
            p.retain_grad()
        loss, items = compute_loss(pred, targets.to(dev))
    loss.backward()                                                       # no GradScaler: bf16 has fp32's exponent range

    pc = [p.detach().float().cpu().requires_grad_(True) for p in pred]
    lo, io = pyref.compute_loss(spec, pc, targets.clone())
    lo.backward()
    print("loss", loss.detach().cpu().tolist(), lo.detach().tolist(), "items", items.cpu().tolist(), io.tolist())
    assert np.allclose(loss.detach().float().cpu().numpy(), lo.detach().numpy(), rtol=TOL, atol=0.0)
    assert np.allclose(items.float().cpu().numpy(), io.numpy(), rtol=TOL, atol=1e-5)
    for a in pred:
        assert a.grad is not None and a.grad.dtype == torch.bfloat16 and bool(torch.isfinite(a.grad.float()).all())
    check_grads(pred, pc, grtol=TOL, atol=1e-7)
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in params)

    opt.step()
    assert sum(float((p.detach() - b).abs().sum()) for p, b in zip(params, before)) > 0
    opt.zero_grad()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        pred2 = model(im)
        loss2, _ = compute_loss(pred2, targets.to(dev))
    loss2.backward()
    assert all(p.dtype == torch.bfloat16 for p in pred2)
    assert bool(torch.isfinite(loss2).all()) and float(loss2) != float(loss)
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in params)
    opt.step()
