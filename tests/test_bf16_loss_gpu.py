"""GPU: ComputeLoss on bfloat16 head outputs (obb_loss_forward / obb_loss_backward with OBB_DTYPE_BF16) against the CPU oracle
(oracle/pyref.py), tests/test_loss_gpu.py::run_both-style: the oracle sees the bf16-rounded logits in fp32.

Tolerance.  The kernels compute in fp32 on the bf16 logits; what differs from the oracle is that tobj is rounded to the head
dtype (utils/loss.py:155) and that the gradients are stored in that dtype.  tests/test_loss_gpu.py::test_fp16_heads allows
2e-3 = four unit roundoffs of fp16 (4 * 2^-11); the same four unit roundoffs of bf16 are 4 * 2^-9 = 2^-7: relative on the loss
scalars, and per channel group through check_grads (grtol, with the fp16 test's atol).  Where the oracle's gradient is exactly
zero ours is too (check_grads asserts it), and build_targets does not depend on the dtype: bit-exact."""
import numpy as np
import pytest
import torch

from oracle import pyref
from tests import loss_cases as LC
from tests import synth
from tests.test_loss_gpu import check_grads, make

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
TOL = 2.0 ** -7            # 4 unit roundoffs of bf16 (module docstring)


def _poison(like):
    """Fill, then free, blocks of the gradients' sizes: the backward's torch.empty_like gets them back from the cache, so an
    element the kernels skip is a NaN."""
    junk = [torch.full_like(x, float("nan")) for x in like]
    del junk


def _run(cl, spec, p, t, dev, tg=None, **okw):
    pc = [x.clone().to(BF16).float().requires_grad_(True) for x in p]         # the oracle sees the bf16-rounded logits
    lo, io = pyref.compute_loss(spec, pc, t.clone(), **okw)
    lo.backward()
    pg = [x.clone().to(device=dev, dtype=BF16).requires_grad_(True) for x in p]
    lg, ig = cl(pg, (t if tg is None else tg).to(dev))
    _poison(pg)
    lg.backward()
    assert lg.shape == (1,) and ig.shape == (4,)
    print("loss", lg.detach().cpu().tolist(), lo.detach().tolist(), "items", ig.cpu().tolist(), io.tolist())
    assert np.allclose(lg.detach().float().cpu().numpy(), lo.detach().numpy(), rtol=TOL, atol=0.0), (lg, lo)
    assert np.allclose(ig.float().cpu().numpy(), io.numpy(), rtol=TOL, atol=1e-5), (ig, io)
    for a in pg:
        assert a.grad.dtype == BF16 and a.grad.shape == a.shape and bool(torch.isfinite(a.grad.float()).all())
    check_grads(pg, pc, grtol=TOL, atol=1e-7)
    return lg


def _targets_bit_exact(cl, spec, p, t, dev):
    ref = pyref.build_targets(spec, p, t)
    tcls, tbox, indices, anch, tcsl = cl.build_targets([x.to(device=dev, dtype=BF16) for x in p], t.to(dev))
    for i, r in enumerate(ref):
        assert np.array_equal(torch.stack(indices[i], 1).cpu().numpy(), torch.stack((r['b'], r['a'], r['gj'], r['gi']), 1).numpy()), i
        assert np.array_equal(tbox[i].cpu().numpy(), r['tbox'].numpy()), i
        assert np.array_equal(anch[i].cpu().numpy(), r['anch'].numpy()), i
        assert np.array_equal(tcls[i].cpu().numpy(), r['tcls'].numpy()), i
        assert np.array_equal(tcsl[i].cpu().numpy(), r['csl'].numpy()), i


def test_bf16_heads(dev):
    """The inputs of test_fp16_heads."""
    cl, spec, p, t = make(dev, nt=100, seed=21)
    _run(cl, spec, p, t, dev)
    _targets_bit_exact(cl, spec, p, t, dev)


def test_bf16_vector_tail_of_the_gradient_store(dev):
    """The shapes of tests/loss_cases.py `nl2_na2_nc2_f16` (maps 13 x 20 and 7 x 10, nc 2, bs 3): the last 64-row region of a
    level ends in a partial 16-byte vector, so k_loss_bwd_dense's element-wise tail stores bf16 values too."""
    from yolov5_obb_amd.utils.loss import ComputeLoss
    case = LC.BY_NAME["nl2_na2_nc2_f16"]
    assert any((case.rows(i) % 64 or 64) * case.no % 8 for i in range(case.nl))
    ag, _, st = LC.head(case)
    cl = ComputeLoss(synth.FakeModel(case.nc, LC.hyp_of(case), dev, anchors=ag, strides=st))
    spec = LC.spec_of(case)
    p, t = LC.random_inputs(case)
    _run(cl, spec, p, t, dev)
    _targets_bit_exact(cl, spec, p, t, dev)


def test_bf16_focal_loss(dev):
    cl, spec, p, t = make(dev, nt=120, seed=51, hyp_over=dict(fl_gamma=1.5, cls_pw=1.3, obj_pw=0.8))
    assert cl.fl_gamma == 1.5
    _run(cl, spec, p, t, dev)


def test_bf16_sort_obj_iou(dev):
    cl, spec, p, t = make(dev, nt=120, seed=14)
    t = t.clone()
    t[:30, 0] = 1
    t[:30, 2:4] = torch.tensor([40.2, 200.1])                        # a crowded cell: the winner sets the objectness target
    cl.sort_obj_iou = True
    _run(cl, spec, p, t, dev, sort_obj_iou=True)


def test_bf16_no_targets(dev):
    cl, spec, p, t = make(dev, nt=0, seed=31)
    _run(cl, spec, p, t, dev)
