"""Generate tests/golden/loss_configs.npz from the REFERENCE's own utils/loss.py (run in the build container only).

    YOLOV5_CONFIG_DIR=/tmp/refcfg python tests/golden/gen_loss_configs.py

The head configurations of tests/loss_cases.py:FIXTURE (nl = 4 / na = 4 on non-square grids, nc = 1 with class-3 targets,
nc = 256, na = 1, the planted-edge targets, ...) through the reference's ComputeLoss, imported with the stubs and the clamp_
patch of gen_golden.py.  Inputs are regenerated from seeds by tests/loss_cases.py; stored per case: the loss and its items,
per level the build_targets indices (b, a, gj, gi) and tbox, and per level and channel group (box, obj, cls, csl) the sum of
the gradient and the sum of its magnitudes.  While generating, the oracle (oracle/pyref.py) is checked against every output.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden                  # noqa: E402  (puts the repository root on sys.path)
from oracle import pyref           # noqa: E402
from tests import loss_cases as LC  # noqa: E402


def main():
    import oracle
    oracle.build(with_ref=True)
    _, _, _, L, _, Y = gen_golden.load_reference()
    torch.set_num_threads(1)
    orig = gen_golden.patch_clamp_()

    class _M(torch.nn.Module):                                       # what ComputeLoss.__init__ reads (utils/loss.py:93-120)
        def __init__(self, case, hyp):
            super().__init__()
            _, apx, st = LC.head(case)
            d = Y.Detect(nc=case.nc, anchors=apx.reshape(case.nl, -1).tolist(), ch=(4,) * case.nl)
            d.stride = st.clone()
            d.anchors /= d.stride.view(-1, 1, 1)
            self.model = torch.nn.ModuleList([d])
            self.hyp = hyp

    out = {}
    for name in LC.FIXTURE:
        case, p, t = LC.fixture_inputs(name)
        hyp = LC.hyp_of(case)
        model = _M(case, hyp)
        cl = L.ComputeLoss(model)
        if LC.balance_of(case):
            cl.balance = list(LC.balance_of(case))
        pr = [q.clone().requires_grad_(True) for q in p]
        loss, items = cl(pr, t.clone())
        loss.backward()
        spec = LC.spec_of(case)
        assert torch.equal(spec.anchors, model.model[0].anchors) and torch.equal(spec.stride, model.model[0].stride), name
        pm = [q.clone().requires_grad_(True) for q in p]
        loss2, items2 = pyref.compute_loss(spec, pm, t.clone())
        loss2.backward()
        assert torch.allclose(loss, loss2, rtol=1e-6, atol=1e-7), (name, loss, loss2)
        assert torch.allclose(items, items2, rtol=1e-6, atol=1e-7), (name, items, items2)
        for q1, q2 in zip(pr, pm):
            assert torch.allclose(q1.grad, q2.grad, rtol=1e-5, atol=1e-8), name
        tg = cl.build_targets(pr, t.clone())
        tg2 = pyref.build_targets(spec, pm, t.clone())
        for i in range(case.nl):
            b, a_, gj, gi = tg[2][i]
            r = tg2[i]
            assert torch.equal(b, r['b']) and torch.equal(a_, r['a']) and torch.equal(gj, r['gj']) and torch.equal(gi, r['gi'])
            assert torch.equal(tg[1][i], r['tbox']) and torch.equal(tg[0][i], r['tcls']) and torch.equal(tg[4][i], r['csl'])
            assert torch.equal(tg[3][i], r['anch'])
            out[f'{name}_idx{i}'] = torch.stack((b, a_, gj, gi), 1).numpy()
            out[f'{name}_tbox{i}'] = tg[1][i].numpy()
            out[f'{name}_gradsum{i}'] = LC.group_sums(pr[i].grad, case.nc)
        out[f'{name}_loss'] = loss.detach().numpy()
        out[f'{name}_items'] = items.numpy()
        print(f"{name}: loss {loss.item():.6f} items {items.tolist()} n_pos {[len(tg[2][i][0]) for i in range(case.nl)]}")
    torch.Tensor.clamp_ = orig
    path = os.path.join(HERE, 'loss_configs.npz')
    np.savez_compressed(path, **out)
    print(f"wrote tests/golden/loss_configs.npz ({os.path.getsize(path) / 1024:.0f} KiB, {len(out)} arrays)")


if __name__ == '__main__':
    main()
