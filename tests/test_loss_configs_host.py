"""CPU checks behind tests/test_loss_configs_gpu.py: the synthetic inputs are stable, the oracle matches the reference's own
utils/loss.py on the new head configurations (tests/golden/loss_configs.npz, written by tests/golden/gen_loss_configs.py),
and the loss entries reject what the C ABI does not accept before any device call."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest
import torch

from oracle import pyref
from tests import loss_cases as LC
from tests import synth


def _digest(p, t):
    m = hashlib.sha256()
    for x in list(p) + [t]:
        m.update(repr((tuple(x.shape), str(x.dtype))).encode())
        m.update(x.contiguous().numpy().tobytes())
    return m.hexdigest()


# digests of synth.s_loss's default-argument outputs, taken before it learned na / (ny, nx) / anchors: the golden loss cases
# (tests/golden/gen_golden.py, section F) regenerate their inputs from these seeds
S_LOSS_DIGESTS = [
    (dict(bs=2, nc=16, nt=50, seed=31, imgsz=256, sizes=[32, 16, 8]), "b53a1a2f453b80e59b8e764d1a53afb03be92d0543b5442649ab6859d16f1159"),
    (dict(bs=4, nc=15, nt=400, seed=33, imgsz=256, sizes=[32, 16, 8]), "82af965641c965b1ff6da4569a2b0dc67de1abecf77f837a7392d736f42f26a7"),
    (dict(bs=2, nc=16, nt=0, seed=32, imgsz=128, sizes=[16, 8, 4]), "7ddc6aa1e55fe705f102f860ff71de69823fce215c69728f9ec6524e432a13f1"),
]


@pytest.mark.parametrize("k", range(len(S_LOSS_DIGESTS)))
def test_s_loss_defaults_are_byte_identical(k):
    cfg, want = S_LOSS_DIGESTS[k]
    cfg = dict(cfg)
    p, t = synth.s_loss(cfg.pop("bs"), cfg.pop("nc"), cfg.pop("nt"), cfg.pop("seed"), **cfg)
    assert _digest(p, t) == want


def test_head_anchors_reuse_the_model_tables():
    a, s = synth.head_anchors(3, 3)
    assert torch.equal(a, torch.tensor(synth.DEFAULT_ANCHORS).float().view(3, 3, 2)) and s.tolist() == synth.DEFAULT_STRIDES
    a, s = synth.head_anchors(4, 3)
    assert torch.equal(a, torch.tensor(synth.P6_ANCHORS).float().view(4, 3, 2)) and s.tolist() == synth.P6_STRIDES
    for nl in (1, 2, 3, 4, 5, 8):
        for na in (1, 2, 3, 4, 8):
            a, s = synth.head_anchors(nl, na)
            assert a.shape == (nl, na, 2) and torch.equal(a, synth.head_anchors(nl, na)[0])
            assert bool((a[..., 0] != a[..., 1]).all())


FIX = None


def fixture():
    global FIX
    if FIX is None:
        FIX = np.load(os.path.join(os.path.dirname(__file__), "golden", "loss_configs.npz"))
    return FIX


@pytest.mark.parametrize("name", list(LC.FIXTURE))
def test_oracle_matches_reference_fixture(name):
    """pyref.build_targets / compute_loss against the reference's ComputeLoss on the same inputs (frozen)."""
    g = fixture()
    case, p, t = LC.fixture_inputs(name)
    spec = LC.spec_of(case)
    pc = [x.clone().requires_grad_(True) for x in p]
    lo, io = pyref.compute_loss(spec, pc, t.clone())
    lo.backward()
    assert np.allclose(lo.detach().numpy(), g[f"{name}_loss"], rtol=1e-6, atol=1e-7)
    assert np.allclose(io.numpy(), g[f"{name}_items"], rtol=1e-6, atol=1e-7)
    if name == "nc1_class3":
        assert np.isfinite(g[f"{name}_loss"]).all() and (t[:, 1] == 3).any()
    bt = pyref.build_targets(spec, p, t)
    for i in range(case.nl):
        r = bt[i]
        assert np.array_equal(torch.stack((r['b'], r['a'], r['gj'], r['gi']), 1).numpy(), g[f"{name}_idx{i}"]), i
        assert np.array_equal(r['tbox'].numpy(), g[f"{name}_tbox{i}"]), i
        ref = g[f"{name}_gradsum{i}"]
        gs = LC.group_sums(pc[i].grad, case.nc)
        assert np.all(np.abs(gs - ref) <= 1e-5 * np.abs(ref[:, 1:2]) + 1e-12), (i, gs, ref)


def _cfg(nl=3, na=3, nc=16, no=None, bs=2, grid=8):
    from yolov5_obb_amd.utils.loss import _LossConfig
    c = _LossConfig()
    c.nl, c.na, c.nc, c.bs = nl, na, nc, bs
    c.no = 5 + nc + 180 if no is None else no
    for i in range(min(nl, 8)):
        c.ny[i], c.nx[i] = grid, grid
        c.stride[i], c.balance[i] = 8.0 * 2 ** i, 1.0
        for a in range(min(na, 8)):
            c.anchors[i][a][0], c.anchors[i][a][1] = 1.0 + a, 2.0 + a
    c.anchor_t = 4.0
    return c


def test_workspace_rejects_unsupported_configs():
    """obb_loss_workspace_bytes answers 0 for what include/obb_hip.h does not accept, with no device call (no GPU here)."""
    from yolov5_obb_amd import _lib
    L = _lib.lib()
    ws = lambda c, nt=10: L.obb_loss_workspace_bytes(C.byref(c), nt)
    for nl, na, nc in ((1, 1, 1), (8, 8, 256), (3, 3, 16)):
        assert ws(_cfg(nl=nl, na=na, nc=nc)) > 0, (nl, na, nc)
    assert ws(_cfg(nl=9)) == 0
    assert ws(_cfg(na=9)) == 0
    assert ws(_cfg(nl=0)) == 0 and ws(_cfg(na=0)) == 0
    assert ws(_cfg(nc=0)) == 0
    assert ws(_cfg(nc=257)) == 0
    assert ws(_cfg(nc=16, no=5 + 16 + 179)) == 0 and ws(_cfg(nc=16, no=5 + 17 + 180)) == 0
    assert ws(_cfg(bs=0)) == 0 and ws(_cfg(grid=0)) == 0
    assert ws(_cfg(), nt=-1) == 0
    # the same answer from the entries themselves: OBB_ERR_BAD_ARG (-1) before anything is launched
    null = C.c_void_p(0)
    assert L.obb_loss_forward(C.byref(_cfg(nc=257)), null, 0, null, 0, 7, null, null, 0, null) == -1
    assert L.obb_loss_backward(C.byref(_cfg(na=9)), null, 0, null, 0, 7, null, null, null, 0, null) == -1
    assert L.obb_loss_build_targets(C.byref(_cfg(nl=9)), null, 0, 7, null, null, 0, null) == -1
