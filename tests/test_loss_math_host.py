"""CPU: the PRODUCT's loss math header (yolov5_obb_amd/csrc/loss_math.h) compiled with g++ and compared with torch
autograd of the pinned oracle (oracle/pyref.py: bbox_ciou, BCEWithLogits) -- forward values and hand-written
gradients, tolerance 1e-5 (BASELINE.json north_star: "within 1e-5 on IoU/loss scalars")."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from oracle import pyref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hl(tmp_path_factory):
    out = tmp_path_factory.mktemp("hl") / "libhostloss.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", f"-I{ROOT}/yolov5_obb_amd/csrc",
                    f"{ROOT}/tests/native/host_loss_math.cpp", "-o", str(out), "-lm"], check=True)
    L = C.CDLL(str(out))
    fp = np.ctypeslib.ndpointer(dtype=np.float32, flags="C_CONTIGUOUS")
    L.hc_ciou.argtypes = [fp, C.c_long, fp]
    L.hc_bce.argtypes = [fp, C.c_long, C.c_float, fp]
    L.hc_focal.argtypes = [fp, C.c_long, C.c_float, C.c_float, fp]
    L.hc_pred.argtypes = [fp, C.c_long, fp]
    L.hc_rem1.argtypes = [fp, C.c_long, fp]
    return L


def test_ciou_forward_and_gradient(hl):
    g = torch.Generator().manual_seed(5)
    n = 20000
    p = torch.cat((torch.rand(n, 2, generator=g) * 1.5 - 0.25, torch.rand(n, 2, generator=g) * 12 + 0.05), 1)
    t = torch.cat((torch.rand(n, 2, generator=g), torch.rand(n, 2, generator=g) * 12 + 0.2), 1)
    p[: n // 4, 2:] = t[: n // 4, 2:] * (1 + 0.05 * torch.randn(n // 4, 2, generator=g))      # near matches
    p = p.clone().requires_grad_(True)
    ciou = pyref.bbox_ciou(p.T, t)
    ciou.sum().backward()
    out = np.zeros((n, 5), np.float32)
    hl.hc_ciou(np.ascontiguousarray(torch.cat((p.detach(), t), 1).numpy()), n, out)
    assert np.allclose(out[:, 0], ciou.detach().numpy(), rtol=1e-5, atol=1e-6)
    gref = p.grad.numpy()
    assert np.allclose(out[:, 1:], gref, rtol=1e-4, atol=2e-6), np.abs(out[:, 1:] - gref).max()


@pytest.mark.parametrize("pw", [1.0, 2.5])
def test_bce_with_logits_forward_and_gradient(hl, pw):
    g = torch.Generator().manual_seed(6)
    n = 20000
    x = (torch.randn(n, generator=g) * 6).requires_grad_(True)
    t = torch.rand(n, generator=g)
    t[: n // 3] = (t[: n // 3] > 0.5).float()
    loss = torch.nn.functional.binary_cross_entropy_with_logits(x, t, pos_weight=torch.tensor([pw]), reduction='none')
    loss.sum().backward()
    out = np.zeros((n, 2), np.float32)
    hl.hc_bce(np.ascontiguousarray(torch.stack((x.detach(), t), 1).numpy()), n, pw, out)
    assert np.allclose(out[:, 0], loss.detach().numpy(), rtol=1e-5, atol=1e-6)
    assert np.allclose(out[:, 1], x.grad.numpy(), rtol=1e-5, atol=1e-6)


def test_pred_box_decode_and_remainder(hl):
    g = torch.Generator().manual_seed(7)
    n = 5000
    lg = (torch.randn(n, 4, generator=g) * 3).requires_grad_(True)
    an = torch.rand(n, 2, generator=g) * 10 + 0.5
    pxy = lg[:, :2].sigmoid() * 2 - 0.5
    pwh = (lg[:, 2:].sigmoid() * 2) ** 2 * an
    torch.cat((pxy, pwh), 1).sum().backward()
    out = np.zeros((n, 8), np.float32)
    hl.hc_pred(np.ascontiguousarray(torch.cat((lg.detach(), an), 1).numpy()), n, out)
    assert np.allclose(out[:, :4], torch.cat((pxy, pwh), 1).detach().numpy(), rtol=1e-5, atol=1e-6)
    assert np.allclose(out[:, 4:], lg.grad.numpy(), rtol=1e-5, atol=1e-6)
    x = ((torch.rand(4000, generator=g) - 0.3) * 200).float()
    r = np.zeros(4000, np.float32)
    hl.hc_rem1(np.ascontiguousarray(x.numpy()), 4000, r)
    assert np.array_equal(r, (x % 1).numpy())


@pytest.mark.parametrize("pw,gamma", [(1.0, 1.5), (2.5, 2.0), (1.0, 0.0)])
def test_focal_bce_forward_and_gradient(hl, pw, gamma):
    """FocalLoss around BCEWithLogitsLoss (utils/loss.py:35-62): element values and hand-written derivative vs torch autograd
    of the restatement; gamma = 0 is the plain BCE."""
    g = torch.Generator().manual_seed(7)
    n = 20000
    x = (torch.randn(n, generator=g) * 5).requires_grad_(True)
    t = torch.rand(n, generator=g)
    t[: n // 3] = (t[: n // 3] > 0.5).float()
    pwt = torch.tensor([pw])
    if gamma > 0:
        loss = pyref.focal_bce(x, t, pwt, gamma) * n          # (mean * n = sum of the element losses)
    else:
        loss = torch.nn.functional.binary_cross_entropy_with_logits(x, t, pos_weight=pwt, reduction='sum')
    loss.backward()
    out = np.zeros((n, 2), np.float32)
    hl.hc_focal(np.ascontiguousarray(torch.stack((x.detach(), t), 1).numpy()), n, pw, gamma, out)
    assert abs(out[:, 0].astype(np.float64).sum() - float(loss)) <= 1e-5 * abs(float(loss))
    assert np.allclose(out[:, 1], x.grad.numpy(), rtol=2e-5, atol=2e-6), np.abs(out[:, 1] - x.grad.numpy()).max()


# ----------------------------------------------------------------------------- saturation grid
# The tests above stay inside |x| < 30 with atol 1e-6, which is larger than anything that happens beyond |x| = 16.  A trained
# head's background sits at -5..-12, peaks and fp16 overflow go to +-inf: the grid below walks through the points where
# sigmoid, 1 - sigmoid and exp(-|x|) leave the fp32 range one after the other (16-17: 1 - sigmoid(x) becomes 0 / 1; 88.8:
# expf overflows; 104: expf(-x) becomes 0 past the subnormals).
SAT_X = [0.0] + [s * v for v in (4.6, 8, 12, 16, 17, 20, 30, 50, 88.8, 100, 104, 200, 1e30, float("inf")) for s in (1, -1)] \
    + [float("nan")]
SAT_T = [0.0, 0.3, 0.95, 1.0]
SAT_RTOL, SAT_ATOL = 1e-5, 1.2e-7         # one fp32 ulp of 1: the size of the 1 - sigmoid cancellation in bce_logits_grad


def _torch_focal(x, t, pw, gamma):
    """(element losses, d sum / dx) of torch fp32: BCEWithLogits(pos_weight), wrapped in FocalLoss when gamma > 0."""
    x = x.clone().requires_grad_(True)
    pwt = torch.tensor([pw])
    if gamma > 0:
        loss = torch.nn.functional.binary_cross_entropy_with_logits(x, t, pos_weight=pwt, reduction='none')
        p = torch.sigmoid(x)
        p_t = t * p + (1 - t) * (1 - p)
        loss = loss * (t * 0.25 + (1 - t) * 0.75) * (1.0 - p_t) ** gamma          # utils/loss.py:35-62, as pyref.focal_bce
    else:
        loss = torch.nn.functional.binary_cross_entropy_with_logits(x, t, pos_weight=pwt, reduction='none')
    loss.sum().backward()
    return loss.detach().numpy(), x.grad.numpy()


def saturation_grid_mismatches(lib, pw, gamma):
    """[(what, x, t, ours, torch)] over SAT_X x SAT_T: an isfinite pattern that differs from torch fp32, or a finite value
    outside SAT_RTOL * |torch| + SAT_ATOL.  inf against NaN is a pattern match: both are non-finite."""
    x = torch.tensor([xv for xv in SAT_X for _ in SAT_T], dtype=torch.float32)
    t = torch.tensor([tv for _ in SAT_X for tv in SAT_T], dtype=torch.float32)
    want = _torch_focal(x, t, pw, gamma)
    out = np.zeros((len(x), 2), np.float32)
    lib.hc_focal(np.ascontiguousarray(torch.stack((x, t), 1).numpy()), len(x), pw, gamma, out)
    bad = []
    for k, what in enumerate(("loss", "grad")):
        got, ref = out[:, k], want[k]
        fin = np.isfinite(ref)
        for i in np.nonzero(np.isfinite(got) != fin)[0]:
            bad.append((what + " isfinite", float(x[i]), float(t[i]), float(got[i]), float(ref[i])))
        both = fin & np.isfinite(got)
        err = np.abs(got[both].astype(np.float64) - ref[both])
        for i in np.nonzero(both)[0][err > SAT_RTOL * np.abs(ref[both]) + SAT_ATOL]:
            bad.append((what, float(x[i]), float(t[i]), float(got[i]), float(ref[i])))
    return bad, out, want


SAT_CONFIGS = [(1.0, 0.0), (2.5, 0.0), (1.0, 1.5), (1.0, 2.0), (1.0, 0.5)]


@pytest.mark.parametrize("pw,gamma", SAT_CONFIGS)
def test_saturation_grid(hl, pw, gamma):
    """bce_logits / bce_focal and their gradients where the logits saturate, overflow or are not finite, against torch fp32:
    the same isfinite pattern and, where finite, |k - torch| <= 1e-5 |torch| + 1.2e-7 (measured: the largest absolute gap is
    2e-8, at x = -17, t = 0, where the header's (1-t) - lw (1 - sigmoid) is exactly 0 and ATen's sigmoid - t keeps 4e-8).
    gamma = 0.5 gives NaN gradients at |x| >= 17 in torch and in the header alike ((1 - p_t)^(gamma - 1) at 0)."""
    bad, out, want = saturation_grid_mismatches(hl, pw, gamma)
    fin = np.isfinite(want[1]) & np.isfinite(out[:, 1])
    print(f"saturation grid pw {pw} gamma {gamma}: largest |grad - torch| {np.abs(out[fin, 1] - want[1][fin]).max():.1e}, "
          f"non-finite losses {int((~np.isfinite(want[0])).sum())}, gradients {int((~np.isfinite(want[1])).sum())} of {len(out)}")
    assert not bad, bad[:8]
    if gamma == 0.5:
        assert (~np.isfinite(want[1])).sum() > (~np.isfinite(want[0])).sum()       # NaN gradients next to finite losses


def test_bce_gradient_does_not_lose_the_background(hl):
    """t = 0, x in [-16, -5] (background objectness): the header's gradient (1-t) - lw (1 - sigmoid(x)) against sigmoid(x) in
    double stays within one fp32 ulp of 1 absolute -- the cancellation's size -- and is never negative."""
    x = torch.linspace(-16.0, -5.0, 4401)
    out = np.zeros((len(x), 2), np.float32)
    hl.hc_bce(np.ascontiguousarray(torch.stack((x, torch.zeros_like(x)), 1).numpy()), len(x), 1.0, out)
    ref = torch.sigmoid(x.double()).numpy()
    assert np.abs(out[:, 1] - ref).max() <= SAT_ATOL and (out[:, 1] >= 0).all()
