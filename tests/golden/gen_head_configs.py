"""Generate tests/golden/head_configs.npz from the REFERENCE's own models/yolo.py (run in the build container only).

    YOLOV5_CONFIG_DIR=/tmp/refcfg python tests/golden/gen_head_configs.py

The head configurations of tests/head_cases.py through the inference branch of the reference's Detect (imported with the stubs
of gen_golden.py; its 1x1 convs replaced by identities, so that the seeded conv outputs of tests/head_cases.py are what it
decodes), on the CPU in fp32.  Stored per case is a digest, not the tensors: per level and channel group (xy, wh, obj, cls,
csl) the sum and the sum of magnitudes of z in float64, and 32 seeded rows of z in full.  While generating, the float64
formula of tests/head_cases.py and the oracle (oracle/pyref.py) are checked against every stored value.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden                  # noqa: E402  (puts the repository root on sys.path)
from oracle import pyref           # noqa: E402
from tests import head_cases as H  # noqa: E402


def check_against(case, z, sums, rows, what):
    """z (numpy, (bs, A, no)) against the stored digest within the project's fp32 rule (1e-6 + 2e-6 |ref|); the sums within
    the same rule summed over their elements."""
    gs = H.group_sums(case, z)
    n = np.array([[case.bs * r * w for w in (2, 2, 1, case.nc, H.CSL)] for r in case.level_rows], np.float64)
    assert np.all(np.abs(gs - sums) <= 1e-6 * n[..., None] + 2e-6 * sums[..., 1:2]), (case.name, what, gs, sums)
    got = np.asarray(z).reshape(-1, case.no)[H.sampled_rows(case)]
    assert H.close_fp32(got, rows).all(), (case.name, what)


def main():
    import oracle
    oracle.build(with_ref=True)
    Y = gen_golden.load_reference()[5]
    torch.set_num_threads(1)
    out = {}
    for case in H.CASES:
        cv = H.convs(case, torch.float32)
        d = Y.Detect(nc=case.nc, anchors=H.detect_anchor_arg(case), ch=(4,) * case.nl)
        d.stride = torch.tensor(H.strides(case))
        d.anchors /= d.stride.view(-1, 1, 1)
        d.m = torch.nn.ModuleList([torch.nn.Identity() for _ in range(case.nl)])
        d.eval()
        with torch.no_grad():
            z, xs = d([c.clone() for c in cv])
        assert z.shape == (case.bs, case.a_total, case.no) and z.dtype == torch.float32
        zn = z.numpy()
        sums = H.group_sums(case, zn)
        rows = zn.reshape(-1, case.no)[H.sampled_rows(case)].copy()
        zr, xr, _ = H.decode_ref(case, None, torch.float32)
        for a, b in zip(xs, xr):
            assert np.array_equal(a.numpy(), b), case.name
        check_against(case, zr, sums, rows, "decode_ref")
        assert H.close_fp32(zr, zn).all(), case.name
        zp = pyref.detect_decode([torch.from_numpy(x) for x in xr], torch.from_numpy(H.anchors_px(case)) / d.stride.view(-1, 1, 1),
                                 d.stride)
        check_against(case, zp.numpy(), sums, rows, "pyref.detect_decode")
        assert H.close_fp32(zp.numpy(), zn).all(), case.name
        out[f"{case.name}_sums"] = sums
        out[f"{case.name}_rows"] = rows
        print(f"{case.name}: z {tuple(z.shape)} sum |z| {np.abs(zn.astype(np.float64)).sum():.6g}")
    path = os.path.join(HERE, "head_configs.npz")
    np.savez_compressed(path, **out)
    print(f"wrote tests/golden/head_configs.npz ({os.path.getsize(path) / 1024:.0f} KiB, {len(out)} arrays)")


if __name__ == "__main__":
    main()
