"""CPU checks behind tests/test_head_configs_gpu.py: the float64 formula of tests/head_cases.py (the reference of the GPU tests)
agrees with the oracle, with torch's own fp16 op chain and with the reference's Detect (tests/golden/head_configs.npz, written
by tests/golden/gen_head_configs.py); and the seeded inputs exercise what the GPU tests are there for -- kept rows, confidences
tied across anchors and across levels -- judged by the oracle's NMS alone."""
import os

import numpy as np
import pytest
import torch

from oracle import pyref
from tests import head_cases as H

FIX = None


def fixture():
    global FIX
    if FIX is None:
        FIX = np.load(os.path.join(os.path.dirname(__file__), "golden", "head_configs.npz"))
    return FIX


def test_cases_cover_the_shape_dependent_code():
    """The properties the cases are named for (csrc/head.hip, csrc/nms_head.h), from the launch arithmetic alone."""
    lds = lambda no, esz: (no * 64 + 2 * (no // 8 + 2)) * esz                        # obb_detect_decode_col
    c = H.BY_NAME
    assert c["nl2_na4_nc6"].no == 191 and lds(191, 4) == 49096 <= 48 * 1024 < lds(c["nl2_na4_nc7"].no, 4) == 49360
    assert lds(c["nl1_na8_nc256_vec"].no, 4) == 113352 and c["nl1_na8_nc256_vec"].no * 65 * 4 == 114660      # decode / head front
    assert c["nl2_na2_nc71"].no == 256 and c["nl2_na2_nc72"].no == 257               # 256 threads: NT / no = 1 and 0
    hw = lambda k, l: k.sizes[l][0] * k.sizes[l][1]
    assert hw(c["nl1_na8_nc256_vec"], 0) % 8 == 0 and hw(c["nl1_na8_nc256_odd"], 0) % 4 != 0
    k = c["nl3_na3_nc16_straddle"]
    assert [hw(k, l) for l in range(3)] == [180, 182, 12] and 180 % 64 == 52 and 64 % k.sizes[0][1] != 0
    k = c["nl3_na5_nc33_hw12"]
    assert k.no % 2 == 0 and hw(k, 0) % 4 == 0 and hw(k, 1) == 12 and all(hw(k, l) % 8 for l in range(3))
    k = c["nl4_na1_nc200_1x1tail"]
    assert [hw(k, l) % 4 for l in range(4)] == [0, 0, 0, 1]
    assert c["nl3_na2_nc2_bs16"].bs * c["nl3_na2_nc2_bs16"].na == 32
    for k in H.CASES:
        assert 1 <= k.nl <= 4 and 1 <= k.na <= 8 and 1 <= k.nc <= 256
        a = H.anchors_px(k)
        assert a.shape == (k.nl, k.na, 2) and len(set(a.reshape(-1).tolist())) == a.size
    assert {k.nl for k in H.CASES} == {1, 2, 3, 4} and {k.na for k in H.CASES} >= {1, 2, 3, 4, 5, 8}
    p6 = H.anchors_px(c["nl4_na8_nc18_p6"])
    assert np.array_equal(p6[:, :3].reshape(4, 6), np.asarray(H.synth.P6_ANCHORS, np.float32))


@pytest.mark.parametrize("name", H.NAMES)
def test_inputs_are_tied_and_saturate(name):
    case = H.BY_NAME[name]
    for dtype in (torch.float32, torch.float16):
        cv = H.convs(case, dtype)
        assert [tuple(c.shape) for c in cv] == [(case.bs, case.na * case.no, ny, nx) for ny, nx in case.sizes]
        assert all(c.dtype == dtype and c.is_contiguous() for c in cv)
        assert 11.0 <= max(float(c.float().abs().max()) for c in cv) <= 12.0
    if case.bs * case.a_total >= 50:                                    # (the 1 x 1 head has two rows in all)
        z16 = H.decode_ref(case, None, torch.float16)[0]
        assert (z16[..., 4:] == 1.0).any(), "no sigmoid saturates in fp16"
        assert (z16[..., 4:] < 2.0 ** -14).any(), "no fp16 subnormal"


@pytest.mark.parametrize("name", H.NAMES)
def test_formula_matches_oracle_fp32(name):
    case = H.BY_NAME[name]
    z, xp, col = H.decode_ref(case, None, torch.float32)
    st = torch.tensor(H.strides(case))
    ref = pyref.detect_decode([torch.from_numpy(x) for x in xp], torch.from_numpy(H.anchors_px(case)) / st.view(-1, 1, 1), st)
    assert z.shape == tuple(ref.shape) == (case.bs, case.a_total, case.no) and z.dtype == np.float32
    assert H.close_fp32(z, ref.numpy()).all()
    assert H.close_fp32(z, H.torch_chain(case, H.convs(case, torch.float32)).numpy()).all()
    assert np.array_equal(col, z[..., 4])


BIT_EQUAL = {}


@pytest.mark.parametrize("name", H.NAMES)
def test_formula_matches_torch_chain_fp16(name):
    """The float64 model with fp16 roundings against torch's CPU fp16 ops: one fp16 ulp, as tests/test_head_gpu.py allows the
    kernel (a float64 value rounded to fp16 can differ from its float32 rounding rounded to fp16 at ties)."""
    case = H.BY_NAME[name]
    z = H.decode_ref(case, None, torch.float16)[0]
    ref = H.torch_chain(case, H.convs(case, torch.float16))
    assert ref.dtype == torch.float16 and z.dtype == np.float16 and z.shape == tuple(ref.shape)
    ref = ref.numpy()
    assert H.close_fp16(z, ref).all()
    same = float((z == ref).mean())
    BIT_EQUAL[name] = same
    print(f"{name}: {same * 100:.4f} % of {z.size} fp16 elements bit-equal to torch's CPU chain")
    assert same > 0.98


@pytest.mark.parametrize("name", H.NAMES)
def test_formula_matches_reference_fixture(name):
    """decode_ref (fp32) against the digest of the reference's own Detect.forward."""
    case, g = H.BY_NAME[name], fixture()
    z = H.decode_ref(case, None, torch.float32)[0]
    sums, rows = g[f"{name}_sums"], g[f"{name}_rows"]
    assert sums.shape == (case.nl, 5, 2) and rows.shape == (min(H.N_SAMPLED, case.bs * case.a_total), case.no)
    got = z.reshape(-1, case.no)[H.sampled_rows(case)]
    assert H.close_fp32(got, rows).all()
    n = np.array([[case.bs * r * w for w in (2, 2, 1, case.nc, H.CSL)] for r in case.level_rows], np.float64)
    gs = H.group_sums(case, z)
    assert np.all(np.abs(gs - sums) <= 1e-6 * n[..., None] + 2e-6 * sums[..., 1:2]), (gs, sums)


@pytest.mark.parametrize("multi_label", [True, False])
@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("name", H.NAMES)
def test_inputs_exercise_the_nms(name, half, multi_label):
    """Conditions on the INPUTS, from the oracle alone (H.coverage_floor)."""
    case = H.BY_NAME[name]
    z = torch.from_numpy(H.decode_ref(case, None, torch.float16 if half else torch.float32)[0])
    kept = pyref.non_max_suppression_obb(z.clone(), multi_label=multi_label, **H.KW)
    got, need = H.nms_coverage(case, z, kept, multi_label), H.coverage_floor(case)
    assert all(g >= n for g, n in zip(got, need)), (got, need)
    assert all(k.shape[0] < H.KW["max_det"] for k in kept)


def test_doubling_a_sigmoid_is_exact_in_fp16():
    """models/yolo.py:73-74 computes y * 2 in the tensor dtype.  For every fp16 y in [0, 1] the product is exact (the exponent
    moves, no bit is lost, 2 is far from overflow), so the rounding after it is an identity: decode_ref's and the kernels'
    (csrc/detect_math.h) round there changes no value, and no test can tell whether it is made.  The roundings after - 0.5 and
    after the square are not identities."""
    y = np.arange(0, 0x3C01, dtype=np.uint16).view(np.float16)                     # every fp16 value in [0, 1]
    assert y[0] == 0.0 and y[-1] == 1.0
    t = y.astype(np.float64) * 2.0
    assert np.array_equal(t.astype(np.float16).astype(np.float64), t)
    u, q = t - 0.5, t * t
    assert (u.astype(np.float16).astype(np.float64) != u).any() and (q.astype(np.float16).astype(np.float64) != q).any()
