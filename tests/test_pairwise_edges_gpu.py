"""GPU parity at the sizes and magnitudes where yolov5_obb_amd/csrc/pairwise.hip takes branches no other test reaches.

A. k_quad_strip with more than one column tile per workgroup (chunk 128, 192 and the clamp 1024; both template flavours):
   the ring queue across tiles, ragged last chunks, a ragged last strip.  Whole matrix against 256-column slabs on the device
   (the chunk == 64 code the other tests pin to the oracle), whole strips against the oracle.
B. NaN, +-inf, +-1e19 .. +-3e38, 1e-40, -0.0, zero / negative sides and wild angles through all four pairwise entries, incl.
   the pairs on which an ungated first cone rule writes +0 where the reference has NaN.
C. obb_eval_best_gt_f64 over more than one grid pass (16384 detections) with a ragged last workgroup.
D. Tile edges of k_riou_matrix, row strides 9 / 10 and views through quad_iou_matrix, the (N, 6) guard of rbox_overlaps, the
   row limit of obb_rotated_iou_matrix_f32.

Wall time of each test on an MI355X (pytest --durations, call phase), and the part of it spent in the CPU oracle (printed by
the tests, `-s`):
  test                                                         wall     oracle
  test_quad_strip_multi_tile_chunks[22037-1000-128-quad]       0.43 s   0.11 s
  test_quad_strip_multi_tile_chunks[22037-1000-128-devkit]     0.12 s   0.11 s
  test_quad_strip_multi_tile_chunks[33027-1000-192-quad]       0.16 s   0.13 s
  test_quad_strip_multi_tile_chunks[33027-1000-192-devkit]     0.19 s   0.17 s
  test_quad_strip_multi_tile_chunks[70465-2500-1024-quad]      0.47 s   0.33 s   (705 MB of output; kept)
  test_quad_strip_multi_tile_chunks[70465-2500-1024-devkit]    0.31 s   0.29 s
  test_quad_iou_matrix_huge_and_non_finite                     0.03 s   0.02 s
  test_rbox_overlaps_huge_and_non_finite                       0.01 s   0.01 s
  test_rotated_iou_huge_and_non_finite                         0.01 s   < 0.01 s
  test_best_gt_beyond_one_grid_pass[16384]                     0.06 s   0.05 s   (pyref on the 714 base detections, once)
  test_best_gt_beyond_one_grid_pass[16385], [32771]            < 0.005 s each
  test_rotated_iou_matrix_tile_edges (five cases)              < 0.005 s each
  test_quad_iou_matrix_row_strides_and_views                   0.13 s   0.01 s
  test_rbox_overlaps_rejects_wider_rows                        < 0.005 s
  test_rotated_iou_matrix_row_limit                            0.01 s
The first test also pays for loading the library (0.3 s).
"""
import time

import numpy as np
import pytest
import torch

import oracle
from oracle import pyref
from tests import synth
from tests.test_eval_gpu import best_gt_inputs

pytestmark = pytest.mark.gpu

_ORACLE_S = [0.0]


def _oracle(fn, *args):
    t0 = time.perf_counter()
    r = fn(*args)
    _ORACLE_S[0] += time.perf_counter() - t0
    return r


@pytest.fixture(autouse=True)
def _oracle_share():
    _ORACLE_S[0] = 0.0
    yield
    print(f" [oracle {_ORACLE_S[0]:.2f} s]", end="")


def _bits_or_nan(got, ref):
    return (got.view(np.uint32) == ref.view(np.uint32)) | (np.isnan(got) & np.isnan(ref))


def _assert_exact(got, ref, what=""):
    same = _bits_or_nan(got, ref)
    if not same.all():
        i = tuple(int(v) for v in np.argwhere(~same)[0])
        raise AssertionError(f"{what}: {np.count_nonzero(~same)} of {same.size} entries differ from the oracle; first at {i}: "
                             f"got {got[i]!r} ({got.view(np.uint32)[i]:08x}), oracle {ref[i]!r} ({ref.view(np.uint32)[i]:08x})")


def _assert_devkit_bar(got, ref, what=""):
    """The bar of test_ops_rbox_overlaps_device_tensors (>= 0.999 of the entries bit-equal, max error <= 1e-5: the two double
    libms may differ in a last bit of cos / sin), with NaN at the same positions."""
    assert np.array_equal(np.isnan(got), np.isnan(ref)), f"{what}: NaN positions differ ({np.isnan(got).sum()} / {np.isnan(ref).sum()})"
    same = _bits_or_nan(got, ref)
    err = np.abs(got[~same] - ref[~same])
    print(f" [{what}: bit-equal {same.mean():.6f}, max err {err.max() if err.size else 0.0:.3g}]", end="")
    assert same.mean() >= 0.999 and (err <= 1e-5).all(), (what, same.mean(), err)


# ---- A. multi-tile chunks of k_quad_strip --------------------------------------------------------------------------------
def _quad_strip_chunk(n, k):
    """quad_strip_launch (csrc/pairwise.hip): columns per workgroup."""
    strips = (n + 15) // 16
    return min(max(strips * k // 10752 // 64 * 64, 64), 1024)


@pytest.mark.parametrize("flavour", ["quad", "devkit"])
@pytest.mark.parametrize("n,k,chunk,extent", [(22037, 1000, 128, 1024.0), (33027, 1000, 192, 200.0), (70465, 2500, 1024, 30000.0)])
def test_quad_strip_multi_tile_chunks(dev, oracle_lib, flavour, n, k, chunk, extent):
    """22037 x 1000: 8 chunks of 128, the last of 104 columns (a full tile and a partial one), 5 rows in the last strip, ~4 % of
    the IoUs non-zero.  33027 x 1000: chunks of 192, the last a 40-column partial tile; most pairs are clipped: the queue drains
    many times per tile.  70465 x 2500: the clamp at 1024; nearly every pair is an exact zero: entries ride the ring across many
    tiles.  (1) every 256-column slab of the matrix, computed on its own -- 64-column chunks, the code the other tests pin to the
    oracle -- has the same bits; (2) strips 0, 1, the middle one, the ragged last one and nine random ones against the oracle."""
    from yolov5_obb_amd import ops
    assert _quad_strip_chunk(n, k) == chunk and _quad_strip_chunk(n, 256) == 64
    a, _ = synth.s_uniform(n, 41, extent=extent)
    b, _ = synth.s_uniform(k, 141, extent=extent)
    if flavour == "quad":
        a, b = synth.rbox_to_quad(a), synth.rbox_to_quad(b)
        b[::5] = b[::5].reshape(-1, 4, 2).flip(1).reshape(-1, 8)                                  # reversed rings
        a[::7] = a[::7].reshape(-1, 4, 2).flip(1).reshape(-1, 8)
        a[1::9] = a[1::9].round(); b[2::9] = b[2::9].round()
        a[5] = torch.tensor([-3.0, -2.0, 40.0, -2.0, 40.0, 30.0, -3.0, 30.0])                     # around the origin: no cone
        entry, ref_fn = ops.quad_iou_matrix, oracle.piou_matrix
    else:
        entry, ref_fn = ops.rbox_overlaps, oracle.devkit_overlaps
    da, db = a.to(dev), b.to(dev)
    full = entry(da, db)
    assert full.shape == (n, k)
    for j0 in range(0, k, 256):
        j1 = min(j0 + 256, k)
        slab = entry(da, db[j0:j1])
        assert torch.equal(full[:, j0:j1].view(torch.int32), slab.view(torch.int32)), f"columns {j0}:{j1} differ from their own slab"
    strips = (n + 15) // 16
    rng = np.random.RandomState(n)
    others = np.setdiff1d(np.arange(2, strips - 1), [strips // 2])
    pick = sorted({0, 1, strips // 2, strips - 1, *rng.choice(others, 9, replace=False).tolist()})
    rows = np.concatenate([np.arange(s * 16, min(s * 16 + 16, n)) for s in pick])
    assert len(pick) == 13 and n - 16 < rows[-1] == n - 1 and n % 16 != 0
    got = full[torch.from_numpy(rows).to(dev)].cpu().numpy()
    ref = _oracle(ref_fn, a[rows].numpy(), b.numpy())
    assert extent > 1024.0 or (ref > 0).sum() > 1000               # (at 30,000 px a 197 x 2500 sample holds a handful at most)
    if flavour == "quad":
        _assert_exact(got, ref, f"{n} x {k}")
    else:
        _assert_devkit_bar(got, ref, f"{n} x {k}")


# ---- B. huge and non-finite inputs ---------------------------------------------------------------------------------------
_SPECIALS = [float("nan"), -float("nan"), float("inf"), -float("inf"), 1e19, -1e19, 1e25, -1e25, 1e30, -1e30, 3e38, -3e38,
             1e-40, -0.0]
_HUGE_SCALES = (1e25, 1e30, 1e37)


def _square_quad(cx, cy, side):
    h = side / 2
    return [cx - h, cy - h, cx + h, cy - h, cx + h, cy + h, cx - h, cy + h]


def _special_quads(n, seed):
    """n ordinary quads; quad 8 v + c carries special value v in coordinate c (112 quads), then the counter-examples of the
    ungated first cone rule: for s = 1e25, 1e30, 1e37 the 0.05 s squares P at (s, 0.1 s) and Q at (0.1 s, s), and an ordinary 5 x 5
    box at (100, 10)."""
    d, _ = synth.s_uniform(n, seed, extent=300.0)
    q = synth.rbox_to_quad(d)
    r = 0
    for v in _SPECIALS:
        for c in range(8):
            q[r, c] = v; r += 1
    for s in _HUGE_SCALES:
        q[r] = torch.tensor(_square_quad(s, 0.1 * s, 0.05 * s)); q[r + 1] = torch.tensor(_square_quad(0.1 * s, s, 0.05 * s)); r += 2
    q[r] = torch.tensor(_square_quad(100.0, 10.0, 5.0)); r += 1
    assert r == 119 <= n
    return q


def _special_rboxes(n, seed):
    """n ordinary rboxes; the specials in every column, zero and negative sides, theta = 1e10 / NaN, and the counter-examples of
    _special_quads as rboxes with theta = 0."""
    d, _ = synth.s_uniform(n, seed, extent=300.0)
    r = 0
    for v in _SPECIALS:
        for c in range(5):
            d[r, c] = v; r += 1
    for c, v in ((2, 0.0), (3, 0.0), (2, -5.0), (3, -7.0), (4, 1e10), (4, float("nan"))):
        d[r, c] = v; r += 1
    d[r, 2:4] = 0.0; r += 1
    for s in _HUGE_SCALES:
        d[r] = torch.tensor([s, 0.1 * s, 0.05 * s, 0.05 * s, 0.0]); d[r + 1] = torch.tensor([0.1 * s, s, 0.05 * s, 0.05 * s, 0.0]); r += 2
    d[r] = torch.tensor([100.0, 10.0, 5.0, 5.0, 0.0]); r += 1
    assert r == 84 <= n
    return d


def test_quad_iou_matrix_huge_and_non_finite(dev, oracle_lib):
    """Every special quad as a row and as a column.  P (row) against Q (column) is where the first cone rule fires without a
    coordinate bound: the reference's products overflow there and its IoU is NaN, not +0."""
    from yolov5_obb_amd import nms_rotated_ext, ops
    qa, qb = _special_quads(130, 51), _special_quads(200, 52)
    got = ops.quad_iou_matrix(qa.to(dev), qb.to(dev)).cpu().numpy()
    ref = _oracle(oracle.piou_matrix, qa.numpy(), qb.numpy())
    assert np.isnan(ref[112, 113]) and np.isnan(ref[118, 113]) and np.isnan(ref).sum() > 1000 and (ref > 0).sum() > 100
    _assert_exact(got, ref, "quad_iou_matrix")
    # the quad NMS on a list with the finite ones of these quads (huge, tiny and -0 coordinates): NaN is never > thr
    fin = torch.isfinite(qb).all(1)
    polys = torch.cat([qb[fin], synth.tie_free(torch.rand(int(fin.sum()), generator=torch.Generator().manual_seed(5)))[:, None]], 1).contiguous()
    assert (polys[:, :8].abs() > 1e24).any(1).sum() >= 30
    assert np.array_equal(nms_rotated_ext.nms_poly(polys.to(dev), 0.1).cpu().numpy(), _oracle(oracle.nms_poly, polys.numpy(), 0.1))


def test_rbox_overlaps_huge_and_non_finite(dev, oracle_lib):
    from yolov5_obb_amd import ops
    a, b = _special_rboxes(130, 53), _special_rboxes(200, 54)
    got = ops.rbox_overlaps(a.to(dev), b.to(dev)).cpu().numpy()
    ref = _oracle(oracle.devkit_overlaps, a.numpy(), b.numpy())
    assert np.isnan(ref[77, 78]) and np.isnan(ref[83, 78]) and np.isnan(ref).sum() > 1000 and (ref > 0).sum() > 100
    _assert_devkit_bar(got, ref, "rbox_overlaps")


def test_rotated_iou_huge_and_non_finite(dev, oracle_lib):
    """k_riou_matrix (with its reject, rbox_certainly_disjoint) and k_riou_pairs: bit for bit, as test_rotated_iou_matrix asks
    at this size."""
    from yolov5_obb_amd import ops
    a, b = _special_rboxes(130, 53), _special_rboxes(200, 54)
    got = ops.rotated_iou_matrix(a.to(dev), b.to(dev)).cpu().numpy()
    ref = _oracle(oracle.riou_matrix, a.numpy(), b.numpy())
    assert (ref > 0).sum() > 100
    _assert_exact(got, ref, "rotated_iou_matrix")
    for b130 in (b[:130], b[70:200], a.roll(1, 0)):
        gp = ops.rotated_iou_pairs(a.to(dev), b130.contiguous().to(dev)).cpu().numpy()
        _assert_exact(gp, _oracle(oracle.riou_pairs, a.numpy(), b130.contiguous().numpy()), "rotated_iou_pairs")


# ---- C. obb_eval_best_gt_f64 beyond one grid pass ------------------------------------------------------------------------
_BEST_GT_BASE = []


def _best_gt_base():
    """The arrays of test_best_gt_vs_oracle_per_detection and the kernel's (ovmax, jmax) on them, checked against pyref once."""
    if not _BEST_GT_BASE:
        from yolov5_obb_amd.DOTA_devkit.dota_evaluation_task1 import best_gt
        dets, dimg, gts, off = best_gt_inputs()
        ov, jm = best_gt(dets, dimg, gts, np.array(off))
        n_nan = n_none = 0
        for d in range(len(dets)):
            ro, rj = _oracle(pyref.task1_best_gt, dets[d], gts[off[dimg[d]]:off[dimg[d] + 1]])
            if rj is None:
                assert ov[d] == -np.inf and jm[d] == -1; n_none += 1
            elif np.isnan(ro):
                assert np.isnan(ov[d]) and jm[d] == rj; n_nan += 1
            else:
                assert ov[d] == ro and jm[d] == rj, (d, ov[d], ro, jm[d], rj)
        assert n_none > 20 and n_nan > 0 and len(dets) - n_none - n_nan > 200
        _BEST_GT_BASE.append((dets, dimg, gts, np.array(off), ov, jm))
    return _BEST_GT_BASE[0]


@pytest.mark.parametrize("nd", [16384, 16385, 2 * 16384 + 3])
def test_best_gt_beyond_one_grid_pass(dev, oracle_lib, nd):
    """k_eval_best_gt runs at most 4096 workgroups x 4 waves = 16384 detections per pass of its grid-stride loop: exactly one
    pass, one detection into the second, and three passes whose last workgroup has one idle wave.  The base detections cycled in
    shuffled order: every copy gets the (ovmax, jmax) of its base detection, bit for bit, NaNs included."""
    from yolov5_obb_amd.DOTA_devkit.dota_evaluation_task1 import best_gt
    dets, dimg, gts, off, ov0, jm0 = _best_gt_base()
    src = np.random.RandomState(nd).permutation(np.arange(nd) % len(dets))
    ov, jm = best_gt(dets[src], dimg[src], gts, off)
    assert ov.shape == (nd,) and np.isnan(ov).any()
    assert np.array_equal(ov.view(np.uint64), ov0[src].view(np.uint64)) and np.array_equal(jm, jm0[src])


# ---- D. wrapper and tile edges -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k", [(1, 1), (64, 64), (65, 1), (1, 65), (129, 63)])
def test_rotated_iou_matrix_tile_edges(dev, oracle_lib, n, k):
    from yolov5_obb_amd import ops
    a, _ = synth.s_uniform(n, 61, extent=120.0)
    b, _ = synth.s_uniform(k, 62, extent=120.0)
    b[0, :2] = a[n - 1, :2] + 1.0                                                   # the last row overlaps the first column
    got = ops.rotated_iou_matrix(a.to(dev), b.to(dev)).cpu().numpy()
    ref = _oracle(oracle.riou_matrix, a.numpy(), b.numpy())
    assert got.shape == (n, k) and ref[n - 1, 0] > 0
    _assert_exact(got, ref, f"{n} x {k}")


def test_quad_iou_matrix_row_strides_and_views(dev, oracle_lib):
    """Rows of 9 (polys + score) and 10 (+ class) floats go to the kernel with their stride; a strided view is made contiguous."""
    from yolov5_obb_amd import ops
    a, sa = synth.s_uniform(150, 63, extent=150.0)
    b, sb = synth.s_uniform(97, 64, extent=150.0)
    qa9 = torch.cat([synth.rbox_to_quad(a), sa[:, None]], 1).to(dev)
    qb10 = torch.cat([synth.rbox_to_quad(b), sb[:, None], torch.arange(97.0)[:, None]], 1).to(dev)
    want = ops.quad_iou_matrix(qa9[:, :8].contiguous(), qb10[:, :8].contiguous())
    _assert_exact(want.cpu().numpy(), _oracle(oracle.piou_matrix, qa9[:, :8].cpu().numpy(), qb10[:, :8].cpu().numpy()), "stride 8")
    assert (want > 0).sum() > 100
    for x, y in ((qa9, qb10), (qa9[:, :8], qb10), (qa9, qb10[:, :9])):
        assert torch.equal(ops.quad_iou_matrix(x, y), want)
    va, vb = qa9[::2], qb10[::2]
    assert not va.is_contiguous() and not vb.is_contiguous()
    assert torch.equal(ops.quad_iou_matrix(va, vb), want[::2, ::2])


def test_rbox_overlaps_rejects_wider_rows(dev):
    """obb_rbox_overlaps_f32 takes no row stride: an (N, 6) tensor (rbox + score) would be read as rows of five."""
    from yolov5_obb_amd import ops
    from yolov5_obb_amd.DOTA_devkit.poly_nms_gpu import poly_overlaps
    a, sa = synth.s_uniform(40, 65, extent=100.0)
    b, _ = synth.s_uniform(30, 66, extent=100.0)
    a6 = torch.cat([a, sa[:, None]], 1)
    with pytest.raises(RuntimeError):
        ops.rbox_overlaps(a6.to(dev), b.to(dev))
    with pytest.raises(RuntimeError):
        ops.rbox_overlaps(a.to(dev), a6.to(dev))
    with pytest.raises(ValueError):
        poly_overlaps(a6.numpy(), b.numpy())
    with pytest.raises(ValueError):
        poly_overlaps(b.numpy(), a6.numpy())
    assert ops.rbox_overlaps(a.to(dev), b.to(dev)).shape == (40, 30)


def test_rotated_iou_matrix_row_limit(dev):
    """k_riou_matrix puts the 64-row tiles on the grid's y axis (<= 65535): one row more is refused before anything is launched."""
    from yolov5_obb_amd import ops
    n = 65535 * 64 + 1
    a = torch.zeros(n, 5, device=dev)
    b = torch.ones(1, 5, device=dev)
    with pytest.raises(RuntimeError, match="obb_rotated_iou_matrix_f32 failed: bad argument"):
        ops.rotated_iou_matrix(a, b)
    torch.cuda.synchronize(dev)
    assert ops.rotated_iou_matrix(a[:65], b).shape == (65, 1)
