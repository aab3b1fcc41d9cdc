"""CPU: obb_non_max_suppression_obb_tta_head without a device -- the symbol, its argument refusals, and the host-only builder of its
entry table (yolov5_obb_amd/csrc/tta_head_plan.h), compiled with g++ behind a serial driver (tests/native/host_tta_head_plan.cpp)
and held to models.yolo.tta_plan."""
import ctypes as C
import math
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F16, BF16 = 0, 1, 3
CASES = {   # name -> (na, nl, no, maps per pass); the first three are tests/test_tta_decode_gpu.py's CASES, the last is bench.py's TTA shape
    "nc3_128": (3, 3, 188, [[(16, 16), (8, 8), (4, 4)], [(16, 16), (8, 8), (4, 4)], [(12, 12), (6, 6), (3, 3)]]),
    "nc16_160x96": (3, 3, 201, [[(20, 12), (10, 6), (5, 3)], [(20, 12), (10, 6), (5, 3)], [(16, 12), (8, 6), (4, 3)]]),
    "nl4_128": (3, 4, 188, [[(16, 16), (8, 8), (4, 4), (2, 2)]] * 3),
    "bench_1024": (3, 3, 203, [[(128, 128), (64, 64), (32, 32)], [(108, 108), (54, 54), (27, 27)], [(88, 88), (44, 44), (22, 22)]]),
}


def test_library_exports_the_entry():
    from yolov5_obb_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    L = C.CDLL(_lib.LIB_PATH)
    assert hasattr(L, "obb_non_max_suppression_obb_tta_head")
    assert "obb_non_max_suppression_obb_tta_head" in _lib.SIGNATURES
    text = open(os.path.join(ROOT, "include", "obb_hip.h")).read()
    assert "int obb_non_max_suppression_obb_tta_head(" in text
    from yolov5_obb_amd.models.yolo import Detect
    assert Detect.lazy_tta is False


def _pass(nl=1, flip=0, scale=1.0, img=(64, 64), conv=256, ny=8, nx=8):
    from yolov5_obb_amd import _lib
    t = _lib.TtaPass()
    t.nl, t.flip, t.scale, t.img_h, t.img_w = nl, flip, scale, img[0], img[1]
    for j in range(_lib.DETECT_MAX_LEVELS):
        t.conv_out[j], t.ny[j], t.nx[j], t.stride[j] = conv, ny, nx, 8.0
    return t


def test_argument_checks_answer_before_any_device_call():
    """Every refusal include/obb_hip.h lists for the entry is OBB_ERR_BAD_ARG.  No pointer here is memory (NULL or a small
    address) and out / out_count / status / ws are NULL: nothing can have reached a device."""
    from yolov5_obb_amd import _lib
    L = _lib.lib()
    null = C.c_void_p(0)

    def call(passes, npass=None, dtype=1, bs=2, na=3, no=5 + 16 + 180, a_total=10 ** 6, table=True):
        arr = (_lib.TtaPass * max(1, len(passes)))(*passes)
        return L.obb_non_max_suppression_obb_tta_head(len(passes) if npass is None else npass, C.cast(arr, C.c_void_p) if table else null, dtype,
                                                      bs, na, no, a_total, 0.25, 0.45, null, 0, 0, 1, 300, 30000, 4096.0, null, 0, 1024, 0,
                                                      null, 0, null, null, null, 0, null, 0, null)
    ok = _pass()
    assert call([ok], npass=0) == -1 and call([ok] * 5, npass=5) == -1 and call([ok], npass=-1) == -1      # npass out of range
    assert call([ok], table=False) == -1                                                                   # no pass table
    assert call([_pass(nl=0)]) == -1 and call([_pass(nl=5)]) == -1                                         # nl out of range
    for flip in (1, 4, -1):
        assert call([_pass(flip=flip)]) == -1                                                              # flip not in {0, 2, 3}
    for scale in (0.0, -0.5, math.inf, math.nan):
        assert call([_pass(scale=scale)]) == -1                                                            # scale <= 0 or not finite
    assert call([_pass(img=(0, 64))]) == -1 and call([_pass(img=(64, 0))]) == -1                           # image size < 1
    assert call([_pass(conv=0)]) == -1 and call([ok, _pass(nl=2, conv=0)]) == -1                           # a listed level without data
    assert call([_pass(ny=0)]) == -1 and call([_pass(nx=-3)]) == -1
    assert call([ok], na=0) == -1 and call([ok], na=9) == -1                                               # na out of range
    assert call([ok], no=5 + 180) == -1 and call([ok], no=5 + 257 + 180) == -1                             # nc out of range
    for dtype in (2, 4, -1):
        assert call([ok], dtype=dtype) == -1                                                               # unknown dtype
    assert call([ok], bs=0) == -1 and call([ok], bs=21846) == -1                                           # bs * na > 65535 (21846 * 3)
    assert call([ok], a_total=3 * 64 - 1) == -1 and call([ok], a_total=0) == -1                            # fewer rows than listed
    assert call([ok, _pass(nl=2)], a_total=3 * 64 * 3 - 1) == -1
    assert call([ok], a_total=(1 << 32) // 16 + 1) == -1                                                   # rows * nc past the key's 32-bit field
    big = _pass(nl=4, ny=46000, nx=46000)                                                                  # ny * nx * na * no past 2^31 (and the grid)
    assert call([big], a_total=1 << 40, no=186) == -1
    assert call([ok, _pass(flip=7)]) == -1                                                                 # ... in a later pass too
    # (with everything above in order the next refusal is run_nms_obb's own, still before any device call: out is NULL)
    assert call([ok]) == -1


# ---- the table builder
@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = tmp_path_factory.mktemp("thp") / "libhostttaheadplan.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", f"-I{ROOT}/yolov5_obb_amd/csrc", f"-I{ROOT}/include",
                    f"{ROOT}/tests/native/host_tta_head_plan.cpp", "-o", str(out)], check=True)
    L = C.CDLL(str(out))
    L.thp_build.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_float)]
    L.thp_build.restype = None
    L.thp_table_bytes.restype = C.c_int
    return L


def build(L, case, dtype, bs=1, scales=(1, 0.83, 0.67), flips=(None, 3, None), img=(1024, 1000), base=1 << 20, a_total=None):
    """The builder on the plan's surviving levels, conv outputs laid out back to back from the 256-byte aligned address `base`
    -> (status, entries as dicts, rows listed, tiles, plan)."""
    from yolov5_obb_amd import _lib
    from yolov5_obb_amd.models.yolo import tta_plan
    na, nl, no, maps = CASES[case]
    plan = tta_plan(maps, na, nl)
    assert plan.on_boundary
    esz = 4 if dtype == F32 else 2
    listed = [(k, p) for k, p in enumerate(plan.passes) if p.levels]
    arr = (_lib.TtaPass * len(listed))()
    rel, want = 0, []                                                  # (offsets from `base`: its misalignment is every entry's)
    for t, (k, p) in zip(arr, listed):
        t.nl, t.flip, t.scale, t.img_h, t.img_w = len(p.levels), int(flips[k] or 0), float(scales[k]), img[0], img[1]
        for j, lv in enumerate(p.levels):
            ny, nx = maps[k][lv]
            at = base + rel
            t.conv_out[j], t.ny[j], t.nx[j], t.stride[j] = at, ny, nx, 8.0 * 2 ** lv
            for a in range(na):
                t.anchors_px[j][a][0], t.anchors_px[j][a][1] = 10.0 * lv + a, 20.0 * lv + a + 0.5
            want.append(dict(k=k, lv=lv, ny=ny, nx=nx, off=p.offsets[j], ptr=at))
            rel = (rel + bs * na * no * ny * nx * esz + 255) // 256 * 256
    out, fout = (C.c_int64 * (4 + 8 * 16))(), (C.c_float * (64 + 256))()
    L.thp_build(len(arr), C.cast(arr, C.c_void_p), dtype, bs, na, no, plan.a_total if a_total is None else a_total, out, fout)
    got = [dict(a_off=out[4 + 8 * e], tile_end=out[5 + 8 * e], vec=out[6 + 8 * e], ny=out[7 + 8 * e], nx=out[8 + 8 * e], flip=out[9 + 8 * e],
                ptr=out[10 + 8 * e], inv_scale=fout[4 * e], img_w=fout[4 * e + 1], img_h=fout[4 * e + 2], stride=fout[4 * e + 3],
                anchors=list(fout[64 + 16 * e:64 + 16 * e + 16])) for e in range(16)]
    return out[0], got, out[1], out[2], out[3], want, plan


@pytest.mark.parametrize("dtype", [F32, F16, BF16], ids=["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("case", list(CASES))
def test_table_matches_tta_plan(lib, case, dtype):
    import numpy as np
    scales, flips, img = (1, 0.83, 0.67), (2, 3, None), (1024, 1000)
    rc, got, n, rows, tiles, want, plan = build(lib, case, dtype, flips=flips, img=img)
    na = CASES[case][0]
    assert rc == 0 and n == len(want) == sum(len(p.levels) for p in plan.passes) and rows == plan.a_total
    tile = 256 // (4 if dtype == F32 else 2)                           # positions per tile: one 256-byte line per channel
    end = 0
    for e, w in zip(got, want):
        end += -(-w["ny"] * w["nx"] // tile)
        assert (e["a_off"], e["ny"], e["nx"], e["ptr"], e["tile_end"]) == (w["off"], w["ny"], w["nx"], w["ptr"], end), (w, e)
        assert e["flip"] == int(flips[w["k"]] or 0) and (e["img_w"], e["img_h"]) == (1000.0, 1024.0) and e["stride"] == 8.0 * 2 ** w["lv"]
        assert e["inv_scale"] == float(np.float32(1.0 / scales[w["k"]]))                         # the reciprocal in double, rounded once
        assert e["anchors"][:2 * na] == [v for a in range(na) for v in (10.0 * w["lv"] + a, 20.0 * w["lv"] + a + 0.5)]
        assert e["anchors"][2 * na:] == [0.0] * (16 - 2 * na)
    assert tiles == end and all(e["tile_end"] == end and e["a_off"] == rows and e["vec"] == 0 for e in got[n:])
    # the last entry's rows end where the concatenation ends
    assert got[n - 1]["a_off"] + na * want[-1]["ny"] * want[-1]["nx"] == plan.a_total


@pytest.mark.parametrize("esz,dtype", [(4, F32), (2, F16), (2, BF16)], ids=["fp32", "fp16", "bf16"])
def test_vec_is_chosen_per_entry(lib, esz, dtype):
    """The load width is the entry's own: 16 bytes when the planes (ny*nx elements) are multiples of 16 bytes, 8 when of 8, else
    element-wise.  Bench shape at bs 1: only the 27 x 27 entry is element-wise; in 2-byte elements 54 x 54 and 22 x 22 (planes of
    16 k + 8 bytes) take the 8-byte loads, everything else -- the 128 x 128 maps among them -- the 16-byte loads."""
    rc, got, n, _, _, want, _ = build(lib, "bench_1024", dtype)
    assert rc == 0 and [(w["ny"]) for w in want] == [128, 64, 108, 54, 27, 44, 22]
    for e, w in zip(got, want):
        plane = w["ny"] * w["nx"] * esz
        assert e["vec"] == (16 if plane % 16 == 0 else 8 if plane % 8 == 0 else 0), (w, e["vec"])
    vec = {w["ny"]: e["vec"] for e, w in zip(got, want)}
    assert vec[27] == 0 and all(v > 0 for ny, v in vec.items() if ny != 27)
    assert vec[128] == vec[64] == vec[108] == vec[44] == 16 and vec[54] == vec[22] == (16 if esz == 4 else 8)
    # a conv output on an 8-byte (4-byte) boundary lowers (drops) the width of every entry behind it alike
    assert {e["vec"] for e in build(lib, "bench_1024", dtype, base=(1 << 20) + 8)[1][:n]} == {8, 0}
    assert {e["vec"] for e in build(lib, "bench_1024", dtype, base=(1 << 20) + 4)[1][:n]} == {0}
    # the small cases (12 x 12 and the first pass's 4 x 4 are clipped): 4 x 4 in 2-byte elements is two 16-byte pieces, 3 x 3 is element-wise
    rc, got, n, _, _, want, _ = build(lib, "nc3_128", dtype, bs=2)
    assert rc == 0 and {(w["ny"], e["vec"]) for e, w in zip(got, want)} == \
        {(16, 16), (8, 16), (4, 16), (6, 16 if esz == 4 else 8), (3, 0)}


def test_builder_refuses_what_the_entry_refuses(lib):
    assert build(lib, "bench_1024", F16, a_total=114626)[0] == -1 and build(lib, "bench_1024", F16, a_total=114627)[0] == 0
    assert build(lib, "bench_1024", 2)[0] == -1 and build(lib, "bench_1024", F16, bs=21846)[0] == -1
    assert build(lib, "bench_1024", F16, scales=(1, 0.0, 0.67))[0] == -1 and build(lib, "bench_1024", F16, flips=(None, 1, None))[0] == -1
    assert lib.thp_table_bytes() < 2048                                # with DecodeArgs well inside the 4 KB of kernel arguments


@pytest.mark.parametrize("k", range(7))
def test_the_gpu_cases_meet_their_preconditions_on_the_cpu(k):
    """The inputs of tests/test_lazy_tta_gpu.py's bit-identity cases, decoded with the oracle (fp32, CPU) and run through the
    oracle's NMS: every listed entry has candidates, every pass a kept detection, a flipped pass among them, and the NMS suppresses
    (tests/lazy_tta_cases.py preconditions).  The GPU tests assert the same on the device's own tensors in every dtype."""
    import torch
    from oracle import pyref
    from tests import lazy_tta_cases as TC
    case, scales, flips, seed = TC.IDENTITY_CASES[k]
    assert len(TC.IDENTITY_CASES) == 7
    convs = TC.heads(case, "cpu", torch.float32, seed)
    z, plan = TC.cpu_chain(case, convs, scales, flips)
    out = pyref.non_max_suppression_obb(z.clone(), **TC.KW)
    n_cand, n_kept, from_pass = TC.preconditions(z, plan, out, flips, TC.KW["conf_thres"], 3, TC.CASES[case][5])
    print(case, flips, "candidates", n_cand, "kept", n_kept, "per pass", from_pass)
