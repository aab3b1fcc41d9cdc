"""CPU: the PRODUCT's float <-> bf16 conversions (yolov5_obb_amd/csrc/bf16_bits.h, what every kernel that reads a bf16 Detect
head calls to widen, round and store an element) compiled with g++ and compared bit for bit with torch's c10::BFloat16.

Pattern set of the rounding: all 65,536 upper halves of a float times the lower halves {0x0000, 0x0001, 0x7FFF, 0x8000,
0x8001, 0xFFFF} -- exact values, just above, just below and exactly on the tie (with even and odd kept halves), just above
the tie, and the largest dropped half: 393,216 patterns, among them subnormals, +-0, +-inf, every NaN payload class and the
overflow boundary 0x7F7F8000 (the first finite float that rounds to inf).  Equality is exact; a NaN need only be a NaN."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOWER = (0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF)


@pytest.fixture(scope="module")
def hb(tmp_path_factory):
    out = tmp_path_factory.mktemp("hb") / "libhostbf16.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", f"-I{ROOT}/yolov5_obb_amd/csrc",
                    f"{ROOT}/tests/native/host_bf16_round.cpp", "-o", str(out)], check=True)
    L = C.CDLL(str(out))
    L.hb_round.argtypes = [np.ctypeslib.ndpointer(dtype=np.uint32, flags="C_CONTIGUOUS"), C.c_long,
                           np.ctypeslib.ndpointer(dtype=np.uint16, flags="C_CONTIGUOUS")]
    L.hb_widen.argtypes = [np.ctypeslib.ndpointer(dtype=np.uint16, flags="C_CONTIGUOUS"), C.c_long,
                           np.ctypeslib.ndpointer(dtype=np.uint32, flags="C_CONTIGUOUS")]
    return L


def _patterns():
    upper = np.arange(1 << 16, dtype=np.uint32) << 16
    return np.ascontiguousarray(np.concatenate([upper | np.uint32(lo) for lo in LOWER]))


def _is_nan16(bits):
    return (bits & 0x7FFF) > 0x7F80


def test_round_to_bf16_matches_torch_on_the_pattern_set(hb):
    pat = _patterns()
    assert pat.size == 393216
    got = np.zeros(pat.size, np.uint16)
    hb.hb_round(pat, pat.size, got)
    x = torch.from_numpy(pat.view(np.int32)).view(torch.float32)
    want = x.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    nan_in = (pat & 0x7FFFFFFF) > 0x7F800000
    assert np.array_equal(_is_nan16(want), nan_in)                  # (the reference side: NaN stays NaN, nothing else becomes one)
    assert np.array_equal(_is_nan16(got), nan_in), "NaN in <=> NaN out"
    assert (got[nan_in] & 0x0040).all(), "a NaN result is quiet"
    fin = ~nan_in
    bad = np.nonzero(got[fin] != want[fin])[0]
    assert bad.size == 0, [(hex(int(pat[fin][i])), hex(int(got[fin][i])), hex(int(want[fin][i]))) for i in bad[:8]]
    # the named corners, spelled out
    def one(u):
        o = np.zeros(1, np.uint16)
        hb.hb_round(np.array([u], np.uint32), 1, o)
        return int(o[0])
    assert one(0x7F800000) == 0x7F80 and one(0xFF800000) == 0xFF80          # +-inf stay
    assert one(0x7F7F7FFF) == 0x7F7F and one(0x7F7F8000) == 0x7F80          # the overflow boundary: largest finite / inf
    assert one(0xFF7FFFFF) == 0xFF80                                        # -FLT_MAX rounds to -inf
    assert one(0x00000000) == 0x0000 and one(0x80000000) == 0x8000          # +-0
    assert one(0x00008000) == 0x0000 and one(0x00018000) == 0x0002          # subnormal ties go to even
    assert one(0x3F808000) == 0x3F80 and one(0x3F818000) == 0x3F82          # ties to even on normal values
    assert one(0x3E80C49C) == 0x3E81                                      # 0.2515f -> 0.251953125 (the threshold-edge case)


def test_widening_load_is_exact_on_every_bf16_value(hb):
    bits = np.arange(1 << 16, dtype=np.uint16)
    got = np.zeros(bits.size, np.uint32)
    hb.hb_widen(bits, bits.size, got)
    want = torch.from_numpy(bits.view(np.int16)).view(torch.bfloat16).float().view(torch.int32).numpy().view(np.uint32)
    nan = _is_nan16(bits)
    assert np.array_equal(got[~nan], want[~nan])
    assert ((got[nan] & 0x7FFFFFFF) > 0x7F800000).all() and ((want[nan] & 0x7FFFFFFF) > 0x7F800000).all()
    assert np.array_equal(got, bits.astype(np.uint32) << 16)                # the value's own bits, payloads included
    # round(widen(h)) == h for every non-NaN h: rounding a value that is already bf16 changes nothing
    back = np.zeros(bits.size, np.uint16)
    hb.hb_round(got, got.size, back)
    assert np.array_equal(back[~nan], bits[~nan])
