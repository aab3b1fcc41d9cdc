"""CPU: the workspace cursor every C-ABI layout is written on (yolov5_obb_amd/csrc/ws_layout.h), compiled with g++ behind a
serial driver (tests/native/host_ws_layout.cpp).  A sizing pass (NULL base) and a placing pass over the same takes agree on the
total; the sizing pass hands out only NULL; the placing pass hands out consecutive 256-byte blocks in the order of the takes,
each large enough, none overlapping, the last inside total(); a nested layout lies where it was placed; ws_ok is the refusal
rule of include/obb_hip.h (NULL, misaligned, short)."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (element size, count): every typed size of the driver, the untyped form (3, 7, 24), counts of 0 and 1, exact multiples of 256
TAKES = [(8, 100), (4, 0), (16, 1), (1, 257), (2, 64), (3, 85), (4, 1), (8, 0), (16, 33), (4, 64), (1, 256), (7, 1), (24, 11), (1, 1)]
NESTS = [(0, 0), (4, 8), (0, 3), (11, 14), (0, 14), (5, 6)]          # [lo, hi) of the takes that form the nested layout


@pytest.fixture(scope="module")
def wl(tmp_path_factory):
    out = tmp_path_factory.mktemp("wl") / "libhostwslayout.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", f"-I{ROOT}/yolov5_obb_amd/csrc",
                    f"{ROOT}/tests/native/host_ws_layout.cpp", "-o", str(out)], check=True)
    L = C.CDLL(str(out))
    L.wl_run.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p),
                         C.POINTER(C.c_uint64)]
    L.wl_run.restype = None
    L.wl_ok.argtypes, L.wl_ok.restype = [C.c_void_p, C.c_uint64, C.c_uint64], C.c_int
    L.wl_align_up.argtypes, L.wl_align_up.restype = [C.c_uint64], C.c_uint64
    return L


def run(L, base, takes, nest):
    n = len(takes)
    es, cn = (C.c_int64 * n)(*[t[0] for t in takes]), (C.c_int64 * n)(*[t[1] for t in takes])
    ptrs, totals = (C.c_void_p * n)(*[1] * n), (C.c_uint64 * 2)()
    L.wl_run(base, es, cn, n, nest[0], nest[1], ptrs, totals)
    return [p or 0 for p in ptrs], int(totals[0]), int(totals[1])


def aligned(buf):
    return (C.addressof(buf) + 255) & ~255


@pytest.mark.parametrize("nest", NESTS)
def test_sizing_and_placing_passes_agree(wl, nest):
    sized, total, inner = run(wl, None, TAKES, nest)
    assert sized == [0] * len(TAKES), "a sizing pass hands out only NULL"
    assert total > 0 and total % 256 == 0 and inner % 256 == 0
    buf = C.create_string_buffer(total + 256)
    base = aligned(buf)
    ptrs, total2, inner2 = run(wl, base, TAKES, nest)
    assert (total2, inner2) == (total, inner)
    end = base
    for (esize, count), p in zip(TAKES, ptrs):
        assert (p - base) % 256 == 0 and p >= base, "every pointer is base + k * 256"
        assert p == end, "blocks come in the order of the takes, each right behind the one before"
        end = p + max(256, -(-esize * count // 256) * 256)          # an empty take is still one block
        assert end >= p + esize * count
    assert end == base + total, "the last block ends at total()"
    if nest[1] > nest[0]:
        assert inner == sum(max(256, -(-e * c // 256) * 256) for e, c in TAKES[nest[0]:nest[1]])
    # the same takes without the nesting: the nested layout lies where its blocks would have been
    assert run(wl, base, TAKES, (0, 0))[:2] == (ptrs, total)


def test_blocks_do_not_depend_on_the_base(wl):
    _, total, _ = run(wl, None, TAKES, (4, 8))
    buf = C.create_string_buffer(total + 1024)
    a = aligned(buf)
    pa, pb = run(wl, a, TAKES, (4, 8))[0], run(wl, a + 512, TAKES, (4, 8))[0]
    assert [p - a for p in pa] == [p - a - 512 for p in pb]


def test_empty_layout_and_align_up(wl):
    assert run(wl, None, [], (0, 0))[1] == 0
    assert [wl.wl_align_up(v) for v in (0, 1, 255, 256, 257, 512)] == [0, 256, 256, 256, 512, 512]
    assert run(wl, None, [(4, 0)], (0, 0))[1] == 256 and run(wl, None, [(4, 1)], (0, 0))[1] == 256
    assert run(wl, None, [(4, 64)], (0, 0))[1] == 256 and run(wl, None, [(4, 65)], (0, 0))[1] == 512


def test_ws_ok_is_the_refusal_rule(wl):
    need = run(wl, None, TAKES, (0, 0))[1]
    buf = C.create_string_buffer(need + 512)
    base = aligned(buf)
    assert wl.wl_ok(None, need, need) == 0
    assert wl.wl_ok(base + 8, need, need) == 0 and wl.wl_ok(base + 128, need, need) == 0
    assert wl.wl_ok(base, need - 1, need) == 0
    assert wl.wl_ok(base, need, need) == 1 and wl.wl_ok(base, need + 1, need) == 1
    assert wl.wl_ok(base + 256, need, need) == 1
