"""CPU: which state of the later launches a call of the fused driver has its first kernel zero (yolov5_obb_amd/csrc/nms_plan.h:
ObbPlan::zero_bar / zero_alive), over every path case of tests/test_nms_plan_host.py.  The rule is stated here from what the launches
of a path READ, not from the header: the barrier block (which holds the abort flag) is read by the persistent kernel and by
k_gather_out; zeroed alive words are what k_sort_prep_lds ORs its bits into (self-sorting segments keep theirs in LDS, the radix-sort
path clears the bitmap itself in front of k_prep_cand)."""
import ctypes as C
import os
import subprocess

import pytest

from tests.test_nms_plan_host import OBB, OBB_IN, env8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = ["lds_sort", "small_nms", "self_sort", "fused_out", "zero_bar", "zero_alive"]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = tmp_path_factory.mktemp("npz") / "libhostnmsplanzero.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", f"-I{ROOT}/yolov5_obb_amd/csrc", f"-I{ROOT}/include",
                    f"{ROOT}/tests/native/host_nms_plan_zero.cpp", "-o", str(out)], check=True)
    L = C.CDLL(str(out))
    L.npz_obb.argtypes, L.npz_obb.restype = [C.POINTER(C.c_int64), C.c_float, C.c_float, C.POINTER(C.c_int), C.POINTER(C.c_int64)], None
    return L


def plan(L, name):
    i, env = OBB[name]
    out = (C.c_int64 * 6)()
    L.npz_obb((C.c_int64 * 16)(*[i[k] for k in OBB_IN]), i["iou_thres"], i["max_wh"], env8(env), out)
    return dict(zip(OUT, list(out)))


@pytest.mark.parametrize("name", list(OBB))
def test_a_call_zeroes_what_its_path_reads(lib, name):
    p = plan(lib, name)
    persistent_kernel = not p["small_nms"]
    gather_launch = not p["fused_out"]
    sort_prep_lds = p["lds_sort"] and not p["self_sort"]
    assert p["zero_bar"] == int(persistent_kernel or gather_launch)
    assert p["zero_alive"] == int(bool(sort_prep_lds))


def test_expected_values(lib):
    z = lambda name: (plan(lib, name)["zero_bar"], plan(lib, name)["zero_alive"])
    assert z("the bench shape") == (0, 0)                  # the filter and k_nms_small<SmallGather, SmallSelfSort>: neither block is read
    assert z("SELF_SORT=0") == (0, 1)                      # k_sort_prep_lds in front of k_nms_small
    assert z("out_packed") == (1, 1)                       # k_gather_out reads the abort flag
    assert z("seg_hint one above") == (1, 1)               # k_sort_prep_lds + the persistent kernel
    assert z("un-hinted first call: radix") == (1, 0)      # the persistent kernel behind the radix sort (which clears the bitmap itself)
    assert z("agnostic") == (1, 1)
    assert z("nc == 1") == (1, 1)
