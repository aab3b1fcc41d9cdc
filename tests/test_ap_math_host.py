"""CPU: the PRODUCT's ap_per_class arithmetic (yolov5_obb_amd/csrc/ap_math.h) compiled with g++ behind a serial driver
(tests/native/host_ap_math.cpp) and compared with the reference's numpy on every golden case with n <= 4097
(tests/golden/ap_cases.npz: the reference's own ap_per_class with np.argsort pinned to kind='stable').

Counts, classes and the best index are equal exactly; ap, p, r, f1 within 1e-12 absolute: each is a double in [0, 1] built from
exact integer counts by fewer than ~200 roundings (<= 2e-14)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import ap_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NC_MAX = 256
TOL = 1e-12


@pytest.fixture(scope="module")
def ha(tmp_path_factory):
    out = tmp_path_factory.mktemp("ha") / "libhostap.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", f"-I{ROOT}/yolov5_obb_amd/csrc",
                    f"{ROOT}/tests/native/host_ap_math.cpp", "-o", str(out), "-lm"], check=True)
    L = C.CDLL(str(out))
    f32 = np.ctypeslib.ndpointer(dtype=np.float32, flags="C_CONTIGUOUS")
    f64 = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
    i32 = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")
    u8 = np.ctypeslib.ndpointer(dtype=np.uint8, flags="C_CONTIGUOUS")
    L.hc_ap_per_class.argtypes = [u8, f32, f32, C.c_long, C.c_int, f32, C.c_long, C.c_int, f64, f64, i32, i32]
    L.hc_ap_per_class.restype = C.c_int
    return L


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "ap_cases.npz"))


def host_ap_per_class(L, tp, conf, pred_cls, target_cls):
    n, niou = tp.shape
    ap = np.zeros((NC_MAX, niou))
    prf = np.zeros((NC_MAX, 5))
    counts = np.zeros((2, NC_MAX), np.int32)
    info = np.zeros(4, np.int32)
    rc = L.hc_ap_per_class(np.ascontiguousarray(tp, dtype=np.uint8), conf, pred_cls, n, niou, target_cls, len(target_cls), NC_MAX,
                           ap, prf, counts, info)
    assert rc == 0
    keep = np.flatnonzero(counts[0] > 0)
    return (prf[keep, 3], prf[keep, 4], prf[keep, 0], prf[keep, 1], prf[keep, 2], ap[keep], keep.astype(np.int32)), int(info[0])


HOST_CASES = [k for k, v in ap_cases.CASES.items() if v["n"] <= ap_cases.HOST_MAX_N and v.get("m", 1) > 0]


@pytest.mark.parametrize("name", HOST_CASES)
def test_host_ap_math_matches_the_reference(ha, golden, name):
    got, best = host_ap_per_class(ha, *ap_cases.build(name))
    want = [golden[f"{name}/{k}"] for k in ("tp", "fp", "p", "r", "f1", "ap", "classes")]
    assert np.array_equal(got[6], want[6]) and got[6].dtype == want[6].dtype
    assert best == int(golden[f"{name}/best"])
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    for g, w, what in zip(got[2:6], want[2:6], ("p", "r", "f1", "ap")):
        assert g.shape == w.shape and np.abs(g - w).max(initial=0.0) <= TOL, (what, np.abs(g - w).max(initial=0.0))


def test_interpolation_points_are_linspace_bits(ha):
    """ap_x / pr_x are np.linspace(0, 1, 101) / np.linspace(0, 1, 1000) bit for bit (10 of the 101 differ from k / 100)."""
    src = ('#include "ap_math.h"\nextern "C" void grids(double* a, double* p) { for (int k = 0; k < 101; k++) a[k] = obb::apm::ap_x(k); '
           'for (int k = 0; k < 1000; k++) p[k] = obb::apm::pr_x(k); }\n')
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "g.cpp"), "w").write(src)
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", f"-I{ROOT}/yolov5_obb_amd/csrc",
                        os.path.join(d, "g.cpp"), "-o", os.path.join(d, "g.so")], check=True)
        G = C.CDLL(os.path.join(d, "g.so"))
        a, p = np.zeros(101), np.zeros(1000)
        f64 = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
        G.grids.argtypes = [f64, f64]
        G.grids(a, p)
    assert np.array_equal(a, np.linspace(0, 1, 101)) and np.array_equal(p, np.linspace(0, 1, 1000))
