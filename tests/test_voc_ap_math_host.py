"""CPU: the PRODUCT's VOC AP arithmetic (yolov5_obb_amd/csrc/voc_ap_math.h) compiled with g++ behind array drivers
(tests/native/host_voc_ap_math.cpp) and held to numpy on this machine, bit for bit: the chunked pairwise sum against np.sum,
both AP metrics against the package's voc_ap (the literal restatement of dota_evaluation_task1.py:54-86), the curve arithmetic
against voc_eval's statements.  The same program, built with -fsanitize=address,undefined, runs once on its own main()."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = f"{ROOT}/tests/native/host_voc_ap_math.cpp"
FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off", f"-I{ROOT}/yolov5_obb_amd/csrc"]


@pytest.fixture(scope="module")
def va(tmp_path_factory):
    out = tmp_path_factory.mktemp("va") / "libhostvocap.so"
    subprocess.run(["g++", *FLAGS, "-fPIC", "-shared", SRC, "-o", str(out), "-lm"], check=True)
    L = C.CDLL(str(out))
    f64 = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
    i64 = np.ctypeslib.ndpointer(dtype=np.int64, flags="C_CONTIGUOUS")
    u64 = np.ctypeslib.ndpointer(dtype=np.uint64, flags="C_CONTIGUOUS")
    L.hc_np_sum.argtypes, L.hc_np_sum.restype = [f64, C.c_long], C.c_double
    L.hc_ap11.argtypes, L.hc_ap11.restype = [f64, f64, C.c_long], C.c_double
    L.hc_ap_all.argtypes, L.hc_ap_all.restype = [f64, f64, C.c_long], C.c_double
    L.hc_curve.argtypes, L.hc_curve.restype = [i64, i64, C.c_long, C.c_longlong, f64, f64], None
    L.hc_score_key.argtypes, L.hc_score_key.restype = [f64, C.c_long, u64], None
    L.hc_index_of.argtypes, L.hc_index_of.restype = [f64, C.c_long, C.c_longlong, i64], None
    return L


def voc_ap(rec, prec, m07):
    from yolov5_obb_amd.DOTA_devkit.dota_evaluation_task1 import voc_ap as f
    with np.errstate(all="ignore"):
        return float(f(rec, prec, m07))


def same(a, b):
    """bit equality, any NaN equal to any NaN"""
    a, b = np.float64(a), np.float64(b)
    return (np.isnan(a) and np.isnan(b)) or a.tobytes() == b.tobytes()


def curve(n, npos, seed, p_tp=0.5):
    """(tp, fp) inclusive counts of n detections, and voc_eval's own rec / prec (:235-241)"""
    rng = np.random.RandomState(seed)
    hit = rng.rand(n) < p_tp
    tp, fp = np.cumsum(hit.astype(np.float64)), np.cumsum((~hit).astype(np.float64))
    with np.errstate(all="ignore"):
        rec = tp / float(npos)
        prec = tp / np.maximum(tp + fp, np.finfo(np.float64).eps)
    return tp.astype(np.int64), fp.astype(np.int64), rec, prec


@pytest.mark.parametrize("n", [0, 1, 7, 8, 9, 127, 128, 129, 257, 1000, 8192, 8193, 16385, 100003])
def test_sum_equals_np_sum(va, n):
    rng = np.random.RandomState(n % 1000 + 5)
    for trial in range(3):
        a = rng.randn(n) * 10.0 ** rng.randint(-12, 13, n)           # mixed magnitudes: every grouping rounds differently
        a = np.ascontiguousarray(a)
        assert same(va.hc_np_sum(a, n), np.sum(a)), (n, trial)
    a = np.full(n, -0.0)
    assert same(va.hc_np_sum(a, n), np.sum(a))


@pytest.mark.parametrize("n,npos,p_tp", [(0, 5, 0.5), (1, 1, 1.0), (1, 1, 0.0), (40, 13, 0.4), (500, 0, 0.5), (500, 0, 0.0), (300, 1000, 0.0),
                                        (3000, 900, 0.3), (20000, 12000, 0.6), (30000, 40000, 0.95), (30000, 100, 0.9)])
def test_both_metrics_equal_voc_ap(va, n, npos, p_tp):
    """empty curves; npos = 0 (NaN / inf recalls); a recall that never moves (no true positive); more than 8192 recall steps
    (the last two: ~12000 and ~28000 kept terms); recalls above 1 (more true positives than npos)."""
    tp, fp, rec, prec = curve(n, npos, 11 * n + npos, p_tp)
    r2, p2 = np.empty(n), np.empty(n)
    va.hc_curve(tp, fp, n, npos, r2, p2)
    assert np.array_equal(r2.view(np.uint64) | (np.isnan(r2) * np.uint64(0xffffffffffffffff)),
                          rec.view(np.uint64) | (np.isnan(rec) * np.uint64(0xffffffffffffffff)))
    assert p2.tobytes() == prec.tobytes()
    if n >= 20000:
        assert np.count_nonzero(np.diff(rec)) > 8192
    got11, want11 = va.hc_ap11(rec, prec, n), voc_ap(rec, prec, True)
    gota, wanta = va.hc_ap_all(rec, prec, n), voc_ap(rec, prec, False)
    assert same(got11, want11), (got11, want11)
    assert same(gota, wanta), (gota, wanta)


def test_nan_precision_propagates_like_numpy(va):
    rec = np.array([0.1, 0.2, 0.2, 0.5, np.nan, 0.9])
    prec = np.array([1.0, np.nan, 0.7, 0.6, 0.5, 0.4])
    for m07, f in ((True, va.hc_ap11), (False, va.hc_ap_all)):
        assert same(f(rec, prec, 6), voc_ap(rec, prec, m07))
    prec = np.array([1.0, 0.9, 0.7, 0.6, 0.5, 0.4])
    for m07, f in ((True, va.hc_ap11), (False, va.hc_ap_all)):
        assert same(f(rec, prec, 6), voc_ap(rec, prec, m07))


def test_score_key_is_argsort_of_the_negated_score_with_stable_ties(va):
    s = np.concatenate([np.random.RandomState(3).randn(500), [0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan, 1e-310, -1e-310, 0.5, 0.5]])
    key = np.empty(len(s), dtype=np.uint64)
    va.hc_score_key(s, len(s), key)
    assert np.array_equal(np.argsort(key, kind="stable"), np.argsort(-s, kind="stable"))


def test_index_of_accepts_only_integers_below_the_limit(va):
    v = np.array([0.0, -0.0, 1.0, 2.0, 2.5, -1.0, np.nan, np.inf, 3.0, 2.9999999999999996, 4294967296.0])
    out = np.empty(len(v), dtype=np.int64)
    va.hc_index_of(v, len(v), 3, out)
    assert out.tolist() == [0, 0, 1, 2, -1, -1, -1, -1, -1, -1, -1]


def test_standalone_program_under_address_and_undefined_sanitizers(tmp_path):
    exe = tmp_path / "host_voc_ap_math_san"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", f"-I{ROOT}/yolov5_obb_amd/csrc", SRC, "-o", str(exe), "-lm"], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "host_voc_ap_math ok" in out.stdout, (out.stdout[-400:], out.stderr[-2000:])
