"""CPU: the PRODUCT's tile-merge arithmetic (yolov5_obb_amd/csrc/tile_merge_math.h) compiled with g++ behind array drivers
(tests/native/host_tile_merge_math.cpp) and held to Python, bit for bit.

round_dec1 / round_dec5 restate what the reference's text hand-off does to a float32: val.py:63-65 round(x, 1) / round(score, 5)
of the widened value, '%s' in tools/TestJson2VocClassTxt.py:45, float() in ResultMerge_multi_process.py:207 -- that is
float(str(round(float(np.float32(v)), d))).  to_source is poly2origpoly (:175-182): float(v + off) / float(rate)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tm(tmp_path_factory):
    out = tmp_path_factory.mktemp("tm") / "libhosttilemerge.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", f"-I{ROOT}/yolov5_obb_amd/csrc",
                    f"{ROOT}/tests/native/host_tile_merge_math.cpp", "-o", str(out), "-lm"], check=True)
    L = C.CDLL(str(out))
    f32 = np.ctypeslib.ndpointer(dtype=np.float32, flags="C_CONTIGUOUS")
    f64 = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
    i32 = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")
    u64 = np.ctypeslib.ndpointer(dtype=np.uint64, flags="C_CONTIGUOUS")
    L.hc_round_dec.argtypes, L.hc_round_dec.restype = [f32, C.c_long, C.c_int, f64], None
    L.hc_to_source.argtypes, L.hc_to_source.restype = [f64, i32, C.c_long, C.c_double, f64], None
    L.hc_class_of.argtypes, L.hc_class_of.restype = [f32, C.c_long, C.c_int, i32], None
    L.hc_sort_key.argtypes, L.hc_sort_key.restype = [i32, f32, C.c_long, C.c_int, u64], None
    return L


def round_dec(L, v, d):
    v = np.ascontiguousarray(v, dtype=np.float32)
    out = np.empty(len(v), dtype=np.float64)
    L.hc_round_dec(v, len(v), d, out)
    return out


def py_round(v, d):
    return np.array([float(str(round(float(x), d))) for x in np.asarray(v, dtype=np.float32)], dtype=np.float64)


def same_bits(got, want):
    bad = np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))
    assert bad.size == 0, (bad.size, "first", int(bad[0]), got[bad[0]], want[bad[0]])


def around(values, ulps=2):
    """every float32 within `ulps` of each value (float32-rounded), both signs"""
    c = np.asarray(values, dtype=np.float64).astype(np.float32)
    out = [c]
    lo = hi = c
    for _ in range(ulps):
        lo, hi = np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))
        out += [lo, hi]
    a = np.concatenate(out)
    return np.concatenate([a, -a])


@pytest.mark.parametrize("d", [1, 5])
def test_round_equals_python_on_a_million_values(tm, d):
    v = np.random.RandomState(20 + d).uniform(-2e4, 2e4, 1_000_000).astype(np.float32)
    same_bits(round_dec(tm, v, d), py_round(v, d))


@pytest.mark.parametrize("d", [1, 5])
def test_round_equals_python_at_the_halves_of_a_decimal(tm, d):
    """k / 20 is a tie of round(x, 1): the float32 values at and next to it land on both sides, and the exact ones (k / 20 with
    k a multiple of 5: x.25, x.75) are ties in binary too -- half to even."""
    v = around(np.arange(4001) / 20.0)
    same_bits(round_dec(tm, v, d), py_round(v, d))


@pytest.mark.parametrize("d", [1, 5])
def test_round_special_values(tm, d):
    v = np.array([0.0, -0.0, -0.04, 0.25, 0.75, 2.5, -0.25, 0.05, 0.15, 0.35, 1e-7, -1e-7, 4e-6, 5e-6, -4e-6], dtype=np.float32)
    got = round_dec(tm, v, d)
    same_bits(got, py_round(v, d))
    if d == 1:
        assert np.signbit(got[1]) and np.signbit(got[2]) and got[2] == 0.0, "round(-0.04, 1) is -0.0"
        assert got[3:6].tolist() == [0.2, 0.8, 2.5]


def test_round_dec5_equals_python_at_the_halves_of_a_score(tm):
    k = np.random.RandomState(7).choice(100000, size=1000, replace=False)
    v = around((2 * k + 1) / 2e5)
    same_bits(round_dec(tm, v, 5), py_round(v, 5))
    v = np.random.RandomState(8).uniform(0, 1, 200000).astype(np.float32)          # confidences
    same_bits(round_dec(tm, v, 5), py_round(v, 5))


@pytest.mark.parametrize("rate", [0.5, 1.0, 1.5])
def test_to_source_equals_python(tm, rate):
    rng = np.random.RandomState(3)
    v = np.concatenate([py_round(rng.uniform(-300, 1400, 20000), 1), [0.0, -0.0, 1023.9, -0.1]])
    off = np.concatenate([rng.choice([0, 476, 824, 976, 3072, 20000], size=20000), [0, 0, 976, 0]]).astype(np.int32)
    got = np.empty(len(v))
    tm.hc_to_source(v, off, len(v), rate, got)
    want = np.array([float(float(a) + int(o)) / float(str(rate)) for a, o in zip(v, off)])          # poly2origpoly on the parsed line
    same_bits(got, want)


def test_class_of_accepts_only_integers_below_nc(tm):
    v = np.array([0.0, -0.0, 1.0, 2.0, 3.0, 3.5, -1.0, 0.5, np.nan, np.inf, 2.9999998, 255.0, 256.0], dtype=np.float32)
    out = np.empty(len(v), dtype=np.int32)
    tm.hc_class_of(v, len(v), 3, out)
    assert out.tolist() == [0, 0, 1, 2, -1, -1, -1, -1, -1, -1, -1, -1, -1]
    tm.hc_class_of(v, len(v), 256, out)
    assert out.tolist() == [0, 0, 1, 2, 3, -1, -1, -1, -1, -1, -1, 255, -1]


def test_sort_key_orders_by_segment_then_printed_score_descending(tm):
    """Text rounding: scores that print alike share a key, others order by the printed value, descending; without it the
    float's own order.  The segment is the high word."""
    rng = np.random.RandomState(11)
    conf = np.concatenate([rng.uniform(0, 1, 5000), around([0.5, 0.123455, 0.9]), [0.0, -0.0, 1.0]]).astype(np.float32)
    seg = rng.randint(0, 7, len(conf)).astype(np.int32)
    key = np.empty(len(conf), dtype=np.uint64)
    tm.hc_sort_key(seg, conf, len(conf), 1, key)
    printed = py_round(conf, 5)
    assert np.array_equal(key >> np.uint64(32), seg.astype(np.uint64))
    low = (key & np.uint64(0xffffffff)).astype(np.int64)
    order = np.argsort(low, kind="stable")
    assert np.all(np.diff(printed[order]) <= 0), "ascending key = descending printed score"
    assert np.array_equal(low[:, None] == low[None, :5], printed[:, None] == printed[None, :5]), "equal keys = equal printed scores"
    tm.hc_sort_key(seg, conf, len(conf), 0, key)
    low = (key & np.uint64(0xffffffff)).astype(np.int64)
    order = np.argsort(low, kind="stable")
    assert np.all(np.diff(conf[order].astype(np.float64)) <= 0)
    assert np.array_equal(low[:, None] == low[None, -8:], conf[:, None] == conf[None, -8:]), "equal keys = equal floats (-0 == +0)"
