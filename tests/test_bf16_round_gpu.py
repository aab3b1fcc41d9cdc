"""GPU: the float <-> bf16 element access of the kernels (csrc/dtype_device.h: st_from_float, round_to_dtype, ld_as_float for
bf16_t) as the gfx950 device code runs it -- the hardware's packed conversion -- on the pattern set of
tests/test_bf16_round_host.py: all 65,536 upper halves times the lower halves {0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF}
(subnormals, +-0, +-inf, every NaN payload class, the overflow boundary).  Bit-equal to torch's c10::BFloat16 on the CPU and
to the host build of csrc/bf16_bits.h; a NaN need only be a NaN.  The device code is tests/native/dev_bf16_round.hip, built by
csrc/Makefile (build()) with the library's flags."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests.test_bf16_round_host import _is_nan16, _patterns, hb  # noqa: F401  (hb: the host build of the same header)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "tests", "native", "dev_bf16_round.so")


@pytest.fixture(scope="module")
def probe():
    assert os.path.exists(PROBE), "tests/native/dev_bf16_round.so is not built (python __graft_entry__.py, or make -C yolov5_obb_amd/csrc)"
    L = C.CDLL(PROBE)
    L.probe_bf16_round.argtypes = [C.c_void_p, C.c_long, C.c_void_p, C.c_void_p, C.c_void_p]
    L.probe_bf16_widen.argtypes = [C.c_void_p, C.c_long, C.c_void_p, C.c_void_p]
    return L


def test_device_rounding_matches_torch_and_the_host_function(dev, probe, hb):
    from yolov5_obb_amd import _lib
    pat = _patterns()
    x = torch.from_numpy(pat.view(np.int32)).view(torch.float32)
    want = x.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    host = np.zeros(pat.size, np.uint16)
    hb.hb_round(pat, pat.size, host)
    xd = x.to(dev)
    stored = torch.zeros(pat.size, dtype=torch.int16, device=dev)
    rounded = torch.zeros(pat.size, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        assert probe.probe_bf16_round(xd.data_ptr(), pat.size, stored.data_ptr(), rounded.data_ptr(), _lib.stream_ptr(dev)) == 0
    torch.cuda.synchronize(dev)
    got = stored.cpu().numpy().view(np.uint16)
    rbits = rounded.cpu().view(torch.int32).numpy().view(np.uint32)
    nan_in = (pat & 0x7FFFFFFF) > 0x7F800000
    assert np.array_equal(_is_nan16(got), nan_in), "NaN in <=> NaN out"
    fin = ~nan_in
    for name, ref in (("torch", want), ("host function", host)):
        bad = np.nonzero(got[fin] != ref[fin])[0]
        assert bad.size == 0, (name, bad.size, [(hex(int(pat[fin][i])), hex(int(got[fin][i])), hex(int(ref[fin][i]))) for i in bad[:8]])
    # round_to_dtype is the stored value widened: the upper half, a zero lower half
    assert np.array_equal(rbits[fin], got[fin].astype(np.uint32) << 16)
    assert ((rbits[nan_in] & 0x7FFFFFFF) > 0x7F800000).all()


def test_device_widening_load_is_exact(dev, probe):
    from yolov5_obb_amd import _lib
    bits = np.arange(1 << 16, dtype=np.uint16)
    bd = torch.from_numpy(bits.view(np.int16)).to(dev)
    out = torch.zeros(bits.size, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        assert probe.probe_bf16_widen(bd.data_ptr(), bits.size, out.data_ptr(), _lib.stream_ptr(dev)) == 0
    torch.cuda.synchronize(dev)
    got = out.cpu().view(torch.int32).numpy().view(np.uint32)
    nan = _is_nan16(bits)
    assert np.array_equal(got[~nan], bits[~nan].astype(np.uint32) << 16)
    assert ((got[nan] & 0x7FFFFFFF) > 0x7F800000).all()
