"""CPU: the head-layout switch of ComputeLoss's C ABI (obb_loss_config.head_layout, include/obb_hip.h) and the helper of
yolov5_obb_amd/utils/loss.py that recognises the permuted view of a conv output (Detect.lazy_train).

  * _LossConfig (ctypes) is obb_loss_config as the compiler lays it out (tests/native/host_loss_layout.cpp, g++);
  * head_layout outside {0, 1}: the workspace query answers 0 and the four entries answer OBB_ERR_BAD_ARG before any device
    call (they are handed ws = NULL, so an entry that let the value pass would answer OBB_ERR_WORKSPACE, not follow a pointer);
  * is_conv_view on CPU tensors: the exact view, a contiguous copy, channels-last, a storage offset, 1x1 grids, a wrong
    permutation."""
import ctypes as C
import os
import subprocess

import pytest
import torch

from yolov5_obb_amd import _lib
from yolov5_obb_amd.utils.loss import LAYOUT_CONV, LAYOUT_ROWS, _LossConfig, is_conv_view

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ll(tmp_path_factory):
    out = tmp_path_factory.mktemp("ll") / "libhostlosslayout.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", f"-I{ROOT}/include", f"{ROOT}/tests/native/host_loss_layout.cpp",
                    "-o", str(out)], check=True)
    L = C.CDLL(str(out))
    for f in ("ll_sizeof_config", "ll_offsetof_head_layout", "ll_offsetof_fl_gamma"):
        getattr(L, f).restype = C.c_ulonglong
    return L


def config(layout):
    cfg = _LossConfig()
    cfg.nl, cfg.na, cfg.nc, cfg.no, cfg.bs = 2, 3, 2, 187, 2
    for i, (ny, nx) in enumerate(((3, 5), (1, 1))):
        cfg.ny[i], cfg.nx[i], cfg.stride[i], cfg.balance[i] = ny, nx, 8.0 * (i + 1), 1.0
        for a in range(3):
            cfg.anchors[i][a][0], cfg.anchors[i][a][1] = 2.0 + a, 1.0 + a
    cfg.anchor_t = 4.0
    cfg.head_layout = layout
    return cfg


def test_ctypes_mirror_is_the_header_struct(ll):
    assert C.sizeof(_LossConfig) == ll.ll_sizeof_config()
    assert _LossConfig.head_layout.offset == ll.ll_offsetof_head_layout()
    assert _LossConfig.fl_gamma.offset == ll.ll_offsetof_fl_gamma() == _LossConfig.head_layout.offset - 4, "appended behind fl_gamma"
    assert _LossConfig._fields_[-1][0] == "head_layout"
    assert (LAYOUT_ROWS, LAYOUT_CONV) == (ll.ll_layout_rows(), ll.ll_layout_conv()) == (0, 1)
    assert _LossConfig().head_layout == LAYOUT_ROWS, "a zero-initialised config is the row layout"


@pytest.mark.parametrize("nt", [0, 5])
def test_known_layouts_have_a_workspace(nt):
    L = _lib.lib()
    rows, conv = (L.obb_loss_workspace_bytes(C.byref(config(k)), nt) for k in (LAYOUT_ROWS, LAYOUT_CONV))
    assert rows > 0 and conv > 0
    assert conv < rows, "the conv layout keeps no dense objectness column"


@pytest.mark.parametrize("layout", [2, -1])
def test_unknown_layout_is_refused_before_any_device_call(layout):
    L = _lib.lib()
    cfg = config(layout)
    assert L.obb_loss_workspace_bytes(C.byref(cfg), 5) == 0
    assert L.obb_loss_workspace_bytes(C.byref(cfg), 0) == 0
    p = C.c_void_p(1 << 20)                                        # never followed
    lv = (C.c_void_p * 2)(1 << 20, 1 << 20)
    assert L.obb_loss_build_targets(C.byref(cfg), p, 5, 187, p, None, 0, None) == -1
    assert L.obb_loss_export_targets(C.byref(cfg), 5, 0, 3, p, p, p, p, p, None, 0, None) == -1
    assert L.obb_loss_forward(C.byref(cfg), lv, 0, p, 5, 187, p, None, 0, None) == -1
    assert L.obb_loss_backward(C.byref(cfg), lv, 0, p, 5, 187, p, lv, None, 0, None) == -1
    for ok in (LAYOUT_ROWS, LAYOUT_CONV):                          # the same calls with a known layout get as far as the workspace check
        cfg.head_layout = ok
        assert L.obb_loss_forward(C.byref(cfg), lv, 0, p, 5, 187, p, None, 0, None) == -2
        assert L.obb_loss_backward(C.byref(cfg), lv, 0, p, 5, 187, p, lv, None, 0, None) == -2


# ---------------------------------------------------------------------------------------------------- is_conv_view
BS, NA, NO = 2, 3, 187


def conv_out(ny, nx, dtype=torch.float32, extra=0):
    """A (bs, na*no, ny, nx) block whose first element is 16-byte aligned, `extra` spare elements behind it."""
    n = BS * NA * NO * ny * nx
    buf = torch.zeros(n + extra + 16, dtype=dtype)
    skip = (-buf.data_ptr() % 16) // buf.element_size()
    return buf[skip:skip + n + extra]


def view_of(c, ny, nx):
    return c.view(BS, NA, NO, ny, nx).permute(0, 1, 3, 4, 2)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("ny,nx", [(8, 8), (3, 5), (1, 7), (2, 1)])
def test_the_permuted_view_of_a_conv_output_is_recognised(ny, nx, dtype):
    v = view_of(conv_out(ny, nx, dtype).view(BS, NA * NO, ny, nx), ny, nx)
    assert v.shape == (BS, NA, ny, nx, NO) and not v.is_contiguous()
    assert is_conv_view(v) and is_conv_view(v, NA) and not is_conv_view(v, NA + 1)
    assert is_conv_view(v.detach()) and is_conv_view(v[:])


def test_a_contiguous_copy_is_not():
    v = view_of(conv_out(3, 5).view(BS, NA * NO, 3, 5), 3, 5)
    assert not is_conv_view(v.contiguous())
    assert not is_conv_view(torch.zeros(BS, NA, 3, 5, NO))


def test_a_channels_last_conv_output_is_not():
    c = conv_out(4, 6).view(BS, NA * NO, 4, 6).contiguous(memory_format=torch.channels_last)
    v = view_of(c, 4, 6)
    assert v.shape == (BS, NA, 4, 6, NO) and not is_conv_view(v)


def test_a_storage_offset_of_one_element_is_not():
    for dtype in (torch.float32, torch.float16, torch.bfloat16):
        c = conv_out(3, 5, dtype, extra=1)
        n = BS * NA * NO * 15
        assert is_conv_view(view_of(c[:n].view(BS, NA * NO, 3, 5), 3, 5))
        v = view_of(c[1:n + 1].view(BS, NA * NO, 3, 5), 3, 5)
        assert v.data_ptr() % 16 == c.element_size() and not is_conv_view(v), dtype


def test_one_by_one_grids():
    """ny = nx = 1: the two layouts are the same bytes, and a dimension of size 1 may carry any stride."""
    c = conv_out(1, 1).view(BS, NA * NO, 1, 1)
    v = view_of(c, 1, 1)
    assert is_conv_view(v) and is_conv_view(v.contiguous())
    one = conv_out(1, 1)[:NO].view(1, NO, 1, 1).view(1, 1, NO, 1, 1).permute(0, 1, 3, 4, 2)          # bs = na = 1 as well
    assert is_conv_view(one) and is_conv_view(one.as_strided(one.shape, (7, 11, 13, 17, 1)))


def test_a_view_of_the_wrong_permutation_is_not():
    c = conv_out(3, 5).view(BS, NA * NO, 3, 5)
    assert not is_conv_view(c.view(BS, NA, NO, 3, 5).permute(0, 1, 4, 3, 2))                   # (nx, ny) swapped
    assert not is_conv_view(c.view(BS, NO, NA, 3, 5).permute(0, 2, 3, 4, 1))                   # channel-major anchors
    assert not is_conv_view(c.view(BS, NA, NO, 3, 5))                                           # not permuted at all
    assert not is_conv_view(c)                                                                   # 4-D
    sq = conv_out(4, 4).view(BS, NA * NO, 4, 4)
    assert not is_conv_view(sq.view(BS, NA, NO, 4, 4).permute(0, 1, 4, 3, 2))                  # square grid, transposed
    assert not is_conv_view(view_of(sq, 4, 4)[:, :, ::2])                                       # every other row
    assert not is_conv_view(view_of(sq, 4, 4)[..., :100])                                       # fewer channels of a wider block
