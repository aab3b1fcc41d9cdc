"""GPU: the memory contract of obb_tile_merge_f32, called through the raw C ABI with the harness of tests/abi_contract.py as
tests/test_abi_contract_gpu.py calls its neighbours: an exact-size poisoned workspace between canaries, a short / NULL /
misaligned `ws` refused before anything is written, a capped grid, a side stream.

(The table of tests/test_abi_contract_gpu.py is tied to the header's `ws_bytes` parameters by a host test of that module; this
entry names the same argument `ws_len` and has its table here.)

The oracle is the host restatement of the file pipeline (tests/tile_merge_cases.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from oracle import pyref
from tests import abi_contract as AC
from tests import tile_merge_cases as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = {"parity": TC.parity_scene, "large": TC.large_scene}


def vp(x):
    return C.c_void_p(int(x)) if x else C.c_void_p(0)


def L_():
    from yolov5_obb_amd import _lib
    return _lib.lib()


def tile_case(name, flags=1):
    from yolov5_obb_amd.tile_merge import TileRec
    scene = TC.memo(name, SCENES[name])
    nc, n_src, ntile = scene["nc"], scene["n_src"], len(scene["tiles"])
    det7 = torch.cat(scene["preds"]).numpy()
    n, nseg = len(det7), n_src * nc
    off = (C.c_int64 * (ntile + 1))(*np.concatenate([[0], np.cumsum([len(p) for p in scene["preds"]])]).tolist())
    recs = (TileRec * ntile)()
    for t, (src, left, up, rate, ratio_pad) in enumerate(scene["tiles"]):
        gain, pad = (ratio_pad[0][0], ratio_pad[1]) if ratio_pad is not None else (1.0, (0.0, 0.0))
        recs[t] = TileRec(src, left, up, rate, pad[0], pad[1], gain)
    nms = pyref.merge_nms_poly_all if flags & 2 else pyref.merge_nms_poly_fast

    def call(L, P, ws, wsb, st, mark):
        return L.obb_tile_merge_f32(vp(P["det7"]), off, recs, ntile, n_src, nc, 0.2, flags, vp(P["out"]), vp(P["out_count"]), vp(P["info"]),
                                    vp(ws), wsb, vp(st))

    def verify(O):
        want = TC.memo(f"{name}_rows{'_all' if flags & 2 else ''}", lambda: TC.expected_rows(scene, True, nms))
        info, count = O("info", np.int32), O("out_count", np.int64)
        assert info.tolist() == [0, 0], (name, info.tolist())
        seg = (want[:, 10] * nc + want[:, 9]).astype(np.int64)
        assert count.tolist() == np.bincount(seg, minlength=nseg).tolist(), name
        out = O("out", np.float64).reshape(n, 11)
        assert out[:len(want)].tobytes() == want.tobytes(), name
        assert (out[len(want):].view(np.uint8) == AC.FILL).all(), "rows behind the merged ones are not written"
        return [info, count, out[:len(want)].copy()]

    return AC.Case(f"tile_merge-{name}-flags{flags}", ["obb_tile_merge_f32"], dict(det7=det7), dict(out=n * 11 * 8, out_count=nseg * 8, info=8),
                   lambda L: L.obb_tile_merge_workspace_bytes(n, n_src, nc), call, verify)


def test_the_entry_is_the_only_one_that_names_its_workspace_size_ws_len():
    """Host: the functions of include/obb_hip.h with a `size_t ws_len` parameter are exactly the entry this module calls."""
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "obb_hip.h")).read(), flags=re.S)
    found = [m.group(1) for m in re.finditer(r"\b(\w+)\s*\(([^;{}()]*)\)\s*;", text) if re.search(r"\bsize_t\s+ws_len\b", m.group(2))]
    assert found == ["obb_tile_merge_f32"]


@pytest.mark.gpu
@pytest.mark.parametrize("name,flags,donor", [("parity", 1, "large"), ("large", 1, "parity"), ("parity", 3, "large")])
def test_exact_poisoned_workspace_between_canaries(dev, oracle_lib, name, flags, donor):
    AC.run_poisons(L_(), dev, tile_case(name, flags), tile_case(donor))


@pytest.mark.gpu
@pytest.mark.parametrize("ws_mode", ["short", "null", "+8", "+128"])
def test_a_short_missing_or_misaligned_workspace_is_refused_before_anything_is_written(dev, oracle_lib, ws_mode):
    AC.run_refused(L_(), dev, tile_case("parity"), ws_mode)


@pytest.mark.gpu
def test_query_and_call_under_a_capped_grid(dev, oracle_lib):
    AC.run_capped(L_(), dev, tile_case("large"))


@pytest.mark.gpu
def test_all_work_is_enqueued_on_the_callers_stream(dev, oracle_lib):
    from tests.test_abi_contract_gpu import DELAY_ITERS, _seed_matrix
    res, pending = AC.run_on_side_stream(L_(), dev, tile_case("large"), DELAY_ITERS, _seed_matrix(dev))
    assert pending, "the delay had drained before the ABI call returned: the run proves nothing"
