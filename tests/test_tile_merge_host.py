"""CPU: the host side of yolov5_obb_amd/tile_merge.py -- the tile origins of the reference's splitter
(DOTA_devkit/SplitOnlyImage_multi_process.py:66-83), the tile names the merge parses back
(ResultMerge_multi_process.py:196-201), the obb_tile_rec layout and the argument checks of obb_tile_merge_f32, which answer
before any device call."""
import ctypes as C

import pytest


def reference_loop(width, height, subsize, gap):
    """SplitOnlyImage_multi_process.py:66-83 as written (two while loops with breaks)."""
    slide, out = subsize - gap, []
    left = 0
    while left < width:
        if left + subsize >= width:
            left = max(width - subsize, 0)
        up = 0
        while up < height:
            if up + subsize >= height:
                up = max(height - subsize, 0)
            out.append((left, up))
            if up + subsize >= height:
                break
            up += slide
        if left + subsize >= width:
            break
        left += slide
    return out


def test_split_origins_of_the_issue():
    from yolov5_obb_amd.tile_merge import split_origins
    o = split_origins(2000, 1500)
    assert o == [(l, u) for l in (0, 824, 976) for u in (0, 476)], o
    assert split_origins(800, 600) == [(0, 0)]
    assert split_origins(1024, 1024) == [(0, 0)]
    assert split_origins(1025, 1024) == [(0, 0), (1, 0)]


@pytest.mark.parametrize("size", [(1, 1), (823, 824), (824, 825), (1848, 1847), (1849, 1024), (4000, 4000), (5000, 1023), (300, 7000)])
@pytest.mark.parametrize("subsize,gap", [(1024, 200), (1024, 0), (600, 150), (512, 511)])
def test_split_origins_equals_the_reference_loop(size, subsize, gap):
    from yolov5_obb_amd.tile_merge import split_origins
    o = split_origins(size[0], size[1], subsize, gap)
    assert o == reference_loop(size[0], size[1], subsize, gap)
    covered_x = max(l for l, _ in o) + subsize >= size[0] and min(l for l, _ in o) == 0
    covered_y = max(u for _, u in o) + subsize >= size[1] and min(u for _, u in o) == 0
    assert covered_x and covered_y


def test_split_origins_refuses_a_step_of_zero():
    from yolov5_obb_amd.tile_merge import split_origins
    with pytest.raises(ValueError):
        split_origins(2000, 1500, 200, 200)
    with pytest.raises(ValueError):
        split_origins(0, 1500)


@pytest.mark.parametrize("rate", [1.0, 0.5, 1.5, 1])
def test_tile_names_parse_back_through_the_merge(tmp_path, rate):
    """tile_name -> a Task1 line -> parse_result_file (the module's own regexes): the source name, the origin and the rate return."""
    from yolov5_obb_amd.DOTA_devkit import ResultMerge_multi_process as RM
    from yolov5_obb_amd.tile_merge import split_origins, tile_name
    lines = []
    for left, up in split_origins(2000, 1500):
        name = tile_name("P0007", rate, left, up)
        assert RM._INT.findall(RM._TILE_XY.findall(name)[0]) == [str(left), str(up)]
        assert RM._TILE_RATE.findall(name)[0] == str(rate) and name.split("__")[0] == "P0007"
        lines.append(name + " 0.5 " + " ".join(["10.0", "20.0"] * 4))
    path = tmp_path / "Task1_plane.txt"
    path.write_text("\n".join(lines) + "\n")
    boxes = RM.parse_result_file(str(path))
    assert list(boxes) == ["P0007"] and len(boxes["P0007"]) == 6
    for det, (left, up) in zip(boxes["P0007"], split_origins(2000, 1500)):
        assert det == [(10.0 + left) / float(rate), (20.0 + up) / float(rate)] * 4 + [0.5]


def test_tile_rec_has_the_headers_layout():
    from yolov5_obb_amd.tile_merge import TileRec
    assert C.sizeof(TileRec) == 40
    assert [getattr(TileRec, f).offset for f, _ in TileRec._fields_] == [0, 4, 8, 16, 24, 28, 32]


def test_argument_checks_answer_before_any_device_call():
    """OBB_ERR_BAD_ARG (-1) for what include/obb_hip.h lists; no pointer here is device memory, so nothing may be launched."""
    from yolov5_obb_amd import _lib
    from yolov5_obb_amd.tile_merge import TileRec
    L = _lib.lib()
    p = C.c_void_p(1 << 20)
    recs = (TileRec * 2)(TileRec(0, 0, 0, 1.0, 0.0, 0.0, 1.0), TileRec(1, 824, 0, 0.5, 0.0, 0.0, 1.0))
    off = (C.c_int64 * 3)(0, 5, 9)

    def call(off=off, recs=recs, ntile=2, n_src=2, nc=3, flags=1, out=p, cnt=p, info=p):
        return L.obb_tile_merge_f32(p, off, recs, ntile, n_src, nc, 0.2, flags, out, cnt, info, None, 0, None)

    assert call() == -2                                            # everything in order: the missing workspace is what stops it
    assert call(nc=0) == -1 and call(nc=257) == -1 and call(n_src=0) == -1 and call(ntile=-1) == -1
    assert call(n_src=1) == -1, "a tile's source image outside [0, n_src)"
    assert call(n_src=1 << 24, nc=256) == -1 and call(n_src=1 << 62, nc=4) == -1, "n_src * nc past int32"
    assert call(flags=4) == -1 and call(cnt=None) == -1 and call(info=None) == -1 and call(out=None) == -1
    assert call(off=(C.c_int64 * 3)(1, 5, 9)) == -1 and call(off=(C.c_int64 * 3)(0, 5, 4)) == -1
    assert call(off=(C.c_int64 * 3)(0, 5, 1 << 31)) == -1, "n past int32"
    for bad in (TileRec(0, 0, 0, 0.0, 0.0, 0.0, 1.0), TileRec(0, 0, 0, 1.0, 0.0, 0.0, 0.0), TileRec(0, 0, 0, float("nan"), 0.0, 0.0, 1.0),
                TileRec(-1, 0, 0, 1.0, 0.0, 0.0, 1.0)):
        assert call(recs=(TileRec * 2)(recs[0], bad)) == -1
    assert L.obb_tile_merge_workspace_bytes(-1, 1, 3) == 0 and L.obb_tile_merge_workspace_bytes(10, 0, 3) == 0
    assert L.obb_tile_merge_workspace_bytes(10, 1, 257) == 0 and L.obb_tile_merge_workspace_bytes(1 << 31, 1, 3) == 0
    assert L.obb_tile_merge_workspace_bytes(10, 1 << 24, 256) == 0 and L.obb_tile_merge_workspace_bytes(10, 1 << 62, 4) == 0


def test_the_planted_pairs_fall_on_both_sides_of_the_threshold(oracle_lib):
    """The GPU tests' scene holds what it claims: among sightings of one object in different tiles there are pairs above and
    below IoU 0.2, and its rounded scores are distinct inside every segment."""
    import numpy as np
    import oracle
    from tests import tile_merge_cases as TC
    scene = TC.memo("parity", TC.parity_scene)
    rows, seg = TC.host_rows(scene, True)
    at = np.flatnonzero(seg == 0)
    iou = oracle.piou_matrix(rows[at, :8].copy(), rows[at, :8].copy())
    near = np.hypot(rows[at, None, 0] - rows[None, at, 0], rows[at, None, 1] - rows[None, at, 1]) < 5
    pairs = iou[np.triu(near, 1)]
    print(f"pairs within 5 px: {len(pairs)}, IoU > 0.2: {(pairs > 0.2).sum()}, IoU <= 0.2: {(pairs <= 0.2).sum()}")
    assert (pairs > 0.2).sum() >= 20 and (pairs <= 0.2).sum() >= 5
    assert TC.scores_distinct_per_segment(scene) and TC.scores_distinct_per_segment(TC.memo("large", TC.large_scene))
