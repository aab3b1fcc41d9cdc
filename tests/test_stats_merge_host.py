"""CPU, world_size 2, gloo: the exchange of the multi-rank device metrics (yolov5_obb_amd/stats_merge.py) on CPU tensors -- the
totals that size the padding, the padded buffers, the ids -- with a numpy restatement of obb_stats_merge_f32 injected for the
device merge (tests/stats_merge_cases.py: merge_numpy), as val_sharded.run takes stand-ins for nms / postprocess / match.
Every rank must end with the statistics of ONE process that saw every image in id order.  The entry itself and val.ValStats
are covered by tests/test_stats_merge_gpu.py."""
import os
import re
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import stats_merge_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = 12                                   # niou + 2


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _check(mg, n_items):
    """mg against the Shard of one accumulator fed images 0 .. n_items - 1 -> a list of what differs."""
    one = SC.shard_of(range(n_items), W)
    bad = [name for name, got, want in (("rows", mg.rows, one.rows), ("rows_obb", mg.rows_obb, one.rows_obb), ("tcls", mg.tcls, one.tcls),
                                        ("img_rows", mg.img_rows, one.img_rows), ("img_labels", mg.img_labels, one.img_labels))
           if not SC.same_bits(got.numpy(), want.numpy())]
    if mg.totals != (int(one.rows.shape[0]), int(one.tcls.shape[0]), n_items) or mg.supplied != n_items:
        bad.append(f"totals {mg.totals} supplied {mg.supplied}")
    if mg.info.tolist() != [[0, int(one.rows.shape[0]), 0, 0]] * 2 + [[0, int(one.tcls.shape[0]), 0, 0]]:
        bad.append(f"info {mg.info.tolist()}")
    return bad


def _worker(rank, world_size, port, n_items, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world_size))
    dist.init_process_group("gloo", rank=rank, world_size=world_size)
    try:
        from yolov5_obb_amd import stats_merge
        from yolov5_obb_amd.utils import shard
        ids = shard.shard_indices(n_items)
        mg = stats_merge.exchange(SC.shard_of(ids, W), W, True, merge=SC.merge_numpy)
        q.put((rank, len(ids), _check(mg, n_items)))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("n_items", [1, 37])
def test_two_rank_exchange_gives_every_rank_the_single_process_statistics(n_items):
    """n_items = 1: rank 1 has no image (empty rows, labels and ids, and the padding of rank 0's share); 37: uneven shards."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, n_items, q)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    got = sorted(q.get(timeout=10) for _ in range(2))
    assert [g[0] for g in got] == [0, 1] and got[0][1] + got[1][1] == n_items and got[1][1] == n_items // 2
    assert got[0][2] == [] and got[1][2] == []


def test_without_a_process_group_the_exchange_is_the_merge_of_one_shard():
    from yolov5_obb_amd import stats_merge
    assert _check(stats_merge.exchange(SC.shard_of(range(9), W), W, True, merge=SC.merge_numpy), 9) == []


@pytest.mark.parametrize("order", [[[0, 2, 4, 6], [1, 3, 5]], [[6, 1], [], [3, 0, 5, 2, 4]]])
def test_parts_in_any_assignment_merge_to_id_order(order):
    """merge_parts (what ValStats.merged runs): strided shards, and shuffled ones with an empty part; the padding differs per part."""
    from yolov5_obb_amd import stats_merge
    assert _check(stats_merge.merge_parts([SC.shard_of(ids, W) for ids in order], W, True, merge=SC.merge_numpy), 7) == []


def test_ids_nobody_supplies_are_images_without_rows():
    from yolov5_obb_amd import stats_merge
    mg = stats_merge.merge_parts([SC.shard_of([1], W), SC.shard_of([4], W)], W, True, n_images_total=6, merge=SC.merge_numpy)
    one = SC.shard_of([1, 4], W)
    assert SC.same_bits(mg.rows.numpy(), one.rows.numpy()) and SC.same_bits(mg.tcls.numpy(), one.tcls.numpy())
    assert mg.img_rows.tolist() == [0, 3, 0, 0, 7, 0] and mg.img_labels.tolist() == [0, 0, 0, 0, 4, 0] and mg.totals == (10, 4, 6) and mg.supplied == 2
    assert stats_merge.describe(mg.info) is None


def test_the_info_words_are_worded_like_gather_results():
    from yolov5_obb_amd import stats_merge
    two = stats_merge.merge_parts([SC.shard_of([0, 5], W), SC.shard_of([1, 5], W)], W, True, n_images_total=6, merge=SC.merge_numpy)
    assert stats_merge.describe(two.info) == "image 5 produced by two ranks"
    far = stats_merge.merge_parts([SC.shard_of([0, 9], W)], W, True, n_images_total=6, merge=SC.merge_numpy)
    assert stats_merge.describe(far.info) == "an image id outside [0, n_images_total)"
    sh = SC.shard_of([0, 1, 2], W)
    short = stats_merge.merge_parts([sh._replace(img_rows=sh.img_rows - 1)], W, True, merge=SC.merge_numpy)
    assert stats_merge.describe(short.info) == "the per-image counts of rank 0 do not add up to its rows"


def test_the_layout_keeps_every_section_on_a_row_boundary():
    from yolov5_obb_amd import stats_merge
    for w, obb, R, M in [(12, True, 0, 0), (12, False, 5, 1), (12, True, 5, 13), (3, True, 7, 2)]:
        o_obb, o_tcls, L = stats_merge.layout(w, obb, R, M)
        assert o_obb == R * w and o_tcls == (2 if obb else 1) * R * w and L % w == 0 and L >= max(w, o_tcls + M) and L < o_tcls + M + 2 * w


def test_the_entry_is_the_only_one_that_names_its_workspace_size_ws_cap():
    """Host: the functions of include/obb_hip.h with a `size_t ws_cap` parameter are exactly the entry whose workspace contract
    tests/test_stats_merge_gpu.py holds (each module that has its own table names the argument differently: ws_bytes, ws_size,
    ws_len, ws_cap)."""
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "obb_hip.h")).read(), flags=re.S)
    found = [m.group(1) for m in re.finditer(r"\b(\w+)\s*\(([^;{}()]*)\)\s*;", text) if re.search(r"\bsize_t\s+ws_cap\b", m.group(2))]
    assert found == ["obb_stats_merge_f32"]
    from yolov5_obb_amd import _lib
    assert "obb_stats_merge_f32" in _lib.SIGNATURES and "obb_stats_merge_workspace_bytes" in _lib.SIGNATURES


def test_every_argument_refusal_answers_without_a_device():
    """The refusals of include/obb_hip.h answer before any device call: every device pointer here is NULL or not memory, and no
    GPU is needed.  (With a device the same calls run in tests/test_stats_merge_gpu.py.)"""
    import ctypes as C
    from yolov5_obb_amd import _lib
    if torch.cuda.is_available():
        pytest.skip("a device is visible: the refusals are tested by the gpu tests, on NULL device pointers")
    L = _lib.lib()
    for rc, kw in SC.refusals():
        assert SC.call_refused(L, C, **kw) == rc, kw
