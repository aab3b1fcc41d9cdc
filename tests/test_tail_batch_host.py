"""CPU: yolov5_obb_amd/tail_batch.py, the one statement of the validation tail's batch layout -- chunks of at most 64 images,
offsets re-based per chunk, the (pad_x, pad_y, gain, w, h) rows, the chunk's labels re-based, the packing rule of the detections
and the split of the statistics rows -- on CPU tensors, against restatements written out here."""
import numpy as np
import pytest
import torch

from yolov5_obb_amd import tail_batch as TB


def _counts(bs, kind):
    g = torch.Generator().manual_seed(bs)
    c = torch.randint(0, 7, (bs,), generator=g).tolist()        # zeros among them
    if kind == "empty_middle":
        c[64:128] = [0] * len(c[64:128])
    if kind == "none":
        c = [0] * bs
    return c


def _restated(counts):
    """(b0, b1, lo, hi, doff) per chunk of <= 64 images with a detection."""
    offs = np.concatenate(([0], np.cumsum(counts))).astype(int)
    out = []
    for b0 in range(0, len(counts), 64):
        b1 = min(len(counts), b0 + 64)
        if offs[b1] > offs[b0]:
            out.append((b0, b1, int(offs[b0]), int(offs[b1]), (offs[b0:b1 + 1] - offs[b0]).tolist()))
    return out


def _shapes(bs):
    return [((1100 + b, 1300 - b), ((0.5 + b / 1024, 0.5 + b / 1024), (4.0 + b % 3, 9.5 + b % 2))) for b in range(bs)]


@pytest.mark.parametrize("kind", ["mixed", "empty_middle", "none"])
@pytest.mark.parametrize("bs", [1, 63, 64, 65, 128, 129, 130])
def test_chunk_ranges_offsets_and_skipped_chunks(bs, kind):
    counts = _counts(bs, kind)
    want = _restated(counts)
    offs = [0] + np.cumsum(counts).tolist()
    # the pure arithmetic, on lists
    assert [r + (TB.rebased(offs, r[0], r[1]),) for r in TB.chunk_ranges(offs)] == want
    # and through TailBatch.chunks on CPU tensors
    tb = TB.TailBatch([torch.zeros(c, 7) for c in counts], torch.zeros(0, 7), torch.device("cpu"))
    assert tb.counts == counts and tb.offs == offs and tb.n == offs[-1] and (tb.tg, tb.nt, tb.tcols) == (None, 0, 0)
    got = [(ch.b0, ch.b1, ch.lo, ch.hi, list(ch.doff), ch.k, len(ch.doff), ch.img5, ch.tg_ptr, ch.ntk, ch.rows) for ch in tb.chunks()]
    assert got == [w + (w[1] - w[0], w[1] - w[0] + 1, None, None, 0, None) for w in want]
    if kind == "none":
        assert want == [] and tb.packed is None
    if kind == "empty_middle" and bs > 128:
        assert [w[0] for w in want] == [0, 128]


@pytest.mark.parametrize("bs", [1, 64, 65, 130])
def test_img5_is_pad_x_pad_y_gain_w_h_per_image(bs):
    shapes = _shapes(bs)
    assert TB.img5_rows(shapes, 0, 1) == [4.0, 9.5, 0.5, 1300, 1100]
    tb = TB.TailBatch([torch.zeros(2, 7)] * bs, torch.zeros(0, 7), torch.device("cpu"))
    seen = 0
    for ch in tb.chunks(shapes):
        want = np.array([[s[1][1][0], s[1][1][1], s[1][0][0], s[0][1], s[0][0]] for s in shapes[ch.b0:ch.b1]], dtype=np.float32)
        assert len(ch.img5) == 5 * ch.k and np.array_equal(np.array(ch.img5[:], dtype=np.float32).reshape(-1, 5), want)
        seen += ch.k
    assert seen == bs


def test_chunk_labels_keep_their_order_are_rebased_and_map_back_to_targets():
    bs = 130
    g = torch.Generator().manual_seed(7)
    targets = torch.rand(400, 9, generator=g)
    targets[:, 0] = torch.randint(0, bs, (400,), generator=g).float()       # shuffled: not sorted by image
    kept = targets.clone()
    tb = TB.TailBatch([torch.zeros(1, 7)] * bs, targets, torch.device("cpu"))
    assert tb.tg is targets and (tb.nt, tb.tcols) == (400, 9)
    chunks = 0
    for ch in tb.chunks():
        rows = torch.nonzero((kept[:, 0] >= ch.b0) & (kept[:, 0] < ch.b1))[:, 0]
        want = kept[rows].clone()
        want[:, 0] -= ch.b0
        assert ch.rows.dtype == torch.int64 and torch.equal(ch.rows, rows) and torch.equal(ch.tg, want)
        assert (ch.ntk, ch.tcols, ch.tg_ptr) == (len(rows), 9, ch.tg.data_ptr()) and ch.tg.is_contiguous() and ch.tg.dtype == torch.float32
        assert ch.tg.data_ptr() != targets.data_ptr() and float(ch.tg[:, 0].min()) >= 0 and float(ch.tg[:, 0].max()) < ch.k
        assert torch.equal(kept[ch.rows, 1:], ch.tg[:, 1:])
        chunks += 1
    assert chunks == 3 and torch.equal(targets, kept)
    # a chunk without labels hands a null pointer
    tb = TB.TailBatch([torch.zeros(1, 7)] * 65, kept[kept[:, 0] < 64], torch.device("cpu"))
    assert [(ch.ntk, ch.tg_ptr) for ch in tb.chunks()][1] == (0, None)
    # one chunk: `targets` itself, no copy, no rows; another dtype or layout is converted once
    tb = TB.TailBatch([torch.zeros(1, 7)] * 64, targets, torch.device("cpu"))
    (ch,) = tb.chunks()
    assert ch.tg is targets and ch.tg_ptr == targets.data_ptr() and ch.rows is None and (ch.ntk, ch.tcols) == (400, 9)
    tb = TB.TailBatch([torch.zeros(1, 7)], targets.double()[:, :8], torch.device("cpu"))
    assert tb.tg.dtype == torch.float32 and tb.tg.is_contiguous() and (tb.nt, tb.tcols) == (400, 8)


def test_packing_uses_consecutive_views_in_place_and_concatenates_anything_else():
    cpu = torch.device("cpu")
    buf = torch.arange(20 * 7, dtype=torch.float32).reshape(20, 7)
    empty = torch.zeros(0, 7)
    views = [buf[0:3], empty, buf[3:3], buf[3:9], empty, buf[9:20]]        # empty images between views are ignored
    tb = TB.TailBatch(views, torch.zeros(0, 7), cpu)
    assert tb.in_place and tb.packed.data_ptr() == buf.data_ptr() and tb.packed.shape == (20, 7) and torch.equal(tb.packed, buf)
    one = TB.TailBatch([empty, buf[5:9]], torch.zeros(0, 7), cpu).packed
    assert one.data_ptr() == buf[5:9].data_ptr() and one.shape == (4, 7)
    wide = torch.zeros(6, 14)
    for other in ([buf[0:3], buf[4:9]],                                  # a gap
                  [buf[0:3], buf[3:9].double()],                         # not float32
                  [buf[0:3], wide[:, ::2]],                              # not contiguous
                  [buf[3:9], buf[0:3]]):                                 # out of order
        tb = TB.TailBatch(other, torch.zeros(0, 7), cpu)
        packed, ptrs = tb.packed, {p.data_ptr() for p in other}
        assert not tb.in_place and tb.packed is packed and packed.data_ptr() not in ptrs and packed.dtype == torch.float32 and packed.is_contiguous()
        assert torch.equal(packed, torch.cat([p.float() for p in other], 0))
    # the slice pointer of a chunk: data_ptr + (base + lo) * cols * 4
    tb = TB.TailBatch([buf[0:3]] * 64 + [buf[3:9]], torch.zeros(0, 7), cpu)
    ch = list(tb.chunks())[1]
    t = torch.zeros(300, 12)
    assert ch.lo == 192 and ch.part(t, 12) == t.data_ptr() + 192 * 48 and ch.part(t, 12, 10) == t.data_ptr() + 202 * 48
    boxes = TB.box_arrays(tb.n, cpu)
    assert [tuple(b.shape) for b in boxes] == [(198, 10), (198, 6), (198, 10), (198, 6)] and all(b.dtype == torch.float32 for b in boxes)
    assert ch.box_parts(boxes) == [b.data_ptr() + 192 * b.shape[1] * 4 for b in boxes] and ch.box_parts(None) == [None] * 4


def test_split_rows_is_the_two_expressions_it_replaces():
    niou, counts = 10, [3, 0, 5, 1, 0]
    g = torch.Generator().manual_seed(3)
    arr = torch.cat(((torch.rand(9, niou, generator=g) > 0.5).float(), torch.rand(9, 2, generator=g)), 1).numpy()
    host = torch.from_numpy(arr)
    correct = torch.from_numpy(arr[:, :niou] > 0.5).split(counts)
    want = list(zip(correct, host[:, niou].split(counts), host[:, niou + 1].split(counts)))
    got = TB.split_rows(arr, niou, counts)
    assert len(got) == 5 and all(g_[0].dtype == torch.bool and g_[0].shape == (c, niou) for g_, c in zip(got, counts))
    assert all(torch.equal(a, b) for g_, w in zip(got, want) for a, b in zip(g_, w))
    assert TB.split_rows(np.zeros((0, niou + 2), dtype=np.float32), niou, [0, 0])[1][0].shape == (0, niou)


def test_the_arrays_are_per_thread():
    import threading
    tb = TB.TailBatch([torch.zeros(2, 7)] * 3, torch.zeros(0, 7), torch.device("cpu"))
    mine = next(tb.chunks()).doff
    theirs = []
    th = threading.Thread(target=lambda: theirs.append(next(tb.chunks()).doff))
    th.start(); th.join()
    assert next(tb.chunks()).doff is mine and theirs[0] is not mine and list(theirs[0]) == list(mine) == [0, 2, 4, 6]
