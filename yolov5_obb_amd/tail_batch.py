"""The batch layout of the validation tail (val.py:209-250 of the reference), stated once for every Python front end that hands
a batch to the C ABI (val.val_tail_batch, val.val_tail_batch_obb, val.ValStats.add_batch, utils.metrics.ConfusionMatrix.add_batch):
per-image counts -> offsets, the packed detections, `targets` on the device, and the chunks of at most MAX_BS images one entry
call takes -- offsets re-based to 0, the per-image (pad_x, pad_y, gain, w, h) rows, the chunk's labels with their image column
re-based.  No kernel call and no device check here (require_cuda stays with the callers): everything runs on CPU tensors too
(tests/test_tail_batch_host.py).  Pointers are plain integers (None: null), which ctypes takes for a void pointer."""
import ctypes as C
import threading
from itertools import accumulate

import torch

MAX_BS = 64      # csrc/head.hip kValTailMaxBs: images per obb_val_tail_batch_f32 / _obb_f32 / obb_confusion_batch_f32 call
_arr_cache = {}


def as_f32(t, dev):
    """t as a contiguous float32 tensor on dev -- without a torch call when it already is one (the common case)."""
    if t.dtype == torch.float32 and t.device == dev and t.is_contiguous():
        return t
    return t.to(device=dev, dtype=torch.float32).contiguous()


def first_of_views(preds, dev):
    """The first non-empty of preds when the non-empty ones are float32 (n_i, 7) views of ONE buffer on dev, one behind the
    other, as non_max_suppression_obb returns them; else None."""
    first = None
    for p in preds:
        if p.shape[0] == 0:
            continue
        if p.device != dev or p.dtype != torch.float32 or p.dim() != 2 or p.shape[1] != 7 or not p.is_contiguous():
            return None
        if first is None:
            first, nxt = p, p.data_ptr()
        if p.data_ptr() != nxt:
            return None
        nxt += p.shape[0] * 28
    return first


def chunk_ranges(offs):
    """(b0, b1, lo, hi) of every chunk of at most MAX_BS images that holds a detection: images [b0, b1), packed rows [lo, hi)."""
    bs, out = len(offs) - 1, []
    for b0 in range(0, bs, MAX_BS):
        b1 = min(bs, b0 + MAX_BS)
        if offs[b1] > offs[b0]:
            out.append((b0, b1, offs[b0], offs[b1]))
    return out


def rebased(offs, b0, b1):
    """offs[b0 .. b1] counted from the chunk's first row."""
    base = offs[b0]
    return [o - base for o in offs[b0:b1 + 1]] if base else offs[b0:b1 + 1]


def img5_rows(shapes, b0, b1):
    """(pad_x, pad_y, gain, w, h) of images [b0, b1), flat, from shapes as LoadImagesAndLabels yields them:
    per image (shape (h, w), ratio_pad ((gain, gain), (pad_x, pad_y)))."""
    flat = []
    for j in range(b0, b1):
        shape, ratio_pad = shapes[j][0], shapes[j][1]
        flat += (ratio_pad[1][0], ratio_pad[1][1], ratio_pad[0][0], shape[1], shape[0])
    return flat


def chunk_labels(tg, b0, b1):
    """The labels of images [b0, b1) in the order of `tg`, as a copy with the image column counted from b0, and their rows in tg."""
    rows = torch.nonzero((tg[:, 0] >= b0) & (tg[:, 0] < b1))[:, 0]
    tgk = tg[rows]                                               # (indexing copies: tg stays as it is)
    tgk[:, 0] -= b0
    return tgk, rows


def split_rows(arr, niou, counts):
    """Host rows (n, niou + 2) [correct x niou as 0 / 1, conf, cls] -> per image (correct bool (n_i, niou), conf (n_i), cls (n_i)),
    what val.py:250 appends."""
    host = torch.from_numpy(arr)
    return list(zip(torch.from_numpy(arr[:, :niou] > 0.5).split(counts), host[:, niou].split(counts), host[:, niou + 1].split(counts)))


def box_arrays(n, dev):
    """Empty (pred_poly (n, 10), pred_hbb (n, 6), pred_polyn (n, 10), pred_hbbn (n, 6)) float32 on dev."""
    return tuple(torch.empty((n, c), dtype=torch.float32, device=dev) for c in (10, 6, 10, 6))


class Chunk:
    """One entry call's share of a batch: images [b0, b1) (k of them), packed rows [lo, hi); doff (c_int64[k + 1], from 0) and
    img5 (c_float[5 k], None without shapes); the labels (tg, tg_ptr, ntk, tcols) and `rows`, where they came from in `targets`
    (None when the chunk is the whole batch and the labels are `targets` itself)."""
    __slots__ = ("b0", "b1", "k", "lo", "hi", "doff", "img5", "tg", "tg_ptr", "ntk", "tcols", "rows")

    def part(self, t, cols, base=0):
        """The address of the chunk's rows in a per-detection float32 / int32 array of `cols` columns that starts at row `base`."""
        return t.data_ptr() + (base + self.lo) * cols * 4

    def box_parts(self, boxes):
        """part() of the four arrays of box_arrays, or four null pointers when the caller wants no boxes."""
        return [self.part(t, t.shape[1]) for t in boxes] if boxes else [None] * 4


class TailBatch:
    """counts, offs, n of a list of per-image detections; tg / nt / tcols: `targets` as contiguous float32 on `device`
    (None / 0 / 0 when there are no labels); packed: the detections as ONE (n, 7) float32 array (None when n = 0), made at its
    first use -- the views of first_of_views in place (in_place: a caller's device check of preds can be left out), else a copy."""

    def __init__(self, preds, targets, device):
        self.preds, self.device, self.bs = preds, device, len(preds)
        self.counts = [p.shape[0] for p in preds]
        self.offs = list(accumulate(self.counts, initial=0))
        self.n = self.offs[-1]
        self._first, self._packed = first_of_views(preds, device), None
        self.in_place = self._first is not None
        self.tg = as_f32(targets, device) if targets.dim() == 2 and targets.shape[0] else None
        self.nt, self.tcols = (self.tg.shape[0], self.tg.shape[1]) if self.tg is not None else (0, 0)

    @property
    def packed(self):
        if self._packed is None and self.n:
            if not self.in_place:
                self._packed = torch.cat([p.to(torch.float32) for p in self.preds], 0).contiguous()
            else:
                first, n = self._first, self.n
                self._packed = first if first.shape[0] == n else torch.as_strided(first, (n, 7), (7, 1))
        return self._packed

    def chunks(self, shapes=None):
        """One Chunk per entry call, chunks without a detection left out.  The ctypes arrays are cached per (thread, k) -- ctypes
        releases the GIL during the call that reads them -- and every entry copies them into its kernel arguments before it
        returns (csrc/head.hip: vt_fill_imgs), so a chunk is valid until the next one is drawn, by this or another loop."""
        whole = self.bs <= MAX_BS                                # (every batch size val.py uses)
        for b0, b1, lo, hi in chunk_ranges(self.offs):
            ch = Chunk()
            ch.b0, ch.b1, ch.lo, ch.hi, k = b0, b1, lo, hi, b1 - b0
            key = (threading.get_ident(), k)
            arrs = _arr_cache.get(key)
            if arrs is None:
                arrs = _arr_cache[key] = ((C.c_int64 * (k + 1))(), (C.c_float * (5 * k))())
            ch.k, ch.doff, ch.img5 = k, arrs[0], arrs[1] if shapes is not None else None
            ch.doff[:] = rebased(self.offs, b0, b1)
            if shapes is not None:
                ch.img5[:] = img5_rows(shapes, b0, b1)
            ch.tg, ch.ntk, ch.tcols, ch.rows = self.tg, self.nt, self.tcols, None
            if self.nt and not whole:                            # a chunk of a very large batch: its labels, re-based
                ch.tg, ch.rows = chunk_labels(self.tg, b0, b1)
                ch.ntk = int(ch.tg.shape[0])
            ch.tg_ptr = ch.tg.data_ptr() if ch.ntk else None
            yield ch
