"""Validation statistics of several ranks -> the statistics of one process.

Sharded validation (val_sharded.py) gives every rank the rows of its own images.  utils.metrics.ap_from_rows orders equal
confidences by ascending row index of the rows IN IMAGE ORDER, and with a strided split image i lives on rank i mod world: the
ranks' rows have to be interleaved image by image.  That is one entry of libobb_hip.so, obb_stats_merge_f32 (csrc/stats_merge.h),
called three times -- rows, the oriented-box rows, target_cls -- on ONE buffer that holds every rank's share at a fixed stride:

    float32 (world, L)      per rank [rows R x w | rows_obb R x w (obb only) | target_cls M | padding to a multiple of w]
    int64   (world, 3, K)   per rank [rows of every image | labels of every image | global id of every image]

with R, M, K the largest row / label / image count of any rank and w = niou + 2.  `exchange` builds it with one all-gather of the
three totals and one of each buffer (RCCL: all_gather_into_tensor on device buffers; any other backend stages through the host,
once per run); `ValStats.merged` builds it from accumulators that already share a device.

Nothing here needs a GPU but `merge_device`: the exchange and the layout run on CPU tensors with a stand-in for it
(tests/test_stats_merge_host.py), as val_sharded.run runs with stand-ins for nms / postprocess / match."""
from collections import namedtuple

import torch

from . import _lib

BAD_ID, TWICE, RUN_TOTAL, CAPACITY = 1, 2, 4, 8            # bits of info[0] (include/obb_hip.h: obb_stats_merge_f32)
INFO_WORDS = 4

# what one rank holds: rows (n, w) and rows_obb (n, w) or None, target_cls (m) -- float32 -- and per image, in the order the
# images were added, its rows, its labels (int32) and its global id (int64)
Shard = namedtuple("Shard", "rows rows_obb tcls img_rows img_labels img_ids")

Merged = namedtuple("Merged", "rows rows_obb tcls img_rows img_labels info totals supplied")


def merge_device(src, src_stride, run_stride, rows_per_run, counts, img_id, images_per_run, n_images_total, width, dst, dst_stride,
                 counts_out, info):
    """obb_stats_merge_f32 on the current stream.  src: a float32 CUDA tensor that starts at row 0 of run 0; counts (world, K)
    int32 and img_id (world, K) int64, contiguous; dst (rows, dst_stride) float32, counts_out (n_images_total) int32 or None,
    info (4) int32 -- all on src's device.  This signature is the `merge` parameter of exchange / merge_gathered."""
    _lib.require_cuda(src, "src")
    dev, world = src.device, len(rows_per_run)
    for name, t, dt in (("counts", counts, torch.int32), ("img_id", img_id, torch.int64), ("dst", dst, torch.float32), ("info", info, torch.int32)):
        if t.device != dev or t.dtype != dt or not t.is_contiguous():
            raise RuntimeError(f"stats merge: {name} must be a contiguous {dt} tensor on {dev}")
    if src.dtype != torch.float32 or counts.shape != img_id.shape or counts.dim() != 2 or counts.shape[0] != world or info.numel() < INFO_WORDS:
        raise RuntimeError("stats merge: src float32, counts and img_id (world, max images per run), info (4)")
    if counts_out is not None and (counts_out.device != dev or counts_out.dtype != torch.int32 or counts_out.numel() < n_images_total):
        raise RuntimeError("stats merge: counts_out must be int32 (n_images_total) on the device of src")
    need = max((r * run_stride + nr for r, nr in enumerate(rows_per_run) if nr > 0), default=0)      # rows of src the entry may read
    if need and src.numel() < (need - 1) * src_stride + width:
        raise RuntimeError("stats merge: src is shorter than its runs")
    L = _lib.lib()
    i64 = _lib.C.c_int64 * world
    with _lib.guard(dev):
        st = _lib.stream_handle(dev)
        ws = _lib.workspace(L.obb_stats_merge_workspace_bytes(n_images_total), dev, st)
        rc = L.obb_stats_merge_f32(_lib.ptr(src), src_stride, run_stride, i64(*rows_per_run), _lib.ptr(counts), _lib.ptr(img_id),
                                   int(counts.shape[1]), i64(*images_per_run), world, n_images_total, width, _lib.ptr(dst), dst_stride,
                                   int(dst.shape[0]), _lib.ptr(counts_out), _lib.ptr(info), _lib.ptr(ws), ws.numel(), st)
    _lib.check(rc, "obb_stats_merge_f32")


def layout(w, obb, R, M):
    """(offset of rows_obb, offset of target_cls, L): one rank's float buffer, in floats; L is a multiple of w and at least w."""
    o_obb = R * w
    o_tcls = (2 if obb else 1) * R * w
    return o_obb, o_tcls, max(1, -(-(o_tcls + M) // w)) * w


def pack(sh, w, obb, R, M, K):
    """One rank's (L) float32 and (3, K) int64 buffers on the shard's device, padded with zeros."""
    o_obb, o_tcls, L = layout(w, obb, R, M)
    dev = sh.rows.device
    n, m, k = int(sh.rows.shape[0]), int(sh.tcls.shape[0]), int(sh.img_ids.shape[0])
    f = torch.zeros(L, dtype=torch.float32, device=dev)
    f[:n * w] = sh.rows.reshape(-1)
    if obb:
        f[o_obb:o_obb + n * w] = sh.rows_obb.reshape(-1)
    f[o_tcls:o_tcls + m] = sh.tcls
    i = torch.zeros((3, K), dtype=torch.int64, device=dev)
    i[0, :k], i[1, :k], i[2, :k] = sh.img_rows, sh.img_labels, sh.img_ids
    return f, i


def merge_gathered(fbuf, ibuf, totals, w, obb, n_images_total=None, merge=None):
    """fbuf (world, L) float32 and ibuf (world, 3, K) int64 on one device (the layout of the module docstring), totals: per rank
    (rows, labels, images) on the host -> Merged: rows (n, w), rows_obb or None, tcls (m), per image id its rows and labels
    (int32), info (3, 4) int32 -- the entry's info of the three merges, to be read where the caller synchronises anyway (see
    describe) --, totals (n, m, n_images_total) and supplied, the images the ranks hold between them.  Nothing waits for the device."""
    merge = merge or merge_device
    dev, world = fbuf.device, len(totals)
    ns, ms, ks = ([int(t[j]) for t in totals] for j in range(3))
    R, M, K = max(ns), max(ms), int(ibuf.shape[2])
    o_obb, o_tcls, L = layout(w, obb, R, M)
    if tuple(fbuf.shape) != (world, L) or tuple(ibuf.shape[:2]) != (world, 3) or max(ks) > K:
        raise RuntimeError(f"stats merge: buffers {tuple(fbuf.shape)} / {tuple(ibuf.shape)} do not fit the totals {totals}")
    n_img = sum(ks) if n_images_total is None else int(n_images_total)
    n, m = sum(ns), sum(ms)
    flat = fbuf.reshape(-1)
    cnt_rows, cnt_lab, ids = (ibuf[:, 0].to(torch.int32).contiguous(), ibuf[:, 1].to(torch.int32).contiguous(), ibuf[:, 2].contiguous())
    info = torch.zeros((3, INFO_WORDS), dtype=torch.int32, device=dev)
    rows = torch.empty((n, w), dtype=torch.float32, device=dev)
    img_rows = torch.empty(n_img, dtype=torch.int32, device=dev)
    merge(flat, w, L // w, ns, cnt_rows, ids, ks, n_img, w, rows, w, img_rows, info[0])
    rows_obb = None
    if obb:
        rows_obb = torch.empty_like(rows)
        merge(flat[o_obb:], w, L // w, ns, cnt_rows, ids, ks, n_img, w, rows_obb, w, None, info[1])
    tcls = torch.empty((m, 1), dtype=torch.float32, device=dev)
    img_labels = torch.empty(n_img, dtype=torch.int32, device=dev)
    merge(flat[o_tcls:], 1, L, ms, cnt_lab, ids, ks, n_img, 1, tcls, 1, img_labels, info[2])
    return Merged(rows, rows_obb, tcls.reshape(-1), img_rows, img_labels, info, (n, m, n_img), sum(ks))


def describe(info):
    """The (3, 4) info of merge_gathered, on the host -> None, or what went wrong (as shard.gather_results words it)."""
    for what, (flags, _, twice, run) in zip(("rows", "rows_obb", "target_cls"), info.tolist()):
        if flags & TWICE:
            return f"image {twice} produced by two ranks"
        if flags & BAD_ID:
            return "an image id outside [0, n_images_total)"
        if flags & RUN_TOTAL:
            return f"the per-image counts of rank {run} do not add up to its {what}"
        if flags & CAPACITY:
            return f"more {what} than the merged array holds"
    return None


def merge_parts(parts, w, obb, n_images_total=None, merge=None):
    """Shards that share one device (virtual ranks) -> Merged, through the layout of the exchange."""
    R, M, K = (max(int(x.shape[0]) for x in col) for col in zip(*[(p.rows, p.tcls, p.img_ids) for p in parts]))
    bufs = [pack(p, w, obb, R, M, K) for p in parts]
    totals = [(int(p.rows.shape[0]), int(p.tcls.shape[0]), int(p.img_ids.shape[0])) for p in parts]
    return merge_gathered(torch.stack([b[0] for b in bufs]), torch.stack([b[1] for b in bufs]), totals, w, obb, n_images_total, merge)


def _all_gather(t, world, group, device_collective):
    """(world,) + t.shape: every rank's t.  RCCL gathers device buffers in place; any other backend gets host tensors."""
    import torch.distributed as dist
    if device_collective:
        out = torch.empty((world,) + tuple(t.shape), dtype=t.dtype, device=t.device)
        dist.all_gather_into_tensor(out, t.contiguous(), group=group)
        return out
    host = t.cpu().contiguous()
    out = torch.empty((world,) + tuple(host.shape), dtype=host.dtype)
    dist.all_gather(list(out.unbind(0)), host, group=group)
    return out


def exchange(sh, w, obb, group=None, n_images_total=None, merge=None):
    """The one exchange of a sharded run: every rank hands in its Shard and gets the Merged statistics of all of them, on the
    device of its own shard.  First the three totals of every rank (they size the padding), then the two padded buffers; then
    merge_gathered, on every rank.  Without an initialised process group: the rank's own shard, through the same merge."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return merge_parts([sh], w, obb, n_images_total, merge)
    world = dist.get_world_size(group)
    dev = sh.rows.device
    on_device = dist.get_backend(group) == "nccl"
    mine = torch.tensor([int(sh.rows.shape[0]), int(sh.tcls.shape[0]), int(sh.img_ids.shape[0])], dtype=torch.int64,
                        device=dev if on_device else "cpu")
    totals = _all_gather(mine, world, group, on_device).tolist()
    R, M, K = (max(t[j] for t in totals) for j in range(3))
    f, i = pack(sh, w, obb, R, M, K)
    fbuf, ibuf = _all_gather(f, world, group, on_device), _all_gather(i, world, group, on_device)
    return merge_gathered(fbuf.to(dev), ibuf.to(dev), totals, w, obb, n_images_total, merge)
