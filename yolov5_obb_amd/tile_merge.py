"""In-memory tile -> full-image merge: detections on a whole DOTA image without the text hand-off of the reference's workflow.

The reference splits a large image into tiles (DOTA_devkit/SplitOnlyImage_multi_process.py), runs the detector per tile, rounds
and writes the per-tile detections as JSON (val.py:50-66), rewrites them as ``Task1_<class>.txt``
(tools/TestJson2VocClassTxt.py) and merges those files per class (DOTA_devkit/ResultMerge_multi_process.py).  Here the list of
per-tile ``(n, 7)`` outputs of ``non_max_suppression_obb`` goes through ONE launch chain (``obb_tile_merge_f32``,
include/obb_hip.h) to the merged detections of the source images; the host reads back the counts.

Two deliberate properties:
  * tie rule: inside a (source image, class) segment the rows are processed by descending score -- with ``text_rounding`` the
    score as the text would print it -- and equal scores in ascending input row (tile order, then the row inside the tile).
    The reference's ``argsort()[::-1]`` leaves ties to numpy's sort; where a segment has no tie the result is the file
    pipeline's, bit for bit;
  * ``text_rounding=False`` keeps the full float32 precision of the polygons and scores, and therefore is NOT the file
    pipeline's result.

GPU only: no CPU fallback.
"""
import ctypes as C
import os

import numpy as np
import torch

from . import _lib

TEXT_ROUNDING, POLY_ALL = 1, 2          # OBB_TILE_MERGE_TEXT_ROUNDING, OBB_TILE_MERGE_POLY_ALL
_VARIANTS = {"poly_fast": 0, "poly_all": POLY_ALL}


class TileRec(C.Structure):
    """obb_tile_rec of include/obb_hip.h (one tile of obb_tile_merge_f32)."""
    _fields_ = [("src_image", C.c_int32), ("left", C.c_int32), ("up", C.c_int32), ("rate", C.c_double),
                ("pad_x", C.c_float), ("pad_y", C.c_float), ("gain", C.c_float)]


def split_origins(width, height, subsize=1024, gap=200):
    """Top-left corners [(left, up), ...] of the tiles of a width x height image, in the order the reference writes them
    (SplitOnlyImage_multi_process.py:66-83): columns left to right, rows top to bottom inside a column, a step of
    subsize - gap, the last tile of a row / column aligned to the border."""
    slide = subsize - gap
    if slide <= 0 or width <= 0 or height <= 0:
        raise ValueError(f"split_origins: subsize {subsize} > gap {gap} and a non-empty image expected")

    def starts(size):
        out, at = [], 0
        while True:
            if at + subsize >= size:
                out.append(max(size - subsize, 0))
                return out
            out.append(at)
            at += slide

    ups = starts(height)
    return [(left, up) for left in starts(width) for up in ups]


def tile_name(stem, rate, left, up):
    """The tile's name as the reference composes it (SplitOnlyImage_multi_process.py:58,74): stem__rate__left___up."""
    return f"{stem}__{rate}__{left}___{up}"


def merge_tiles(preds, tiles, nc, thresh=0.2, text_rounding=True, variant="poly_fast", n_src=None):
    """preds: the list non_max_suppression_obb returns, one (n_t, 7) float32 CUDA tensor [cx cy l s theta conf cls] per tile.
    tiles: one (src_image, left, up, rate, ratio_pad) per tile; ratio_pad None or ((gain, gain), (pad_x, pad_y)).
    Returns (rows (m, 11) float64 CUDA [8 source-image coordinates, score, cls, src_image] -- source image ascending, class
    ascending, processing order inside --, counts (n_src, nc) int64 on the host).  n_src: the number of source images
    (default: the largest src_image + 1).  One launch chain and one copy back."""
    if variant not in _VARIANTS:
        raise ValueError(f"merge_tiles: variant 'poly_fast' or 'poly_all' expected, got {variant!r}")
    if len(preds) != len(tiles):
        raise ValueError(f"merge_tiles: {len(preds)} predictions for {len(tiles)} tiles")
    if not torch.cuda.is_available():
        raise RuntimeError("yolov5_obb_amd merge_tiles needs a HIP device (no CPU fallback)")
    for p in preds:
        _lib.require_cuda(p, "pred")
        if p.dim() != 2 or p.shape[1] != 7 or p.dtype != torch.float32:
            raise RuntimeError(f"merge_tiles: every pred must be (n, 7) float32, got {tuple(p.shape)} {p.dtype}")
    ntile = len(tiles)
    if n_src is None:
        n_src = max((int(t[0]) for t in tiles), default=0) + 1
    dev = preds[0].device if ntile else torch.device("cuda", torch.cuda.current_device())
    recs = (TileRec * max(ntile, 1))()
    off = (C.c_int64 * (ntile + 1))()
    for t, (p, (src, left, up, rate, ratio_pad)) in enumerate(zip(preds, tiles)):
        gain, pad = (ratio_pad[0][0], ratio_pad[1]) if ratio_pad is not None else (1.0, (0.0, 0.0))
        recs[t] = TileRec(int(src), int(left), int(up), float(rate), float(pad[0]), float(pad[1]), float(gain))
        off[t + 1] = off[t] + int(p.shape[0])
    n = int(off[ntile])
    nseg = int(n_src) * int(nc)
    L = _lib.lib()
    with _lib.guard(dev):
        det7 = torch.cat([p for p in preds if p.shape[0]]).contiguous() if n else torch.zeros((0, 7), dtype=torch.float32, device=dev)
        out = torch.empty((n, 11), dtype=torch.float64, device=dev)
        tail = torch.empty(nseg + 1, dtype=torch.int64, device=dev)          # out_count (nseg) int64, then info (2) int32
        need = L.obb_tile_merge_workspace_bytes(n, int(n_src), int(nc))
        if need == 0:
            raise RuntimeError(f"merge_tiles: n = {n}, n_src = {n_src}, nc = {nc} is outside what obb_tile_merge_f32 accepts")
        ws = _lib.workspace(need, dev)
        flags = (TEXT_ROUNDING if text_rounding else 0) | _VARIANTS[variant]
        rc = L.obb_tile_merge_f32(_lib.ptr(det7), off, recs, ntile, int(n_src), int(nc), float(thresh), flags, _lib.ptr(out), _lib.ptr(tail),
                                  C.c_void_p(tail.data_ptr() + nseg * 8), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev))
        _lib.check(rc, "obb_tile_merge_f32")
        tail_h = tail.cpu().numpy()
    info = tail_h[nseg:].view(np.int32)
    if info[1]:
        raise _lib.NmsAborted("obb_tile_merge_f32: the NMS kernel aborted (a workgroup barrier timed out); results are invalid")
    if info[0]:
        raise RuntimeError(f"merge_tiles: a detection's class is not an integer in [0, {nc})")
    counts = tail_h[:nseg].reshape(int(n_src), int(nc)).copy()
    return out[:int(counts.sum())], counts


def write_task1(dstpath, rows, counts, image_names, class_names):
    """The merged Task1_<class>.txt files of merge_tiles' result, one per class with detections, in the text of the reference's
    mergesingle (ResultMerge_multi_process.py:218-233: confidence to 2 decimals, coordinates to 1) through the native writer.
    Lines: source image ascending, processing order inside.  Returns the paths written."""
    from .DOTA_devkit.ResultMerge_multi_process import format_result_line, format_result_text
    counts = np.asarray(counts)
    n_src, nc = counts.shape
    if len(image_names) != n_src or len(class_names) != nc:
        raise ValueError(f"write_task1: counts {counts.shape} for {len(image_names)} images and {len(class_names)} classes")
    rows_h = rows.cpu().numpy() if isinstance(rows, torch.Tensor) else np.asarray(rows)
    first = np.zeros(n_src * nc + 1, dtype=np.int64)
    first[1:] = np.cumsum(counts.reshape(-1))
    os.makedirs(dstpath, exist_ok=True)
    written = []
    for c in range(nc):
        if not counts[:, c].any():
            continue
        pick = np.concatenate([np.arange(first[s * nc + c], first[s * nc + c + 1]) for s in range(n_src)])
        names = [image_names[s] for s in range(n_src) for _ in range(int(counts[s, c]))]
        path = os.path.join(dstpath, f"Task1_{class_names[c]}.txt")
        dets = rows_h[pick, :9]
        # (str(round(v, d)) is the d-decimal string of the native writer while that string has <= 15 significant digits: mergesingle's rule)
        if np.isfinite(dets).all() and np.abs(dets[:, :8]).max(initial=0.0) < 1e14 and np.abs(dets[:, 8]).max(initial=0.0) < 1e13:
            text = format_result_text(names, dets)
        else:
            text = "".join(format_result_line(name, det) + "\n" for name, det in zip(names, dets.tolist())).encode()
        with open(path, "wb") as f:
            f.write(text)
        written.append(path)
    return written


def detect_large(model, image, nc, subsize=1024, gap=200, rate=1.0, batch=16, conf_thres=0.25, iou_thres=0.45, merge_thresh=0.2,
                 text_rounding=True, **nms_kwargs):
    """Detections on a whole large image: `image` is a (3, H, W) uint8 CUDA tensor ALREADY at `rate` (resizing stays with the
    caller: the reference's INTER_CUBIC is OpenCV's).  Tiles of split_origins are cropped on the device and zero-padded to
    subsize like saveimagepatches does (SplitOnlyImage_multi_process.py:37-45), go through `model` in batches of `batch` as
    float / 255 (the tile is the model's input: no letterbox), then non_max_suppression_obb, then merge_tiles.
    Returns merge_tiles' (rows, counts) for the one source image."""
    from .utils.general import non_max_suppression_obb
    _lib.require_cuda(image, "image")
    if image.dim() != 3 or image.shape[0] != 3 or image.dtype != torch.uint8:
        raise RuntimeError(f"detect_large: a (3, H, W) uint8 image expected, got {tuple(image.shape)} {image.dtype}")
    height, width = int(image.shape[1]), int(image.shape[2])
    origins = split_origins(width, height, subsize, gap)
    param = next(model.parameters(), None) if hasattr(model, "parameters") else None
    dtype = param.dtype if param is not None and param.is_floating_point() else torch.float32
    preds = []
    for b0 in range(0, len(origins), batch):
        part = origins[b0:b0 + batch]
        x = torch.zeros((len(part), 3, subsize, subsize), dtype=torch.uint8, device=image.device)
        for k, (left, up) in enumerate(part):
            crop = image[:, up:up + subsize, left:left + subsize]
            x[k, :, :crop.shape[1], :crop.shape[2]] = crop
        y = model(x.to(dtype) / 255)
        y = y[0] if isinstance(y, (tuple, list)) else y
        preds.extend(non_max_suppression_obb(y, conf_thres=conf_thres, iou_thres=iou_thres, **nms_kwargs))
    tiles = [(0, left, up, rate, None) for left, up in origins]
    return merge_tiles(preds, tiles, nc, thresh=merge_thresh, text_rounding=text_rounding, n_src=1)
