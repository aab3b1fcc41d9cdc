"""Every entry of include/obb_hip.h that takes `ws, ws_bytes`, called through the raw C ABI the way a C caller who follows
INTEGRATION.md calls it: a FRESH workspace of EXACTLY the queried size, every buffer of the call between 1 MiB canaries
(tests/abi_contract.py), the workspace pre-filled with zeros, with ones and with what another call of the entry left behind.
The three runs must give the oracle's result, bit for bit the same.  The same workspace one byte short, NULL or misaligned must
be refused with OBB_ERR_WORKSPACE before anything is written.  One size per entry runs again under obb_nms_set_max_grid(8)
(query and call sized from the same value) and on a side stream behind a delay (every launch, memset and copy on `stream`).

The sizes are the edges of the workspace carves (csrc/nms_driver.h: carve, csrc/nmsobb_impl.h: obb_carve): the grid block at
n = 8192, both implementations at n = 16384, grid_slots at 32768, cap_max(nseg) at nseg = 1 | 64 | 65, more segments than
teams, and the helper scratch of the small-segment kernel that aliases the edge lists.

Oracles: oracle.nms_rotated / nms_poly, oracle.pyref (merge variants, non_max_suppression_obb, the val.py tail, process_batch,
ComputeLoss), the host build of the confusion rules (tests/native/host_confusion.cpp) and tests/golden/ap_cases.npz -- the ones the
tests of each entry use, with their comparisons (exact everywhere except ap / p / r / f1 within 1e-12 and the loss scalars and
gradients within the bounds of tests/test_loss_configs_gpu.py).  The val.py-tail cases are axis-aligned (theta = 0), where the
host chain and the device agree in every bit (tests/test_valtail_dense_gpu.py).

The delay of the side-stream runs is sized from a measurement on an MI355X: the figures stand next to DELAY_ITERS."""
import ctypes as C
import dataclasses
import os
import re
import types

import numpy as np
import pytest
import torch

from tests import abi_contract as AC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu

# The delay in front of the real inputs on the side stream: DELAY_ITERS dependent 2048 x 2048 float32 products (17 GFLOP each).
# Measured on an MI355X, over the cases of representatives():
#   slowest enqueue (host time, perf_counter around the ctypes call)  2.674 ms  obb_nms_rotated_f32, n = 8192, the first call of the
#                                                                               process; 0.013 .. 0.095 ms for every later call
#   the delay (device time, events around it)                        50.3 ms   400 iterations, 0.126 ms each
# 50.3 / 2.674 = 18.8: the margin of five the host side of a shared machine is given, with room for a slower first call.
DELAY_N = 2048
DELAY_ITERS = 400

_vp = C.c_void_p


def vp(x):
    return _vp(int(x)) if x else _vp(0)


def L_():
    from yolov5_obb_amd import _lib
    return _lib.lib()


def cu_count():
    cu, wave = C.c_int(0), C.c_int(0)
    name = C.create_string_buffer(64)
    assert L_().obb_device_info(C.byref(cu), C.byref(wave), name, 64) == 0
    return cu.value


_memo = {}


def memo(key, fn):
    """Expected results are computed once and shared (read-only) by every test that needs them."""
    if key not in _memo:
        _memo[key] = fn()
    return _memo[key]


# ------------------------------------------------------------------------------------------------ single-list NMS
def _clustered(n, seed):
    from tests import synth
    dets, scores = synth.s_clustered(n, max(1, n // 10), seed)      # ~10 near-duplicates per object: the kept set is neither all nor one
    return dets, synth.tie_free(scores)


def rotated_case(n, max_keep=0, flags=0, f64=False, env=None):
    import oracle
    dets, scores = _clustered(n, 40 + n % 97)
    if flags:
        dets[::5, 2] = 0.0005                                      # OBB_NMS_DROP_SMALL: a fifth of the boxes is ignored
    if f64:
        dets, scores = dets.double(), scores.double()
    thr = 0.4

    def want():
        d, s = dets.numpy(), scores.numpy()
        if flags:
            valid = (dets[:, 2:4].min(1)[0] >= 0.001).numpy()
            ref = np.nonzero(valid)[0][oracle.nms_rotated(d[valid], s[valid], thr, threads=8)]
        else:
            ref = oracle.nms_rotated(d, s, thr, threads=8)
        return ref[:max_keep] if max_keep > 0 else ref
    entry = "obb_nms_rotated_f64" if f64 else "obb_nms_rotated_f32"
    name = f"{entry}-n{n}" + (f"-max{max_keep}" if max_keep else "") + ("-dropsmall" if flags else "") + \
        "".join(f"-{k}={v}" for k, v in (env or {}).items())

    def call(L, P, ws, wsb, st, mark):
        return getattr(L, entry)(vp(P["dets"]), vp(P["scores"]), n, thr, flags, max_keep, vp(P["keep_out"]), vp(P["num_keep"]), vp(ws), wsb, vp(st))

    def verify(O):
        ref = memo(name.split("-OBB")[0], want)
        num = O("num_keep", np.int64)
        keep = O("keep_out", np.int64)[:max(int(num[0]), 0)]
        assert int(num[0]) == len(ref) and np.array_equal(keep, ref), (name, int(num[0]), len(ref))
        if n > 2:
            assert 1 < len(ref) < n
        return [num, keep]
    return AC.Case(name, [entry], dict(dets=dets.numpy(), scores=scores.numpy()), dict(keep_out=n * 8, num_keep=8),
                   lambda L: L.obb_nms_workspace_bytes(n, 1, 3 if f64 else 0), call, verify, env=env)


def poly_case(n, row_stride=9):
    import oracle
    from tests import synth
    dets, scores = synth.s_clustered(n, max(1, n // 12), 7 + n % 89, extent=300.0)
    scores = synth.tie_free(scores)
    polys = torch.cat([synth.rbox_to_quad(dets), scores[:, None]], 1).contiguous()
    polys[::9, :8] = polys[::9, :8].reshape(-1, 4, 2).flip(1).reshape(-1, 8)            # some clockwise rings
    rows = polys if row_stride == 9 else torch.cat([polys, torch.full((n, row_stride - 9), float("nan"))], 1).contiguous()
    thr, name = 0.3, f"obb_nms_poly_f32-n{n}-stride{row_stride}"

    def call(L, P, ws, wsb, st, mark):
        return L.obb_nms_poly_f32(vp(P["polys"]), row_stride, n, thr, 0, vp(P["keep_out"]), vp(P["num_keep"]), vp(ws), wsb, vp(st))

    def verify(O):
        ref = memo(f"poly{n}", lambda: oracle.nms_poly(polys.numpy(), thr))
        num = O("num_keep", np.int64)
        keep = O("keep_out", np.int64)[:max(int(num[0]), 0)]
        assert int(num[0]) == len(ref) and np.array_equal(keep, ref), name
        return [num, keep]
    return AC.Case(name, ["obb_nms_poly_f32"], dict(polys=rows.numpy()), dict(keep_out=n * 8, num_keep=8),
                   lambda L: L.obb_nms_workspace_bytes(n, 1, 1), call, verify)


# ------------------------------------------------------------------------------------------------ merge NMS
MERGE = {2: ("obb_merge_nms_poly_f64", "merge_nms_poly_fast", 8), 4: ("obb_merge_nms_poly_all_f64", "merge_nms_poly_all", 8),
         5: ("obb_merge_nms_hbb_f64", "merge_nms_hbb", 4)}


def _segment_sizes(nseg):
    if nseg == 1:
        return [120]
    rng = np.random.RandomState(nseg)
    mid = rng.choice([0, 1, 2, 3, 5, 17, 64, 65, 130, 300], size=nseg - 2, p=[.1, .15, .15, .15, .15, .1, .08, .06, .04, .02]).tolist()
    if nseg > 2:
        mid[0] = 300                                               # sizes 0 .. 300, an empty segment first and last
    return [0] + mid + [0]


def merge_case(kind, nseg_spec):
    from oracle import pyref
    from tests.test_merge_gpu import _dets
    entry, ref_name, score_col = MERGE[kind]
    nseg = cu_count() + 44 if nseg_spec == "cu+44" else int(nseg_spec)
    sizes = _segment_sizes(nseg)
    segs = [_dets(m, 500 + 7 * g, 40 + 2 * m) if m else np.zeros((0, 9)) for g, m in enumerate(sizes)]
    dets = np.ascontiguousarray(np.concatenate(segs), dtype=np.float64)
    off = np.zeros(nseg + 1, dtype=np.int32)
    off[1:] = np.cumsum(sizes)
    n = int(off[-1])
    order = np.concatenate([s[:, score_col].argsort()[::-1] + off[g] for g, s in enumerate(segs)]).astype(np.int32)
    thr, name = 0.2, f"{entry}-nseg{nseg_spec}"

    def want():
        with np.errstate(all="ignore"):
            return [np.asarray(getattr(pyref, ref_name)(s, thr), dtype=np.int64) + off[g] for g, s in enumerate(segs)]

    def call(L, P, ws, wsb, st, mark):
        a = (vp(P["order"]), vp(P["seg_off"]), nseg, thr, vp(P["keep_out"]), vp(P["num_keep"]), vp(ws), wsb, vp(st))
        return L.obb_merge_nms_hbb_f64(vp(P["dets"]), 9, n, *a) if kind == 5 else getattr(L, entry)(vp(P["dets"]), n, *a)

    def verify(O):
        ref = memo(name, want)
        num, keep = O("num_keep", np.int64), O("keep_out", np.int64)
        assert num.tolist() == [len(r) for r in ref], name
        kept = [keep[off[g]:off[g] + num[g]] for g in range(nseg)]
        for g in range(nseg):
            assert np.array_equal(kept[g], ref[g]), (name, "segment", g)
        return [num] + kept
    return AC.Case(name, [entry], dict(dets=dets, order=order, seg_off=off), dict(keep_out=n * 8, num_keep=nseg * 8),
                   lambda L: L.obb_nms_workspace_bytes(n, nseg, kind), call, verify)


# ------------------------------------------------------------------------------------------------ fused NMS driver
MAX_DET, HEAD_SIZES = 300, (24, 12, 6)                            # A = 3 * (576 + 144 + 36) = 2268 anchors for the _head entry
FUSED_SHAPES = {"bs1_agn": (1, 15, 1), "bs2": (2, 15, 0), "bs5": (5, 15, 0), "bs20": (20, 16, 0)}      # nseg = 1, 30, 75, 320
FAST_HINT = 6144 | (1 << 32)                                      # in-LDS sort + the small-segment kernel: the host layer's first guess


def _decode_head_on_device(dev, convs, nc, half):
    """z of obb_detect_decode_levels (the tensor the _head entry is defined by, include/obb_hip.h), on the host."""
    from tests import synth
    L = L_()
    bs, no = convs[0].shape[0], 5 + nc + 180
    d = [c.to(dev) for c in convs]
    A = sum(3 * c.shape[2] * c.shape[3] for c in convs)
    z = torch.empty((bs, A, no), dtype=convs[0].dtype, device=dev)
    arr = (C.c_void_p * 3)(*[c.data_ptr() for c in d])
    ny = (C.c_int64 * 3)(*[c.shape[2] for c in convs]); nx = (C.c_int64 * 3)(*[c.shape[3] for c in convs])
    px = (C.c_float * 18)(*[float(v) for row in synth.DEFAULT_ANCHORS for v in row]); st = (C.c_float * 3)(*synth.DEFAULT_STRIDES)
    rc = L.obb_detect_decode_levels(3, arr, int(half), bs, 3, no, ny, nx, px, st, None, vp(z.data_ptr()), A, None,
                                    vp(torch.cuda.current_stream(dev).cuda_stream))
    assert rc == 0
    return z.cpu()


def _candidates(pred, conf, multi=True):
    """Largest candidate count of an image: rows with obj > conf, then the classes with obj * cls > conf (in the tensor's dtype)."""
    nc = pred.shape[2] - 185
    best = 0
    for x in pred:
        x = x[x[:, 4] > conf]
        c = x[:, 5:5 + nc] * x[:, 4:5]
        best = max(best, int((c > conf).sum()))
    return best


def fused_case(dev, entry, shape, half, packed, hint=0, cap=None, pred=None, tag="", env=None, conf=0.25):
    from oracle import pyref
    from tests import synth
    from yolov5_obb_amd.utils import general
    bs, nc, agn = FUSED_SHAPES[shape] if isinstance(shape, str) else shape
    no, dt = 5 + nc + 180, torch.float16 if half else torch.float32
    npdt = np.float16 if half else np.float32
    head = entry.endswith("_head")
    if head:
        convs = memo(("convs", bs, nc, half), lambda: synth.s_head(bs, nc, sizes=HEAD_SIZES, seed=60 + bs, n_obj=40, dtype=dt))
        z = memo(("z", bs, nc, half), lambda: _decode_head_on_device(dev, convs, nc, half))
        inputs = {f"conv{i}": c.numpy() for i, c in enumerate(convs)}
    else:
        z = pred if pred is not None else memo(("pred", bs, nc, half), lambda: synth.s_pred(bs, 2000, nc, seed=20 + bs, dtype=dt))
        inputs = dict(pred=z.numpy())
        if entry.endswith("_col") or entry.endswith("_st"):
            inputs["objcol"] = z[..., 4].contiguous().numpy()
    A = z.shape[1]
    kw = dict(conf_thres=conf, iou_thres=0.45, agnostic=bool(agn), multi_label=True, max_det=MAX_DET)
    cap_img = int(cap if cap is not None else min(A * nc, 65536))
    name = f"{entry}-{shape if isinstance(shape, str) else tag}-{'f16' if half else 'f32'}-{'packed' if packed else 'rows'}-hint{hint >> 32}" + \
        (f"-cap{cap}" if cap is not None else "") + "".join(f"-{k}={v}" for k, v in (env or {}).items())
    zkey = ("nms", tag or shape, head, half, conf)
    tail = (conf, 0.45, None, 0, agn, 1, MAX_DET, general._MAX_NMS, float(general._MAX_WH), None, 0, cap_img, hint)
    if head:
        ny = (C.c_int64 * 3)(*HEAD_SIZES); nx = (C.c_int64 * 3)(*HEAD_SIZES)
        px = (C.c_float * 18)(*[float(v) for row in synth.DEFAULT_ANCHORS for v in row]); sta = (C.c_float * 3)(*synth.DEFAULT_STRIDES)

    def call(L, P, ws, wsb, st, mark):
        o = (vp(P["out"]), packed, vp(P["out_count"]), vp(P["status"]), vp(ws), wsb)
        if head:
            arr = (C.c_void_p * 3)(P["conv0"], P["conv1"], P["conv2"])
            return L.obb_non_max_suppression_obb_head(3, arr, int(half), bs, 3, no, ny, nx, px, sta, *tail, *o, vp(P["state"]),
                                                      state_bytes(L) if P["state"] else 0, vp(st))
        if entry.endswith("_st"):
            return L.obb_non_max_suppression_obb_st(vp(P["pred"]), vp(P["objcol"]), int(half), bs, A, no, *tail, *o, vp(P["state"]), state_bytes(L), vp(st))
        if entry.endswith("_col"):
            return L.obb_non_max_suppression_obb_col(vp(P["pred"]), vp(P["objcol"]), int(half), bs, A, no, *tail, *o, vp(st))
        return L.obb_non_max_suppression_obb(vp(P["pred"]), int(half), bs, A, no, *tail, *o, vp(st))

    def state_bytes(L):
        return L.obb_nms_obb_state_bytes(bs)

    def verify(O):
        count, status = O("out_count", np.int64), O("status", np.int64)
        most = memo(zkey + ("cand",), lambda: _candidates(z, conf))
        assert int(status[1] & 0xffffffff) == most, (name, "largest candidate count", int(status[1] & 0xffffffff), most)
        if most > AC._up(cap_img, 64):                             # more candidates than slots: the count, and nothing else is promised
            assert int(status[0]) == most, (name, status.tolist())
            return [status]
        ref = memo(zkey, lambda: pyref.non_max_suppression_obb(z.clone(), **kw))
        assert int(status[0]) == 0 and count.tolist() == [int(r.shape[0]) for r in ref], (name, status.tolist(), count.tolist())
        assert sum(count.tolist()) > bs, name
        out = O("out", np.float32).reshape(bs * MAX_DET, 7)
        rows, at = [], 0
        for b, r in enumerate(ref):
            lo = at if packed else b * MAX_DET
            rows.append(out[lo:lo + len(r)].copy())
            at += len(r)
            assert rows[-1].tobytes() == r.float().numpy().tobytes(), (name, "image", b)
        return [count, status] + rows
    uses_state = entry.endswith("_st") or (head and packed)        # (_head: `state` may be NULL; both forms run)
    return AC.Case(name, [entry], inputs, dict(out=bs * MAX_DET * 7 * 4, out_count=bs * 8, status=16),
                   lambda L: L.obb_nms_obb_workspace_bytes(bs, cap_img, nc, agn), call, verify,
                   state_bytes=state_bytes if uses_state else None, env=env)


FUSED_ENTRIES = ["obb_non_max_suppression_obb", "obb_non_max_suppression_obb_col", "obb_non_max_suppression_obb_st",
                 "obb_non_max_suppression_obb_head"]
# pairwise over shape x entry x dtype x out_packed x hint: every entry meets both dtypes, both layouts and both kernel families
FUSED_TABLE = [(e, s, (i + j) % 2 == 1, int((i + j // 2) % 2 == 0), FAST_HINT if (i + 2 * j) % 3 else 0)
               for i, s in enumerate(FUSED_SHAPES) for j, e in enumerate(FUSED_ENTRIES)]


def overflow_case(dev):
    """cap_img below the candidate count of the image: status[0] is that count, and nothing outside the buffers is touched."""
    from tests import synth
    pred = memo("overflow_pred", lambda: _overflow_pred(synth))
    return fused_case(dev, "obb_non_max_suppression_obb", (1, 15, 0), False, 1, cap=4096, pred=pred, tag="overflow", conf=0.05)


def _overflow_pred(synth):
    pred = synth.s_pred(1, 2000, 15, seed=9, fg_frac=0.9)            # test_fused_nms_obb_candidate_overflow_retry's recipe at A = 2000
    pred[..., 4] = pred[..., 4].clamp(min=0.9)
    pred[..., 5:20] = pred[..., 5:20].clamp(min=0.5)                  # every class passes: 30,000 candidates > 4096 slots
    return pred


def helper_scratch_case(dev, packed, env):
    """Segment hint 1, bs * ncs = 8 segments (below the CU count), the largest between 256 and 384: the sort kernel hands large
    segments to helper workgroups whose lists live INSIDE the edge region of the workspace (nmsobb_impl.h: `have`)."""
    pred = memo("helper_pred", _helper_pred)
    return fused_case(dev, "obb_non_max_suppression_obb_col", (2, 4, 0), False, packed, hint=FAST_HINT, pred=pred, tag="helpers", env=env)


def _helper_pred():
    from tests import synth
    from tests.test_nmsobb_gpu import _set_class
    nc, A = 4, 6000                                              # test_large_segments_shared_by_several_workgroups at A = 6000
    pred = synth.s_pred(2, A, nc, seed=77, n_obj=40, fg_frac=0.01)
    g = torch.Generator().manual_seed(5)
    r0 = 3000
    for img, cls, cnt in ((0, 0, 100), (0, 1, 150), (0, 2, 215), (0, 3, 270), (1, 0, 320), (1, 2, 180), (1, 3, 245)):
        rows = torch.arange(r0, r0 + cnt)
        r0 += cnt
        k = max(1, cnt // 12)
        ctr = torch.rand(k, 2, generator=g) * 800 + 100
        which = torch.randint(0, k, (cnt,), generator=g)
        pred[img, rows, 0:2] = ctr[which] + torch.randn(cnt, 2, generator=g) * 6
        pred[img, rows, 2:4] = torch.tensor([80.0, 28.0]) * (1 + 0.1 * torch.randn(cnt, 2, generator=g))
        _set_class(pred, img, rows, cls, nc)
        pred[img, rows, 4] = 0.5 + 0.45 * torch.rand(cnt, generator=g)
        pred[img, rows, 5 + nc:] = 0.02
        pred[img, rows, 5 + nc + torch.randint(0, 180, (cnt,), generator=g)] = 0.9
    return pred


# ------------------------------------------------------------------------------------------------ val.py tail, metrics
NIOU = 10
TAIL_IMAGES = {"n0_nt0": [(0, 0, 2, 0, 0)], "n1_nt0": [(1, 0, 2, 0, 0)], "n0_nt7": [(0, 7, 2, 0, 0)], "n300_nt40": [(300, 40, 2, 3, 0)],
               "bs5": [(100, 30, 2, 2, 0), (0, 0, 1, 0, 0), (1, 1, 1, 0, 0), (129, 40, 2, 0, 0), (60, 0, 2, 0, 0)]}
PER_IMAGE = ["n0_nt0", "n1_nt0", "n0_nt7", "n300_nt40"]


def _tail_batch(name):
    from tests import valtail_cases as VC
    def make():
        preds, targets, shapes = VC.make_batch(80 + len(name), TAIL_IMAGES[name], axis=True)
        return preds, targets, shapes, VC.oracle_chain(preds, targets, shapes)
    return memo(("tail", name), make)


def _host_arrays(preds, shapes):
    bs = len(preds)
    off = (C.c_int64 * (bs + 1))(*np.concatenate(([0], np.cumsum([p.shape[0] for p in preds]))).tolist())
    flat = []
    for (h, w), ((gain, _), pad) in shapes:
        flat += (pad[0], pad[1], gain, w, h)
    return off, (C.c_float * len(flat))(*flat)


def tail_case(entry, name):
    from tests import valtail_cases as VC
    preds, targets, shapes, chain = _tail_batch(name)
    bs, n, nt = len(preds), sum(p.shape[0] for p in preds), int(targets.shape[0])
    off, img5 = _host_arrays(preds, shapes)
    rows_form, polled = entry.endswith("_rows_f32"), entry.endswith("_polled_f32")
    stride = 320                                                   # rows form: image b at row b * stride, NaN rows in the gaps
    if rows_form:
        det = torch.full((bs * stride, 7), float("nan"))
        for b, p in enumerate(preds):
            det[b * stride:b * stride + p.shape[0]] = p
        det_row = (C.c_int64 * bs)(*[b * stride for b in range(bs)])
    else:
        det = torch.cat(preds, 0)
    outs = dict(poly10=n * 40, hbb6=n * 24, polyn10=n * 40, hbbn6=n * 24)
    pinned = dict(stats=n * (NIOU + 2) * 4, done=8) if polled else None
    if not polled:
        outs["stats"] = n * (NIOU + 2) * 4

    def call(L, P, ws, wsb, st, mark):
        a = (bs, vp(P["targets"]), nt, 9, img5, vp(P["iouv"]), NIOU, vp(P["poly10"]), vp(P["hbb6"]), vp(P["polyn10"]), vp(P["hbbn6"]),
             vp(P["stats"]), vp(ws), wsb, vp(st))
        if rows_form:
            return L.obb_val_tail_batch_rows_f32(vp(P["det7"]), det_row, off, *a, None)
        if polled:
            return L.obb_val_tail_batch_polled_f32(vp(P["det7"]), off, *a, vp(P["done"]))
        return L.obb_val_tail_batch_f32(vp(P["det7"]), off, *a)

    def verify(O):
        got = [O("poly10", np.float32).reshape(n, 10), O("hbb6", np.float32).reshape(n, 6), O("polyn10", np.float32).reshape(n, 10),
               O("hbbn6", np.float32).reshape(n, 6)]
        stats = O("stats", np.float32).reshape(n, NIOU + 2)
        at = 0
        for b, (boxes, _, correct) in enumerate(chain):
            k = preds[b].shape[0]
            for g, w in zip(got, boxes):
                assert g[at:at + k].tobytes() == w.numpy().tobytes(), (entry, name, "boxes of image", b)
            want = torch.cat((correct.float(), preds[b][:, 5:7]), 1).numpy()
            assert stats[at:at + k].tobytes() == want.tobytes(), (entry, name, "stats of image", b)
            at += k
        res = got + [stats]
        if polled:
            done = O("done", np.int64)
            assert int(done[0]) == n, (name, int(done[0]))
        return res
    return AC.Case(f"{entry}-{name}", [entry], dict(det7=det.numpy(), targets=targets.numpy(), iouv=VC.IOUV.numpy()), outs,
                   lambda L: L.obb_val_tail_batch_workspace_bytes(n, nt), call, verify, pinned=pinned, index_inputs=("det7", "targets"))


def _one_image(name):
    preds, targets, shapes, chain = _tail_batch(name)
    boxes, lab, correct = chain[0]
    return boxes[3].contiguous(), lab.contiguous(), correct


def process_batch_case(name):
    from tests import valtail_cases as VC
    det, lab, correct = _one_image(name)
    n, m = det.shape[0], lab.shape[0]

    def call(L, P, ws, wsb, st, mark):
        return L.obb_process_batch_f32(vp(P["det6"]), n, vp(P["lab5"]), m, vp(P["iouv"]), NIOU, vp(P["correct"]), vp(ws), wsb, vp(st))

    def verify(O):
        got = O("correct", np.uint8).reshape(n, NIOU)
        assert np.array_equal(got, correct.numpy().astype(np.uint8)), name
        return [got]
    return AC.Case(f"obb_process_batch_f32-{name}", ["obb_process_batch_f32"], dict(det6=det.numpy(), lab5=lab.numpy(), iouv=VC.IOUV.numpy()),
                   dict(correct=n * NIOU), lambda L: L.obb_process_batch_workspace_bytes(n, m), call, verify, index_inputs=("det6", "lab5"))


_HC = []


@pytest.fixture(scope="module")
def host_confusion_lib(tmp_path_factory):
    """The host build of csrc/confusion_math.h (tests/native/host_confusion.cpp, pinned to the golden matrices by
    tests/test_confusion_host.py), by that module's own recipe: the oracle of the confusion cases."""
    from tests.test_confusion_host import build_host_confusion
    _HC.append(build_host_confusion(tmp_path_factory.mktemp("hc") / "libhostconfusion.so"))
    yield _HC[0]
    _HC.clear()


def host_confusion():
    assert _HC, "the test must request the host_confusion_lib fixture"
    return _HC[0]


CM_NC = 3


def _cm_prefill():
    return (np.arange((CM_NC + 1) ** 2 + 1, dtype=np.int64) * 7 + 3)       # a known non-zero matrix: the entry accumulates into it


def _cm_want(name, images):
    def make():
        H = host_confusion()
        _, _, _, chain = _tail_batch(name)
        mat = _cm_prefill()
        for b in images:
            boxes, lab, _ = chain[b]
            det = np.ascontiguousarray(boxes[3].numpy()); lb = np.ascontiguousarray(lab.numpy())
            assert H.hc_confusion(det, det.shape[0], lb, lb.shape[0], CM_NC, 0.25, 0.45, mat, 0) == 0
        return mat
    return memo(("cm", name, tuple(images)), make)


def confusion_case(entry, name):
    preds, targets, shapes, chain = _tail_batch(name)
    batch = entry == "obb_confusion_batch_f32"
    if batch:
        bs, n, nt = len(preds), sum(p.shape[0] for p in preds), int(targets.shape[0])
        off, img5 = _host_arrays(preds, shapes)
        inputs = dict(det7=torch.cat(preds, 0).numpy(), targets=targets.numpy())
    else:
        det, lab, _ = _one_image(name)
        n, nt = det.shape[0], lab.shape[0]
        inputs = dict(det6=det.numpy(), lab5=lab.numpy())

    def call(L, P, ws, wsb, st, mark):
        if batch:
            return L.obb_confusion_batch_f32(vp(P["det7"]), off, bs, vp(P["targets"]), nt, 9, img5, CM_NC, 0.25, 0.45, vp(P["matrix"]), vp(ws), wsb, vp(st))
        return L.obb_confusion_process_batch_f32(vp(P["det6"]), n, vp(P["lab5"]), nt, CM_NC, 0.25, 0.45, vp(P["matrix"]), vp(ws), wsb, vp(st))

    def verify(O):
        got = O("matrix", np.int64)
        want = _cm_want(name, range(len(preds)) if batch else [0])
        assert np.array_equal(got, want), (entry, name, np.flatnonzero(got != want).tolist())
        return [got]
    return AC.Case(f"{entry}-{name}", [entry], inputs, dict(matrix=_cm_prefill()), lambda L: L.obb_confusion_workspace_bytes(n, nt), call, verify, index_inputs=tuple(inputs))


AP_NAMES = ["n0_nc5", "n1_nc5", "m0", "n65_nc5", "n1025_nc5"]
NC_MAX = 256


def ap_case(name, curves=False):
    from tests import ap_cases
    tp, conf, pcls, tcls = ap_cases.build(name)
    n, niou, m = len(conf), tp.shape[1], len(tcls)
    rows = np.concatenate((tp.astype(np.float32), conf[:, None], pcls[:, None]), 1).astype(np.float32)
    outs = dict(ap=NC_MAX * niou * 8, prf=NC_MAX * 5 * 8, counts=2 * NC_MAX * 4, info=16)
    if curves:
        outs["curves"] = 3 * NC_MAX * 1000 * 8

    def call(L, P, ws, wsb, st, mark):
        return L.obb_ap_per_class_f32(vp(P["stats"]), niou + 2, n, niou, vp(P["target_cls"]), m, NC_MAX, vp(P["ap"]), vp(P["prf"]), vp(P["counts"]),
                                      vp(P["info"]), vp(P["curves"]) if curves else None, vp(ws), wsb, vp(st))

    def verify(O):
        from tests.test_metrics_gpu import KEYS, check_against
        ap, prf = O("ap", np.float64).reshape(NC_MAX, niou), O("prf", np.float64).reshape(NC_MAX, 5)
        counts, info = O("counts", np.int32).reshape(2, NC_MAX), O("info", np.int32)
        assert info[2] == 0 and info[3] == 0
        keep = np.flatnonzero(counts[0] > 0)
        assert np.array_equal(counts[0], np.bincount(tcls.astype(np.int64), minlength=NC_MAX))
        if m:
            assert int(info[1]) == int(tp[:, 0].sum())
            g = np.load(os.path.join(ROOT, "tests", "golden", "ap_cases.npz"))
            got = (prf[keep, 3].copy(), prf[keep, 4].copy(), prf[keep, 0].copy(), prf[keep, 1].copy(), prf[keep, 2].copy(), ap[keep].copy(),
                   keep.astype(np.int32))
            check_against(got, [g[f"{name}/{k}"] for k in KEYS], name)
            assert int(info[0]) == int(g[f"{name}/best"])
        else:
            assert not ap.any() and not prf.any()
        res = [ap, prf, counts, info]
        if curves:
            res.append(O("curves", np.float64))
        return res
    return AC.Case(f"obb_ap_per_class_f32-{name}" + ("-curves" if curves else ""), ["obb_ap_per_class_f32"], dict(stats=rows, target_cls=tcls), outs,
                   lambda L: L.obb_ap_per_class_workspace_bytes(n, niou, NC_MAX), call, verify, index_inputs=("stats", "target_cls"))


# ------------------------------------------------------------------------------------------------ training loss
LOSS_BASES = ["nl1_na1_nc1", "nl4_na4_nc200"]                     # the smallest of tests/loss_cases.py, and one with nl = 4
LOSS_TABLE = [(b, nt, half) for b in LOSS_BASES for nt in (0, 1, 50) for half in (False, True)]


def _loss_setup(dev, base, nt, half):
    from oracle import pyref
    from tests import loss_cases as LC
    from tests import synth
    from yolov5_obb_amd.utils.loss import ComputeLoss

    def make():
        case = dataclasses.replace(LC.BY_NAME[base], nt=nt, half=half)
        p, t = LC.random_inputs(case)
        ag, _, st = LC.head(case)
        cl = ComputeLoss(synth.FakeModel(case.nc, LC.hyp_of(case), dev, anchors=ag, strides=st))
        cl.sort_obj_iou = case.sort_obj_iou
        cfg = cl._config(p)
        spec = LC.spec_of(case)
        dt = torch.float16 if half else torch.float32
        ph = [x.to(dt) for x in p]
        ref_targets = pyref.build_targets(spec, p, t)
        pc = [x.float().clone().requires_grad_(True) for x in ph]         # the oracle sees the dtype-rounded logits
        lo, io = pyref.compute_loss(spec, pc, t.clone(), sort_obj_iou=case.sort_obj_iou)
        lo.backward()
        return case, cfg, ph, t, ref_targets, (lo.detach().numpy(), io.numpy(), pc)
    return memo(("loss", base, nt, half), make)


def loss_targets_case(dev, base, nt, half):
    """obb_loss_build_targets, then obb_loss_export_targets of every level on the workspace it filled (a chain that reads the
    counts back in between: synchronous by construction)."""
    case, cfg, ph, t, ref, _ = _loss_setup(dev, base, nt, half)
    ns = [int(r['b'].shape[0]) for r in ref]
    outs = dict(counts=9 * 4)
    for i, k in enumerate(ns):
        outs.update({f"idx{i}": k * 32, f"tbox{i}": k * 16, f"anch{i}": k * 8, f"tcls{i}": k * 8, f"csl{i}": k * 720})

    def call(L, P, ws, wsb, st, mark):
        rc = L.obb_loss_build_targets(C.byref(cfg), vp(P["targets"]), nt, 187, vp(P["counts"]), vp(ws), wsb, vp(st))
        mark()
        if rc:
            return rc
        torch.cuda.synchronize(dev)                               # the caller reads the counts before it sizes the exports
        got = P["_peek"]("counts", np.int32)
        assert got[:case.nl].tolist() == ns and got[8] == 0, (got.tolist(), ns)     # (the buffers are sized by the oracle's counts)
        for i, k in enumerate(ns):
            rc = L.obb_loss_export_targets(C.byref(cfg), nt, i, k, vp(P[f"idx{i}"]), vp(P[f"tbox{i}"]), vp(P[f"anch{i}"]), vp(P[f"tcls{i}"]),
                                           vp(P[f"csl{i}"]), vp(ws), wsb, vp(st))
            if rc:
                return rc
        return 0

    def verify(O):
        res = [O("counts", np.int32)[:case.nl].copy()]
        for i, r in enumerate(ref):
            idx = torch.stack((r['b'], r['a'], r['gj'], r['gi']), 1).numpy().astype(np.int64)
            for got, want in ((O(f"idx{i}", np.int64).reshape(-1, 4), idx), (O(f"tbox{i}", np.float32).reshape(-1, 4), r['tbox'].numpy()),
                              (O(f"anch{i}", np.float32).reshape(-1, 2), r['anch'].numpy()), (O(f"tcls{i}", np.int64), r['tcls'].numpy().astype(np.int64)),
                              (O(f"csl{i}", np.float32).reshape(-1, 180), r['csl'].numpy())):
                assert got.shape == want.shape and got.tobytes() == want.tobytes(), (base, nt, "level", i)
                res.append(got)
        return res
    return AC.Case(f"obb_loss_build_targets+export-{base}-nt{nt}-{'f16' if half else 'f32'}", ["obb_loss_build_targets", "obb_loss_export_targets"],
                   dict(targets=t.numpy()), outs, lambda L: L.obb_loss_workspace_bytes(C.byref(cfg), nt), call, verify, synchronous=True, index_inputs=("targets",))


def loss_step_case(dev, base, nt, half):
    """obb_loss_forward, then obb_loss_backward on the workspace the forward filled."""
    from tests.test_loss_gpu import check_grads
    case, cfg, ph, t, _, (lo, io, pc) = _loss_setup(dev, base, nt, half)
    nl = case.nl
    inputs = {f"p{i}": x.numpy() for i, x in enumerate(ph)}
    inputs.update(targets=t.numpy(), grad_scale=np.ones(1, dtype=np.float32))
    outs = dict(loss=(5 + nl) * 4)                                 # "loss_out (device, 5 + nl floats)"
    outs.update({f"g{i}": x.numel() * x.element_size() for i, x in enumerate(ph)})

    def call(L, P, ws, wsb, st, mark):
        parr = (C.c_void_p * nl)(*[P[f"p{i}"] for i in range(nl)])
        garr = (C.c_void_p * nl)(*[P[f"g{i}"] for i in range(nl)])
        rc = L.obb_loss_forward(C.byref(cfg), parr, int(half), vp(P["targets"]), nt, 187, vp(P["loss"]), vp(ws), wsb, vp(st))
        mark()
        if rc:
            return rc
        return L.obb_loss_backward(C.byref(cfg), parr, int(half), vp(P["targets"]), nt, 187, vp(P["grad_scale"]), garr, vp(ws), wsb, vp(st))

    def verify(O):
        loss = O("loss", np.float32)
        grads = [O(f"g{i}", np.float16 if half else np.float32).reshape(tuple(x.shape)) for i, x in enumerate(ph)]
        rt = 2e-3 if half else 1e-5                                # the bounds of tests/test_loss_configs_gpu.py:run_case
        assert np.allclose(loss[0:1], lo, rtol=rt, atol=0 if half else 1e-6), (loss, lo)
        assert np.allclose(loss[1:5], io, rtol=rt, atol=1e-5 if half else 1e-6), (loss, io)
        pg = [types.SimpleNamespace(grad=torch.from_numpy(g.copy()), dtype=torch.float16 if half else torch.float32, shape=g.shape) for g in grads]
        if half:
            check_grads(pg, pc, grtol=2e-3, atol=1e-7)
        else:
            check_grads(pg, pc)
        return [loss] + grads
    return AC.Case(f"obb_loss_forward+backward-{base}-nt{nt}-{'f16' if half else 'f32'}", ["obb_loss_forward", "obb_loss_backward"], inputs, outs,
                   lambda L: L.obb_loss_workspace_bytes(C.byref(cfg), nt), call, verify, index_inputs=("targets",))


# ------------------------------------------------------------------------------------------------ the table
ROT_SIZES = [1, 2, 65, 2049, 8191, 8192, 32768]
ROT32, ROT64, POLY, PB, AP = "obb_nms_rotated_f32", "obb_nms_rotated_f64", "obb_nms_poly_f32", "obb_process_batch_f32", "obb_ap_per_class_f32"
LOSS_T, LOSS_S = ("obb_loss_build_targets", "obb_loss_export_targets"), ("obb_loss_forward", "obb_loss_backward")


def table(dev):
    """[(test id, the header's entries the case calls, builder)]: built lazily, a case holds its inputs."""
    t = []

    def add(ident, entries, fn, *a, **k):
        t.append((ident, (entries,) if isinstance(entries, str) else tuple(entries), lambda: fn(*a, **k)))
    for n in ROT_SIZES:
        add(f"rotated_f32-n{n}", ROT32, rotated_case, n)
    for mk in ("0", "1"):                                          # n = 16384: the first size with two implementations, both
        add(f"rotated_f32-n16384-mk{mk}", ROT32, rotated_case, 16384, env={"OBB_NMS_MK": mk})
    add("rotated_f32-n8192-max_keep", ROT32, rotated_case, 8192, max_keep=100)
    add("rotated_f32-n2049-drop_small", ROT32, rotated_case, 2049, flags=1)
    for n in (1, 2049, 4097):
        add(f"rotated_f64-n{n}", ROT64, rotated_case, n, f64=True)
    for n in (1, 513, 2500):
        add(f"poly-n{n}", POLY, poly_case, n)
    add("poly-n513-stride11", POLY, poly_case, 513, row_stride=11)
    for kind in MERGE:
        for nseg in (1, 3, 64, 65, "cu+44"):
            add(f"{MERGE[kind][0][4:-4]}-nseg{nseg}", MERGE[kind][0], merge_case, kind, nseg)
    for e, s, half, packed, hint in FUSED_TABLE:
        add(f"{e[4:]}-{s}-{'f16' if half else 'f32'}-{'packed' if packed else 'rows'}-hint{hint >> 32}", e, fused_case, dev, e, s, half, packed, hint)
    add("non_max_suppression_obb-overflow", FUSED_ENTRIES[0], overflow_case, dev)
    add("non_max_suppression_obb_col-helpers-packed", FUSED_ENTRIES[1], helper_scratch_case, dev, 1, None)
    add("non_max_suppression_obb_col-helpers-sort_kernel", FUSED_ENTRIES[1], helper_scratch_case, dev, 0, {"OBB_NMS_SELF_SORT": "0"})
    for e in ("obb_val_tail_batch_f32", "obb_val_tail_batch_polled_f32", "obb_val_tail_batch_rows_f32"):
        for name in TAIL_IMAGES:
            add(f"{e[4:]}-{name}", e, tail_case, e, name)
    for name in PER_IMAGE:
        add(f"process_batch-{name}", PB, process_batch_case, name)
    for name in PER_IMAGE:
        add(f"confusion_process_batch-{name}", "obb_confusion_process_batch_f32", confusion_case, "obb_confusion_process_batch_f32", name)
    for name in TAIL_IMAGES:
        add(f"confusion_batch-{name}", "obb_confusion_batch_f32", confusion_case, "obb_confusion_batch_f32", name)
    for name in AP_NAMES:
        add(f"ap_per_class-{name}", AP, ap_case, name)
    add("ap_per_class-n65_nc5-curves", AP, ap_case, "n65_nc5", curves=True)
    for b, nt in [(b, nt) for b in LOSS_BASES for nt in (0, 1, 50)]:      # (build_targets takes no head dtype)
        add(f"loss_targets-{b}-nt{nt}", LOSS_T, loss_targets_case, dev, b, nt, False)
    for b, nt, half in LOSS_TABLE:
        add(f"loss_step-{b}-nt{nt}-{'f16' if half else 'f32'}", LOSS_S, loss_step_case, dev, b, nt, half)
    return t


TABLE = table(None)
N_CASES = len(TABLE)


def test_every_entry_with_a_workspace_is_in_the_table():
    """Host: the functions of include/obb_hip.h with a `ws_bytes` parameter are exactly the entries the table calls."""
    text = open(os.path.join(ROOT, "include", "obb_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    found = sorted(m.group(1) for m in re.finditer(r"\b(\w+)\s*\(([^;{}()]*)\)\s*;", text) if re.search(r"\bsize_t\s+ws_bytes\b", m.group(2)))
    in_table = sorted({e for _, entries, _ in TABLE for e in entries})
    assert len(found) >= 20 and found == in_table, (sorted(set(found) - set(in_table)), sorted(set(in_table) - set(found)))
    assert len({i for i, _, _ in TABLE}) == N_CASES


def test_a_misaligned_workspace_is_refused_without_a_device():
    """Host: ws + 8 and ws + 128 answer OBB_ERR_WORKSPACE where the aligned pointer passes the check, for one entry of every source
    file -- before any device call, so the pointers are never followed and no GPU is needed (the entries whose first device call
    would follow are only called with the misaligned pointers)."""
    if torch.cuda.is_available():
        # Only for a machine WITHOUT a device (-m "not gpu"): the addresses below are not memory, and nothing but the check under
        # test stands between them and a kernel.  With a device the same refusals run on real buffers (the gpu tests below).
        pytest.skip("a device is visible: the refusals are tested on real buffers by the gpu tests of this module")
    L = L_()
    p, null = 1 << 20, None
    for shift in (8, 128):
        ws = _vp(p + shift)
        need = L.obb_nms_workspace_bytes(100, 1, 0)
        assert L.obb_nms_rotated_f32(_vp(p), _vp(p), 100, 0.4, 0, 0, _vp(p), _vp(p), ws, need, null) == -2
        assert L.obb_nms_rotated_f64(_vp(p), _vp(p), 100, 0.4, 0, 0, _vp(p), _vp(p), ws, L.obb_nms_workspace_bytes(100, 1, 3), null) == -2
        assert L.obb_nms_poly_f32(_vp(p), 9, 100, 0.4, 0, _vp(p), _vp(p), ws, L.obb_nms_workspace_bytes(100, 1, 1), null) == -2
        assert L.obb_merge_nms_poly_f64(_vp(p), 100, _vp(p), _vp(p), 3, 0.2, _vp(p), _vp(p), ws, L.obb_nms_workspace_bytes(100, 3, 2), null) == -2
        assert L.obb_merge_nms_hbb_f64(_vp(p), 9, 100, _vp(p), _vp(p), 3, 0.2, _vp(p), _vp(p), ws, L.obb_nms_workspace_bytes(100, 3, 5), null) == -2
        need = L.obb_nms_obb_workspace_bytes(2, 4096, 15, 0)
        assert L.obb_non_max_suppression_obb(_vp(p), 0, 2, 2000, 200, 0.25, 0.45, null, 0, 0, 1, 300, 30000, 4096.0, null, 0, 4096, 0, _vp(p), 1,
                                             _vp(p), _vp(p), ws, need, null) == -2
        assert L.obb_non_max_suppression_obb_st(_vp(p), null, 0, 2, 2000, 200, 0.25, 0.45, null, 0, 0, 1, 300, 30000, 4096.0, null, 0, 4096, 0,
                                                _vp(p), 1, _vp(p), _vp(p), ws, need, _vp(p), L.obb_nms_obb_state_bytes(2), null) == -2
        off, img5 = (C.c_int64 * 2)(0, 9), (C.c_float * 5)(0, 0, 1, 800, 600)
        assert L.obb_val_tail_batch_f32(_vp(p), off, 1, _vp(p), 5, 9, img5, _vp(p), 10, null, null, null, null, _vp(p), ws,
                                        L.obb_val_tail_batch_workspace_bytes(9, 5), null) == -2
        assert L.obb_process_batch_f32(_vp(p), 9, _vp(p), 5, _vp(p), 10, _vp(p), ws, L.obb_process_batch_workspace_bytes(9, 5), null) == -2
        need = L.obb_confusion_workspace_bytes(9, 5)
        assert L.obb_confusion_batch_f32(_vp(p), off, 1, _vp(p), 5, 9, img5, 16, 0.25, 0.45, _vp(p), ws, need, null) == -2
        assert L.obb_confusion_process_batch_f32(_vp(p), 9, _vp(p), 5, 16, 0.25, 0.45, _vp(p), ws, need, null) == -2
        assert L.obb_confusion_process_batch_f32(_vp(p), 0, _vp(p), 5, 16, 0.25, 0.45, _vp(p), ws, need, null) == 0      # (nothing to do: no workspace needed)
        assert L.obb_ap_per_class_f32(_vp(p), 12, 100, 10, _vp(p), 10, 16, _vp(p), _vp(p), _vp(p), _vp(p), null, ws,
                                      L.obb_ap_per_class_workspace_bytes(100, 10, 16), null) == -2
        from yolov5_obb_amd.utils.loss import _LossConfig
        cfg = _LossConfig()
        cfg.nl, cfg.na, cfg.nc, cfg.no, cfg.bs = 1, 1, 1, 186, 1
        cfg.ny[0], cfg.nx[0], cfg.stride[0], cfg.balance[0], cfg.anchor_t = 4, 4, 8.0, 1.0, 4.0
        cfg.anchors[0][0][0], cfg.anchors[0][0][1] = 2.0, 1.0
        need = L.obb_loss_workspace_bytes(C.byref(cfg), 5)
        assert need > 0
        lv = (C.c_void_p * 1)(p)
        assert L.obb_loss_build_targets(C.byref(cfg), _vp(p), 5, 187, _vp(p), ws, need, null) == -2
        assert L.obb_loss_export_targets(C.byref(cfg), 5, 0, 3, _vp(p), _vp(p), _vp(p), _vp(p), _vp(p), ws, need, null) == -2
        assert L.obb_loss_forward(C.byref(cfg), lv, 0, _vp(p), 5, 187, _vp(p), ws, need, null) == -2
        assert L.obb_loss_backward(C.byref(cfg), lv, 0, _vp(p), 5, 187, _vp(p), lv, ws, need, null) == -2


def _build(dev, i):
    return table(dev)[i][2]()


def _donor(dev, i):
    """Another case of the same entry for the `leftover` fill: a neighbour in the table."""
    tab = table(dev)
    for j in sorted(range(len(tab)), key=lambda j: abs(j - i)):
        if j != i and tab[j][1] == tab[i][1]:
            return tab[j][2]()
    raise AssertionError("no other case of the entry")


def _env(monkeypatch, case):
    for k in ("OBB_NMS_MK", "OBB_NMS_SELF_SORT", "OBB_NMS_SMALL_HELPERS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)


@gpu
@pytest.mark.parametrize("i", range(N_CASES), ids=[t[0] for t in TABLE])
def test_exact_poisoned_workspace_between_canaries(dev, oracle_lib, host_confusion_lib, monkeypatch, i):
    case = _build(dev, i)
    _env(monkeypatch, case)
    AC.run_poisons(L_(), dev, case, _donor(dev, i))


# one case per entry (or chain) for the refusals and the two further conditions
def representatives(dev):
    return [lambda: rotated_case(8192), lambda: rotated_case(2049, f64=True), lambda: poly_case(513), lambda: merge_case(2, 65),
            lambda: merge_case(4, 3), lambda: merge_case(5, 64), lambda: fused_case(dev, FUSED_ENTRIES[0], "bs2", False, 1, FAST_HINT),
            lambda: fused_case(dev, FUSED_ENTRIES[1], "bs5", True, 0, 0), lambda: fused_case(dev, FUSED_ENTRIES[2], "bs2", False, 0, FAST_HINT),
            lambda: fused_case(dev, FUSED_ENTRIES[3], "bs2", True, 1, 0), lambda: tail_case("obb_val_tail_batch_f32", "bs5"),
            lambda: tail_case("obb_val_tail_batch_polled_f32", "n300_nt40"), lambda: tail_case("obb_val_tail_batch_rows_f32", "bs5"),
            lambda: process_batch_case("n300_nt40"), lambda: confusion_case("obb_confusion_batch_f32", "bs5"),
            lambda: confusion_case("obb_confusion_process_batch_f32", "n300_nt40"), lambda: ap_case("n1025_nc5"),
            lambda: loss_targets_case(dev, "nl4_na4_nc200", 50, False), lambda: loss_step_case(dev, "nl4_na4_nc200", 50, True)]


N_REP = len(representatives(None))
REP_IDS = ["rotated_f32", "rotated_f64", "poly", "merge_poly", "merge_poly_all", "merge_hbb", "fused", "fused_col", "fused_st", "fused_head",
           "val_tail", "val_tail_polled", "val_tail_rows", "process_batch", "confusion_batch", "confusion_process_batch", "ap_per_class",
           "loss_targets", "loss_step"]


@gpu
@pytest.mark.parametrize("ws_mode", ["short", "null", "+8", "+128"])
@pytest.mark.parametrize("k", range(N_REP), ids=REP_IDS)
def test_a_short_missing_or_misaligned_workspace_is_refused_before_anything_is_written(dev, oracle_lib, host_confusion_lib, monkeypatch, k, ws_mode):
    """ws_bytes - 1, ws = NULL, ws + 8 and ws + 128 -> OBB_ERR_WORKSPACE; every output still 0xC3, `state` still zero, the canaries
    and the workspace untouched.  (The alignment check sits next to the size check, in front of every launch and memset of the
    entry: a misaligned pointer never reaches a kernel.)"""
    case = representatives(dev)[k]()
    _env(monkeypatch, case)
    AC.run_refused(L_(), dev, case, ws_mode)


@gpu
def test_every_entry_was_refused(dev, oracle_lib, host_confusion_lib):
    got = set()
    for r in representatives(dev):
        got.update(r().entries)
    assert sorted(got) == sorted({e for _, entries, _ in TABLE for e in entries})


@gpu
def test_a_misaligned_state_is_refused(dev, oracle_lib, host_confusion_lib):
    case = fused_case(dev, FUSED_ENTRIES[2], "bs2", False, 0, FAST_HINT)
    inner = case.call
    case.call = lambda L, P, ws, wsb, st, mark: inner(L, dict(P, state=P["state"] + 128), ws, wsb, st, mark)
    r = AC.Run(L_(), dev, case)
    r.poison_ws("ff")
    assert r.run(torch.cuda.current_stream(dev).cuda_stream) == AC.OBB_ERR_WORKSPACE
    torch.cuda.current_stream(dev).synchronize()
    r.check()
    r.outputs_untouched()


@gpu
@pytest.mark.parametrize("k", range(N_REP), ids=REP_IDS)
def test_query_and_call_under_a_capped_grid(dev, oracle_lib, host_confusion_lib, monkeypatch, k):
    """obb_nms_set_max_grid(8) around the workspace query and the call (same thread; restored in a finally)."""
    case = representatives(dev)[k]()
    _env(monkeypatch, case)
    AC.run_capped(L_(), dev, case)


def _seed_matrix(dev):
    g = torch.Generator().manual_seed(1)
    return (torch.rand(DELAY_N, DELAY_N, generator=g) * 2e-3).to(dev)


@gpu
@pytest.mark.parametrize("k", range(N_REP), ids=REP_IDS)
def test_all_work_is_enqueued_on_the_callers_stream(dev, oracle_lib, host_confusion_lib, monkeypatch, k):
    case = representatives(dev)[k]()
    _env(monkeypatch, case)
    res, pending = AC.run_on_side_stream(L_(), dev, case, DELAY_ITERS, _seed_matrix(dev))
    if not case.synchronous:
        assert pending, "the delay had drained before the ABI call returned: the run proves nothing"
