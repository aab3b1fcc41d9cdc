"""Shared by tests/test_lazy_tta_gpu.py and tests/test_lazy_tta_abi_gpu.py: conv outputs of the passes of augmented inference with
planted confident cells, a stand-in model that hands them to forward_augment, and the eager chain the lazy path is held to.

The oracle for everything on the GPU is the eager path on the same device: _decode_tta (Detect.fused_tta) followed by
non_max_suppression_obb on that tensor.  The shapes are those of tests/test_tta_decode_gpu.py (CASES)."""
import torch
import torch.nn as nn

from tests.test_tta_decode_gpu import CASES, DTYPES, FLIPS, SCALES, make_detect  # noqa: F401  (re-exported)

KW = dict(conf_thres=0.25, iou_thres=0.45, multi_label=True, max_det=300)


def heads(case, dev, dtype, seed):
    """Per pass and level a conv output (bs, na*no, ny, nx) like tests/test_lazy_nms_gpu.py's _heads: background (objectness logit
    ~ N(-6, 1.5), class / angle ~ N(-4, 0.5)) plus confident cells with a class and a two-bin CSL tie -- at least 4 per image and
    map, one per 6 positions on the larger maps.  Every second planted cell gets a TWIN in the next column: the same channel vector
    with wide boxes (wh logit 2), so the two overlap, tie in confidence, and the NMS suppresses the one with the higher row."""
    nc, anchors, _, _, bs, maps = CASES[case]
    na, no = len(anchors[0]) // 2, nc + 185
    g = torch.Generator().manual_seed(seed)
    out = []
    for level_maps in maps:
        cs = []
        for ny, nx in level_maps:
            x = torch.randn(bs, na, ny, nx, no, generator=g) * 0.5
            x[..., 4] = torch.randn(bs, na, ny, nx, generator=g) * 1.5 - 6.0
            x[..., 5:] -= 4.0
            kk = max(4, ny * nx // 6)
            for b in range(bs):
                a = torch.randint(0, na, (kk,), generator=g)
                yy, xx = torch.randint(0, ny, (kk,), generator=g), torch.randint(0, nx, (kk,), generator=g)
                cls, ang = torch.randint(0, nc, (kk,), generator=g), torch.randint(0, 180, (kk,), generator=g)
                x[b, a, yy, xx, 4] = 1.0 + 3.0 * torch.rand(kk, generator=g)
                x[b, a, yy, xx, 5 + cls] = 1.5 + 2.0 * torch.rand(kk, generator=g)
                x[b, a, yy, xx, 5 + nc + ang] = 4.0
                x[b, a, yy, xx, 5 + nc + (ang + 1) % 180] = 4.0      # two equal bins: the first maximum decides
                for j in range(0, kk, 2):
                    if int(xx[j]) + 1 < nx:
                        x[b, a[j], yy[j], xx[j], 2:4] = 2.0
                        x[b, a[j], yy[j], xx[j] + 1] = x[b, a[j], yy[j], xx[j]]
            cs.append(x.permute(0, 1, 4, 2, 3).contiguous().view(bs, na * no, ny, nx).to(dtype).to(dev))
        out.append(cs)
    return out


class Passes(nn.Module):
    """A model as forward_augment sees one: `_forward_once` hands the head (identity Detect.m) the conv outputs of the next pass."""

    def __init__(self, det, convs):
        super().__init__()
        self.model = nn.ModuleList([det])
        self.stride = det.stride
        self.inplace = True
        self.convs, self.calls = convs, 0

    def _forward_once(self, x):
        cs = self.convs[self.calls % len(self.convs)]
        self.calls += 1
        return self.model[-1](list(cs))


def image(case, dev, dtype):
    h, w = CASES[case][3]
    return torch.zeros(CASES[case][4], 3, h, w, dtype=dtype, device=dev)


def augment(det, convs, case, scales, flips, **flags):
    """forward_augment on the passes' conv outputs with the given Detect flags (restored afterwards) -> z."""
    from yolov5_obb_amd.models.yolo import forward_augment
    model = Passes(det, convs)
    for k, v in flags.items():
        setattr(det, k, v)
    try:
        z, none = forward_augment(model, image(case, convs[0][0].device, convs[0][0].dtype), scales=scales, flips=flips)
    finally:
        for k in flags:
            delattr(det, k)
    assert none is None and model.calls == len(scales)
    return z


def eager(det, convs, case, scales, flips):
    """(z of _decode_tta, plan): the tensor the lazy output stands for."""
    from yolov5_obb_amd.models.yolo import _decode_tta, tta_plan
    plan = tta_plan([[tuple(c.shape[2:]) for c in cs] for cs in convs], det.na, det.nl)
    assert plan.on_boundary
    img = CASES[case][3]
    with torch.no_grad():
        return _decode_tta(det, convs, plan, list(scales), list(flips), img[0], img[1]), plan


def cpu_chain(case, convs, scales, flips):
    """The eager chain restated on the CPU in fp32 with the oracle's decode (oracle/pyref.py detect_decode) and the reference's
    torch ops -> (z, plan).  Only to hold the cases to their preconditions without a GPU; the GPU tests compare GPU with GPU."""
    from oracle import pyref
    from yolov5_obb_amd.models.yolo import _clip_rows, tta_plan
    nc, anchors, strides, img, bs, maps = CASES[case]
    nl, na, no = len(anchors), len(anchors[0]) // 2, nc + 185
    st = torch.tensor(strides, dtype=torch.float32)
    an = torch.tensor(anchors, dtype=torch.float32).view(nl, na, 2) / st.view(-1, 1, 1)
    y = []
    for cs, s, f in zip(convs, scales, flips):
        xs = [c.float().cpu().view(bs, na, no, c.shape[2], c.shape[3]).permute(0, 1, 3, 4, 2) for c in cs]
        p = pyref.detect_decode(xs, an, st)
        p[..., :4] /= s
        if f == 2:
            p[..., 1] = img[0] - p[..., 1]
        elif f == 3:
            p[..., 0] = img[1] - p[..., 0]
        y.append(p)
    lo, hi = _clip_rows([p.shape[1] for p in y], nl)
    plan = tta_plan(maps, na, nl)
    return torch.cat([p[:, a:b] for p, a, b in zip(y, lo, hi)], 1), plan


def preconditions(z, plan, out, flips, conf, na, maps):
    """On an eager z and its kept lists (multi-label): every listed (pass, level) entry has a row with obj > conf and obj * cls >
    conf; every pass has a kept detection from its row range (kept rows are matched to rows of z by exact box and confidence), one of
    them a flipped pass; 0 < kept < candidates.  Returns the figures (candidates, kept, kept per pass)."""
    nc = z.shape[2] - 185
    obj = z[..., 4]
    cls_conf = z[..., 5:5 + nc] * obj[..., None]                       # utils/general.py:820, in the tensor dtype
    cand = (obj[..., None] > conf) & (cls_conf > conf)
    bounds, at = [], 0
    for k, p in enumerate(plan.passes):
        for lv, off in zip(p.levels, p.offsets):
            rows = na * maps[k][lv][0] * maps[k][lv][1]
            assert bool(cand[:, off:off + rows].any()), f"pass {k} level {lv}: no row passes both thresholds"
        bounds.append((at, at + p.rows))
        at += p.rows
    assert at == z.shape[1]
    n_cand, n_kept = int(cand.sum()), sum(int(o.shape[0]) for o in out)
    from_pass = [0] * len(plan.passes)
    for b, o in enumerate(out):
        if not len(o):
            continue
        box = (o[:, None, :4] == z[b, None, :, :4].float()).all(-1)                              # (kept, rows)
        score = cls_conf[b].float()[:, o[:, 6].long()].t() == o[:, None, 5]                      # (kept, rows)
        hit = box & score
        assert bool(hit.any(1).all()), "a kept detection matches no row of the eager z"
        row = hit.float().argmax(1)
        for k, (lo, hi) in enumerate(bounds):
            from_pass[k] += int(((row >= lo) & (row < hi)).sum())
    assert all(n > 0 for (lo, hi), n in zip(bounds, from_pass) if hi > lo), from_pass
    assert any(n > 0 for n, f in zip(from_pass, flips) if f), "no kept detection comes from a flipped pass"
    assert 0 < n_kept < n_cand, (n_kept, n_cand)
    return n_cand, n_kept, from_pass


# the cases of tests/test_lazy_tta_gpu.py's bit-identity tests: (case, scales, flips, seed)
SEED = {"nc3_128": 11, "nc16_160x96": 12, "nl4_128": 13}
IDENTITY_CASES = [(c, SCALES, f, SEED[c]) for c in CASES for f in FLIPS] + [("nc3_128", (1, 0.85, 0.85), (None, 2, 3), 14)]


def same(a, b):
    assert len(a) == len(b)
    for i, (p, q) in enumerate(zip(a, b)):
        assert p.shape == q.shape and torch.equal(p, q), (i, p.shape, q.shape)
