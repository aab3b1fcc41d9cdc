"""Shared by tests/test_stats_merge_host.py and tests/test_stats_merge_gpu.py: synthetic per-rank statistics whose every float
names its (image, row, column), the expected merge as a numpy permutation, and a numpy restatement of obb_stats_merge_f32 with
the signature of yolov5_obb_amd.stats_merge.merge_device (the stand-in the host test injects; the oracle of the GPU test)."""
import numpy as np
import torch

COUNTS = (0, 0, 1, 2, 65, 300)          # per-image row counts are drawn from these
BIG = 1500                              # ... plus one image of this many rows


def encode(image, rows, width):
    """(rows, width) float32 whose bit pattern is image << 16 | row << 5 | column: below 2^29, so never a NaN or an infinity, and
    distinct for image < 8192, row < 2048, column < 32.  Compare as uint32."""
    r, c = np.meshgrid(np.arange(rows, dtype=np.uint32), np.arange(width, dtype=np.uint32), indexing="ij")
    return ((np.uint32(image) << np.uint32(16)) | (r << np.uint32(5)) | c).astype(np.uint32).view(np.float32)


def image_counts(n_images, seed):
    """Rows of every image: COUNTS drawn with a seeded generator, and BIG for one image when there are at least three."""
    rng = np.random.RandomState(seed)
    cnt = rng.choice(COUNTS, size=n_images).astype(np.int64)
    if n_images >= 3:
        cnt[int(rng.randint(n_images))] = BIG
    return cnt


def assignment(n_images, world, shuffled, seed):
    """ids of every rank, in the order the rank holds them: the strided split, or a shuffled assignment of ids to ranks."""
    if not shuffled:
        return [np.arange(r, n_images, world, dtype=np.int64) for r in range(world)]
    rng = np.random.RandomState(seed + 1)
    perm = rng.permutation(n_images).astype(np.int64)
    cuts = np.sort(rng.randint(0, n_images + 1, size=world - 1)) if world > 1 else np.zeros(0, dtype=np.int64)
    return np.split(perm, cuts)


class Problem:
    """One call of the entry: src (world runs, run_stride rows apart, rows of src_stride floats, NaN-free garbage between them),
    counts / ids (world, K) with garbage in the padding, and the expected dst rows (total, width)."""

    def __init__(self, world, n_images, width, src_stride=None, shuffled=False, seed=0, slack_rows=3):
        self.world, self.n_images, self.width = world, n_images, width
        self.src_stride = src_stride or width
        cnt = image_counts(n_images, seed)
        self.ids = assignment(n_images, world, shuffled, seed)
        self.images_per_run = [len(a) for a in self.ids]
        self.rows_per_run = [int(cnt[a].sum()) for a in self.ids]
        self.K = max(self.images_per_run) + 2                     # (padding that must not be read)
        self.run_stride = max(self.rows_per_run) + slack_rows
        self.src = np.full((world, self.run_stride, self.src_stride), 0x3fc00000, dtype=np.uint32).view(np.float32)      # 1.5 everywhere
        self.counts = np.full((world, self.K), 123456, dtype=np.int32)
        self.img_id = np.full((world, self.K), -7, dtype=np.int64)
        for r, a in enumerate(self.ids):
            at = 0
            for j, i in enumerate(a):
                c = int(cnt[i])
                self.src[r, at:at + c, :width] = encode(i, c, width)
                self.counts[r, j], self.img_id[r, j] = c, i
                at += c
        self.count_by_id = cnt.astype(np.int32)
        self.total = int(cnt.sum())
        self.want = np.concatenate([encode(i, int(cnt[i]), width) for i in range(n_images)] + [np.zeros((0, width), np.float32)], 0)


def merge_numpy(src, src_stride, run_stride, rows_per_run, counts, img_id, images_per_run, n_images_total, width, dst, dst_stride,
                counts_out, info):
    """obb_stats_merge_f32 restated on CPU tensors (include/obb_hip.h): same arguments as stats_merge.merge_device, same info
    words, and like the entry it copies nothing when info[0] is set."""
    s = src.numpy().reshape(-1)
    cnt, ids = counts.numpy(), img_id.numpy()
    slot, flags, twice, bad_run = {}, 0, 0, 0
    for r, (nr, k) in enumerate(zip(rows_per_run, images_per_run)):
        at = 0
        for j in range(k):
            c, i = int(cnt[r, j]), int(ids[r, j])
            if c < 0:
                c, flags, bad_run = 0, flags | 4, r
            if not 0 <= i < n_images_total:
                flags |= 1
            elif i in slot:
                flags, twice = flags | 2, i
            else:
                slot[i] = (r * run_stride + at, c)
            at += c
        if at != nr:
            flags, bad_run = flags | 4, r
    total = sum(c for _, c in slot.values())
    if total > dst.shape[0]:
        flags |= 8
    by_id = np.zeros(n_images_total, dtype=np.int32)
    out = dst.numpy().reshape(-1)
    at = 0
    for i in range(n_images_total):
        first, c = slot.get(i, (0, 0))
        by_id[i] = c
        if not flags:
            for q in range(c):
                out[(at + q) * dst_stride:(at + q) * dst_stride + width] = s[(first + q) * src_stride:(first + q) * src_stride + width]
        at += c
    if counts_out is not None:
        counts_out[:n_images_total] = torch.from_numpy(by_id)
    info[:4] = torch.tensor([flags, total, twice, bad_run], dtype=torch.int32)


# ---- statistics of a run as val.ValStats holds them: (n, w) rows, rows_obb, target_cls and the per-image arrays
def image_stats(i, w):
    """rows (c, w), rows_obb (c, w), tcls (l) of image i: functions of i alone; images without rows, without labels, with neither."""
    c, l = (0, 3, 1, 0, 7, 2)[i % 6], (2, 0, 1, 0, 4)[i % 5]
    rows = encode(i, c, w)
    return rows, encode(i + 4096, c, w), np.arange(l, dtype=np.float32) + 100 * i


def shard_of(ids, w):
    """The yolov5_obb_amd.stats_merge.Shard (CPU tensors) of an accumulator that was fed the images `ids` in that order."""
    from yolov5_obb_amd.stats_merge import Shard
    per = [image_stats(int(i), w) for i in ids]
    cat = lambda k, shape: torch.from_numpy(np.concatenate([p[k] for p in per] + [np.zeros(shape, np.float32)], 0))
    return Shard(cat(0, (0, w)), cat(1, (0, w)), cat(2, (0,)), torch.tensor([len(p[0]) for p in per], dtype=torch.int32),
                 torch.tensor([len(p[2]) for p in per], dtype=torch.int32), torch.tensor([int(i) for i in ids], dtype=torch.int64))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- the argument refusals of the entry (host test: no device; gpu test: NULL device pointers)
def refusals():
    """(expected code, the arguments that differ from a valid call)."""
    return [(-1, dict(world=0)), (-1, dict(width=0)), (-1, dict(src_stride=11)), (-1, dict(dst_stride=11)), (-1, dict(rows=None)),
            (-1, dict(images=None)), (-1, dict(info=0)), (-1, dict(src=0)), (-1, dict(counts=0)), (-1, dict(img_id=0)), (-1, dict(dst=0)),
            (-1, dict(rows=[5, 9])), (-1, dict(images=[3, 1])), (-1, dict(n_images_total=-1)), (-1, dict(n_images_total=2 ** 31 - 1)),
            (-1, dict(rows=[2 ** 30, 2 ** 30], run_stride=2 ** 30)), (-2, dict(ws=0)), (-2, dict(ws=4096 + 8)), (-2, dict(ws=4096 + 128)),
            (-2, dict(short=1))]


def call_refused(L, C, world=2, width=12, src_stride=12, dst_stride=12, rows=(5, 8), images=(2, 2), info=4096, src=4096, counts=4096,
                 img_id=4096, dst=4096, n_images_total=4, run_stride=8, ws=4096, short=0, dst_rows=13):
    """One call that must be refused: 4096 stands for a device pointer that is never followed."""
    arr = lambda v: None if v is None else (C.c_int64 * len(v))(*v)
    need = L.obb_stats_merge_workspace_bytes(4)
    assert need > 0
    return L.obb_stats_merge_f32(C.c_void_p(src), src_stride, run_stride, arr(rows), C.c_void_p(counts), C.c_void_p(img_id), 2, arr(images),
                                 world, n_images_total, width, C.c_void_p(dst), dst_stride, dst_rows, None, C.c_void_p(info), C.c_void_p(ws),
                                 need - short, None)
