"""Time the in-memory DOTA Task-1 evaluation against the file path it replaces, in one process and from one seed.

    python tools/time_task1_rows.py [--images 100] [--dets 1500] [--classes 16] [--gt 60] [--windows 5] [--out FILE.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/time_task1_rows.py --only-rows 20      (the per-kernel split of (a))

The shape is the one the tile merge was timed on: merged rows of 100 source images x 1500 detections x 16 classes, a ground
truth of about 60 records per image.  Interleaved, median of `windows` windows:
  (a) evaluate_rows on a resident GroundTruth (one launch chain, one copy back; the window ends in that copy);
  (b) the same rows through write_task1 + evaluate: text files in a temporary directory, read back, one class at a time.
Both mAPs are printed: (b) sees the rows through mergesingle's second rounding (scores to 2 decimals, coordinates to 1), so they
agree only as far as that rounding allows: the tool fails (exit status 1, `maps_agree` / `rows_faster` in the JSON) when they
differ by more than kMapTol or when (a) is not faster than (b).  Needs a GPU; the last line of stdout is one JSON object."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


kMapTol = 0.01          # |mAP rows - mAP files| allowed for mergesingle's second rounding (see main)


def quads(cx, cy, w, h, t):
    c, s = np.cos(t), np.sin(t)
    cols = []
    for sx, sy in ((1, 1), (1, -1), (-1, -1), (-1, 1)):
        cols += [cx + sx * w / 2 * c - sy * h / 2 * s, cy + sx * w / 2 * s + sy * h / 2 * c]
    return np.stack(cols, 1)


def make_set(n_img, n_det, nc, n_gt, seed):
    """(rows (n, 11) sorted by (image, class), counts (n_img, nc), ground truth arrays): per image ~n_gt records on a 4000 px
    field; detections are jittered copies of them (some of another class) and clutter, scores favouring the copies."""
    rng = np.random.RandomState(seed)
    rows, bbox, gcls, gimg, gdiff = [], [], [], [], []
    for im in range(n_img):
        k = int(n_gt * (0.75 + 0.5 * rng.rand()))
        cx, cy = rng.rand(k) * 4000, rng.rand(k) * 4000
        w, h, t = rng.rand(k) * 70 + 10, rng.rand(k) * 25 + 6, (rng.rand(k) - 0.5) * np.pi
        c = rng.randint(0, nc, k)
        bbox.append(quads(cx, cy, w, h, t)); gcls.append(c); gimg.append(np.full(k, im)); gdiff.append(rng.rand(k) < 0.1)
        n_copy = n_det * 2 // 3
        src = rng.randint(0, k, n_copy)
        j = rng.randn(n_copy, 2) * (1 + 5 * rng.rand(n_copy, 1))
        dq = quads(cx[src] + j[:, 0], cy[src] + j[:, 1], w[src] * (1 + rng.randn(n_copy) * 0.08), h[src] * (1 + rng.randn(n_copy) * 0.08),
                   t[src] + rng.randn(n_copy) * 0.05)
        dc = np.where(rng.rand(n_copy) < 0.9, c[src], rng.randint(0, nc, n_copy))
        ds = np.clip(0.35 + 0.65 * rng.rand(n_copy), 0, 1)
        n_cl = n_det - n_copy
        cq = quads(rng.rand(n_cl) * 4000, rng.rand(n_cl) * 4000, rng.rand(n_cl) * 70 + 10, rng.rand(n_cl) * 25 + 6, (rng.rand(n_cl) - 0.5) * np.pi)
        q = np.concatenate([dq, cq]); cl = np.concatenate([dc, rng.randint(0, nc, n_cl)]); sc = np.concatenate([ds, rng.rand(n_cl) * 0.6])
        rows.append(np.concatenate([q, sc[:, None], cl[:, None].astype(np.float64), np.full((n_det, 1), float(im))], 1))
    rows = np.concatenate(rows)
    rows = rows[np.lexsort((-rows[:, 8], rows[:, 9], rows[:, 10]))]          # merge_tiles' order: image, class, score descending
    counts = np.zeros((n_img, nc), dtype=np.int64)
    np.add.at(counts, (rows[:, 10].astype(int), rows[:, 9].astype(int)), 1)
    return rows, counts, (np.concatenate(bbox), np.concatenate(gcls), np.concatenate(gimg), np.concatenate(gdiff))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=100)
    ap.add_argument("--dets", type=int, default=1500)
    ap.add_argument("--classes", type=int, default=16)
    ap.add_argument("--gt", type=int, default=60)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10, help="calls of (a) per window")
    ap.add_argument("--only-rows", type=int, default=0, help="run (a) this many times and nothing else (for a kernel trace)")
    ap.add_argument("--all-point", action="store_true", help="the all-point metric instead of the 11-point one")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/time_task1_rows.py needs a GPU"
    from yolov5_obb_amd.DOTA_devkit import dota_evaluation_task1 as EV
    from yolov5_obb_amd.tile_merge import write_task1
    dev = torch.device("cuda:0")
    m07 = not args.all_point
    rows_h, counts, (bbox, gcls, gimg, gdiff) = make_set(args.images, args.dets, args.classes, args.gt, args.seed)
    images = [f"P{i:04d}" for i in range(args.images)]
    classes = [f"class{c:02d}" for c in range(args.classes)]
    rows = torch.from_numpy(rows_h).to(dev)
    gt = EV.GroundTruth.from_arrays(bbox, gcls, gimg, gdiff, args.images, classes, images)

    def run_rows():
        return EV.evaluate_rows(rows, gt, use_07_metric=m07)                 # ends in the copy back: synchronous

    for _ in range(3):
        map_rows, _ = run_rows()
    if args.only_rows:
        for _ in range(args.only_rows):
            run_rows()
        torch.cuda.synchronize()
        print(json.dumps({"only_rows": args.only_rows, "nd": len(rows_h), "map_rows": map_rows}))
        return

    with tempfile.TemporaryDirectory() as td:
        os.makedirs(os.path.join(td, "labelTxt"))
        for i, name in enumerate(images):
            sel = gimg == i
            with open(os.path.join(td, "labelTxt", name + ".txt"), "w") as f:
                for q, c, d in zip(bbox[sel], gcls[sel], gdiff[sel]):
                    f.write(" ".join(repr(float(v)) for v in q) + f" {classes[c]} {int(d)}\n")
        with open(os.path.join(td, "imgnamefile.txt"), "w") as f:
            f.write("\n".join(images) + "\n")
        annopath, imagesetfile = os.path.join(td, "labelTxt", "{:s}.txt"), os.path.join(td, "imgnamefile.txt")
        res = os.path.join(td, "res")

        def run_files():
            write_task1(res, rows, counts, images, classes)
            return EV.evaluate(os.path.join(res, "Task1_{:s}.txt"), annopath, imagesetfile, classes, use_07_metric=m07)

        map_files, _ = run_files()                                           # warm-up of every shape the windows use
        ta, tb = [], []
        for _ in range(args.windows):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.reps):
                run_rows()
            t1 = time.perf_counter()
            run_files()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            ta.append((t1 - t0) / args.reps); tb.append(t2 - t1)
    a, b = statistics.median(ta), statistics.median(tb)
    print(f"rows {len(rows_h)}  records {len(bbox)}  metric {'11-point' if m07 else 'all-point'}")
    print(f"(a) evaluate_rows           median {a * 1e3:9.3f} ms   windows {[round(t * 1e3, 3) for t in ta]}")
    print(f"(b) write_task1 + evaluate  median {b * 1e3:9.3f} ms   windows {[round(t * 1e3, 3) for t in tb]}")
    print(f"mAP rows {map_rows:.6f}   mAP files {map_files:.6f}   (b) / (a) = {b / a:.1f}")
    # The text carries scores at 2 decimals and coordinates at 1: IoUs near ovthresh and the order of scores that now tie can move
    # single detections between TP and FP, nothing more.  kMapTol is far above that and far below a broken chain (a lost class
    # alone moves the mean by 1 / classes).
    maps_agree = abs(map_rows - map_files) <= kMapTol
    faster = a < b
    line = dict(nd=len(rows_h), ng=len(bbox), classes=args.classes, images=args.images, use_07_metric=m07, rows_ms=a * 1e3, files_ms=b * 1e3,
                ratio=b / a, map_rows=map_rows, map_files=map_files, maps_agree=bool(maps_agree), map_tol=kMapTol, rows_faster=bool(faster),
                rows_windows_ms=[t * 1e3 for t in ta], files_windows_ms=[t * 1e3 for t in tb])
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(line, f)
    print(json.dumps(line))
    if not maps_agree:
        print(f"FAILED: the two mAPs differ by {abs(map_rows - map_files):.6f} > {kMapTol}", file=sys.stderr)
    if not faster:
        print("FAILED: evaluate_rows is not faster than write_task1 + evaluate", file=sys.stderr)
    if not (maps_agree and faster):
        sys.exit(1)


if __name__ == "__main__":
    main()
