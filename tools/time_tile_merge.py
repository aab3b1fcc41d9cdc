"""The in-memory tile merge (yolov5_obb_amd/tile_merge.py: merge_tiles, one launch chain) beside the file path it replaces
(mergebypoly on the same detections written as Task1 text: parse, group, numpy argsort, one device call per class file):
python tools/time_tile_merge.py [out.json]
Workload: 4 source images of 4000 x 4000 -> 100 tiles of 1024 with a 200 px overlap, ~1500 detections per tile, 16 classes
(150k rows, 64 segments of ~2300).  Both paths inside ONE run (the boxes of a pool differ by several percent): wall time of a
call that ends with its result on the host, warmed up, median of 30; next to it the device time of merge_tiles' launch chain
(events around the call) and merge_tiles + write_task1, the in-memory path's way to the same files."""
import json
import os
import shutil
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from tests import tile_merge_cases as TC
from yolov5_obb_amd import tile_merge as TM
from yolov5_obb_amd.DOTA_devkit import ResultMerge_multi_process as RM
from yolov5_obb_amd.val import val_postprocess

NC, N_SRC, SIZE, PER_IMAGE, REPS, WARM = 16, 4, 4000, 23000, 30, 3


def scene():
    rng = np.random.RandomState(1)
    tiles = [(s, l, u, 1.0, None) for s in range(N_SRC) for l, u in TC.origins(SIZE, SIZE)]
    objs = [np.concatenate([TC.objects(rng, PER_IMAGE // NC, c, SIZE, SIZE) for c in range(NC)]) for _ in range(N_SRC)]
    preds = [TC.sightings(rng, objs[t[0]], t, [0.0] * 4000) for t in tiles]
    # scores: distinct multiples of 1e-5 (+- 0.3e-5) inside every (image, class) segment, so that numpy's argsort in the file path has
    # no ties to order its own way and the two paths' files can be compared
    seg = np.concatenate([np.full(len(p), t[0] * NC) + p[:, 6].numpy().astype(np.int64) for p, t in zip(preds, tiles)])
    conf = np.zeros(len(seg))
    for g in np.unique(seg):
        at = np.flatnonzero(seg == g)
        conf[at] = (rng.choice(np.arange(5000, 99000), size=len(at), replace=False) + rng.uniform(-0.3, 0.3, len(at))) / 1e5
    at = 0
    for p in preds:
        p[:, 5] = torch.from_numpy(conf[at:at + len(p)].astype(np.float32))
        at += len(p)
    return preds, tiles


def wall_ms(fn):
    for _ in range(WARM):
        fn()
    ts = []
    for _ in range(REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def main():
    assert torch.cuda.is_available(), "time_tile_merge.py needs a GPU"
    dev = torch.device("cuda:0")
    preds, tiles = scene()
    preds = [p.to(dev) for p in preds]
    names = [f"P{s:04d}" for s in range(N_SRC)]
    classes = [f"class{c:02d}" for c in range(NC)]
    tmp = tempfile.mkdtemp(prefix="tile_merge_")
    src, dst, dst2 = os.path.join(tmp, "src"), os.path.join(tmp, "dst"), os.path.join(tmp, "dst2")
    os.makedirs(src)
    # the text the reference's workflow hands over: save_one_json's rounding, TestJson2VocClassTxt's lines
    files = {c: open(os.path.join(src, f"Task1_{classes[c]}.txt"), "w") for c in range(NC)}
    for p, (s, left, up, rate, _) in zip(preds, tiles):
        name = TM.tile_name(names[s], rate, left, up)
        for r in val_postprocess(p, ratio_pad=((1.0, 1.0), (0.0, 0.0)))[2].cpu().tolist():
            files[int(r[9])].write("%s %s %s %s %s %s %s %s %s %s\n" % (name, round(r[8], 5), *[round(x, 1) for x in r[:8]]))
    for f in files.values():
        f.close()
    n = sum(int(p.shape[0]) for p in preds)

    file_ms = wall_ms(lambda: RM.mergebypoly(src, dst))
    mem_ms = wall_ms(lambda: TM.merge_tiles(preds, tiles, NC, n_src=N_SRC))
    both_ms = wall_ms(lambda: TM.write_task1(dst2, *TM.merge_tiles(preds, tiles, NC, n_src=N_SRC), names, classes))
    dev_ts = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        TM.merge_tiles(preds, tiles, NC, n_src=N_SRC)
        b.record()
        b.synchronize()
        dev_ts.append(a.elapsed_time(b))
    rows, counts = TM.merge_tiles(preds, tiles, NC, n_src=N_SRC)
    same = all(open(os.path.join(dst, f)).read() == open(os.path.join(dst2, f)).read() for f in sorted(os.listdir(dst)))
    out = {"workload": f"{len(tiles)} tiles, {n} detections, {NC} classes, {N_SRC} source images; {int(counts.sum())} merged rows",
           "file_path_mergebypoly_ms": {"median": file_ms[0], "min": file_ms[1], "max": file_ms[2]},
           "merge_tiles_ms": {"median": mem_ms[0], "min": mem_ms[1], "max": mem_ms[2]},
           "merge_tiles_plus_write_task1_ms": {"median": both_ms[0], "min": both_ms[1], "max": both_ms[2]},
           "merge_tiles_device_ms": {"median": float(np.median(dev_ts)), "min": float(min(dev_ts)), "max": float(max(dev_ts))},
           "ratio_file_over_merge_tiles": file_ms[0] / mem_ms[0], "ratio_file_over_merge_tiles_plus_write": file_ms[0] / both_ms[0],
           "files_identical_to_mergebypoly": bool(same), "reps": REPS}
    shutil.rmtree(tmp)
    text = json.dumps(out, indent=1)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
