"""Child process of tests/test_val_sharded_device_gpu.py: ONE rank of a sharded validation run with device metrics.

    python tests/helpers/val_sharded_rank.py <rank> <world> <port> <backend> <device index> <out.npz>

The parent imports this file too, for the data set, the stand-in model and its own world-1 run.  The data set has 10 images;
image i is named by its first pixel, the stand-in model reads that pixel and answers with seeded predictions of i alone (a small
head: 1,200 anchors, 15 classes), so an image's detections do not depend on the batch or the rank it lands in.  Half of the
objects the predictions are planted on are labels too; image 3 has no labels, image 4 no detections, image 7 neither."""
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests import synth                      # noqa: E402

N_IMAGES, NC, ANCHORS, N_OBJ, BATCH = 10, 15, 1200, 12, 4
NO_LABELS, NO_DETECTIONS = (3, 7), (4, 7)


def objects(i):
    """The planted objects of synth.s_pred(1, ANCHORS, NC, seed=300 + i, n_obj=N_OBJ): its first four draws, as label rows
    [cls cx cy l s theta]."""
    g = torch.Generator().manual_seed(300 + i)
    cxy = torch.rand(1, N_OBJ, 2, generator=g) * 1024.0
    lw = torch.stack((torch.rand(1, N_OBJ, generator=g) * 150 + 12, torch.rand(1, N_OBJ, generator=g) * 40 + 6), -1)
    obin = torch.randint(0, 180, (1, N_OBJ), generator=g)
    ocls = torch.randint(0, NC, (1, N_OBJ), generator=g)
    theta = (obin[0].float() - 90) / 180 * math.pi
    return torch.cat((ocls[0].float()[:, None], cxy[0], lw[0], theta[:, None]), 1)


class Set(torch.utils.data.Dataset):
    def __len__(self):
        return N_IMAGES

    def __getitem__(self, i):
        im = torch.full((3, 32, 32), 128, dtype=torch.uint8)
        im[0, 0, 0] = i
        lab6 = objects(i)[::2] if i not in NO_LABELS else torch.zeros(0, 6)
        lab = torch.cat((torch.zeros(lab6.shape[0], 1), lab6), 1)
        return im, lab, f"img{i}.png", ((1024, 1024), ((1.0, 1.0), (0.0, 0.0)))

    @staticmethod
    def collate_fn(batch):
        im, lab, path, shapes = zip(*batch)
        for k, l in enumerate(lab):
            l[:, 0] = k
        return torch.stack(im, 0), torch.cat(lab, 0), path, shapes


def loader():
    return torch.utils.data.DataLoader(Set(), batch_size=BATCH, shuffle=False, collate_fn=Set.collate_fn)


def model_on(dev):
    def model(im):
        out = []
        for b in range(im.shape[0]):
            i = int(round(float(im[b, 0, 0, 0]) * 255))
            out.append(synth.s_pred(1, ANCHORS, NC, seed=300 + i, n_obj=N_OBJ, fg_frac=0.0 if i in NO_DETECTIONS else 0.05))
        return (torch.cat(out, 0).to(dev),)
    return model


def run(dev, ldr):
    """val_sharded.run with the device tail, the oriented-box rows and a confusion matrix -> what the ranks must agree on."""
    from yolov5_obb_amd import val_sharded
    from yolov5_obb_amd.utils.metrics import ConfusionMatrix
    res = val_sharded.run(model_on(dev), ldr, n_total=N_IMAGES, conf_thres=0.25, iou_thres=0.45, half=False, device=dev,
                          device_metrics=True, obb_metrics=True, confusion_matrix=ConfusionMatrix(nc=NC, device=dev))
    out = {"seen": np.array(res["seen"]), "world": np.array(res["world"]), "matrix": res["confusion_matrix"].matrix,
           "rows": res["val_stats"].rows.cpu().numpy(), "rows_obb": res["val_stats"].rows_obb.cpu().numpy(),
           "tcls": res["val_stats"].target_cls.cpu().numpy(), "dt": np.array(res["dt"])}
    for key in ("metrics", "metrics_obb"):
        out[f"{key}_none"] = np.array(res[key] is None)
        for j, a in enumerate(res[key] or ()):
            out[f"{key}_{j}"] = a
    return out


def main(rank, world, port, backend, index, path):
    import torch.distributed as dist
    from yolov5_obb_amd import val_sharded
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dev = torch.device("cuda", index)
    torch.cuda.set_device(dev)
    dist.init_process_group(backend, rank=rank, world_size=world)
    try:
        out = run(dev, val_sharded.shard_loader(loader()))
        np.savez(path, **out)                                     # (every rank: the metrics are returned on all of them)
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main(int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], int(sys.argv[5]), sys.argv[6])
