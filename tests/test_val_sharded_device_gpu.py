"""GPU: val_sharded.run(device_metrics=True, obb_metrics=True, confusion_matrix=...) on TWO ranks -- two fresh child processes
(tests/helpers/val_sharded_rank.py) that share the exchange of ValStats.all_gather and ConfusionMatrix.all_reduce -- must return,
on every rank, exactly what one process returns over the whole image list: metrics, metrics_obb, the matrix, and the merged rows
themselves.  gloo on one GPU (the exchange stages through the host); the RCCL variant needs two devices."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HELPER = os.path.join(ROOT, "tests", "helpers", "val_sharded_rank.py")
TIMEOUT = 240                            # seconds per child: interpreter start, HIP initialisation, three batches


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _two_ranks(tmp_path, backend, devices):
    """Both children, each under its time limit; if one fails or runs out of time both are killed and the test fails."""
    port = _free_port()
    paths = [str(tmp_path / f"rank{r}.npz") for r in range(2)]
    procs = [subprocess.Popen([sys.executable, HELPER, str(r), "2", str(port), backend, str(devices[r]), paths[r]], cwd=ROOT,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
    logs, failed = ["", ""], None
    try:
        for r, p in enumerate(procs):
            try:
                logs[r], _ = p.communicate(timeout=TIMEOUT)
            except subprocess.TimeoutExpired:
                failed = f"rank {r} ran out of time"
                break
            if p.returncode != 0:
                failed = f"rank {r} exited with {p.returncode}"
                break
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.communicate()
    assert failed is None, (failed, logs)
    return [dict(np.load(path)) for path in paths]


def _single(dev):
    from tests.helpers import val_sharded_rank as H
    return H.run(dev, H.loader())


def _same(got, want, rank):
    assert int(got["world"]) == 2 and int(got["seen"]) == int(want["seen"]) == 10
    assert sorted(got) == sorted(want), (rank, sorted(set(got) ^ set(want)))
    for key in want:
        if key not in ("world", "dt"):
            assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), (rank, key)


def _check(ranks, one):
    assert not bool(one["metrics_none"]) and not bool(one["metrics_obb_none"])
    assert float(one["metrics_5"][:, 0].mean()) > 0.0 and float(one["matrix"].sum()) > 0 and one["rows"].shape[0] > 20
    for r, got in enumerate(ranks):
        _same(got, one, r)
    assert np.array_equal(ranks[0]["dt"], ranks[1]["dt"])         # the slowest rank's, on both


def test_two_ranks_with_gloo_equal_one_process(dev, tmp_path):
    one = _single(dev)
    _check(_two_ranks(tmp_path, "gloo", (0, 0)), one)


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="RCCL needs one device per rank")
def test_two_ranks_with_rccl_equal_one_process(dev, tmp_path):
    one = _single(dev)
    _check(_two_ranks(tmp_path, "nccl", (0, 1)), one)
