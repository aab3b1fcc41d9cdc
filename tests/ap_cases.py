"""Seeded inputs of ap_per_class for tests/golden/ap_cases.npz (written by tests/golden/gen_ap_cases.py from the reference's own
utils/metrics.py with np.argsort pinned to kind='stable') -- the golden file stores outputs only, the inputs are rebuilt here.

build(name) -> (tp bool (n, niou), conf float32 (n), pred_cls float32 (n), target_cls float32 (m)), the arguments of
ap_per_class as val.py:269 concatenates them."""
import numpy as np

# name -> dict(seed, n, nc, m (default max(1, n // 8)), niou (default 10), ids (class id of builder class k), pred_ids
# (ids the predictions draw from, default ids), n_l (exact labels per class instead of random ones), conf (tie mode),
# reindex (seed of reindex_within_ties applied to tp and pred_cls))
CASES = {}
for _n in (0, 1, 63, 64, 65, 1023, 1024, 1025, 4097, 70001):          # wave, scan-tile (1024) and multi-tile boundaries
    for _nc in (1, 5):
        CASES[f"n{_n}_nc{_nc}"] = dict(seed=0, n=_n, nc=_nc)
for _nl in (7, 50, 100):                                               # recall k / n_l lands on the 101-point AP grid
    CASES[f"nl{_nl}"] = dict(seed=0, n=400, nc=3, n_l=_nl)
CASES.update({
    "labels_no_preds": dict(seed=0, n=300, nc=4, pred_ids=(0, 1, 3)),              # class 2: labels, no prediction
    "preds_no_labels": dict(seed=0, n=300, nc=3, ids=(0, 1, 2), pred_ids=(0, 1, 2, 5)),    # class 5: predictions, no label
    "sparse_ids": dict(seed=0, n=500, nc=4, ids=(0, 3, 9, 255)),
    "m0": dict(seed=0, n=50, nc=3, m=0),
    "niou1": dict(seed=0, n=300, nc=3, niou=1),
    "niou16": dict(seed=0, n=300, nc=3, niou=16),
    "ties_floor100": dict(seed=0, n=5000, nc=3, conf="floor100"),                  # numpy's default order differs by up to 8e-3
    "ties_all_equal": dict(seed=0, n=300, nc=3, conf="equal"),
    "ties_fp16": dict(seed=0, n=5000, nc=3, conf="fp16"),
    # ties_floor100 with the rows shuffled INSIDE every group of equal conf: another stable order, another golden
    "ties_floor100_reindexed": dict(seed=0, n=5000, nc=3, conf="floor100", reindex=1),
})
# seeds moved off 0 where gen_ap_cases.py's conditions (a) (b) (c) asked for it (gen_ap_cases.py REF --find-seeds)
SEEDS = {"n1_nc5": 8, "n63_nc1": 4}
for _k, _s in SEEDS.items():
    CASES[_k]["seed"] = _s

HOST_MAX_N = 4097          # tests/test_ap_math_host.py runs the cases up to this size


def build_raw(seed, n, nc, m=None, niou=10, ids=None, pred_ids=None, n_l=None, conf=None, reindex=None):
    rng = np.random.RandomState(seed)
    ids = np.arange(nc) if ids is None else np.asarray(ids)
    pred_ids = ids if pred_ids is None else np.asarray(pred_ids)
    m = max(1, n // 8) if m is None else m
    c = rng.rand(n).astype(np.float32)
    if conf == "floor100":
        c = (np.floor(c * 100) / 100).astype(np.float32)
    elif conf == "equal":
        c[:] = 0.5
    elif conf == "fp16":
        c = c.astype(np.float16).astype(np.float32)
    pred_cls = pred_ids[rng.randint(len(pred_ids), size=n)].astype(np.float32)
    if n_l is None:
        target_cls = ids[rng.randint(len(ids), size=m)].astype(np.float32)
    else:
        target_cls = np.repeat(ids, n_l).astype(np.float32)
    thr = np.linspace(0.2, 0.7, niou)
    tp = np.zeros((n, niou), dtype=bool)
    for j in range(niou):
        tp[:, j] = (rng.rand(n) * (0.4 + 0.6 * c)) > thr[j]
    if reindex is not None:
        order = reindex_within_ties(c, reindex)
        tp, pred_cls = tp[order], pred_cls[order]
    return tp, c, pred_cls, target_cls


def build(name):
    return build_raw(**CASES[name])


def timing_inputs(n, nc=16, niou=10, seed=0):
    """The inputs of tools/time_metrics.py and gen_ap_cases.py REF --time."""
    return build_raw(seed, n, nc, niou=niou)


def reindex_within_ties(conf, perm_seed):
    """A permutation of the rows that keeps conf's multiset in place but shuffles the rows inside every group of equal conf."""
    rng = np.random.RandomState(perm_seed)
    order = np.arange(len(conf))
    for v in np.unique(conf):
        at = np.flatnonzero(conf == v)
        order[at] = at[rng.permutation(len(at))]
    return order
