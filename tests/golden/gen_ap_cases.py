"""Freezes outputs of the reference's OWN ap_per_class (utils/metrics.py:21-86) on the seeded inputs of tests/ap_cases.py
-> tests/golden/ap_cases.npz.  Needs a checkout of the reference (hukaixuan19970627/yolov5_obb): REF=<its directory>
    python tests/golden/gen_ap_cases.py REF                 write the golden file
    python tests/golden/gen_ap_cases.py REF --find-seeds    print, per case, the first seed that meets the conditions below
    python tests/golden/gen_ap_cases.py REF --time          seconds of the reference function on the timing inputs (this CPU)
np.argsort is wrapped to kind='stable' for the duration of every call: conf descending, ties by ascending row index is the
order this package pins; numpy's default (introsort) leaves ties in an unspecified order.  Only outputs are stored.

Every stored case must meet three conditions (else its seed in tests/ap_cases.py::SEEDS is changed):
 (a) no index k of the class-mean F1 curve has 0 < |mean_f1[k] - max| <= 1e-9 (the best index cannot hinge on a rounding);
 (b) r * n_l and tp / (p + eps) - tp are at least 1e-6 away from a half-integer for every class (neither can tp / fp);
 (c) mAP@0.5 lies strictly between 0.05 and 0.999 -- except the cases with n = 0 or m = 0, whose result is all zeros / empty
     by construction and which are there for exactly that."""
import importlib.util
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import ap_cases  # noqa: E402

EPS = 1e-16


def load_reference():
    dirs = [a for a in sys.argv[1:] if not a.startswith("--")]
    if len(dirs) != 1:
        sys.exit(__doc__)
    spec = importlib.util.spec_from_file_location("ref_metrics", os.path.join(dirs[0], "utils", "metrics.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def ref_ap_per_class(ref, tp, conf, pred_cls, target_cls):
    """(the reference's 7-tuple, the (nc, 1000) F1 curves) in the stable order.  The F1 curves are what the reference hands to
    its plot function: plot=True with both plot functions replaced by recorders."""
    seen = {}
    orig = np.argsort
    ref.plot_pr_curve = lambda *a, **k: None
    ref.plot_mc_curve = lambda px, py, path, names=(), xlabel='Confidence', ylabel='Metric': seen.__setitem__(ylabel, np.array(py))
    np.argsort = lambda a, *args, **kw: orig(a, kind='stable')
    try:
        out = ref.ap_per_class(tp, conf, pred_cls, target_cls, plot=True, save_dir='.', names={})
    finally:
        np.argsort = orig
    return out, seen["F1"]


def conditions(name, out, f1, target_cls):
    """The violated conditions of one case, as strings."""
    tp, fp, p, r, f1b, ap, uc = out
    bad = []
    cfg = ap_cases.CASES[name]
    mean = f1.mean(0)
    gap = np.abs(mean - mean.max())
    if ((gap > 0) & (gap <= 1e-9)).any():
        bad.append("a")
    nt = np.array([(target_cls == c).sum() for c in uc])
    for v in (r * nt, tp / (p + EPS) - tp):
        if (np.abs(np.abs(v - np.floor(v)) - 0.5) < 1e-6).any():
            bad.append("b")
    if cfg["n"] > 0 and cfg.get("m", 1) > 0 and not 0.05 < ap[:, 0].mean() < 0.999:
        bad.append("c")
    return bad


def run_case(ref, name, seed=None):
    cfg = dict(ap_cases.CASES[name])
    if seed is not None:
        cfg["seed"] = seed
    tp, conf, pred_cls, target_cls = ap_cases.build_raw(**cfg)
    if len(target_cls) == 0:           # the reference's argmax of an empty mean raises: val.py never calls it without labels
        return None, [], None
    out, f1 = ref_ap_per_class(ref, tp, conf, pred_cls, target_cls)
    return out, conditions(name, out, f1, target_cls), int(f1.mean(0).argmax())


def main():
    ref = load_reference()
    if "--time" in sys.argv:
        for n in (200_000, 4_000_000):
            args = ap_cases.timing_inputs(n)
            ts = []
            for _ in range(3):
                t0 = time.perf_counter()
                ref.ap_per_class(*args, plot=False, names={})
                ts.append(time.perf_counter() - t0)
            print(f"reference ap_per_class, n = {n}, 16 classes, 10 IoU levels: median {sorted(ts)[1]:.3f} s of {['%.3f' % t for t in ts]}")
        return
    if "--find-seeds" in sys.argv:
        for name in ap_cases.CASES:
            for seed in range(200):
                if not run_case(ref, name, seed)[1]:
                    print(name, seed)
                    break
            else:
                print(name, "NO SEED")
        return
    store = {}
    for name in ap_cases.CASES:
        out, bad, best = run_case(ref, name)
        assert not bad, (name, bad)
        if out is None:
            continue
        for key, val in zip(("tp", "fp", "p", "r", "f1", "ap", "classes"), out):
            store[f"{name}/{key}"] = val
        store[f"{name}/best"] = np.int64(best)
    np.savez_compressed(os.path.join(HERE, "ap_cases.npz"), **store)
    print(f"wrote tests/golden/ap_cases.npz: {len(store) // 8} cases")


if __name__ == "__main__":
    main()
