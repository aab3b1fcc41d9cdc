"""Generate tests/golden/task1_rows_reference.npz from the REFERENCE ITSELF (run in the build container only):

    YOLOV5_CONFIG_DIR=/tmp/refcfg python tests/golden/gen_task1_rows_golden.py

What is frozen: rec, prec and both APs of the reference's own DOTA_devkit/dota_evaluation_task1.voc_eval -- imported in place the
way gen_golden.py does (load_reference; the SWIG module polyiou backed by the reference's polyiou.cpp compiled into oracle/_ref
and the other devkit stubs are the ones of gen_devkit_eval_cases.load_reference, shared, not copied)
-- on the TIE-FREE sets of tests/task1_rows_cases.py, per class with a result file.  The generator asserts that no class has two
equal scores: that is the condition under which np.argsort(-confidence), and with it the reference's result, is defined.
Data only; the GPU tests read the .npz and regenerate the inputs from seeds.
"""
import contextlib
import io
import os
import sys
import tempfile
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import task1_rows_cases as RC                           # noqa: E402
from tests.golden.gen_devkit_eval_cases import load_reference as devkit_stubs   # noqa: E402
from tests.golden.gen_golden import eval_write, load_reference     # noqa: E402


def main():
    load_reference()                                                   # sys.path / cwd of the reference, its stubs (builds oracle/_ref)
    devkit_stubs()                                                     # polyiou backed by oracle/_ref, matplotlib, numpy's removed aliases
    import DOTA_devkit.dota_evaluation_task1 as EV

    out = {}
    for name in RC.TIE_FREE:
        gt, det = RC.tie_free_set(name)
        total = 0
        for cls, lines in det.items():
            scores = [float(ln.split(' ')[1]) for ln in lines]
            assert len(set(scores)) == len(scores) and not np.isnan(scores).any(), (name, cls, "two equal scores: the reference's order is undefined")
            assert [repr(s) for s in scores] == [ln.split(' ')[1] for ln in lines], "the text must carry the doubles exactly"
            total += len(lines)
        if name == 'wide':
            assert total >= 2100 and len(RC.CLASSES[name]) == 3
        with tempfile.TemporaryDirectory() as td:
            detpath, annopath, imagesetfile = eval_write(td, gt, det)
            for cls in RC.CLASSES[name]:
                if not det.get(cls):
                    assert not os.path.exists(detpath.format(cls))
                    print(f"{name} {cls}: no detection, no result file (skipped by the reference's main loop)")
                    continue
                for m07 in (True, False):
                    with contextlib.redirect_stdout(io.StringIO()), warnings.catch_warnings(), np.errstate(all='ignore'):
                        warnings.simplefilter('ignore')
                        rec, prec, ap = EV.voc_eval(detpath, annopath, imagesetfile, cls, ovthresh=0.5, use_07_metric=m07)
                    out[f'{name}_{cls}_ap{int(m07)}'] = np.array(ap, dtype=np.float64)
                out[f'{name}_{cls}_rec'], out[f'{name}_{cls}_prec'] = rec, prec
                print(f"{name} {cls}: nd {len(rec)} ap07 {float(out[f'{name}_{cls}_ap1']):.4f} ap {float(ap):.4f} nan in rec {int(np.isnan(rec).sum())}")
    path = os.path.join(HERE, 'task1_rows_reference.npz')
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB, {len(out)} arrays)")


if __name__ == '__main__':
    main()
