"""GPU: the filter kernel (csrc/nmsobb_front.h: k_decode) at two and four rows per thread, and the sorts behind it on tie words that
need their fourth byte, against oracle/pyref.py -- bit for bit and in the same order (torch.equal per image, no tolerance).

The host plan (csrc/nms_plan.h: plan_nms_obb) picks the rows per thread G from bs * A: 1 below 491,520 rows, 2 below 983,040,
then 4.  The smaller tests of the kernel (tests/test_decode_rowload_gpu.py, tests/test_decode_state_gpu.py) run at G = 1.  The
shapes here (tests/decode_big_cases.py: SHAPES) are the smallest that reach each G and each of its boundaries; the tensors are
zeros plus planted rows, chosen from the kernel's row map: both ends of the image, one workgroup planted in full (512 G listed
rows: at G = 4 its LDS row list is exactly full and its waves flush their stage many times), every q slot of two further
workgroups.  What G a shape gets is asserted on the host from tests/test_host_index_maps.py: _rows_per_thread
(tests/test_decode_big_cases_host.py); tests/test_nms_plan_host.py holds the library's plan to that formula.  The device itself
does not report G.

A call of a shape whose hints were cleared starts from the library's optimistic first-call hints (the in-LDS sort), so every
sequence here says which sort it wants: `_run` of tests/test_decode_rowload_gpu.py for the filter cases (the filter kernel is the
same launch on every path), hint_set(cand=0) in front of the tie cases (the radix sort of segsort.h for bs = 2, the three-launch
sort of psrs_sort.h for bs = 1, then two hinted calls).

Seconds per case on an MI355X (the oracle's reference included where the case is the first to ask for it; the first case of a
process also loads the library):

  rows_equal_the_oracle   g1_top 0.40   g2_floor 0.12   g2_tail f32 0.16, f16 0.12, bf16 0.12   g2_top 0.16   g4_floor 0.36
                          g4_tail f32 0.45, f16 0.37, bf16 0.38   g4_nc33 0.35
  between_nans            g2_tail 0.11 / 0.01   g4_tail 0.01 / 0.01 (lead 64 / 65)
  counts_exact            0.11
  tie_byte3               0.22

The whole file: under 6 s.  Seen by the two skip-work mutants it was written against: `q < G - 1` for G > 1 in k_decode fails every
case here but g1_top (and no test at G = 1); a radix mask without key byte 3 on the single-list branch fails tie_byte3 at its
first call (agnostic, bs = 2) and the plan's own host test."""
import pytest
import torch

from tests import decode_big_cases as BC
from tests.test_decode_rowload_gpu import _cmp, _run
from tests.test_decode_state_gpu import MAX_DET, Buffers, _tail, vp

pytestmark = pytest.mark.gpu

KW = BC.KW          # max_det = 4500: above every case's candidate count, so no kept row is cut and every planted row shows


@pytest.mark.parametrize("name,dt", BC.CASES)
def test_rows_equal_the_oracle(dev, oracle_lib, name, dt):
    from yolov5_obb_amd.utils import general
    bs, A, nc = BC.SHAPES[name][:3]
    ref_multi, ref_best = BC.reference(name, dt)
    pred = BC.case(name, dt, device=dev)
    # nc = 2: the full workgroup alone gives a class more than 384 candidates (the persistent kernel); nc = 33: the small-segment kernel
    _run(dev, pred, ref_multi, ref_best, (name, dt), nc, expect_small=nc > 2, kw=KW)
    if nc > 2:
        assert 0 < general.hint_get(dev, A, nc, False, KW["conf_thres"])["seg"] <= general._SEG_SMALL
    general.hints_clear()
    general.hint_set(dev, A, nc, True, KW["conf_thres"], cand=0)      # hint 0: the radix sort (bs 2) / the three-launch sort (bs 1)
    _cmp(general.non_max_suppression_obb(pred, multi_label=True, **KW), ref_multi, (name, dt, "hint 0"))
    del pred
    torch.cuda.empty_cache()


@pytest.mark.parametrize("lead", [64, 65])
@pytest.mark.parametrize("name", ["g2_tail", "g4_tail"])
def test_between_nans(dev, oracle_lib, name, lead):
    """The tensor is an exact-size view inside a device buffer of NaNs, `lead` elements in front (65: a base address that is only
    element-aligned).  Rows 0 and A - 1 of both images pass.  A lane without a row (q >= G, or behind row A - 1) must not reach past
    the image: a NaN read as objectness fails the filter silently, one read as an angle bin or class score would win its arg-max."""
    bs, A, nc = BC.SHAPES[name][:3]
    ref_multi, ref_best = BC.reference(name, "f16")
    assert all(r.shape[0] > 0 for r in ref_multi)
    n = bs * A * (nc + 185)
    buf = torch.full((lead + n + 4096,), float("nan"), dtype=torch.float16, device=dev)
    view = buf[lead:lead + n].view(bs, A, nc + 185)
    view.zero_()
    for b, (rows, vals) in enumerate(BC.planted(bs, A, nc, torch.float16, BC.seed_of(name))):
        view[b, rows.to(dev)] = vals.to(dev)
    assert view.is_contiguous() and view.data_ptr() == buf.data_ptr() + lead * buf.element_size()
    _run(dev, view, ref_multi, ref_best, ("between NaNs", name, lead), nc, expect_small=False, kw=KW)
    assert bool(torch.isnan(buf[:lead]).all()) and bool(torch.isnan(buf[lead + n:]).all())
    del view, buf
    torch.cuda.empty_cache()


def test_counts_exact(dev, oracle_lib):
    """The candidate counters of the filter kernel at G = 4 (one atomic per full wave stage plus one per workgroup), through the C
    entry and independently of the NMS.  include/obb_hip.h: an image that produces more candidates than cap_img makes status[0]
    that count (the largest of any image: csrc/nmsobb_impl.h writes the maximum); status[1] bits 0..31 are the largest candidate
    count of any image.  Both are the number of (row, class) pairs with obj > thr and obj * cls > thr in the input dtype."""
    from yolov5_obb_amd import _lib
    L = _lib.lib()
    name = "g4_tail"
    bs, A, nc = BC.SHAPES[name][:3]
    kw = dict(KW, agnostic=False, multi_label=True, max_det=MAX_DET)
    ref = [r[:MAX_DET] for r in BC.reference(name, "f16")[0]]      # (the oracle cuts its kept list at max_det: the first rows of the uncut one)
    assert ref[0].shape[0] == MAX_DET
    host = BC.case(name, "f16")
    counts = [c for c, _ in BC.candidate_counts(host, multi_label=True)]
    largest = max(counts)
    small_cap, cap = 1024, 4096
    assert small_cap < counts[0] == largest <= cap and counts[1] < small_cap
    d = host.to(dev)
    del host
    B = Buffers(dev, L, [(bs, small_cap, nc, 0), (bs, cap, nc, 0)])
    st = torch.cuda.current_stream(dev).cuda_stream

    def call(cap_img, hint):
        B.count.fill_(-7)
        B.status.fill_(-7)
        rc = L.obb_non_max_suppression_obb_col(vp(d.data_ptr()), vp(0), 1, bs, A, nc + 185, *_tail(kw, cap_img, hint), vp(B.out.data_ptr()), 0,
                                               vp(B.count.data_ptr()), vp(B.status.data_ptr()), vp(B.ws.data_ptr()), B.ws_bytes, vp(st))
        assert rc == 0, (cap_img, hint, rc)
        torch.cuda.synchronize()
        return B.status.cpu().tolist()

    status = call(small_cap, 0)
    assert status[0] == largest, ("overflow", status, counts)
    for hint in (0, 6144 | (1000 << 32)):                     # the radix sort; the in-LDS sort in front of the persistent kernel
        status = call(cap, hint)
        B.results(bs, ref, ("sufficient cap_img", hint))
        assert status[1] & 0xFFFFFFFF == largest, (hint, status, counts)
    del d
    torch.cuda.empty_cache()


def _three_calls(dev, pred, ref, what, **kw):
    """hint 0 in front of the first call: the radix sort (several images) or the three-launch sort (one image); the second and third
    call run on what the first reported."""
    from yolov5_obb_amd.utils import general
    A, nc = pred.shape[1], pred.shape[2] - 185
    general.hints_clear()
    general.hint_set(dev, A, nc, kw["multi_label"], KW["conf_thres"], cand=0)
    for rep in range(3):
        got = general.non_max_suppression_obb(pred, **KW, **kw)
        _cmp(got, ref, (what, "call", rep))
    hint = general.hint_get(dev, A, nc, kw["multi_label"], KW["conf_thres"])
    assert 0 < hint["cand"] <= 6144, (what, hint)            # the last two calls took the in-LDS regime


def test_tie_byte3(dev, oracle_lib):
    """Equal confidences whose tie words differ in byte 3 (A * nc >= 2^24): the row with the SMALLER word must come first, and it
    is the one with the larger low three bytes.  agnostic: one list per image, the key's low word is the tie word (the radix sort
    needs its fourth pass, csrc/nms_plan.h: radix_mask); nc = 40 without agnostic: the class-key mode."""
    A, nc = BC.TIE_SHAPE
    pred, pairs = BC.tie_case(A, nc, torch.float16, BC.TIE_SEED, device=dev)
    assert len(pairs) >= 8
    for mode in ("agnostic", "class_key"):
        ref = BC.tie_reference(mode)
        _three_calls(dev, pred, ref, (mode, "bs 2"), **BC.TIE_KW[mode])
        _three_calls(dev, pred[:1], ref[:1], (mode, "bs 1"), **BC.TIE_KW[mode])
    del pred
    torch.cuda.empty_cache()
