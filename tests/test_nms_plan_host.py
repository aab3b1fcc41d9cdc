"""CPU: which path a call of the NMS drivers takes (yolov5_obb_amd/csrc/nms_plan.h), compiled with g++ behind a serial driver
(tests/native/host_nms_plan.cpp).  The reference is a FROZEN restatement, in Python, of the decision code as it stood inline in
run_nms / mk_choose / mk_cross_in_lds / mk_steps (nms.hip) and run_nms_obb (nmsobb_impl.h) before the header existed: written from
that source, never from the header, compared exactly and field by field.  A change of policy edits the header AND this file."""
import ctypes as C
import os
import random
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- the constants as the decision code used them
CAP_FIRST, GRID_MIN_N, MK_MIN_N, MK_MIN_KEPT, MK_X_ROWS, MK_PEND1 = 2048, 8192, 16384, 256, 3072, 1 << 21
SMALL_MAX, SMALL_WORDS, SMALL_HELP_MAX, SORT_LDS_HINT, PS_MAX_N, DEC_THREADS = 384, 6, 256, 6144, 131072, 512
PS_SCRATCH = 256 * 16 * 8 + 256 * 256 * 4 + 256          # what the three-launch sort needs (psrs_sort.h)
ENV_DEFAULT = dict(mk=2, mk_xlds=-1, small_helpers=-1, self_sort=2, mk_steps=0, mk_pend=MK_PEND1, phase_prof=0, quad_skip=3)
ENV_ORDER = ["mk", "mk_xlds", "small_helpers", "self_sort", "mk_steps", "mk_pend", "phase_prof", "quad_skip"]
ENV_NAMES = ["OBB_NMS_MK", "OBB_NMS_MK_XLDS", "OBB_NMS_SMALL_HELPERS", "OBB_NMS_SELF_SORT", "OBB_NMS_MK_STEPS", "OBB_NMS_MK_PEND",
             "OBB_NMS_PHASE_PROF", "OBB_NMS_POLY_STRICT"]


def f32(x):
    return struct.unpack("f", struct.pack("f", x))[0]


def atoi(s):                                              # C's atoi on the strings of this file
    s = s.lstrip(" \t\n\v\f\r")
    sign, i = 1, 0
    if s[:1] in ("+", "-"):
        sign, i = (-1 if s[0] == "-" else 1), 1
    j = i
    while j < len(s) and s[j].isdigit():
        j += 1
    return sign * int(s[i:j]) if j > i else 0


# ---- the parsers, as the getenv lambdas stood
def ref_parse(which, e):
    if which == 0:
        return atoi(e) if e is not None else 2
    if which == 1:
        return int(e[0]) if e and e[0] in "01" else -1
    if which == 2:
        v = atoi(e) if e else -1
        return SMALL_HELP_MAX if v > SMALL_HELP_MAX else v
    if which == 3:
        return int(e[0]) if e and "0" <= e[0] <= "2" else 2
    if which == 4:
        return atoi(e) if e is not None else 0
    if which == 5:
        v = atoi(e) if e is not None else 0
        return v if 0 < v < MK_PEND1 else MK_PEND1
    if which == 6:
        return 1 if e is not None and atoi(e) else 0
    v = atoi(e) if e is not None else 0
    return 1 if v == 1 else (0 if v >= 2 else 3)


# ---- one list: run_nms with mk_feedback / mk_choose / mk_cross_in_lds / mk_steps
def ref_single(kind, n, thr, max_keep, has_grid, has_mk, words, calls, env):
    """-> (fields, whether the call counter advanced).  words: the eight pinned words, None: the thread has none."""
    thr = f32(thr)
    use_grid = kind == 0 and has_grid and thr >= 0.0 and n < (1 << 24)
    reach = use_grid and has_mk and n >= MK_MIN_N and max_keep <= 0
    fbk = words if reach else None                        # MkFeedback* fbk = (...) ? mk_feedback(n) : nullptr
    counted = False

    def mk_choose(f):
        nonlocal counted
        mode = env["mk"]
        if mode == 0:
            return False
        if mode == 1 or f is None:
            return mode == 1
        k = calls                                         # f->calls++
        counted = True
        kept, slab = f[1], f[2]
        if kept < 0 or (k & 63) == 0:
            return False
        if not (slab != 1 and kept >= MK_MIN_KEPT):
            return False
        t_persist, t_mk, k_persist, k_mk = f[4], f[5], f[6], f[7]

        def stale(kk):
            return kk < 0 or abs(kk - kept) > kept // 4 + 16
        if t_mk <= 0 or stale(k_mk):
            return True
        if t_persist <= 0 or stale(k_persist):
            return False
        if (k & 63) == 32:
            return t_mk >= t_persist
        return t_mk < t_persist

    use_mk = bool(reach and mk_choose(fbk))
    use_slabs = bool(use_grid and not use_mk and max_keep <= 0)
    kept_prev = fbk[1] if fbk is not None else -1
    cap_first = slab_cap = xlds = steps = pend = 0
    if use_mk:
        cap_first = 4096 if (kept_prev >= 0 and kept_prev * 8 > n) else 2048
        pend = env["mk_pend"]
        steps = 4                                         # mk_steps
        if fbk is not None:
            h = fbk[0]
            if h >= 0:
                steps = h
            elif h == -2:
                last = fbk[3]
                steps = 2 * last if last > 0 else 8
        if env["mk_steps"] > 0:
            steps = env["mk_steps"]
        steps = max(1, min(32, steps))
        if env["mk_xlds"] in (0, 1):                      # mk_cross_in_lds
            xlds = env["mk_xlds"]
        else:
            xlds = int(0 <= kept_prev <= 2 * MK_X_ROWS)
    if use_slabs:
        slab_cap = 2048 if (kept_prev >= 0 and kept_prev * 8 > n) else 1024
    return [int(use_grid), int(use_mk), int(use_slabs), cap_first, slab_cap, xlds, steps, pend], counted


# ---- the fused driver: run_nms_obb
def ref_cap_max(nseg):
    return 8192 if nseg == 1 else (2048 if nseg <= 64 else 1024)


def ref_nms_grid(nseg, n_slots, cap_first, cus):
    nb = (n_slots + 511) // 512
    per_seg = (n_slots + nseg - 1) // nseg
    c = min(per_seg, cap_first)
    tiles = ((c + 63) // 64) * ((c + 63) // 64 + 1) // 2 * nseg
    nb = max(nb, (tiles + 7) // 8)
    if n_slots >= 8192:
        nb = cus
    nb = max(nb, nseg)
    nb = min(nb, cus)
    return max(nb, 1)


def ref_nms_window(max_keep):
    if max_keep <= 0:
        return 0
    w = min(max(4 * max_keep, 8192), 1 << 30)
    return (w + 63) // 64 * 64


def blk(nbytes):                                          # a take of the workspace cursor: 256-byte blocks, an empty one is one block
    return max(256, -(-nbytes // 256) * 256)


def ref_help_bytes(helpers, nseg, n_pos):
    return blk(helpers * 4) + 2 * blk(nseg * 4) + blk(n_pos * SMALL_WORDS * 8) + blk(helpers * SMALL_MAX * SMALL_WORDS * 8)


OBB_IN = ["bs", "A", "nc", "agnostic", "multi_label", "n_extra", "cap_img", "max_nms", "max_det", "expected_cand", "out_packed", "hw_cus",
          "cus", "ecap", "sort_tmp_bytes", "ps_scratch_bytes"]
OBB_OUT = ["ncs", "class_ok", "multi_label", "expected_cand", "seg_hint", "small_hint", "lds_sort", "small_nms", "self_sort", "helpers",
           "fused_out", "rows_per_thread", "parts", "plan_nb", "plan_chunk", "max_seg", "radix_mask", "psrs", "gparts", "window"]


def ref_obb(i, env):
    iou, max_wh = f32(i["iou_thres"]), f32(i["max_wh"])
    bs, A, nc, cap_img = i["bs"], i["A"], i["nc"], i["cap_img"]
    word = i["expected_cand"]
    seg_hint = (word >> 32) & 0x1fffffff
    small_hint = (word >> 62) & 1
    expected = word & 0xffffffff
    ncs = 1 if i["agnostic"] else nc
    class_ok = int(not i["agnostic"] and nc > 1 and A + i["n_extra"] < (1 << 24) and iou >= 0.0 and max_wh > 0.0)
    lds_sort = 0 < expected <= SORT_LDS_HINT
    rows = 4 if bs * A >= 4 * DEC_THREADS * 480 else (2 if bs * A >= 2 * DEC_THREADS * 480 else 1)
    max_seg = i["max_nms"] if 0 < i["max_nms"] < cap_img else cap_img
    plan_chunk = min(CAP_FIRST, ref_cap_max(bs * ncs))
    small_nms = bool(lds_sort and class_ok and 0 < seg_hint <= SMALL_MAX and iou >= 0.0 and bs * ncs <= 65535)
    plan_nb = ref_nms_grid(bs * ncs, bs * max_seg, CAP_FIRST, i["cus"]) if (bs * ncs > 1 and not small_nms) else 0
    helpers_env, self_env = env["small_helpers"], env["self_sort"]
    self_possible = small_nms and not i["out_packed"] and ncs * SMALL_MAX <= cap_img and self_env != 0
    helpers = 0
    if small_nms and not (self_possible and self_env == 2 and helpers_env < 0):
        free_cus = i["hw_cus"] - bs * ncs
        helpers = helpers_env if helpers_env >= 0 else (0 if free_cus < 0 else min(free_cus, SMALL_HELP_MAX))
    if helpers > 0:
        have = min(bs * ncs, i["cus"]) * i["ecap"] * 4
        if ref_help_bytes(helpers, bs * ncs, bs * cap_img) > have:
            helpers = 0
    self_sort = bool(self_possible and helpers == 0)
    parts = mask = psrs = 0
    if self_sort:
        pass
    elif lds_sort:
        parts = 4 if (class_ok and ncs >= 8) else 1
    else:
        tb = 0
        while (1 << tb) < A * nc + i["n_extra"] + 1:
            tb += 1
        mask = 0xF0
        for d in range(4):
            if tb > d * 8:
                mask |= 1 << d
        if class_ok:
            mask = 0xFF
        psrs = int(bs == 1 and cap_img <= PS_MAX_N and i["sort_tmp_bytes"] >= i["ps_scratch_bytes"])
    fused_out = bool(small_nms and not i["out_packed"])
    gparts = 0
    if not fused_out:
        gparts = 1 if expected <= 2048 else min((expected + 1023) // 1024, 16)
    out = dict(ncs=ncs, class_ok=class_ok, multi_label=int(bool(i["multi_label"]) and nc > 1), expected_cand=expected, seg_hint=seg_hint,
               small_hint=small_hint, lds_sort=int(lds_sort), small_nms=int(small_nms), self_sort=int(self_sort), helpers=helpers,
               fused_out=int(fused_out), rows_per_thread=rows, parts=parts, plan_nb=plan_nb, plan_chunk=plan_chunk, max_seg=max_seg,
               radix_mask=mask, psrs=psrs, gparts=gparts, window=ref_nms_window(i["max_det"]))
    return [out[k] for k in OBB_OUT]


# ---- the library side
@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = tmp_path_factory.mktemp("np") / "libhostnmsplan.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", f"-I{ROOT}/yolov5_obb_amd/csrc", f"-I{ROOT}/include",
                    f"{ROOT}/tests/native/host_nms_plan.cpp", "-o", str(out)], check=True)
    L = C.CDLL(str(out))
    L.np_env_parse.argtypes, L.np_env_parse.restype = [C.c_int, C.c_char_p], C.c_int
    L.np_env_read.argtypes, L.np_env_read.restype = [C.POINTER(C.c_int)], None
    L.np_single.argtypes = [C.c_int, C.c_int64, C.c_float, C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_uint, C.POINTER(C.c_int),
                            C.POINTER(C.c_int)]
    L.np_single.restype = C.c_int
    L.np_obb.argtypes, L.np_obb.restype = [C.POINTER(C.c_int64), C.c_float, C.c_float, C.POINTER(C.c_int), C.POINTER(C.c_int64)], None
    L.np_help_bytes.argtypes, L.np_help_bytes.restype = [C.c_int, C.c_int64, C.c_int64], C.c_uint64
    L.np_help_place.argtypes, L.np_help_place.restype = [C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.POINTER(C.c_uint64)], None
    L.np_nms_grid.argtypes, L.np_nms_grid.restype = [C.c_int64, C.c_int64, C.c_int, C.c_int], C.c_int
    L.np_nms_window.argtypes, L.np_nms_window.restype = [C.c_int64], C.c_int
    L.np_class_mask.argtypes, L.np_class_mask.restype = [C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_uint64)], None
    return L


def env8(env):
    return (C.c_int * 8)(*[env[k] for k in ENV_ORDER])


def lib_single(L, kind, n, thr, max_keep, has_grid, has_mk, words, calls, env):
    out = (C.c_int * 8)()
    w = (C.c_int * 8)(*words) if words is not None else None
    counted = L.np_single(kind, n, thr, max_keep, int(has_grid), int(has_mk), w, calls, env8(env), out)
    return list(out), bool(counted)


def lib_obb(L, i, env):
    out = (C.c_int64 * 20)()
    L.np_obb((C.c_int64 * 16)(*[i[k] for k in OBB_IN]), i["iou_thres"], i["max_wh"], env8(env), out)
    return list(out)


# ---- one list: one case per branch.  words: steps, kept, slabs, enqueued, t_persist, t_mk, k_persist, k_mk
NEVER = [-1] * 8
BOTH = [3, 4000, 0, 3, 500, 400, 4000, 4000]                      # both paths have reported on such data: the phase kernels are faster


def S(**kw):
    d = dict(kind=0, n=100000, thr=0.4, max_keep=0, has_grid=True, has_mk=True, words=BOTH, calls=5, env={})
    d.update(kw)
    d["env"] = dict(ENV_DEFAULT, **d["env"])
    return d


def W(**kw):                                                       # BOTH with some words replaced
    w = list(BOTH)
    for k, v in kw.items():
        w[int(k[1:])] = v
    return w


SINGLE = {
    "mode 0": S(env=dict(mk=0)),
    "mode 1": S(env=dict(mk=1), words=NEVER),
    "mode 1, the thread has no words": S(env=dict(mk=1), words=None),
    "mode 2, no feedback": S(words=None),
    "first call (kept < 0)": S(words=NEVER),
    "every 64th call": S(calls=128),
    "slab found": S(words=W(w2=1)),
    "kept below kMkMinKept": S(words=W(w1=MK_MIN_KEPT - 1, w6=MK_MIN_KEPT - 1, w7=MK_MIN_KEPT - 1)),
    "kept at kMkMinKept": S(words=W(w1=MK_MIN_KEPT, w6=MK_MIN_KEPT, w7=MK_MIN_KEPT)),
    "t_mk unknown": S(words=W(w5=-1, w4=100)),
    "t_mk zero": S(words=W(w5=0, w4=100)),
    "k_mk stale": S(words=W(w7=4000 + 1000 + 17, w5=900)),
    "k_mk at the edge of stale": S(words=W(w7=4000 + 1000 + 16, w5=900)),
    "k_mk never written": S(words=W(w7=-1, w5=900)),
    "t_persist unknown": S(words=W(w4=-1)),
    "k_persist stale": S(words=W(w6=4000 - 1000 - 17)),
    "the slower one's turn, phase kernels faster": S(calls=32),
    "the slower one's turn, phase kernels slower": S(calls=96, words=W(w5=600)),
    "the slower one's turn, equal times": S(calls=32, words=W(w5=500)),
    "faster wins: the phase kernels": S(),
    "faster wins: the persistent kernel": S(words=W(w5=600)),
    "equal times": S(words=W(w5=500)),
    "step hint 0": S(words=W(w0=0)),
    "step hint 7": S(words=W(w0=7)),
    "hint -2 with a previous enqueued count": S(words=W(w0=-2, w3=5)),
    "hint -2 without one": S(words=W(w0=-2, w3=-1)),
    "hint -1": S(words=W(w0=-1)),
    "the 32 cap by hint": S(words=W(w0=33)),
    "the 32 cap by doubling": S(words=W(w0=-2, w3=17)),
    "fixed_steps": S(env=dict(mk_steps=2)),
    "fixed_steps above the cap": S(env=dict(mk_steps=40)),
    "xlds pinned to 0": S(env=dict(mk_xlds=0)),
    "xlds pinned to 1": S(env=dict(mk_xlds=1), words=W(w1=30000, w6=30000, w7=30000)),
    "xlds: kept at 2 * kMkXRows": S(words=W(w1=2 * MK_X_ROWS, w6=2 * MK_X_ROWS, w7=2 * MK_X_ROWS)),
    "xlds: one above": S(words=W(w1=2 * MK_X_ROWS + 1, w6=2 * MK_X_ROWS + 1, w7=2 * MK_X_ROWS + 1)),
    "cap_first: kept * 8 == n": S(words=W(w1=12500, w6=12500, w7=12500)),
    "cap_first: one above": S(words=W(w1=12501, w6=12501, w7=12501)),
    "slab_cap: kept * 8 == n": S(env=dict(mk=0), words=W(w1=12500)),
    "slab_cap: one above": S(env=dict(mk=0), words=W(w1=12501)),
    "n = kMkMinN - 1": S(n=MK_MIN_N - 1, words=W(w1=3000)),
    "n = kMkMinN": S(n=MK_MIN_N, words=W(w1=3000, w6=3000, w7=3000)),
    "n = kGridMinN - 1 (no index carved)": S(n=GRID_MIN_N - 1, has_grid=False, has_mk=False),
    "n = kGridMinN": S(n=GRID_MIN_N),
    "n = 2^24 - 1": S(n=(1 << 24) - 1),
    "n = 2^24": S(n=1 << 24),
    "max_keep > 0": S(max_keep=300),
    "thr < 0": S(thr=-0.5),
    "kind 1": S(kind=1, has_grid=False, has_mk=False),
    "kind 1 on a carve with the index": S(kind=1),
    "pend_cap from the environment": S(env=dict(mk_pend=300)),
}
# what the hand-written cases are there for (use_mk), beside the field-by-field compare
SINGLE_USE_MK = {"mode 0": 0, "mode 1": 1, "mode 1, the thread has no words": 1, "mode 2, no feedback": 0, "first call (kept < 0)": 0,
                 "every 64th call": 0, "slab found": 0, "kept below kMkMinKept": 0, "kept at kMkMinKept": 1, "t_mk unknown": 1,
                 "k_mk stale": 1, "k_mk at the edge of stale": 0, "t_persist unknown": 0, "k_persist stale": 0,
                 "the slower one's turn, phase kernels faster": 0, "the slower one's turn, phase kernels slower": 1,
                 "the slower one's turn, equal times": 1, "faster wins: the phase kernels": 1, "faster wins: the persistent kernel": 0,
                 "equal times": 0, "n = kMkMinN - 1": 0, "n = kMkMinN": 1, "max_keep > 0": 0, "thr < 0": 0, "kind 1": 0, "n = 2^24": 0}


@pytest.mark.parametrize("name", list(SINGLE))
def test_single_list_branch(lib, name):
    c = SINGLE[name]
    want, want_counted = ref_single(**c)
    got, counted = lib_single(lib, **c)
    assert dict(zip("use_grid use_mk use_slabs cap_first slab_cap xlds steps pend_cap".split(), got)) == \
        dict(zip("use_grid use_mk use_slabs cap_first slab_cap xlds steps pend_cap".split(), want))
    assert counted == want_counted, "the call counter advances in mode 2 with feedback words, and only then"
    if name in SINGLE_USE_MK:
        assert got[1] == SINGLE_USE_MK[name]


def test_single_list_expected_values(lib):
    """A few plans spelt out, so that the restatement itself is pinned to the numbers the comments of the policy give."""
    assert lib_single(lib, **SINGLE["faster wins: the phase kernels"])[0] == [1, 1, 0, 2048, 0, 1, 3, MK_PEND1]
    assert lib_single(lib, **SINGLE["cap_first: one above"])[0] == [1, 1, 0, 4096, 0, 0, 3, MK_PEND1]
    assert lib_single(lib, **SINGLE["slab_cap: one above"])[0] == [1, 0, 1, 0, 2048, 0, 0, 0]
    assert lib_single(lib, **SINGLE["hint -2 with a previous enqueued count"])[0][6] == 10
    assert lib_single(lib, **SINGLE["hint -2 without one"])[0][6] == 8
    assert lib_single(lib, **SINGLE["the 32 cap by doubling"])[0][6] == 32
    assert lib_single(lib, **SINGLE["step hint 0"])[0][6] == 1
    assert lib_single(lib, **SINGLE["mode 2, no feedback"])[0] == [1, 0, 1, 0, 1024, 0, 0, 0]
    assert lib_single(lib, **SINGLE["max_keep > 0"])[0] == [1, 0, 0, 0, 0, 0, 0, 0]
    assert lib_single(lib, **SINGLE["kind 1 on a carve with the index"])[0] == [0] * 8


WORD_VALUES = [-2, -1, 0, 1, 2, 4, 16, 17, 31, 32, 33, 255, 256, 257, 300, 1000, 2047, 2048, 2049, 3000, 3734, 3735, 3766, 3767, 4000, 4984, 4985,
               5016, 5017, 6143, 6144, 6145, 12499, 12500, 12501, 36030, 40024, 100000, 0x3fffffff]


def test_single_list_random(lib):
    rng = random.Random(20260119)
    ns = [0, 1, GRID_MIN_N - 1, GRID_MIN_N, MK_MIN_N - 1, MK_MIN_N, 32000, 49152, 100000, 8 * 6144, 8 * 6144 + 1, (1 << 24) - 1, 1 << 24, 1 << 26]
    mk_used = 0
    for _ in range(24000):
        c = dict(kind=rng.choice([0, 0, 0, 1]), n=rng.choice(ns), thr=rng.choice([0.4, 0.4, 0.0, -0.1]), max_keep=rng.choice([0, 0, 0, -1, 300]),
                 has_grid=rng.random() < 0.9, has_mk=rng.random() < 0.9,
                 words=None if rng.random() < 0.1 else [rng.choice(WORD_VALUES) for _ in range(8)],
                 calls=rng.choice([0, 1, 31, 32, 33, 63, 64, 65, 96, 128, 0xffffffe0, 0xffffffff, rng.randrange(1 << 32)]),
                 env=dict(ENV_DEFAULT, mk=rng.choice([2, 2, 2, 0, 1, 3, -1]), mk_xlds=rng.choice([-1, -1, 0, 1]),
                          mk_steps=rng.choice([0, 0, 0, 1, 3, 40, -1]), mk_pend=rng.choice([MK_PEND1, 300, 70000])))
        if c["words"] is not None and rng.random() < 0.5:            # the comparable regime: times for kept counts near the last one
            kept = rng.choice([300, 4000, 12501, 40024])
            c["words"][1], c["words"][2] = kept, rng.choice([0, 0, -1, 1])
            c["words"][6], c["words"][7] = kept + rng.choice([0, 16, kept // 4 + 16, kept // 4 + 17, -17]), kept - rng.choice([0, kept // 4 + 16, kept // 4 + 17])
        want = ref_single(**c)
        assert lib_single(lib, **c) == want, c
        mk_used += want[0][1]
    assert 1000 < mk_used < 23000, "the generator reaches both outcomes a thousand times at least"


# ---- the fused driver
def ecap_of(nseg):
    c = ref_cap_max(nseg)
    return c * (c - 1) // 2


def O(env=None, **kw):
    d = dict(bs=16, A=64512, nc=16, agnostic=0, multi_label=1, iou_thres=0.45, max_wh=4096.0, n_extra=0, cap_img=65536, max_nms=30000,
             max_det=300, expected_cand=1700 | (230 << 32), out_packed=0, hw_cus=256, cus=256, ecap=None, sort_tmp_bytes=PS_SCRATCH,
             ps_scratch_bytes=PS_SCRATCH)
    d.update(kw)
    if d["ecap"] is None:
        d["ecap"] = ecap_of(d["bs"] * (1 if d["agnostic"] else d["nc"]))
    return d, dict(ENV_DEFAULT, **(env or {}))


def word(cand, seg=0, small=0):
    return cand | (seg << 32) | (small << 62)


OBB = {
    "the bench shape": O(),
    "bs 1, SELF_SORT=1": O(dict(self_sort=1), bs=1),
    "bs 4, SELF_SORT=1": O(dict(self_sort=1), bs=4),
    "bs 8, SELF_SORT=1": O(dict(self_sort=1), bs=8),
    "bs 16, SELF_SORT=1: no CU is free": O(dict(self_sort=1)),
    "bs 8, SELF_SORT=1, the layout does not fit ecap": O(dict(self_sort=1), bs=8, ecap=10000),     # 128 teams x 40 KB against 25 MB of bit matrices
    "bs 8, SELF_SORT=1, the layout fits exactly": O(dict(self_sort=1), bs=8, ecap=-(-ref_help_bytes(128, 128, 8 * 65536) // (128 * 4))),
    "bs 8, SELF_SORT=1, one word short": O(dict(self_sort=1), bs=8, ecap=-(-ref_help_bytes(128, 128, 8 * 65536) // (128 * 4)) - 1),
    "SELF_SORT=0": O(dict(self_sort=0)),
    "SELF_SORT=0, bs 4": O(dict(self_sort=0), bs=4),
    "SMALL_HELPERS=0": O(dict(small_helpers=0), bs=4),
    "SMALL_HELPERS=7": O(dict(small_helpers=7), bs=4),
    "SMALL_HELPERS=256, a capped grid": O(dict(small_helpers=256), bs=4, cus=8),
    "un-hinted first call: radix": O(expected_cand=0),
    "un-hinted first call, bs 1: PSRS": O(bs=1, expected_cand=0),
    "bs 1, cap_img = kPsMaxN": O(bs=1, expected_cand=0, cap_img=PS_MAX_N),
    "bs 1, cap_img above kPsMaxN": O(bs=1, expected_cand=0, cap_img=PS_MAX_N + 64),
    "bs 1, scratch too small for PSRS": O(bs=1, expected_cand=0, sort_tmp_bytes=PS_SCRATCH - 1),
    "agnostic": O(agnostic=1),
    "agnostic, un-hinted": O(agnostic=1, expected_cand=0),
    "nc == 1": O(nc=1),
    "nc == 1, bs 1": O(nc=1, bs=1),
    "iou_thres < 0": O(iou_thres=-0.5),
    "iou_thres == 0": O(iou_thres=0.0),
    "max_wh <= 0": O(max_wh=0.0),
    "A + n_extra = 2^24 - 1": O(A=(1 << 24) - 4, n_extra=3, bs=1),
    "A + n_extra = 2^24": O(A=(1 << 24) - 4, n_extra=4, bs=1),
    "A + n_extra = 2^24, un-hinted": O(A=(1 << 24) - 4, n_extra=4, bs=1, expected_cand=0),
    "out_packed": O(out_packed=1),
    "out_packed, bs 4": O(out_packed=1, bs=4),
    "seg_hint = kSmallMax": O(expected_cand=word(1700, SMALL_MAX)),
    "seg_hint one above": O(expected_cand=word(1700, SMALL_MAX + 1)),
    "seg_hint unknown": O(expected_cand=word(1700, 0)),
    "expected_cand = kSortLdsHint": O(expected_cand=word(SORT_LDS_HINT, 230)),
    "expected_cand one above": O(expected_cand=word(SORT_LDS_HINT + 1, 230)),
    "short-sided boxes seen": O(expected_cand=word(1700, 230, 1)),
    "short-sided boxes seen, agnostic": O(expected_cand=word(1700, 230, 1), agnostic=1),
    "bs * ncs = 65535": O(bs=257, nc=255, A=1000, cap_img=98304 // 12),
    "bs * ncs = 65536": O(bs=256, nc=256, A=1000, cap_img=98304 // 12),
    "ncs * kSmallMax = cap_img": O(cap_img=16 * SMALL_MAX),
    "ncs * kSmallMax one block above cap_img": O(cap_img=16 * SMALL_MAX - 64),
    "rows_per_thread 1": O(bs=1, A=2 * DEC_THREADS * 480 - 1),
    "rows_per_thread 2": O(bs=1, A=2 * DEC_THREADS * 480),
    "rows_per_thread 2, top": O(bs=1, A=4 * DEC_THREADS * 480 - 1),
    "rows_per_thread 4": O(bs=1, A=4 * DEC_THREADS * 480),
    "gparts at 2048": O(expected_cand=word(2048, 500)),
    "gparts at 2049": O(expected_cand=word(2049, 500)),
    "gparts 16": O(expected_cand=word(16 * 1024, 500)),
    "gparts capped at 16": O(expected_cand=word(16 * 1024 + 1, 500)),
    "radix mask, tie word of 8 bits": O(agnostic=1, expected_cand=0, A=255, nc=1, bs=2),
    "radix mask, tie word of 9 bits": O(agnostic=1, expected_cand=0, A=256, nc=1, bs=2),
    "radix mask, tie word of 24 bits": O(agnostic=1, expected_cand=0, A=(1 << 24) - 1, nc=1, bs=2, cap_img=4096),
    "radix mask, tie word of 25 bits": O(agnostic=1, expected_cand=0, A=1 << 24, nc=1, bs=2, cap_img=4096),
    "radix mask, class keys": O(expected_cand=0, A=255, nc=2, bs=2),
    "sort parts: seven classes": O(nc=7, expected_cand=word(1700, 500)),
    "sort parts: eight classes": O(nc=8, expected_cand=word(1700, 500)),
    "planner grid: a capped grid": O(expected_cand=word(1700, 500), cus=8),
    "max_nms below cap_img": O(max_nms=1000, expected_cand=word(1700, 500)),
    "max_nms = 0": O(max_nms=0, expected_cand=word(1700, 500)),
    "multi_label with one class": O(nc=1, multi_label=1),
    "max_det large": O(max_det=1 << 29),
}


@pytest.mark.parametrize("name", list(OBB))
def test_fused_driver_branch(lib, name):
    i, env = OBB[name]
    assert dict(zip(OBB_OUT, lib_obb(lib, i, env))) == dict(zip(OBB_OUT, ref_obb(i, env)))


def test_fused_driver_expected_values(lib):
    def plan(name):
        return dict(zip(OBB_OUT, lib_obb(lib, *OBB[name])))
    p = plan("the bench shape")                 # three launches: the filter, k_nms_small with its own ordering and output stage
    assert (p["small_nms"], p["self_sort"], p["helpers"], p["fused_out"], p["parts"], p["radix_mask"], p["psrs"], p["gparts"]) == (1, 1, 0, 1, 0, 0, 0, 0)
    assert (p["ncs"], p["class_ok"], p["lds_sort"], p["rows_per_thread"], p["plan_nb"]) == (16, 1, 1, 4, 0)
    for bs in (1, 4, 8):                        # helpers: the CUs the segments leave free
        p = plan(f"bs {bs}, SELF_SORT=1")
        assert (p["helpers"], p["self_sort"], p["parts"]) == (256 - 16 * bs, 0, 4)
    assert plan("bs 16, SELF_SORT=1: no CU is free")["helpers"] == 0 and plan("bs 16, SELF_SORT=1: no CU is free")["self_sort"] == 1
    p = plan("bs 8, SELF_SORT=1, the layout does not fit ecap")
    assert (p["helpers"], p["self_sort"]) == (0, 1)
    assert plan("bs 8, SELF_SORT=1, the layout fits exactly")["helpers"] == 128
    assert plan("bs 8, SELF_SORT=1, one word short")["helpers"] == 0
    assert plan("un-hinted first call: radix")["radix_mask"] == 0xFF and plan("un-hinted first call: radix")["psrs"] == 0
    assert plan("un-hinted first call, bs 1: PSRS")["psrs"] == 1 and plan("bs 1, cap_img = kPsMaxN")["psrs"] == 1
    assert plan("bs 1, cap_img above kPsMaxN")["psrs"] == 0
    assert [plan(f"radix mask, tie word of {b} bits")["radix_mask"] for b in (8, 9, 24, 25)] == [0xF1, 0xF3, 0xF7, 0xFF]
    assert [plan(n)["gparts"] for n in ("gparts at 2048", "gparts at 2049", "gparts 16", "gparts capped at 16")] == [1, 3, 16, 16]
    assert [plan(n)["small_nms"] for n in ("bs * ncs = 65535", "bs * ncs = 65536")] == [1, 0]
    assert [plan(n)["class_ok"] for n in ("A + n_extra = 2^24 - 1", "A + n_extra = 2^24")] == [1, 0]
    assert [plan(n)["self_sort"] for n in ("ncs * kSmallMax = cap_img", "ncs * kSmallMax one block above cap_img")] == [1, 0]
    assert [plan(n)["small_nms"] for n in ("seg_hint = kSmallMax", "seg_hint one above")] == [1, 0]
    assert [plan(n)["lds_sort"] for n in ("expected_cand = kSortLdsHint", "expected_cand one above")] == [1, 0]


def test_fused_driver_random(lib):
    rng = random.Random(20260120)
    seen = {k: set() for k in ("small_nms", "self_sort", "psrs", "fused_out", "lds_sort", "class_ok")}
    helpers_cut = 0
    for _ in range(24000):
        bs = rng.choice([1, 1, 2, 4, 8, 16, 16, 17, 64, 65, 256, 257])
        nc = rng.choice([1, 2, 7, 8, 15, 16, 16, 18, 80, 255, 256])
        agnostic = int(rng.random() < 0.15)
        ncs = 1 if agnostic else nc
        A = rng.choice([255, 256, 1000, 3000, 64512, 2 * 512 * 480 - 1, 2 * 512 * 480, 4 * 512 * 480, (1 << 24) - 2, 1 << 24])
        while A * nc > 0xffffff00:
            A //= 2
        cap_img = rng.choice([64, 1024, ncs * SMALL_MAX - 64, ncs * SMALL_MAX, 8192, 65536, PS_MAX_N, PS_MAX_N + 64])
        cap_img = max(64, (cap_img + 63) // 64 * 64)
        while bs * cap_img > 0x7fffffff:
            cap_img //= 2
        cand = rng.choice([0, 1, 300, 1700, 2048, 2049, 5000, SORT_LDS_HINT, SORT_LDS_HINT + 1, 16384, 16385, 100000])
        seg = rng.choice([0, 1, 128, 230, SMALL_MAX, SMALL_MAX + 1, 5000])
        i = dict(bs=bs, A=A, nc=nc, agnostic=agnostic, multi_label=rng.randrange(2), iou_thres=rng.choice([0.45, 0.45, 0.45, 0.0, -0.5]),
                 max_wh=rng.choice([4096.0, 4096.0, 4096.0, 0.0, -1.0]), n_extra=rng.choice([0, 0, 1, 2, 100]), cap_img=cap_img,
                 max_nms=rng.choice([30000, 30000, 0, 1000, cap_img]), max_det=rng.choice([300, 1, 2048, 2049, 1000, 1 << 29]),
                 expected_cand=word(cand, seg, rng.randrange(2)), out_packed=int(rng.random() < 0.2),
                 hw_cus=rng.choice([256, 256, 304, 64]), cus=rng.choice([256, 256, 8, 64]),
                 ecap=rng.choice([ecap_of(bs * ncs), ecap_of(bs * ncs), 1, 100000]),
                 sort_tmp_bytes=rng.choice([PS_SCRATCH, PS_SCRATCH, PS_SCRATCH - 1]), ps_scratch_bytes=PS_SCRATCH)
        env = dict(ENV_DEFAULT, small_helpers=rng.choice([-1, -1, -1, 0, 7, 256]), self_sort=rng.choice([2, 2, 1, 1, 0]))
        want = ref_obb(i, env)
        assert lib_obb(lib, i, env) == want, (i, env)
        p = dict(zip(OBB_OUT, want))
        for k in seen:
            seen[k].add(p[k])
        helpers_cut += int(p["small_nms"] and env["self_sort"] == 1 and not i["out_packed"] and p["helpers"] == 0 and i["ecap"] <= 100000)
    assert all(v == {0, 1} for v in seen.values()), seen
    assert helpers_cut > 50


# ---- the helpers' blocks, the launch geometry, the parsers
@pytest.mark.parametrize("helpers,nseg,n_pos", [(1, 1, 64), (5, 33, 1000), (64, 64, 4096), (128, 128, 8 * 65536), (256, 16, 65536), (7, 65535, 64)])
def test_helper_blocks(lib, helpers, nseg, n_pos):
    need = lib.np_help_bytes(helpers, nseg, n_pos)
    assert need == ref_help_bytes(helpers, nseg, n_pos)
    off = (C.c_uint64 * 5)()
    lib.np_help_place(256 * 1000, helpers, nseg, n_pos, off)        # (an address that is never touched: the layout only adds to it)
    sizes = [helpers * 4, nseg * 4, nseg * 4, n_pos * SMALL_WORDS * 8, helpers * SMALL_MAX * SMALL_WORDS * 8]
    at = 0
    for o, sz in zip(off, sizes):                                   # work, seg_np, seg_ticket, part_main, part_help: in this order, back to back
        assert o == at
        at += blk(sz)
    assert at == need


def test_launch_geometry(lib):
    rng = random.Random(7)
    for nseg, n_slots, cus in [(1, 100, 256), (1, 8191, 256), (1, 8192, 256), (256, 256 * 30000, 256), (300, 1000, 256), (16, 16 * 1700, 8), (2, 0, 256)]:
        assert lib.np_nms_grid(nseg, n_slots, CAP_FIRST, cus) == ref_nms_grid(nseg, n_slots, CAP_FIRST, cus)
    for _ in range(2000):
        nseg, cus = rng.choice([1, 2, 16, 64, 65, 256, 4096]), rng.choice([1, 8, 64, 256, 304])
        n_slots = rng.choice([0, 1, 511, 512, 513, 4096, 8191, 8192, 100000, 1 << 30])
        cf = rng.choice([1024, 2048])
        assert lib.np_nms_grid(nseg, n_slots, cf, cus) == ref_nms_grid(nseg, n_slots, cf, cus)
    for mk in (-1, 0, 1, 300, 2047, 2048, 2049, 100000, 1 << 28, (1 << 28) + 1, 1 << 40):
        assert lib.np_nms_window(mk) == ref_nms_window(mk)
    assert lib.np_nms_window(300) == 8192 and lib.np_nms_window(1 << 40) == 1 << 30


# ---- the class filter's bits (class_mask_fill): the fill as it stood inline in run_nms_obb
def ref_class_mask(classes, n):
    """-> (w[0..3], all).  classes None: a NULL pointer; n: the count the caller states."""
    w = [0, 0, 0, 0]
    for c in (classes or [])[:max(n, 0)]:
        if 0 <= c < 256:
            w[c >> 6] |= 1 << (c & 63)
    return w, int(classes is None or n <= 0)


def lib_class_mask(L, classes, n):
    out = (C.c_uint64 * 5)(*([0xdeadbeefdeadbeef] * 5))               # (every word is written)
    arr = (C.c_int32 * max(len(classes), 1))(*classes) if classes is not None else None
    L.np_class_mask(arr, n, out)
    return list(out[:4]), int(C.c_int64(out[4]).value)


CLASS_MASKS = {
    "NULL": (None, 3),
    "NULL, n = 0": (None, 0),
    "n = 0": ([5, 6], 0),
    "n < 0": ([5, 6], -1),
    "ids outside 0..255 are ignored": ([-1, 256, 1000], 3),
    "the edges of every word": ([0, 63, 64, 127, 128, 255], 6),
    "a repeated id": ([17, 17, 200, 17], 4),
    "only the first n ids": ([1, 2, 3, 4], 2),
    "ignored ids among valid ones": ([-1, 0, 256, 255, 1000, 64], 6),
}


@pytest.mark.parametrize("name", list(CLASS_MASKS))
def test_class_mask(lib, name):
    classes, n = CLASS_MASKS[name]
    assert lib_class_mask(lib, classes, n) == ref_class_mask(classes, n)


def test_class_mask_expected_values(lib):
    assert lib_class_mask(lib, *CLASS_MASKS["NULL"]) == ([0, 0, 0, 0], 1)
    assert lib_class_mask(lib, *CLASS_MASKS["n = 0"]) == ([0, 0, 0, 0], 1)
    assert lib_class_mask(lib, *CLASS_MASKS["ids outside 0..255 are ignored"]) == ([0, 0, 0, 0], 0), "a filter that allows nothing"
    assert lib_class_mask(lib, *CLASS_MASKS["the edges of every word"]) == ([1 | 1 << 63, 1 | 1 << 63, 1, 1 << 63], 0), "exactly their bits"
    assert lib_class_mask(lib, *CLASS_MASKS["a repeated id"]) == ([1 << 17, 0, 0, 1 << (200 - 192)], 0)
    for c in range(256):                                                # one id, one bit
        w, all_ = lib_class_mask(lib, [c], 1)
        assert all_ == 0 and sum(bin(x).count("1") for x in w) == 1 and (w[c >> 6] >> (c & 63)) & 1


STRINGS = [None, "", "0", "1", "2", "3", "-1", "999", "x", "1x", " 2", "01", "10", "300", str(MK_PEND1), str(MK_PEND1 - 1)]


@pytest.mark.parametrize("which", range(8))
def test_env_parsers(lib, which):
    for s in STRINGS:
        got = lib.np_env_parse(which, None if s is None else s.encode())
        assert got == ref_parse(which, s), (ENV_NAMES[which], s)


def test_env_parsers_expected_values(lib):
    def p(which, s):
        return lib.np_env_parse(which, None if s is None else s.encode())
    assert [p(0, s) for s in (None, "", "0", "1", "2", "x")] == [2, 0, 0, 1, 2, 0]
    assert [p(1, s) for s in (None, "", "0", "1", "2", "10", "x")] == [-1, -1, 0, 1, -1, 1, -1]
    assert [p(2, s) for s in (None, "", "0", "3", "-1", "999", "x")] == [-1, -1, 0, 3, -1, SMALL_HELP_MAX, 0]
    assert [p(3, s) for s in (None, "", "0", "1", "2", "3", "-1", "x")] == [2, 2, 0, 1, 2, 2, 2, 2]
    assert [p(5, s) for s in (None, "0", "-1", "300", str(MK_PEND1), "x")] == [MK_PEND1, MK_PEND1, MK_PEND1, 300, MK_PEND1, MK_PEND1]
    assert [p(7, s) for s in (None, "0", "1", "2", "3", "-1", "x")] == [3, 3, 1, 0, 0, 3, 3]


def test_the_reader_reads_the_per_call_switches_on_every_call(lib, monkeypatch):
    for name in ENV_NAMES:
        monkeypatch.delenv(name, raising=False)
    out = (C.c_int * 8)()
    lib.np_env_read(out)
    assert list(out) == [ENV_DEFAULT[k] for k in ENV_ORDER]
    for name, v in zip(ENV_NAMES, ["1", "0", "999", "1", "3", "300", "1", "1"]):
        monkeypatch.setenv(name, v)                                  # (through os.environ, which calls putenv: the C library sees it)
    lib.np_env_read(out)
    assert list(out)[:4] == [1, 0, SMALL_HELP_MAX, 1], "read per call: tests switch paths inside one process"
    assert list(out)[4:] == [ENV_DEFAULT[k] for k in ENV_ORDER[4:]], "read once per process, by the first call"
