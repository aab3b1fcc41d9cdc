"""CPU: the caller's side of the fused NMS driver -- obb_nms_obb_hints_init / _cap / _word / _update of include/obb_hip.h
(csrc/nmsobb_hints.h), the one implementation both bindings call -- against a frozen pure-Python restatement of the policy as
utils/general.py:_run_fused spelled it out before it moved into the library (module dicts per shape, the four retry cases, the
8-call hold).  Synthetic out_count / status words, no device call.  Exact: the action, cap_img, the next expected_cand word and
every field of the struct after every step."""
import ctypes as C
import os
import random

import pytest

from yolov5_obb_amd import _lib

DONE, RETRY, RETRY_SMALL_GRID = 0, 1, 2          # include/obb_hip.h OBB_HINTS_*
FIELDS = ("cap", "cand", "seg", "hold_cand", "hold_seg", "small_boxes", "small_resolved")


class ParentPolicy:
    """The policy of the ctypes binding before the move, restated (frozen: this is the oracle, it does not follow the product).
    One shape: `key` is constant and the module dicts are this object's."""
    _SORT_LDS_HINT, _SORT_LDS_MAX, _SEG_SMALL, _HOLD = 6144, 8192, 384, 8
    key = "shape"

    def __init__(self):
        self._cap_memo, self._cand_memo, self._seg_memo, self._hold, self._small_memo = {}, {}, {}, {}, {}

    def first_cap(self, worst):
        return min(worst, max(self._cap_memo.get(self.key, 0), 65536))

    def word(self):
        hint = int(self._cand_memo.get(self.key, self._SORT_LDS_HINT))
        seg_hint = int(self._seg_memo.get(self.key, 1))
        return (hint & 0xffffffff) | ((seg_hint & 0x1fffffff) << 32) | ((1 << 62) if self._small_memo.get(self.key) else 0)

    def force(self, cand=None, seg=None):               # hint_set
        if cand is not None:
            self._cand_memo[self.key] = int(cand); self._hold[self.key, "cand"] = 0
        if seg is not None:
            self._seg_memo[self.key] = int(seg); self._hold[self.key, "seg"] = 0

    def update(self, cap, worst, counts, status):
        """What one pass of the loop did with the words it read back; -> (action, cap)."""
        key, bs = self.key, len(counts)
        hint = int(self._cand_memo.get(key, self._SORT_LDS_HINT))
        m = list(counts) + list(status)
        self._small_memo[key] = bool((m[bs + 1] >> 62) & 1)
        self._small_memo[key, "resolved"] = bool((m[bs + 1] >> 61) & 1)
        seg_max, m[bs + 1] = (m[bs + 1] >> 32) & 0x1fffffff, m[bs + 1] & 0xffffffff
        if m[bs] == -1:
            self._seg_memo[key] = max(int(seg_max), self._SEG_SMALL + 1)
            self._hold[key, "seg"] = self._HOLD
            return RETRY, cap
        if min(m[:bs]) < 0:
            return RETRY_SMALL_GRID, cap
        if m[bs] > cap:
            return RETRY, min(worst, max(int(m[bs]), 2 * cap))
        if 0 < hint <= self._SORT_LDS_HINT and m[bs + 1] > self._SORT_LDS_MAX:
            self._cand_memo[key] = int(m[bs + 1])
            self._hold[key, "cand"] = self._HOLD
            return RETRY, cap
        self._cap_memo[key] = cap
        cand, seg = int(m[bs + 1]), int(seg_max)
        if self._hold.get((key, "cand"), 0) > 0 and cand > self._SORT_LDS_HINT * 3 // 4:
            self._hold[key, "cand"] -= 1
            cand = max(cand, self._SORT_LDS_HINT + 1)
        else:
            self._hold[key, "cand"] = 0
        if self._hold.get((key, "seg"), 0) > 0 and (seg == 0 or seg > self._SEG_SMALL * 3 // 4):
            self._hold[key, "seg"] -= 1
            seg = max(seg, self._SEG_SMALL + 1)
        else:
            self._hold[key, "seg"] = 0
        self._cand_memo[key] = cand
        self._seg_memo[key] = seg
        return DONE, cap

    def fields(self):
        key = self.key
        return {"cap": self._cap_memo.get(key, 0), "cand": self._cand_memo.get(key, self._SORT_LDS_HINT), "seg": self._seg_memo.get(key, 1),
                "hold_cand": self._hold.get((key, "cand"), 0), "hold_seg": self._hold.get((key, "seg"), 0),
                "small_boxes": int(self._small_memo.get(key, False)), "small_resolved": int(self._small_memo.get((key, "resolved"), False))}


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


class Pair:
    """The library's struct and the oracle, driven in lockstep; every method compares all there is to compare."""

    def __init__(self, L):
        self.L, self.h, self.ref = L, _lib.NmsObbHints(), ParentPolicy()
        for name in FIELDS + ("reserved",):
            setattr(self.h, name, -12345)                # init must write every field
        L.obb_nms_obb_hints_init(C.byref(self.h))
        assert self.h.reserved == 0
        self.same()

    def same(self):
        assert {n: getattr(self.h, n) for n in FIELDS} == self.ref.fields()
        assert self.L.obb_nms_obb_hints_word(C.byref(self.h)) == self.ref.word()

    def first_cap(self, worst):
        cap = self.L.obb_nms_obb_hints_cap(C.byref(self.h), worst)
        assert cap == self.ref.first_cap(worst)
        return cap

    def force(self, cand=None, seg=None):                # what hint_set of either binding stores
        if cand is not None:
            self.h.cand, self.h.hold_cand = cand, 0
        if seg is not None:
            self.h.seg, self.h.hold_seg = seg, 0
        self.ref.force(cand, seg)
        self.same()

    def step(self, cap, worst, counts, st0, st1):
        cap_c = C.c_int64(cap)
        cnt = (C.c_int64 * len(counts))(*counts)
        st = (C.c_int64 * 2)(st0, st1)
        action = self.L.obb_nms_obb_hints_update(C.byref(self.h), C.byref(cap_c), worst, cnt, len(counts), st)
        want = self.ref.update(cap, worst, counts, (st0, st1))
        assert (action, cap_c.value) == want, (counts, st0, hex(st1))
        assert list(cnt) == list(counts) and list(st) == [st0, st1]     # inputs are inputs
        self.same()
        return action, cap_c.value


def st1(cand, seg=0, small=0, resolved=0):
    return cand | (seg << 32) | (resolved << 61) | (small << 62)


def test_struct_is_eight_words():
    assert C.sizeof(_lib.NmsObbHints) == 64 and [f[0] for f in _lib.NmsObbHints._fields_][:7] == list(FIELDS)


def test_no_history(L):
    p = Pair(L)
    assert (p.h.cap, p.h.cand, p.h.seg) == (0, 6144, 1)
    assert p.first_cap(10 ** 6) == 65536 and p.first_cap(4000) == 4000 and p.first_cap(65536) == 65536
    assert p.step(65536, 10 ** 6, [3, 0], 1700, st1(1700, 120)) == (DONE, 65536)
    assert (p.h.cap, p.h.cand, p.h.seg, p.h.hold_cand, p.h.hold_seg) == (65536, 1700, 120, 0, 0)
    assert p.first_cap(10 ** 6) == 65536


def test_large_segment_retry_and_its_hold(L):
    """status[0] == -1: nothing is valid, the reported segment (at least 385) is the hint, held for 8 calls while the batch stays
    above 288 boxes per segment (or does not report a segment), released at once below."""
    p = Pair(L)
    cap = p.first_cap(900000)
    assert p.step(cap, 900000, [0] * 16, -1, st1(5000, 700)) == (RETRY, cap)
    assert (p.h.seg, p.h.hold_seg) == (700, 8)
    assert p.step(cap, 900000, [5] * 16, 5000, st1(5000, 700)) == (DONE, cap)
    assert (p.h.seg, p.h.hold_seg) == (700, 7)
    for k, seg in enumerate((300, 289, 0, 384, 385, 290, 0)):                  # hovering around the limit: held, counted down
        assert p.step(p.first_cap(900000), 900000, [5] * 16, 5000, st1(5000, seg))[0] == DONE
        assert (p.h.seg, p.h.hold_seg) == (max(seg, 385), 6 - k)
    assert p.step(cap, 900000, [5] * 16, 5000, st1(5000, 300)) == (DONE, cap)  # the hold has run out
    assert (p.h.seg, p.h.hold_seg) == (300, 0)
    # a report below the small kernel's own limit still answers with 385; a drop to 288 releases the hold at once
    assert p.step(cap, 900000, [0], -1, st1(100, 12))[0] == RETRY and (p.h.seg, p.h.hold_seg) == (385, 8)
    assert p.step(cap, 900000, [1], 100, st1(100, 400))[0] == DONE and (p.h.seg, p.h.hold_seg) == (400, 7)
    assert p.step(cap, 900000, [1], 100, st1(100, 288))[0] == DONE and (p.h.seg, p.h.hold_seg) == (288, 0)
    assert p.step(cap, 900000, [1], 100, st1(100, 0))[0] == DONE and (p.h.seg, p.h.hold_seg) == (0, 0)     # seg_max == 0, no hold
    # -1 wins over everything else the words say
    assert p.step(cap, 900000, [-1, 4], -1, st1(9000, 500, 1, 1))[0] == RETRY and (p.h.small_boxes, p.h.small_resolved) == (1, 1)


def test_small_grid_retry(L):
    p = Pair(L)
    cap = p.first_cap(500000)
    before = p.ref.fields()
    assert p.step(cap, 500000, [4, -1], 2000, st1(2000, 90)) == (RETRY_SMALL_GRID, cap)
    assert p.ref.fields() == before                                             # nothing is learned from an aborted call
    assert p.step(cap, 500000, [-1, -1], cap + 5, st1(9000, 90))[0] == RETRY_SMALL_GRID   # ... and it is looked at before cap and sort hint
    assert p.step(cap, 500000, [4, 6], 2000, st1(2000, 90)) == (DONE, cap)


def test_cap_overflow(L):
    p = Pair(L)
    cap = p.first_cap(10 ** 6)
    assert p.step(cap, 10 ** 6, [0], 70000, st1(70000)) == (RETRY, 131072)      # doubling
    assert p.step(131072, 10 ** 6, [0], 400000, st1(400000)) == (RETRY, 400000)   # jumping to the reported count
    assert p.step(400000, 10 ** 6, [0], 900000, st1(900000)) == (RETRY, 900000)
    assert p.step(900000, 10 ** 6, [0], 950000, st1(950000)) == (RETRY, 10 ** 6)  # clamped at worst
    assert p.h.cap == 0                                                         # committed with a valid call only
    assert p.step(10 ** 6, 10 ** 6, [7], 950000, st1(950000))[0] == RETRY      # (then the undersold sort hint, next test)
    assert p.step(10 ** 6, 10 ** 6, [7], 950000, st1(950000)) == (DONE, 10 ** 6)
    assert p.h.cap == 10 ** 6 and p.first_cap(10 ** 6) == 10 ** 6 and p.first_cap(2 * 10 ** 6) == 10 ** 6
    q = Pair(L)
    assert q.step(3000, 100000, [0], 3001, st1(3001)) == (RETRY, 6000)
    assert q.step(65536, 100000, [0], 65537, st1(65537)) == (RETRY, 100000)


def test_undersold_sort_hint_and_its_hold(L):
    p = Pair(L)
    cap = p.first_cap(900000)
    assert p.step(cap, 900000, [9], 8192, st1(8192, 50)) == (DONE, cap)        # 8192 still fits the in-LDS sort
    assert p.h.cand == 8192 and p.step(cap, 900000, [9], 9000, st1(9000, 50)) == (DONE, cap)   # a hint above 6144 is never undersold
    p.force(cand=100)
    assert p.step(cap, 900000, [0], 8193, st1(8193, 50)) == (RETRY, cap)
    assert (p.h.cand, p.h.hold_cand) == (8193, 8)
    for k, cand in enumerate((8193, 4609, 6144, 6145, 5000, 7000, 4700, 4609)):  # above 4608: held at 6145 or more
        assert p.step(cap, 900000, [9], cand, st1(cand, 50))[0] == DONE
        assert (p.h.cand, p.h.hold_cand) == (max(cand, 6145), 7 - k)
    assert p.step(cap, 900000, [9], 5000, st1(5000, 50))[0] == DONE and (p.h.cand, p.h.hold_cand) == (5000, 0)
    p.force(cand=6144)
    assert p.step(cap, 900000, [0], 20000, st1(20000, 50))[0] == RETRY
    assert p.step(cap, 900000, [9], 20000, st1(20000, 50))[0] == DONE and p.h.hold_cand == 7
    assert p.step(cap, 900000, [9], 4608, st1(4608, 50))[0] == DONE and (p.h.cand, p.h.hold_cand) == (4608, 0)   # released at once


def test_hint_zero(L):
    """A hint of 0 (the generic sort, always valid) is never undersold, and the next call gets what this one reported."""
    p = Pair(L)
    p.force(cand=0)
    assert p.L.obb_nms_obb_hints_word(C.byref(p.h)) == 1 << 32
    cap = p.first_cap(900000)
    assert p.step(cap, 900000, [9, 9], 30000, st1(30000)) == (DONE, cap)
    assert (p.h.cand, p.h.seg, p.h.hold_cand) == (30000, 0, 0)
    p.force(cand=0, seg=1)
    assert p.step(cap, 900000, [9, 9], 3000, st1(3000, 200)) == (DONE, cap) and (p.h.cand, p.h.seg) == (3000, 200)


def test_small_box_bits(L):
    """status[1] bit 62 comes back as bit 62 of the next word; bit 61 is kept for hint_get only; both before any retry."""
    p = Pair(L)
    cap = p.first_cap(900000)
    for small, resolved in ((1, 0), (1, 1), (0, 1), (0, 0)):
        assert p.step(cap, 900000, [2], 1000, st1(1000, 40, small, resolved)) == (DONE, cap)
        assert (p.h.small_boxes, p.h.small_resolved) == (small, resolved)
        assert p.L.obb_nms_obb_hints_word(C.byref(p.h)) == 1000 | (40 << 32) | (small << 62)
    assert p.step(cap, 900000, [0], cap + 1, st1(1000, 40, 1, 1))[0] == RETRY and (p.h.small_boxes, p.h.small_resolved) == (1, 1)
    assert p.step(cap, 900000, [-1], 0, st1(1000, 40, 0, 1))[0] == RETRY_SMALL_GRID and (p.h.small_boxes, p.h.small_resolved) == (0, 1)
    p.force(cand=100)
    assert p.step(cap, 900000, [0], 9000, st1(9000, 40, 1, 0))[0] == RETRY and (p.h.small_boxes, p.h.small_resolved) == (1, 0)


@pytest.mark.parametrize("binding", ("compiled", "ctypes"))
def test_hint_introspection_is_the_struct_per_thread_and_bounded(L, monkeypatch, binding):
    """hint_get / hint_set / hints_clear of utils/general.py on either binding (no device call): the same keys, the calling
    thread's shapes only, at most 512 of them."""
    import threading
    from yolov5_obb_amd.utils import general
    if binding == "ctypes":
        monkeypatch.setattr(_lib, "_ext", None)
        monkeypatch.setattr(_lib, "_ext_tried", True)
    else:
        if not os.path.exists(_lib.EXT_PATH):
            import __graft_entry__
            __graft_entry__.build_torch_ext()
            monkeypatch.setattr(_lib, "_ext_tried", False)
        assert _lib.compiled() is not None
    general.hints_clear()
    shape = ("cuda:0", 1000, 15, True, 0.25)
    assert general.hint_get(*shape) is None
    general.hint_set(*shape, cand=0)
    fresh = dict(cap=0, cand=0, seg=1, hold_cand=0, hold_seg=0, small_boxes=False, small_resolved=False)
    assert general.hint_get(*shape) == fresh
    general.hint_set(*shape, seg=400)
    assert general.hint_get(*shape) == dict(fresh, seg=400)
    seen = []
    t = threading.Thread(target=lambda: seen.append(general.hint_get(*shape)))
    t.start()
    t.join()
    assert seen == [None]                                # another thread has hints of its own
    for i in range(511):
        general.hint_set("cuda:0", 2000 + i, 15, True, 0.25, seg=1)
    assert general.hint_get(*shape) == dict(fresh, seg=400)                    # 512 shapes are kept ...
    general.hint_set("cuda:0", 2511, 15, True, 0.25, seg=1)
    assert general.hint_get(*shape) is None                                    # ... the next one starts over
    assert general.hint_get("cuda:0", 2511, 15, True, 0.25) == dict(fresh, cand=6144)
    general.hints_clear()
    assert general.hint_get("cuda:0", 2511, 15, True, 0.25) is None


def test_random_steps_equal_the_parent_policy(L):
    rng = random.Random(20261019)
    steps = 0
    around = lambda centres, spread: max(0, rng.choice(centres) + rng.randint(-spread, spread))
    for episode in range(250):                       # short ones: cap_img only grows within a shape's history
        p = Pair(L)
        worst = rng.choice((3000, 65536, 70000, 200000, 967680, 16128000))
        bs = rng.choice((1, 2, 16))
        cap = p.first_cap(worst)
        for _ in range(100):
            r = rng.random()
            if r < 0.02:
                p.force(cand=rng.choice((None, 0, 100, 6144, 6145)), seg=rng.choice((None, 0, 1, 384, 385)))
            cand_max = around((4608, 6144, 8192), rng.choice((2, 40, 3000)))
            seg_max = around((0, 288, 384), rng.choice((2, 30, 300)))
            word = st1(cand_max, seg_max, rng.random() < 0.1, rng.random() < 0.1)
            r = rng.random()
            if r < 0.12:
                st0 = -1
            elif r < 0.75:
                st0 = rng.choice((0, cand_max, cap, rng.randint(0, cap)))
            else:
                st0 = rng.choice((cap + 1, 2 * cap, 2 * cap + 1, rng.randint(cap + 1, 3 * cap), worst, worst + rng.randint(1, 50)))
            counts = [rng.randint(0, 1500) for _ in range(bs)]
            if rng.random() < 0.05:
                counts[rng.randrange(bs)] = rng.choice((-1, -1, -7))
            action, cap = p.step(cap, worst, counts, st0, word)
            steps += 1
            if action == DONE:
                cap = p.first_cap(worst)                 # the next call of the shape
    assert steps >= 20000
