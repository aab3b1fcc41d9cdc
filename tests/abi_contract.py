"""Harness of tests/test_abi_contract_gpu.py: one C-ABI call (or a chain of calls that share a workspace) on buffers cut from ONE
arena, every buffer between canaries, the workspace at exactly the queried size and filled with a chosen poison.

What include/obb_hip.h promises for every entry that takes `ws, ws_bytes`, and what this module makes observable:
  * `ws` needs exactly what the *_workspace_bytes query returns   -> `ws` is a slice of exactly that many bytes;
  * `ws` is 256-byte aligned                                      -> every buffer starts on a 256-byte boundary of the arena;
  * inputs are never modified                                     -> check() compares every input with its upload, byte for byte;
  * the entry writes only its outputs                             -> a guard band of GUARD bytes of 0xC3 in front of and behind
                                                                     every buffer; outputs are pre-filled with 0xC3 as well;
  * all work is enqueued on `stream`                              -> run_on_side_stream(): the inputs hold poison until a delay
                                                                     on the caller's stream has passed.

REACH OF THE GUARDS: a stray store is seen when it lands within GUARD = 1 MiB of the buffer it belongs to (or in another buffer
of the call, whose contents are compared with the oracle or with the upload).  One that lands further away is outside the arena
and out of this harness's reach.

A Case describes one call: the device inputs (numpy arrays), the outputs (byte counts, or initial contents for buffers the
entry accumulates into), outputs in pinned host memory where the header asks for that, the workspace query, the call itself
and verify(), which holds the outputs to the oracle and returns the arrays that must be bit-identical from run to run."""
import numpy as np
import torch

GUARD = 1 << 20
FILL = 0xC3
ALIGN = 256
POISONS = ("00", "ff", "leftover")
OBB_ERR_WORKSPACE = -2


def _up(x, a=ALIGN):
    return (x + a - 1) // a * a


class Case:
    """entries: the header's names this case calls.  inputs: name -> numpy array (device inputs).  outputs: name -> byte count |
    numpy array (initial contents of a buffer that is accumulated into).  pinned: name -> byte count (outputs in pinned host
    memory).  ws_query(L) -> bytes (called at run time: the library sizes the workspace from the calling thread's grid cap).
    state_bytes(L) -> bytes of the caller-kept `state` (0: none).  call(L, P, ws, ws_bytes, stream, mark) -> rc, with P[name] the
    address of a buffer (an int; P['state'] the state), ws an int or None; a chain calls mark() behind its FIRST ABI call.
    verify(O) -> list of numpy arrays, O(name, dtype) being the buffer after the call; it asserts against the oracle.
    synchronous: the entry (or the chain) waits for the device by contract.  env: environment the library reads per call.
    index_inputs: names of floating inputs that carry indices (image / class columns): zero poison, like the integer arrays."""

    def __init__(self, name, entries, inputs, outputs, ws_query, call, verify, pinned=None, state_bytes=None, synchronous=False,
                 env=None, index_inputs=()):
        self.name, self.entries = name, tuple(entries)
        self.inputs = {k: np.ascontiguousarray(v) for k, v in inputs.items()}
        self.outputs, self.pinned = dict(outputs), dict(pinned or {})
        self.ws_query, self.call, self.verify = ws_query, call, verify
        self.state_bytes, self.synchronous, self.env, self.index_inputs = state_bytes, synchronous, dict(env or {}), tuple(index_inputs)

    def __repr__(self):
        return self.name


class Arena:
    """One uint8 tensor; buffers at 256-byte aligned offsets with GUARD bytes of FILL around each of them."""

    def __init__(self, device, sizes, pinned=False):
        self.off, self.size, self.guards = {}, dict(sizes), []
        cur = 0
        for name, nbytes in sizes.items():
            start = _up(cur + GUARD)
            self.guards.append((cur, start, name))
            self.off[name] = start
            cur = start + int(nbytes)
        total = _up(cur + GUARD)
        self.guards.append((cur, total, "end"))
        if pinned:
            self.mem = torch.full((total,), FILL, dtype=torch.uint8).pin_memory()
        else:
            self.mem = torch.full((total,), FILL, dtype=torch.uint8, device=device)
        assert self.mem.data_ptr() % ALIGN == 0 or not (pinned or self.mem.is_cuda)

    def view(self, name):
        return self.mem[self.off[name]:self.off[name] + self.size[name]]

    def ptr(self, name):
        return self.mem.data_ptr() + self.off[name]

    def check_guards(self):
        names = list(self.off)
        for i, (a, b, nxt) in enumerate(self.guards):
            g = self.mem[a:b]
            if bool((g != FILL).any()):
                bad = torch.nonzero(g != FILL).flatten()
                first, last = int(bad[0]), int(bad[-1])
                before = names[i - 1] if i > 0 else "start"
                raise AssertionError(f"guard between `{before}` and `{nxt}` damaged: {len(bad)} bytes, first {first} bytes behind the end of "
                                     f"`{before}`, last {b - a - last} bytes in front of `{nxt}`")


class Run:
    """The buffers of one case, laid out and filled; run() makes the call."""

    def __init__(self, L, dev, case, ws_mode="exact"):
        self.L, self.dev, self.case, self.ws_mode = L, dev, case, ws_mode
        self.ws_bytes = int(case.ws_query(L))
        assert self.ws_bytes > 0, "the workspace query refused the case's arguments"
        self.state_bytes = int(case.state_bytes(L)) if case.state_bytes else 0
        sizes = {k: v.nbytes for k, v in case.inputs.items()}
        sizes.update({k: (v.nbytes if isinstance(v, np.ndarray) else int(v)) for k, v in case.outputs.items()})
        # ws placements: exact | short (one byte less, and told so) | null | +8 / +128 (a misaligned pointer into a buffer that
        # is long enough: the entry must refuse it before anything reaches the device)
        self.shift = {"+8": 8, "+128": 128}.get(ws_mode, 0)
        sizes["ws"] = self.ws_bytes - 1 if ws_mode == "short" else self.ws_bytes + self.shift
        if self.state_bytes:
            sizes["state"] = self.state_bytes
        self.arena = Arena(dev, sizes)
        self.host = Arena(dev, case.pinned, pinned=True) if case.pinned else None
        self.uploads = {k: torch.from_numpy(v.view(np.uint8).reshape(-1)).to(dev) for k, v in case.inputs.items()}
        self.initial = {k: torch.from_numpy(v.view(np.uint8).reshape(-1)).to(dev) for k, v in case.outputs.items() if isinstance(v, np.ndarray)}
        for k, t in self.initial.items():
            self.arena.view(k).copy_(t)
        if self.state_bytes:
            self.arena.view("state").zero_()                     # zeroed ONCE by the caller, as the header demands; never poisoned
        self.load_inputs()

    def load_inputs(self):
        for k, t in self.uploads.items():
            self.arena.view(k).copy_(t)

    def poison_inputs(self):
        """NaN bit patterns (all ones) for floating data, zeros for every index / offset / count array -- and for the floating
        arrays that carry an image or class index in a column (Case.index_inputs)."""
        for k, v in self.case.inputs.items():
            self.arena.view(k).fill_(0xFF if v.dtype.kind == "f" and k not in self.case.index_inputs else 0)

    def poison_ws(self, mode, leftover=None):
        ws = self.arena.view("ws")
        if mode == "00":
            ws.zero_()
        elif mode == "ff":
            ws.fill_(0xFF)
        else:
            assert mode == "leftover" and leftover is not None and leftover.numel() > 0
            reps = (ws.numel() + leftover.numel() - 1) // leftover.numel()
            ws.copy_(leftover.repeat(reps)[:ws.numel()] if reps > 1 else leftover[:ws.numel()])

    def pointers(self):
        P = {k: self.arena.ptr(k) for k in self.arena.off if k != "ws"}
        if self.host is not None:
            P.update({k: self.host.ptr(k) for k in self.host.off})
        P.setdefault("state", 0)
        P["_peek"] = self.output                                 # (a chain that reads a count back between its calls)
        return P

    def run(self, stream=0, mark=None):
        ws = None if self.ws_mode == "null" else self.arena.ptr("ws") + self.shift
        told = self.ws_bytes - 1 if self.ws_mode == "short" else self.ws_bytes
        return self.case.call(self.L, self.pointers(), ws, told, stream, mark or (lambda: None))

    def check(self):
        """After a stream synchronise: every guard byte intact, every input byte-identical to its upload."""
        self.arena.check_guards()
        if self.host is not None:
            self.host.check_guards()
        for k, t in self.uploads.items():
            if not torch.equal(self.arena.view(k), t):
                first = int(torch.nonzero(self.arena.view(k) != t).flatten()[0])
                raise AssertionError(f"input `{k}` was modified, first at byte {first}")

    def output(self, name, dtype):
        a = self.host if (self.host is not None and name in self.host.off) else self.arena
        return a.view(name).cpu().numpy().copy().view(dtype)

    def outputs_untouched(self):
        """Every output still holds its initial contents (0xC3, or what an accumulating buffer was given); state still zero."""
        for k in self.case.outputs:
            v = self.arena.view(k)
            same = torch.equal(v, self.initial[k]) if k in self.initial else bool((v == FILL).all())
            assert same, f"output `{k}` was written by a call that was refused"
        if self.host is not None:
            for k in self.host.off:
                assert bool((self.host.view(k) == FILL).all()), f"pinned output `{k}` was written by a call that was refused"
        if self.state_bytes:
            assert not bool(self.arena.view("state").any()), "`state` is not zero after a call that was refused"


def _sync(dev):
    torch.cuda.current_stream(dev).synchronize()


def same_arrays(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def run_exact(L, dev, case, poison, leftover=None):
    """One call on the exact workspace filled with `poison` -> (verify()'s arrays, the workspace as the call left it)."""
    r = Run(L, dev, case)
    r.poison_ws(poison, leftover)
    _sync(dev)
    rc = r.run(torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0, (case, "rc", rc)
    _sync(dev)
    r.check()
    if r.state_bytes:
        assert not bool(r.arena.view("state").any()), "`state` must be left zeroed by the call"
    res = case.verify(r.output)
    return res, r.arena.view("ws").clone()


def run_poisons(L, dev, case, donor):
    """The case on all three fills; `donor`: another case of the same entry whose workspace is the `leftover` fill."""
    _, left = run_exact(L, dev, donor, "00")
    results = {p: run_exact(L, dev, case, p, left)[0] for p in POISONS}
    for p in POISONS[1:]:
        assert same_arrays(results[POISONS[0]], results[p]), (case, "the result depends on what the workspace held:", POISONS[0], "vs", p)
    return results[POISONS[0]]


def run_refused(L, dev, case, ws_mode):
    """ws one byte short, NULL or misaligned: OBB_ERR_WORKSPACE, and nothing was written anywhere."""
    r = Run(L, dev, case, ws_mode)
    r.poison_ws("ff")
    _sync(dev)
    rc = r.run(torch.cuda.current_stream(dev).cuda_stream)
    _sync(dev)
    assert rc == OBB_ERR_WORKSPACE, (case, ws_mode, "rc", rc)
    r.check()
    r.outputs_untouched()
    if ws_mode != "null":
        assert bool((r.arena.view("ws") == 0xFF).all()), "the workspace was written by a call that was refused"


def run_capped(L, dev, case, grid=8):
    """Workspace query AND call under obb_nms_set_max_grid(grid) on this thread: one call sizes both from the same value."""
    L.obb_nms_set_max_grid(grid)
    try:
        res, _ = run_exact(L, dev, case, "ff")
    finally:
        L.obb_nms_set_max_grid(0)
    return res


def delay(dev, a, iters):
    """`iters` dependent matrix products on the current stream (plain torch ops): the device-side delay of run_on_side_stream."""
    for _ in range(iters):
        a = torch.mm(a, a).clamp_(-1.0, 1.0)
    return a


def run_on_side_stream(L, dev, case, iters, seed_matrix):
    """The call on a stream of its own.  Order of work on that stream: poison in the workspace and in the inputs (NaN bits / zero
    indices), the delay, the workspace poison once more, the real inputs, the ABI call.  A launch that went to the null stream
    instead reads poison; a memset or zeroing kernel that went there runs before the second poison and is overwritten by it:
    either way verify() fails.  Returns (arrays, whether the delay was still running when the ABI call returned)."""
    r = Run(L, dev, case)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        r.poison_ws("ff")
        r.poison_inputs()
        delay(dev, seed_matrix, iters)
        ev = torch.cuda.Event()
        ev.record(side)
        r.poison_ws("ff")                                        # again, BEHIND the delay: a leaked zeroing has run by now and
        r.load_inputs()                                          # is overwritten -- the kernels then meet 0xFF counters
        pending = []
        rc = r.run(side.cuda_stream, mark=lambda: pending.append(not ev.query()))
        if not pending:
            pending.append(not ev.query())
        assert rc == 0, (case, "rc", rc)
    side.synchronize()
    torch.cuda.current_stream(dev).wait_stream(side)
    r.check()
    return case.verify(r.output), pending[0]
