"""Helpers of tests/test_z_workspace_gpu.py and tests/test_z_streams_gpu.py (not collected): the three contracts of the C ABI that
the wrappers in phasegen/ops.py hide -- a call gets EXACTLY the workspace its query asks for, may find anything in it, writes nothing
outside it, and runs on the stream it is given without waiting for the device.

``strict_workspaces(poison)`` replaces ``ops._StreamCache.get`` while its body runs.  Every request is served from a fresh uint8
buffer [front guard 4 KiB .. | view of exactly max(nbytes_fn(), at_least) bytes, 256-byte aligned (+ ``offset``) | rear guard], all of
it filled with ``poison``; ``ops._workspace`` and the wrappers that pass ``ws.numel()`` then hand the library the exact size by
themselves.  On exit it synchronises, asserts that both guards of every buffer still hold the poison and releases the buffers.

Poisons.  0xFF bytes are a NaN as float and as double and -1 as an integer: a sum over a slot nobody wrote becomes NaN.  A maximum
does not: fmaxf / fmax return the other operand, so the peak reductions (stitch, ISTFT, wave_compare) pass over such a slot.  0x7F
bytes are 3.39e38 as float and 1.4e306 as double, finite and larger than any partial: they win every maximum.  pg_phase_lock keeps
gather INDICES in its workspace, so its cases use 0x00 and stale contents of an earlier, larger call (``stale=``) instead: a mistake
has to show as wrong values, never as wrong addresses.
"""
import contextlib
import ctypes

import torch

POISONS = (0xFF, 0x7F)
FRONT = 4096
ALIGN = 256
REAR_MIN, REAR_MAX = 64 << 10, 64 << 20
HOLD_MAX = 2 << 30            # bytes of strict buffers held before the finished ones are checked and released (compositions)


def stream_symbols():
    """the entry points of include/phasegen.h that take a stream: int f(..., void* stream), the launch-free *_describe twins excluded"""
    from phasegen import _lib
    return [n for n, (res, args) in _lib.SYMBOLS.items()
            if res is ctypes.c_int and len(args) >= 2 and args[-1] is ctypes.c_void_p and not n.endswith("_describe")]


def workspace_symbols():
    """... and of those, the ones whose argument struct has a `workspace` field"""
    from phasegen import _lib
    out = []
    for n in stream_symbols():
        first = _lib.SYMBOLS[n][1][0]
        struct = getattr(first, "_type_", None)
        if struct is not None and any(f[0] == "workspace" for f in getattr(struct, "_fields_", ())):
            out.append(n)
    return out


def bits(t):
    """t as integers of its element size, for bit-for-bit comparison (NaN payloads and the sign of zero included)."""
    t = t.contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


class _Strict:
    def __init__(self, poison, offset, stale, keep, tamper=None):
        self.poison, self.offset, self.stale, self.keep = poison, offset, stale, keep
        self.tamper = tamper or {}        # symbol -> function(argument struct), applied just before the library is called
        self.calls = []                   # (symbol, stream handle, return code) of every stream-taking library call of the body
        self.held = []            # (buffer, start, need)
        self.requests = []        # need of every request, in order
        self.contents = []        # with keep: a copy of every view as the body left it
        self.checked = 0

    def get(self, cache, device, nbytes_fn, at_least=0):
        need = int(max(nbytes_fn(), at_least))
        assert need >= 0
        if sum(b.numel() for b, _, _ in self.held) > HOLD_MAX:
            self.check()
        rear = min(max(REAR_MIN, need), REAR_MAX)
        with torch.cuda.device(torch.device(device)):
            buf = torch.empty(FRONT + ALIGN + self.offset + need + rear, device=device, dtype=torch.uint8)
        buf.fill_(self.poison)
        start = FRONT + (-(buf.data_ptr() + FRONT)) % ALIGN + self.offset
        view = buf[start:start + need]
        assert view.numel() == need and (view.data_ptr() - self.offset) % ALIGN == 0
        if self.stale is not None:
            n = min(need, self.stale.numel())
            view[:n].copy_(self.stale[:n])
        self.held.append((buf, start, need))
        self.requests.append(need)
        return view

    def spy(self, name, fn):
        def call(*args):
            if name in self.tamper:
                self.tamper[name](args[0]._obj)           # byref(a)._obj: the struct the wrapper built
            rc = fn(*args)
            st = args[-1]
            self.calls.append((name, int(getattr(st, "value", st) or 0), rc))
            return rc
        return call

    def symbols(self):
        return {name for name, _, rc in self.calls if rc == 0}

    def check(self):
        """synchronise, assert the guards of every held buffer, release them"""
        torch.cuda.synchronize()
        held, self.held = self.held, []
        for buf, start, need in held:
            front_ok = bool((buf[:start] == self.poison).all())
            rear_ok = bool((buf[start + need:] == self.poison).all())
            if self.keep:
                self.contents.append(buf[start:start + need].clone())
            self.checked += 1
            assert front_ok, f"a byte in front of a {need}-byte workspace was written"
            assert rear_ok, f"a byte behind a {need}-byte workspace was written"


@contextlib.contextmanager
def strict_workspaces(poison, offset=0, stale=None, keep=False, tamper=None):
    """Serve every workspace request of the body from a fresh, exactly sized, poisoned and guarded buffer (module docstring).
    ``offset``: bytes by which the view is moved off its 256-byte alignment (the documented-alignment cases).  ``stale``: a uint8
    device tensor copied over the head of every view after the poison.  ``keep``: leave a copy of every view in ``.contents``.
    ``tamper``: {symbol: function(struct)} edits the argument struct a wrapper built just before the library sees it (the refusal
    cases).  Yields the bookkeeping object: ``.requests`` lists the sizes asked for, ``.calls`` every stream-taking library call of
    the body as (symbol, stream handle, return code)."""
    from phasegen import _lib, ops
    s = _Strict(poison, offset, stale, keep, tamper)
    lib = _lib.load()
    original = ops._StreamCache.get
    bound = {name: getattr(lib, name) for name in stream_symbols()}
    ops._StreamCache.get = lambda cache, device, nbytes_fn, at_least=0: s.get(cache, device, nbytes_fn, at_least)
    for name, fn in bound.items():
        setattr(lib, name, s.spy(name, fn))
    try:
        yield s
    finally:
        ops._StreamCache.get = original
        for name, fn in bound.items():
            setattr(lib, name, fn)
    s.check()                 # (not after an exception in the body: that one is the finding)


def strict_view(poison, need, offset=0):
    """One guarded view outside a wrapper: (checker, uint8 view of `need` bytes).  Call ``checker.check()`` after the work."""
    s = _Strict(poison, offset, None, True)
    return s, s.get(None, torch.device("cuda", torch.cuda.current_device()), lambda: need)


# ---- a stream that is busy for a known time -------------------------------------------------------------------------------------
_delay = {}


def _passes(buf, n):
    for _ in range(n):
        buf.neg_()


def delay_ms(min_ms=200.0):
    """(passes, milliseconds): how many in-place passes over the delay buffer take at least ``min_ms`` on an idle device, measured
    once per process with events and grown by doubling."""
    if "ms" not in _delay or _delay["ms"] < min_ms:
        buf = _delay.setdefault("buf", torch.zeros(1 << 29, device="cuda"))         # 2 GiB: a pass moves 4 GiB
        n = _delay.get("passes", 32)
        _passes(buf, 4)
        while True:
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            _passes(buf, n)
            b.record()
            torch.cuda.synchronize()
            ms = a.elapsed_time(b)
            if ms >= min_ms:
                break
            n *= 2
            assert n <= 1 << 16, f"the delay does not grow: {n} passes took {ms} ms"
        _delay.update(passes=n, ms=ms)
        print(f"\ndelayed_stream: {n} passes over {buf.numel() * 4 >> 20} MiB take {ms:.1f} ms on an idle device (at least {min_ms:.0f} ms wanted)")
    return _delay["passes"], _delay["ms"]


def side_stream():
    """the one side stream of the process (a torch.cuda.Stream: it does not block on the default stream)"""
    if "stream" not in _delay:
        _delay["stream"] = torch.cuda.Stream()
    return _delay["stream"]


def delayed_stream(min_ms=200.0):
    """A side stream (non-blocking with respect to the default stream, as every torch.cuda.Stream) with at least ``min_ms`` of work
    already enqueued on it.  The device is idle when the delay starts.  One stream per process: the allocator's pool of that stream is
    warm from the second case on."""
    n, _ = delay_ms(min_ms)
    side = side_stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        _passes(_delay["buf"], n)
    return side
