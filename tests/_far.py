"""Helpers of tests/test_far_offsets_host.py and tests/test_z_far_offsets_gpu.py (not collected): rows of one tensor placed so far
apart that the offset of row 1 passes 2^31 bytes, 2^32 bytes, 2^31 elements or 2^32 elements.

Arena.  ONE flat allocation of 2^(b+1) + 2^21 four-byte words (b = 31 on the device: 16 GiB + 8 MiB), every word the sentinel
SENT: a quiet NaN with a payload no kernel produces.  A case places each tensor in a *lane*: a small base offset of its own, rows S
words apart.  Row 0 is near, row 1 is far.  All rows of all tensors of a call are *windows*; whatever the call writes must land in
a window, so after the call

    non-sentinel words of the whole arena  ==  non-sentinel words inside the windows

-- a store whose index was truncated lands BELOW its true address, outside every window, and is counted wherever that is.  A load
whose index was truncated reads the sentinel NaN (or, through a buffer descriptor whose extent was truncated, 0): the result then
differs from the call on compact strides, which the GPU module compares bit for bit.  The windows are refilled afterwards.

Stride classes, in four-byte words, for b = 31 (`strides(b)` scales them: the host module runs the same machinery on a numpy arena
with b = 15, where "32 bits" means 16):

    A   2^29 + 64    row 1 begins past 2^31 bytes
    B   2^30 + 64    ... past 2^32 bytes
    C   2^31 + 64    ... past 2^31 elements
    D   2^32 + 64    ... past 2^32 elements
    A'  2^29 + 61    as A, 1 mod 4: the unaligned (scalar) load and store paths

`Arena` works on anything that slices like a flat integer array (a numpy array, a torch tensor), so the host module tests the
class the GPU module uses."""
import itertools

SENT = 0x7FC5A17E                    # a quiet NaN (exponent all ones, top mantissa bit set) with payload 0x5A17E
SPARE = 1 << 21                      # words behind 2^(b+1): room for row 1 of every lane in class D
LANE = 1 << 17                       # words between the bases of two lanes (a row is at most LANE - 64 words)
CLASSES = ("A", "A'", "B", "C", "D")


def strides(b=31):
    """{class: words between rows} with 2^b in the place of 2^31"""
    return {"A": (1 << (b - 2)) + 64, "A'": (1 << (b - 2)) + 61, "B": (1 << (b - 1)) + 64, "C": (1 << b) + 64, "D": (1 << (b + 1)) + 64}


def arena_words(b=31):
    return (1 << (b + 1)) + SPARE


def compact_stride(S, row_words):
    """a small stride in S's residue class mod 4 words that holds a row (the plan and the vector / scalar path stay the same)"""
    return (row_words + 3) // 4 * 4 + 8 + S % 4


def windows_of(base, shape, stride_words):
    """[(first word, words)] of a view: the trailing contiguous dimensions form one window per index of the leading ones"""
    inner, d = 1, len(shape)
    while d > 0 and stride_words[d - 1] == inner:
        inner *= shape[d - 1]
        d -= 1
    return [(base + sum(i * s for i, s in zip(idx, stride_words[:d])), inner) for idx in itertools.product(*[range(n) for n in shape[:d]])]


class Arena:
    def __init__(self, words, chunk=1 << 28):
        self.words, self.n, self.chunk = words, int(words.shape[0]), chunk
        self.windows = []            # (first word, words), disjoint
        self.scans = 0

    def _chunks(self, lo, hi):
        for c in range(lo, hi, self.chunk):
            yield c, min(c + self.chunk, hi)

    def fill(self, value=SENT):
        for lo, hi in self._chunks(0, self.n):
            self.words[lo:hi] = value

    def declare(self, lo, n):
        assert n > 0 and 0 <= lo and lo + n <= self.n, f"window [{lo}, {lo + n}) leaves the arena of {self.n} words"
        for a, m in self.windows:
            assert lo + n <= a or a + m <= lo, f"window [{lo}, {lo + n}) overlaps [{a}, {a + m})"
        self.windows.append((lo, n))

    def count(self, lo, hi):
        """non-sentinel words in [lo, hi)"""
        return sum(int((self.words[a:b] != SENT).sum()) for a, b in self._chunks(lo, hi))

    def foreign(self):
        """non-sentinel words outside every declared window"""
        self.scans += 1
        return self.count(0, self.n) - sum(self.count(lo, lo + n) for lo, n in self.windows)

    def reset(self):
        for lo, n in self.windows:
            self.words[lo:lo + n] = SENT
        self.windows = []


class FarFault(AssertionError):
    pass


def check_rows(arena, got, want, what=""):
    """after a call: nothing outside the windows changed, and the rows read back equal the expected ones bit for bit"""
    stray = arena.foreign()
    if stray:
        raise FarFault(f"{what}: {stray} words outside the declared windows were written")
    for i, (g, w) in enumerate(zip(got, want)):
        if not (g.shape == w.shape and bool((g == w).all())):
            bad = g != w if g.shape == w.shape else None
            detail = "" if bad is None else (f": {int(bad.sum())} of {bad.shape[0]} words differ; the row holds {int((g == 0).sum())} zero and "
                                             f"{int((g == SENT).sum())} sentinel words")
            raise FarFault(f"{what}: row {i} differs from the compact call{detail}")


# ---- torch side (imported lazily: the module itself needs neither torch nor a device) -------------------------------------------------------
class Lanes:
    """Places the tensors of ONE call: far=True in the arena, rows S apart; far=False the same call on compact strides in small buffers
    of its own (the expected bits).  view() returns a strided torch view to hand to a phasegen.ops wrapper."""

    def __init__(self, arena, S, far):
        self.arena, self.S, self.far = arena, S, far
        self.next_lane = 0
        self.outs = []               # (name, flat tensor, windows) to read back
        self.initial = []            # what results() would have returned before the call (a refused call must leave exactly this)

    def _alloc(self, dtype, shape, stride_el, per_word, foot_el):
        import torch
        span_el = sum((n - 1) * s for n, s in zip(shape, stride_el)) + 1
        if self.far:
            flat = self.arena.words.view(dtype)     # (4-byte types: the same indices; bf16: twice as many)
            while True:                             # the first lane in which no window of this view meets one declared before
                base = 64 + self.next_lane * LANE
                wins = windows_of(base * per_word, shape, stride_el)
                lo_hi = [(lo // per_word, -(-(lo + n) // per_word)) for lo, n in wins]
                if all(hi <= a or a + m <= lo for lo, hi in lo_hi for a, m in self.arena.windows):
                    break
                self.next_lane += 1
            for lo, hi in lo_hi:
                self.arena.declare(lo, hi - lo)
            self.next_lane += -(-(foot_el // per_word + 64) // LANE)          # the lanes the near end of this view covers
            return torch.as_strided(flat, shape, stride_el, base * per_word), wins, flat
        buf = torch.empty(64 + -(-span_el // per_word) + 64, dtype=torch.int32, device=self.arena.words.device)
        buf.fill_(SENT)              # (the same words as the arena's, whatever the element size: untouched tails compare equal)
        flat = buf.view(dtype)
        return torch.as_strided(flat, shape, stride_el, 64 * per_word), windows_of(64 * per_word, shape, stride_el), flat

    def view(self, name, shape, far_dims=(0,), dtype=None, data=None, out=False, S=None):
        """a view of `shape` whose dimensions in far_dims are S elements apart when far, and compactly
        strided in S's residue class otherwise; the other dimensions are contiguous inside.  data: a tensor copied in window by
        window.  out=True: the windows are read back by results()."""
        import torch
        dtype = dtype or torch.float32
        per_word = 4 // torch.empty(0, dtype=dtype).element_size()
        stride_el, inner, foot = [0] * len(shape), 1, None
        for d in range(len(shape) - 1, -1, -1):
            if d in far_dims:
                S = self.S if S is None else S           # (S=: a stride of this view's own, e.g. the largest one a call accepts)
                s = S if self.far else compact_stride(S, inner)
                assert s >= inner, (name, d, s, inner)
                foot = inner if foot is None else foot
                stride_el[d], inner = s, s * (shape[d] - 1) + inner
            else:
                stride_el[d], inner = inner, inner * shape[d]
        v, wins, flat = self._alloc(dtype, tuple(shape), tuple(stride_el), per_word, inner if foot is None else foot)
        if data is not None:
            src = data.to(device=flat.device, dtype=dtype).contiguous().view(-1)
            at = 0
            for lo, n in wins:
                flat[lo:lo + n].copy_(src[at:at + n])
                at += n
            assert at == src.numel(), (name, at, src.numel())
        if out:
            self.outs.append((name, flat, wins))
            self.initial += self._read(flat, wins)
        return v

    def dense(self, name, shape, dtype=None, data=None, out=False):
        """a plain dense device tensor outside the arena (an operand without a stride field): sentinel-filled, or a copy of data"""
        import torch
        dtype = dtype or torch.float32
        n = 1
        for d in shape:
            n *= d
        size = torch.empty(0, dtype=dtype).element_size()
        buf = torch.empty(max(n * size // 4, 1) if size >= 4 else (n + 1) // 2, dtype=torch.int32, device=self.arena.words.device)
        buf.fill_(SENT)
        flat = buf.view(dtype)[:n]
        if data is not None:
            flat.copy_(data.to(device=flat.device, dtype=dtype).contiguous().view(-1))
        if out:
            self.outs.append((name, flat, [(0, n)]))
            self.initial += self._read(flat, [(0, n)])
        return flat.view(shape)

    @staticmethod
    def _read(flat, wins):
        import torch
        it = {2: torch.int16, 4: torch.int32, 8: torch.int64}[flat.element_size()]
        return [flat[lo:lo + n].clone().view(it) for lo, n in wins]

    def results(self):
        """the output windows, as int16 / int32 words, in declaration order"""
        res = []
        for name, flat, wins in self.outs:
            res += self._read(flat, wins)
        return res
