"""CPU: what stands behind tests/test_z_far_offsets_gpu.py.

1. The arena machinery of tests/_far.py catches what it is for: a numpy stand-in of a strided row copy runs on a scaled-down arena
   (2^15 in the place of 2^31, so "32-bit" registers hold 16 bits) with planted faults -- a truncated store index, a truncated load
   index, a truncated descriptor extent -- in byte and in element units, unsigned and signed.  Every planted fault is reported in
   exactly the classes whose offsets it cannot represent, and the honest copy passes everywhere.  The torch side (Lanes) places fp32
   and bf16 views on a CPU arena the same way.
2. Refusals before launch: the largest accepted extent of every operand a conv gathers is accepted by pg_conv_describe /
   pg_conv_fwd_h_describe and one element more is PG_ERR_SHAPE with the documented message; the weight bound, the wgrad's
   B*L < 2^24 - 64, and the B*L / B*C / n_signals * n_frames bounds of bn, clipnorm and stft_crops in the same table.
3. The coverage gate: every (symbol, field) with a 64-bit stride, pitch or length in phasegen/_lib.py is in the GPU module's table or
   in EXCLUDED with its reason."""
import ctypes

import numpy as np
import pytest

import _far
from test_kernel_families import _args

B15 = 15                             # the scaled arena: 2^15 stands for 2^31


# ---- 1. planted faults ------------------------------------------------------------------------------------------------------------------
def index_fault(unit, signed, bits=16):
    """how a `bits`-bit register holding (index * unit) misreads an index (unit 4: a byte offset, 1: an element index); None = lost"""
    def f(i):
        v = (i * unit) & ((1 << bits) - 1)
        if signed and v >= 1 << (bits - 1):
            return None                  # a negative offset: in front of the tensor (the stand-in drops the access)
        return v // unit
    return f


def faulty_copy(words, src, dst, rows, n, S_src, S_dst, fault, unit, signed):
    """dst row r = src row r (n words each, rows S words apart) as a kernel whose index registers follow the chosen model would do it.
    fault None: 64-bit throughout; "store" / "load": that index goes through the register; "extent": the load goes through a descriptor
    whose extent (rows - 1) * S_src + n was truncated, and a load past it returns 0"""
    wrong = index_fault(unit, signed)
    extent = (rows - 1) * S_src + n
    if fault == "extent":
        extent = ((extent * unit) & 0xFFFF) // unit
    for r in range(rows):
        for i in range(n):
            li, si = r * S_src + i, r * S_dst + i
            if fault == "load":
                li = wrong(li)
            if fault == "store":
                si = wrong(si)
            v = _far.SENT if li is None else (words[src + li] if li < extent else 0)
            if si is not None:
                words[dst + si] = v


def representable(S, n, unit, signed):
    top = (S + n) * unit
    return top < (1 << (15 if signed else 16))


def run_copy(cls, fault, unit, signed):
    """-> None if the machinery accepts the copy, else the FarFault's message"""
    S = _far.strides(B15)[cls]
    n = 37
    words = np.empty(_far.arena_words(B15), np.int32)
    arena = _far.Arena(words, chunk=1 << 14)
    arena.fill()
    data = (np.arange(2 * n, dtype=np.int32) + 1000).reshape(2, n)
    # the compact call: the honest copy on small strides
    Sc = _far.compact_stride(S, n)
    small = np.full(4 * Sc + 256, _far.SENT, np.int32)
    for r in range(2):
        small[64 + r * Sc:64 + r * Sc + n] = data[r]
    faulty_copy(small, 64, 64 + 2 * Sc, 2, n, Sc, Sc, None, 1, False)
    want = [small[64 + 2 * Sc + r * Sc:][:n].copy() for r in range(2)]
    assert all((w == d).all() for w, d in zip(want, data))
    src, dst = 64, 64 + _far.LANE
    for r in range(2):
        arena.declare(src + r * S, n)
        arena.declare(dst + r * S, n)
        words[src + r * S:src + r * S + n] = data[r]
    faulty_copy(words, src, dst, 2, n, S, S, fault, unit, signed)
    got = [words[dst + r * S:dst + r * S + n].copy() for r in range(2)]
    try:
        _far.check_rows(arena, got, want, f"{fault} {cls}")
    except _far.FarFault as e:
        return str(e)
    finally:
        arena.reset()
    return None


@pytest.mark.parametrize("cls", _far.CLASSES)
def test_the_honest_copy_passes_in_every_class(cls):
    assert run_copy(cls, None, 1, False) is None
    S = _far.strides()[cls]
    assert S % 4 == _far.compact_stride(S, 37) % 4 and _far.strides(B15)[cls] % 4 == S % 4


@pytest.mark.parametrize("signed", [False, True], ids=["unsigned", "signed"])
@pytest.mark.parametrize("unit", [4, 1], ids=["bytes", "elements"])
@pytest.mark.parametrize("fault", ["store", "load", "extent"])
def test_planted_faults_are_reported_where_the_offset_does_not_fit(fault, unit, signed):
    if fault == "extent" and signed:
        signed = False               # (an extent is a count: the unsigned rows cover it)
    caught = {cls: run_copy(cls, fault, unit, signed) for cls in _far.CLASSES}
    for cls, msg in caught.items():
        fits = representable(_far.strides(B15)[cls], 37, unit, signed)
        assert (msg is None) == fits, (fault, unit, signed, cls, msg)
    # every fault is caught in class D, a byte-offset fault from class B on (signed: from A), and no class is caught by accident
    assert caught["D"] is not None
    if unit == 4:
        assert caught["B"] is not None and caught["C"] is not None and (not signed or (caught["A"] is not None and caught["A'"] is not None))
    if fault == "store":
        assert all("outside the declared windows" in m or "differs" in m for m in caught.values() if m)


def test_the_classes_pass_the_thresholds_they_are_named_for():
    s = _far.strides()
    assert s["A"] * 4 > 2**31 > (s["A"] - 65) * 4 and s["A'"] * 4 > 2**31 and s["A'"] % 4 == 1
    assert s["B"] * 4 > 2**32 and s["B"] < 2**31 and s["C"] > 2**31 and s["C"] < 2**32 and s["D"] > 2**32
    assert _far.arena_words() == 2**32 + 2**21 and s["D"] + 15 * _far.LANE + 64 < _far.arena_words()
    f = np.array([_far.SENT], np.uint32).view(np.float32)[0]
    assert np.isnan(f)


def test_windows_and_overlaps():
    assert _far.windows_of(10, (2, 3, 4), (100, 4, 1)) == [(10, 12), (110, 12)]
    assert _far.windows_of(10, (2, 2, 4), (100, 10, 1)) == [(10, 4), (20, 4), (110, 4), (120, 4)]
    arena = _far.Arena(np.full(1000, _far.SENT, np.int32))
    arena.declare(10, 12)
    with pytest.raises(AssertionError):
        arena.declare(21, 5)
    with pytest.raises(AssertionError):
        arena.declare(990, 11)
    arena.words[500] = 7
    assert arena.foreign() == 1
    arena.declare(500, 1)
    assert arena.foreign() == 0
    arena.reset()
    assert arena.count(0, 1000) == 0


@pytest.mark.parametrize("cls", _far.CLASSES)
def test_lanes_place_fp32_and_bf16_views_on_a_cpu_arena(cls):
    """the torch side on a CPU arena: views are S apart when far and compact in S's residue class otherwise, data lands in the declared
    windows, results() reads them back, and a copy through the views passes check_rows"""
    import torch
    S = _far.strides(B15)[cls]
    arena = _far.Arena(torch.full((_far.arena_words(B15),), _far.SENT, dtype=torch.int32), chunk=1 << 14)
    x = torch.arange(2 * 3 * 10, dtype=torch.float32).view(2, 3, 10) + 1
    res = {}
    for far in (False, True):
        L = _far.Lanes(arena, S, far)
        xv = L.view("x", (2, 3, 10), data=x)
        yv = L.view("y", (2, 3, 10), out=True)
        hv = L.view("h", (2, 3, 16), dtype=torch.bfloat16, out=True)
        dv = L.dense("d", (2, 6), dtype=torch.float64, out=True)
        assert xv.stride() == ((S if far else _far.compact_stride(S, 30)), 10, 1) and xv.stride(0) % 4 == S % 4
        assert hv.stride(0) == (S if far else _far.compact_stride(S, 48)) and torch.equal(xv, x)
        assert (xv.data_ptr() - yv.data_ptr()) % 16 == 0 and xv.data_ptr() % 16 == 0
        halves = (_far.SENT >> 16, (_far.SENT & 0xFFFF) - 0x10000)          # the two int16 halves of the sentinel word
        assert all(bool(((i == halves[0]) | (i == halves[1])).all() if i.element_size() == 2 else (i.view(torch.int32) == _far.SENT).all()) for i in L.initial)
        for b in range(2):               # (row by row: what a kernel does)
            yv[b].copy_(xv[b] * 2)
            hv[b, :, :10].copy_(xv[b])
        dv.fill_(1.5)
        res[far] = L.results()
        if far:
            assert len(arena.windows) == 6 and arena.foreign() == 0
            _far.check_rows(arena, res[True], res[False], cls)
            arena.words[arena.windows[3][0] - 1] = 0          # one word in front of y's far row
            with pytest.raises(_far.FarFault, match="outside the declared windows"):
                _far.check_rows(arena, res[True], res[False], cls)
            arena.words[arena.windows[3][0] - 1] = _far.SENT
            arena.reset()
            assert arena.count(0, arena.n) == 0
    assert len(res[True]) == 2 + 2 + 1 and torch.equal(res[True][0].view(torch.float32).view(3, 10), x[0] * 2)


# ---- 2. refusals before launch -------------------------------------------------------------------------------------------------------------------
WORDS_MAX = 0x1ffffffb               # ((B - 1) bs + C L) * 4 < 0x7ffffff0
ACT_MSG = b"conv: activation tensor exceeds 2 GiB (31-bit buffer offsets)"
ADD_MSG = b"conv: dx_add / dx_ref exceeds 2 GiB (31-bit buffer offsets)"
GEOMS = [(False, 8, 8, 4, 2, 1, 30), (True, 32, 16, 8, 2, 1, 3), (False, 24, 40, 7, 3, 2, 50), (True, 24, 40, 7, 3, 2, 17)]


def lib():
    from phasegen import _lib
    return _lib, _lib.load()


def describe(a, op):
    _lib, L = lib()
    buf = ctypes.create_string_buffer(1024)
    rc = L.pg_conv_describe(ctypes.byref(a), op, buf, 1024)
    return rc, (L.pg_last_error_string() or b"") if rc else buf.value


# (op name, gathered operands: (stride field, channels, frames))
def gathered(op, Cin, Cout, Lin, Lout):
    return {"fwd": [("x_bs", Cin, Lin)], "dgrad": [("dy_bs", Cout, Lout), ("dx_add_bs", Cin, Lin), ("dx_ref_bs", Cin, Lin)],
            "wgrad": [("x_bs", Cin, Lin), ("dy_bs", Cout, Lout)]}[op]


@pytest.mark.parametrize("B", [2, 3])
@pytest.mark.parametrize("op", ["fwd", "dgrad", "wgrad"])
@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: f"{'T' if g[0] else 'C'}{g[1]}-{g[2]}-k{g[3]}s{g[4]}")
def test_conv_gathered_operands_at_and_past_the_largest_extent(geom, op, B):
    _lib, L = lib()
    tr, Cin, Cout, k, s, p, Lin = geom
    opc = {"fwd": (_lib.OP_CONV1D_FWD, _lib.OP_CONVT1D_FWD), "dgrad": (_lib.OP_CONV1D_DGRAD, _lib.OP_CONVT1D_DGRAD),
           "wgrad": (_lib.OP_CONV1D_WGRAD, _lib.OP_CONVT1D_WGRAD)}[op][tr]
    base = _args(_lib, B, Cin, Cout, Lin, k, s, p, tr)
    want = describe(base, opc)
    assert want[0] == 0, want
    for field, C_, L_ in gathered(op, Cin, Cout, Lin, base.Lout):
        a = _args(_lib, B, Cin, Cout, Lin, k, s, p, tr)
        if field in ("dx_add_bs", "dx_ref_bs"):
            a.dx_add = a.dx_ref = 4096
            a.dx_add_bs = a.dx_ref_bs = Cin * Lin
            a.dx_mask = 1
            want_f = describe(a, opc)
        else:
            want_f = want
        # the largest stride whose extent fits (B - 1 may not divide the room: then the extent stays a few words below the bound)
        bs = (WORDS_MAX - C_ * L_) // (B - 1)
        setattr(a, field, bs)
        assert describe(a, opc) == want_f, (field, bs)               # accepted, and the plan does not depend on the stride
        past = bs + 1 if B == 2 else (WORDS_MAX - C_ * L_) // (B - 1) + 1
        setattr(a, field, past)
        rc, msg = describe(a, opc)
        assert rc == _lib.ERR_SHAPE and msg.startswith(ADD_MSG if field.startswith("dx_") else ACT_MSG), (field, past, rc, msg)
        # ... and the launching entry point gives the same answer before it touches anything (no device here: it never gets that far)
        fn = getattr(L, {0: "pg_conv1d_fwd", 1: "pg_conv1d_dgrad", 2: "pg_conv1d_wgrad", 3: "pg_convt1d_fwd", 4: "pg_convt1d_dgrad", 5: "pg_convt1d_wgrad"}[opc])
        assert fn(ctypes.byref(a), None) == _lib.ERR_SHAPE
        if B == 2:                                                   # exactly at the bound: one word less than `past`
            assert ((B - 1) * bs + C_ * L_) * 4 == 0x7ffffff0 - 4
    if op == "dgrad":                                                # a mask source that dx_mask does not use is never read: any stride
        a = _args(_lib, B, Cin, Cout, Lin, k, s, p, tr)
        a.dx_ref, a.dx_ref_bs, a.dx_mask = 4096, 1 << 40, 0
        assert describe(a, opc)[0] == 0


def test_conv_weight_bound():
    """Cin * Cout * k * 4 >= 0x7ffffff0 is refused: 511 * 262657 * 4 floats is the first such product; 2044 floats less is accepted"""
    _lib, _ = lib()
    assert 511 * 262657 * 4 * 4 == 0x7ffffff0
    for op in (_lib.OP_CONV1D_FWD, _lib.OP_CONV1D_DGRAD, _lib.OP_CONV1D_WGRAD):
        assert describe(_args(_lib, 1, 511, 262656, 8, 4, 2, 1, False), op)[0] == 0
        rc, msg = describe(_args(_lib, 1, 511, 262657, 8, 4, 2, 1, False), op)
        assert rc == _lib.ERR_SHAPE and msg.startswith(b"conv: weight tensor exceeds 2 GiB"), (rc, msg)


@pytest.mark.parametrize("tr", [False, True])
def test_wgrad_frames_bound(tr):
    """wgrad: B * L of the P operand must stay below 2^24 - 64 (its slab loops divide by the float reciprocal)"""
    _lib, _ = lib()
    op = _lib.OP_CONVT1D_WGRAD if tr else _lib.OP_CONV1D_WGRAD
    top = (1 << 24) - 64
    for B, Lin, ok in ((1, top - 1, True), (1, top, False), (64, top // 64, False), (64, top // 64 - 1, True)):
        rc, msg = describe(_args(_lib, B, 2, 2, Lin, 1, 1, 0, tr), op)
        assert (rc == 0) == ok and (ok or (rc == _lib.ERR_UNSUPPORTED and msg.startswith(b"wgrad: B*L must stay below 2^24"))), (B, Lin, rc, msg)


def h_args(B, Cin, Cout, Lin, k, s, p, tr):
    from phasegen import ops
    _lib, _ = lib()
    a = _lib.ConvhArgs()
    a.B, a.Cin, a.Cout, a.Lin, a.k, a.stride, a.pad, a.transposed = B, Cin, Cout, Lin, k, s, p, int(tr)
    a.Lout = (Lin - 1) * s - 2 * p + k if tr else (Lin + 2 * p - k) // s + 1
    a.x_pitch = ops.h_pitch(Lin)
    a.x_bs = Cin * a.x_pitch
    a.x = a.w = a.y = 4096
    a.y_bs = Cout * a.Lout
    a.workspace, a.workspace_bytes = 4096, _lib.load().pg_workspace_bytes_conv()
    return a


@pytest.mark.parametrize("geom", [(False, 16, 16, 8, 1, 2, 13), (True, 32, 16, 8, 2, 1, 3)], ids=["C", "T"])
def test_conv_fwd_h_x_at_and_past_the_largest_extent(geom):
    """bf16 x: ((B - 1) x_bs + Cin x_pitch) * 2 < 0x7ffffff0, x_bs even"""
    _lib, L = lib()
    tr, Cin, Cout, k, s, p, Lin = geom
    buf = ctypes.create_string_buffer(1024)
    a = h_args(2, Cin, Cout, Lin, k, s, p, tr)
    assert L.pg_conv_fwd_h_describe(ctypes.byref(a), buf, 1024) == 0
    want = buf.value
    top = (0x7ffffff0 - 2) // 2 - Cin * a.x_pitch
    a.x_bs = top - top % 2
    assert L.pg_conv_fwd_h_describe(ctypes.byref(a), buf, 1024) == 0 and buf.value == want
    a.x_bs += 2
    assert L.pg_conv_fwd_h_describe(ctypes.byref(a), buf, 1024) == _lib.ERR_SHAPE
    assert L.pg_last_error_string().startswith(b"conv_fwd_h: activation tensor exceeds 2 GiB (31-bit buffer offsets)")
    assert L.pg_conv_fwd_h(ctypes.byref(a), None) == _lib.ERR_SHAPE
    for f in ("y_bs", "yh_bs", "yh2_bs"):                            # the outputs are stored at 64-bit offsets: no bound
        a = h_args(2, Cin, Cout, Lin, k, s, p, tr)
        a.yh = a.yh2 = 4096
        a.yh_pitch = a.yh2_pitch = a.Lout + a.Lout % 2 + 8
        setattr(a, f, (1 << 40) + 64)
        assert L.pg_conv_fwd_h_describe(ctypes.byref(a), buf, 1024) == 0 and buf.value == want, f


def test_index_width_bounds_of_bn_and_clipnorm_refused_side():
    """The REFUSED side of the bounds that keep 32-bit row counters in range, at their first refused products (2^31).  The accepted side
    is not pinned anywhere: these calls have no describe twin, so an accepted call launches, and B * L = 2^31 - 1 means an 8 GiB input
    beside an 8 GiB output.  An off-by-one that refused the legal product 2^31 - 1 would pass here."""
    _lib, L = lib()
    a = _lib.BnArgs()
    a.B, a.C, a.L = 1 << 16, 2, 1 << 15                              # B * L = 2^31
    a.x = a.y = a.gamma = a.beta = a.save_mean = a.save_invstd = a.dy = a.dx = a.dgamma = a.dbeta = 4096
    a.x_bs = a.y_bs = a.dy_bs = a.dx_bs = a.C * a.L
    for fn in (L.pg_bn_fwd, L.pg_bn_bwd):
        assert fn(ctypes.byref(a), None) == _lib.ERR_SHAPE and L.pg_last_error_string().startswith(b"bn: B*L too large")
    c = _lib.ClipNormArgs()
    c.B, c.C, c.L = 1 << 16, 1 << 15, 4                              # B * C = 2^31
    c.x = c.y = c.gamma = c.beta = 4096
    c.x_bs = c.y_bs = c.C * c.L
    assert L.pg_clipnorm_fwd(ctypes.byref(c), None) == _lib.ERR_SHAPE and L.pg_last_error_string().startswith(b"clipnorm: B*C too large")


def test_stft_crops_frame_count_bound():
    """n_signals * n_frames <= 2^31 - 1 (a prime: reached exactly by ONE crop of 2^31 - 1 frames); 32768 crops of 65536 frames are 2^31"""
    _lib, L = lib()
    buf = ctypes.create_string_buffer(512)
    for n_sig, n_samples, ok in ((1, 2**31 - 2, True), (32767, 65535, True), (32768, 65535, False)):
        a = _lib.StftCropsArgs()
        a.n_signals, a.n_samples, a.n_fft, a.hop, a.n_frames = n_sig, n_samples, 32, 1, 1 + n_samples
        a.src = a.crop_begin = a.crop_end = a.out = 4096
        rc = L.pg_stft_crops_describe(ctypes.byref(a), buf, 512)
        assert (rc == 0) == ok, (n_sig, n_samples, rc, L.pg_last_error_string())
        if not ok:
            assert rc == _lib.ERR_SHAPE and L.pg_last_error_string().startswith(b"stft_crops: n_signals * n_frames must fit in 31 bits")
            assert L.pg_stft_crops(ctypes.byref(a), None) == _lib.ERR_SHAPE


def test_far_conv_rows_plan_is_the_family_and_epilogue_their_id_names():
    """tests/test_z_far_offsets_gpu.py takes VIEW_CASES' geometries at B = 2: the plan of every row, as it runs there, still names the
    row's kernel family and epilogue, and the column-tail rows (kept at their own B) still have their tail launch"""
    from phasegen import ops
    from test_kernel_families import _epilogue, _opcode, _view_args, family
    from test_z_far_offsets_gpu import CONV_ROWS, CLASSES, fits
    _lib, _ = lib()
    assert len([r for r in CONV_ROWS if r[5] == "tail"]) == 6
    for row in CONV_ROWS:
        geom, op, sched, fam, epi, form = row
        d = ops.conv_describe(_view_args(_lib, row, None), _opcode(_lib, row))
        assert (family(d), _epilogue(d)) == (fam, epi), (row, d)
        assert ("|tail=conv_raw_kernel<" in d) == (form == "tail"), (row, d)
        assert fits(row, "A") and fits(row, "A'") and (geom[7] > 2 or all(fits(row, c) for c in CLASSES)), row
    for kind in ("F", "T", "Tpm"):                                    # every kind of tail runs far, in a class past 2^32 bytes
        assert any(r[5] == "tail" and r[4] == kind and fits(r, "B") for r in CONV_ROWS), kind


# ---- 3. the coverage gate ---------------------------------------------------------------------------------------------------------------------
CONV_SYMBOLS = ("pg_conv1d_fwd", "pg_conv1d_dgrad", "pg_conv1d_wgrad", "pg_convt1d_fwd", "pg_convt1d_dgrad", "pg_convt1d_wgrad")
CONV_READS = {"fwd": {"x_bs", "y_bs", "y2_bs"}, "dgrad": {"dy_bs", "dx_bs", "dx_add_bs", "dx_ref_bs"}, "wgrad": {"x_bs", "dy_bs"}}
EXCLUDED = {
    ("*", "workspace_bytes"): "a size, not an offset: tests/test_z_workspace_gpu.py holds every call to exactly the queried bytes",
    ("pg_bn_fwd", "dy_bs"): "pg_bn_args is shared: the forward does not read dy / dx",
    ("pg_bn_fwd", "dx_bs"): "pg_bn_args is shared: the forward does not read dy / dx",
    ("pg_bn_bwd", "y_bs"): "pg_bn_args is shared: the backward writes dx only",
    ("pg_bn_bwd", "y2_bs"): "pg_bn_args is shared: the backward writes dx only",
    ("pg_bn_bwd", "yh_bs"): "pg_bn_args is shared: the backward writes dx only",
    ("pg_bn_bwd", "yh2_bs"): "pg_bn_args is shared: the backward writes dx only",
    ("pg_resample", "n_in"): "rows longer than 2^31 samples (37 hours at 16 kHz in ONE row): tests/test_resample_gpu.py::test_indexing_beyond_2_to_the_31 covers the row index",
    ("pg_resample", "n_out"): "as n_in",
    ("pg_stitch", "n_out"): "a track of 2^31 samples has no realistic use; 64-bit by reading (DESIGN.md, Far offsets)",
    ("pg_spec_clips", "F_src"): "frame counts above 2^31 have no realistic use",
    ("pg_phase_vocoder", "F_src"): "frame counts above 2^31 have no realistic use",
    ("pg_phase_vocoder", "F_out"): "frame counts above 2^31 have no realistic use",
    ("pg_phase_lock", "F_src"): "frame counts above 2^31 have no realistic use",
    ("pg_phase_lock", "F_out"): "frame counts above 2^31 have no realistic use",
    ("pg_phase_lock_linked", "F_src"): "frame counts above 2^31 have no realistic use",
    ("pg_phase_lock_linked", "F_out"): "frame counts above 2^31 have no realistic use",
    ("pg_phase_spsi", "F"): "frame counts above 2^31 have no realistic use",
    ("pg_hpss", "F"): "frame counts above 2^31 have no realistic use",
    ("pg_ola_stretch", "n_in"): "one signal of 2^31 samples has no realistic use; 64-bit by reading (DESIGN.md, Far offsets)",
    ("pg_ola_stretch", "n_out"): "as n_in",
}


def int64_fields():
    """every (symbol, field) of a stream-taking entry point whose argument struct has a c_int64 field, and every direct c_int64 argument
    (as "arg<i>"), from the ctypes table of phasegen/_lib.py"""
    from _strict import stream_symbols
    _lib, _ = lib()
    out = []
    for name in stream_symbols():
        for i, t in enumerate(_lib.SYMBOLS[name][1]):
            struct = getattr(t, "_type_", None)
            if struct is not None and hasattr(struct, "_fields_"):
                out += [(name, f) for f, ft in struct._fields_ if ft is ctypes.c_int64]
            elif t is ctypes.c_int64:
                out.append((name, f"arg{i}"))
    return out


def test_every_64_bit_field_is_in_the_gpu_table_or_excluded_with_a_reason():
    from test_z_far_offsets_gpu import GPU_FIELDS
    fields = int64_fields()
    assert len(fields) > 100 and ("pg_stitch", "clip_stride") in fields and ("pg_fill", "arg1") in fields
    missing, stale = [], []
    for sym, f in fields:
        if sym in CONV_SYMBOLS and f.endswith("_bs") and f not in CONV_READS[sym.rsplit("_", 1)[1]]:
            continue                                                 # pg_conv_args is shared by the six ops: a field the op never reads
        if (sym, f) in GPU_FIELDS or (sym, f) in EXCLUDED or ("*", f) in EXCLUDED:
            continue
        missing.append((sym, f))
    assert not missing, missing
    for key in list(GPU_FIELDS) + [k for k in EXCLUDED if k[0] != "*"]:
        if key not in fields:
            stale.append(key)
    assert not stale, stale
    assert not set(GPU_FIELDS) & set(EXCLUDED)
    assert all(isinstance(r, str) and len(r) > 4 for r in EXCLUDED.values())
