"""GPU: every entry point of include/phasegen.h that takes a workspace, held to the workspace contract of the C ABI --

    the caller allocates everything and pg_workspace_bytes_* says how much; the contents are garbage between calls;
    nothing outside the given bytes is touched; a workspace that is too small is refused before any launch.

The wrappers of phasegen/ops.py hide a violation: their caches hand out a buffer that is at least as large as the request (and pass
its size), nothing stands behind it, and all but the conv workspace start as whatever torch.empty returns.  Here every row runs once
plainly (default stream, cached workspace: the value the other modules hold to float64) and then once per poison under
tests/_strict.py's allocator: a fresh view of EXACTLY the queried size between poisoned guards, itself poisoned.  The two results must
agree bit for bit -- a plan is a function of the shapes, never of the workspace -- and the guards must still hold the poison.

Poisons: 0xFF bytes (NaN as float / double, -1 as an integer: a SUM over a slot nobody wrote shows) and 0x7F bytes (3.39e38 /
1.4e306, finite: a MAXIMUM over such a slot shows, where fmaxf would drop a NaN).  pg_phase_lock's workspace holds gather indices, so
its rows use 0x00 and the stale contents of an earlier call on a larger plane instead: a mistake must show as wrong values, never as
wrong addresses.

Widest access each kernel makes to its workspace, by reading csrc/ (the documented-alignment cases rest on it):
    pg_stitch         StPartial {float peak; int32 bad}: two 4-byte stores / loads per slot (stitch.hip; the check demands 8)
    pg_moments        double partial[block]: 8 bytes (pointwise.hip; the check demands 8)
    pg_wave_compare   double partial[6 per chunk]: 8 bytes (compare.hip; the check demands 8)
    pg_spec_compare   double cellpart / tilepart / framepart, region offsets multiples of 8: 8 bytes (the check demands 8)
    pg_phase_lock     uint32 S / C / T words, one per bin: 4 bytes (lock.hip; the check demands 4)
No kernel makes a wider access than its check demands, so each runs one row with the view moved off its 256-byte alignment by exactly
that many bytes.  (The conv, loss, ISTFT and overlap-add workspaces hold floats read as 4-byte or, in the fixup, 16-byte units at
offsets that are multiples of 16; their header lines state no alignment below 16 and they are given 256-byte aligned views.)

The module is named to be collected behind the value modules: where both fail, theirs is the broader finding."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import unet_ref  # noqa: F401  (disables oneDNN: see the bug note in oracle/unet_ref.py)
from phasegen import detgen
from _strict import POISONS, same_bits, strict_view, strict_workspaces, workspace_symbols
from test_kernel_families import FIXUP_CASES, FIXUP_CASES_H, TAIL, VIEW_CASES, _fields, fixup_case_id
from test_ops_gpu import rnd

pytestmark = pytest.mark.gpu
SENT = -77.0
REACHED = set()              # library symbols called (return code 0) under the strict allocator by a case that passed


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def sent(*shape, dtype=torch.float32):
    return torch.full(shape, SENT, device=dev(), dtype=dtype)


def off4(t):
    """a dense copy of t that begins 4 bytes (one float) into its allocation: never 16-byte aligned"""
    flat = torch.empty(t.numel() + 1, device=dev(), dtype=t.dtype)
    v = flat[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


class Case:
    """One call of one wrapper.  ins: {name: device tensor} read by the call (float ones may be refilled by the stream module);
    make_outs() -> {name: device tensor} written by the call, pre-filled with a sentinel (or, for tensors updated in place, their
    initial state); run(ins, outs) -> list of tensors that are the call's result."""

    def __init__(self, id, ins, make_outs, run, poisons=POISONS, symbol=None, needs_ws=True, lock=False, fixed=()):
        self.id, self.ins, self.make_outs, self.run, self.poisons, self.symbol, self.needs_ws, self.lock = id, ins, make_outs, run, poisons, symbol, needs_ws, lock
        self.fixed = fixed           # names of inputs that hold their values from the start in the stream module (gains, statistics)

    def __repr__(self):
        return self.id


def check(case, **strict):
    """plain call == the call on an exact, poisoned, guarded workspace, bit for bit, for every poison of the case"""
    want = case.run(case.ins, case.make_outs())
    torch.cuda.synchronize()
    assert want
    reached = set()
    for poison in case.poisons:
        with strict_workspaces(poison, **strict) as s:
            got = case.run(case.ins, case.make_outs())
        assert not case.needs_ws or s.requests, "the call asked for no workspace"
        assert s.checked == len(s.requests)
        assert len(got) == len(want)
        for i, (g, w) in enumerate(zip(got, want)):
            assert same_bits(g, w), f"{case.id}: result {i} differs under poison {poison:#x} (exact workspace of {s.requests} bytes)"
        reached |= s.symbols()
    if case.symbol is not None:
        assert case.symbol in reached, (case.symbol, reached)
    REACHED.update(reached)


# ---- conv -------------------------------------------------------------------------------------------------------------------------------
def conv_lout(tr, k, s, p, Lin):
    return (Lin - 1) * s - 2 * p + k if tr else (Lin + 2 * p - k) // s + 1


def conv_case(row, adam=False, precision="fp32"):
    from phasegen import ops
    (tr, Cin, Cout, k, s, p, Lin, B), op, sched = row[:3]
    Lout = conv_lout(tr, k, s, p, Lin)
    wshape = (Cin, Cout, k) if tr else (Cout, Cin, k)
    ins = {"x": rnd(61, B, Cin, Lin).to(dev()), "w": (rnd(62, *wshape) * 0.1).to(dev()), "dy": rnd(63, B, Cout, Lout).to(dev())}
    kw = dict(transposed=tr, precision=precision, schedule=sched)
    sym = "pg_conv" + ("t" if tr else "") + "1d_" + op
    if op == "fwd":
        return Case(fixup_case_id(row), {"x": ins["x"], "w": ins["w"]}, lambda: {"y": sent(B, Cout, Lout)},
                    lambda i, o: [ops.conv_fwd(i["x"], i["w"], o["y"], s, p, **kw)], symbol=sym)
    if op == "dgrad":
        return Case(fixup_case_id(row), {"dy": ins["dy"], "w": ins["w"]}, lambda: {"dx": sent(B, Cin, Lin)},
                    lambda i, o: [ops.conv_dgrad(i["dy"], i["w"], o["dx"], s, p, **kw)], symbol=sym)
    if not adam:
        return Case(fixup_case_id(row), {"x": ins["x"], "dy": ins["dy"]}, lambda: {"dw": sent(*wshape)},
                    lambda i, o: [ops.conv_wgrad(i["x"], i["dy"], o["dw"], s, p, x_act=ops.ACT_LEAKY, **kw)], symbol=sym)
    m0, v0 = rnd(66, *wshape).to(dev()) * 0.01, rnd(67, *wshape).to(dev()).abs() * 1e-4

    def run(i, o):
        ad = ops.adam_args(o["p"], o["m"], o["v"], 3)
        ops.conv_wgrad(i["x"], i["dy"], o["dw"], s, p, adam=ad, **kw)
        return [o["dw"], o["p"], o["m"], o["v"]]

    return Case(fixup_case_id(row) + "-adam", {"x": ins["x"], "dy": ins["dy"]},
                lambda: {"dw": sent(*wshape), "p": ins["w"].clone(), "m": m0.clone(), "v": v0.clone()}, run, symbol=sym)


CONV_ROWS = FIXUP_CASES + [c for c in VIEW_CASES if c[5] == "tail"]
# the packed fp32 wgrads of VIEW_CASES: flat K (k = 32), per-sample slabs (k = 8) and k = 5's 255-column tiles, each under one tile per
# workgroup and under the forced stream-K split
PACKED_GEOMS = ((False, 40, 48, 32, 2, 16, 258, 2), (False, 33, 40, 8, 1, 2, 129, 3), (True, 64, 103, 5, 2, 1, 30, 2))
PACKED_WGRADS = [c for c in VIEW_CASES if c[1] == "wgrad" and c[0] in PACKED_GEOMS]


@pytest.mark.parametrize("row", CONV_ROWS, ids=fixup_case_id)
def test_conv_fixup_and_tail_rows(row):
    """main launch, fixup, tail launch and tail fixup share one buffer of pg_workspace_bytes_conv() bytes (a wgrad: of
    pg_workspace_bytes_wgrad() bytes, which the wrapper asks for through at_least=)"""
    if row[5] == "tail":
        assert row[2] == TAIL
    check(conv_case(row))


@pytest.mark.parametrize("adam", [False, True], ids=["plain", "adam"])
@pytest.mark.parametrize("row", PACKED_WGRADS, ids=fixup_case_id)
def test_packed_wgrads(row, adam):
    """flat K and per-sample slabs, one tile per workgroup and forced stream-K: the packed operands lie behind the stream-K region, and
    the view ends with them"""
    from phasegen import _lib, ops
    assert len(PACKED_WGRADS) == 6
    case = conv_case(row, adam=adam)
    check(case)
    (tr, Cin, Cout, k, s, p, Lin, B) = row[0]
    a = ops._conv_args(tr, B, Cin, Cout, Lin, k, s, p, None, "fp32", row[2])
    need = _lib.load().pg_workspace_bytes_wgrad(ctypes.byref(a), _lib.OP_CONVT1D_WGRAD if tr else _lib.OP_CONV1D_WGRAD)
    assert need > _lib.load().pg_workspace_bytes_conv()
    with strict_workspaces(0xFF) as st:
        case.run(case.ins, case.make_outs())
    assert st.requests[-1] == need, (st.requests, need)           # the call ran on exactly the queried bytes


def convh_case(geom, sched):
    from phasegen import ops
    tr, Cin, Cout, k, s, p, Lin, B = geom
    Lout = conv_lout(tr, k, s, p, Lin)
    w = (rnd(52, *((Cin, Cout, k) if tr else (Cout, Cin, k))) * 0.1).to(dev())
    xh = ops.h_alloc(B, Cin, Lin, dev())
    ops.cast_rows_bf16(rnd(51, B, Cin, Lin).to(dev()), xh)
    wh = ops.shadow_weights(w, tr, s)

    def run(i, o):
        ops.conv_fwd_h(i["xh"], Lin, i["wh"], tuple(w.shape), s, p, transposed=tr, y=o["y"], yh=o["yh"], yh_act=ops.ACT_LEAKY, yh2=o["yh2"],
                       yh2_act=ops.ACT_RELU, schedule=sched)
        return [o["y"], o["yh"], o["yh2"]]

    return Case(f"h-{'T' if tr else 'C'}{Cin}-{Cout}-k{k}s{s}-sched{sched}", {"xh": xh, "wh": wh},
                lambda: {"y": sent(B, Cout, Lout), "yh": ops.h_alloc(B, Cout, Lout, dev()), "yh2": ops.h_alloc(B, Cout, Lout, dev())}, run,
                symbol="pg_conv_fwd_h")


@pytest.mark.parametrize("sched", [1, 2])
@pytest.mark.parametrize("row", FIXUP_CASES_H, ids=lambda c: f"{'T' if c[0][0] else 'C'}{c[0][1]}-{c[0][2]}-k{c[0][3]}s{c[0][4]}-{c[1]}-{c[2]}")
def test_conv_fwd_h(row, sched):
    check(convh_case(row[0], sched))


def _short_scratch_rows():
    """forward rows of FIXUP_CASES whose forced stream-K split does not fit 1 MiB of scratch (two of the ten do fit: their grids are 2
    and 4 workgroups)"""
    from phasegen import _lib, ops
    from test_kernel_families import _args
    rows = []
    for row in FIXUP_CASES:
        (tr, Cin, Cout, k, s, p, Lin, B), op, sched = row[:3]
        if op != "fwd":
            continue
        a = _args(_lib, B, Cin, Cout, Lin, k, s, p, tr, schedule=sched)
        opc = _lib.OP_CONVT1D_FWD if tr else _lib.OP_CONV1D_FWD
        assert _fields(ops.conv_describe(a, opc))["split"] == "1"
        a.workspace_bytes = 1 << 20
        if _fields(ops.conv_describe(a, opc))["split"] == "0":
            rows.append(row)
    return rows


@pytest.mark.parametrize("scratch", ["1MiB", "null", "zero-bytes"])
def test_conv_with_too_little_scratch(scratch):
    """A conv is never refused for its workspace (only the packed wgrad is): with less than its split needs -- or none -- it runs one
    tile per workgroup, says so in pg_conv_describe, gives the bits of PG_SCHED_TILE_PER_WG and touches nothing beyond the bytes given."""
    from phasegen import _lib, ops
    lib = _lib.load()
    rows = _short_scratch_rows()
    assert len(rows) >= 2
    for row in (rows[0], rows[-1]):
        (tr, Cin, Cout, k, s, p, Lin, B), op, sched = row[:3]
        case = conv_case(row)
        want = ops.conv_fwd(case.ins["x"], case.ins["w"], sent(B, Cout, conv_lout(tr, k, s, p, Lin)), s, p, transposed=tr, precision="fp32",
                            schedule=(sched & ~3) | 1)
        for poison in POISONS:
            a = ops._conv_args(tr, B, Cin, Cout, Lin, k, s, p, None, "fp32", sched)
            y = sent(*want.shape)
            a.x, a.x_bs = ops._act3(case.ins["x"], "x")
            a.y, a.y_bs = ops._act3(y, "y")
            a.w = case.ins["w"].data_ptr()
            guard, view = strict_view(poison, 1 << 20)
            if scratch == "1MiB":
                a.workspace, a.workspace_bytes = view.data_ptr(), view.numel()
            elif scratch == "zero-bytes":
                a.workspace, a.workspace_bytes = view.data_ptr(), 0
            opc = _lib.OP_CONVT1D_FWD if tr else _lib.OP_CONV1D_FWD
            assert _fields(ops.conv_describe(a, opc))["split"] == "0"
            fn = lib.pg_convt1d_fwd if tr else lib.pg_conv1d_fwd
            assert fn(ctypes.byref(a), ops._stream()) == 0
            guard.check()
            assert same_bits(y, want), (row, scratch, poison)
            if scratch != "1MiB":                            # nothing was given: nothing of the view changes either
                assert bool((guard.contents[0] == poison).all())


# ---- loss, moments, clipnorm -----------------------------------------------------------------------------------------------------------------
def loss_case(B, Cc, L):
    from phasegen import ops
    ins = {"pred": cuda(detgen.normal(31, (B, 2 * Cc, L))), "batch": cuda(detgen.normal(32, (B, 2, Cc, L)))}
    return Case(f"loss-{B}x{Cc}x{L}", ins, lambda: {"dpred": sent(B, 2 * Cc, L), "losses": sent(3)},
                lambda i, o: [ops.loss_fwd_bwd(i["pred"], i["batch"], dpred=o["dpred"], losses=o["losses"]), o["dpred"]], symbol="pg_loss_fwd_bwd")


@pytest.mark.parametrize("shape", [(1, 8, 24), (5, 33, 77), (5, 33, 1700)])
def test_loss(shape):
    """one workgroup; several; B C L > 262 144: the grid is capped at 1024 workgroups and every one of the 1024 partial slots is live"""
    check(loss_case(*shape))


def moments_case(n, misaligned):
    from phasegen import ops
    x = cuda(detgen.normal(33, (n,)) * np.float32(3.0) + np.float32(0.5))
    if misaligned:
        x = off4(x)
    x0 = x.clone()               # (the stream module overwrites the inputs of a case for a while: the in-place tensor starts from its own copy)
    return Case(f"moments-{n}-{'off4' if misaligned else 'al16'}", {"x": x},
                lambda: {"x": off4(x0) if misaligned else x0.clone(), "stats": sent(2, dtype=torch.float64)},
                lambda i, o: [ops.moments(i["x"], o["stats"]).clone(), ops.standardize_(o["x"]), o["x"]], symbol="pg_moments")


@pytest.mark.parametrize("misaligned", [False, True], ids=["al16", "off4"])
@pytest.mark.parametrize("n", [5, 1023, 1048577 + 3])
def test_moments_and_standardize(n, misaligned):
    check(moments_case(n, misaligned))


def clipnorm_case(B, Cc, L, poison=None, offset=0):
    """the wrapper's workspace= takes the strict view directly: `poison` None = the plain call (the wrapper's own torch.empty)"""
    from phasegen import ops
    ins = {"x": cuda(detgen.normal(34, (B, Cc, L))), "gamma": cuda(detgen.uniform(35, (Cc,), 0.5, 1.5)), "beta": cuda(detgen.normal(36, (Cc,)))}
    rm0, rv0 = cuda(detgen.normal(37, (Cc,))), cuda(detgen.uniform(38, (Cc,), 0.5, 2.0))

    def run(i, o):
        ops.clipnorm_fwd(i["x"], o["y"], i["gamma"], i["beta"], running_mean=o["rm"], running_var=o["rv"], num_batches_tracked=o["nbt"],
                         workspace=o.get("ws"))
        return [o["y"], o["rm"], o["rv"], o["nbt"]]

    def make_outs():
        o = {"y": sent(B, Cc, L), "rm": rm0.clone(), "rv": rv0.clone(), "nbt": torch.full((), 7, dtype=torch.int64, device=dev())}
        if poison is not None:
            o["guard"], view = strict_view(poison, 8 * B * Cc, offset)
            o["ws"] = view.view(torch.float32)
        return o

    return Case(f"clipnorm-{B}x{Cc}x{L}", ins, make_outs, run, symbol="pg_clipnorm_fwd", needs_ws=False)


@pytest.mark.parametrize("shape", [(1, 8, 24), (5, 33, 77), (64, 40, 129)])
def test_clipnorm_with_running_buffers(shape):
    from phasegen import _lib
    a = _lib.ClipNormArgs()
    a.B, a.C, a.L = shape
    assert _lib.load().pg_workspace_bytes_clipnorm(ctypes.byref(a)) == 8 * shape[0] * shape[1]
    plain = clipnorm_case(*shape)
    want = plain.run(plain.ins, plain.make_outs())
    for poison in POISONS:
        case = clipnorm_case(*shape, poison=poison)
        outs = case.make_outs()
        with strict_workspaces(poison) as s:                  # (records the library call; the wrapper asks no cache)
            got = case.run(case.ins, outs)
        outs["guard"].check()
        assert not s.requests and all(same_bits(g, w) for g, w in zip(got, want)), (shape, poison)
        REACHED.update(s.symbols())


# ---- istft, overlap-add, Griffin-Lim ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _istft_inputs(bins, hop, frames, signals, mode):
    """white spectra (tests/test_z_signal_values_gpu.py: inverse_input), on the device, shared by the cases of one shape"""
    shape = (signals, bins, frames)
    if mode == 1:
        return cuda(detgen.normal(810 + bins % 13, shape)), cuda(detgen.normal(811 + hop % 17, shape))
    return cuda(np.abs(detgen.normal(812, shape))), cuda(detgen.uniform(813, shape, -3.1415, 3.1415))


def istft_case(bins, hop, frames, signals, mode, normalize, misaligned, id=None):
    from phasegen import ops
    a, b = _istft_inputs(bins, hop, frames, signals, mode)
    length = hop * (frames - 1)

    def make_outs():
        out = sent(signals, length)
        return {"audio": off4(out) if misaligned else out}

    return Case(id or f"istft-{bins}-{hop}-{frames}-{signals}-m{mode}-n{int(normalize)}-{'off4' if misaligned else 'al16'}", {"a": a, "b": b},
                make_outs, lambda i, o: [ops.istft(i["a"], i["b"], hop, mode=mode, normalize=normalize, out=o["audio"])], symbol="pg_istft")


def _inverse_cases():
    from test_z_signal_values_gpu import INVERSE_CASES
    return INVERSE_CASES


@pytest.mark.parametrize("case", _inverse_cases(), ids=[c.id for c in _inverse_cases()])
def test_istft(case):
    """modes 0 and 1, normalize on and off, `out` 16-byte aligned (the fused path where the shape allows) and 4 bytes off (always the
    three-kernel path): ONE query serves both paths, and the peak fold reads part_per slots per signal of a region sized for the larger
    of the two counts"""
    for mode in (0, 1):
        for normalize in (False, True):
            for misaligned in (False, True):
                check(istft_case(case.bins, case.hop, case.frames, case.signals, mode, normalize, misaligned))


def test_istft_of_70_signals_is_two_calls_with_two_needs():
    case = istft_case(512, 256, 9, 70, 1, True, False)
    check(case)
    with strict_workspaces(0x7F) as s:
        case.run(case.ins, case.make_outs())
    assert len(s.requests) == 2 and s.requests[0] > s.requests[1] > 0, s.requests        # 64 signals, then 6


def ola_case(clips, normalize, n_fft=2046, hop=512, frames=9):
    from phasegen import ops
    lead = (clips,) if clips else ()
    fr = cuda(detgen.normal(361, lead + (n_fft, frames)))
    return Case(f"ola-{n_fft}-{clips}-n{int(normalize)}", {"fr": fr}, lambda: {"audio": sent(*lead, hop * (frames - 1))},
                lambda i, o: [ops.ola_nt(i["fr"], hop, o["audio"], normalize=normalize)], symbol="pg_ola_nt")


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("clips", [0, 3], ids=["one-clip", "three-clips"])
def test_ola_nt(clips, normalize):
    """the 256 bytes hold one peak word per clip, zeroed by a memset on the call's stream: under 0x7F an unzeroed word would win the
    integer maximum"""
    check(ola_case(clips, normalize))


def test_griffin_lim_batch():
    from phasegen import audio as pg_audio
    mag = cuda(np.abs(detgen.normal(81, (3, 16, 24))) + np.float32(0.1))

    def run(i, o):
        res = pg_audio.griffin_lim_batch(i["mag"], 32, 8, 2, seed=9)
        return [t for t in res if torch.is_tensor(t)]

    check(Case("griffin-lim-2-iterations", {"mag": mag}, dict, run))


# ---- stitch --------------------------------------------------------------------------------------------------------------------------------------
def stitch_case(shape, normalize, status, misaligned=False):
    from phasegen import ops
    from test_stitch_gpu import make_clips, n_out_of
    n_tracks, n_clips, T, V, cut = shape
    clips = cuda(make_clips(shape))
    if misaligned:
        clips = off4(clips)
    n_out = n_out_of(shape)

    def run(i, o):
        res = ops.stitch(i["clips"], T - V, n_out, normalize=normalize, out=o["out"], return_status=status)
        return list(res) if status else [res]

    return Case(f"stitch-{shape}-n{int(normalize)}-s{int(status)}", {"clips": clips}, lambda: {"out": sent(n_tracks, n_out)}, run, symbol="pg_stitch")


def _stitch_shapes():
    from test_stitch_gpu import SHAPES
    return SHAPES


@pytest.mark.parametrize("shape", _stitch_shapes())
def test_stitch(shape):
    """one workgroup up to the 40-clip case (nparts > 256: the finish kernel's strided fold); 16-byte and scalar accesses"""
    for normalize, status in ((True, True), (False, True), (True, False)):
        check(stitch_case(shape, normalize, status))
    check(stitch_case(shape, True, True, misaligned=True))


# ---- phase lock --------------------------------------------------------------------------------------------------------------------------------
def lock_case(F_out, bins, n_ch=2, spo=1 / 1.5):
    from phasegen import ops
    from test_z_lock_gpu import f_src_for, planes
    A, M = planes(3000 + F_out + bins, n_ch, bins, f_src_for(F_out, spo))
    return Case(f"lock-F{F_out}-b{bins}", {"A": cuda(A), "M": cuda(M)}, lambda: {"out": sent(n_ch, bins, F_out)},
                lambda i, o: [ops.phase_lock(i["A"], F_out, spo, logmag=i["M"], reset_below=0.5, out=o["out"])], poisons=(0x00,), symbol="pg_phase_lock",
                lock=True)


def lock_stale(F_out, bins, n_ch=2):
    """the workspace a call on a larger plane (more bins, more chunks) leaves behind: valid S, C and T of ANOTHER problem"""
    big = lock_case(F_out + 70, min(2 * bins + 3, 4096), n_ch)
    with strict_workspaces(0x00, keep=True) as s:
        big.run(big.ins, big.make_outs())
    (stale,) = s.contents
    assert bool((stale != 0).any())
    return stale


@pytest.mark.parametrize("bins", [1, 5, 64, 1025])
@pytest.mark.parametrize("F_out", [1, 32, 33, 65])
def test_phase_lock(F_out, bins):
    """chunk boundaries (32 frames) x widths (one bin, a few, a full wave, two bins per thread and an odd last word)"""
    n_ch = 1 if bins == 1025 else 2
    case = lock_case(F_out, bins, n_ch)
    check(case)
    stale = lock_stale(F_out, bins, n_ch)
    want = case.run(case.ins, case.make_outs())
    with strict_workspaces(0x00, stale=stale) as s:
        got = case.run(case.ins, case.make_outs())
    assert s.requests == [12 * n_ch * bins * ((F_out + 31) // 32)] and stale.numel() > s.requests[0]
    assert same_bits(got[0], want[0]), (F_out, bins, "stale workspace")


# ---- compare ----------------------------------------------------------------------------------------------------------------------------------------
def wave_case(n_sig, n):
    from phasegen import ops
    x = detgen.normal(41, (n_sig, n))
    y = (np.float32(0.8) * x + np.float32(0.05) * detgen.normal(42, (n_sig, n))).astype(np.float32)
    gain = torch.linspace(0.9, 1.3, n_sig, dtype=torch.float64, device=dev())
    return Case(f"wave-{n_sig}x{n}", {"x": cuda(x), "y": cuda(y), "gain": gain}, lambda: {"out": sent(n_sig, 6, dtype=torch.float64)},
                lambda i, o: [ops.wave_compare(i["x"], i["y"], gain=i["gain"], out=o["out"])], symbol="pg_wave_compare", fixed=("gain",))


@pytest.mark.parametrize("n_sig", [1, 3])
@pytest.mark.parametrize("n", [1, 8191, 8192, 8193, 3 * 8192 + 5])
def test_wave_compare(n, n_sig):
    """the chunk fold: slot 4 is a maximum (0x7F), the others sums (0xFF)"""
    check(wave_case(n_sig, n))


def spec_case(n_sig, bins, frames):
    from phasegen import ops
    R = detgen.normal(43, (n_sig, 2, bins, frames))
    E = (np.float32(0.9) * R + np.float32(0.1) * detgen.normal(44, (n_sig, 2, bins, frames))).astype(np.float32)
    return Case(f"spec-{n_sig}x{bins}x{frames}", {"R": cuda(R), "E": cuda(E)}, lambda: {"out": sent(n_sig, 6, dtype=torch.float64)},
                lambda i, o: [ops.spec_compare(i["R"], i["E"], gain=1.1, out=o["out"])], symbol="pg_spec_compare")


@pytest.mark.parametrize("n_sig", [1, 2])
@pytest.mark.parametrize("bins,frames", [(1, 1), (64, 256), (65, 257), (130, 515)])
def test_spec_compare(bins, frames, n_sig):
    """the cell, tile and frame regions: one workgroup; exactly one tile and one bin block; one more of each; several"""
    check(spec_case(n_sig, bins, frames))


# ---- compositions: successive different ops share _compare_ws and _conv_ws ----------------------------------------------------------------------
def _small_model():
    from phasegen.model import UNetModel
    return UNetModel(16, 32, gpu_ids=[0]).load_numpy(detgen.make_params(16, seed=0))


def test_compare_audio_whole():
    from phasegen import metrics
    from test_track_metrics_gpu import make_signal
    x = make_signal(1000, 2)
    y = (0.8 * x + 0.05 * detgen.normal(72, x.shape)).astype(np.float32)
    want = metrics.compare_audio(x, y, 32, 8)
    for poison in POISONS:
        with strict_workspaces(poison) as s:
            got = metrics.compare_audio(x, y, 32, 8)
        assert got == want and len(s.requests) >= 4, (poison, s.requests)
        assert {"pg_wave_compare", "pg_spec_compare", "pg_stft"} <= s.symbols()


def test_reconstruct_track_whole():
    from phasegen import track
    from test_track_metrics_gpu import SMALL, STATS, make_signal
    a = make_signal(1000, 2)
    want = track.reconstruct_track(_small_model(), a, stats=STATS, join="waveform", **SMALL)
    for poison in POISONS:
        with strict_workspaces(poison) as s:
            got = track.reconstruct_track(_small_model(), a, stats=STATS, join="waveform", **SMALL)
        assert same_bits(got, want), poison
        assert {"pg_istft", "pg_stitch"} <= s.symbols() and s.requests
        REACHED.update(s.symbols())


def test_trainer_step_whole():
    """one eager training step at C = 16, L = 64, B = 3: every conv forward, dgrad and wgrad, the loss and the optimiser on exact scratch"""
    from phasegen.trainer import Trainer
    batch = cuda(detgen.make_batch(3, 16, 64, seed=1))

    def step():
        model = _small_model()
        trainer = Trainer(model, lr=1e-3)
        losses = trainer.step(batch)
        torch.cuda.synchronize()
        arena = model.engine.arena
        return [losses.clone()] + [arena.p(k).clone() for k in detgen.param_order()] + [arena.g(k).clone() for k in detgen.param_order()]

    want = step()
    for poison in POISONS:
        with strict_workspaces(poison) as s:
            got = step()
        assert len(s.requests) >= 3 and all(same_bits(g, w) for g, w in zip(got, want)), (poison, len(s.requests))
        REACHED.update(s.symbols())


# ---- refusal leaves no trace -----------------------------------------------------------------------------------------------------------------------
def _one_byte_short(a):
    assert a.workspace and a.workspace_bytes > 0
    a.workspace_bytes -= 1


REFUSALS = {
    "wgrad": lambda: conv_case(PACKED_WGRADS[2]),
    "loss": lambda: loss_case(1, 8, 24),
    "moments": lambda: moments_case(5, False),
    "istft": lambda: istft_case(16, 8, 5, 1, 1, True, False),
    "ola_nt": lambda: ola_case(0, True),
    "stitch": lambda: stitch_case(_stitch_shapes()[0], True, True),
    "phase_lock": lambda: lock_case(1, 1),
    "wave_compare": lambda: wave_case(1, 1),
    "spec_compare": lambda: spec_case(1, 1, 1),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_refusal_leaves_no_trace(name):
    """workspace_bytes = need - 1: PG_ERR_WORKSPACE, and after a synchronise every output still holds its sentinel (a tensor updated
    in place: its initial state) and the workspace its poison -- refused means nothing was launched, no memset either"""
    from phasegen import _lib
    case = REFUSALS[name]()
    poison = 0x00 if case.lock else 0xFF
    outs, fresh = case.make_outs(), case.make_outs()
    with strict_workspaces(poison, keep=True, tamper={case.symbol: _one_byte_short}) as s:
        with pytest.raises(RuntimeError):
            case.run(case.ins, outs)
    assert [(n, rc) for n, _, rc in s.calls] == [(case.symbol, _lib.ERR_WORKSPACE)], s.calls
    assert s.contents and all(bool((c == poison).all()) for c in s.contents)
    for k in outs:
        assert same_bits(outs[k], fresh[k]), (name, k)


def test_clipnorm_refusal_leaves_no_trace():
    from phasegen import _lib
    case = clipnorm_case(1, 8, 24, poison=0xFF)
    outs, fresh = case.make_outs(), case.make_outs()
    with strict_workspaces(0xFF, tamper={"pg_clipnorm_fwd": _one_byte_short}) as s:
        with pytest.raises(RuntimeError):
            case.run(case.ins, outs)
    assert [(n, rc) for n, _, rc in s.calls] == [("pg_clipnorm_fwd", _lib.ERR_WORKSPACE)], s.calls
    outs["guard"].check()
    assert bool((outs["guard"].contents[0] == 0xFF).all())
    for k in ("y", "rm", "rv", "nbt"):
        assert same_bits(outs[k], fresh[k]), k


# ---- documented alignment --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,offset", [("stitch", 8), ("moments", 8), ("wave_compare", 8), ("spec_compare", 8), ("phase_lock", 4)])
def test_documented_workspace_alignment(name, offset):
    """the view moved off its 256-byte alignment by exactly the alignment the call's check demands (module docstring: no kernel makes a
    wider access to its workspace): same bits"""
    case = {"stitch": lambda: stitch_case(_stitch_shapes()[1], True, True), "moments": lambda: moments_case(1023, False),
            "wave_compare": lambda: wave_case(3, 8193), "spec_compare": lambda: spec_case(2, 65, 257), "phase_lock": lambda: lock_case(33, 5)}[name]()
    check(case, offset=offset)


# ---- the list is complete ----------------------------------------------------------------------------------------------------------------------------
def test_zz_every_workspace_entry_point_was_reached_by_a_passing_case():
    """every entry point of include/phasegen.h whose argument struct has a workspace ran under the strict allocator in a case that
    passed (a deselected or failed case leaves its symbol out: run the module whole)"""
    missing = sorted(set(workspace_symbols()) - REACHED)
    assert not missing, missing
