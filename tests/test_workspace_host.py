"""CPU: the workspace queries of include/phasegen.h.  Every pg_workspace_bytes_* is a host function of the fields its header comment
names -- never of pointers, strides or alignment -- has the closed form pinned below, and answers the call's own negative error code
for arguments the call refuses.  The device side of the same contract (a call given exactly that many bytes, with anything in them,
writes nothing outside them) is tests/test_z_workspace_gpu.py."""
import ctypes

import pytest

ALIGNED, ODD = 4096, 4100          # pointers are never dereferenced: a query launches nothing
MIB = 1 << 20


def lib():
    from phasegen import _lib
    return _lib, _lib.load()


def ceil_div(a, b):
    return -(-a // b)


def vary(a, fields, answer, what):
    """the query's answer does not move when the pointer and stride fields in `fields` (name -> values) change, one at a time"""
    base = answer(a)
    assert base > 0, (what, base)
    for name, values in fields.items():
        old = getattr(a, name)
        for v in values:
            setattr(a, name, v)
            assert answer(a) == base, (what, name, v)
        setattr(a, name, old)
    return base


POINTERS = (None, ALIGNED, ODD, ODD + 1)
STRIDES = (0, 1, 12345, 1 << 40)


# ---- istft ------------------------------------------------------------------------------------------------------------------------
def istft_args(signals, bins, frames, hop, single=0, normalize=1, mode=1):
    _lib, _ = lib()
    a = _lib.IstftArgs()
    a.n_signals, a.bins, a.n_frames, a.hop, a.mode, a.normalize, a.single_frame = signals, bins, frames, hop, mode, normalize, single
    return a


@pytest.mark.parametrize("signals,bins,frames,hop", [(1, 16, 5, 8), (3, 64, 8, 50), (64, 16, 33, 8), (2, 512, 9, 256), (2, 512, 7, 512),
                                                      (64, 1024, 72, 512), (2, 1024, 9, 1024), (2, 2048, 3, 1024), (6, 1024, 16, 512)])
def test_istft_query_is_a_function_of_the_sizes_alone(signals, bins, frames, hop):
    _lib, L = lib()
    a = istft_args(signals, bins, frames, hop)
    q = lambda a: L.pg_workspace_bytes_istft(ctypes.byref(a))
    # no pointer at all: the query must not require them; `audio` decides the PATH of a call (fused needs 16-byte alignment), not the size
    got = vary(a, {"a": POINTERS, "b": POINTERS, "audio": POINTERS, "workspace": POINTERS, "a_bs": STRIDES, "b_bs": STRIDES,
                   "workspace_bytes": (0, 1, 1 << 40), "mode": (0, 1), "normalize": (0, 1), "single_frame": (0, 1)}, q, "istft")
    n_fft, length, groups = 2 * bins, hop * (frames - 1), ceil_div(frames, 8)
    per = max(ceil_div(length, 1024), 2 * groups)          # peak partials per signal: the overlap-add's blocks or two per group of 8 frames
    assert got == 256 + ceil_div(signals * per * 4, 256) * 256 + signals * frames * n_fft * 4


def test_istft_query_refuses_what_the_call_refuses():
    """The query used to answer 0 for NULL and a size computed from shapes the call refuses; now both go through the same checks."""
    _lib, L = lib()
    assert L.pg_workspace_bytes_istft(None) == _lib.ERR_NULL
    buf = ctypes.create_string_buffer(256)
    for (signals, bins, frames, hop), code in {(2, 24, 5, 8): _lib.ERR_UNSUPPORTED,          # 2 * bins = 48: no power of two
                                               (2, 8, 5, 4): _lib.ERR_UNSUPPORTED,           # n_fft 16 < 32
                                               (2, 4096, 5, 512): _lib.ERR_UNSUPPORTED,      # n_fft 8192 > 4096
                                               (2, 16, 1, 8): _lib.ERR_SHAPE,                # n_frames < 2
                                               (65, 16, 5, 8): _lib.ERR_SHAPE,               # more than 64 signals
                                               (0, 16, 5, 8): _lib.ERR_SHAPE,
                                               (2, 16, 5, 33): _lib.ERR_SHAPE,               # hop > n_fft
                                               (2, 16, 5, 0): _lib.ERR_SHAPE}.items():
        a = istft_args(signals, bins, frames, hop)
        assert L.pg_workspace_bytes_istft(ctypes.byref(a)) == code, (signals, bins, frames, hop)
        # ... and the call (here: its launch-free twin, which makes the call's checks) gives the same code once the pointers are there
        a.a = a.b = a.audio = a.workspace = ALIGNED
        a.a_bs = a.b_bs = bins * frames
        a.workspace_bytes = 1 << 40
        assert L.pg_istft_describe(ctypes.byref(a), buf, 256) == code, (signals, bins, frames, hop)
        assert L.pg_istft(ctypes.byref(a), None) == code, (signals, bins, frames, hop)        # refused before any launch: no device needed
    a = istft_args(2, 16, 5, 32)                                                               # hop == n_fft is allowed
    assert L.pg_workspace_bytes_istft(ctypes.byref(a)) > 0


def test_ops_workspace_raises_on_a_negative_answer():
    from phasegen import ops
    _lib, L = lib()
    a = istft_args(65, 16, 5, 8)
    with pytest.raises(RuntimeError, match="workspace_bytes_istft"):
        ops._workspace(ops._istft_ws, "cpu", L.pg_workspace_bytes_istft(ctypes.byref(a)), "workspace_bytes_istft")


# ---- the constant queries ------------------------------------------------------------------------------------------------------------
def test_constant_queries():
    _lib, L = lib()
    assert L.pg_workspace_bytes_conv() == 512 * MIB
    assert L.pg_workspace_bytes_moments() == 1024 * 8
    a = _lib.LossArgs()
    for B, Cc, Ln in ((1, 8, 24), (5, 33, 77), (64, 1024, 256)):
        a.B, a.C, a.L = B, Cc, Ln
        assert vary(a, {"pred": POINTERS, "batch": POINTERS, "dpred": POINTERS, "losses": POINTERS, "workspace": POINTERS,
                        "workspace_bytes": (0, 1 << 40)}, lambda a: L.pg_workspace_bytes_loss(ctypes.byref(a)), "loss") == 1024 * 3 * 4


def test_ola_needs_256_bytes():
    """pg_ola_nt has no query; its header line says 256 bytes.  One byte less is refused before any launch (no device needed)."""
    _lib, L = lib()
    a = _lib.OlaArgs()
    a.n_fft, a.frames, a.hop, a.n = 30, 9, 7, 2
    a.fr = a.audio = a.workspace = ALIGNED
    a.workspace_bytes = 255
    assert L.pg_ola_nt(ctypes.byref(a), None) == _lib.ERR_WORKSPACE


# ---- stitch ----------------------------------------------------------------------------------------------------------------------------
def stitch_args(n_tracks=2, n_clips=4, T=184, step=92, n_out=None):
    _lib, _ = lib()
    a = _lib.StitchArgs()
    a.n_tracks, a.n_clips, a.clip_len, a.step = n_tracks, n_clips, T, step
    a.n_out = (n_clips - 1) * step + T if n_out is None else n_out
    return a


def test_stitch_query():
    _lib, L = lib()
    q = lambda a: L.pg_workspace_bytes_stitch(ctypes.byref(a))
    for shape in ((1, 1, 184, 120), (2, 4, 184, 92), (2, 40, 4096, 3072), (1, 9, 23, 12)):
        a = stitch_args(*shape)
        assert vary(a, {"clips": POINTERS, "out": POINTERS, "ramp": POINTERS, "peak": POINTERS, "n_nonfinite": POINTERS, "workspace": POINTERS,
                        "clip_stride": STRIDES, "track_stride": STRIDES, "out_stride": STRIDES, "normalize": (0, 1),
                        "workspace_bytes": (0, 1 << 40)}, q, "stitch") == 2048 * 8
    assert L.pg_workspace_bytes_stitch(None) == _lib.ERR_NULL
    for bad in (stitch_args(0), stitch_args(step=185), stitch_args(step=91), stitch_args(n_out=3 * 92), stitch_args(n_out=3 * 92 + 185)):
        assert q(bad) == _lib.ERR_SHAPE
        bad.clips = bad.out = bad.ramp = bad.workspace = ALIGNED
        bad.clip_stride, bad.track_stride, bad.out_stride, bad.workspace_bytes = 184, 4 * 184, bad.n_out, 1 << 20
        assert L.pg_stitch(ctypes.byref(bad), None) == _lib.ERR_SHAPE


# ---- clipnorm --------------------------------------------------------------------------------------------------------------------------
def test_clipnorm_query():
    _lib, L = lib()
    q = lambda a: L.pg_workspace_bytes_clipnorm(ctypes.byref(a))
    a = _lib.ClipNormArgs()
    for B, Cc, Ln in ((1, 8, 24), (5, 33, 77), (64, 40, 129), (64, 2048, 256)):
        a.B, a.C, a.L = B, Cc, Ln
        assert vary(a, {"x": POINTERS, "y": POINTERS, "yh": POINTERS, "gamma": POINTERS, "running_mean": POINTERS, "running_var": POINTERS,
                        "workspace": POINTERS, "x_bs": STRIDES, "y_bs": STRIDES, "yh_pitch": (0, 8, 130), "L": (1, 7, 4096),
                        "workspace_bytes": (0, 1 << 40)}, q, "clipnorm") == 8 * B * Cc
    assert L.pg_workspace_bytes_clipnorm(None) == _lib.ERR_NULL
    for B, Cc, Ln in ((0, 8, 24), (1, 0, 24), (1, 8, 0), (65536, 65536, 1)):
        a.B, a.C, a.L = B, Cc, Ln
        assert q(a) == _lib.ERR_SHAPE
        a.x = a.y = a.gamma = a.beta = a.running_mean = a.running_var = a.workspace = ALIGNED
        a.workspace_bytes = 1 << 40
        assert L.pg_clipnorm_fwd(ctypes.byref(a), None) == _lib.ERR_SHAPE


# ---- phase lock --------------------------------------------------------------------------------------------------------------------------
def test_phase_lock_query():
    _lib, L = lib()
    q = lambda a: L.pg_workspace_bytes_phase_lock(ctypes.byref(a))
    a = _lib.PhaseLockArgs()
    for n_ch, bins, F_out in ((1, 1, 1), (1, 5, 32), (3, 64, 33), (2, 1025, 65), (1, 4096, 1000), (2, 130, 64)):
        a.n_ch, a.bins, a.F_out = n_ch, bins, F_out
        assert vary(a, {"A": POINTERS, "M": POINTERS, "out": POINTERS, "workspace": POINTERS, "a_stride": STRIDES, "m_stride": STRIDES,
                        "F_src": (0, 1, 7, 1 << 40), "src_per_out": (0.5, 1.0, 3.0), "reset_below": (0.0, 0.5),
                        "workspace_bytes": (0, 1 << 40)}, q, "phase_lock") == 12 * n_ch * bins * ceil_div(F_out, 32)
    assert L.pg_workspace_bytes_phase_lock(None) == _lib.ERR_NULL
    for n_ch, bins, F_out in ((0, 5, 32), (1, 0, 32), (1, 5, 0), (1, 4097, 32)):
        a.n_ch, a.bins, a.F_out = n_ch, bins, F_out
        assert q(a) == _lib.ERR_SHAPE
        a.A = a.M = a.out = a.workspace = ALIGNED
        a.F_src, a.src_per_out, a.a_stride, a.m_stride, a.workspace_bytes = 40, 1.0, 1 << 30, 1 << 30, 1 << 40
        assert L.pg_phase_lock(ctypes.byref(a), None) == _lib.ERR_SHAPE


# ---- compare ------------------------------------------------------------------------------------------------------------------------------
def test_wave_compare_query():
    _lib, L = lib()
    q = lambda a: L.pg_workspace_bytes_wave_compare(ctypes.byref(a))
    a = _lib.WaveCompareArgs()
    for n_sig, n in ((1, 1), (1, 8191), (3, 8192), (1, 8193), (3, 3 * 8192 + 5), (64, 1 << 24)):
        a.n_signals, a.n = n_sig, n
        assert vary(a, {"x": POINTERS, "y": POINTERS, "gain": POINTERS, "out": POINTERS, "workspace": POINTERS, "x_stride": STRIDES,
                        "y_stride": STRIDES, "workspace_bytes": (0, 1 << 40)}, q, "wave_compare") == 48 * n_sig * ceil_div(n, 8192)
    assert L.pg_workspace_bytes_wave_compare(None) == _lib.ERR_NULL
    for n_sig, n in ((0, 5), (1, 0), (1 << 20, 1 << 40)):
        a.n_signals, a.n = n_sig, n
        assert q(a) == _lib.ERR_SHAPE
        a.x = a.y = a.out = a.workspace = ALIGNED
        a.x_stride = a.y_stride = 1 << 41
        a.workspace_bytes = 1 << 40
        assert L.pg_wave_compare(ctypes.byref(a), None) == _lib.ERR_SHAPE


def test_spec_compare_query():
    _lib, L = lib()
    q = lambda a: L.pg_workspace_bytes_spec_compare(ctypes.byref(a))
    a = _lib.SpecCompareArgs()
    a.floor_power = 1e-10
    for n_sig, bins, frames in ((1, 1, 1), (1, 64, 256), (2, 65, 257), (2, 130, 515), (3, 1024, 5), (1, 16, 24)):
        a.n_signals, a.bins, a.frames = n_sig, bins, frames
        tiles, blocks = ceil_div(frames, 256), ceil_div(bins, 64)
        # three regions of doubles: six sums per workgroup (tile x bin block), six per tile, one per (bin block, frame)
        want = 8 * n_sig * (tiles * blocks * 6 + tiles * 6 + blocks * frames)
        assert vary(a, {"R": POINTERS, "E": POINTERS, "gain": POINTERS, "out": POINTERS, "workspace": POINTERS, "r_stride": STRIDES,
                        "e_stride": STRIDES, "floor_power": (1e-30, 1.0), "workspace_bytes": (0, 1 << 40)}, q, "spec_compare") == want
    assert L.pg_workspace_bytes_spec_compare(None) == _lib.ERR_NULL
    for n_sig, bins, frames, floor in ((0, 16, 24, 1e-10), (1, 0, 24, 1e-10), (1, 16, 0, 1e-10), (1, 16, 24, 0.0), (1, 16, 24, float("inf")),
                                       (1, 16, 24, float("nan"))):
        a.n_signals, a.bins, a.frames, a.floor_power = n_sig, bins, frames, floor
        assert q(a) == _lib.ERR_SHAPE
        a.R = a.E = a.out = a.workspace = ALIGNED
        a.r_stride = a.e_stride = 1 << 30
        a.workspace_bytes = 1 << 40
        assert L.pg_spec_compare(ctypes.byref(a), None) == _lib.ERR_SHAPE


# ---- wgrad ----------------------------------------------------------------------------------------------------------------------------------
def test_wgrad_query_reads_no_pointer():
    from test_kernel_families import VIEW_CASES
    _lib, L = lib()
    rows = [c for c in VIEW_CASES if c[1] == "wgrad"]
    assert len(rows) >= 10
    packed = 0
    for (tr, Cin, Cout, k, s, p, Lin, B), _, sched, fam, *_ in rows:
        a = _lib.ConvArgs()
        a.B, a.Cin, a.Cout, a.Lin, a.k, a.stride, a.pad, a.schedule = B, Cin, Cout, Lin, k, s, p, sched
        a.Lout = (Lin - 1) * s - 2 * p + k if tr else (Lin + 2 * p - k) // s + 1
        op = _lib.OP_CONVT1D_WGRAD if tr else _lib.OP_CONV1D_WGRAD
        q = lambda a: L.pg_workspace_bytes_wgrad(ctypes.byref(a), op)
        adam = _lib.AdamArgs()                              # (a HOST struct, unlike the device pointers: a real one, and checked)
        adam.n, adam.p, adam.m, adam.v, adam.step = Cin * Cout * k, ALIGNED, ALIGNED, ALIGNED, 1
        got = vary(a, {"x": POINTERS, "dy": POINTERS, "dw": POINTERS, "w": POINTERS, "workspace": POINTERS, "adam": (None, ctypes.addressof(adam)),
                       "x_bs": (0, 1, 12345, 1 << 20), "dy_bs": (0, 1, 12345, 1 << 20), "workspace_bytes": (0, 1, 1 << 40)}, q, fam)
        assert got >= 512 * MIB and got % 4 == 0
        packed += got > 512 * MIB
        for prec in (1, 2):                                 # only the fp32 kernels pack operands
            a.precision = prec
            assert q(a) == 512 * MIB or fam not in ("conv_g_raw", "conv_g_ps"), (fam, prec)
        a.precision = 0
        assert L.pg_workspace_bytes_wgrad(ctypes.byref(a), _lib.OP_CONV1D_FWD) == _lib.ERR_UNSUPPORTED
    assert packed >= 6                                      # the raw-window rows (flat K and per-sample slabs) pack
