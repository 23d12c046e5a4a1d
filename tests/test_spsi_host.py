"""CPU: the host half of single-pass spectrogram inversion (pg_phase_spsi, phasegen.ops.phase_spsi, phasegen.track phase="spsi"): the
exported symbols and the struct, every argument error (validation runs before any launch), the workspace query, the Python surface,
properties of the numpy restatement (tests/_spsi_ref.py), and -- in float64 -- the condition on the INPUT of the GPU ordering test.

The melody condition.  On the synthetic melody of _vocoder_ref.melody (6 s at 16 kHz, n_fft 2048, hop 512) the float64 chain gives,
with the project's own analysis resampled to the output grid, the spectral convergence

    stretch   spsi     zero
    1.0       0.0833   0.898
    1.5       0.0718   0.899

so SC(spsi) < 0.25 SC(zero) holds with room: the largest ratio is 0.0833 / 0.898 = 0.093."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import _lock_ref as lref
import _spsi_ref as sref
import _vocoder_ref as ref


# ---- the C entry point ---------------------------------------------------------------------------------------------------

def test_symbols_are_exported_and_listed():
    from phasegen import _lib
    lib = _lib.load()
    for name in ("pg_phase_spsi", "pg_workspace_bytes_phase_spsi"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    assert lib.pg_version() == 400                                                  # additive within ABI 0.4


def test_struct_layout():
    from phasegen import _lib
    A = _lib.PhaseSpsiArgs
    assert ctypes.sizeof(A) == 72                                                   # include/phasegen.h: "72 bytes"
    assert (A.n_ch.offset, A.bins.offset, A.F.offset, A.n_fft.offset, A.hop.offset, A.bin0.offset) == (0, 4, 8, 16, 20, 24)
    assert (A.M.offset, A.m_stride.offset, A.out.offset, A.workspace.offset, A.workspace_bytes.offset) == (32, 40, 48, 56, 64)
    h = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "phasegen.h")).read()
    assert re.search(r"\}\s*pg_phase_spsi_args;\s*/\*\s*72 bytes\s*\*/", h)


def _args(_lib):
    """2 channels of 5 bins, 25 frames at 32 / 8; pointers are fake and never dereferenced."""
    a = _lib.PhaseSpsiArgs()
    a.n_ch, a.bins, a.F, a.n_fft, a.hop, a.bin0 = 2, 5, 25, 32, 8, 1
    a.M = a.out = a.workspace = 4096
    a.m_stride, a.workspace_bytes = 5 * 25, 1 << 20
    return a


def _set(**fields):
    def change(a):
        for k, v in fields.items():
            setattr(a, k, v)
    return change


def test_argument_errors_are_reported_before_any_launch():
    from phasegen import _lib
    lib = _lib.load()
    f = lib.pg_phase_spsi
    assert f(None, None) == _lib.ERR_NULL
    t = [(f"{n} NULL", _set(**{n: None}), _lib.ERR_NULL, b"required") for n in ("M", "out")]
    t += [(f"{n} = {bad}", _set(**{n: bad}), _lib.ERR_SHAPE, b"non-positive") for n in ("n_ch", "bins", "F") for bad in (0, -3)]
    t += [("4097 bins", _set(bins=4097, m_stride=4097 * 25), _lib.ERR_SHAPE, b"4096 bins")]
    t += [(f"hop {hop} n_fft {n_fft}", _set(hop=hop, n_fft=n_fft), _lib.ERR_SHAPE, b"hop")
          for hop, n_fft in ((0, 32), (-1, 32), (33, 32), (8, 0), (8, -32), (1, 0))]
    t += [(f"bin0 = {bad}", _set(bin0=bad), _lib.ERR_SHAPE, b"bin0") for bad in (-1, 65537, 1 << 30)]
    t += [("2^62 plane", _set(F=1 << 61, m_stride=1 << 62), _lib.ERR_SHAPE, b"2^62")]
    t += [("m_stride short", _set(m_stride=5 * 25 - 1), _lib.ERR_SHAPE, b"m_stride")]
    t += [("2^62 output", _set(n_ch=1 << 30, bins=4096, F=1 << 49, m_stride=1 << 62), _lib.ERR_SHAPE, b"2^62")]
    t += [(f"{n} + {off}", _set(**{n: 4096 + off}), _lib.ERR_ALIGN, b"misaligned") for n in ("M", "out", "workspace") for off in (1, 2, 3)]
    need = lib.pg_workspace_bytes_phase_spsi(ctypes.byref(_args(_lib)))
    assert need == 12 * 2 * 5 * 1
    t += [(f"workspace {ws}, {n} bytes", _set(workspace=ws, workspace_bytes=n), _lib.ERR_WORKSPACE, b"workspace")
          for ws, n in ((None, 1 << 20), (4096, need - 1), (4096, 0), (4096, -1))]
    for label, change, code, word in t:
        a = _args(_lib)
        change(a)
        got = f(ctypes.byref(a), None)
        msg = lib.pg_last_error_string()
        assert got == code and word in msg and msg.startswith(b"phase_spsi: "), (label, got, msg)
    # the order of pg_stretch_check: NULL before shape before alignment before the workspace
    for fields, code in ((dict(M=None, bins=0), _lib.ERR_NULL), (dict(bins=0, out=4097), _lib.ERR_SHAPE), (dict(hop=0, bin0=-1), _lib.ERR_SHAPE),
                         (dict(out=4097, workspace_bytes=0), _lib.ERR_ALIGN), (dict(bin0=-1, workspace=None), _lib.ERR_SHAPE)):
        a = _args(_lib)
        _set(**fields)(a)
        assert f(ctypes.byref(a), None) == code, fields
    a = _args(_lib)
    _set(hop=0, bin0=-1)(a)
    assert f(ctypes.byref(a), None) == _lib.ERR_SHAPE and b"hop" in lib.pg_last_error_string()      # hop / n_fft before bin0
    # the limits themselves are accepted as far as the host goes: hop == n_fft, bin0 == 65536, bin0 == 0 (refused only by the workspace)
    for fields in (dict(hop=32), dict(bin0=65536), dict(bin0=0), dict(hop=1, n_fft=1)):
        a = _args(_lib)
        _set(workspace_bytes=0, **fields)(a)
        assert f(ctypes.byref(a), None) == _lib.ERR_WORKSPACE, fields


def test_workspace_query():
    """A host function of n_ch, bins and F: positive, monotone in F, 12 bytes per bin, channel and chunk -- pg_phase_lock's."""
    from phasegen import _lib, ops
    lib = _lib.load()
    q = lib.pg_workspace_bytes_phase_spsi
    assert q(None) == _lib.ERR_NULL
    L = ops.PHASE_LOCK_CHUNK
    last = 0
    for F in (1, 2, L - 1, L, L + 1, 3 * L + 5, 10 ** 6, 10 ** 9):
        a = _args(_lib)
        a.F = F
        a.M = a.out = a.workspace = None                                            # the query looks at no pointer
        n = q(ctypes.byref(a))
        lk = _lib.PhaseLockArgs()
        lk.n_ch, lk.bins, lk.F_out = 2, 5, F
        assert n == 12 * 2 * 5 * -(-F // L) == lib.pg_workspace_bytes_phase_lock(ctypes.byref(lk)) and n > 0 and n >= last, (F, n)
        last = n
    for field, bad in (("n_ch", 0), ("bins", 0), ("F", 0), ("bins", 4097), ("F", -1)):
        a = _args(_lib)
        setattr(a, field, bad)
        assert q(ctypes.byref(a)) == _lib.ERR_SHAPE, (field, bad)
    a = _args(_lib)
    a.n_ch, a.F = 1 << 20, 1 << 50                                                  # more (channel, chunk) pairs than a grid holds
    assert q(ctypes.byref(a)) == _lib.ERR_SHAPE


# ---- the Python surface --------------------------------------------------------------------------------------------------

def test_python_surface():
    """Signatures and tuples only (the calls need a GPU)."""
    from phasegen import ops, track
    p = inspect.signature(ops.phase_spsi).parameters
    assert list(p) == ["logmag", "n_fft", "hop", "bin0", "out"] and (p["bin0"].default, p["out"].default) == (1, None)
    assert track.STRETCH_PHASES == ("unet", "vocoder", "zero", "vocoder_locked", "spsi")
    assert track.PHASES == ("unet", "zero", "original", "griffinlim")                              # unchanged
    assert track.REPORT_PHASES == track.PHASES + ("spsi",)
    assert inspect.signature(track.evaluate_stretch).parameters["phases"].default == ("unet", "vocoder", "zero")
    assert track.evaluate_track.options == {"join": "waveform"} and track.evaluate_track.later_options == {"gl_init": "noise"}
    assert track.reconstruct_track.options == {"join": "waveform", "stretch": 1.0}


def test_bad_combinations_are_refused_before_any_device_work():
    from phasegen import track
    x = np.zeros(1000, np.float32)
    small = dict(n_fft=32, hop_length=8, frames=24, overlap_frames=4)
    for kw, msg in ((dict(join="waveform"), "phase 'spsi' needs join='spectral'"), (dict(), "phase 'spsi' needs join='spectral'"),
                    (dict(join="waveform", stretch=1.5), "stretch 1.5 needs join='spectral'"), (dict(join="sideways"), "join must be")):
        with pytest.raises(ValueError, match=msg):
            track.reconstruct_track(None, x, phase="spsi", **kw, **small)
    with pytest.raises(ValueError, match="phase 'spsi' needs join='spectral'"):
        track.evaluate_track(None, x, phases=("spsi",), **small)                                  # the waveform join
    with pytest.raises(ValueError, match="gl_init must be"):
        track.evaluate_track(None, x, phases=("zero",), gl_init="silence", **small)
    for phases, msg in ((("spsi", "spsi"), "without repetitions"), (("spsi", "original"), "unknown phase 'original'"),
                        (("spsi", "unet"), "needs a model")):
        with pytest.raises(ValueError, match=msg):
            track.evaluate_stretch(None, x, 1.5, phases=phases, **small)
    with pytest.raises(ValueError):
        track.pitch_shift(None, x, 25, phase="spsi", **small)


# ---- the restatement itself ----------------------------------------------------------------------------------------------

def test_ref_closed_form_on_constant_columns():
    """Every column the same: the regions never change, so Theta_g[b] = g * adv[P(b)] exactly (mod 2^32), for any bin0 and hop."""
    rs = np.random.RandomState(1)
    for bins, (n_fft, hop, bin0) in ((40, (2048, 512, 1)), (9, (8, 3, 0)), (130, (32, 1, 1)), (5, (2048, 2048, 1))):
        F = 101
        m = rs.uniform(0, 1, bins).astype(np.float32)
        out, theta = sref.phase_spsi(np.repeat(m[None, :, None], F, 2), n_fft, hop, bin0, return_theta=True)
        P, adv = lref.peak_map(m), sref.advance(m, n_fft, hop, bin0)
        g = np.arange(F, dtype=np.uint64)
        want = ((g[None, :] * adv[P].astype(np.uint64)[:, None]) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
        assert theta.dtype == np.uint32 and np.array_equal(theta[0], want)
        assert np.array_equal(out[0], ref.angle_of(want + sref.parity(bins, bin0)[:, None]))
        assert out.dtype == np.float32 and np.abs(out).max() <= np.float32(np.pi)
        if hop == n_fft:                                                                        # whole turns but for the offset
            flat = np.flatnonzero(sref.offset(m, np.arange(bins))[0][P] == 0)
            assert not theta[0, flat].any()


def test_ref_the_offset_is_within_half_a_bin_and_the_curvature_negative_at_every_peak():
    rs = np.random.RandomState(2)
    seen = 0
    for trial in range(200):
        bins = int(rs.randint(3, 200))
        m = (rs.uniform(0, 1, bins) ** rs.choice([1, 4])).astype(np.float32)
        if trial % 5 == 0:
            m[rs.randint(0, bins, bins // 3)] = m[rs.randint(0, bins)]                          # plateaus and ties
        pk = np.flatnonzero(lref.peaks(m))
        inner = pk[(pk > 0) & (pk < bins - 1)]
        delta, d = sref.offset(m, pk)
        assert (np.abs(delta) <= 0.5).all() and delta.dtype == np.float32
        # an interior peak is > its lower neighbour and >= its upper one: d = (alpha - beta) + (gamma - beta) < 0 strictly
        assert (sref.offset(m, inner)[1] < 0).all()
        assert not delta[(pk == 0) | (pk == bins - 1)].any()                                    # the edges have no parabola
        seen += inner.size
    assert seen > 2000
    f = lambda *v: np.array(v, np.float32)
    assert sref.offset(f(1, 3, 1), [1])[0][0] == 0 and sref.offset(f(1, 3, 2), [1])[0][0] == np.float32(-0.5) / np.float32(-3)
    assert sref.offset(f(0, 2, 2), [1])[0][0] == np.float32(0.5)                                # a plateau's first bin: exactly half a bin
    assert sref.offset(f(3, 1, 3), [1])[0][0] == 0                                              # d > 0: not a maximum
    assert sref.offset(f(np.nan, 2, 1), [1])[0][0] == 0 and sref.offset(f(np.inf, np.inf, 0), [1])[0][0] == 0      # NaN covers inf - inf
    assert sref.offset(f(0, np.inf, 0), [1])[0][0] == 0


def test_ref_theta_is_constant_over_each_region_and_odd_bins_get_half_a_turn():
    rs = np.random.RandomState(3)
    M = rs.uniform(0, 1, (2, 40, 30)).astype(np.float32)
    for bin0 in (0, 1):
        out, theta = sref.phase_spsi(M, 64, 16, bin0, return_theta=True)
        assert not theta[..., 0].any()
        assert np.array_equal(out[..., 0], np.broadcast_to(ref.angle_of(sref.parity(40, bin0)), (2, 40)))
        assert set(np.unique(out[..., 0])) == {np.float32(0), np.float32(-np.pi)}
        for c in range(2):
            for g in range(1, 30):
                P = lref.peak_map(M[c, :, g])
                assert np.array_equal(theta[c, :, g], theta[c, P, g]), (c, g)
    one = sref.phase_spsi(M[:1], 64, 16)
    assert np.array_equal(one, sref.phase_spsi(M, 64, 16)[:1])                                  # a channel does not depend on n_ch


# ---- the input condition of the GPU ordering test, in float64 ---------------------------------------------------------------

@pytest.fixture(scope="module")
def melody():
    return ref.melody()[None]


@pytest.mark.parametrize("stretch", [1.0, 1.5])
def test_melody_spsi_is_four_times_as_consistent_as_zero_phase(melody, stretch):
    from phasegen.track import spectral_plan
    pl = spectral_plan(melody.shape[1], 128, 512, 32, stretch)
    logmag, _ang = ref.analysis64(melody, pl.n_src, 2048, 512)
    mag = ref.resample64(logmag, pl.F_out, 1.0 / stretch)
    spsi = ref.consistency64(mag, 2048, 512, phase=sref.phase_spsi(mag.astype(np.float32), 2048, 512))["spectral_convergence"]
    zero = ref.consistency64(mag, 2048, 512, phase=np.zeros_like(mag))["spectral_convergence"]
    print(f"\nmelody, stretch {stretch}: SC spsi {spsi:.4f}, zero {zero:.4f} (ratio {spsi / zero:.3f})")
    assert spsi < 0.25 * zero, (spsi, zero)
