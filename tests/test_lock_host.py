"""CPU: the host half of identity phase locking (pg_phase_lock, phasegen.ops.phase_lock, phasegen.track phase="vocoder_locked"): the
exported symbols and the struct, every argument error (validation runs before any launch), the workspace query, the Python surface,
the combinations refused before any device work, properties of the numpy restatement (tests/_lock_ref.py), and -- in float64 -- the
condition on the INPUT of the GPU ordering test.

The melody condition.  On the synthetic melody of _vocoder_ref.melody (6 s at 16 kHz, n_fft 2048, hop 512) the float64 chain gives,
with the project's own analysis, the spectral convergence

    stretch   zero     plain, floor 0   plain, floor 0.2   locked, floor 0   locked, floor 0.2
    1.5       0.8991   0.4413           0.2022             0.0631            0.0631
    0.75      0.8965   0.4747           0.2159             0.0600            0.0598

so SC(locked) < 0.5 SC(plain, same floor) holds with room: the largest ratio is 0.0631 / 0.2022 = 0.312."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import _lock_ref as lref
import _stretch_args as shared
import _vocoder_ref as ref


# ---- the C entry point ---------------------------------------------------------------------------------------------------

def test_symbols_are_exported_and_listed():
    from phasegen import _lib
    lib = _lib.load()
    for name in ("pg_phase_lock", "pg_workspace_bytes_phase_lock"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    assert lib.pg_version() == 400                                                  # additive within ABI 0.4


def test_struct_layout():
    from phasegen import _lib
    A = _lib.PhaseLockArgs
    assert ctypes.sizeof(A) == 96                                                   # include/phasegen.h: "96 bytes"
    assert (A.n_ch.offset, A.bins.offset, A.F_src.offset, A.F_out.offset, A.src_per_out.offset, A.reset_below.offset) == (0, 4, 8, 16, 24, 32)
    assert (A.A.offset, A.a_stride.offset, A.M.offset, A.m_stride.offset, A.out.offset) == (40, 48, 56, 64, 72)
    assert (A.workspace.offset, A.workspace_bytes.offset) == (80, 88)
    h = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "phasegen.h")).read()
    assert re.search(r"\}\s*pg_phase_lock_args;\s*/\*\s*96 bytes\s*\*/", h)
    assert re.search(r"#define\s+PG_LOCK_REACH\s+2\b", h) and lref.REACH == 2


def _args(_lib):
    """2 channels of 5 bins, 19 source frames -> 25 output frames; pointers are fake and never dereferenced."""
    return shared.args(_lib, "pg_phase_lock")


def test_argument_errors_are_reported_before_any_launch():
    """The table pg_phase_lock shares with pg_phase_vocoder, pg_phase_lock_linked and the mapped twins (tests/_stretch_args.py), run through all six: same codes, same words;
    then what is pg_phase_lock's own."""
    from phasegen import _lib
    lib = _lib.load()
    f = lib.pg_phase_lock
    shared.run_all(_lib)
    a = _args(_lib)                                                                 # M is required here: the one documented difference
    a.M = None
    assert f(ctypes.byref(a), None) == _lib.ERR_NULL and b"required" in lib.pg_last_error_string()
    # the additions: the widest plane, and the workspace
    a = _args(_lib)
    a.bins, a.a_stride, a.m_stride = 4097, 4097 * 19, 4097 * 19
    assert f(ctypes.byref(a), None) == _lib.ERR_SHAPE and b"4096 bins" in lib.pg_last_error_string()
    for off in (1, 2, 3):
        a = _args(_lib)
        a.workspace = 4096 + off
        assert f(ctypes.byref(a), None) == _lib.ERR_ALIGN and b"misaligned" in lib.pg_last_error_string(), off
    need = lib.pg_workspace_bytes_phase_lock(ctypes.byref(_args(_lib)))
    for ws, nbytes in ((None, 1 << 20), (4096, need - 1), (4096, 0), (4096, -1)):
        a = _args(_lib)
        a.workspace, a.workspace_bytes = ws, nbytes
        assert f(ctypes.byref(a), None) == _lib.ERR_WORKSPACE and b"workspace" in lib.pg_last_error_string(), (ws, nbytes)


def test_workspace_query():
    """A host function of n_ch, bins and F_out: positive, monotone in F_out, 12 bytes per bin, channel and chunk."""
    from phasegen import _lib, ops
    lib = _lib.load()
    q = lib.pg_workspace_bytes_phase_lock
    assert q(None) == _lib.ERR_NULL
    L = ops.PHASE_LOCK_CHUNK
    assert L >= 4 and L % 4 == 0
    last = 0
    for F_out in (1, 2, L - 1, L, L + 1, 3 * L + 5, 10 ** 6, 10 ** 9):
        a = _args(_lib)
        a.F_out = F_out
        a.A = a.M = a.out = a.workspace = None                                      # the query looks at no pointer
        n = q(ctypes.byref(a))
        assert n == 12 * 2 * 5 * -(-F_out // L) and n > 0 and n >= last, (F_out, n)
        last = n
    for field, bad in (("n_ch", 0), ("bins", 0), ("F_out", 0), ("bins", 4097), ("F_out", -1)):
        a = _args(_lib)
        setattr(a, field, bad)
        assert q(ctypes.byref(a)) == _lib.ERR_SHAPE, (field, bad)
    a = _args(_lib)
    a.n_ch, a.F_out = 1 << 20, 1 << 50                                              # more (channel, chunk) pairs than a grid holds
    assert q(ctypes.byref(a)) == _lib.ERR_SHAPE


# ---- the Python surface --------------------------------------------------------------------------------------------------

def test_python_surface():
    """Signatures only (the calls need a GPU)."""
    from phasegen import ops, track
    p = inspect.signature(ops.phase_lock).parameters
    assert list(p) == ["angle", "F_out", "src_per_out", "logmag", "reset_below", "out"]
    assert (p["src_per_out"].default, p["logmag"].default, p["reset_below"].default, p["out"].default) == (1.0, None, 0.0, None)
    assert list(p) == list(inspect.signature(ops.phase_vocoder).parameters)
    with pytest.raises(ValueError, match="logmag"):
        ops.phase_lock(None, 5)                                                     # refused before anything is looked at
    assert "vocoder_locked" in track.STRETCH_PHASES and track.STRETCH_PHASES[:3] == ("unet", "vocoder", "zero")
    assert "vocoder_locked" not in track.PHASES
    assert inspect.signature(track.evaluate_stretch).parameters["phases"].default == ("unet", "vocoder", "zero")


def test_bad_combinations_are_refused_before_any_device_work():
    from phasegen import track
    x = np.zeros(1000, np.float32)
    small = dict(n_fft=32, hop_length=8, frames=24, overlap_frames=4)
    # (the messages are those of a KNOWN phase: an unknown name is refused with "phase must be ...")
    for kw, msg in ((dict(join="waveform"), "phase 'vocoder_locked' needs join='spectral'"), (dict(), "phase 'vocoder_locked' needs join='spectral'"),
                    (dict(join="waveform", stretch=1.5), "stretch 1.5 needs join='spectral'"), (dict(join="sideways"), "join must be")):
        with pytest.raises(ValueError, match=msg):
            track.reconstruct_track(None, x, phase="vocoder_locked", **kw, **small)
    with pytest.raises(ValueError):
        track.reconstruct_track(None, x, phase="phaselock", join="spectral", **small)             # the name stays refused
    for join in ("waveform", "spectral"):
        with pytest.raises(ValueError):
            track.evaluate_track(None, x, phases=("vocoder_locked",), join=join, **small)         # PHASES is untouched
    for phases, msg in ((("vocoder_locked", "vocoder_locked"), "without repetitions"), (("vocoder_locked", "original"), "unknown phase 'original'"),
                        (("vocoder_locked", "unet"), "needs a model"), (("phaselock",), "unknown phase 'phaselock'")):
        with pytest.raises(ValueError, match=msg):
            track.evaluate_stretch(None, x, 1.5, phases=phases, **small)
    with pytest.raises(ValueError, match="reset_below"):
        track.evaluate_stretch(None, x, 1.5, phases=("vocoder_locked",), reset_below=-0.1, **small)
    with pytest.raises(ValueError):
        track.pitch_shift(None, x, 25, phase="vocoder_locked", **small)


# ---- the restatement itself ----------------------------------------------------------------------------------------------

def test_ref_peak_map_plateau_tie_and_nan():
    f = lambda *v: np.array(v, np.float32)
    nan, inf = np.nan, np.inf
    assert list(lref.peaks(f(1, 3, 3, 3, 1))) == [False, True, False, False, False]            # the first bin of a plateau
    assert list(lref.peak_map(f(1, 3, 3, 3, 1, 0, 0, 2, 0, 0, 0))) == [1, 1, 1, 1, 1, 7, 7, 7, 7, 7, 7]      # bin 4: 3 from both, the lower
    assert list(lref.peak_map(f(5, 0, 0, 0, 5, 0, 0, 0, 5))) == [0, 0, 0, 4, 4, 4, 4, 8, 8]      # ties at bins 2 and 6
    assert not lref.peaks(f(0, 0, 7, nan, 0, 0, 9, 0, nan)).any()                              # a NaN within reach disqualifies 7 and 9
    assert list(np.flatnonzero(lref.peaks(f(0, 0, 7, nan, 0, 0, 9, 0, 0, nan)))) == [6]        # ... one bin further off it does not
    assert list(lref.peaks(f(0, 0, 9, 0, 0))) == [False, False, True, False, False]             # (bin 0 of an all-equal start is a peak
    assert list(lref.peaks(f(0, 0, 0, 0))) == [True, False, False, False]                       #  unless a larger bin is within reach)
    assert list(lref.peaks(f(2, 1, 3, 1, 2))) == [False, False, True, False, False]             # reach 2: bins 0 and 4 see the 3
    assert list(lref.peaks(f(2, 1, 1, 3, 1, 1, 2))) == [True, False, False, True, False, False, True]       # (the 3 is out of their reach)
    assert list(lref.peaks(f(0, inf, inf, -inf, -inf))) == [False, True, False, False, False]
    assert list(lref.peak_map(f(nan, nan, nan))) == [0, 1, 2] and list(lref.peak_map(f(nan, 1, nan))) == [0, 1, 2]      # no peak: P(b) = b
    assert list(lref.peak_map(f(4.0))) == [0] and list(lref.peak_map(f(nan))) == [0]
    assert lref.peak_map(f(1, 2)).dtype == np.int64 and list(lref.peak_map(f(1, 2))) == [1, 1] and list(lref.peak_map(f(2, 2))) == [0, 0]


def test_ref_equals_the_plain_vocoder_where_every_bin_is_its_own_region():
    rs = np.random.RandomState(1)
    A = rs.uniform(-np.pi, np.pi, (2, 5, 19)).astype(np.float32)
    M = rs.uniform(0, 1, A.shape).astype(np.float32)
    for rate in (1.0, 0.5, 1 / 1.3, 2.0):
        one = lref.phase_lock(A[:, :1], 25, rate, M[:, :1], 0.4)                                # bins = 1
        assert one.shape == (2, 1, 25) and one.dtype == np.float32
        assert np.array_equal(one, ref.phase_vocoder(A[:, :1], 25, rate, M[:, :1], 0.4)), rate
        nan = np.full_like(M, np.nan)
        assert np.array_equal(lref.phase_lock(A, 25, rate, nan, 0.4), ref.phase_vocoder(A, 25, rate, nan, 0.4)), rate
        assert np.array_equal(lref.phase_lock(A, 25, rate, nan, 0.4), ref.phase_vocoder(A, 25, rate)), rate
    assert not np.array_equal(lref.phase_lock(A, 25, 0.5, M, 0.0), ref.phase_vocoder(A, 25, 0.5, M, 0.0))


def test_ref_telescopes_at_rate_one():
    rs = np.random.RandomState(2)
    A = rs.uniform(-np.pi, np.pi, (2, 9, 19)).astype(np.float32)
    M = rs.uniform(0, 1, A.shape).astype(np.float32)
    for floor in (0.0, 0.5):
        out, T = lref.phase_lock(A, 25, 1.0, M, floor, return_rotation=True)
        assert np.array_equal(out[..., :19], ref.angle_of(ref.q(A))) and not T[..., :19].any()  # the rotation stays zero
        assert np.array_equal(out[..., 19:], np.repeat(out[..., 18:19], 6, -1))                 # past the end the advance is zero


def test_ref_rotation_is_constant_over_each_region():
    rs = np.random.RandomState(3)
    A = rs.uniform(-np.pi, np.pi, (2, 40, 30)).astype(np.float32)
    M = rs.uniform(0, 1, A.shape).astype(np.float32)
    for rate, floor in ((0.5, 0.0), (1 / 1.3, 0.5), (2.0, 0.5)):
        F_out = 35
        out, T = lref.phase_lock(A, F_out, rate, M, floor, return_rotation=True)
        i0, _ = ref.positions(F_out, rate, 30)
        assert T.dtype == np.uint32 and not T[..., 0].any()
        moved = 0
        for c in range(2):
            for g in range(1, F_out):
                P = lref.peak_map(M[c, :, i0[g]])
                assert np.array_equal(T[c, :, g], T[c, P, g]), (rate, c, g)                     # identity locking
                assert np.array_equal(out[c, :, g], ref.angle_of(T[c, :, g] + ref.q(A[c, :, i0[g]])))
                moved += int(T[c, :, g].any())
        assert moved > F_out                                                                    # (and it does rotate)


def test_ref_a_quiet_peak_resets_its_region_and_a_quiet_bin_under_a_loud_peak_stays_locked():
    # bins 0 .. 3 belong to the loud peak at bin 1, bins 4 .. 7 to the quiet peak at bin 6 (bin 3 is 2 from bin 1 and 3 from bin 6)
    m = np.array([0.5, 2.0, 0.01, 0.02, 0.03, 0.04, 0.1, 0.05], np.float32)
    assert list(lref.peak_map(m)) == [1, 1, 1, 1, 6, 6, 6, 6]
    rs = np.random.RandomState(4)
    A = rs.uniform(-np.pi, np.pi, (8, 12)).astype(np.float32)
    M = np.repeat(m[:, None], 12, 1)
    out, T = lref.phase_lock(A, 20, 0.5, M, 0.3, return_rotation=True)
    i0, _ = ref.positions(20, 0.5, 12)
    assert np.array_equal(out[4:], ref.angle_of(ref.q(A[4:][:, i0]))) and not T[4:].any()       # the analysis phase itself
    assert T[:4, 2:].all() and np.array_equal(T[:4], np.repeat(T[1:2], 4, 0))                   # bins 2 and 3 are below the floor, and locked
    plain = ref.phase_vocoder(A, 20, 0.5, M, 0.3)
    assert np.array_equal(out[1], plain[1])                                                     # the peak itself is the plain vocoder's bin
    assert np.array_equal(plain[2:4], ref.angle_of(ref.q(A[2:4][:, i0]))) and not np.array_equal(out[2:4], plain[2:4])


# ---- the input condition of the GPU ordering test, in float64 ---------------------------------------------------------------

@pytest.fixture(scope="module")
def melody():
    return ref.melody()[None]


@pytest.mark.parametrize("stretch", [1.5, 0.75])
def test_melody_locked_is_twice_as_consistent_as_the_plain_vocoder(melody, stretch):
    from phasegen.track import spectral_plan
    pl = spectral_plan(melody.shape[1], 128, 512, 32, stretch)
    logmag, ang = ref.analysis64(melody, pl.n_src, 2048, 512)
    mag = ref.resample64(logmag, pl.F_out, 1.0 / stretch)
    A, M = ang.astype(np.float32), logmag.astype(np.float32)
    for floor in (0.0, 0.2):
        plain = ref.consistency64(mag, 2048, 512, phase=ref.phase_vocoder(A, pl.F_out, 1.0 / stretch, M, floor))["spectral_convergence"]
        locked = ref.consistency64(mag, 2048, 512, phase=lref.phase_lock(A, pl.F_out, 1.0 / stretch, M, floor))["spectral_convergence"]
        print(f"\nmelody, stretch {stretch}, floor {floor:g}: SC plain {plain:.4f}, locked {locked:.4f} (ratio {locked / plain:.3f})")
        assert locked < 0.5 * plain, (floor, locked, plain)
