"""CPU: the host half of the phase vocoder (pg_phase_vocoder, phasegen.ops.phase_vocoder, phasegen.track phase="vocoder" and
evaluate_stretch, phasegen.metrics.consistency): the exported symbol and its struct, every argument error (validation runs before
any launch), the Python signatures, the combinations refused before any device work, properties of the numpy restatement
(tests/_vocoder_ref.py), and -- in float64 -- the condition on the INPUT of the GPU ordering test.

The melody condition.  On the synthetic melody of _vocoder_ref.melody (6 s at 16 kHz, n_fft 2048, hop 512) the float64 chain gives
spectral convergence SC(vocoder) < 0.5 SC(zero) at stretch 1.5 and 0.75.  Measured with the project's own analysis (the track's own
moments: (v - mean) / std over all real and imaginary parts; log-magnitudes interpolated, as pg_spec_clips does):

    stretch   zero     floor 0   0.01     0.05     0.2
    1.5       0.8991   0.4413    0.3389   0.2419   0.2022
    0.75      0.8965   0.4747    0.3072   0.2604   0.2159

Without any reset (floor 0) the ratio is 0.491 at 1.5 and 0.530 at 0.75: the figures of a vocoder without reset move with how the
magnitudes are interpolated (a trial with linearly interpolated magnitudes and the crude standardisation S / std|S| gave 0.39 and 0.34
against 0.90), so the 0.5 x condition is kept and asserted for the floors 0.01 and 0.05, the two smallest floors that reset at all;
the floor-0 figures are printed, and floor 0.05 is required to beat floor 0."""
import ctypes
import inspect

import numpy as np
import pytest

import _stretch_args as shared
import _vocoder_ref as ref


# ---- the C entry point ---------------------------------------------------------------------------------------------------

def test_symbol_is_exported_and_listed():
    from phasegen import _lib
    lib = _lib.load()
    assert "pg_phase_vocoder" in _lib.SYMBOLS and hasattr(lib, "pg_phase_vocoder")
    assert lib.pg_version() == 400                                                  # additive within ABI 0.4


def test_struct_layout():
    from phasegen import _lib
    A = _lib.PhaseVocoderArgs
    assert ctypes.sizeof(A) == 80                                                   # include/phasegen.h: "80 bytes"
    assert (A.n_ch.offset, A.bins.offset, A.F_src.offset, A.F_out.offset, A.src_per_out.offset, A.reset_below.offset) == (0, 4, 8, 16, 24, 32)
    assert (A.A.offset, A.a_stride.offset, A.M.offset, A.m_stride.offset, A.out.offset) == (40, 48, 56, 64, 72)
    import os
    import re
    h = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "phasegen.h")).read()
    assert re.search(r"\}\s*pg_phase_vocoder_args;\s*/\*\s*80 bytes\s*\*/", h)


def _args(_lib):
    """2 channels of 5 bins, 19 source frames -> 25 output frames; pointers are fake and never dereferenced."""
    return shared.args(_lib, "pg_phase_vocoder")


def test_argument_errors_are_reported_before_any_launch():
    """The table pg_phase_vocoder shares with pg_phase_lock, pg_phase_lock_linked and the mapped twins of all three (tests/_stretch_args.py: null fields, non-positive sizes, the bad
    src_per_out and reset_below, short strides, misaligned pointers, the 2^62 overflow), run through all six: same codes, same words."""
    from phasegen import _lib
    lib = _lib.load()
    shared.run_all(_lib)
    a = _args(_lib)                                                                 # without M its stride is not looked at
    a.M, a.m_stride, a.n_ch, a.bins, a.F_out = None, 0, 1 << 30, 1 << 30, 1 << 62
    a.a_stride = (1 << 30) * 19
    assert lib.pg_phase_vocoder(ctypes.byref(a), None) == _lib.ERR_SHAPE and b"2^62" in lib.pg_last_error_string()


# ---- the Python surface --------------------------------------------------------------------------------------------------

def test_python_surface():
    """Signatures only (the calls need a GPU)."""
    from phasegen import metrics, ops, track
    p = inspect.signature(ops.phase_vocoder).parameters
    assert list(p) == ["angle", "F_out", "src_per_out", "logmag", "reset_below", "out"]
    assert (p["src_per_out"].default, p["logmag"].default, p["reset_below"].default, p["out"].default) == (1.0, None, 0.0, None)
    p = inspect.signature(metrics.consistency).parameters
    assert list(p) == ["logmag", "audio", "n_fft", "hop_length", "floor"] and p["floor"].default == 1e-10
    p = inspect.signature(track.evaluate_stretch).parameters
    assert list(p) == ["model", "audio", "stretch", "n_fft", "hop_length", "frames", "overlap_frames", "stats", "osr", "sr", "res_type",
                       "clip_batch", "phases", "reset_below", "floor", "return_audio"]
    assert p["phases"].default == ("unet", "vocoder", "zero") and p["reset_below"].default is None and p["n_fft"].default == 2048
    assert (p["hop_length"].default, p["frames"].default, p["overlap_frames"].default, p["clip_batch"].default) == (512, 128, 32, 64)
    assert track.VOCODER_RESET_BELOW in (0.0, 0.01, 0.05, 0.2)
    # what the earlier features pinned stays as it was
    assert track.reconstruct_track.options == {"join": "waveform", "stretch": 1.0} and track.evaluate_track.options == {"join": "waveform"}
    assert track.PHASES == ("unet", "zero", "original", "griffinlim") and track.JOINS == ("waveform", "spectral")
    assert "consistency" not in metrics.KEYS and len(metrics.KEYS) == 10


def test_bad_combinations_are_refused_before_any_device_work():
    from phasegen import track
    x = np.zeros(1000, np.float32)
    small = dict(n_fft=32, hop_length=8, frames=24, overlap_frames=4)
    for kw in (dict(join="waveform"), dict(), dict(join="waveform", stretch=1.5), dict(join="sideways")):
        with pytest.raises(ValueError):
            track.reconstruct_track(None, x, phase="vocoder", **kw, **small)
    with pytest.raises(ValueError):
        track.reconstruct_track(None, x, phase="phaselock", join="spectral", **small)
    with pytest.raises(ValueError):
        track.evaluate_track(None, x, phases=("zero", "vocoder"), join="spectral", **small)       # PHASES is untouched
    for phases in ((), ("vocoder", "vocoder"), ("zero", "original"), ("griffinlim",), ("vocoder", "nope"), ("unet", "zero")):
        with pytest.raises(ValueError):
            track.evaluate_stretch(None, x, 1.5, phases=phases, **small)                          # ("unet" without a model)
    for bad in (-0.1, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            track.evaluate_stretch(None, x, 1.5, phases=("vocoder",), reset_below=bad, **small)
    with pytest.raises(ValueError):
        track.pitch_shift(None, x, 25, phase="vocoder", **small)


# ---- the restatement itself ----------------------------------------------------------------------------------------------

def test_ref_quantisation():
    x = np.array([0.0, np.pi, -np.pi, np.nan, np.inf, -np.inf, 2.0 ** 20, 2.0 ** 20 * (1 + 2.0 ** -23), -3e6, 1e-12], np.float32)
    got = ref.q(x)
    assert got.dtype == np.uint32
    assert list(got[[0, 3, 4, 5, 7, 8, 9]]) == [0] * 7
    # fp32 pi is 8.74e-8 above pi: 2^31 + rint(8.74e-8 K) = 2^31 + 60; -pi is its two's complement
    assert int(got[1]) == 2 ** 31 + 60 and int(got[2]) == 2 ** 32 - (2 ** 31 + 60)
    assert int(got[6]) == int(np.rint(2.0 ** 20 * ref.K)) % 2 ** 32                 # |x| == 2^20 is still quantised
    a = ref.angle_of(got[1:3]).astype(np.float64)                                   # pi_f comes back from the other side of the cut
    assert a[0] < 0 < a[1] and abs(a[0] + 2 * np.pi - float(x[1])) <= 2.0 ** -23 + 2.0 ** -30 and a[1] == -a[0]
    assert ref.angle_of(np.array([2 ** 31, 2 ** 31 - 1], np.uint32)).tolist() == [-float(np.float32(np.pi)), float(np.float32(np.pi))]
    assert np.all(np.abs(ref.angle_of(np.arange(0, 2 ** 32, 2 ** 20 - 1, dtype=np.uint64).astype(np.uint32))) <= np.float32(np.pi))


def test_ref_telescopes_at_rate_one():
    rs = np.random.RandomState(1)
    A = rs.uniform(-np.pi, np.pi, (2, 5, 19)).astype(np.float32)
    out = ref.phase_vocoder(A, 25, 1.0)
    assert out.shape == (2, 5, 25) and out.dtype == np.float32
    assert np.array_equal(out[..., :19], ref.angle_of(ref.q(A)))                    # acc[g] = q(A[g]) exactly
    assert np.array_equal(out[..., 19:], np.repeat(out[..., 18:19], 6, -1))         # past the end the advance is zero
    d = np.angle(np.exp(1j * (out[..., :19].astype(np.float64) - A.astype(np.float64))))
    assert np.abs(d).max() <= 2.0 ** -23 + 2.0 ** -30


def test_ref_half_rate_repeats_every_advance_twice():
    rs = np.random.RandomState(2)
    A = rs.uniform(-np.pi, np.pi, (3, 11)).astype(np.float32)
    out = ref.phase_vocoder(A, 20, 0.5)
    qA = ref.q(A).astype(np.int64)
    acc = qA[:, 0].copy()
    for g in range(20):
        assert np.array_equal(out[:, g], ref.angle_of((acc % 2 ** 32).astype(np.uint32))), g
        acc += qA[:, g // 2 + 1] - qA[:, g // 2]                                    # frames 2 i and 2 i + 1 both advance by d[i]
    # so the even output frames run at twice the analysis' advance
    twice = (qA[:, :1] + 2 * (qA[:, :10] - qA[:, :1])) % 2 ** 32
    assert np.array_equal(out[:, 0:20:2], ref.angle_of(twice.astype(np.uint32)))


def test_ref_all_reset_plane_returns_the_analysis_phase():
    rs = np.random.RandomState(3)
    A = rs.uniform(-np.pi, np.pi, (2, 3, 13)).astype(np.float32)
    M = np.zeros_like(A)
    for rate in (1.0, 0.5, 1 / 1.3, 2.0):
        out = ref.phase_vocoder(A, 17, rate, M, 0.3)
        i0, _ = ref.positions(17, rate, 13)
        assert np.array_equal(out, ref.angle_of(ref.q(A[..., i0]))), rate
    never = ref.phase_vocoder(A, 17, 0.5, np.ones_like(A), 0.3)
    assert np.array_equal(never, ref.phase_vocoder(A, 17, 0.5)) and np.array_equal(never, ref.phase_vocoder(A, 17, 0.5, M, 0.0))
    nan = ref.phase_vocoder(A, 17, 0.5, np.full_like(A, np.nan), 0.3)              # a NaN magnitude does not reset
    assert np.array_equal(nan, never)


def test_ref_resumes_from_the_analysis_phase_after_a_reset():
    A = np.linspace(-3, 3, 12).astype(np.float32)[None]
    M = np.ones_like(A)
    M[0, 4:7] = 0.0
    out = ref.phase_vocoder(A, 24, 0.5, M, 0.3)
    qA = ref.q(A)[0].astype(np.int64)
    # output frames 8 .. 13 sit on source frames 4 .. 6: reset; frame 14 resumes from q(A[6]) plus the advance measured at frame 13
    assert np.array_equal(out[0, 8:14], ref.angle_of(ref.q(A[0, [4, 4, 5, 5, 6, 6]])))
    assert out[0, 14] == ref.angle_of(np.uint32((qA[6] + qA[7] - qA[6]) % 2 ** 32))
    assert out[0, 15] == ref.angle_of(np.uint32((qA[7] + qA[8] - qA[7]) % 2 ** 32))


def test_ref_consistency_of_a_consistent_spectrogram_is_zero():
    rs = np.random.RandomState(4)
    t = np.arange(8 * 40, dtype=np.float64)
    x = np.stack([sum(rs.uniform(0.2, 1.0) * np.cos(2 * np.pi * k * t / 32 + rs.uniform(0, 2 * np.pi)) for k in (3, 5, 9)) for _ in range(2)])
    S = ref.stft64(x, 32, 8)
    assert S.shape == (2, 16, 41)
    c = ref.consistency64(np.log1p(np.abs(S)), 32, 8, phase=np.angle(S))
    # tones at bin centres have no DC wherever a frame sees them alone; only the reflected edge frames lose something with the DC row
    print(f"\nconsistency64 of a consistent spectrogram: SC {c['spectral_convergence']:.3e}, LSD {c['lsd_db']:.3e} dB")
    assert c["n_frames"] == 41 - 4 and c["channels"] == 2 and c["spectral_convergence"] < 0.05
    z = ref.consistency64(np.log1p(np.abs(S)), 32, 8, phase=np.zeros(S.shape))
    assert z["spectral_convergence"] > 2 * c["spectral_convergence"] and z["lsd_db"] > c["lsd_db"]
    a = ref.istft64(S, 32, 8)
    again = ref.consistency64(np.log1p(np.abs(S)), 32, 8, audio=a)
    assert again == pytest.approx(c, rel=1e-9)                                      # (expm1(log1p m) is m to a rounding)


# ---- the input condition of the GPU ordering test, in float64 ---------------------------------------------------------------

@pytest.fixture(scope="module")
def melody():
    x = ref.melody()
    assert x.shape == (96000,) and x.dtype == np.float32
    return x[None]


@pytest.mark.parametrize("stretch", [1.5, 0.75])
def test_melody_vocoder_is_twice_as_consistent_as_zero_phase(melody, stretch):
    from phasegen.track import spectral_plan
    pl = spectral_plan(melody.shape[1], 128, 512, 32, stretch)
    logmag, ang = ref.analysis64(melody, pl.n_src, 2048, 512)
    assert logmag.shape == (1, 1024, pl.F_src)
    mag = ref.resample64(logmag, pl.F_out, 1.0 / stretch)
    zero = ref.consistency64(mag, 2048, 512, phase=np.zeros_like(mag))["spectral_convergence"]
    sc = {}
    for floor in (0.0, 0.01, 0.05):
        ph = ref.phase_vocoder(ang.astype(np.float32), pl.F_out, 1.0 / stretch, logmag.astype(np.float32), floor)
        sc[floor] = ref.consistency64(mag, 2048, 512, phase=ph)["spectral_convergence"]
    print(f"\nmelody, stretch {stretch}: SC zero {zero:.4f}; vocoder " + ", ".join(f"floor {k:g}: {v:.4f}" for k, v in sc.items()))
    assert 0.85 < zero < 0.95
    for floor in (0.01, 0.05):
        assert sc[floor] < 0.5 * zero, (floor, sc[floor], zero)
    assert sc[0.05] < sc[0.0]                                                       # the reset helps
