"""CPU: the host half of the spectral track join (pg_spec_clips, pg_phase_join, phasegen.track.spectral_plan): exported symbols,
struct layouts, every argument error (validation runs before any launch), the frame-grid plan for hand-computed cases, the pitch
ratio, and the float64 reference helper itself.  Nothing here needs a GPU."""
import ctypes
import inspect
import math

import numpy as np
import pytest

import _spectral_ref as ref


def test_symbols_are_exported_and_listed():
    from phasegen import _lib
    lib = _lib.load()
    for name in ("pg_spec_clips", "pg_phase_join"):
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
    assert lib.pg_version() == 400                                                  # additive within ABI 0.4


def test_struct_layouts():
    from phasegen import _lib
    A = _lib.SpecClipsArgs
    assert ctypes.sizeof(A) == 64
    assert (A.n_clips.offset, A.n_ch.offset, A.bins.offset, A.frames.offset, A.sf.offset) == (0, 4, 8, 12, 16)
    assert (A.F_src.offset, A.src_per_out.offset, A.P.offset, A.p_stride.offset, A.out.offset) == (24, 32, 40, 48, 56)
    B = _lib.PhaseJoinArgs
    assert ctypes.sizeof(B) == 72
    assert (B.n_clips.offset, B.n_ch.offset, B.bins.offset, B.frames.offset, B.sf.offset) == (0, 4, 8, 12, 16)
    assert (B.phi.offset, B.clip_stride.offset, B.ch_stride.offset, B.row_pitch.offset, B.out.offset, B.ramp.offset) == (24, 32, 40, 48, 56, 64)


def _sc_args(_lib):
    """3 clips of 8 frames, 5 apart, of a (2, 5, 19) plane; pointers are fake and never dereferenced."""
    a = _lib.SpecClipsArgs()
    a.n_clips, a.n_ch, a.bins, a.frames, a.sf, a.F_src, a.src_per_out = 3, 2, 5, 8, 5, 19, 0.8
    a.P = a.out = 4096
    a.p_stride = 5 * 19
    return a


def test_spec_clips_argument_errors_are_reported_before_any_launch():
    from phasegen import _lib
    lib = _lib.load()
    f = lib.pg_spec_clips
    assert f(None, None) == _lib.ERR_NULL
    for field in ("P", "out"):
        a = _sc_args(_lib)
        setattr(a, field, None)
        assert f(ctypes.byref(a), None) == _lib.ERR_NULL and b"required" in lib.pg_last_error_string(), field
    for field in ("n_clips", "n_ch", "bins", "frames", "F_src"):
        for bad in (0, -3):
            a = _sc_args(_lib)
            setattr(a, field, bad)
            assert f(ctypes.byref(a), None) == _lib.ERR_SHAPE and b"non-positive" in lib.pg_last_error_string(), (field, bad)
    for bad in (0, -1):
        a = _sc_args(_lib)
        a.sf = bad
        assert f(ctypes.byref(a), None) == _lib.ERR_SHAPE and b"sf" in lib.pg_last_error_string(), bad
    for bad in (0.0, -0.5, float("inf"), float("-inf"), float("nan")):
        a = _sc_args(_lib)
        a.src_per_out = bad
        assert f(ctypes.byref(a), None) == _lib.ERR_SHAPE and b"src_per_out" in lib.pg_last_error_string(), bad
    a = _sc_args(_lib)
    a.p_stride = 5 * 19 - 1
    assert f(ctypes.byref(a), None) == _lib.ERR_SHAPE and b"p_stride" in lib.pg_last_error_string()
    for field in ("P", "out"):
        for off in (1, 2, 3):
            a = _sc_args(_lib)
            setattr(a, field, 4096 + off)
            assert f(ctypes.byref(a), None) == _lib.ERR_ALIGN and b"misaligned" in lib.pg_last_error_string(), (field, off)


def _pj_args(_lib):
    """3 clips of 8 frames, 5 apart (Vf = 3), 2 channels of 5 bins, dense; pointers are fake and never dereferenced."""
    a = _lib.PhaseJoinArgs()
    a.n_clips, a.n_ch, a.bins, a.frames, a.sf = 3, 2, 5, 8, 5
    a.phi = a.out = a.ramp = 4096
    a.row_pitch, a.ch_stride, a.clip_stride = 8, 5 * 8, 2 * 5 * 8
    return a


def test_phase_join_argument_errors_are_reported_before_any_launch():
    from phasegen import _lib
    lib = _lib.load()
    f = lib.pg_phase_join
    assert f(None, None) == _lib.ERR_NULL
    for field in ("phi", "out", "ramp"):
        a = _pj_args(_lib)
        setattr(a, field, None)
        assert f(ctypes.byref(a), None) == _lib.ERR_NULL and b"required" in lib.pg_last_error_string(), field
    for field in ("n_clips", "n_ch", "bins", "frames"):
        for bad in (0, -3):
            a = _pj_args(_lib)
            setattr(a, field, bad)
            assert f(ctypes.byref(a), None) == _lib.ERR_SHAPE and b"non-positive" in lib.pg_last_error_string(), (field, bad)
    for bad in (0, -1, 8, 9):                                                       # sf < 1; Vf = frames - sf < 1
        a = _pj_args(_lib)
        a.sf = bad
        assert f(ctypes.byref(a), None) == _lib.ERR_SHAPE and b"sf" in lib.pg_last_error_string(), bad
    a = _pj_args(_lib)
    a.sf = 3                                                                        # 2 Vf = 10 > 8
    assert f(ctypes.byref(a), None) == _lib.ERR_SHAPE and b"overlap" in lib.pg_last_error_string()
    for field, bad in (("row_pitch", 7), ("ch_stride", 4 * 8 + 7), ("clip_stride", 4 * 8 + 7)):
        a = _pj_args(_lib)
        setattr(a, field, bad)
        assert f(ctypes.byref(a), None) == _lib.ERR_SHAPE and field.encode() in lib.pg_last_error_string(), field
    for field in ("phi", "out", "ramp"):
        for off in (1, 2, 3):
            a = _pj_args(_lib)
            setattr(a, field, 4096 + off)
            assert f(ctypes.byref(a), None) == _lib.ERR_ALIGN and b"misaligned" in lib.pg_last_error_string(), (field, off)


def test_spectral_plan_hand_computed():
    from phasegen.track import spectral_plan, track_plan
    # frames 24, hop 8, overlap 4: T = 184, step = 152 = 8 * 19, sf = 19, Vf = 5
    p = spectral_plan(100, 24, 8, 4)                                                # a_len <= T: one clip
    assert tuple(p) == (19, 5, 100, 1, 24, 25, 192)
    assert (p.sf, p.Vf, p.a_out, p.n_clips, p.F_out, p.F_src, p.n_src) == tuple(p)
    assert tuple(spectral_plan(184, 24, 8, 4)) == (19, 5, 184, 1, 24, 25, 192)      # a_len == T
    assert tuple(spectral_plan(185, 24, 8, 4)) == (19, 5, 185, 2, 43, 44, 344)
    assert tuple(spectral_plan(184 + 3 * 152, 24, 8, 4)) == (19, 5, 640, 4, 81, 82, 648)       # an exact multiple: no ragged tail
    assert tuple(spectral_plan(1000, 24, 8, 4)) == (19, 5, 1000, 7, 138, 139, 1104)           # 1 + ceil(816 / 152) = 7
    assert tuple(spectral_plan(1000, 24, 8, 4, 1.0)) == tuple(spectral_plan(1000, 24, 8, 4))
    # stretch 0.5: a_out 500 -> 1 + ceil(316 / 152) = 4 clips, F_out 81, F_src = floor(80 / 0.5) + 2 = 162
    assert tuple(spectral_plan(1000, 24, 8, 4, 0.5)) == (19, 5, 500, 4, 81, 162, 1288)
    # stretch 1.25: a_out 1250 -> 1 + ceil(1066 / 152) = 9 clips, F_out 176, F_src = floor(175 / 1.25) + 2 = 142
    assert tuple(spectral_plan(1000, 24, 8, 4, 1.25)) == (19, 5, 1250, 9, 176, 142, 1128)
    # stretch 4: a_out 4000 -> 1 + ceil(3816 / 152) = 27 clips, F_out 518, F_src = floor(517 / 4) + 2 = 131
    assert tuple(spectral_plan(1000, 24, 8, 4, 4)) == (19, 5, 4000, 27, 518, 131, 1040)
    assert tuple(spectral_plan(1000, 24, 8, 4, 0.25))[2:4] == (250, 2)
    # no overlap: neighbouring clips still share their edge frame
    assert tuple(spectral_plan(1000, 24, 8, 0)) == (23, 1, 1000, 6, 139, 140, 1112)
    assert tuple(spectral_plan(160000, 128, 512, 32)) == (95, 33, 160000, 3, 318, 319, 512 * 318)
    for a_len in (1, 100, 184, 185, 640, 1000, 4321):
        for stretch in (0.25, 0.5, 0.75, 1.0, 1.25, 1.5, 2.0, 3.3, 4.0):
            for ov in (0, 4, 11):
                if round(a_len * stretch) < 1:
                    continue
                p = spectral_plan(a_len, 24, 8, ov, stretch)
                T, step, n = track_plan(p.a_out, 24, 8, ov)
                assert step == 8 * p.sf and n == p.n_clips and p.F_out == (n - 1) * p.sf + 24
                assert 8 * (p.F_out - 1) >= p.a_out                                 # the ISTFT delivers every output sample
                assert p.F_src - 1 >= (p.F_out - 1) / stretch                       # the upper neighbour of every position exists
                assert p.F_src - 2 <= (p.F_out - 1) / stretch and p.n_src == 8 * (p.F_src - 1)
                assert p.Vf >= 1 and 2 * p.Vf <= 24 and p.sf + p.Vf == 24


def test_spectral_plan_errors():
    from phasegen.track import spectral_plan
    for bad in (0.2499, 4.001, 0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            spectral_plan(1000, 24, 8, 4, bad)
    with pytest.raises(ValueError):
        spectral_plan(1000, 24, 8, 12)                                              # track_plan's: 2 * 12 > 23
    with pytest.raises(ValueError):
        spectral_plan(1000, 24, 8, -1)
    with pytest.raises(ValueError):
        spectral_plan(1000, 100, 8, 8)                                              # frames the U-Net cannot concatenate
    with pytest.raises(ValueError):
        spectral_plan(0, 24, 8, 4)
    with pytest.raises(ValueError):
        spectral_plan(1, 24, 8, 4, 0.25)                                            # round(0.25) = 0 output samples


def test_pitch_ratio_and_its_error_in_cents():
    from phasegen.track import pitch_ratio
    assert pitch_ratio(12) == (2.0, 2) and pitch_ratio(0) == (1.0, 1) and pitch_ratio(-24)[1] == pytest.approx(0.25)
    worst = 0.0
    for s in range(-24, 25):
        stretch, q = pitch_ratio(s)
        assert q.denominator <= 1024 and 0.25 <= stretch <= 4.0
        worst = max(worst, abs(1200.0 * math.log2(float(q) / stretch)))
    assert worst <= 0.027
    for s in np.linspace(-24, 24, 4801):
        stretch, q = pitch_ratio(float(s))
        assert q.denominator <= 1024 and abs(1200.0 * math.log2(float(q) / stretch)) <= 0.85
    for bad in (24.01, -24.01, float("nan")):
        with pytest.raises(ValueError):
            pitch_ratio(bad)


def test_python_surface():
    """Signatures only (the calls need a GPU)."""
    from phasegen import ops, track
    p = inspect.signature(track.spectral_plan).parameters
    assert list(p) == ["a_len", "frames", "hop_length", "overlap_frames", "stretch"] and p["stretch"].default == 1.0
    # join / stretch are keyword-only options on top of the waveform-only calls' positional lists, which stay as they were
    assert track.reconstruct_track.options == {"join": "waveform", "stretch": 1.0}
    assert track.evaluate_track.options == {"join": "waveform"}
    assert list(inspect.signature(track.reconstruct_track).parameters)[-2:] == ["phase", "normalize"]
    assert list(inspect.signature(track.evaluate_track).parameters)[-1] == "return_audio"
    with pytest.raises(TypeError):
        track.reconstruct_track(None, np.zeros(1000, np.float32), 32, 8, 24, 4, phase="zero", joint="spectral")      # an unknown keyword
    p = inspect.signature(track.pitch_shift).parameters
    assert list(p)[:3] == ["model", "audio", "semitones"]
    assert list(inspect.signature(ops.spec_clips).parameters) == ["plane", "n_clips", "frames", "sf", "src_per_out", "out"]
    assert list(inspect.signature(ops.phase_join).parameters) == ["phi", "sf", "ramp", "out"]
    assert track.JOINS == ("waveform", "spectral")


def test_join_and_stretch_combinations_are_refused_before_any_device_work():
    from phasegen import track
    x = np.zeros(1000, np.float32)
    for kw in (dict(join="sideways"), dict(stretch=1.5), dict(join="waveform", stretch=0.5),
               dict(join="spectral", stretch=1.5, phase="original"), dict(join="spectral", phase="griffinlim")):
        with pytest.raises(ValueError):
            track.reconstruct_track(None, x, 32, 8, 24, 4, phase=kw.pop("phase", "zero"), **kw)
    with pytest.raises(ValueError):
        track.evaluate_track(None, x, 32, 8, 24, 4, phases=("zero", "griffinlim"), join="spectral")
    with pytest.raises(ValueError):
        track.evaluate_track(None, x, 32, 8, 24, 4, phases=("zero",), join="both")


# ---- the reference helper itself ----------------------------------------------------------------------------------------

def test_ref_ramp_is_pg_stitch_ramp():
    from phasegen import ops
    for V in (1, 3, 4, 33):
        assert np.array_equal(ref.ramp(V), ops.stitch_ramp_host(V))


def test_ref_gather_at_rate_one_is_a_copy():
    rs = np.random.RandomState(3)
    P = rs.standard_normal((2, 5, 19)).astype(np.float32)
    for fn in (ref.spec_clips, ref.spec_clips_f32):
        out = fn(P, 3, 8, 5, 1.0)
        assert out.shape == (3, 2, 5, 8)
        for k in range(3):
            assert np.array_equal(out[k], P[:, :, 5 * k:5 * k + 8])
        out = fn(P, 4, 8, 5, 1.0)                                                   # clip 3 covers frames 15 .. 22: clamped at 18
        assert np.array_equal(out[3, :, :, :4], P[:, :, 15:19]) and np.array_equal(out[3, :, :, 4:], np.repeat(P[:, :, 18:19], 4, 2))
    assert ref.spec_clips_f32(P, 3, 8, 5, 1.0).dtype == np.float32
    whole = ref.spec_clips_f32(P, 1, 19, 19, 1.0)
    assert np.array_equal(whole[0], P)


def test_ref_gather_interpolates_linearly():
    P = (np.arange(19, dtype=np.float32) * 2.0)[None, None, :] + np.zeros((2, 5, 1), np.float32)      # a ramp: exact in both forms
    out = ref.spec_clips(P, 3, 8, 5, 0.75)
    g = (np.arange(3)[:, None] * 5 + np.arange(8)[None, :]) * 0.75
    assert np.allclose(out[:, 0, 0], 2.0 * g, rtol=0, atol=1e-12)
    assert np.array_equal(ref.spec_clips_f32(P, 3, 8, 5, 0.75).astype(np.float64), out)
    rs = np.random.RandomState(4)
    Q = rs.standard_normal((2, 5, 19)).astype(np.float32)
    a, b = ref.spec_clips(Q, 3, 8, 5, 1.0 / 3.0), ref.spec_clips_f32(Q, 3, 8, 5, 1.0 / 3.0)
    assert np.abs(a - b).max() <= 4 * 2.0 ** -24 * np.abs(Q).max() * 2                    # three roundings of values below 2 max|Q|


def test_ref_join_of_identical_phases_returns_them():
    rs = np.random.RandomState(5)
    for frames, sf in ((8, 7), (8, 5), (8, 4)):
        n_clips = 4
        F_out = (n_clips - 1) * sf + frames
        track_phi = rs.uniform(-np.pi, np.pi, (2, 5, F_out))
        phi = np.stack([track_phi[:, :, k * sf:k * sf + frames] for k in range(n_clips)])
        out = ref.phase_join(phi, sf)
        assert out.shape == (2, 5, F_out)
        d = np.angle(np.exp(1j * (out - track_phi)))
        assert np.abs(d).max() <= 1e-12
        z, shared = ref.phase_join_z(phi, sf)
        assert shared.sum() == (n_clips - 1) * (frames - sf)
        assert np.array_equal(out[:, :, ~shared], track_phi[:, :, ~shared])                  # copies, unwrapped
        assert np.abs(np.abs(z) - 1.0).max() <= 2.0 ** -22                                   # a + b is within 2^-23 of 1


def test_ref_join_conditioning_of_a_cancelling_blend_and_reach_of_a_nan():
    phi = np.zeros((2, 1, 1, 4))
    phi[1, 0, 0, 0] = np.pi                                                         # lo = 0, hi = pi under equal weights: z = 0 to 1e-16
    phi[1, 0, 0, 1] = np.nan
    out = ref.phase_join(phi[:, :, :, :2], 1, np.array([0.5], np.float32))         # frames 2, sf 1, Vf 1
    assert out.shape == (1, 1, 3)
    z, shared = ref.phase_join_z(phi[:, :, :, :2], 1, np.array([0.5], np.float32))
    assert list(shared) == [False, True, False] and abs(z[0, 0, 1]) < 1e-15
    assert np.isnan(out[0, 0, 2]) and out[0, 0, 0] == 0.0                           # the NaN stays in the frames its clip covers
