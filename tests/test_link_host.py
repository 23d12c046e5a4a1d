"""CPU: the host half of channel-linked phase locking (pg_phase_lock_linked, phasegen.ops.phase_lock_linked, phasegen.track
link_channels): the exported symbols and the struct, the workspace query, every argument error in the documented order (validation
runs before any launch), the Python surface, the combinations refused before any device work, properties of the numpy restatement
(tests/_link_ref.py), and -- in float64 -- what linking buys on a stereo signal.

The stereo condition.  On _link_ref.stereo_melody (6 s at 16 kHz, two channels, every note at a pan position and an inter-channel
delay of its own) the float64 chain gives, at n_fft 512 / hop 128 with the project's own analysis (the channels' moments) and the
floor 0.2: per-channel SC / SC of the channel mean against the mean's magnitudes / rms error of the inter-channel phase difference

    stretch   independent (pg_phase_lock per channel)   linked to the channel mean
    1.5       0.0662 / 0.3194 / 1.373 rad               0.0818 / 0.0715 / 6.4e-8 rad
    0.8       0.0561 / 0.2704 / 1.643 rad               0.0702 / 0.0570 / 6.1e-8 rad

(test_linking_keeps_the_mid_signal_and_the_phase_differences prints them), so "the linked mid SC is below half the independent one"
holds with room (ratios 0.224 and 0.211), and the phase difference is kept to the rounding of the fp32 output (half an ulp of a
value below pi is 1.2e-7 rad; the rms over two roundings stays below that)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import _link_ref as kref
import _lock_ref as lref
import _vocoder_ref as ref


# ---- the C entry point ---------------------------------------------------------------------------------------------------

def test_symbols_are_exported_and_listed():
    from phasegen import _lib
    lib = _lib.load()
    for name in ("pg_phase_lock_linked", "pg_workspace_bytes_phase_lock_linked"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    assert _lib.SYMBOLS["pg_workspace_bytes_phase_lock_linked"][0] is ctypes.c_int64
    assert lib.pg_version() == 400                                                  # additive within ABI 0.4


def test_struct_layout():
    from phasegen import _lib
    A = _lib.PhaseLockLinkedArgs
    assert ctypes.sizeof(A) == 96
    assert (A.n_ch.offset, A.bins.offset, A.F_src.offset, A.F_out.offset, A.src_per_out.offset, A.reset_below.offset) == (0, 4, 8, 16, 24, 32)
    assert (A.A.offset, A.a_stride.offset, A.Aref.offset, A.Mref.offset, A.out.offset) == (40, 48, 56, 64, 72)
    assert (A.workspace.offset, A.workspace_bytes.offset) == (80, 88)
    h = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "phasegen.h")).read()
    assert re.search(r"\}\s*pg_phase_lock_linked_args;\s*/\*\s*96 bytes\s*\*/", h)


def _args(_lib):
    """2 channels of 5 bins, 19 source frames -> 25 output frames; pointers are fake and never dereferenced."""
    a = _lib.PhaseLockLinkedArgs()
    a.n_ch, a.bins, a.F_src, a.F_out, a.src_per_out, a.reset_below = 2, 5, 19, 25, 0.75, 0.05
    a.A = a.Aref = a.Mref = a.out = 4096
    a.a_stride = 5 * 19
    a.workspace, a.workspace_bytes = 4096, 1 << 20
    return a


def test_workspace_query():
    """A host function of bins and F_out alone: one channel's worth, 12 bytes per bin and chunk, whatever n_ch."""
    from phasegen import _lib, ops
    lib = _lib.load()
    q = lib.pg_workspace_bytes_phase_lock_linked
    assert q(None) == _lib.ERR_NULL
    L = ops.PHASE_LOCK_CHUNK
    last = 0
    for F_out in (1, 2, L - 1, L, L + 1, 3 * L + 5, 10 ** 6, 10 ** 9):
        got = []
        for n_ch in (1, 2, 7):
            a = _args(_lib)
            a.n_ch, a.F_out = n_ch, F_out
            a.A = a.Aref = a.Mref = a.out = a.workspace = None                      # the query looks at no pointer
            got.append(q(ctypes.byref(a)))
        assert got[0] == got[1] == got[2] == 12 * 5 * -(-F_out // L) and got[0] >= last > -1, (F_out, got)
        last = got[0]
        one = _lib.PhaseLockArgs()                                                  # pg_phase_lock's for ONE channel
        one.n_ch, one.bins, one.F_src, one.F_out = 1, 5, 19, F_out
        assert lib.pg_workspace_bytes_phase_lock(ctypes.byref(one)) == got[0]
    for bins in (1, 1024, 4096):
        a = _args(_lib)
        a.bins, a.F_out = bins, 97
        assert q(ctypes.byref(a)) == 12 * bins * 4
    for field, bad in (("n_ch", 0), ("n_ch", -1), ("bins", 0), ("F_out", 0), ("bins", 4097), ("F_out", -1)):
        a = _args(_lib)
        setattr(a, field, bad)
        assert q(ctypes.byref(a)) == _lib.ERR_SHAPE, (field, bad)
    a = _args(_lib)
    a.n_ch, a.F_out = 1 << 20, 1 << 50                                              # more (channel, chunk) pairs than a grid holds
    assert q(ctypes.byref(a)) == _lib.ERR_SHAPE


def test_argument_errors_are_reported_before_any_launch_and_in_order():
    """NULL before shapes before alignment before the workspace: each class alone, then every pair of classes in one call."""
    from phasegen import _lib
    lib = _lib.load()
    f = lib.pg_phase_lock_linked
    assert f(None, None) == _lib.ERR_NULL

    def code(**fields):
        a = _args(_lib)
        for k, v in fields.items():
            setattr(a, k, v)
        rc = f(ctypes.byref(a), None)
        msg = lib.pg_last_error_string()
        assert rc != 0 and msg.startswith(b"phase_lock_linked: "), (fields, rc, msg)
        return rc, msg

    null = [dict(A=None), dict(Aref=None), dict(Mref=None), dict(out=None)]
    shape = ([{k: bad} for k in ("n_ch", "bins", "F_src", "F_out") for bad in (0, -3)] + [dict(bins=4097, a_stride=4097 * 19)]
             + [dict(src_per_out=bad) for bad in (0.0, -0.5, float("inf"), float("-inf"), float("nan"))]
             + [dict(reset_below=bad) for bad in (-1e-30, -1.0, float("inf"), float("-inf"), float("nan"))]
             + [dict(a_stride=5 * 19 - 1), dict(n_ch=1 << 30, bins=4096, F_out=1 << 62, a_stride=4096 * 19)])
    align = [{k: 4096 + off} for k in ("A", "Aref", "Mref", "out", "workspace") for off in (1, 2, 3)]
    need = lib.pg_workspace_bytes_phase_lock_linked(ctypes.byref(_args(_lib)))
    assert need == 12 * 5
    work = [dict(workspace=None), dict(workspace_bytes=need - 1), dict(workspace_bytes=0), dict(workspace_bytes=-1)]
    classes = ((null, _lib.ERR_NULL, b"required"), (shape, _lib.ERR_SHAPE, b""), (align, _lib.ERR_ALIGN, b"misaligned"),
               (work, _lib.ERR_WORKSPACE, b"workspace"))
    for cases, want, word in classes:
        for c in cases:
            rc, msg = code(**c)
            assert rc == want and word in msg, (c, rc, msg)
    assert b"4096 bins" in code(bins=4097, a_stride=4097 * 19)[1] and b"2^62" in code(**shape[-1])[1] and b"a_stride" in code(a_stride=94)[1]
    for i, (first, want, _) in enumerate(classes):                                  # the earlier class wins
        for later, _, _ in classes[i + 1:]:
            for c1 in first[:4]:
                for c2 in later[:4]:
                    if set(c1) & set(c2):
                        continue
                    assert code(**c1, **c2)[0] == want, (c1, c2)
    a = _args(_lib)                                                                 # a single channel: its stride is still checked
    a.n_ch, a.a_stride = 1, 94
    assert f(ctypes.byref(a), None) == _lib.ERR_SHAPE


# ---- the Python surface --------------------------------------------------------------------------------------------------

def test_python_surface():
    """Signatures only (the calls need a GPU), and what earlier features pinned stays as it was."""
    from phasegen import ops, track
    p = inspect.signature(ops.phase_lock_linked).parameters
    assert list(p) == ["angle", "ref_angle", "ref_logmag", "F_out", "src_per_out", "reset_below", "out"]
    assert (p["src_per_out"].default, p["reset_below"].default, p["out"].default) == (1.0, 0.0, None)
    assert list(inspect.signature(ops.phase_lock).parameters) == ["angle", "F_out", "src_per_out", "logmag", "reset_below", "out"]
    assert track.reconstruct_track.options == {"join": "waveform", "stretch": 1.0}
    assert track.reconstruct_track.later_options == {"link_channels": False}
    assert track.evaluate_stretch.options == {} and track.evaluate_stretch.later_options == {"link_channels": False}
    assert track.evaluate_track.options == {"join": "waveform"} and track.evaluate_track.later_options == {"gl_init": "noise"}
    assert list(inspect.signature(track.reconstruct_track).parameters)[-2:] == ["phase", "normalize"]
    p = inspect.signature(track.evaluate_stretch).parameters
    assert list(p) == ["model", "audio", "stretch", "n_fft", "hop_length", "frames", "overlap_frames", "stats", "osr", "sr", "res_type",
                       "clip_batch", "phases", "reset_below", "floor", "return_audio"]
    assert p["phases"].default == ("unet", "vocoder", "zero")
    p = inspect.signature(track.pitch_shift).parameters
    assert list(p)[:3] == ["model", "audio", "semitones"] and p["link_channels"].default is False
    assert p["link_channels"].kind is inspect.Parameter.KEYWORD_ONLY
    assert track.STRETCH_PHASES == ("unet", "vocoder", "zero", "vocoder_locked", "spsi")
    assert track.VOCODER_PHASES == ("vocoder", "vocoder_locked") and track.GRID_PHASES == ("vocoder", "vocoder_locked", "spsi")
    assert track.PHASES == ("unet", "zero", "original", "griffinlim") and track.REPORT_PHASES == track.PHASES + ("spsi",)
    assert track.JOINS == ("waveform", "spectral") and track.GL_INITS == ("noise", "spsi")
    with pytest.raises(TypeError):
        track.evaluate_stretch(None, np.zeros((2, 1000), np.float32), 1.5, phases=("zero",), link_channel=True)      # an unknown keyword


def test_link_channels_is_refused_with_another_phase_or_join_before_any_device_work():
    from phasegen import track
    x = np.zeros((2, 1000), np.float32)
    small = dict(n_fft=32, hop_length=8, frames=24, overlap_frames=4)
    for kw in (dict(phase="vocoder", join="spectral"), dict(phase="zero", join="spectral", stretch=1.5), dict(phase="spsi", join="spectral"),
               dict(phase="original", join="spectral"), dict(phase="zero", join="waveform"), dict(phase="original")):
        with pytest.raises(ValueError, match="link_channels needs"):
            track.reconstruct_track(None, x, link_channels=True, **kw, **small)
    with pytest.raises(ValueError, match="needs join='spectral'"):                 # (the phase's own refusal comes first)
        track.reconstruct_track(None, x, phase="vocoder_locked", join="waveform", link_channels=True, **small)
    for phases in (("vocoder",), ("zero", "vocoder"), ("spsi",)):
        with pytest.raises(ValueError, match="link_channels needs"):
            track.evaluate_stretch(None, x, 1.5, phases=phases, link_channels=True, **small)
    with pytest.raises(ValueError, match="unknown phase"):
        track.evaluate_stretch(None, x, 1.5, phases=("vocoder_locked", "original"), link_channels=True, **small)
    for phase in ("vocoder", "zero", "spsi"):
        with pytest.raises(ValueError, match="link_channels needs"):
            track.pitch_shift(None, x, 5, phase=phase, link_channels=True, **small)


# ---- the restatement itself ----------------------------------------------------------------------------------------------

def _planes(seed, n_ch=3, bins=9, F_src=19):
    rs = np.random.RandomState(seed)
    A = rs.uniform(-np.pi, np.pi, (n_ch, bins, F_src)).astype(np.float32)
    M = rs.uniform(0, 1, (bins, F_src)).astype(np.float32)
    return A, M


def test_ref_a_channel_equal_to_the_reference_has_phase_locks_bits():
    A, M = _planes(1)
    for rate, floor in ((1.0, 0.4), (0.5, 0.0), (1 / 1.3, 0.4), (2.0, 0.4)):
        for c in range(3):
            got = kref.phase_lock_linked(A, A[c], M, 25, rate, floor)
            assert got.shape == (3, 9, 25) and got.dtype == np.float32
            assert np.array_equal(got[c], lref.phase_lock(A[c], 25, rate, M, floor)), (rate, c)
        one = kref.phase_lock_linked(A[1:2], A[1], M, 25, rate, floor)              # n_ch == 1 with A == Aref
        assert np.array_equal(one[0], lref.phase_lock(A[1], 25, rate, M, floor))
    assert not np.array_equal(kref.phase_lock_linked(A, A[0], M, 25, 0.5)[1], lref.phase_lock(A[1], 25, 0.5, M))


def test_ref_rate_one_returns_the_analysis_phase():
    A, M = _planes(2)
    for floor in (0.0, 0.5):
        got = kref.phase_lock_linked(A, A[2], M, 25, 1.0, floor)
        assert np.array_equal(got[..., :19], ref.angle_of(ref.q(A)))
        assert np.array_equal(got[..., 19:], np.repeat(got[..., 18:19], 6, -1))     # past the end the advance is zero


def test_ref_the_rotation_cancels_between_channels_and_a_channel_does_not_depend_on_the_others():
    A, M = _planes(3, n_ch=4, bins=40, F_src=30)
    Aref = np.random.RandomState(4).uniform(-np.pi, np.pi, M.shape).astype(np.float32)
    F_out = 35
    out = kref.phase_lock_linked(A, Aref, M, F_out, 1 / 1.3, 0.5)
    T = lref.phase_lock(Aref, F_out, 1 / 1.3, M, 0.5, return_rotation=True)[1]
    i0, _ = ref.positions(F_out, 1 / 1.3, 30)
    qa = ref.q(A)[..., i0]
    assert T.any() and np.array_equal(out, ref.angle_of(T[None] + qa))
    assert np.array_equal((T + qa[0]) - (T + qa[3]), qa[0] - qa[3])                  # in uint32, before the final rounding
    for c in range(4):
        assert np.array_equal(kref.phase_lock_linked(A[c:c + 1], Aref, M, F_out, 1 / 1.3, 0.5)[0], out[c])
    assert np.array_equal(kref.phase_lock_linked(A[::-1], Aref, M, F_out, 1 / 1.3, 0.5), out[::-1])


def test_ref_stereo_melody_is_what_the_issue_defines():
    x = kref.stereo_melody()
    assert x.shape == (2, 96000) and x.dtype == np.float32
    rs = np.random.RandomState(3)
    pans = []
    for _ in ref.NOTES:
        pans.append(rs.uniform(0.15, 0.85))
        assert 0 <= int(rs.randint(0, 12)) < 12
    # the first note alone sounds in [0.5 s, 1.0 s): the channels' energies there are in the ratio of its pan gains
    seg = x[:, 8800:15200].astype(np.float64)
    ratio = np.sqrt((seg[1] ** 2).sum() / (seg[0] ** 2).sum())
    assert abs(ratio - np.tan(pans[0] * np.pi / 2)) < 1e-3 * ratio
    assert not np.array_equal(x[0], x[1]) and np.abs(x).max() < 4.0


# ---- what linking buys, in float64 -----------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def stereo():
    return kref.stereo_melody()


@pytest.mark.parametrize("stretch", [1.5, 0.8])
def test_linking_keeps_the_mid_signal_and_the_phase_differences(stereo, stretch):
    """n_fft 512, hop 128, floor 0.2: the channel mean of the linked output is more than twice as consistent as that of the
    independently locked channels (the issue's prototype: ratios 0.22 and 0.21), and the inter-channel phase difference of the
    analysis survives to below 1e-5 rad where independent locking leaves more than 0.5 rad."""
    from phasegen.track import spectral_plan
    n_fft, hop, floor, spo = 512, 128, 0.2, 1.0 / stretch
    pl = spectral_plan(stereo.shape[1], 128, hop, 32, stretch)
    logmag, ang = kref.linked_analysis64(stereo, pl.n_src, n_fft, hop)
    mag = ref.resample64(logmag, pl.F_out, spo)                                     # (3, bins, F_out): L, R and the mid row
    A, M = ang.astype(np.float32), logmag.astype(np.float32)
    indep = lref.phase_lock(A[:2], pl.F_out, spo, M[:2], floor)
    linked = kref.phase_lock_linked(A[:2], A[2], M[2], pl.F_out, spo, floor)
    res = {}
    for name, ph in (("independent", indep), ("linked", linked)):
        sc = ref.consistency64(mag[:2], n_fft, hop, phase=ph)["spectral_convergence"]
        mid = kref.mid_consistency64(mag[2], n_fft, hop, phase=ph, logmag=mag[:2])["spectral_convergence"]
        res[name] = (sc, mid, kref.ipd_error(ph, A[:2], mag[:2], spo))
        print(f"\nstereo melody, {n_fft} / {hop}, stretch {stretch}, {name}: per-channel SC {sc:.4f}, mid SC {res[name][1]:.4f}, "
              f"rms IPD error {res[name][2]:.3e} rad")
    print(f"mid SC ratio linked / independent {res['linked'][1] / res['independent'][1]:.3f}")
    assert res["linked"][1] < 0.5 * res["independent"][1]
    assert res["linked"][2] < 1e-5 and res["independent"][2] > 0.5
