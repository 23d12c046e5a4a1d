"""CPU: pg_formant_shift's host side (include/phasegen.h) -- symbols and struct layout, the error table in its order, the basis
table against the float64 formula, the properties of the smoother the header quotes, the Python surface -- and the comparison the
GPU module uses (tests/_formant_ref.py): it accepts the sequential float32 stand-in and rejects six planted faults.  The last test
holds the REFERENCE to the quality the estimator was chosen for, on idealised vowels: a condition on ref64, not a tolerance for
the kernel."""
import ctypes
import inspect
import math

import numpy as np
import pytest

import _formant_ref as fref


def _args(_lib, **kw):
    a = _lib.FormantArgs()
    a.n_ch, a.bins, a.F, a.m_ch_rows, a.order, a.hold, a.iters = 2, 40, 19, 40, 5, 3, 2
    a.ratio, a.eps = 1.25, 0.01
    a.M, a.basis, a.env, a.out = 4096, 8192, 12288, 16384           # never dereferenced: every call below stops before a launch
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_symbols_and_struct_layout():
    from phasegen import _lib
    lib = _lib.load()
    for name in ("pg_formant_shift", "pg_formant_basis", "pg_formant_basis_elems"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    A = _lib.FormantArgs
    assert ctypes.sizeof(A) == 80
    assert [f for f, _ in A._fields_] == ["n_ch", "bins", "F", "m_ch_rows", "order", "hold", "iters", "_pad0", "ratio", "eps", "_pad1",
                                           "M", "basis", "env", "out"]
    assert (A.ratio.offset, A.eps.offset, A.M.offset, A.out.offset) == (32, 40, 48, 72)
    assert not [f for f, t in A._fields_ if t is ctypes.c_int64]    # sizes are int32 and the channel stride counts rows
    assert lib.pg_formant_basis_elems(1024, 64) == 1024 * 64 + 64 and lib.pg_formant_basis_elems(5, 1) == 6
    for bins, order in ((0, 1), (4097, 4), (8, 0), (8, 9), (100, 65), (-1, -1)):
        assert lib.pg_formant_basis_elems(bins, order) == _lib.ERR_SHAPE, (bins, order)
    assert lib.pg_version() == 400


def test_argument_errors_are_reported_before_any_launch_and_in_order():
    from phasegen import _lib
    lib = _lib.load()
    assert lib.pg_formant_shift(None, None) == _lib.ERR_NULL

    def code(**kw):
        rc = lib.pg_formant_shift(ctypes.byref(_args(_lib, **kw)), None)
        return rc, lib.pg_last_error_string()

    null = [dict(M=None), dict(basis=None), dict(env=None, out=None)]
    shape = ([{k: bad} for k in ("n_ch", "bins", "F") for bad in (0, -3)]
             + [dict(bins=4097, m_ch_rows=5000), dict(m_ch_rows=39), dict(m_ch_rows=0)]
             + [dict(order=bad) for bad in (0, -1, 41, 65)] + [dict(bins=100, m_ch_rows=100, order=65)]
             + [dict(hold=bad) for bad in (-1, 65, 1 << 20)] + [dict(iters=bad) for bad in (-1, 17)]
             + [dict(ratio=bad) for bad in (0.0, 0.2499, 4.0001, -1.0, float("inf"), float("nan"))]
             + [dict(eps=bad) for bad in (0.0, -0.01, float("inf"), float("nan"))]
             + [dict(n_ch=1 << 30, m_ch_rows=(1 << 31) - 1, F=(1 << 31) - 1)])
    align = [{k: 4096 + off} for k in ("M", "basis", "env", "out") for off in (1, 2, 3)]
    for cases, want, word in ((null, _lib.ERR_NULL, b"required"), (shape, _lib.ERR_SHAPE, b""), (align, _lib.ERR_ALIGN, b"misaligned")):
        for kw in cases:
            rc, msg = code(**kw)
            assert rc == want and msg.startswith(b"formant_shift: ") and word in msg, (kw, rc, msg)
    # the order NULL, SHAPE, ALIGN decides what a doubly bad call reports
    assert code(M=None, bins=0, out=4097)[0] == _lib.ERR_NULL
    assert code(order=0, out=4097)[0] == _lib.ERR_SHAPE
    assert b"m_ch_rows" in code(m_ch_rows=39)[1] and b"order" in code(order=41)[1] and b"hold" in code(hold=65)[1]
    assert b"iters" in code(iters=17)[1] and b"ratio" in code(ratio=5.0)[1] and b"eps" in code(eps=0.0)[1] and b"2^62" in code(**shape[-1])[1]
    # one of env and out is enough, either one
    for kw in (dict(env=None), dict(out=None)):
        assert code(bins=0, **kw)[0] == _lib.ERR_SHAPE
    buf = np.empty(8, np.float32)
    assert lib.pg_formant_basis(None, 4, 1) == _lib.ERR_NULL
    for bins, order in ((0, 1), (4, 5), (4097, 1), (70, 65)):
        assert lib.pg_formant_basis(buf.ctypes.data_as(ctypes.c_void_p), bins, order) == _lib.ERR_SHAPE


def test_basis_is_the_double_formula_rounded_once():
    from phasegen import ops
    for bins, order in ((1, 1), (5, 1), (5, 5), (40, 5), (40, 40), (1024, 64), (4096, 64), (1000, 33)):
        got = ops.formant_basis_host(bins, order)
        T = np.array([[math.cos(math.pi * q * (k + 0.5) / bins) for k in range(bins)] for q in range(order)], np.float64)
        s = np.array([(1.0 if q == 0 else 2.0) / bins * 0.5 * (1.0 + math.cos(math.pi * q / order)) for q in range(order)], np.float64)
        want = np.concatenate([T.reshape(-1), s]).astype(np.float32)
        assert got.dtype == np.float32 and got.shape == (order * bins + order,)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (bins, order)
        assert np.array_equal(want.view(np.uint32), fref.basis32(bins, order).view(np.uint32))
    with pytest.raises(RuntimeError):
        ops.formant_basis_host(8, 9)


@pytest.mark.parametrize("order", (1, 5, 32, 64))
def test_the_smoother_preserves_constants_and_does_not_amplify(order):
    """float64: the rows of S = T' diag(s) T sum to one within 1e-12 and its infinity norm is at most 1.05 (Hann lifter; a rectangular
    one reaches 2.4 .. 2.9, which the iterations would turn into amplified rounding)"""
    for bins in (64, 1024):
        T, s = fref.basis64(bins, order)
        S = T.T @ (s[:, None] * T)
        assert np.abs(S.sum(axis=1) - 1.0).max() <= 1e-12, (bins, order)
        assert np.abs(S).sum(axis=1).max() <= 1.05, (bins, order, np.abs(S).sum(axis=1).max())
    if order >= 32:
        c = np.where(np.arange(order) == 0, 1.0 / 1024, 2.0 / 1024)
        R = T.T @ (c[:, None] * T)
        assert np.abs(R).sum(axis=1).max() > 2.0                      # what the lifter is there for


def _plane(seed, shape, top=6.0):
    rs = np.random.RandomState(seed)
    M = rs.uniform(0.0, top, shape).astype(np.float32)
    M[rs.uniform(size=shape) < 0.1] = 0.0
    return M


def test_the_comparison_accepts_the_stand_in_and_rejects_planted_faults():
    bins, order, hold, iters, ratio, eps = 96, 24, 4, 2, 2.0 ** (4.0 / 12.0), 0.01
    M = _plane(1, (2, bins, 9))
    M[1, :, 4] = 0.0                                                  # a silent frame
    basis = fref.basis32(bins, order)
    ref, thr = fref.thresholds(M, basis, order, hold, iters, ratio, eps)
    assert 0.0 < thr[2] < 64.0 and 0.0 < thr[3] < 64.0, thr           # seq32 itself is a few units of 2^-24 of the frame's peak
    env, out = fref.seq32(M, basis, order, hold, iters, ratio, eps)
    assert fref.accepted(env, out, ref, thr)[0]
    assert not env[1, :, 4].any() and not out[1, :, 4].any()
    for fault in fref.FAULTS:
        fe, fo = fref.seq32(M, basis, order, hold, iters, ratio, eps, fault=fault)
        ok, r = fref.accepted(fe, fo, ref, thr)
        assert not ok, (fault, r, thr)
    dirty = env.copy()
    dirty[1, 3, 4] = 1e-30                                            # a silent frame must be EXACTLY zero
    assert not fref.accepted(dirty, out, ref, thr)[0]
    # ratio 1.0 copies, a zero stays a zero, a plane constant along frequency is its own envelope
    e1, o1 = fref.seq32(M, basis, order, hold, iters, 1.0, eps)
    assert np.array_equal(o1.view(np.uint32), M.view(np.uint32))
    assert np.array_equal(fref.ref64(M, basis, order, hold, iters, 1.0, eps)[1], M.astype(np.float64))
    assert not out[M == 0.0].any() and not np.signbit(out[M == 0.0]).any()
    flat = np.broadcast_to(np.float32([0.5, 3.0, 80.0])[None, None, :], (1, bins, 3)).copy()
    assert np.abs(fref.ref64(flat, basis, order, hold, iters, 1.0, eps)[0] - flat).max() <= 1e-5 * 80.0


def test_python_surface_and_the_earlier_option_tiers():
    from phasegen import ops, track
    p = inspect.signature(ops.formant_shift).parameters
    assert list(p) == ["logmag", "ratio", "order", "hold", "iters", "eps", "return_env", "out"]
    assert [p[k].default for k in list(p)[2:]] == [64, 16, 2, 0.01, False, None]
    assert list(inspect.signature(ops.formant_basis_host).parameters) == ["bins", "order"]
    assert (track.FORMANT_ORDER, track.FORMANT_HOLD, track.FORMANT_ITERS, track.FORMANT_EPS) == (64, 16, 2, 0.01)
    assert track.FORMANTS == (None, "keep")
    # the earlier tiers are what existing callers compare; the new option has a tier of its own
    assert track.reconstruct_track.options == {"join": "waveform", "stretch": 1.0}
    assert track.reconstruct_track.later_options == {"link_channels": False} and track.reconstruct_track.newer_options == {"transients": None}
    assert track.reconstruct_track.newest_options == {"formant_semitones": 0.0}
    assert track.evaluate_stretch.options == {} and track.evaluate_stretch.later_options == {"link_channels": False}
    assert track.evaluate_stretch.newer_options == {"transients": None} and track.evaluate_stretch.newest_options == {"formant_semitones": 0.0}
    assert track.evaluate_track.newer_options == {} and track.evaluate_track.newest_options == {}
    assert list(inspect.signature(track.reconstruct_track).parameters)[-2:] == ["phase", "normalize"]
    p = inspect.signature(track.pitch_shift).parameters
    assert p["formants"].default is None and p["formants"].kind is inspect.Parameter.KEYWORD_ONLY and list(p)[-1] == "formants"
    with pytest.raises(ValueError):
        ops.formant_shift(None, 1.0)


def test_bad_combinations_are_refused_before_any_device_work():
    from phasegen import track
    x = np.zeros(1000, np.float32)
    small = dict(n_fft=32, hop_length=8, frames=24, overlap_frames=4)
    for kw in (dict(), dict(join="waveform")):
        with pytest.raises(ValueError, match="needs join='spectral'"):
            track.reconstruct_track(None, x, phase="zero", formant_semitones=3.0, **kw, **small)
    for bad in (float("nan"), 25.0, -24.5, float("inf")):
        with pytest.raises(ValueError, match="formant_semitones must be within"):
            track.reconstruct_track(None, x, phase="zero", join="spectral", formant_semitones=bad, **small)
        with pytest.raises(ValueError, match="formant_semitones must be within"):
            track.evaluate_stretch(None, x, 1.5, phases=("zero",), formant_semitones=bad, **small)
    for bad in ("Keep", True, 1, ""):
        with pytest.raises(ValueError, match="formants must be None or 'keep'"):
            track.pitch_shift(None, x, 4.0, phase="zero", formants=bad, **small)
    with pytest.raises(TypeError):
        track.pitch_shift(None, x, 4.0, 32, 8, 24, 4, None, None, 16000, "kaiser_best", 64, "zero", True, False, None, "keep")   # keyword only


def test_the_reference_halves_the_envelope_error_on_idealised_vowels():
    """Harmonic combs at four pitches under four Lorentzian formants, 1024 bins at 16 kHz, five shifts: the rms dB error of the
    harmonics as they will be PLAYED against the true envelope (300 Hz .. 4 kHz, median removed), without correction and with
    ref64's at the defaults.  Every one of the 20 rows must come out at no more than half its uncorrected error."""
    from phasegen import track
    order, hold, iters, eps = track.FORMANT_ORDER, track.FORMANT_HOLD, track.FORMANT_ITERS, track.FORMANT_EPS
    basis = fref.basis32(1024, order)
    rows = []
    for f0 in fref.F0S:
        frame = fref.vowel_frame(f0)
        for st in fref.SHIFTS:
            r = 2.0 ** (st / 12.0)                                   # pitch_shift(st, formants="keep") corrects with ratio 2^(st / 12)
            out = fref.ref64(frame[None, :, None], basis, order, hold, iters, r, eps)[1][0, :, 0]
            rows.append((f0, st, fref.harmonic_error_db(frame, f0, r), fref.harmonic_error_db(out, f0, r)))
    for f0, st, raw, fixed in rows:
        print(f"f0 {f0:5.0f} Hz  {st:+5.1f} st   uncorrected {raw:5.2f} dB   corrected {fixed:5.2f} dB   ratio {fixed / raw:4.2f}")
    print(f"mean uncorrected {np.mean([r[2] for r in rows]):.2f} dB, corrected {np.mean([r[3] for r in rows]):.2f} dB")
    assert len(rows) == 20
    for f0, st, raw, fixed in rows:
        assert fixed <= 0.5 * raw, (f0, st, raw, fixed)
