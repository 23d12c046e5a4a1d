"""CPU: the host half of pitch detection -- pg_pitch_track's symbol, struct layout and error table in its order (validation runs
before any launch), the accuracy of the contract itself, measured on its numpy restatement (tests/_pitch_ref.py) alone, the rules
the contract states, and ``PitchCurve.correcting``.

Accuracy (16 kHz, window 1024, hop 256, lags 16 .. 320, theta 0.15).  Steady tones at 55 * 2^(k / 7.3) Hz up to 950 Hz in three
spectra (harmonics 1, 1/2, 1/4, 1/10; a weak fundamental 0.05, 1, 0.7, 0.5; a pure sine) with 1e-3 of noise, six frames each of the
steady part (the frames begin where the generator's 10 ms attack ends: inside the ramp a tone is not steady, and a frame that holds it
at 55 Hz, where the ramp is half a period, is 7.2 cents off): no estimate more than 50 cents off (no octave error), the largest error
at most 3 cents, every frame voiced.  Measured on 558 frames: 1.98 cents (harmonic), 2.39 (weak fundamental), 2.55 (sine, at 949 Hz,
where a period is 17 samples and the parabola through three of them carries the error).
float32 against float64: the same lag on every tone frame and on 60 frames of white noise, |cm32 - cm64| <= 1e-5 (measured: 4.7e-6),
white noise unvoiced everywhere (the smallest ap: 0.868)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import _pitch_ref as pref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL, SHAPE, ALIGN, UNSUPPORTED = -1, -2, -3, -4
NAN = float("nan")
SR, W, HOP, TAU_MIN, TAU_MAX, THETA = 16000, 1024, 256, 16, 320, 0.15
TINY = dict(hop=8, W=32, tau_min=2, tau_max=24)                   # the small shape of the rule tests (and of the GPU tests)


def _header_fields(struct):
    h = open(os.path.join(ROOT, "include", "phasegen.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), h, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            first, *more = decl.split(",")
            names.append(re.findall(r"(\w+)\s*$", first)[0])
            names.extend(m.strip() for m in more)
    return names


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


# ---- the C entry point -----------------------------------------------------------------------------------------------------

def test_symbol_and_struct_layout():
    from phasegen import _lib
    lib = _lib.load()
    assert "pg_pitch_track" in _lib.SYMBOLS and hasattr(lib, "pg_pitch_track")
    assert lib.pg_version() == 400                                                  # additive within ABI 0.4
    P = _lib.PitchTrackArgs
    assert ctypes.sizeof(P) == 64
    h = open(os.path.join(ROOT, "include", "phasegen.h")).read()
    assert re.search(r"\}\s*pg_pitch_track_args;\s*/\*\s*64 bytes\s*\*/", h)
    assert [f[0] for f in P._fields_] == _header_fields("pg_pitch_track_args")
    assert not any(t in (ctypes.c_int64, ctypes.c_double) for _, t in P._fields_)   # int32 sizes: nothing for the far-offset tables
    assert "workspace" not in dict(P._fields_)
    assert (P.hop.offset, P.window.offset, P.tau_min.offset, P.tau_max.offset, P.x_stride.offset, P.out_stride.offset) == (12, 16, 20, 24, 28, 32)
    assert (P.threshold.offset, P.x.offset, P.period.offset, P.ap.offset) == (36, 40, 48, 56)
    assert (_lib.PITCH_MIN_WINDOW, _lib.PITCH_MAX_WINDOW, _lib.PITCH_MIN_TAU, _lib.PITCH_MAX_TAU) == (4, 2048, 2, 1024)


def _good(_lib):
    a = _lib.PitchTrackArgs()
    a.n_sig, a.n_in, a.frames, a.hop, a.window, a.tau_min, a.tau_max, a.x_stride, a.out_stride = 2, 300, 7, 8, 32, 2, 24, 300, 7
    a.threshold = 0.15
    a.x = a.period = a.ap = 4096                                  # never dereferenced: every case below fails before the launch
    return a


def test_argument_errors_are_reported_before_any_launch_and_in_order():
    from phasegen import _lib
    lib = _lib.load()
    assert lib.pg_pitch_track(None, None) == NULL
    assert lib.pg_last_error_string().startswith(b"pitch_track: ")
    # (what is broken, expected code), in the documented order: each case also carries every fault that comes LATER in the order
    later = [({"ap": 0}, NULL), ({"out_stride": 6}, SHAPE), ({"tau_max": 1025}, UNSUPPORTED), ({"hop": 0}, SHAPE)]
    for k in range(len(later)):
        a = _good(_lib)
        for fields, _code in later[:k + 1]:
            for f, v in fields.items():
                setattr(a, f, v)
        assert lib.pg_pitch_track(ctypes.byref(a), None) == later[k][1], later[k]
        assert lib.pg_last_error_string().startswith(b"pitch_track: ")
    singles = [({"n_sig": 0}, SHAPE), ({"n_in": -1}, SHAPE), ({"frames": 0}, SHAPE), ({"hop": -3}, SHAPE),
               ({"window": 3}, UNSUPPORTED), ({"window": 2049}, UNSUPPORTED), ({"tau_min": 1}, UNSUPPORTED), ({"tau_min": 24}, UNSUPPORTED),
               ({"tau_min": 30}, UNSUPPORTED), ({"tau_max": 1025}, UNSUPPORTED), ({"tau_max": 2}, UNSUPPORTED),
               ({"x_stride": 299}, SHAPE), ({"out_stride": 6}, SHAPE), ({"x": 0}, NULL), ({"period": 0}, NULL), ({"ap": 0}, NULL)]
    for fields, code in singles:
        a = _good(_lib)
        for f, v in fields.items():
            setattr(a, f, v)
        assert lib.pg_pitch_track(ctypes.byref(a), None) == code, fields
        assert lib.pg_last_error_string().startswith(b"pitch_track: ")
    for fields in ({"window": 4}, {"window": 2048}, {"tau_min": 2, "tau_max": 3}, {"tau_min": 1023, "tau_max": 1024}):
        a = _good(_lib)
        for f, v in fields.items():
            setattr(a, f, v)
        a.ap = 0                                                  # the limits themselves pass on to the next rows
        assert lib.pg_pitch_track(ctypes.byref(a), None) == NULL, fields


def test_python_surface_without_a_gpu():
    import torch
    from phasegen import ops, track
    sig = inspect.signature(ops.pitch_track)
    assert list(sig.parameters) == ["x", "frames", "hop", "window", "tau_min", "tau_max", "threshold", "out"]
    assert [sig.parameters[n].default for n in list(sig.parameters)[1:]] == [None, 256, 1024, 16, 320, 0.15, None]
    assert ops.pitch_frames(1344) == 1 and ops.pitch_frames(1343) == 1 and ops.pitch_frames(1600) == 2 and ops.pitch_frames(10) == 1
    with pytest.raises(ValueError, match="pitch_track: expected a 1-D or 2-D float32 device tensor"):
        ops.pitch_track(torch.zeros(2000))
    d = inspect.signature(track.detect_pitch)
    assert list(d.parameters) == ["audio", "sr", "osr", "fmin", "fmax", "hop_length", "window", "threshold", "median", "res_type"]
    assert [p.default for p in list(d.parameters.values())[1:]] == [16000, None, 50.0, 1000.0, 256, 1024, 0.15, 5, "kaiser_best"]
    assert track.PitchTrack._fields == ("times", "f0", "voiced", "ap")
    assert track.pitch_lags(16000, 50.0, 1000.0) == (16, 320) and track.pitch_lags(44100, 10.0, 30000.0) == (2, 1024)
    for args in ((16000, 0.0, 100.0), (16000, 200.0, 100.0), (0, 50.0, 1000.0), (16000, 9000.0, 9500.0)):
        with pytest.raises(ValueError, match="detect_pitch: "):
            track.pitch_lags(*args)
    a = list(inspect.signature(track.autotune).parameters)
    assert a[:6] == ["model", "audio", "strength", "scale", "a4", "retune_ms"] and "return_curve" in a and "formants" in a
    assert inspect.signature(track.autotune).parameters["retune_ms"].default == 50.0
    with pytest.raises(ValueError, match="autotune: formants='keep' is not available"):
        track.autotune(None, np.zeros(4000, np.float32), phase="zero", formants="keep")


# ---- the accuracy of the contract, on the restatement alone ------------------------------------------------------------------

FRAMES = 6
N_TONE = (FRAMES - 1) * HOP + W + TAU_MAX
ATTACK = 160                                                      # the generator's 10 ms attack at 16 kHz
SPECTRA = {"harmonic": pref.SPECTRUM, "weak fundamental": pref.WEAK_FUNDAMENTAL, "sine": pref.SINE}


def tone_frequencies():
    f = [55.0 * 2.0 ** (k / 7.3) for k in range(64)]
    return [v for v in f if v <= 950.0]


@pytest.fixture(scope="module")
def tones():
    """every tone as one row, tracked once in float32 and once in float64 (shared, left unchanged)"""
    rows, f0 = [], []
    for name, spectrum in SPECTRA.items():
        for i, f in enumerate(tone_frequencies()):
            y, _ = pref.take([(f, (ATTACK + N_TONE) / SR)], SR, spectrum=spectrum, seed=1000 + i)
            rows.append(y[ATTACK:ATTACK + N_TONE])                # the steady part: the frames begin where the attack ends
            f0.append((name, f))
    x = np.stack(rows)
    r32 = pref.pitch_track(x, FRAMES, HOP, W, TAU_MIN, TAU_MAX, THETA, details=True)
    r64 = pref.pitch_track(x, FRAMES, HOP, W, TAU_MIN, TAU_MAX, THETA, dtype=np.float64, details=True)
    return x, f0, r32, r64


@pytest.fixture(scope="module")
def noise():
    x = np.random.RandomState(5).standard_normal((59) * HOP + W + TAU_MAX).astype(np.float32) * 0.3
    r32 = pref.pitch_track(x, 60, HOP, W, TAU_MIN, TAU_MAX, THETA, details=True)
    r64 = pref.pitch_track(x, 60, HOP, W, TAU_MIN, TAU_MAX, THETA, dtype=np.float64, details=True)
    return x, r32, r64


def test_steady_tones_are_tracked_within_three_cents_and_all_voiced(tones):
    _x, f0, (period, ap, _tau, _cm), _r64 = tones
    assert period.dtype == np.float32 and period.shape == (len(f0), FRAMES)
    worst = {}
    for (name, f), p, a in zip(f0, period, ap):
        err = np.abs(pref.cents(SR / p.astype(np.float64), f))
        worst[name] = max(worst.get(name, 0.0), float(err.max()))
        assert (err <= 50.0).all(), (name, f, err)                # no octave error
        assert (a < THETA).all(), (name, f, a)
    print(f"{period.size} frames of {len(tone_frequencies())} tones x 3 spectra: the largest error in cents is "
          + ", ".join(f"{v:.2f} ({k})" for k, v in worst.items()) + f"; the largest ap is {float(ap.max()):.3f}")
    assert max(worst.values()) <= 3.0, worst


def test_float32_picks_the_lags_of_float64(tones, noise):
    _x, _f0, r32, r64 = tones
    _n, n32, n64 = noise
    for what, a, b in (("tones", r32, r64), ("noise", n32, n64)):
        differ = int((a[2] != b[2]).sum())
        gap = float(np.abs(a[3].astype(np.float64) - b[3]).max())
        print(f"{what}: {differ} of {a[2].size} frames pick another lag in float32; max |cm32 - cm64| = {gap:.2e}")
        assert differ == 0 and (a[2] >= TAU_MIN).all()
        assert gap <= 1e-5
    print(f"white noise: the smallest ap is {float(n32[1].min()):.3f}")
    assert (n32[1] >= THETA).all() and (n64[1] >= THETA).all()   # unvoiced everywhere


# ---- the rules of the contract -------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def tiny_row():
    """the first row of the GPU tests: white noise with samples 100 .. 199 replaced by a sine of period 11.3 (both branches of the
    pick in one row)"""
    x = np.random.RandomState(21).standard_normal(300).astype(np.float32) * 0.5
    x[100:200] = np.sin(2 * np.pi * np.arange(100, 200) / 11.3).astype(np.float32)
    return x


def tiny(x, frames=40, theta=THETA, **kw):
    return pref.pitch_track(x, frames, TINY["hop"], TINY["W"], TINY["tau_min"], TINY["tau_max"], theta, **kw)


def test_the_tiny_row_takes_both_branches(tiny_row):
    period, ap, tau, cm = tiny(tiny_row, details=True)
    print(f"tiny row: ap runs from {float(ap.min()):.3f} to {float(ap.max()):.3f}")
    assert ap.min() < 0.05 and (ap < THETA).any() and (ap >= THETA).any() and ap.max() == 1.0
    assert (period[-2:] == TINY["tau_min"]).all() and (ap[-2:] == 1.0).all()         # frames 38 and 39 begin past the row: all zeros
    voiced = ap < 0.05
    assert np.abs(period[voiced] - 11.3).max() < 0.2


def test_silence_and_a_constant_row_give_tau_min_and_one():
    for row in (np.zeros(300, np.float32), np.full(300, 1e-25, np.float32)):       # (1e-25: the squares underflow)
        period, ap = tiny(row, frames=40)
        assert (period == TINY["tau_min"]).all() and (ap == 1.0).all()
    period, ap = tiny(np.full(300, 0.37, np.float32), frames=30)                   # (the last frames see the row's edge: a step to zero)
    whole = np.arange(30) * TINY["hop"] + TINY["W"] + TINY["tau_max"] <= 300
    assert (period[whole] == TINY["tau_min"]).all() and (ap[whole] == 1.0).all() and whole.sum() >= 20


def test_a_power_of_two_keeps_the_bits_and_1e25_overflows(tiny_row):
    period, ap = tiny(tiny_row)
    for e in (40, -40):
        p2, a2 = tiny(tiny_row * np.float32(2.0 ** e))
        assert bits_equal(p2, period) and bits_equal(a2, ap), e
    with np.errstate(over="ignore"):
        p3, a3 = tiny(tiny_row * np.float32(1e25))
    inside = np.arange(40) * TINY["hop"] < 300
    assert np.isnan(p3[inside]).all() and np.isnan(a3[inside]).all()
    assert (p3[~inside] == TINY["tau_min"]).all() and (a3[~inside] == 1.0).all()
    assert (p3[inside].view(np.int32) == 0x7fc00000).all()       # quiet, positive


@pytest.mark.parametrize("i", [0, 55, 56, 199, 299])
def test_a_nan_reaches_exactly_the_frames_that_hold_it(tiny_row, i):
    period, ap = tiny(tiny_row)
    x = tiny_row.copy()
    x[i] = NAN
    p2, a2 = tiny(x)
    hit = pref.cone(i, 40, TINY["hop"], TINY["W"], TINY["tau_max"])
    assert hit.any() and not hit.all()
    assert np.array_equal(np.isnan(p2), hit) and np.array_equal(np.isnan(a2), hit)
    assert bits_equal(p2[~hit], period[~hit]) and bits_equal(a2[~hit], ap[~hit])


def test_a_nan_threshold_takes_the_fallback_and_two_takes_the_first_walk_down(tiny_row):
    lo, hi = TINY["tau_min"], TINY["tau_max"]
    _p, ap_nan, tau_nan, cm = tiny(tiny_row, theta=NAN, details=True)
    _p, ap_0, tau_0, _cm = tiny(tiny_row, theta=0.0, details=True)
    for f in range(40):
        A = cm[f, lo:hi]
        assert tau_nan[f] == lo + int(np.argmin(A)) and ap_nan[f] == A.min()
    assert np.array_equal(tau_0, tau_nan)                         # cm >= 0: nothing is below 0 either
    _p, _a, tau_2, _cm = tiny(tiny_row, theta=2.0, details=True)
    stepped = 0
    for f in range(40):
        t = lo
        if not cm[f, lo] < 2.0:                                   # (cm may pass 2 where d grows faster than its mean)
            continue
        while t + 1 <= hi - 1 and cm[f, t + 1] < cm[f, t]:
            t += 1
        assert tau_2[f] == t
        stepped += t > lo
    assert stepped >= 5


# ---- PitchCurve.correcting -----------------------------------------------------------------------------------------------------

def _track(f0, voiced=None, hop=256, window=1024, sr=16000):
    from phasegen import track
    f0 = np.asarray(f0, np.float64)
    voiced = np.ones(f0.shape[0], bool) if voiced is None else np.asarray(voiced, bool)
    times = (np.arange(f0.shape[0]) * hop + window / 2) / sr
    return track.PitchTrack(times, np.where(voiced, f0, 0.0), voiced, np.where(voiced, 0.01, 1.0))


def _hz(midi, a4=440.0):
    return a4 * 2.0 ** ((np.asarray(midi, np.float64) - 69.0) / 12.0)


def test_a_constant_detune_is_corrected_by_its_negative():
    from phasegen import track
    pt = _track(np.full(50, 440.0 * 2 ** (30 / 1200)))
    for strength, want in ((1.0, -0.30), (0.5, -0.15), (0.0, 0.0)):
        c = track.PitchCurve.correcting(pt, strength=strength)
        assert isinstance(c, track.PitchCurve) and len(c.seconds) == 51
        assert c.seconds[0] == 0.0 and (np.diff(c.seconds) > 0).all() and np.array_equal(c.seconds[1:], pt.times)
        assert np.allclose(c.semitones, want, rtol=0, atol=1e-12), (strength, c.semitones[:3])
    c = track.PitchCurve.correcting(_track(np.full(50, 452.0)), a4=452.0)
    assert np.allclose(c.semitones, 0.0, atol=1e-12)


def test_scales_and_ties():
    from phasegen import track
    C = track.PitchCurve.correcting

    def corr(midi, scale):
        return C(_track([_hz(midi)] * 3), scale=scale).semitones[-1]
    assert corr(61.1, "C:maj") == pytest.approx(62 - 61.1) and corr(60.9, "C:maj") == pytest.approx(60 - 60.9)
    assert corr(61.1, "chromatic") == pytest.approx(-0.1)
    assert corr(63.2, "C:min") == pytest.approx(-0.2) and corr(63.2, "C:maj") == pytest.approx(64 - 63.2)       # Eb is in C minor
    assert corr(61.0, "Db:maj") == pytest.approx(0.0) and corr(61.0, "C#:maj") == pytest.approx(0.0)
    assert corr(57.9, "A:min") == pytest.approx(57 - 57.9) and corr(58.6, "A:min") == pytest.approx(59 - 58.6)
    # ties go to the lower note: 60.5 exactly (chromatic) and 61 between C and D (C major); both are exact in float64
    t = C(_track([_hz(69.5)] * 2))
    assert _hz(69.5) == 440.0 * 2.0 ** (0.5 / 12) and t.semitones[-1] == pytest.approx(-0.5)
    assert corr(61.0, "C:maj") == pytest.approx(-1.0)
    assert track.scale_classes("chromatic") == frozenset(range(12)) and track.scale_classes("G:maj") == frozenset({7, 9, 11, 0, 2, 4, 6})
    assert track.scale_classes("B:min") == frozenset({11, 1, 2, 4, 6, 7, 9})


def test_unvoiced_frames_hold_and_an_unvoiced_track_is_flat():
    from phasegen import track
    f0 = _hz([0, 0, 60.2, 60.2, 0, 0, 64.7, 0])
    voiced = [False, False, True, True, False, False, True, False]
    c = track.PitchCurve.correcting(_track(f0, voiced))
    want = np.array([-0.2, -0.2, -0.2, -0.2, -0.2, -0.2, 0.3, 0.3])
    assert np.allclose(c.semitones, np.concatenate([[want[0]], want]), atol=1e-9)
    flat = track.PitchCurve.correcting(_track(np.zeros(5), np.zeros(5, bool)))
    assert len(flat.seconds) == 6 and (flat.semitones == 0.0).all()
    one = track.PitchCurve.correcting(_track([_hz(60.25)]))
    assert one.anchors == [(0.0, pytest.approx(-0.25)), (512 / 16000, pytest.approx(-0.25))]


def test_retune_ms_is_the_one_pole_recursion():
    from phasegen import track
    f0 = _hz([60.4] * 10 + [62.3] * 10 + [59.55] * 10)
    pt = _track(f0)
    c = np.array([-0.4] * 10 + [-0.3] * 10 + [0.45] * 10)
    for retune_ms in (0.0, 20.0, 50.0, 400.0):
        got = track.PitchCurve.correcting(pt, retune_ms=retune_ms).semitones
        alpha = 1.0 if retune_ms == 0 else 1.0 - np.exp(-256 / (16000 * retune_ms / 1000.0))
        y, prev = [], c[0]
        for v in c:
            prev = prev + alpha * (v - prev)
            y.append(prev)
        assert np.allclose(got[1:], y, rtol=0, atol=1e-9) and got[0] == got[1], retune_ms
    slow = track.PitchCurve.correcting(pt, retune_ms=400.0).semitones
    assert slow[11] < -0.38 and slow[-1] < 0.2                    # a slow retune lags behind the notes


def test_every_rejection():
    from phasegen import track
    C = track.PitchCurve.correcting
    pt = _track([440.0] * 4)
    for kw, word in ((dict(strength=1.5), "strength"), (dict(strength=-0.1), "strength"), (dict(strength=NAN), "strength"),
                     (dict(a4=0.0), "a4"), (dict(a4=float("inf")), "a4"), (dict(retune_ms=-1.0), "retune_ms"), (dict(retune_ms=NAN), "retune_ms")):
        with pytest.raises(ValueError, match="PitchCurve.correcting: .*" + word):
            C(pt, **kw)
    for scale in ("major", "H:maj", "C:dorian", "c:maj", "", None, 7):
        with pytest.raises(ValueError, match="scale must be"):
            C(pt, scale=scale)
    with pytest.raises(ValueError, match="expected a PitchTrack"):
        C([440.0, 440.0])
    with pytest.raises(ValueError, match="one length"):
        C(track.PitchTrack(pt.times, pt.f0[:-1], pt.voiced, pt.ap))
    with pytest.raises(ValueError, match="strictly increasing"):
        C(track.PitchTrack(pt.times[::-1], pt.f0, pt.voiced, pt.ap))
    with pytest.raises(ValueError, match="positive and finite at voiced"):
        C(track.PitchTrack(pt.times, np.array([440.0, 0.0, 440.0, 440.0]), pt.voiced, pt.ap))
