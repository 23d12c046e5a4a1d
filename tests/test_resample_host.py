"""CPU: the host half of pg_resample (sample-rate conversion, include/phasegen.h).  The filter definition is restated here in
float64 numpy and tied to scipy.signal.upfirdn; pg_resample_bank (built on the host in double) is checked against it; the length /
tap formulas, the struct layout and every argument error are checked without a GPU."""
import ctypes
import inspect
import math
from fractions import Fraction

import numpy as np
import pytest

# ---- float64 restatement of the definition (include/phasegen.h) ---------------------------------------------------------------
FILTERS = {0: (64, 14.769656459379492, 0.9475937167399596), 1: (16, 8.555504641634386, 0.85)}   # quality: Z, beta, roll-off


def geometry(up, down, quality):
    g = math.gcd(up, down)
    U, D = up // g, down // g
    W = Fraction(FILTERS[quality][0]) / min(Fraction(1), Fraction(U, D))
    return U, D, math.floor(W), math.floor(W) + math.ceil(W) + 1                   # U, D, H, taps


def h64(t, quality):
    Z, beta, r = FILTERS[quality]
    t = np.asarray(t, np.float64)
    win = np.i0(beta * np.sqrt(np.clip(1.0 - (t / Z) ** 2, 0.0, None))) / np.i0(beta)
    return np.where(np.abs(t) <= Z, r * np.sinc(r * t) * win, 0.0)


def bank64(up, down, quality):
    """(taps, U): bank[k * U + p] = s h(s (p/U + H - k)).  The argument is formed as (p + U (H - k)) / max(U, D), ONE division of
    exact integers, so that |t| <= Z is decided exactly at the edge of the support (h(+-Z) is ~2e-8 there, not 0)."""
    U, D, H, taps = geometry(up, down, quality)
    k, p = np.arange(taps)[:, None], np.arange(U)[None, :]
    return min(1.0, U / D) * h64((p + U * (H - k)) / max(U, D), quality)


def out_len(n_in, up, down):
    g = math.gcd(up, down)
    return (n_in * (up // g) + down // g - 1) // (down // g)


def bank_form64(x, up, down, quality):
    U, D, H, taps = geometry(up, down, quality)
    b, x = bank64(up, down, quality), np.asarray(x, np.float64)
    xp = np.concatenate([np.zeros(H + taps), x, np.zeros(2 * taps)])               # xp[n + H + taps] = x[n]
    y = np.empty(out_len(len(x), up, down))
    for t in range(len(y)):
        n0, p = divmod(t * D, U)
        y[t] = np.dot(b[:, p], xp[n0 + taps:n0 + 2 * taps])
    return y


def direct64(x, up, down, quality):
    """y[t] = sum_n x[n] s h(s (t D / U - n)): no bank, no phases (argument as in bank64: (t D - n U) / max(U, D))."""
    U, D, _, _ = geometry(up, down, quality)
    x = np.asarray(x, np.float64)
    t = np.arange(out_len(len(x), up, down))[:, None]
    return (min(1.0, U / D) * h64((t * D - np.arange(len(x))[None, :] * U) / max(U, D), quality) * x[None, :]).sum(axis=1)
# -------------------------------------------------------------------------------------------------------------------------------


PAIRS = [(160, 441), (441, 160), (1, 2), (2, 1), (3, 2), (147, 160)]


@pytest.mark.parametrize("quality", [0, 1])
@pytest.mark.parametrize("up,down", PAIRS + [(80, 441), (16000, 44100)])
def test_restatement_agrees_with_upfirdn(up, down, quality):
    """The direct sum, the bank form and scipy's polyphase upfirdn on the same prototype (sampled U per input sample, padded in
    front so that its centre is a multiple of D) are one filter: 1e-12."""
    from scipy.signal import upfirdn
    U, D, H, taps = geometry(up, down, quality)
    s = min(1.0, U / D)
    M = math.ceil(Fraction(FILTERS[quality][0] * U) / min(Fraction(1), Fraction(U, D)))          # prototype half length, ceil(W U)
    proto = np.concatenate([np.zeros((-M) % D), s * h64(np.arange(-M, M + 1) / max(U, D), quality)])
    c = (M + (-M) % D) // D
    rng = np.random.default_rng(5)
    for n_in in (1, 100, 1500):
        x = rng.standard_normal(n_in)
        n_out = out_len(n_in, up, down)
        ref = upfirdn(proto, x, U, D)[c:c + n_out]
        assert len(ref) == n_out
        yb, yd = bank_form64(x, up, down, quality), direct64(x, up, down, quality)
        assert np.abs(yb - ref).max() <= 1e-12 and np.abs(yd - ref).max() <= 1e-12, (n_in, np.abs(yb - ref).max(), np.abs(yd - ref).max())


def _bank(up, down, quality):
    from phasegen import _lib
    lib = _lib.load()
    n = lib.pg_resample_bank_elems(up, down, quality)
    assert n > 0
    b = np.full(n + 8, np.float32(-77.0))                                          # guard words: nothing past the bank is written
    assert lib.pg_resample_bank(b.ctypes.data_as(ctypes.c_void_p), up, down, quality) == 0
    assert (b[n:] == -77.0).all()
    return b[:n]


@pytest.mark.parametrize("quality", [0, 1])
@pytest.mark.parametrize("up,down", PAIRS)
def test_bank_is_float32_of_the_float64_bank(up, down, quality):
    from phasegen import _lib
    lib = _lib.load()
    U, D, H, taps = geometry(up, down, quality)
    assert lib.pg_resample_taps(up, down, quality) == taps and lib.pg_resample_bank_elems(up, down, quality) == taps * U
    got, want = _bank(up, down, quality).astype(np.float64), bank64(up, down, quality).reshape(-1)
    err = np.abs(got - want.astype(np.float32).astype(np.float64))
    assert (err <= 2.0 ** -23 * np.abs(want) + 1e-12).all(), err.max()
    assert np.abs(got).max() > 0.3 * min(1.0, U / D)                               # (a real filter: the centre tap)


@pytest.mark.parametrize("quality", [0, 1])
def test_unreduced_rates_give_the_reduced_bank(quality):
    assert np.array_equal(_bank(16000, 44100, quality), _bank(160, 441, quality))
    assert np.array_equal(_bank(44100, 16000, quality), _bank(441, 160, quality))


def test_taps_and_lengths_follow_the_formulas():
    from phasegen import _lib
    lib = _lib.load()
    assert geometry(160, 441, 0) == (160, 441, 176, 354)                            # the issue's worked example
    assert lib.pg_resample_taps(160, 441, 0) == 354 and lib.pg_resample_bank_elems(16000, 44100, 0) == 354 * 160
    rates = (8000, 11025, 16000, 22050, 32000, 44100, 48000)
    beyond = set()
    for a in rates:                                                                 # a -> b
        for b in rates:
            for q in (0, 1):
                U, D, H, taps = geometry(b, a, q)
                assert taps <= 2048
                if U > 1024:                                                        # 32000 / 11025 = 1280 / 441
                    beyond.add((a, b))
                    assert lib.pg_resample_taps(b, a, q) == _lib.ERR_UNSUPPORTED
                else:
                    assert lib.pg_resample_taps(b, a, q) == taps and lib.pg_resample_bank_elems(b, a, q) == taps * U, (a, b, q)
    assert beyond == {(11025, 32000)}                              # every other pair of the common rates is covered
    for up, down in PAIRS + [(16000, 44100), (48000, 44100), (7, 7)]:
        for n_in in (1, 2, 100, 2823, 2824, 44100, 13_500_000, 2 ** 31 + 11, 2 ** 40 + 3):
            assert lib.pg_resample_out_len(n_in, up, down) == out_len(n_in, up, down), (n_in, up, down)
    assert 3_000_000_017 * 441 > 2 ** 32 and lib.pg_resample_out_len(3_000_000_017, 441, 160) == -(-3_000_000_017 * 441 // 160)
    assert lib.pg_resample_out_len(1, 160, 441) == 1 and lib.pg_resample_out_len(1, 441, 160) == 3


def test_limits_are_unsupported_not_wrong():
    from phasegen import _lib
    lib = _lib.load()
    assert lib.pg_resample_taps(1024, 1023, 0) == 129                               # U = 1024: the last supported phase count
    assert lib.pg_resample_taps(1025, 1024, 0) == _lib.ERR_UNSUPPORTED and b"phases" in lib.pg_last_error_string()
    assert lib.pg_resample_taps(2050, 2048, 0) == _lib.ERR_UNSUPPORTED              # reduced first: 1025 / 1024
    assert lib.pg_resample_taps(2048, 2046, 0) == 129                               # ... 1024 / 1023
    assert lib.pg_resample_taps(64, 1023, 0) == 2047                                # W = 1023: 2047 taps
    assert lib.pg_resample_taps(1, 16, 0) == _lib.ERR_UNSUPPORTED and b"taps" in lib.pg_last_error_string()   # 2049
    assert lib.pg_resample_taps(1, 16, 1) == 513                                    # kaiser_fast is four times shorter
    assert lib.pg_resample_bank_elems(1, 16, 0) == _lib.ERR_UNSUPPORTED
    buf = (ctypes.c_float * 4)()
    assert lib.pg_resample_bank(buf, 1, 16, 0) == _lib.ERR_UNSUPPORTED


def test_resample_args_layout():
    from phasegen import _lib
    A = _lib.ResampleArgs
    assert ctypes.sizeof(A) == 72
    assert (A.n_signals.offset, A.up.offset, A.down.offset, A.quality.offset) == (0, 4, 8, 12)
    assert (A.n_in.offset, A.n_out.offset, A.x.offset, A.x_stride.offset) == (16, 24, 32, 40)
    assert (A.y.offset, A.y_stride.offset, A.bank.offset) == (48, 56, 64)
    assert (_lib.RS_KAISER_BEST, _lib.RS_KAISER_FAST) == (0, 1)
    for name in ("pg_resample_out_len", "pg_resample_taps", "pg_resample_bank_elems", "pg_resample_bank", "pg_resample"):
        assert name in _lib.SYMBOLS
    assert _lib.load().pg_version() == 400                                          # additive within ABI 0.4


def _args(_lib):
    a = _lib.ResampleArgs()
    a.n_signals, a.up, a.down, a.quality, a.n_in, a.n_out = 3, 160, 441, 0, 2824, 1025
    a.x = a.y = a.bank = 4096                                                       # never dereferenced: every call below fails first
    a.x_stride, a.y_stride = 2824, 1025
    return a


def test_argument_errors_are_reported_before_any_launch():
    from phasegen import _lib
    lib = _lib.load()
    rs = lib.pg_resample
    assert out_len(2824, 160, 441) == 1025
    assert rs(None, None) == _lib.ERR_NULL
    for field in ("n_signals", "n_in", "up", "down"):
        for bad in (0, -3):
            a = _args(_lib)
            setattr(a, field, bad)
            assert rs(ctypes.byref(a), None) == _lib.ERR_SHAPE, (field, bad)
            assert b"non-positive" in lib.pg_last_error_string()
    for q in (2, -1, 99):
        a = _args(_lib)
        a.quality = q
        assert rs(ctypes.byref(a), None) == _lib.ERR_UNSUPPORTED and b"quality" in lib.pg_last_error_string()
        assert lib.pg_resample_taps(160, 441, q) == _lib.ERR_UNSUPPORTED
        assert lib.pg_resample_bank_elems(160, 441, q) == _lib.ERR_UNSUPPORTED
    for n_out in (1024, 1026, 0, -1):
        a = _args(_lib)
        a.n_out = n_out
        assert rs(ctypes.byref(a), None) == _lib.ERR_SHAPE and b"n_out" in lib.pg_last_error_string()
    for field, v in (("x_stride", 2823), ("y_stride", 1024), ("x_stride", 0), ("y_stride", -1025)):
        a = _args(_lib)
        setattr(a, field, v)
        assert rs(ctypes.byref(a), None) == _lib.ERR_SHAPE and b"stride" in lib.pg_last_error_string(), field
    for field in ("x", "y", "bank"):
        a = _args(_lib)
        setattr(a, field, None)
        assert rs(ctypes.byref(a), None) == _lib.ERR_NULL and b"required" in lib.pg_last_error_string(), field
    a = _args(_lib)
    a.up, a.down, a.n_out = 1025, 1024, out_len(2824, 1025, 1024)
    assert rs(ctypes.byref(a), None) == _lib.ERR_UNSUPPORTED
    a = _args(_lib)
    a.up, a.down, a.n_out = 1, 16, out_len(2824, 1, 16)
    assert rs(ctypes.byref(a), None) == _lib.ERR_UNSUPPORTED
    for n_in, up, down in ((0, 1, 2), (-5, 1, 2), (10, 0, 2), (10, 2, 0), (10, -1, 2)):
        assert lib.pg_resample_out_len(n_in, up, down) == _lib.ERR_SHAPE
    assert lib.pg_resample_taps(0, 2, 0) == _lib.ERR_SHAPE and lib.pg_resample_bank_elems(2, -2, 0) == _lib.ERR_SHAPE
    assert lib.pg_resample_bank(None, 160, 441, 0) == _lib.ERR_NULL


def test_load_audio_converts_like_the_loading_half_of_librosa_load(tmp_path):
    """scipy's wav reader + the integer scalings + mono averaging; no GPU involved."""
    from scipy.io import wavfile
    from phasegen import preproc
    rng = np.random.default_rng(2)
    s16 = rng.integers(-32768, 32768, size=(1000, 2), dtype=np.int16)
    s16[0] = (-32768, 32767)
    s32 = rng.integers(-2 ** 31, 2 ** 31, size=777, dtype=np.int32)
    u8 = rng.integers(0, 256, size=(300, 3), dtype=np.uint8)
    f32 = rng.standard_normal(555).astype(np.float32)
    for name, sr, d in (("a", 44100, s16), ("b", 48000, s32), ("c", 8000, u8), ("d", 22050, f32)):
        wavfile.write(tmp_path / f"{name}.wav", sr, d)
    a, sr = preproc.load_audio(str(tmp_path / "a.wav"))
    assert sr == 44100 and a.dtype == np.float32 and np.array_equal(a, (s16.astype(np.float32) / np.float32(32768)).mean(axis=1))
    a2, _ = preproc.load_audio(str(tmp_path / "a.wav"), mono=False)
    assert a2.shape == (2, 1000) and np.array_equal(a2, s16.T.astype(np.float32) / np.float32(32768)) and a2.min() == -1.0
    a, sr = preproc.load_audio(str(tmp_path / "b.wav"))
    assert sr == 48000 and a.dtype == np.float32 and np.array_equal(a, s32.astype(np.float32) / np.float32(2.0 ** 31))
    a, sr = preproc.load_audio(str(tmp_path / "c.wav"))
    assert sr == 8000 and np.array_equal(a, ((u8.astype(np.float32) - 128) / 128).mean(axis=1)) and a.dtype == np.float32
    a, sr = preproc.load_audio(str(tmp_path / "d.wav"))
    assert sr == 22050 and a.dtype == np.float32 and np.array_equal(a, f32)


def test_python_surface():
    """Signatures only (the calls need a GPU)."""
    from phasegen import ops, preproc
    p = inspect.signature(ops.resample).parameters
    assert list(p) == ["x", "orig_sr", "target_sr", "res_type", "out"] and p["res_type"].default == "kaiser_best" and p["out"].default is None
    p = inspect.signature(preproc.resample).parameters
    assert list(p) == ["audio", "orig_sr", "target_sr", "res_type", "device"] and p["res_type"].default == "kaiser_best"
    p = inspect.signature(preproc.get_mix_chunks).parameters
    assert list(p) == ["fn", "t_slice", "n_fft", "hop_length", "n_random", "rsr", "osr", "rng", "device"] and p["osr"].default == 44100
    p = inspect.signature(preproc.build_dataset).parameters
    assert p["osr"].default is None and p["rsr"].default == 16000 and list(p)[0] == "tracks"
    assert inspect.signature(preproc.load_audio).parameters["mono"].default is True
    b = ops.resample_bank_host(16000, 44100)
    assert b.shape == (354, 160) and b.dtype == np.float32
