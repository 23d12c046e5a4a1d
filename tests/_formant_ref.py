"""pg_formant_shift restated (include/phasegen.h; not collected): the helpers of tests/test_formant_host.py and
tests/test_z_formant_gpu.py.

    ref64   the contract word for word in float64, on the fp32 plane and the fp32 table;
    seq32   the same steps in numpy float32 with strictly sequential accumulation along both sums: the honest stand-in for a
            kernel that is allowed its own summation order, and the source of every threshold;
    errors  the per-frame error r = |got - ref64| / (2^-24 max_k h[k]) of an envelope (h: the peak-held frame) and, for `out`,
            r = |got - ref64| / (2^-24 max_k |out_ref64[k]|).

A result is accepted when its largest r is at most MARGIN = 4 times seq32's own largest r ON THE SAME INPUT (the convention of
tests/_conv_ref64.py and tests/_signal_ref64.py): the threshold is never derived from the kernel.  A frame whose h is all zero
must come out exactly zero.  seq32 takes a `fault`: the mistakes the comparison must reject (tests/test_formant_host.py).

The idealised vowels of the quality rows live here too: harmonic combs under four Lorentzian formants, as Hann main lobes on the
project's bin grid (bin k is FFT bin k + 1)."""
import numpy as np

MARGIN = 4.0
U24 = 2.0 ** -24
LOG2E = np.float32(1.44269504088896341)
FAULTS = ("no_lifter", "hold_short", "k_for_k_plus_1", "no_eps", "one_iteration_less", "neighbour_frame")


def basis64(bins, order):
    """pg_formant_basis's formula in float64: (T (order, bins), s (order,))"""
    q = np.arange(order, dtype=np.float64)[:, None]
    k = np.arange(bins, dtype=np.float64)[None, :]
    T = np.cos(np.pi * q * (k + 0.5) / bins)
    c = np.where(np.arange(order) == 0, 1.0 / bins, 2.0 / bins)
    w = 0.5 * (1.0 + np.cos(np.pi * np.arange(order, dtype=np.float64) / order))
    return T, c * w


def basis32(bins, order):
    """... rounded once: the table the library hands out, as one flat float32 array"""
    T, s = basis64(bins, order)
    return np.concatenate([T.reshape(-1), s]).astype(np.float32)


def split(basis, bins, order):
    return basis[:order * bins].reshape(order, bins), basis[order * bins:order * bins + order]


def peak_hold(x, hold, lo=None, hi=None):
    """h[k] = max over d = -lo .. hi of x[clamp(k + d)] along axis -2 (exact in any type); lo = hi = hold by default"""
    lo = hold if lo is None else lo
    hi = hold if hi is None else hi
    bins = x.shape[-2]
    k = np.arange(bins)
    h = x.copy()
    for d in range(-lo, hi + 1):
        h = np.maximum(h, np.take(x, np.clip(k + d, 0, bins - 1), axis=-2))
    return h


def positions(bins, ratio, offset=1):
    """(i0, i1, w as the float32 the contract names)"""
    p = np.clip((np.arange(bins, dtype=np.float64) + offset) * float(ratio) - offset, 0.0, bins - 1.0)
    i0 = np.floor(p).astype(np.int64)
    i1 = np.minimum(i0 + 1, bins - 1)
    return i0, i1, (p - i0).astype(np.float32)


def ref64(M, basis, order, hold, iters, ratio, eps):
    """-> (env, out, h), float64, shaped like M (n_ch, bins, F)"""
    bins = M.shape[-2]
    T, s = (v.astype(np.float64) for v in split(basis, bins, order))
    x = M.astype(np.float64)
    h = peak_hold(x, hold)

    def S(v):
        return np.einsum("qk,cqg->ckg", T, s[None, :, None] * np.einsum("qj,cjg->cqg", T, v))

    e = S(h)
    for _ in range(iters):
        e = S(np.maximum(h, e))
    if float(ratio) == 1.0:
        return e, x.copy(), h
    i0, i1, w = positions(bins, ratio)
    w = w.astype(np.float64)[None, :, None]
    ew = e[:, i0] + w * (e[:, i1] - e[:, i0])
    eps = float(np.float32(eps))
    a = np.expm1(np.maximum(ew, 0.0)) + eps
    b = np.expm1(np.maximum(e, 0.0)) + eps
    out = np.log1p(np.expm1(x) * (a / b))
    out[x == 0.0] = 0.0
    return e, out, h


def expm1_32(m):
    """the library's expm1: 2^(m log2 e) - 1 in float32"""
    return (np.exp2((m * LOG2E).astype(np.float32)).astype(np.float32) - np.float32(1.0)).astype(np.float32)


def log1p_32(x):
    """the library's log1p for x >= 0: log(u) + (x - (u - 1)) / u with u = fl(1 + x)"""
    u = (np.float32(1.0) + x).astype(np.float32)
    d = (u - np.float32(1.0)).astype(np.float32)
    return (np.log(u).astype(np.float32) + ((x - d).astype(np.float32) / u).astype(np.float32)).astype(np.float32)


def seq32(M, basis, order, hold, iters, ratio, eps, fault=None):
    """-> (env, out), float32: every product and every addition rounded to float32, both sums strictly in ascending index order"""
    assert fault is None or fault in FAULTS, fault
    f32 = np.float32
    n_ch, bins, F = M.shape
    T, s = split(basis.astype(f32), bins, order)
    if fault == "no_lifter":
        s = np.where(np.arange(order) == 0, 1.0 / bins, 2.0 / bins).astype(f32)
    x = M.astype(f32)
    h = peak_hold(x, hold, hi=hold - 1) if (fault == "hold_short" and hold > 0) else peak_hold(x, hold)

    def S(v):
        c = np.zeros((n_ch, order, F), f32)
        for j in range(bins):
            c = (c + (T[None, :, j, None] * v[:, None, j, :]).astype(f32)).astype(f32)
        c = (s[None, :, None] * c).astype(f32)
        e = np.zeros((n_ch, bins, F), f32)
        for q in range(order):
            e = (e + (T[None, q, :, None] * c[:, q, None, :]).astype(f32)).astype(f32)
        return e

    e = S(h)
    for _ in range(iters - 1 if (fault == "one_iteration_less" and iters > 0) else iters):
        e = S(np.maximum(h, e))
    if fault == "neighbour_frame" and F > 1:
        e = np.roll(e, 1, axis=2)
    if float(ratio) == 1.0:
        return e, x.copy()
    i0, i1, w = positions(bins, ratio, offset=0 if fault == "k_for_k_plus_1" else 1)
    w = w[None, :, None]
    ew = (e[:, i0] + (w * (e[:, i1] - e[:, i0]).astype(f32)).astype(f32)).astype(f32)
    eps = f32(0.0) if fault == "no_eps" else f32(eps)
    a = (expm1_32(np.maximum(ew, f32(0.0))) + eps).astype(f32)
    b = (expm1_32(np.maximum(e, f32(0.0))) + eps).astype(f32)
    with np.errstate(divide="ignore", invalid="ignore"):
        out = log1p_32((expm1_32(x) * (a / b).astype(f32)).astype(f32))
    out[x == 0.0] = 0.0
    return e, out


def errors(got_env, got_out, ref):
    """(r_max of env, r_max of out) of float arrays against ref = ref64(...)'s triple; either `got` may be None (-> 0.0).  A frame whose
    h is all zero (its envelope and its out are exactly zero in ref64) must be exactly zero: anything else returns inf."""
    env, out, h = ref
    hmax = h.max(axis=1)                                              # (n_ch, F)
    omax = np.abs(out).max(axis=1)
    res = []
    for got, want, scale in ((got_env, env, hmax), (got_out, out, omax)):
        if got is None:
            res.append(0.0)
            continue
        d = np.abs(np.asarray(got, np.float64) - want).max(axis=1)
        d = np.where(np.isnan(d), np.inf, d)
        silent = hmax == 0.0
        r = np.where(silent, np.where(d == 0.0, 0.0, np.inf), d / (U24 * np.where(scale > 0.0, scale, 1.0)))
        r = np.where(~silent & (scale == 0.0) & (d > 0.0), np.inf, r)
        res.append(float(r.max()))
    return tuple(res)


def thresholds(M, basis, order, hold, iters, ratio, eps, ref=None):
    """(ref64 triple, (thr_env, thr_out, seq_env, seq_out)): MARGIN times seq32's own r_max on this input"""
    ref = ref64(M, basis, order, hold, iters, ratio, eps) if ref is None else ref
    se, so = errors(*seq32(M, basis, order, hold, iters, ratio, eps), ref)
    return ref, (MARGIN * se, MARGIN * so, se, so)


def accepted(got_env, got_out, ref, thr):
    ge, go = errors(got_env, got_out, ref)
    return ge <= thr[0] and go <= thr[1], (ge, go)


# ---- idealised vowels -------------------------------------------------------------------------------------------------------------------
SR, N_FFT = 16000, 2048
FORMANT_HZ = ((730.0, 200.0), (1090.0, 220.0), (2440.0, 340.0), (3400.0, 500.0))     # (centre, full width at half maximum) of an open vowel
FORMANT_GAIN = (1.0, 0.7, 0.35, 0.25)
FORMANT_FLOOR = 0.005                                                  # what is left between and above the resonances
F0S = (110.0, 180.0, 260.0, 400.0)
SHIFTS = (4.0, -4.0, 7.0, 12.0, -7.0)
BAND = (300.0, 4000.0)
PEAK = 60.0                                                            # linear magnitude of the strongest partial (log1p: 4.1)


def true_envelope(f):
    """linear amplitude of the vowel's envelope at frequency f (Hz): four Lorentzians g / (1 + ((f - c) / (w / 2))^2) and a floor"""
    f = np.asarray(f, np.float64)
    return sum(g / (1.0 + ((f - c) / (0.5 * bw)) ** 2) for (c, bw), g in zip(FORMANT_HZ, FORMANT_GAIN)) + FORMANT_FLOOR


def hann_lobe(d):
    """|spectrum| of a Hann window at d bins from its centre, 1 at d = 0"""
    d = np.asarray(d, np.float64)
    return np.abs(np.sinc(d) + 0.5 * np.sinc(d - 1.0) + 0.5 * np.sinc(d + 1.0))


def vowel_frame(f0, bins=N_FFT // 2, sr=SR):
    """log1p magnitudes (bins,) float32 of a steady vowel at f0: every harmonic below Nyquist as a Hann main lobe"""
    fb = (np.arange(bins, dtype=np.float64) + 1.0) * sr / (2.0 * bins)            # bin k is FFT bin k + 1
    hz = sr / (2.0 * bins)
    mag = np.zeros(bins)
    m = 1
    while m * f0 < sr / 2.0:
        mag += true_envelope(m * f0) * hann_lobe((fb - m * f0) / hz)
        m += 1
    return np.log1p(PEAK * mag / true_envelope(FORMANT_HZ[0][0])).astype(np.float32)


def harmonic_error_db(frame, f0, played_ratio, bins=N_FFT // 2, sr=SR):
    """rms dB error of the harmonics of a log1p frame whose partials sit at m f0 and will be PLAYED at played_ratio m f0, against the
    true envelope there, over BAND, after removing the median"""
    hz = sr / (2.0 * bins)
    lin = np.expm1(np.asarray(frame, np.float64))
    diffs = []
    m = 1
    while m * f0 < sr / 2.0:
        f_play = played_ratio * m * f0
        k = int(round(m * f0 / hz)) - 1
        if BAND[0] <= f_play <= BAND[1] and 0 <= k < bins and lin[k] > 0.0:
            diffs.append(20.0 * np.log10(lin[k]) - 20.0 * np.log10(true_envelope(f_play)))
        m += 1
    d = np.array(diffs)
    d = d - np.median(d)
    return float(np.sqrt(np.mean(d * d)))


def vowel_audio(f0, seconds, sr=SR):
    """a harmonic source through the four resonances: sum of cosines with the envelope's amplitudes, peak 0.5 (float32)"""
    t = np.arange(int(round(seconds * sr)), dtype=np.float64) / sr
    y = np.zeros_like(t)
    m = 1
    while m * f0 < 0.45 * sr:
        y += true_envelope(m * f0) * np.cos(2.0 * np.pi * m * f0 * t + 0.7 * m * m)
        m += 1
    return (0.5 * y / np.abs(y).max()).astype(np.float32)


def played_error_db(y, f0, sr=SR, n=8192):
    """rms dB error of the partials of a steady tone at f0 against the vowel's true envelope over 300 Hz .. 4 kHz, median removed:
    amplitudes from a Hann-windowed transform of the middle n samples, zero-padded four times (the largest value around each partial:
    less than 0.1 dB of scalloping)"""
    seg = np.asarray(y, np.float64)[len(y) // 2 - n // 2:len(y) // 2 + n // 2] * np.hanning(n)
    spec = np.abs(np.fft.rfft(seg, 4 * n))
    diffs, m = [], 1
    while m * f0 < sr / 2.0:
        f = m * f0
        k = int(round(f * 4 * n / sr))
        if BAND[0] <= f <= BAND[1]:
            diffs.append(20.0 * np.log10(spec[k - 8:k + 9].max()) - 20.0 * np.log10(true_envelope(f)))
        m += 1
    d = np.array(diffs)
    d -= np.median(d)
    return float(np.sqrt(np.mean(d * d)))
