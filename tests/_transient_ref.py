"""numpy restatements of pg_hpss's and pg_ola_stretch's contracts (include/phasegen.h) word for word, for the tests of the
transient-preserving stretch (no GPU, no phasegen import).  The device must reproduce both BIT FOR BIT.

  key, unkey      the IEEE total order on the bit pattern as a uint32, and back
  hpss            M (..., bins, F) float32 -> (harm, perc): medians by SORTING the keys of every edge-replicated window
  ola_window      the periodic Hann window, from the double formula
  ola_stretch     x (n_sig, n_in) -> (n_sig, n_out): fp32 sums over the covering frames in ascending g (dtype=np.float64: the same
                  loop in double, for the float64 chain)
  clicky_melody, crests, stretch64   the synthetic signal of the ordering tests, its figure of merit, and the float64 chain around
                  both kernels (the analysis, the ISTFT and the phase restatements are tests/_vocoder_ref.py's and tests/_lock_ref.py's)
"""
import math

import numpy as np

import _lock_ref as lref
import _vocoder_ref as ref


# ---- pg_hpss ---------------------------------------------------------------------------------------------------------------------

def key(x):
    """float32 array -> uint32: bits ^ (sign ? 0xFFFFFFFF : 0x80000000)"""
    u = np.ascontiguousarray(np.asarray(x, np.float32)).view(np.uint32)
    return u ^ np.where(u >> np.uint32(31), np.uint32(0xFFFFFFFF), np.uint32(0x80000000))


def unkey(k):
    k = np.ascontiguousarray(np.asarray(k, np.uint32))
    return (k ^ np.where(k >> np.uint32(31), np.uint32(0x80000000), np.uint32(0xFFFFFFFF))).view(np.float32)


def _median_keys(K, h, axis):
    """the element of rank h among K[clamp(i + d)], d = -h .. h, along ``axis``"""
    pad = [(0, 0)] * K.ndim
    pad[axis] = (h, h)
    win = np.lib.stride_tricks.sliding_window_view(np.pad(K, pad, mode="edge"), 2 * h + 1, axis=axis)
    return np.sort(win, axis=-1)[..., h]


def hpss(M, win_t, win_f):
    """M (..., bins, F) float32 -> (harm, perc) float32: a cell is harmonic iff key(H) >= key(P)."""
    assert win_t % 2 == 1 and win_f % 2 == 1 and 1 <= win_t <= 31 and 1 <= win_f <= 31
    M = np.ascontiguousarray(np.asarray(M, np.float32))
    K = key(M)
    H = _median_keys(K, (win_t - 1) // 2, K.ndim - 1)
    P = _median_keys(K, (win_f - 1) // 2, K.ndim - 2)
    harmonic = H >= P
    zero = np.float32(0.0)
    return np.where(harmonic, M, zero), np.where(harmonic, zero, M)


# ---- pg_ola_stretch --------------------------------------------------------------------------------------------------------------

def ola_window(win_len):
    """(float)(0.5 - 0.5 cos(2 pi j / win_len)) in double, rounded once (math.cos: the C library's)"""
    return np.array([0.5 - 0.5 * math.cos(2.0 * 3.141592653589793 * j / win_len) for j in range(win_len)], np.float64).astype(np.float32)


def ola_frames(n_out, win_len, hop):
    """(g_lo, g_hi) int64 (n_out,): the frames g >= 0 with g hop - w/2 <= t <= g hop + w/2 - 1"""
    t = np.arange(n_out, dtype=np.int64)
    half = win_len // 2
    g_lo = np.maximum(-((half - 1 - t) // hop), 0)                        # ceil((t - w/2 + 1) / hop)
    return g_lo, (t + half) // hop


def centres(g, hop, src_per_out):
    """c_g = (int64) rint((double)(g hop) * src_per_out) and whether it is inside 2^62"""
    c = np.rint((np.asarray(g, np.int64) * hop).astype(np.float64) * float(src_per_out))
    inside = c < 2.0 ** 62
    return np.where(inside, c, 0.0).astype(np.int64), inside


def ola_stretch(x, n_out, src_per_out, win, hop, base=None, dtype=np.float32, return_reads=False):
    """x (n_sig, n_in), win (w,), base None or (n_sig, n_out) -> (n_sig, n_out): per output sample, over its covering frames in
    ascending g, den = fl(den + win[j]), num = fl(num + fl(win[j] x[s])) where 0 <= s < n_in, r = den > 0 ? num / den : 0,
    y = base ? fl(base + r) : r.  ``return_reads``: also, per output sample, the list of the s it read (for the cone of a NaN)."""
    x = np.asarray(x, dtype)
    win = np.asarray(win, dtype)
    n_sig, n_in = x.shape
    w = win.shape[0]
    half = w // 2
    t = np.arange(n_out, dtype=np.int64)
    g_lo, g_hi = ola_frames(n_out, w, hop)
    den, num = np.zeros(n_out, dtype), np.zeros((n_sig, n_out), dtype)
    reads = [[] for _ in range(n_out)] if return_reads else None
    for k in range(int((g_hi - g_lo).max()) + 1):                         # the k-th covering frame of every sample: ascending g
        g = g_lo + k
        covered = g <= g_hi
        j = np.where(covered, t - g * hop + half, 0)
        assert ((j >= 0) & (j < w)).all()
        cg, inside = centres(g, hop, src_per_out)
        s = cg + j - half
        wj = win[j]
        den = np.where(covered, den + wj, den)
        term = covered & inside & (s >= 0) & (s < n_in)
        sc = np.where(term, s, 0)
        with np.errstate(invalid="ignore", over="ignore"):
            num = np.where(term, num + wj * x[:, sc], num)
        if return_reads:
            for i in np.flatnonzero(term):
                reads[i].append(int(s[i]))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        r = np.where(den > 0, num / np.where(den > 0, den, dtype(1)), dtype(0)).astype(dtype)
        y = r if base is None else (np.asarray(base, dtype) + r).astype(dtype)
    return (y, reads) if return_reads else y


# ---- the synthetic signal of the ordering tests and the float64 chain ------------------------------------------------------------

CLICK_TIMES = (0.93, 1.78, 2.83, 3.41, 4.47)                             # seconds; none on a note's attack
CLICK_SAMPLES = 32                                                        # 2 ms at 16 kHz
CLICK_AMPLITUDE = 8.0
BACKGROUND = 0.05                                                         # std of the stationary noise under the melody


def clicky_melody(sr=16000, seed=0, background=BACKGROUND):
    """The melody of tests/_vocoder_ref.py (6 s) over stationary white noise of std ``background`` (26 dB under a note's fundamental),
    plus five 2 ms bursts of uniform noise of amplitude 8 -> (float32 (samples,), the bursts' centres in samples).  The noise makes
    the material DENSE: no bin falls silent between events, so the vocoder's reset floor cannot rescue an onset by itself (on the
    bare melody it does, for the clicks that happen to sit well on the output grid: tests/test_transient_host.py has the figures)."""
    x = ref.melody(sr).astype(np.float64)
    rs = np.random.RandomState(1000 + seed)
    x += background * rs.standard_normal(x.shape[0])
    at = []
    for tc in CLICK_TIMES:
        c = int(round(tc * sr))
        x[c - CLICK_SAMPLES // 2:c + CLICK_SAMPLES // 2] += CLICK_AMPLITUDE * rs.uniform(-1.0, 1.0, CLICK_SAMPLES)
        at.append(c)
    return x.astype(np.float32), tuple(at)


def crests(y, at, stretch, near=96, around=2048):
    """For every click: the peak of |y| within +-near samples of where the click belongs, over the rms of +-around samples."""
    y = np.asarray(y, np.float64)
    out = []
    for c in at:
        p = int(round(c * stretch))
        out.append(float(np.abs(y[p - near:p + near + 1]).max() / np.sqrt((y[p - around:p + around + 1] ** 2).mean())))
    return out


def stretch64(x, stretch, n_fft=2048, hop=512, frames=128, overlap_frames=32, floor=0.2, split=True, hpss_win=(17, 17), win_len=256,
              ola_hop=64):
    """The track layer's phase="vocoder_locked" stretch of a mono signal in float64 (the phase itself by the bit-exact restatement on
    the float32 planes), without and with the harmonic / percussive split -> (hop * (F_out - 1),) float64."""
    from phasegen.track import spectral_plan
    pl = spectral_plan(x.shape[0], frames, hop, overlap_frames, stretch)
    logmag, ang = ref.analysis64(np.asarray(x, np.float64)[None], pl.n_src, n_fft, hop)
    A, M = ang.astype(np.float32), logmag.astype(np.float32)
    spo = 1.0 / stretch
    if split:
        M, perc = hpss(M, *hpss_win)
    mag = ref.resample64(M, pl.F_out, spo)
    ph = lref.phase_lock(A, pl.F_out, spo, M, floor)
    y = ref.istft64(np.expm1(mag) * np.exp(1j * ph.astype(np.float64)), n_fft, hop)
    if split:
        p_audio = ref.istft64(np.expm1(perc.astype(np.float64)) * np.exp(1j * A.astype(np.float64)), n_fft, hop)      # (the fp32 plane's phase)
        y = ola_stretch(p_audio, y.shape[1], spo, ola_window(win_len).astype(np.float64), ola_hop, base=y, dtype=np.float64)
    return y[0]
