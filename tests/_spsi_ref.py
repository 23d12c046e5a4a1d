"""numpy restatement of pg_phase_spsi's contract (include/phasegen.h) word for word, for the single-pass-inversion tests (no GPU, no
phasegen import): a plain Python loop over the frames, IEEE fp32 for the offset (one division, nothing contracted: numpy never
fuses), double for the advance, uint32 wrap-around sums.  The device must reproduce it BIT FOR BIT.

  offset       one frame's magnitudes (bins,) and peak bins p -> (delta float32, d float32) of every p
  advance      one frame's magnitudes (bins,) -> adv (bins,) uint32 of EVERY bin taken as a peak p
  phase_spsi   M (..., bins, F) float32 -> (..., bins, F) float32; with return_theta also Theta (..., bins, F) uint32
"""
import numpy as np

from _lock_ref import peak_map
from _vocoder_ref import angle_of


def offset(m, p):
    """alpha = m[p-1], beta = m[p], gamma = m[p+1]; d = fl(fl(alpha - beta) + fl(gamma - beta)); n = 0.5f * fl(alpha - gamma);
    delta = n / d if 0 < p < bins - 1 and d < 0, otherwise 0; if not (|delta| <= 0.5), which covers NaN, delta = 0."""
    m = np.asarray(m, np.float32)
    p = np.asarray(p, np.int64)
    bins = m.shape[0]
    inner = (p > 0) & (p < bins - 1)
    lo, hi = np.clip(p - 1, 0, bins - 1), np.clip(p + 1, 0, bins - 1)
    with np.errstate(all="ignore"):
        al, be, ga = m[lo], m[p], m[hi]
        d = ((al - be).astype(np.float32) + (ga - be).astype(np.float32)).astype(np.float32)
        n = (np.float32(0.5) * (al - ga).astype(np.float32)).astype(np.float32)
        use = inner & (d < np.float32(0))
        delta = np.where(use, (n / np.where(use, d, np.float32(1))).astype(np.float32), np.float32(0)).astype(np.float32)
        delta = np.where(np.abs(delta) <= np.float32(0.5), delta, np.float32(0)).astype(np.float32)
    return delta, d


def advance(m, n_fft, hop, bin0=1):
    """x = ((double)(p + bin0) + (double)delta) * ((double)hop / (double)n_fft); adv[p] = (uint32)(int64) rint(x * 4294967296.0)."""
    m = np.asarray(m, np.float32)
    p = np.arange(m.shape[0], dtype=np.int64)
    delta, _ = offset(m, p)
    x = ((p + int(bin0)).astype(np.float64) + delta.astype(np.float64)) * (float(hop) / float(n_fft))
    return np.rint(x * 4294967296.0).astype(np.int64).astype(np.uint32)      # two's-complement wrap


def parity(bins, bin0=1):
    """((b + bin0) & 1) << 31: the half turn of the odd FFT bins."""
    return (((np.arange(bins, dtype=np.int64) + int(bin0)) & 1) << 31).astype(np.uint32)


def phase_spsi(M, n_fft, hop, bin0=1, return_theta=False):
    M = np.asarray(M, np.float32)
    assert M.ndim >= 2
    lead, (bins, F) = M.shape[:-2], M.shape[-2:]
    M2 = M.reshape(-1, bins, F)
    half = parity(bins, bin0)
    out = np.empty(M2.shape, np.float32)
    theta = np.empty(M2.shape, np.uint32)
    for c in range(M2.shape[0]):
        T = np.zeros(bins, np.uint32)                                       # Theta_0 = 0
        for g in range(F):
            if g >= 1:
                m = M2[c, :, g]
                P = peak_map(m)
                T = T[P] + advance(m, n_fft, hop, bin0)[P]                  # uint32 + uint32 wraps
            theta[c, :, g] = T
            out[c, :, g] = angle_of(T + half)
    out, theta = out.reshape(lead + (bins, F)), theta.reshape(lead + (bins, F))
    return (out, theta) if return_theta else out
