"""numpy restatement of pg_phase_lock_linked's contract (include/phasegen.h) and the float64 chain around it, for the channel-linking
tests (no GPU, no phasegen import).  It is built from tests/_lock_ref.py and tests/_vocoder_ref.py and changes neither.

  phase_lock_linked   A (n_ch, bins, F_src), Aref, Mref (bins, F_src) float32 -> (n_ch, bins, F_out) float32: the rotation T that
                      _lock_ref.phase_lock forms for the single channel (Aref, Mref), added to q(A) of every channel.  The device
                      must reproduce it BIT FOR BIT.
  stereo_melody       the melody of _vocoder_ref with every note panned and delayed between two channels: float32 (2, n)
  linked_analysis64   _vocoder_ref.analysis64 with one more row, the channel mean, standardised with the channels' moments
  mid_consistency64   _vocoder_ref.consistency64 of the channel mean of an output against the mid row's magnitudes
  ipd_error           how far the inter-channel phase difference of an output is from the analysis' own, in radians (rms)
"""
import numpy as np

import _lock_ref as lref
import _vocoder_ref as ref
from _vocoder_ref import angle_of, positions, q


def phase_lock_linked(A, Aref, Mref, F_out, spo, reset_below=0.0):
    A, Aref, Mref = np.asarray(A, np.float32), np.asarray(Aref, np.float32), np.asarray(Mref, np.float32)
    assert A.ndim == 3 and Aref.shape == Mref.shape == A.shape[1:]
    T = lref.phase_lock(Aref, F_out, spo, Mref, reset_below, return_rotation=True)[1]       # (bins, F_out) uint32
    i0, _ = positions(F_out, spo, A.shape[-1])
    return angle_of(T[None] + q(A)[..., i0])                                                # uint32 + uint32 wraps


def stereo_melody(sr=16000, seconds=6.0):
    """The notes of _vocoder_ref.melody, each at a pan position of its own (constant power) and delayed by up to 11 samples in the
    right channel, plus 1e-4 * randn per channel: float32 (2, samples)."""
    rs = np.random.RandomState(3)
    n = int(round(sr * seconds))
    t = np.arange(n, dtype=np.float64) / sr
    L, R = np.zeros(n), np.zeros(n)
    for f, t0 in ref.NOTES:
        u = t - t0
        env = np.clip(np.minimum(u / 0.010, (0.6 - u) / 0.050), 0.0, 1.0)
        s = env * (np.sin(2 * np.pi * f * u) + 0.5 * np.sin(4 * np.pi * f * u) + 0.25 * np.sin(6 * np.pi * f * u))
        pan = rs.uniform(0.15, 0.85)
        d = int(rs.randint(0, 12))
        L += np.cos(pan * np.pi / 2) * s
        R += np.sin(pan * np.pi / 2) * np.roll(s, d)
    L += 1e-4 * rs.standard_normal(n)
    R += 1e-4 * rs.standard_normal(n)
    return np.stack([L, R]).astype(np.float32)


def linked_analysis64(x, n_src, n_fft, hop):
    """phasegen.track._analyse_spectral(link=True) in float64 with the track's own moments: the channels (n_ch, samples) and, as row
    n_ch, their mean, zero-filled to n_src samples, STFT without the DC row, (v - mean) / std with the moments of the CHANNELS' real
    and imaginary parts -> (log1p|z|, angle z), (n_ch + 1, bins, F_src) each."""
    x = np.asarray(x, np.float64)
    n_ch = x.shape[0]
    xp = np.zeros((n_ch + 1, n_src))
    n = min(x.shape[1], n_src)
    xp[:n_ch, :n] = x[:, :n]
    xp[n_ch] = xp[:n_ch].mean(0)
    S = ref.stft64(xp, n_fft, hop)
    parts = np.stack([S[:n_ch].real, S[:n_ch].imag])
    mean, std = parts.mean(), parts.std()
    z = (S.real - mean) / std + 1j * ((S.imag - mean) / std)
    return np.log1p(np.abs(z)), np.angle(z)


def mid_consistency64(mid_logmag, n_fft, hop, phase=None, logmag=None, audio=None, floor=1e-10):
    """consistency64 on the mean channel: mid_logmag (bins, F), the imposed magnitudes of the channel mean, against the mean over
    the channels of an output -- ``audio`` (n_ch, hop (F - 1)), or the float64 ISTFT of ``logmag`` (n_ch, bins, F) under ``phase``."""
    if audio is None:
        audio = ref.istft64(np.expm1(np.asarray(logmag, np.float64)) * np.exp(1j * np.asarray(phase, np.float64)), n_fft, hop)
    audio = np.asarray(audio, np.float64)
    return ref.consistency64(np.asarray(mid_logmag)[None], n_fft, hop, audio=audio.mean(0, keepdims=True), floor=floor)


def ipd_error(ph, A, logmag_out, spo):
    """ph (2, bins, F_out): an output phase; A (2, bins, F_src): the analysis' angle planes; logmag_out (2, bins, F_out): the
    magnitudes on the output grid -> the rms over all cells, weighted by the product of the two linear magnitudes, of
    angle_of(q(ph_L) - q(ph_R) - (q(A_L) - q(A_R))[i0]) in radians."""
    ph, A = np.asarray(ph, np.float32), np.asarray(A, np.float32)
    i0, _ = positions(ph.shape[-1], spo, A.shape[-1])
    qa = q(A)
    d = angle_of(q(ph[0]) - q(ph[1]) - (qa[0] - qa[1])[..., i0]).astype(np.float64)
    lin = np.expm1(np.asarray(logmag_out, np.float64))
    w = lin[0] * lin[1]
    return float(np.sqrt((w * d * d).sum() / w.sum()))
