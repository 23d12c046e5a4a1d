"""numpy / torch-CPU restatements for the phase-vocoder tests (no GPU, no phasegen import).

  phase_vocoder    pg_phase_vocoder's contract (include/phasegen.h) word for word: np.rint on a double product, uint32 wrap-around
                   sums, a plain Python loop over the output frames.  The device must reproduce it BIT FOR BIT.
  consistency64    phasegen.metrics.consistency's whole chain in float64 with torch.stft / torch.istft on the CPU: periodic Hann,
                   center=True, reflect padding, the DC row dropped from the analysis and zero-prepended for the synthesis.
  melody, analysis64, stretch64   the synthetic melody of the ordering tests and the float64 analysis / resampling around it.
"""
import math

import numpy as np
import torch

TWO_PI = 6.283185307179586
K = 4294967296.0 / TWO_PI
R = TWO_PI / 4294967296.0


def q(x):
    """float32 array -> uint32: 0 where x is not finite or |x| > 2^20, else (uint32)(int64) rint((double)x * K)."""
    x = np.asarray(x, np.float32)
    ok = np.isfinite(x) & (np.abs(x) <= np.float32(2.0 ** 20))
    r = np.rint(np.where(ok, x, np.float32(0)).astype(np.float64) * K)
    return r.astype(np.int64).astype(np.uint32)                          # two's-complement wrap


def positions(F_out, src_per_out, F_src):
    """(i0, i1) of every output frame: pg_spec_clips's positions."""
    p = np.arange(F_out, dtype=np.float64) * float(src_per_out)
    i0 = np.minimum(np.floor(p), F_src - 1).astype(np.int64)
    return i0, np.minimum(i0 + 1, F_src - 1)


def angle_of(acc):
    """uint32 -> float32 in [-pi, pi]: (float)((double)(int32)acc * R)."""
    return (np.asarray(acc, np.uint32).view(np.int32).astype(np.float64) * R).astype(np.float32)


def phase_vocoder(A, F_out, src_per_out, M=None, reset_below=0.0):
    """A (..., F_src) float32, M None or like A -> (..., F_out) float32, frame after frame."""
    A = np.asarray(A, np.float32)
    F_src = A.shape[-1]
    i0, i1 = positions(F_out, src_per_out, F_src)
    qA = q(A)
    floor = np.float32(reset_below)
    out = np.empty(A.shape[:-1] + (F_out,), np.float32)
    acc = np.zeros(A.shape[:-1], np.uint32)
    delta = np.zeros(A.shape[:-1], np.uint32)
    for g in range(F_out):
        if g == 0:
            reset = np.ones(A.shape[:-1], bool)
        elif M is None:
            reset = np.zeros(A.shape[:-1], bool)
        else:
            reset = np.asarray(M, np.float32)[..., i0[g]] < floor         # (False for a NaN)
        acc = np.where(reset, qA[..., i0[g]], acc + delta)               # uint32 + uint32 wraps
        delta = qA[..., i1[g]] - qA[..., i0[g]]
        out[..., g] = angle_of(acc)
    return out


# ---- consistency in float64 ----------------------------------------------------------------------------------------------

def _window(n_fft):
    return torch.hann_window(n_fft, periodic=True, dtype=torch.float64)


def stft64(x, n_fft, hop):
    """(n, samples) float64 -> complex (n, n_fft / 2, 1 + samples // hop): the DC row dropped, like the project's STFT."""
    S = torch.stft(torch.as_tensor(np.asarray(x, np.float64)), n_fft, hop, window=_window(n_fft), center=True, pad_mode="reflect",
                   return_complex=True)
    return S[:, 1:n_fft // 2 + 1].numpy()


def istft64(Z, n_fft, hop):
    """complex (n, n_fft / 2, F) without a DC row -> (n, hop * (F - 1)) float64."""
    Z = np.asarray(Z, np.complex128)
    full = np.concatenate([np.zeros((Z.shape[0], 1, Z.shape[2]), np.complex128), Z], 1)
    return torch.istft(torch.from_numpy(full), n_fft, hop, window=_window(n_fft), center=True, length=hop * (Z.shape[2] - 1)).numpy()


def consistency64(logmag, n_fft, hop, phase=None, audio=None, floor=1e-10):
    """logmag (n_ch, bins, F) and either the phase imposed on it (the ISTFT runs here, in float64) or the ISTFT output itself
    (n_ch, hop * (F - 1)) -> {"spectral_convergence", "lsd_db", "n_frames", "channels"} over the frames [e, F - e),
    e = ceil(n_fft / (2 hop))."""
    logmag = np.asarray(logmag, np.float64)
    n_ch, bins, F = logmag.shape
    mR = np.expm1(logmag)
    if audio is None:
        audio = istft64(mR * np.exp(1j * np.asarray(phase, np.float64)), n_fft, hop)
    audio = np.asarray(audio, np.float64)
    assert audio.shape == (n_ch, hop * (F - 1)), audio.shape
    mE = np.abs(stft64(audio, n_fft, hop))
    e = -(-n_fft // (2 * hop))
    assert F > 2 * e
    mR, mE = mR[:, :, e:F - e], mE[:, :, e:F - e]
    level = lambda m: 10.0 * np.log10(np.maximum(m * m, floor))
    d = level(mR) - level(mE)
    return {"spectral_convergence": math.sqrt(((mR - mE) ** 2).sum() / (mR ** 2).sum()),
            "lsd_db": float(np.sqrt((d ** 2).mean(axis=1)).mean()),
            "n_frames": F - 2 * e, "channels": n_ch}


# ---- the melody of the ordering tests -------------------------------------------------------------------------------------

NOTES = ((440, 0.5), (494, 1.0), (523, 1.5), (587, 2.0), (659, 2.5), (440, 3.0), (330, 3.0), (262, 3.6), (392, 4.2), (523, 4.8))


def melody(sr=16000, seconds=6.0, seed=0):
    """Ten notes of 0.6 s, each sin(2 pi f t) + 0.5 sin(4 pi f t) + 0.25 sin(6 pi f t) under a 10 ms linear attack and a 50 ms linear
    release, plus 1e-4 * randn: float32 (samples,)."""
    n = int(round(sr * seconds))
    t = np.arange(n, dtype=np.float64) / sr
    x = np.zeros(n)
    for f, t0 in NOTES:
        u = t - t0
        env = np.clip(np.minimum(u / 0.010, (0.6 - u) / 0.050), 0.0, 1.0)
        x += env * (np.sin(2 * np.pi * f * u) + 0.5 * np.sin(4 * np.pi * f * u) + 0.25 * np.sin(6 * np.pi * f * u))
    x += 1e-4 * np.random.RandomState(seed).standard_normal(n)
    return x.astype(np.float32)


def analysis64(x, n_src, n_fft, hop):
    """The track's analysis in float64 with its own moments (phasegen.track._analyse_spectral): the track (n_ch, samples) zero-filled
    to n_src samples, STFT without the DC row, (v - mean) / std over all real and imaginary parts, -> (log1p|z|, angle z)."""
    x = np.asarray(x, np.float64)
    xp = np.zeros((x.shape[0], n_src))
    n = min(x.shape[1], n_src)
    xp[:, :n] = x[:, :n]
    S = stft64(xp, n_fft, hop)
    parts = np.stack([S.real, S.imag])
    mean, std = parts.mean(), parts.std()
    z = (S.real - mean) / std + 1j * ((S.imag - mean) / std)
    return np.log1p(np.abs(z)), np.angle(z)


def resample64(P, F_out, src_per_out):
    """pg_spec_clips's whole-plane form in float64: P (..., F_src) at the positions g * src_per_out, linearly interpolated."""
    P = np.asarray(P, np.float64)
    i0, i1 = positions(F_out, src_per_out, P.shape[-1])
    p = np.arange(F_out, dtype=np.float64) * float(src_per_out)
    w = (p - np.floor(p)).astype(np.float32).astype(np.float64)
    return np.where(w == 0, P[..., i0], P[..., i0] + w * (P[..., i1] - P[..., i0]))
