"""How good is a reconstruction?  Scale-invariant waveform and spectral distances between a reference signal and an estimate,
reduced on the device (pg_wave_compare, pg_spec_compare) -- a yardstick that can be asked of a whole track, unlike
``phasegen.validate``'s reference-faithful MSE / NOPMSE / LMSE of three dataset clips (which stay as they are).

  si_sdr_db             Le Roux et al., "SDR -- half-baked or well done?" (2019): with the optimal scaling g = <x, y> / <y, y> of the
                        estimate and q = |x - g y|^2 / |x|^2, SI-SDR = 10 log10((1 - q) / q) = rho^2 / (1 - rho^2) in dB
  snr_db                -10 log10 q, the gain-matched SNR
  spectral_convergence  sqrt(sum (mR - g_m mE)^2 / sum mR^2) over the STFT magnitudes, g_m = <mR, mE> / <mE, mE>: the gain is
                        taken in the MAGNITUDE domain on purpose -- the waveform gain of a zero-phase reconstruction is about -0.07,
                        which would scale the estimate away and pin the figure near 1 whatever the spectrum looks like
  lsd_db                log-spectral distance: mean over frames of the rms over bins of the difference of the levels
                        10 log10(max(m^2, floor)), with the estimate scaled by g_m; floor = 1e-10 is librosa.power_to_db's amin

``consistency`` needs no reference signal (a time-stretched track has none): it compares the magnitudes that were imposed on an ISTFT
with the spectrogram of what came out, by the same spectral convergence and log-spectral distance at gain 1.
"""
import math

import numpy as np
import torch

from . import ops, preproc

KEYS = ("si_sdr_db", "snr_db", "gain", "spectral_convergence", "lsd_db", "mag_gain", "max_abs_error", "n_samples", "n_frames", "channels")


def _signal(a, name):
    if torch.is_tensor(a):
        t = a.to(a.device if a.is_cuda else preproc._device_of(None), torch.float32)
    else:
        t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(preproc._device_of(None))
    if t.dim() not in (1, 2):
        raise ValueError(f"compare_audio: {name} must be (samples,) or (channels, samples), got {tuple(t.shape)}")
    return (t[None] if t.dim() == 1 else t).contiguous()


def _ratio(num, den):
    """num / den where den > 0, else 0 -- on the device."""
    return torch.where(den > 0, num / torch.where(den > 0, den, torch.ones_like(den)), torch.zeros_like(den))


def _db(v):
    return math.inf if v == math.inf else (-math.inf if v <= 0 else 10.0 * math.log10(v))


def consistency(logmag, audio, n_fft, hop_length, floor=1e-10):
    """Spectrogram consistency, the reference-free measure of the phase-retrieval literature: how far |STFT(ISTFT(imposed
    magnitudes, some phase))| lands from the imposed magnitudes.  ``logmag`` (n_ch, bins, F) float32 device tensor: the log1p
    magnitude plane that was imposed (bins = n_fft / 2, the DC row dropped); ``audio`` (n_ch, hop_length * (F - 1)): the ISTFT output
    BEFORE any trimming.  E = ops.stft(audio), R = [expm1(logmag); 0] in the same layout; both are cut to the frames [e, F - e),
    e = ceil(n_fft / (2 hop_length)) -- those whose window does not reach the reflect padding -- and compared by ONE
    ops.spec_compare with gain 1, summed over the channels.
    -> {"spectral_convergence": sqrt(sum (mR - mE)^2 / sum mR^2), "lsd_db", "n_frames": F - 2 e, "channels"}, formed as
    ``compare_audio`` forms them.  ValueError: F <= 2 e; "Audio buffer is not finite everywhere" when a cell of either is not finite."""
    n_fft, hop_length = int(n_fft), int(hop_length)
    if not (torch.is_tensor(logmag) and logmag.is_cuda and logmag.dtype == torch.float32 and logmag.dim() == 3):
        raise ValueError("consistency: logmag must be a 3-D float32 device tensor (n_ch, bins, F)")
    n_ch, bins, F = logmag.shape
    if n_fft < 2 or hop_length < 1 or bins != n_fft // 2:
        raise ValueError(f"consistency: logmag has {bins} bins, n_fft {n_fft} (hop {hop_length}) needs {n_fft // 2}")
    if not (torch.is_tensor(audio) and audio.is_cuda and audio.dtype == torch.float32 and tuple(audio.shape) == (n_ch, hop_length * (F - 1))):
        raise ValueError(f"consistency: audio must be the untrimmed ISTFT output, a float32 device tensor {(n_ch, hop_length * (F - 1))}")
    e = -(-n_fft // (2 * hop_length))
    if F <= 2 * e:
        raise ValueError(f"consistency: {F} frames leave none whose window stays clear of the padding (need more than {2 * e})")
    with torch.cuda.device(logmag.device), torch.no_grad():
        E = ops.stft(audio.contiguous(), n_fft, hop_length)[:, :, :, e:F - e].contiguous()   # (n_ch, 2, bins, F - 2 e)
        R = torch.zeros_like(E)
        R[:, 0] = torch.expm1(logmag[:, :, e:F - e])
        s = ops.spec_compare(R, E, floor=floor).sum(0)
        smm, serr, lsd_sum, bad = s[[0, 3, 4, 5]].cpu().tolist()
    if bad != 0:
        raise ValueError("Audio buffer is not finite everywhere")
    n_frames = F - 2 * e
    return {
        "spectral_convergence": math.sqrt(serr / smm) if smm > 0 else (0.0 if serr == 0 else math.inf),
        "lsd_db": lsd_sum / (n_ch * n_frames),
        "n_frames": int(n_frames),
        "channels": int(n_ch),
    }


def compare_audio(ref, est, n_fft=2048, hop_length=512, floor=1e-10):
    """ref, est: (samples,) or (channels, samples) of equal shape, host arrays or device tensors -> dict of ``KEYS``.  The metrics
    are taken over all channels jointly, with ONE gain (the peak normalisation of a track is joint as well).  Four reduction calls
    and two STFTs (whole signal, one launch each) on the device; nothing leaves it before one final copy of the sums.  Raises
    ValueError("Audio buffer is not finite everywhere") when either signal (or its spectrogram) holds a NaN or an infinity."""
    x, y = _signal(ref, "ref"), _signal(est, "est")
    if x.shape != y.shape:
        raise ValueError(f"compare_audio: shapes differ: ref {tuple(x.shape)}, est {tuple(y.shape)}")
    if x.device != y.device:
        y = y.to(x.device)
    n_ch, n = x.shape
    with torch.cuda.device(x.device), torch.no_grad():
        w0 = ops.wave_compare(x, y).sum(0)
        g = _ratio(w0[2], w0[1])
        w1 = ops.wave_compare(x, y, gain=g)
        R = ops.stft(x, n_fft, hop_length)
        E = ops.stft(y, n_fft, hop_length)
        s0 = ops.spec_compare(R, E, floor=floor).sum(0)
        gm = _ratio(s0[2], s0[1])
        s1 = ops.spec_compare(R, E, gain=gm, floor=floor)
        n_frames = R.shape[3]
        del R, E
        ws, ss = w1.sum(0), s1.sum(0)
        host = torch.stack([ws[0], ws[3], w1[:, 4].max(), ws[5] + w0[5], g, ss[0], ss[3], ss[4], ss[5] + s0[5], gm]).cpu().tolist()
    sxx, err, max_err, bad_w, gain, smm, serr, lsd_sum, bad_s, mag_gain = host
    if bad_w != 0 or bad_s != 0:
        raise ValueError("Audio buffer is not finite everywhere")
    q = err / sxx if sxx > 0 else (0.0 if err == 0 else math.inf)
    return {
        "si_sdr_db": math.inf if q == 0 else (-math.inf if q >= 1 else _db((1.0 - q) / q)),
        "snr_db": math.inf if q == 0 else 0.0 - _db(q),
        "gain": gain,
        "spectral_convergence": math.sqrt(serr / smm) if smm > 0 else (0.0 if serr == 0 else math.inf),
        "lsd_db": lsd_sum / (n_ch * n_frames),
        "mag_gain": mag_gain,
        "max_abs_error": max_err,
        "n_samples": int(n),
        "n_frames": int(n_frames),
        "channels": int(n_ch),
    }
