"""Whole-track phase reconstruction: a recording of any length goes through the model as overlapped clips of ``frames`` columns
and comes back as one signal.  The reference stops at dataset clips (demo.py:33-45); what is added here is the plan of the clip
starts, the training set's (x - mean) / std applied to new audio, and the crossfaded join (pg_stitch).  Every stage runs on the
device:

  resample       preproc.resample (pg_resample), when the audio is not at the model's rate
  chunk + STFT   ONE ops.stft launch over all (clip, channel) pairs reading the track in place (chunk_start / chunk_row); clip k
                 begins at sample k * step, step a multiple of hop, so clip frames lie on the track's global hop grid; the last
                 clip's tail reads as zero
  standardise    (x - mean) / std with the training set's statistics (``build_dataset(..., return_stats=True)``) or, without
                 them, with this track's own moments
  polar          data.py:39-47, [log1p|z| ; angle]
  forward        ``model.forward(..., per_clip=True)`` in batches of ``clip_batch`` clips, in clip order: the BatchNorm running
                 buffers end as after the reference's one-clip-at-a-time loop
  ISTFT          audio.synthesize, un-normalised clips of T = hop * (frames - 1) samples
  stitch         ops.stitch: sin^2 crossfade over the overlap, finite check and peak normalisation over the whole result

``evaluate_track`` runs the analysis once, synthesises the track from several phase sources (the model's, none at all, the
analysis' own, Griffin-Lim's) and reports ``metrics.compare_audio`` of each against the input.
"""
import numpy as np
import torch

from . import audio as pg_audio
from . import metrics, ops, preproc
from .unet import frame_plan


def track_plan(a_len, frames, hop_length, overlap_frames):
    """(T, step, n_clips) for a track of ``a_len`` samples: clips of T = hop * (frames - 1) samples that begin ``step`` = T -
    overlap_frames * hop apart; one clip while a_len <= T, else 1 + ceil((a_len - T) / step).  At most two clips may cover a
    sample: 0 <= 2 * overlap_frames <= frames - 1."""
    a_len, frames, hop_length, overlap_frames = int(a_len), int(frames), int(hop_length), int(overlap_frames)
    frame_plan(frames)                                           # ValueError for frame counts the U-Net cannot concatenate
    if a_len < 1 or hop_length < 1:
        raise ValueError(f"track_plan: a_len {a_len} and hop_length {hop_length} must be positive")
    if not 0 <= 2 * overlap_frames <= frames - 1:
        raise ValueError(f"track_plan: overlap_frames {overlap_frames} must satisfy 0 <= 2 * overlap_frames <= frames - 1 = {frames - 1}")
    T = hop_length * (frames - 1)
    step = T - overlap_frames * hop_length
    n_clips = 1 if a_len <= T else 1 + -(-(a_len - T) // step)
    return T, step, n_clips


PHASES = ("unet", "zero", "original", "griffinlim")


class _Analysis:
    """What every phase source shares: the track at ``sr`` (a2: (channels, a_len)), the clip plan and the clips' [log1p|z| ; angle]."""
    __slots__ = ("a2", "mono", "n_ch", "a_len", "T", "step", "n_clips", "bins", "pol")


def _analyse(audio, n_fft, hop_length, frames, overlap_frames, stats, osr, sr, res_type):
    """resample -> chunked STFT -> standardise -> polar, once per track."""
    if osr is not None:
        a = preproc.resample(audio, osr, sr, res_type=res_type)
    elif torch.is_tensor(audio):
        a = audio.to(audio.device if audio.is_cuda else preproc._device_of(None), torch.float32)
    else:
        a = torch.from_numpy(np.ascontiguousarray(audio, dtype=np.float32)).to(preproc._device_of(None))
    if a.dim() not in (1, 2):
        raise ValueError(f"reconstruct_track: audio must be (samples,) or (channels, samples), got {tuple(a.shape)}")
    an = _Analysis()
    an.mono = a.dim() == 1
    an.a2 = a2 = (a[None] if an.mono else a).contiguous()
    an.n_ch, an.a_len = n_ch, a_len = a2.shape
    an.T, an.step, an.n_clips = T, step, n_clips = track_plan(a_len, frames, hop_length, overlap_frames)
    an.bins = n_fft // 2
    dev = a2.device
    with torch.cuda.device(dev), torch.no_grad():
        # signal order (clip, channel), as preproc.chunk_audio
        starts = np.repeat(np.arange(n_clips, dtype=np.int64) * step, n_ch)
        chans = np.tile(np.arange(n_ch, dtype=np.int64), n_clips)
        if stats is not None:
            # the training set's statistics: STFT, standardisation and polar in ONE launch (pg_stft_crops; the same bits as the three
            # calls below).  Channel c is the region [c a_len, (c + 1) a_len) of the flat buffer.
            begin = torch.from_numpy(chans * a_len + starts).to(dev)
            end = torch.from_numpy((chans + 1) * a_len).to(dev)
            an.pol = ops.stft_crops(a2.reshape(-1), begin, end, T, n_fft, hop_length, polar=True, stats=(stats[0], stats[1]))
            return an
        # the track's own moments need the unnormalised tensor: three launches
        st, rows = torch.from_numpy(starts).to(dev), torch.from_numpy(chans.astype(np.int32)).to(dev)
        x = ops.stft(a2, n_fft, hop_length, chunk_start=st, chunk_row=rows, chunk_len=T)      # (n_clips * n_ch, 2, bins, frames)
        ops.standardize_(x)
        an.pol = ops.polar(x)
    return an


def _clips(an, model, phase, hop_length, clip_batch, gl_iters=250, gl_seed=0):
    """Un-normalised clip audio (n_clips * n_ch, T) of one phase source."""
    logmag = an.pol[:, 0]
    n_sig, bins, frames = logmag.shape
    if phase == "griffinlim":
        n_fft = 2 * bins
        return pg_audio.griffin_lim_batch(torch.exp(logmag) - 1.0, n_fft, hop_length, gl_iters, seed=gl_seed, normalize=False)[0]
    if phase == "unet":
        ph = torch.empty(n_sig, bins, frames, device=logmag.device)
        for i in range(0, n_sig, clip_batch):
            ph[i:i + clip_batch] = model.forward(logmag[i:i + clip_batch], per_clip=True)[:, :bins]
    elif phase == "zero":
        ph = torch.zeros_like(logmag)
    else:
        ph = an.pol[:, 1]
    return pg_audio.synthesize(logmag, ph, hop_length, normalize=False)


def _synthesise(an, model, phase, hop_length, clip_batch, normalize, gl_iters=250, gl_seed=0):
    """One phase source -> the stitched track (channels, a_len); raises when a sample is not finite."""
    with torch.cuda.device(an.a2.device), torch.no_grad():
        clips = _clips(an, model, phase, hop_length, clip_batch, gl_iters, gl_seed)            # (n_clips * n_ch, T)
        out, _, bad = ops.stitch(clips.view(an.n_clips, an.n_ch, an.T).transpose(0, 1), an.step, an.a_len, normalize=normalize, return_status=True)
        if int(bad.item()) != 0:
            raise ValueError("Audio buffer is not finite everywhere")       # librosa.util.valid_audio's ParameterError
    return out


def peak_normalize(audio):
    """utils.py:42 for a whole track on the device: audio (samples,) or (channels, samples) divided by its joint peak -- the second
    launch of pg_stitch over one clip per channel, so ``peak_normalize(reconstruct_track(..., normalize=False))`` has the bits of
    ``reconstruct_track(..., normalize=True)``."""
    a2 = audio[None] if audio.dim() == 1 else audio
    n = a2.shape[1]
    with torch.cuda.device(a2.device):
        out = ops.stitch(a2[:, None, :], n, n, normalize=True)
    return out[0] if audio.dim() == 1 else out


def reconstruct_track(model, audio, n_fft=2048, hop_length=512, frames=128, overlap_frames=32, stats=None,
                      osr=None, sr=16000, res_type="kaiser_best", clip_batch=64, phase="unet", normalize=True):
    """audio (samples,) or (channels, samples), host array or device tensor, at ``sr`` -- or at ``osr`` when given (resampled to
    ``sr`` first) -> float32 device tensor of the same shape with the a_len samples per channel of the track at ``sr``, its phase
    predicted by ``model`` (phase="unet"), kept from the analysis (phase="original": the chunk / stitch round trip) or all zero
    (phase="zero", the reference's "no phase" comparator); ``model`` may be None for the last two.  ``stats`` = (mean, std) of the
    training set; None: the track's own moments.  ``normalize``: peak-normalise over all channels jointly (utils.py:42 for the whole
    track).  Raises ValueError("Audio buffer is not finite everywhere") as ``audio.generate_audio`` does."""
    if phase not in ("unet", "original", "zero"):
        raise ValueError(f"reconstruct_track: phase must be 'unet', 'original' or 'zero', got {phase!r}")
    if phase == "unet" and model is None:
        raise ValueError("reconstruct_track: phase='unet' needs a model")
    if clip_batch < 1:
        raise ValueError("reconstruct_track: clip_batch must be positive")
    an = _analyse(audio, n_fft, hop_length, frames, overlap_frames, stats, osr, sr, res_type)
    out = _synthesise(an, model, phase, hop_length, clip_batch, normalize)
    return out[0] if an.mono else out


def evaluate_track(model, audio, n_fft=2048, hop_length=512, frames=128, overlap_frames=32, stats=None, osr=None, sr=16000,
                   res_type="kaiser_best", clip_batch=64, phases=("unet", "zero", "original"), gl_iters=250, gl_seed=0, floor=1e-10,
                   return_audio=False):
    """The quality report of a track: ONE analysis (as ``reconstruct_track``), then for every entry of ``phases`` -- "unet" (the
    model's phase), "zero" (none), "original" (the analysis' own: what the chunk / stitch round trip alone costs), "griffinlim"
    (``audio.griffin_lim_batch`` on exp(logmag) - 1 per clip, ``gl_iters`` iterations from noise seeded ``gl_seed`` + clip index) --
    the un-normalised stitched track and ``metrics.compare_audio(input at sr, track, n_fft, hop_length, floor)``.
    -> {"n_samples", "sr", "n_clips", "metrics": {phase: dict}} and, with ``return_audio``, "audio": {phase: device tensor shaped
    like the input}.  The "unet" audio has the bits of ``reconstruct_track(..., normalize=False)``.  ``model`` may be None when
    "unet" is not asked for."""
    phases = tuple(phases)
    for p in phases:
        if p not in PHASES:
            raise ValueError(f"evaluate_track: unknown phase {p!r} (expected some of {PHASES})")
    if len(set(phases)) != len(phases) or not phases:
        raise ValueError("evaluate_track: phases must be a non-empty list without repetitions")
    if "unet" in phases and model is None:
        raise ValueError("evaluate_track: phase 'unet' needs a model")
    if clip_batch < 1:
        raise ValueError("evaluate_track: clip_batch must be positive")
    an = _analyse(audio, n_fft, hop_length, frames, overlap_frames, stats, osr, sr, res_type)
    ref = an.a2[0] if an.mono else an.a2
    res = {"n_samples": int(an.a_len), "sr": int(sr), "n_clips": int(an.n_clips), "metrics": {}}
    if return_audio:
        res["audio"] = {}
    for p in phases:
        out = _synthesise(an, model, p, hop_length, clip_batch, False, gl_iters, gl_seed)
        out = out[0] if an.mono else out
        res["metrics"][p] = metrics.compare_audio(ref, out, n_fft, hop_length, floor)
        if return_audio:
            res["audio"][p] = out
    return res
