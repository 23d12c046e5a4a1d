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
"""
import numpy as np
import torch

from . import audio as pg_audio
from . import ops, preproc
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


def reconstruct_track(model, audio, n_fft=2048, hop_length=512, frames=128, overlap_frames=32, stats=None,
                      osr=None, sr=16000, res_type="kaiser_best", clip_batch=64, phase="unet", normalize=True):
    """audio (samples,) or (channels, samples), host array or device tensor, at ``sr`` -- or at ``osr`` when given (resampled to
    ``sr`` first) -> float32 device tensor of the same shape with the a_len samples per channel of the track at ``sr``, its phase
    predicted by ``model`` (phase="unet") or kept from the analysis (phase="original", ``model`` may be None: the chunk / stitch
    round trip).  ``stats`` = (mean, std) of the training set; None: the track's own moments.  ``normalize``: peak-normalise over
    all channels jointly (utils.py:42 for the whole track).  Raises ValueError("Audio buffer is not finite everywhere") as
    ``audio.generate_audio`` does."""
    if phase not in ("unet", "original"):
        raise ValueError(f"reconstruct_track: phase must be 'unet' or 'original', got {phase!r}")
    if phase == "unet" and model is None:
        raise ValueError("reconstruct_track: phase='unet' needs a model")
    if clip_batch < 1:
        raise ValueError("reconstruct_track: clip_batch must be positive")
    if osr is not None:
        a = preproc.resample(audio, osr, sr, res_type=res_type)
    elif torch.is_tensor(audio):
        a = audio.to(audio.device if audio.is_cuda else preproc._device_of(None), torch.float32)
    else:
        a = torch.from_numpy(np.ascontiguousarray(audio, dtype=np.float32)).to(preproc._device_of(None))
    if a.dim() not in (1, 2):
        raise ValueError(f"reconstruct_track: audio must be (samples,) or (channels, samples), got {tuple(a.shape)}")
    mono = a.dim() == 1
    a2 = (a[None] if mono else a).contiguous()
    n_ch, a_len = a2.shape
    T, step, n_clips = track_plan(a_len, frames, hop_length, overlap_frames)
    bins = n_fft // 2
    dev = a2.device
    with torch.cuda.device(dev), torch.no_grad():
        # signal order (clip, channel), as preproc.chunk_audio
        st = torch.tensor(np.repeat(np.arange(n_clips, dtype=np.int64) * step, n_ch), device=dev)
        rows = torch.tensor(np.tile(np.arange(n_ch, dtype=np.int32), n_clips), device=dev)
        x = ops.stft(a2, n_fft, hop_length, chunk_start=st, chunk_row=rows, chunk_len=T)      # (n_clips * n_ch, 2, bins, frames)
        if stats is None:
            ops.standardize_(x)
        else:
            ops.standardize_with_(x, stats[0], stats[1])
        pol = ops.polar(x)
        logmag = pol[:, 0]
        if phase == "unet":
            ph = torch.empty(n_clips * n_ch, bins, frames, device=dev)
            for i in range(0, n_clips * n_ch, clip_batch):
                ph[i:i + clip_batch] = model.forward(logmag[i:i + clip_batch], per_clip=True)[:, :bins]
        else:
            ph = pol[:, 1]
        clips = pg_audio.synthesize(logmag, ph, hop_length, normalize=False)                   # (n_clips * n_ch, T)
        out, _, bad = ops.stitch(clips.view(n_clips, n_ch, T).transpose(0, 1), step, a_len, normalize=normalize, return_status=True)
        if int(bad.item()) != 0:
            raise ValueError("Audio buffer is not finite everywhere")       # librosa.util.valid_audio's ParameterError
    return out[0] if mono else out
