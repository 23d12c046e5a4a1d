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

``join="spectral"`` joins the clips on the track's global FRAME grid instead (clip k = frames k sf .. k sf + frames - 1, sf = step /
hop): ONE whole-track STFT per channel (ops.stft_crops), clip windows of its log-magnitude plane (ops.spec_clips), the same forward,
ONE phase per frame (ops.phase_join: where two clips overlap, the circular mean of their phases under the stitch's ramp), ONE ISTFT
with the plane's exact magnitudes.  ``stretch`` resamples the magnitudes along time in the same kernel (the result is ``stretch``
times as long at the same pitch) and ``pitch_shift`` resamples that back (same length, other pitch).  ``spectral_plan`` is the plan.

``evaluate_track`` runs the analysis once, synthesises the track from several phase sources (the model's, none at all, the
analysis' own, Griffin-Lim's) and reports ``metrics.compare_audio`` of each against the input.

phase="vocoder" (spectral join) is the phase vocoder, the comparator of every time-stretch method: the analysis' own phase carried
along the output frames by its measured advance (ops.phase_vocoder); it needs no model.  phase="vocoder_locked" is that vocoder with
identity phase locking (ops.phase_lock: only the peaks of a frame advance, every other bin follows its peak).  A stretched track has
no reference waveform, so ``evaluate_stretch`` reports ``metrics.consistency`` instead: how far the spectrogram of each phase source's result
lands from the magnitudes that were imposed.  On its own that locking works per channel, each with its own peaks and its own
rotation, so the phases of one source in two channels drift apart; ``link_channels=True`` gives all channels ONE rotation, that of
the channel mean (ops.phase_lock_linked), so the analysis' inter-channel phase differences -- the stereo image, and how the channels
sum to mono -- survive the stretch, and ``evaluate_stretch`` then also reports the consistency of the channel mean ("mid_metrics").

phase="spsi" (spectral join) is single-pass spectrogram inversion (ops.phase_spsi): a phase from the output grid's magnitudes ALONE
-- peaks advance by their interpolated frequency, every other bin follows its peak -- with no analysis phase, no weights and no
iteration: the baseline a predicted phase has to beat, and the only comparator that uses nothing a stretched spectrogram lacks.
``evaluate_track(gl_init="spsi")`` starts Griffin-Lim from it instead of from noise.

``transients="ola"`` (spectral join) keeps the clicks of a stretched track clicks (Driedger, Mueller & Ewert 2014).  Resampling the
magnitudes along time spreads every onset over ``stretch`` times as many frames, and no phase can put it back together.  With the
option the log-magnitude plane is split by median filtering into a harmonic and a percussive plane (ops.hpss, ``HPSS_WIN``); the
harmonic plane goes through the chosen phase source exactly as the whole plane does without the option, the percussive plane is
inverted on the SOURCE grid with the analysis' own phase and moved to the output grid in the time domain by overlap-add of a short
window (ops.ola_stretch, ``TRANSIENT_WINDOW`` / ``TRANSIENT_HOP``), which relocates transients instead of stretching them.

``stretch`` may be a ``TimeMap`` wherever it may be a number: a tempo map, a time-varying stretch given by anchors (source seconds,
output seconds) and piecewise linear between them.  ``TimeMap.plan`` is ``spectral_plan`` for it and holds one source position per
output frame (and one source centre per overlap-add grain); the tables go to the device once per call and every stretch kernel
reads them instead of the one rate (``pos=`` of ops.spec_clips, phase_vocoder, phase_lock, phase_lock_linked, ola_stretch).

``pitch_shift`` takes a ``PitchCurve`` wherever it takes a number of semitones: a transposition given by anchors (seconds,
semitones), piecewise linear between them.  ``PitchCurve.plan`` turns it into a tempo map for the stretch (every 256 samples at the
stretch 2 ** (semitones / 12) of their midpoint) and into the position and bandwidth tables of the variable-rate resampler that plays
the stretched track back (ops.varispeed), block by block of 64 samples, so that the result has the input's length and tempo.

``detect_pitch`` measures what a curve is drawn against: the fundamental frequency of a monophonic take, frame by frame (YIN on the
device, ops.pitch_track), as a ``PitchTrack`` of host arrays.  ``PitchCurve.correcting`` turns a track into the curve that pulls
every voiced frame to the nearest degree of a scale, and ``autotune`` is the three in a row: detect, correct, ``pitch_shift``.
"""
import collections
import fractions
import functools
import inspect
import math

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
REPORT_PHASES = PHASES + ("spsi",)                                # what evaluate_track reports ("spsi": spectral join only)
GL_INITS = ("noise", "spsi")


class _Analysis:
    """What every phase source shares: the track at ``sr`` (a2: (channels, a_len)), the clip plan and the clips' [log1p|z| ; angle]."""
    __slots__ = ("a2", "mono", "n_ch", "a_len", "T", "step", "n_clips", "bins", "pol", "plan", "stretch", "link", "pos", "grains")


def _load(audio, osr, sr, res_type):
    """The track at ``sr`` on the device, as an _Analysis with a2, mono, n_ch and a_len set."""
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
    an.link = False
    an.pos = an.grains = None
    an.a2 = (a[None] if an.mono else a).contiguous()
    an.n_ch, an.a_len = an.a2.shape
    return an


def _analyse(audio, n_fft, hop_length, frames, overlap_frames, stats, osr, sr, res_type):
    """resample -> chunked STFT -> standardise -> polar, once per track."""
    an = _load(audio, osr, sr, res_type)
    a2, n_ch, a_len = an.a2, an.n_ch, an.a_len
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


def _clips(an, model, phase, hop_length, clip_batch, gl_iters=250, gl_seed=0, gl_init="noise"):
    """Un-normalised clip audio (n_clips * n_ch, T) of one phase source."""
    logmag = an.pol[:, 0]
    n_sig, bins, frames = logmag.shape
    if phase == "griffinlim":
        n_fft = 2 * bins
        init = None
        if gl_init == "spsi":                                    # every clip starts from its single-pass inversion instead of noise
            init = ops.istft(logmag, ops.phase_spsi(logmag, n_fft, hop_length), hop_length, mode=0, normalize=False)
        return pg_audio.griffin_lim_batch(torch.exp(logmag) - 1.0, n_fft, hop_length, gl_iters, seed=gl_seed, normalize=False, init=init)[0]
    if phase == "unet":
        ph = torch.empty(n_sig, bins, frames, device=logmag.device)
        for i in range(0, n_sig, clip_batch):
            ph[i:i + clip_batch] = model.forward(logmag[i:i + clip_batch], per_clip=True)[:, :bins]
    elif phase == "zero":
        ph = torch.zeros_like(logmag)
    else:
        ph = an.pol[:, 1]
    return pg_audio.synthesize(logmag, ph, hop_length, normalize=False)


def _synthesise(an, model, phase, hop_length, clip_batch, normalize, gl_iters=250, gl_seed=0, gl_init="noise"):
    """One phase source -> the stitched track (channels, a_len); raises when a sample is not finite."""
    with torch.cuda.device(an.a2.device), torch.no_grad():
        clips = _clips(an, model, phase, hop_length, clip_batch, gl_iters, gl_seed, gl_init)   # (n_clips * n_ch, T)
        out, _, bad = ops.stitch(clips.view(an.n_clips, an.n_ch, an.T).transpose(0, 1), an.step, an.a_len, normalize=normalize, return_status=True)
        if int(bad.item()) != 0:
            raise ValueError("Audio buffer is not finite everywhere")       # librosa.util.valid_audio's ParameterError
    return out


JOINS = ("waveform", "spectral")
SpectralPlan = collections.namedtuple("SpectralPlan", "sf Vf a_out n_clips F_out F_src n_src")


def spectral_plan(a_len, frames, hop_length, overlap_frames, stretch=1.0):
    """The frame-grid plan of the spectral join for a track of ``a_len`` samples played ``stretch`` times as long (host only):
      sf = frames - 1 - overlap_frames     frame stride between clips (``track_plan``'s step / hop)
      Vf = overlap_frames + 1              frames two neighbouring clips share (their edge frames coincide even without overlap)
      a_out = round(a_len * stretch)       output samples;  n_clips = track_plan(a_out, ...)'s
      F_out = (n_clips - 1) * sf + frames  output frames: hop * (F_out - 1) >= a_out samples come out of the ISTFT
      F_src = floor((F_out - 1) / stretch) + 2     source frames, so that F_src - 1 >= (F_out - 1) / stretch: the interpolation's
                                                   upper neighbour exists for every output frame
      n_src = hop * (F_src - 1)            length of the analysed signal, the track zero-filled past a_len
    ValueError: ``stretch`` not finite or outside [0.25, 4], whatever ``track_plan`` raises, 2 * Vf > frames (odd ``frames`` at the
    largest overlap: more than two clips would cover a frame)."""
    stretch = float(stretch)
    if not (stretch == stretch and 0.25 <= stretch <= 4.0):
        raise ValueError(f"spectral_plan: stretch must be finite and within [0.25, 4], got {stretch}")
    a_len, frames, hop_length, overlap_frames = int(a_len), int(frames), int(hop_length), int(overlap_frames)
    if a_len < 1:
        raise ValueError(f"spectral_plan: a_len {a_len} must be positive")
    a_out = int(round(a_len * stretch))
    _T, _step, n_clips = track_plan(a_out, frames, hop_length, overlap_frames)
    sf, Vf = frames - 1 - overlap_frames, overlap_frames + 1
    if 2 * Vf > frames:
        raise ValueError(f"spectral_plan: overlap_frames {overlap_frames} + 1 shared frames exceed half a clip of {frames} frames")
    F_out = (n_clips - 1) * sf + frames
    F_src = int(math.floor((F_out - 1) / stretch)) + 2
    return SpectralPlan(sf, Vf, a_out, n_clips, F_out, F_src, hop_length * (F_src - 1))


MappedPlan = collections.namedtuple("MappedPlan", SpectralPlan._fields + ("pos", "grains"))


class TimeMap:
    """A tempo map: a time-varying stretch, piecewise linear between anchors (host only, float64).  ``anchors``: a sequence of
    (source_seconds, output_seconds) that begins with (0, 0), has at least two entries, is finite and strictly increasing in both
    columns; every segment's stretch (output per source) must lie within [0.25, 4], the domain of a uniform stretch.  Past the last
    anchor the last segment's line continues, so ``TimeMap([(0, 0), (1, R)])`` is the uniform stretch R.  ValueError otherwise.
    ``stretch=`` takes one wherever it takes a number (``reconstruct_track``, ``evaluate_stretch``)."""

    def __init__(self, anchors):
        try:
            a = np.array([[float(v) for v in row] for row in anchors], dtype=np.float64)
        except (TypeError, ValueError) as e:
            raise ValueError(f"TimeMap: anchors must be (source_seconds, output_seconds) pairs ({e})")
        if a.ndim != 2 or a.shape[1] != 2 or a.shape[0] < 2:
            raise ValueError("TimeMap: at least two anchors (source_seconds, output_seconds)")
        if not np.isfinite(a).all():
            raise ValueError("TimeMap: anchors must be finite")
        if a[0, 0] != 0.0 or a[0, 1] != 0.0:
            raise ValueError(f"TimeMap: the first anchor must be (0, 0), got ({a[0, 0]}, {a[0, 1]})")
        d = np.diff(a, axis=0)
        if not (d > 0.0).all():
            raise ValueError("TimeMap: anchors must increase strictly in both columns")
        slopes = d[:, 1] / d[:, 0]
        if not ((slopes >= 0.25) & (slopes <= 4.0)).all():
            raise ValueError(f"TimeMap: every segment's stretch must lie within [0.25, 4], got {slopes.min():g} .. {slopes.max():g}")
        self.src, self.out = a[:, 0].copy(), a[:, 1].copy()
        self.src.setflags(write=False)
        self.out.setflags(write=False)

    @property
    def anchors(self):
        return [(float(s), float(o)) for s, o in zip(self.src, self.out)]

    @property
    def stretches(self):
        """every segment's stretch, output seconds per source second"""
        return np.diff(self.out) / np.diff(self.src)

    def __repr__(self):
        return f"TimeMap({self.anchors!r})"

    @staticmethod
    def _eval(x, xs, ys):
        """y on the segment of x: y_k + (x - x_k) * ((y_{k+1} - y_k) / (x_{k+1} - x_k)): one division per segment, so every anchor
        is hit exactly; from the last anchor on, k is the last anchor and the slope the last segment's"""
        x = np.asarray(x, np.float64)
        k = np.clip(np.searchsorted(xs, x, side="right") - 1, 0, len(xs) - 1)
        slope = (ys[1:] - ys[:-1]) / (xs[1:] - xs[:-1])
        y = ys[k] + (x - xs[k]) * slope[np.minimum(k, len(xs) - 2)]
        return float(y) if y.ndim == 0 else y

    def src_of_out(self, t, sr=16000):
        """the source position, in samples at ``sr``, that plays at output sample ``t`` (a number or an array)"""
        return self._eval(t, self.out * float(sr), self.src * float(sr))

    def out_of_src(self, s, sr=16000):
        """the output position, in samples at ``sr``, at which source sample ``s`` plays"""
        return self._eval(s, self.src * float(sr), self.out * float(sr))

    @classmethod
    def ramp(cls, duration_s, r0, r1, n=64):
        """A stretch that goes linearly from ``r0`` to ``r1`` over ``duration_s`` seconds of source: ``n`` equal segments, each at
        the stretch of its midpoint (past the end the last one continues)."""
        duration_s, r0, r1, n = float(duration_s), float(r0), float(r1), int(n)
        if not (duration_s > 0.0 and duration_s < math.inf) or n < 1:
            raise ValueError(f"TimeMap.ramp: duration_s {duration_s} must be positive and finite and n {n} at least 1")
        if not (0.25 <= r0 <= 4.0 and 0.25 <= r1 <= 4.0):
            raise ValueError(f"TimeMap.ramp: r0 {r0} and r1 {r1} must lie within [0.25, 4]")
        src = duration_s * (np.arange(n + 1, dtype=np.float64) / n)
        r = r0 + (r1 - r0) * ((np.arange(n, dtype=np.float64) + 0.5) / n)
        out = np.concatenate([[0.0], np.cumsum(np.diff(src) * r)])
        return cls(list(zip(src, out)))

    @classmethod
    def load(cls, path):
        """A text file of two columns per line, source seconds and output seconds, separated by blanks or a comma; ``#`` begins a
        comment; empty lines are skipped."""
        anchors = []
        with open(path) as f:
            for n, line in enumerate(f, 1):
                cols = line.split("#", 1)[0].replace(",", " ").split()
                if not cols:
                    continue
                if len(cols) != 2:
                    raise ValueError(f"TimeMap.load: {path}:{n}: expected two columns, got {len(cols)}")
                try:
                    anchors.append((float(cols[0]), float(cols[1])))
                except ValueError:
                    raise ValueError(f"TimeMap.load: {path}:{n}: not two numbers: {line.strip()!r}")
        return cls(anchors)

    def save(self, path):
        with open(path, "w") as f:
            f.write("# source_seconds output_seconds\n")
            for s, o in zip(self.src, self.out):
                f.write(f"{float(s)!r} {float(o)!r}\n")

    def plan(self, a_len, frames, hop_length, overlap_frames, sr=16000):
        """``spectral_plan`` for this map (host only): a ``MappedPlan`` with ``spectral_plan``'s fields and two position tables,
          a_out = round(out_of_src(a_len));  n_clips, F_out: ``track_plan(a_out, ...)``'s, as for a uniform stretch
          pos[g] = src_of_out(g * hop) / hop         the source-frame position of output frame g (float64, F_out entries)
          F_src = floor(max(pos)) + 2;  n_src = hop * (F_src - 1)
          grains[g] = src_of_out(g * TRANSIENT_HOP)  the source centre, in samples, of every grain of ``transients="ola"``
        so ``TimeMap([(0, 0), (1, R)])`` with a dyadic R gives ``spectral_plan(stretch=R)`` and pos == arange * (1 / R) exactly."""
        a_len, frames, hop_length, overlap_frames = int(a_len), int(frames), int(hop_length), int(overlap_frames)
        if a_len < 1:
            raise ValueError(f"TimeMap.plan: a_len {a_len} must be positive")
        a_out = int(round(self.out_of_src(a_len, sr)))
        _T, _step, n_clips = track_plan(a_out, frames, hop_length, overlap_frames)
        sf, Vf = frames - 1 - overlap_frames, overlap_frames + 1
        if 2 * Vf > frames:
            raise ValueError(f"TimeMap.plan: overlap_frames {overlap_frames} + 1 shared frames exceed half a clip of {frames} frames")
        F_out = (n_clips - 1) * sf + frames
        pos = self.src_of_out(np.arange(F_out, dtype=np.float64) * hop_length, sr) / hop_length
        F_src = int(math.floor(pos.max())) + 2
        grains = self.src_of_out(np.arange(ops.ola_grains(hop_length * (F_out - 1), TRANSIENT_WINDOW, TRANSIENT_HOP), dtype=np.float64)
                                 * TRANSIENT_HOP, sr)
        return MappedPlan(sf, Vf, a_out, n_clips, F_out, F_src, hop_length * (F_src - 1), pos, grains)


def _grid(an):
    """how a kernel is told the time grid of this analysis: the keyword of ops.spec_clips / phase_vocoder / phase_lock(_linked)"""
    return {"src_per_out": 1.0 / an.stretch} if an.pos is None else {"pos": an.pos}


def _analyse_spectral(audio, n_fft, hop_length, frames, overlap_frames, stats, osr, sr, res_type, stretch, link=False):
    """resample -> ONE whole-track STFT per channel -> standardise -> polar: an.pol (n_ch, 2, bins, F_src) on the global frame grid.
    ``link``: one more row is analysed, the channel mean (the reference of ops.phase_lock_linked), standardised with the SAME
    (mean, std) as the channels -- the track's own moments are those of the channels alone -- so an.pol is (n_ch + 1, 2, bins, F_src)
    and an.pol[:n_ch] has the bits it has without the option."""
    an = _load(audio, osr, sr, res_type)
    an.link = bool(link)
    n_ch, a_len = an.n_ch, an.a_len
    a2 = torch.cat([an.a2, an.a2.mean(0, keepdim=True)]) if an.link else an.a2      # (rows, a_len); one channel: the mean is the channel
    rows = a2.shape[0]
    dev = a2.device
    if isinstance(stretch, TimeMap):
        # a tempo map: the plan's two position tables go to the device once, and every kernel below reads them (``_grid``)
        an.stretch = stretch
        an.plan = pl = stretch.plan(a_len, frames, hop_length, overlap_frames, sr)
        an.pos, an.grains = torch.from_numpy(pl.pos).to(dev), torch.from_numpy(pl.grains).to(dev)
    else:
        an.stretch = float(stretch)
        an.plan = pl = spectral_plan(a_len, frames, hop_length, overlap_frames, stretch)
        an.pos = an.grains = None
    an.n_clips, an.bins = pl.n_clips, n_fft // 2
    with torch.cuda.device(dev), torch.no_grad():
        if stats is not None:
            # channel c is the region [c a_len, (c + 1) a_len) of the flat buffer; the crop is zero past its end (pg_stft_crops)
            begin = torch.arange(rows, dtype=torch.int64) * a_len
            an.pol = ops.stft_crops(a2.reshape(-1), begin.to(dev), (begin + a_len).to(dev), pl.n_src, n_fft, hop_length, polar=True,
                                    stats=(stats[0], stats[1]))
            return an
        # the track's own moments (zero tail included) need the unnormalised tensor: three launches on the zero-padded track
        padded = torch.zeros(rows, pl.n_src, device=dev, dtype=torch.float32)
        n = min(a_len, pl.n_src)
        padded[:, :n] = a2[:, :n]
        x = ops.stft(padded, n_fft, hop_length)                                               # (rows, 2, bins, F_src)
        if an.link:
            ops.standardize_stats_(x, ops.moments(x[:n_ch]))                                  # the channels' moments, for the mean row too
        else:
            ops.standardize_(x)
        an.pol = ops.polar(x)
    return an


# log1p|z| of the standardised spectrogram below which phase="vocoder" resets a bin: of {0, 0.01, 0.05, 0.2} the floor with the
# smallest consistency on the synthetic melody at stretch 1.5 (tools/vocoder_bench.py; the four figures are in DESIGN.md section 4.11)
VOCODER_RESET_BELOW = 0.2
STRETCH_PHASES = ("unet", "vocoder", "zero", "vocoder_locked", "spsi")
VOCODER_PHASES = ("vocoder", "vocoder_locked")                    # the analysis' own phase, propagated: no model, spectral join only
GRID_PHASES = VOCODER_PHASES + ("spsi",)                          # computed on the track's frame grid: no model, spectral join only
TRANSIENTS = (None, "ola")
HPSS_WIN = (17, 17)                                               # ops.hpss windows (frames, bins) of transients="ola"
TRANSIENT_WINDOW = 256                                            # ops.ola_stretch window and hop of the percussive part:
TRANSIENT_HOP = 64                                                # 16 ms and 4 ms at 16 kHz
FORMANTS = (None, "keep")
# ops.formant_shift's estimator under formant_semitones / formants="keep": cosine order, peak hold (bins on either side), iterations and
# the floor under both linear envelopes (tools/formant_bench.py; the figures are in DESIGN.md section 4.18)
FORMANT_ORDER, FORMANT_HOLD, FORMANT_ITERS, FORMANT_EPS = 64, 16, 2, 0.01


def _invert_spectral(an, model, phase, hop_length, frames, clip_batch, reset_below=None, transients=None, formant_semitones=0.0):
    """One phase source -> (mag, audio): the log-magnitude plane on the output grid (n_ch, bins, F_out) and the un-normalised,
    untrimmed ISTFT of it under that phase (n_ch, hop * (F_out - 1)).  Called under the device and no_grad.
    ``transients="ola"``: the phase source sees the harmonic part of the plane only and the percussive part comes back through the
    time domain (``_add_transients``); ``mag`` stays the FULL plane on the output grid, what the result is meant to show.
    ``formant_semitones`` != 0: the whole analysed plane, the linked mean row included, is first replaced by itself with its spectral
    envelope moved by that many semitones (ONE ops.formant_shift call), so the split, every phase source, the ISTFT magnitudes and
    ``mag`` see the corrected plane."""
    pl, n_ch, bins = an.plan, an.n_ch, an.bins
    grid = _grid(an)
    pol = an.pol[:n_ch]                                                                       # (linked: row n_ch is the channel mean)
    plane = an.pol[:, 0]
    if formant_semitones != 0.0:
        plane = ops.formant_shift(plane, 2.0 ** (-formant_semitones / 12.0), min(FORMANT_ORDER, bins), FORMANT_HOLD, FORMANT_ITERS,
                                  FORMANT_EPS)                                                # (a model narrower than the order: all its bins)
    if transients is not None:
        # all rows are split, the linked mean row too: the reference's magnitudes are its own harmonic part.  The cells handed to
        # the percussive side are zeros in `harm` and fall under the reset floor by themselves.
        harm, perc = ops.hpss(plane, *HPSS_WIN)
        mag, audio = _invert_plane(an, model, phase, hop_length, frames, clip_batch, reset_below, pol, harm[:n_ch], harm[n_ch:])
        audio = _add_transients(an, hop_length, pol, perc[:n_ch], audio)                      # ("ola": the one way there is)
        return ops.spec_clips(plane[:n_ch], 1, pl.F_out, pl.F_out, **grid)[0], audio
    return _invert_plane(an, model, phase, hop_length, frames, clip_batch, reset_below, pol, plane[:n_ch], plane[n_ch:])


def _add_transients(an, hop_length, pol, perc, audio):
    """The percussive plane (n_ch, bins, F_src) under the analysis' own phase, inverted on the source grid and moved onto the output
    grid by overlap-add of a short window, added to the harmonic ``audio`` (n_ch, hop * (F_out - 1)) in the same launch."""
    p_audio = ops.istft(perc, pol[:, 1], hop_length, mode=0, normalize=False)                 # (n_ch, hop * (F_src - 1))
    if an.grains is not None:                                                                 # (a tempo map: one source centre per grain)
        return ops.ola_stretch(p_audio, audio.shape[1], 1.0, TRANSIENT_WINDOW, TRANSIENT_HOP, base=audio, pos=an.grains)
    return ops.ola_stretch(p_audio, audio.shape[1], 1.0 / an.stretch, TRANSIENT_WINDOW, TRANSIENT_HOP, base=audio)


def _invert_plane(an, model, phase, hop_length, frames, clip_batch, reset_below, pol, logmag, ref_logmag):
    """``_invert_spectral`` for one log-magnitude plane ``logmag`` (n_ch, bins, F_src) -- the analysis' own, read in place, or its
    harmonic part -- and, linked, the plane of the channel mean ``ref_logmag`` (1, bins, F_src)."""
    pl, n_ch, bins = an.plan, an.n_ch, an.bins
    grid = _grid(an)
    if phase == "zero":
        ph = torch.zeros(n_ch, bins, pl.F_out, device=logmag.device)                          # (the join of zeros is zero)
    elif phase == "original":
        ph = ops.phase_join(ops.spec_clips(pol[:, 1], pl.n_clips, frames, pl.sf, **grid), pl.sf)
    elif phase == "vocoder":
        # the analysis' own phase, propagated along the output grid by its measured advance (no model, no clips)
        ph = ops.phase_vocoder(pol[:, 1], pl.F_out, logmag=logmag,
                               reset_below=VOCODER_RESET_BELOW if reset_below is None else reset_below, **grid)
    elif phase == "vocoder_locked":
        # ... with identity phase locking: only the peaks of a frame advance, every other bin takes its peak's rotation
        # (linked: ONE rotation for all channels, the channel mean's, so the analysis' inter-channel phase differences survive)
        floor = VOCODER_RESET_BELOW if reset_below is None else reset_below
        if an.link:
            ph = ops.phase_lock_linked(pol[:, 1], an.pol[n_ch, 1], ref_logmag[0], pl.F_out, reset_below=floor, **grid)
        else:
            ph = ops.phase_lock(pol[:, 1], pl.F_out, logmag=logmag, reset_below=floor, **grid)
    elif phase == "spsi":
        # from the magnitudes on the output grid alone: they come first, and nothing of the analysis' phase is read
        mag = ops.spec_clips(logmag, 1, pl.F_out, pl.F_out, **grid)[0]
        ph = ops.phase_spsi(mag, 2 * bins, hop_length)
        return mag, ops.istft(mag, ph, hop_length, mode=0, normalize=False)
    else:
        x = ops.spec_clips(logmag, pl.n_clips, frames, pl.sf, **grid).view(pl.n_clips * n_ch, bins, frames)   # (clip, channel) order
        n_sig = x.shape[0]
        if n_sig <= clip_batch:       # one forward: the phase half of its (n_sig, 2 bins, frames) output is joined in place
            phi = model.forward(x, per_clip=True).view(pl.n_clips, n_ch, 2 * bins, frames)[:, :, :bins]
        else:
            phi = torch.empty(pl.n_clips, n_ch, bins, frames, device=logmag.device)
            flat = phi.view(n_sig, bins, frames)
            for i in range(0, n_sig, clip_batch):
                flat[i:i + clip_batch] = model.forward(x[i:i + clip_batch], per_clip=True)[:, :bins]
        ph = ops.phase_join(phi, pl.sf)
    # the magnitudes on the output grid: the plane itself, cut (or time-resampled) to F_out frames by the same kernel
    mag = ops.spec_clips(logmag, 1, pl.F_out, pl.F_out, **grid)[0]
    return mag, ops.istft(mag, ph, hop_length, mode=0, normalize=False)                       # (n_ch, hop * (F_out - 1))


def _trim_spectral(an, audio, normalize):
    """The first a_out samples of the whole-track ISTFT, finite-checked (and peak-normalised): (channels, a_out)."""
    pl = an.plan
    out, _, bad = ops.stitch(audio[:, None, :pl.a_out], pl.a_out, pl.a_out, normalize=normalize, return_status=True)
    if int(bad.item()) != 0:
        raise ValueError("Audio buffer is not finite everywhere")
    return out


def _synthesise_spectral(an, model, phase, hop_length, frames, clip_batch, normalize, reset_below=None, transients=None, formant_semitones=0.0):
    """One phase source -> the track (channels, a_out) through the spectral join: clip windows of the log-magnitude plane, forward,
    ONE phase per global frame (ops.phase_join; phase="vocoder": ops.phase_vocoder on the analysis' phase instead), ONE ISTFT with
    the plane's own magnitudes; raises when a sample is not finite."""
    with torch.cuda.device(an.a2.device), torch.no_grad():
        _mag, audio = _invert_spectral(an, model, phase, hop_length, frames, clip_batch, reset_below, transients, formant_semitones)
        return _trim_spectral(an, audio, normalize)


def _check_join(who, join, stretch, phase_list):
    if join not in JOINS:
        raise ValueError(f"{who}: join must be 'waveform' or 'spectral', got {join!r}")
    if isinstance(stretch, TimeMap):                             # a tempo map is a stretch other than 1, whatever its slopes
        if join != "spectral":
            raise ValueError(f"{who}: a TimeMap needs join='spectral'")
        for p in phase_list:
            if p not in STRETCH_PHASES:
                raise ValueError(f"{who}: a TimeMap needs phase 'unet', 'vocoder', 'vocoder_locked', 'spsi' or 'zero', got {p!r} (the analysis' own phase does not fit a resampled spectrogram)")
        return stretch
    stretch = float(stretch)
    if stretch != 1.0 and join != "spectral":
        raise ValueError(f"{who}: stretch {stretch} needs join='spectral'")
    for p in phase_list:
        if join == "spectral" and p == "griffinlim":
            raise ValueError(f"{who}: phase 'griffinlim' is not available under join='spectral'")
        if join != "spectral" and p in GRID_PHASES:
            raise ValueError(f"{who}: phase {p!r} needs join='spectral' (it propagates the phase on the track's frame grid)")
        if stretch != 1.0 and p not in STRETCH_PHASES:
            raise ValueError(f"{who}: stretch {stretch} needs phase 'unet', 'vocoder', 'vocoder_locked', 'spsi' or 'zero', got {p!r} (the analysis' own phase does not fit a resampled spectrogram)")
    return stretch


def _check_link(who, link_channels, join, phase_list):
    """link_channels: only the locked vocoder under the spectral join has channels to link"""
    if link_channels and (join != "spectral" or "vocoder_locked" not in phase_list):
        raise ValueError(f"{who}: link_channels needs join='spectral' and phase 'vocoder_locked', got join {join!r} and {tuple(phase_list)!r}")
    return bool(link_channels)


def _check_transients(who, transients, join):
    """transients: None or "ola"; the split works on the whole-track plane, which only the spectral join has"""
    if transients not in TRANSIENTS:
        raise ValueError(f"{who}: transients must be None or 'ola', got {transients!r}")
    if transients is not None and join != "spectral":
        raise ValueError(f"{who}: transients={transients!r} needs join='spectral', got join {join!r}")
    return transients


def _check_formants(who, formant_semitones, join):
    """formant_semitones: a finite shift within two octaves; the correction works on the whole-track plane, which only the spectral
    join has"""
    fs = float(formant_semitones)
    if not (fs == fs and -24.0 <= fs <= 24.0):
        raise ValueError(f"{who}: formant_semitones must be within [-24, 24], got {formant_semitones}")
    if fs != 0.0 and join != "spectral":
        raise ValueError(f"{who}: formant_semitones={fs} needs join='spectral', got join {join!r}")
    return fs


def peak_normalize(audio):
    """utils.py:42 for a whole track on the device: audio (samples,) or (channels, samples) divided by its joint peak -- the second
    launch of pg_stitch over one clip per channel, so ``peak_normalize(reconstruct_track(..., normalize=False))`` has the bits of
    ``reconstruct_track(..., normalize=True)``."""
    a2 = audio[None] if audio.dim() == 1 else audio
    n = a2.shape[1]
    with torch.cuda.device(a2.device):
        out = ops.stitch(a2[:, None, :], n, n, normalize=True)
    return out[0] if audio.dim() == 1 else out


def _keyword_options(impl, later=None, newer=None, newest=None, **options):
    """Decorator for the two public track functions: the decorated ``def`` states the POSITIONAL parameter list and the docstring --
    the list callers of the waveform-only functions have always seen, which stays as it is (``inspect.signature`` reports it) -- and
    the call itself goes to ``impl`` with, in addition, the keyword-only ``options`` (name=default), which may be passed by keyword
    only.  ``fn.options`` lists them.  ``later``: keyword-only options (name=default) added since callers began to compare
    ``fn.options``, which therefore stays as it was; ``fn.later_options`` lists those.  ``newer``: the same once more, for options
    added since callers began to compare ``fn.later_options``; ``fn.newer_options`` lists those.  ``newest``: and once more, for
    options added since callers began to compare ``fn.newer_options``; ``fn.newest_options`` lists those."""
    later, newer, newest = dict(later or {}), dict(newer or {}), dict(newest or {})

    def deco(fn):
        sig = inspect.signature(fn)

        @functools.wraps(fn)
        def call(*args, **kw):
            opts = {k: kw.pop(k, d) for k, d in {**options, **later, **newer, **newest}.items()}
            bound = sig.bind(*args, **kw)
            bound.apply_defaults()
            return impl(**bound.arguments, **opts)
        call.options = dict(options)
        call.later_options = dict(later)
        call.newer_options = dict(newer)
        call.newest_options = dict(newest)
        return call
    return deco


def _reconstruct_track(model, audio, n_fft, hop_length, frames, overlap_frames, stats, osr, sr, res_type, clip_batch, phase, normalize,
                       join, stretch, link_channels, transients, formant_semitones):
    """``reconstruct_track`` with its keyword-only options spelled out."""
    if phase not in ("unet", "original", "zero") + GRID_PHASES:
        raise ValueError(f"reconstruct_track: phase must be 'unet', 'original', 'zero', 'vocoder', 'vocoder_locked' or 'spsi', got {phase!r}")
    if phase == "unet" and model is None:
        raise ValueError("reconstruct_track: phase='unet' needs a model")
    if clip_batch < 1:
        raise ValueError("reconstruct_track: clip_batch must be positive")
    stretch = _check_join("reconstruct_track", join, stretch, (phase,))
    link = _check_link("reconstruct_track", link_channels, join, (phase,))
    transients = _check_transients("reconstruct_track", transients, join)
    formant_semitones = _check_formants("reconstruct_track", formant_semitones, join)
    if join == "spectral":
        an = _analyse_spectral(audio, n_fft, hop_length, frames, overlap_frames, stats, osr, sr, res_type, stretch, link)
        out = _synthesise_spectral(an, model, phase, hop_length, frames, clip_batch, normalize, transients=transients,
                                   formant_semitones=formant_semitones)
        return out[0] if an.mono else out
    an = _analyse(audio, n_fft, hop_length, frames, overlap_frames, stats, osr, sr, res_type)
    out = _synthesise(an, model, phase, hop_length, clip_batch, normalize)
    return out[0] if an.mono else out


@_keyword_options(_reconstruct_track, later={"link_channels": False}, newer={"transients": None}, newest={"formant_semitones": 0.0},
                  join="waveform", stretch=1.0)
def reconstruct_track(model, audio, n_fft=2048, hop_length=512, frames=128, overlap_frames=32, stats=None,
                      osr=None, sr=16000, res_type="kaiser_best", clip_batch=64, phase="unet", normalize=True):
    """audio (samples,) or (channels, samples), host array or device tensor, at ``sr`` -- or at ``osr`` when given (resampled to
    ``sr`` first) -> float32 device tensor of the same shape with the a_len samples per channel of the track at ``sr``, its phase
    predicted by ``model`` (phase="unet"), kept from the analysis (phase="original": the chunk / stitch round trip) or all zero
    (phase="zero", the reference's "no phase" comparator); ``model`` may be None for the last two.  ``stats`` = (mean, std) of the
    training set; None: the track's own moments.  ``normalize``: peak-normalise over all channels jointly (utils.py:42 for the whole
    track).  Raises ValueError("Audio buffer is not finite everywhere") as ``audio.generate_audio`` does.
    Keyword-only options (``reconstruct_track.options``; the positional parameter list above is the waveform-only call's and stays):
    ``join="waveform"`` inverts every clip and crossfades the waveforms (ops.stitch); ``join="spectral"`` joins the clips' PHASES on
    the track's frame grid (ops.phase_join: one phase per frame, the circular mean where two clips overlap) and inverts the whole
    track once with its exact magnitudes.  ``stretch=1.0`` (spectral join, phase "unet", "vocoder" or "zero"): the magnitudes are
    resampled along time and the result has round(a_len * stretch) samples per channel at the same pitch; a ``TimeMap`` in place of
    the number stretches every part of the track at its own rate (round(out_of_src(a_len)) samples).  phase="vocoder" (spectral
    join only, ``model`` may be None) is the phase vocoder: the analysis' own phase, propagated along the output frames by its
    measured advance (ops.phase_vocoder, floor ``VOCODER_RESET_BELOW``) -- the standard comparator of a time stretch.
    phase="vocoder_locked" (the same conditions) is that vocoder with identity phase locking (ops.phase_lock): only the spectral peaks
    of a frame advance and every other bin keeps its analysis phase relation to its peak -- the stretch to use without weights.
    phase="spsi" (the same conditions) is single-pass spectrogram inversion (ops.phase_spsi): a phase from the output grid's
    magnitudes alone, the model-free baseline that reads nothing of the analysis' phase.
    ``link_channels=False`` (``reconstruct_track.later_options``; spectral join and phase="vocoder_locked" only, else ValueError): all
    channels take ONE rotation, that of their mean (ops.phase_lock_linked), instead of one each, so the phase difference between two
    channels stays the analysis' own in every cell and the stereo image and the mono sum survive the stretch; mono input gives the
    bits of the unlinked call.
    ``transients=None`` (``reconstruct_track.newer_options``; spectral join only, else ValueError; with every phase and with
    ``link_channels``): ``"ola"`` splits the log-magnitude plane into a harmonic and a percussive part by median filtering (ops.hpss,
    ``HPSS_WIN``), hands the harmonic part to the chosen phase source in the plane's place, inverts the percussive part on the source
    grid with the analysis' own phase and moves it onto the output grid in the time domain (ops.ola_stretch, ``TRANSIENT_WINDOW`` /
    ``TRANSIENT_HOP``): onsets are relocated instead of stretched.  None: not one launch and not one bit differs from a call
    without the keyword.
    ``formant_semitones=0.0`` (``reconstruct_track.newest_options``; spectral join only, else ValueError; with every phase, with
    ``link_channels`` and with ``transients``): the spectral envelope of every analysed frame -- peak hold, liftered cosine smoothing,
    a few iterations (ops.formant_shift, ``FORMANT_ORDER`` / ``FORMANT_HOLD`` / ``FORMANT_ITERS`` / ``FORMANT_EPS``) -- is moved by that
    many semitones while the partials stay where they are; the corrected plane replaces the analysed one before anything else reads
    it.  ``pitch_shift(formants="keep")`` passes the negative of its shift, so that the resampling puts the formants back.  0.0: not
    one launch and not one bit differs from a call without the keyword."""


def _evaluate_track(model, audio, n_fft, hop_length, frames, overlap_frames, stats, osr, sr, res_type, clip_batch, phases, gl_iters,
                    gl_seed, floor, return_audio, join, gl_init):
    """``evaluate_track`` with its keyword-only options spelled out."""
    phases = tuple(phases)
    for p in phases:
        if p not in REPORT_PHASES:
            raise ValueError(f"evaluate_track: unknown phase {p!r} (expected some of {REPORT_PHASES})")
    if gl_init not in GL_INITS:
        raise ValueError(f"evaluate_track: gl_init must be 'noise' or 'spsi', got {gl_init!r}")
    if len(set(phases)) != len(phases) or not phases:
        raise ValueError("evaluate_track: phases must be a non-empty list without repetitions")
    if "unet" in phases and model is None:
        raise ValueError("evaluate_track: phase 'unet' needs a model")
    if clip_batch < 1:
        raise ValueError("evaluate_track: clip_batch must be positive")
    _check_join("evaluate_track", join, 1.0, phases)
    if join == "spectral":
        an = _analyse_spectral(audio, n_fft, hop_length, frames, overlap_frames, stats, osr, sr, res_type, 1.0)
    else:
        an = _analyse(audio, n_fft, hop_length, frames, overlap_frames, stats, osr, sr, res_type)
    ref = an.a2[0] if an.mono else an.a2
    res = {"n_samples": int(an.a_len), "sr": int(sr), "n_clips": int(an.n_clips), "join": join, "gl_init": gl_init, "metrics": {}}
    if return_audio:
        res["audio"] = {}
    for p in phases:
        if join == "spectral":
            out = _synthesise_spectral(an, model, p, hop_length, frames, clip_batch, False)
        else:
            out = _synthesise(an, model, p, hop_length, clip_batch, False, gl_iters, gl_seed, gl_init)
        out = out[0] if an.mono else out
        res["metrics"][p] = metrics.compare_audio(ref, out, n_fft, hop_length, floor)
        if return_audio:
            res["audio"][p] = out
    return res


@_keyword_options(_evaluate_track, later={"gl_init": "noise"}, join="waveform")
def evaluate_track(model, audio, n_fft=2048, hop_length=512, frames=128, overlap_frames=32, stats=None, osr=None, sr=16000,
                   res_type="kaiser_best", clip_batch=64, phases=("unet", "zero", "original"), gl_iters=250, gl_seed=0, floor=1e-10,
                   return_audio=False):
    """The quality report of a track: ONE analysis (as ``reconstruct_track``), then for every entry of ``phases`` -- "unet" (the
    model's phase), "zero" (none), "original" (the analysis' own: what the chunk / stitch round trip alone costs), "griffinlim"
    (``audio.griffin_lim_batch`` on exp(logmag) - 1 per clip, ``gl_iters`` iterations from noise seeded ``gl_seed`` + clip index) --
    the un-normalised stitched track and ``metrics.compare_audio(input at sr, track, n_fft, hop_length, floor)``.
    -> {"n_samples", "sr", "n_clips", "join", "metrics": {phase: dict}} and, with ``return_audio``, "audio": {phase: device tensor
    shaped like the input}.  The "unet" audio has the bits of ``reconstruct_track(..., normalize=False)``.  ``model`` may be None
    when "unet" is not asked for.  Keyword-only options (``evaluate_track.options`` and ``.later_options``): ``join="waveform"`` or ``"spectral"``, as in
    ``reconstruct_track`` ("griffinlim" is not available under "spectral"; "spsi", ops.phase_spsi on the track's magnitudes, only
    there: ``REPORT_PHASES``); ``gl_init="noise"`` or ``"spsi"``: every clip's Griffin-Lim starts from noise or from the ISTFT of
    its single-pass inversion (``griffin_lim_batch``'s ``init``).  The report records ``gl_init``.
    Every synthesis is finite-checked before it is measured: raises ValueError("Audio buffer is not finite everywhere"), as
    ``reconstruct_track`` does, and returns no report, when a sample of any of them is not finite."""


def _evaluate_stretch(model, audio, stretch, n_fft, hop_length, frames, overlap_frames, stats, osr, sr, res_type, clip_batch, phases,
                      reset_below, floor, return_audio, link_channels, transients, formant_semitones):
    """``evaluate_stretch`` with its keyword-only options spelled out."""
    phases = tuple(phases)
    for p in phases:
        if p not in STRETCH_PHASES:
            raise ValueError(f"evaluate_stretch: unknown phase {p!r} (expected some of {STRETCH_PHASES})")
    if len(set(phases)) != len(phases) or not phases:
        raise ValueError("evaluate_stretch: phases must be a non-empty list without repetitions")
    if "unet" in phases and model is None:
        raise ValueError("evaluate_stretch: phase 'unet' needs a model")
    if clip_batch < 1:
        raise ValueError("evaluate_stretch: clip_batch must be positive")
    reset_below = VOCODER_RESET_BELOW if reset_below is None else float(reset_below)
    if not 0.0 <= reset_below < math.inf:
        raise ValueError(f"evaluate_stretch: reset_below must be finite and not negative, got {reset_below}")
    stretch = _check_join("evaluate_stretch", "spectral", stretch, phases)
    link = _check_link("evaluate_stretch", link_channels, "spectral", phases)
    transients = _check_transients("evaluate_stretch", transients, "spectral")
    formant_semitones = _check_formants("evaluate_stretch", formant_semitones, "spectral")
    an = _analyse_spectral(audio, n_fft, hop_length, frames, overlap_frames, stats, osr, sr, res_type, stretch, link)
    # (under a TimeMap "stretch" is the mean one, n_out / n_samples: the report keeps its keys and stays a plain JSON object)
    res = {"n_samples": int(an.a_len), "n_out": int(an.plan.a_out), "sr": int(sr),
           "stretch": an.plan.a_out / an.a_len if an.pos is not None else stretch, "n_clips": int(an.n_clips),
           "reset_below": reset_below, "metrics": {}}
    if link:
        res["link_channels"], res["mid_metrics"] = True, {}
    if transients is not None:
        res["transients"] = transients
    if formant_semitones != 0.0:
        res["formant_semitones"] = formant_semitones
    if return_audio:
        res["audio"] = {}
    with torch.cuda.device(an.a2.device), torch.no_grad():
        if link:        # the mid signal's imposed magnitudes: the mean row's plane, resampled as the channels' are
            mid_mag = ops.spec_clips(an.pol[an.n_ch:, 0], 1, an.plan.F_out, an.plan.F_out, **_grid(an))[0]
        for p in phases:
            mag, full = _invert_spectral(an, model, p, hop_length, frames, clip_batch, reset_below, transients, formant_semitones)
            out = _trim_spectral(an, full, False)
            res["metrics"][p] = metrics.consistency(mag, full, n_fft, hop_length, floor)
            if link:
                res["mid_metrics"][p] = metrics.consistency(mid_mag, full.mean(0, keepdim=True), n_fft, hop_length, floor)
            if return_audio:
                res["audio"][p] = out[0] if an.mono else out
    return res


@_keyword_options(_evaluate_stretch, later={"link_channels": False}, newer={"transients": None}, newest={"formant_semitones": 0.0})
def evaluate_stretch(model, audio, stretch, n_fft=2048, hop_length=512, frames=128, overlap_frames=32, stats=None, osr=None, sr=16000,
                     res_type="kaiser_best", clip_batch=64, phases=("unet", "vocoder", "zero"), reset_below=None, floor=1e-10,
                     return_audio=False):
    """The quality report of a STRETCHED track, which has no reference waveform to be compared with: ONE spectral analysis (as
    ``reconstruct_track(join="spectral", stretch=stretch)``), then for every entry of ``phases`` -- "unet" (the model's phase),
    "vocoder" (ops.phase_vocoder with the floor ``reset_below``; None: ``VOCODER_RESET_BELOW``), "zero" (none), "vocoder_locked"
    (ops.phase_lock with the same floor), "spsi" (ops.phase_spsi on the resampled magnitudes alone) -- one synthesis and
    ``metrics.consistency`` of its untrimmed ISTFT output against the resampled log-magnitude plane it was made from: how far the
    spectrogram of the result lands from the magnitudes that were imposed.
    -> {"n_samples", "n_out", "sr", "stretch", "n_clips", "reset_below", "metrics": {phase: dict}} and, with ``return_audio``,
    "audio": {phase: un-normalised device tensor of round(a_len * stretch) samples per channel}.  The "unet" and "zero" audio has the
    bits of ``reconstruct_track(..., normalize=False, join="spectral", stretch=stretch)``.  ``model`` may be None when "unet" is not
    asked for.  Keyword-only option (``evaluate_stretch.later_options``): ``link_channels=False``, as in ``reconstruct_track``
    ("vocoder_locked" must be among ``phases``, which alone it changes); with it the report also holds "link_channels": True and
    "mid_metrics": {phase: ``metrics.consistency`` of the channel mean of the untrimmed output against the resampled log-magnitude
    plane of the channel mean of the input}, for every phase asked for: what the channels' sum to mono lost.  Without it the report
    has the keys above and no others.  ``transients=None`` (``evaluate_stretch.newer_options``): ``"ola"`` synthesises every phase
    as ``reconstruct_track(..., transients="ola")`` does and records "transients": "ola" in the report; the consistency is still
    measured against the FULL plane's magnitudes on the output grid.  ``formant_semitones=0.0`` (``evaluate_stretch.newest_options``):
    as in ``reconstruct_track``; a value other than 0 is recorded as "formant_semitones" and the consistency is measured against the
    CORRECTED plane's magnitudes, the ones that were imposed.
    Every synthesis is finite-checked before it is measured: raises ValueError("Audio buffer is not finite everywhere"), as
    ``reconstruct_track`` does, and returns no report, when one of the round(a_len * stretch) samples of any of them is not finite."""


def pitch_ratio(semitones, max_denominator=1024):
    """(stretch, Fraction p / q): the stretch 2 ** (semitones / 12) and the rational p / q closest to it with q <= 1024, the most
    phases pg_resample takes (its taps stay below 2048 for every ratio up to 4).  Resampling by q / p shifts the pitch by p / q
    instead of the exact ratio: at most 0.85 cent off for any shift within two octaves, at most 0.027 cent for a whole number of
    semitones (1200 log2((p / q) / stretch), evaluated for every shift in steps of 0.001 semitone)."""
    stretch = 2.0 ** (float(semitones) / 12.0)
    if not (stretch == stretch and 0.25 <= stretch <= 4.0):
        raise ValueError(f"pitch_shift: semitones must be within [-24, 24], got {semitones}")
    return stretch, fractions.Fraction(stretch).limit_denominator(max_denominator)


CurvePlan = collections.namedtuple("CurvePlan", "time_map pos scale step")
PITCH_CURVE_STEP, PITCH_CURVE_SEGMENT = 64, 256                   # ops.varispeed's block and PitchCurve.plan's segment, in samples


PitchTrack = collections.namedtuple("PitchTrack", "times f0 voiced ap")
TONICS = {"C": 0, "C#": 1, "Db": 1, "D": 2, "D#": 3, "Eb": 3, "E": 4, "F": 5, "F#": 6, "Gb": 6, "G": 7, "G#": 8, "Ab": 8, "A": 9, "A#": 10,
          "Bb": 10, "B": 11}
SCALE_DEGREES = {"maj": (0, 2, 4, 5, 7, 9, 11), "min": (0, 2, 3, 5, 7, 8, 10)}


def scale_classes(scale):
    """the pitch classes (0 = C) of "chromatic", "<tonic>:maj" or "<tonic>:min" (natural minor), as a frozenset"""
    if scale == "chromatic":
        return frozenset(range(12))
    tonic, _, mode = scale.partition(":") if isinstance(scale, str) else ("", "", "")
    if tonic not in TONICS or mode not in SCALE_DEGREES:
        raise ValueError(f"scale must be 'chromatic', '<tonic>:maj' or '<tonic>:min' with a tonic among {', '.join(TONICS)}, got {scale!r}")
    return frozenset((TONICS[tonic] + d) % 12 for d in SCALE_DEGREES[mode])


class PitchCurve:
    """A pitch curve: a time-varying transposition, piecewise linear in semitones between anchors and constant past the last one
    (host only, float64).  ``anchors``: a sequence of (seconds, semitones) with at least two entries, finite, the first at 0 s,
    seconds strictly increasing, |semitones| <= 24 (the domain of a uniform ``pitch_shift``).  ValueError otherwise.
    ``pitch_shift`` takes one in place of its number of semitones: a glide, a vibrato, a correction, a tape stop."""

    def __init__(self, anchors):
        try:
            if isinstance(anchors, np.ndarray) and anchors.dtype == np.float64:
                a = anchors.copy()                                # (thousands of anchors, as ``correcting`` makes them: no Python lists)
            else:
                a = np.array([[float(v) for v in row] for row in anchors], dtype=np.float64)
        except (TypeError, ValueError) as e:
            raise ValueError(f"PitchCurve: anchors must be (seconds, semitones) pairs ({e})")
        if a.ndim != 2 or a.shape[1] != 2 or a.shape[0] < 2:
            raise ValueError("PitchCurve: at least two anchors (seconds, semitones)")
        if not np.isfinite(a).all():
            raise ValueError("PitchCurve: anchors must be finite")
        if a[0, 0] != 0.0:
            raise ValueError(f"PitchCurve: the first anchor must be at 0 s, got {a[0, 0]}")
        if not (np.diff(a[:, 0]) > 0.0).all():
            raise ValueError("PitchCurve: seconds must increase strictly")
        if not (np.abs(a[:, 1]) <= 24.0).all():
            raise ValueError(f"PitchCurve: semitones must be within [-24, 24], got {a[:, 1].min():g} .. {a[:, 1].max():g}")
        self.seconds, self.semitones = a[:, 0].copy(), a[:, 1].copy()
        self.seconds.setflags(write=False)
        self.semitones.setflags(write=False)

    @property
    def anchors(self):
        return [(float(t), float(s)) for t, s in zip(self.seconds, self.semitones)]

    def __repr__(self):
        return f"PitchCurve({self.anchors!r})"

    def semitones_at(self, t):
        """the transposition at ``t`` seconds (a number or an array): linear between anchors, the last anchor's from there on"""
        y = np.interp(np.asarray(t, np.float64), self.seconds, self.semitones)
        return float(y) if y.ndim == 0 else y

    @classmethod
    def vibrato(cls, duration_s, depth, rate_hz, per_cycle=16):
        """``depth`` semitones of vibrato at ``rate_hz`` over ``duration_s`` seconds: depth * sin(2 pi rate_hz t), sampled
        ``per_cycle`` times per cycle (the last anchor lies at or beyond ``duration_s``)."""
        duration_s, depth, rate_hz, per_cycle = float(duration_s), float(depth), float(rate_hz), int(per_cycle)
        if not (0.0 < duration_s < math.inf and 0.0 < rate_hz < math.inf) or per_cycle < 4:
            raise ValueError(f"PitchCurve.vibrato: duration_s {duration_s} and rate_hz {rate_hz} must be positive and finite and "
                             f"per_cycle {per_cycle} at least 4")
        if not abs(depth) <= 24.0:
            raise ValueError(f"PitchCurve.vibrato: depth must be within [-24, 24], got {depth}")
        k = np.arange(int(math.ceil(duration_s * rate_hz * per_cycle)) + 1, dtype=np.float64)
        return cls(list(zip(k / (rate_hz * per_cycle), depth * np.sin(2.0 * np.pi * (k / per_cycle)))))

    @classmethod
    def load(cls, path):
        """A text file in ``TimeMap.load``'s format: two columns per line, seconds and semitones."""
        anchors = []
        with open(path) as f:
            for n, line in enumerate(f, 1):
                cols = line.split("#", 1)[0].replace(",", " ").split()
                if not cols:
                    continue
                if len(cols) != 2:
                    raise ValueError(f"PitchCurve.load: {path}:{n}: expected two columns, got {len(cols)}")
                try:
                    anchors.append((float(cols[0]), float(cols[1])))
                except ValueError:
                    raise ValueError(f"PitchCurve.load: {path}:{n}: not two numbers: {line.strip()!r}")
        return cls(anchors)

    def save(self, path):
        with open(path, "w") as f:
            f.write("# seconds semitones\n")
            for t, s in zip(self.seconds, self.semitones):
                f.write(f"{float(t)!r} {float(s)!r}\n")

    @classmethod
    def correcting(cls, pitch_track, strength=1.0, scale="chromatic", a4=440.0, retune_ms=0.0):
        """The curve that corrects a detected ``PitchTrack`` (``detect_pitch``) towards the nearest note of ``scale`` (host, float64).
          m_k = 69 + 12 log2(f0_k / a4) at a voiced frame; its target is the nearest note whose pitch class is in the scale, the
          lower one on a tie.  ``scale``: "chromatic", "<tonic>:maj" or "<tonic>:min" (natural minor), tonic C, C#, Db, ... B.
          c_k = strength (target - m_k) at voiced frames; an unvoiced frame holds the previous voiced value, the frames before the
          first voiced one take its value, a track without a voiced frame gives the zero curve.
          y_k = y_{k-1} + alpha (c_k - y_{k-1}), y_{-1} = c_0, alpha = 1 - exp(-dt / (retune_ms / 1000)) with dt the spacing of the
          track's frames (hop / sr); alpha = 1 for retune_ms = 0: how fast a note is pulled in.
        Anchors: (0, y_0) and then (times[k], y_k).  ``strength`` within [0, 1], ``a4`` and ``retune_ms`` finite, a4 > 0,
        retune_ms >= 0, else ValueError."""
        who = "PitchCurve.correcting"
        try:
            times, f0, voiced = (np.asarray(v) for v in (pitch_track.times, pitch_track.f0, pitch_track.voiced))
        except AttributeError:
            raise ValueError(f"{who}: expected a PitchTrack (times, f0, voiced, ap)")
        times, f0, voiced = times.astype(np.float64), f0.astype(np.float64), voiced.astype(bool)
        if times.ndim != 1 or times.shape[0] < 1 or f0.shape != times.shape or voiced.shape != times.shape:
            raise ValueError(f"{who}: times, f0 and voiced must be 1-D arrays of one length, at least 1")
        if not (np.isfinite(times).all() and times[0] > 0.0 and (np.diff(times) > 0.0).all()):
            raise ValueError(f"{who}: times must be finite, positive and strictly increasing")
        strength, a4, retune_ms = float(strength), float(a4), float(retune_ms)
        if not 0.0 <= strength <= 1.0:
            raise ValueError(f"{who}: strength must be within [0, 1], got {strength}")
        if not (0.0 < a4 < math.inf):
            raise ValueError(f"{who}: a4 must be positive and finite, got {a4}")
        if not (0.0 <= retune_ms < math.inf):
            raise ValueError(f"{who}: retune_ms must be non-negative and finite, got {retune_ms}")
        classes = scale_classes(scale)
        if voiced.any() and not (np.isfinite(f0[voiced]).all() and (f0[voiced] > 0.0).all()):
            raise ValueError(f"{who}: f0 must be positive and finite at voiced frames")
        c = np.zeros(times.shape[0], np.float64)
        if voiced.any():
            m = 69.0 + 12.0 * np.log2(f0[voiced] / a4)
            notes = np.array([n for n in range(-60, 200) if n % 12 in classes], dtype=np.float64)
            if m.min() < notes[0] or m.max() > notes[-1]:
                raise ValueError(f"{who}: f0 outside the notes {notes[0]:.0f} .. {notes[-1]:.0f} of a4 = {a4}")
            hi = np.searchsorted(notes, m, side="left")                              # notes[hi - 1] < m <= notes[hi]
            hi = np.clip(hi, 1, len(notes) - 1)
            below, above = notes[hi - 1], notes[hi]
            target = np.where(above - m < m - below, above, below)                   # a tie goes to the lower note
            idx = np.flatnonzero(voiced)
            held = np.maximum.accumulate(np.where(voiced, np.arange(times.shape[0]), -1))   # the last voiced frame at or before k
            held = np.where(held < 0, idx[0], held)
            full = np.zeros(times.shape[0], np.float64)
            full[idx] = strength * (target - m)
            c = full[held]
        if retune_ms > 0.0 and times.shape[0] > 1:
            alpha = 1.0 - math.exp(-float(times[1] - times[0]) / (retune_ms / 1000.0))
            y = np.empty_like(c)
            prev = c[0]
            for k in range(c.shape[0]):
                prev = prev + alpha * (c[k] - prev)
                y[k] = prev
        else:
            y = c
        return cls(np.column_stack([np.concatenate([[0.0], times]), np.concatenate([y[:1], y])]))

    def plan(self, a_len, sr=16000, step=PITCH_CURVE_STEP, segment=PITCH_CURVE_SEGMENT):
        """The two halves of a pitch shift along this curve for a track of ``a_len`` samples at ``sr`` (host only): a
        ``CurvePlan(time_map, pos, scale, step)``.
          segment i covers the samples [i segment, (i + 1) segment) and is stretched by r_i = 2 ** (semitones_at(its midpoint) / 12)
          time_map    the ``TimeMap`` through (i segment, sum of segment r_k for k < i) / sr: what ``reconstruct_track`` stretches by
          pos[j] = time_map.out_of_src(j step, sr), j = 0 .. nb, nb = ceil(a_len / step): where output block j of ``ops.varispeed``
                      begins in the stretched track
          scale[j] = float32(min(1, step / (pos[j + 1] - pos[j]))): the band of a block that is read faster than it is written
        ``segment`` is a multiple of ``step``, so every block lies inside one segment: the resampler undoes the stretch exactly at
        every block boundary, and the tempo is the input's by construction."""
        a_len, sr, step, segment = int(a_len), int(sr), int(step), int(segment)
        if a_len < 1 or sr < 1:
            raise ValueError(f"PitchCurve.plan: a_len {a_len} and sr {sr} must be positive")
        if not (1 <= step <= 4096 and step & (step - 1) == 0):
            raise ValueError(f"PitchCurve.plan: step must be a power of two within [1, 4096], got {step}")
        if segment < step or segment % step:
            raise ValueError(f"PitchCurve.plan: segment {segment} must be a multiple of step {step}")
        n_seg = -(-a_len // segment)
        src = np.arange(n_seg + 1, dtype=np.float64) * segment
        r = 2.0 ** (self.semitones_at((src[:-1] + 0.5 * segment) / sr) / 12.0)
        out = np.concatenate([[0.0], np.cumsum(np.diff(src) * r)])
        time_map = TimeMap(list(zip(src / sr, out / sr)))
        nb = -(-a_len // step)
        pos = np.asarray(time_map.out_of_src(np.arange(nb + 1, dtype=np.float64) * step, sr), np.float64)
        scale = np.minimum(1.0, step / np.diff(pos)).astype(np.float32)
        return CurvePlan(time_map, pos, scale, step)


def _pitch_curve(model, audio, curve, n_fft, hop_length, frames, overlap_frames, stats, osr, sr, res_type, clip_batch, phase, normalize,
                 link_channels, transients):
    """``pitch_shift`` along a ``PitchCurve``: stretch by the plan's tempo map, play back along its positions."""
    a = preproc.resample(audio, osr, sr, res_type=res_type) if osr is not None else audio
    a_len = int(a.shape[-1])
    pl = curve.plan(a_len, sr)
    out = reconstruct_track(model, a, n_fft, hop_length, frames, overlap_frames, stats, None, sr, res_type, clip_batch, phase,
                            normalize=False, join="spectral", stretch=pl.time_map, link_channels=link_channels, transients=transients)
    with torch.cuda.device(out.device):
        out = ops.varispeed(out, torch.from_numpy(pl.pos).to(out.device), torch.from_numpy(pl.scale).to(out.device), a_len, step=pl.step,
                            res_type=res_type)
    return peak_normalize(out) if normalize else out


def pitch_shift(model, audio, semitones, n_fft=2048, hop_length=512, frames=128, overlap_frames=32, stats=None, osr=None, sr=16000,
                res_type="kaiser_best", clip_batch=64, phase="unet", normalize=True, *, link_channels=False, transients=None, formants=None):
    """Pitch shift by ``semitones`` (within two octaves) without a change of tempo: the track is stretched by 2 ** (semitones / 12)
    through the spectral join (``reconstruct_track(join="spectral", stretch=...)``: same pitch, longer or shorter) and played back
    faster or slower by the same ratio (``preproc.resample`` by q / p, see ``pitch_ratio`` for the error in cents), then trimmed or
    zero-padded to the input's length at ``sr``.  ``phase``: "unet", "vocoder", "vocoder_locked", "spsi" or "zero", as in
    ``reconstruct_track``; ``link_channels`` and ``transients`` (keyword only) are forwarded to it.  ``formants`` (keyword only): None
    lets the spectral envelope move with the partials (a voice shifted up sounds smaller); ``"keep"`` forwards
    ``formant_semitones=-semitones``, so the envelope is moved the other way on the analysed plane and the resampling puts it back
    where it was.
    ``semitones`` may be a ``PitchCurve``: the transposition then varies along the track.  The track is stretched by the curve's tempo
    map (``PitchCurve.plan``; ``reconstruct_track(stretch=TimeMap)``) and played back along the plan's position table by the
    variable-rate resampler (``ops.varispeed``), which undoes the stretch at every block boundary: the result has exactly the
    input's length, without a trim or a pad.  ``formants="keep"`` is not available with a curve (ValueError).
    -> float32 device tensor shaped like the input at ``sr``."""
    if formants not in FORMANTS:
        raise ValueError(f"pitch_shift: formants must be None or 'keep', got {formants!r}")
    if isinstance(semitones, TimeMap):
        raise ValueError("pitch_shift: a TimeMap is not a pitch: a time-varying pitch is a PitchCurve of (seconds, semitones) anchors")
    if isinstance(semitones, PitchCurve):
        if formants is not None:
            raise ValueError("pitch_shift: formants='keep' is not available with a PitchCurve (per-frame envelope ratios are not built)")
        _check_link("pitch_shift", link_channels, "spectral", (phase,))
        _check_transients("pitch_shift", transients, "spectral")
        return _pitch_curve(model, audio, semitones, n_fft, hop_length, frames, overlap_frames, stats, osr, sr, res_type, clip_batch, phase,
                            normalize, link_channels, transients)
    stretch, ratio = pitch_ratio(semitones)
    _check_link("pitch_shift", link_channels, "spectral", (phase,))
    _check_transients("pitch_shift", transients, "spectral")
    a = preproc.resample(audio, osr, sr, res_type=res_type) if osr is not None else audio
    a_len = int(a.shape[-1])
    out = reconstruct_track(model, a, n_fft, hop_length, frames, overlap_frames, stats, None, sr, res_type, clip_batch, phase,
                            normalize=False, join="spectral", stretch=stretch, link_channels=link_channels, transients=transients,
                            formant_semitones=0.0 if formants is None else -float(semitones))
    if ratio != 1:
        out = preproc.resample(out, ratio.numerator, ratio.denominator, res_type=res_type)
    if out.shape[-1] >= a_len:
        out = out[..., :a_len]
    else:
        out = torch.nn.functional.pad(out, (0, a_len - out.shape[-1]))
    return peak_normalize(out) if normalize else out.contiguous()


def pitch_lags(sr, fmin, fmax):
    """(tau_min, tau_max) of ``detect_pitch``: max(2, floor(sr / fmax)) and min(1024, ceil(sr / fmin))"""
    sr, fmin, fmax = int(sr), float(fmin), float(fmax)
    if sr < 1 or not (0.0 < fmin < fmax < math.inf):
        raise ValueError(f"detect_pitch: sr {sr} must be positive and 0 < fmin < fmax, got {fmin} and {fmax}")
    tau_min, tau_max = max(2, int(math.floor(sr / fmax))), min(1024, int(math.ceil(sr / fmin)))
    if tau_min >= tau_max:
        raise ValueError(f"detect_pitch: fmin {fmin} .. fmax {fmax} leaves no lags at sr {sr} (tau_min {tau_min}, tau_max {tau_max})")
    return tau_min, tau_max


def _median_log(f0, voiced, median):
    """f0 at voiced frames replaced by the median, in log frequency, of the voiced frames within k +- median // 2 (the mean of the
    two middle ones when their count is even)"""
    half = int(median) // 2
    out = f0.copy()
    if half < 1 or not voiced.any():
        return out
    n = f0.shape[0]
    logf = np.full(n + 2 * half, np.inf)
    logf[half:half + n] = np.where(voiced, np.log(np.where(voiced, f0, 1.0)), np.inf)
    win = np.sort(np.stack([logf[k:k + n] for k in range(2 * half + 1)], axis=1), axis=1)      # the voiced ones first, ascending
    count = np.isfinite(win).sum(axis=1)
    rows = np.flatnonzero(voiced)
    c = count[rows]
    mid = (win[rows, (c - 1) // 2] + win[rows, c // 2]) / 2.0
    out[rows] = np.exp(mid)
    return out


def detect_pitch(audio, sr=16000, osr=None, fmin=50.0, fmax=1000.0, hop_length=256, window=1024, threshold=0.15, median=5,
                 res_type="kaiser_best"):
    """The fundamental frequency of a monophonic take, frame by frame: YIN on the device (ops.pitch_track) -> a ``PitchTrack(times,
    f0, voiced, ap)`` of host arrays (float64, bool).  ``audio``: (samples,) or (channels, samples), numpy or tensor, at ``osr``
    (resampled to ``sr`` on the device, as ``reconstruct_track``) or at ``sr``; stereo is tracked on the channel mean, formed on the
    device.  Lags: ``pitch_lags(sr, fmin, fmax)``; the complete frames of ``window + tau_max`` samples, ``hop_length`` apart.
      times[k] = (k hop_length + window / 2) / sr        the middle of frame k's window, in seconds
      voiced   = isfinite(ap) & (ap < threshold)
      f0       = sr / period at voiced frames, then replaced by the median, in log frequency, of the voiced frames within
                 k +- median // 2 (isolated octave slips go); 0 at unvoiced frames."""
    tau_min, tau_max = pitch_lags(sr, fmin, fmax)
    hop_length, window, median = int(hop_length), int(window), int(median)
    if median < 1:
        raise ValueError(f"detect_pitch: median must be at least 1, got {median}")
    an = _load(audio, osr, sr, res_type)
    with torch.cuda.device(an.a2.device), torch.no_grad():
        mono = an.a2[0] if an.n_ch == 1 else an.a2.mean(dim=0)
        period, ap = ops.pitch_track(mono, None, hop_length, window, tau_min, tau_max, threshold)
        both = torch.stack([period, ap]).cpu().numpy().astype(np.float64)          # the one copy to the host
    period, ap = both[0], both[1]
    times = (np.arange(period.shape[0], dtype=np.float64) * hop_length + window / 2.0) / sr
    with np.errstate(invalid="ignore", divide="ignore"):
        voiced = np.isfinite(ap) & (ap < float(threshold))
        f0 = np.where(voiced, sr / np.where(voiced, period, 1.0), 0.0)
    return PitchTrack(times, _median_log(f0, voiced, median), voiced, ap)


def autotune(model, audio, strength=1.0, scale="chromatic", a4=440.0, retune_ms=50.0, n_fft=2048, hop_length=512, frames=128,
             overlap_frames=32, stats=None, osr=None, sr=16000, res_type="kaiser_best", clip_batch=64, phase="unet", normalize=True, *,
             link_channels=False, transients=None, formants=None, fmin=50.0, fmax=1000.0, threshold=0.15, median=5, return_curve=False):
    """Pitch correction of a monophonic take: ``detect_pitch`` (``fmin``, ``fmax``, ``threshold``, ``median``), then
    ``PitchCurve.correcting`` (``strength``, ``scale``, ``a4``, ``retune_ms``), then ``pitch_shift`` along that curve with the other
    arguments -> float32 device tensor shaped like the input at ``sr``; with ``return_curve=True`` -> (tensor, PitchTrack,
    PitchCurve).  ``strength=0`` is ``pitch_shift`` along the zero curve.  The refusals are the curve path's (``formants="keep"``)."""
    if formants not in FORMANTS:
        raise ValueError(f"autotune: formants must be None or 'keep', got {formants!r}")
    if formants is not None:
        raise ValueError("autotune: formants='keep' is not available with a PitchCurve (per-frame envelope ratios are not built)")
    _check_link("autotune", link_channels, "spectral", (phase,))
    _check_transients("autotune", transients, "spectral")
    a = preproc.resample(audio, osr, sr, res_type=res_type) if osr is not None else audio
    pt = detect_pitch(a, sr, None, fmin, fmax, threshold=threshold, median=median)
    curve = PitchCurve.correcting(pt, strength, scale, a4, retune_ms)
    out = pitch_shift(model, a, curve, n_fft, hop_length, frames, overlap_frames, stats, None, sr, res_type, clip_batch, phase, normalize,
                      link_channels=link_channels, transients=transients)
    return (out, pt, curve) if return_curve else out
