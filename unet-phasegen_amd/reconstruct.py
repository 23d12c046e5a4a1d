#!/usr/bin/env python3
"""Whole-track phase reconstruction from the command line: a wav file of any length and rate goes through a trained U-Net as
overlapped clips and comes back as one wav at ``--sr`` with the predicted phase (``phasegen.track.reconstruct_track``).  The
reference's ``demo.py`` stops at dataset clips; flags shared with it keep its names and defaults.

``--stats`` is the ``{genre}_audio_stats.npy`` that ``phasegen.preproc.build_dataset(..., return_stats=True)`` writes beside the
training set: the (mean, std) the model's inputs were normalised with.  Without it the track's own moments are used.
WAV files are written with scipy (float32 PCM), as in ``demo.py``.

``--report PATH`` also measures the result (``phasegen.track.evaluate_track``): SI-SDR, gain-matched SNR, spectral convergence and
log-spectral distance of the track against the input at ``--sr``, for the model's phase and for the comparators of
``--report_phases`` (``zero``: no phase at all, ``original``: the analysis' own phase, i.e. what chunking and stitching alone cost,
``griffinlim``: ``--gl_iters`` Griffin-Lim iterations from noise), written as JSON.  The model still runs once and the wav is the
same file, byte for byte.

``--join spectral`` joins the clips in the spectrogram domain (one phase per frame of the track, one ISTFT with the exact
magnitudes) instead of crossfading their waveforms.  ``--stretch R`` plays the track R times as long at the same pitch and
``--pitch SEMITONES`` shifts its pitch at the same tempo; both imply the spectral join, and neither can be reported against the input.

``--phase vocoder`` takes the phase from the phase vocoder instead of the model (the analysis' own phase, propagated along the output
frames by its measured advance: the standard comparator of a time stretch) and ``--phase zero`` uses none; neither needs ``--weight``,
and ``vocoder`` implies the spectral join.  ``--phase vocoder_locked`` is that vocoder with identity phase locking (only the spectral
peaks advance, every other bin follows its peak): the time stretch to use without weights; it implies the spectral join too.
``--stretch_report PATH`` (with ``--stretch``) measures what a stretched track can be
measured by, spectrogram consistency (``phasegen.track.evaluate_stretch``): spectral convergence and log-spectral distance between
the magnitudes that were imposed and the spectrogram of the result, for ``--phase`` and the other phase sources that need no
weights (and the model's when ``--weight`` is given), written as JSON.

``--phase spsi`` is single-pass spectrogram inversion: a phase from the magnitudes alone (peaks advance by their interpolated
frequency, every other bin follows its peak), the model-free baseline; it needs no ``--weight`` and implies the spectral join, like
the vocoders.  ``--report_phases`` accepts ``spsi`` with ``--join spectral``, and ``--gl_init spsi`` starts the ``griffinlim`` report
phase from that inversion instead of from noise.

``--link_channels`` (with ``--stereo`` and ``--phase vocoder_locked``; for ``--stretch``, ``--pitch`` and ``--stretch_report``) gives
all channels ONE rotation, that of their mean, instead of one each (``phasegen.ops.phase_lock_linked``): the phase difference
between the channels stays the analysis' own, so the stereo image and the sum to mono survive the stretch.  The stretch report then
also holds ``mid_metrics``, the consistency of the channels' mean.

``--transients ola`` (for ``--stretch``, ``--pitch`` and ``--stretch_report``, with every ``--phase``) keeps onsets sharp: the
magnitudes are split into a harmonic and a percussive part by median filtering (``phasegen.ops.hpss``), the harmonic part is
stretched with the chosen phase and the percussive part is moved in the time domain by overlap-add of a 16 ms window
(``phasegen.ops.ola_stretch``), which relocates clicks instead of stretching them.

``--formants keep`` (with ``--pitch``) keeps the timbre where it was: the spectral envelope of every frame is estimated on the device
(``phasegen.ops.formant_shift``) and moved against the shift before the resampling moves it along with the partials, so a voice
shifted up does not turn into a smaller voice.  ``--formant_shift SEMITONES`` moves the envelope alone, at the same pitch and tempo
(implies the spectral join; not with ``--pitch``, ``--formants`` or ``--report``).

``--tempo_map FILE`` (instead of ``--stretch``; not with ``--pitch``) stretches every part of the track at its own rate: the file
holds two columns per line, source seconds and output seconds (``#`` begins a comment), the map is piecewise linear between these
anchors and every segment's stretch must lie within [0.25, 4] (``phasegen.track.TimeMap``).  It implies what ``--stretch`` implies
and works with ``--phase``, ``--link_channels``, ``--transients``, ``--formant_shift`` and ``--stretch_report``.

``--pitch_curve FILE`` (instead of ``--pitch``) shifts the pitch along a curve at the same tempo: the file holds two columns per
line, seconds and semitones (``#`` begins a comment), the transposition is piecewise linear between these anchors, constant past the
last one and within +-24 semitones (``phasegen.track.PitchCurve``): a glide, a vibrato, a correction.  The result has exactly the
input's length at ``--sr``.  It implies the spectral join, works with ``--phase``, ``--link_channels`` and ``--transients`` as
``--pitch`` does, and excludes ``--pitch``, ``--stretch``, ``--tempo_map``, ``--formants``, ``--formant_shift``, ``--report`` and
``--stretch_report``.

``--autotune [STRENGTH]`` corrects the pitch of a monophonic take: the fundamental is tracked frame by frame on the device
(``phasegen.track.detect_pitch``, YIN between ``--fmin`` and ``--fmax`` Hz), every voiced frame is pulled by STRENGTH (0 .. 1,
default 1) of its distance to the nearest note of ``--scale`` (``chromatic``, ``<tonic>:maj`` or ``<tonic>:min``; ``--a4`` tunes the
reference, ``--retune_ms`` sets how fast a note is pulled in) and the take is shifted along that curve as by ``--pitch_curve``, whose
exclusions it shares; it excludes ``--pitch_curve`` itself.  ``--pitch_report FILE`` writes the detected track as JSON (``times``,
``f0``, ``voiced``, ``ap`` and, with ``--autotune``, the ``curve``'s anchors); it also works alone, beside whatever else is written.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


GRID_PHASES = ("vocoder", "vocoder_locked", "spsi")              # computed on the track's frame grid: no weights, spectral join


def main():
    parser = argparse.ArgumentParser(description="Reconstruct the phase of a whole track.")
    parser.add_argument("--weight", default=None, help="a UNetModel.save checkpoint (required for --phase unet)")
    parser.add_argument("--input", required=True, help="wav in")
    parser.add_argument("--output", required=True, help="wav out")
    parser.add_argument("--stats", default=None, help="*_audio_stats.npy of the training set (default: this track's own moments)")
    parser.add_argument("--channels", default=1024, type=int, help="bins = model width")
    parser.add_argument("--n_fft", default=None, type=int, help="default: 2 * channels")
    parser.add_argument("--hop", default=None, type=int, help="default: n_fft / 4")
    parser.add_argument("--frames", default=128, type=int)
    parser.add_argument("--overlap_frames", default=32, type=int)
    parser.add_argument("--sr", default=16000, type=int)
    parser.add_argument("--precision", choices=["fp32", "bf16x3", "bf16"], default="fp32",
                        help="MFMA operand mode of the convolutions (pg_conv_args.precision): fp32 = the reference's arithmetic")
    parser.add_argument("--gpu", default=0, type=int)
    parser.add_argument("--stereo", action="store_true", help="keep the file's channels instead of their mono average")
    parser.add_argument("--report", default=None, metavar="PATH", help="write a JSON quality report of the result against the input")
    parser.add_argument("--report_phases", default="unet,zero,original",
                        help="comma list of phase sources to report: unet, zero, original, griffinlim, spsi (spsi: with --join spectral; "
                             "'unet' is always included)")
    parser.add_argument("--gl_iters", default=250, type=int, help="Griffin-Lim iterations of the 'griffinlim' report phase")
    parser.add_argument("--gl_init", choices=["noise", "spsi"], default="noise",
                        help="where the 'griffinlim' report phase starts: noise (default) or the single-pass inversion of every clip")
    parser.add_argument("--join", choices=["waveform", "spectral"], default=None,
                        help="how overlapped clips become one track: crossfade the clips' waveforms (default), or join their phases "
                             "on the track's frame grid and invert once with the exact magnitudes")
    parser.add_argument("--stretch", default=None, type=float, metavar="R",
                        help="play R times as long at the same pitch, 0.25 <= R <= 4 (implies --join spectral)")
    parser.add_argument("--tempo_map", default=None, metavar="FILE",
                        help="a time-varying stretch: a text file of two columns per line, source seconds and output seconds, piecewise "
                             "linear between them (phasegen.track.TimeMap; instead of --stretch, implies --join spectral)")
    parser.add_argument("--pitch", default=None, type=float, metavar="SEMITONES",
                        help="shift the pitch at the same tempo, within +-24 semitones (implies --join spectral)")
    parser.add_argument("--pitch_curve", default=None, metavar="FILE",
                        help="a time-varying pitch shift at the same tempo: a text file of two columns per line, seconds and semitones, "
                             "piecewise linear between them (phasegen.track.PitchCurve; instead of --pitch, implies --join spectral)")
    parser.add_argument("--autotune", default=None, type=float, nargs="?", const=1.0, metavar="STRENGTH",
                        help="correct the pitch of a monophonic take towards the nearest note of --scale, by STRENGTH of the distance "
                             "(0 .. 1, default 1; phasegen.track.autotune; implies --join spectral)")
    parser.add_argument("--scale", default="chromatic", help="with --autotune: chromatic (default), <tonic>:maj or <tonic>:min, e.g. A:min")
    parser.add_argument("--a4", default=440.0, type=float, help="with --autotune: the frequency of A4 in Hz")
    parser.add_argument("--retune_ms", default=50.0, type=float, help="with --autotune: the time constant with which a note is pulled in (0: at once)")
    parser.add_argument("--fmin", default=50.0, type=float, help="with --autotune or --pitch_report: the lowest fundamental looked for, Hz")
    parser.add_argument("--fmax", default=1000.0, type=float, help="with --autotune or --pitch_report: the highest fundamental looked for, Hz")
    parser.add_argument("--pitch_report", default=None, metavar="FILE",
                        help="write the detected pitch track as JSON: times, f0, voiced, ap and, with --autotune, the curve's anchors")
    parser.add_argument("--phase", choices=["unet", "vocoder", "vocoder_locked", "spsi", "zero"], default="unet",
                        help="where the phase comes from: the model (default), the phase vocoder, plain or with identity phase locking, "
                             "single-pass inversion of the magnitudes alone (all three imply --join spectral), or none")
    parser.add_argument("--stretch_report", default=None, metavar="PATH",
                        help="with --stretch: write a JSON report of the spectrogram consistency of every phase source")
    parser.add_argument("--link_channels", action="store_true",
                        help="with --phase vocoder_locked: one rotation for all channels, that of their mean (keeps the stereo image)")
    parser.add_argument("--transients", choices=["ola"], default=None,
                        help="with --stretch or --pitch: split off the percussive part and move it in the time domain by overlap-add "
                             "(keeps onsets sharp)")
    parser.add_argument("--formants", choices=["keep"], default=None,
                        help="with --pitch: keep the spectral envelope (the formants) where it was instead of moving it with the partials")
    parser.add_argument("--formant_shift", default=None, type=float, metavar="SEMITONES",
                        help="move the spectral envelope alone, within +-24 semitones, at the same pitch (implies --join spectral)")
    args = parser.parse_args()
    if args.phase == "unet" and args.weight is None:
        parser.error("the following arguments are required: --weight")
    if args.autotune is not None:
        for flag in ("pitch", "stretch", "tempo_map", "pitch_curve", "formants", "formant_shift", "report", "stretch_report"):
            if getattr(args, flag) is not None:
                parser.error(f"--autotune is a pitch shift of its own: it excludes --{flag}")
        if args.join == "waveform":
            parser.error("--autotune needs --join spectral")
        if not 0.0 <= args.autotune <= 1.0:
            parser.error("--autotune STRENGTH must be within [0, 1]")
    if args.pitch_curve is not None:
        for flag in ("pitch", "stretch", "tempo_map", "formants", "formant_shift", "report", "stretch_report"):
            if getattr(args, flag) is not None:
                parser.error(f"--pitch_curve is a pitch shift of its own: it excludes --{flag}")
        if args.join == "waveform":
            parser.error("--pitch_curve needs --join spectral")
    if args.stretch is not None and args.pitch is not None:
        parser.error("--stretch and --pitch exclude each other")
    if args.tempo_map is not None and (args.stretch is not None or args.pitch is not None):
        parser.error("--tempo_map is a stretch of its own: it excludes --stretch and --pitch")
    stretched = args.stretch is not None or args.tempo_map is not None
    if args.formants is not None and args.pitch is None:
        parser.error("--formants needs --pitch")
    if args.formant_shift is not None and (args.pitch is not None or args.formants is not None):
        parser.error("--formant_shift moves the formants alone: it excludes --pitch and --formants")
    if args.formant_shift is not None and not -24.0 <= args.formant_shift <= 24.0:
        parser.error("--formant_shift must be within +-24 semitones")
    if args.formant_shift is not None and args.join == "waveform":
        parser.error("--formant_shift needs --join spectral")
    if args.formant_shift is not None and args.report is not None:
        parser.error("--report compares against the input: it does not work with --formant_shift")
    formant_shift = 0.0 if args.formant_shift is None else args.formant_shift
    modified = ((args.stretch is not None and args.stretch != 1.0) or args.pitch is not None or args.tempo_map is not None
                or args.pitch_curve is not None or args.autotune is not None)
    if modified and args.join == "waveform":
        parser.error("--stretch and --pitch need --join spectral")
    if modified and args.report is not None:
        parser.error("--report compares against the input: it works with --join, not with --stretch or --pitch")
    if args.phase in GRID_PHASES and args.join == "waveform":
        parser.error("--phase {} needs --join spectral".format(args.phase))
    if args.phase != "unet" and args.report is not None:
        parser.error("--report measures the model's phase: it needs --phase unet")
    if args.link_channels and args.phase != "vocoder_locked":
        parser.error("--link_channels needs --phase vocoder_locked")
    if args.transients is not None and not stretched and args.pitch is None and args.pitch_curve is None and args.autotune is None:
        parser.error("--transients needs --stretch or --pitch")
    if args.transients is not None and args.report is not None:
        parser.error("--report compares against the input: it does not work with --transients")
    if args.transients is not None and args.join == "waveform":
        parser.error("--transients needs --join spectral")
    if args.stretch_report is not None and not stretched:
        parser.error("--stretch_report needs --stretch")
    if args.stretch_report is not None and args.pitch is not None:
        parser.error("--stretch_report measures the stretched track on the analysed frame grid: it does not work with --pitch")
    if args.stretch_report is not None and args.report is not None:
        parser.error("--report and --stretch_report exclude each other")
    join = ("spectral" if (modified or stretched or args.formant_shift is not None or args.phase in GRID_PHASES) and args.join is None
            else (args.join or "waveform"))
    if args.stretch_report is not None and join != "spectral":
        parser.error("--stretch_report needs --join spectral")
    n_fft = 2 * args.channels if args.n_fft is None else args.n_fft
    hop = n_fft // 4 if args.hop is None else args.hop
    if n_fft != 2 * args.channels:
        parser.error("--n_fft must be 2 * --channels (the model takes n_fft / 2 bins)")

    import numpy as np
    import torch
    from scipy.io import wavfile
    from cycleGAN import UNetModel
    from phasegen import preproc, track

    torch.cuda.set_device(args.gpu)
    model = None
    if args.weight is not None:
        model = UNetModel(args.channels, args.channels * 2, gpu_ids=[args.gpu], precision=args.precision).cuda(args.gpu)
        model.load(args.weight)
    stats = None
    if args.stats is not None:
        mean, std = (float(v) for v in np.load(args.stats))
        stats = (mean, std)
    else:
        print("reconstruct: no --stats given, normalising with this track's own mean and std", file=sys.stderr)
    audio, file_sr = preproc.load_audio(args.input, mono=not args.stereo)
    stretch = 1.0 if args.stretch is None else args.stretch
    if args.tempo_map is not None:
        stretch = track.TimeMap.load(args.tempo_map)

    phases = [p.strip() for p in args.report_phases.split(",") if p.strip()]
    if args.report is not None:
        if "unet" not in phases:
            phases.insert(0, "unet")
        for p in phases:
            if p not in track.REPORT_PHASES:
                parser.error(f"--report_phases: unknown phase {p!r} (expected some of {', '.join(track.REPORT_PHASES)})")
            if p == "spsi" and join != "spectral":
                parser.error("--report_phases: spsi needs --join spectral")

    start = time.time()
    kw = dict(n_fft=n_fft, hop_length=hop, frames=args.frames, overlap_frames=args.overlap_frames, stats=stats, osr=file_sr, sr=args.sr)
    report = None
    stretch_report = None
    pitch_track = pitch_curve = None
    if args.autotune is not None:
        try:
            out, pitch_track, pitch_curve = track.autotune(model, audio, args.autotune, args.scale, args.a4, args.retune_ms, phase=args.phase,
                                                           link_channels=args.link_channels, transients=args.transients, fmin=args.fmin,
                                                           fmax=args.fmax, return_curve=True, **kw)
        except ValueError as e:
            parser.error(f"--autotune: {e}")
    elif args.pitch is not None or args.pitch_curve is not None:
        semitones = args.pitch if args.pitch_curve is None else track.PitchCurve.load(args.pitch_curve)
        out = track.pitch_shift(model, audio, semitones, phase=args.phase, link_channels=args.link_channels, transients=args.transients,
                                formants=args.formants, **kw)
    elif args.stretch_report is not None:
        # (the locked vocoder and spsi are reported when they are asked for; the other modes' reports stay as they were)
        others = [p for p in track.STRETCH_PHASES if p not in (args.phase, "vocoder_locked", "spsi") and (p != "unet" or model is not None)]
        stretch_report = track.evaluate_stretch(model, audio, stretch, phases=[args.phase] + others, return_audio=True,
                                                link_channels=args.link_channels, transients=args.transients,
                                                formant_semitones=formant_shift, **kw)
        out = track.peak_normalize(stretch_report.pop("audio")[args.phase])
    elif args.report is None:
        out = track.reconstruct_track(model, audio, phase=args.phase, join=join, stretch=stretch,
                                      link_channels=args.link_channels, transients=args.transients, formant_semitones=formant_shift, **kw)
    else:
        report = track.evaluate_track(model, audio, phases=phases, gl_iters=args.gl_iters, return_audio=True, join=join, gl_init=args.gl_init, **kw)
        out = track.peak_normalize(report.pop("audio")["unet"])
    if args.pitch_report is not None and pitch_track is None:
        pitch_track = track.detect_pitch(audio, args.sr, file_sr, args.fmin, args.fmax)
    out = out.cpu().numpy()
    took = time.time() - start
    n = out.shape[-1]
    _, _, n_clips = track.track_plan(n, args.frames, hop, args.overlap_frames)
    wavfile.write(args.output, args.sr, np.ascontiguousarray(out.T if out.ndim == 2 else out, dtype=np.float32))
    print("Reconstructed {:.2f} s of audio in {:.3f} s ({} clips).".format(n / args.sr, took, n_clips))
    if pitch_track is not None and args.pitch_report is not None:
        doc = dict(input=os.path.abspath(args.input), sr=args.sr, times=pitch_track.times.tolist(), f0=pitch_track.f0.tolist(),
                   voiced=pitch_track.voiced.tolist(), ap=[None if v != v else v for v in pitch_track.ap.tolist()])
        if pitch_curve is not None:
            doc["curve"] = [list(a) for a in pitch_curve.anchors]
        with open(args.pitch_report, "w") as f:
            json.dump(doc, f, indent=1)
        voiced = pitch_track.voiced
        print("Pitch report: {} of {} frames voiced{}.".format(int(voiced.sum()), voiced.shape[0], "" if not voiced.any() else
              ", f0 {:.1f} .. {:.1f} Hz".format(float(pitch_track.f0[voiced].min()), float(pitch_track.f0[voiced].max()))))
    if report is not None:
        report.update(input=os.path.abspath(args.input), seconds=n / args.sr, flags=vars(args))
        with open(args.report, "w") as f:
            json.dump(report, f, indent=1)
        print("Report: " + "; ".join("{} SI-SDR {:.2f} dB, spectral convergence {:.4f}, LSD {:.2f} dB".format(
            p, m["si_sdr_db"], m["spectral_convergence"], m["lsd_db"]) for p, m in ((p, report["metrics"].get(p)) for p in ("unet", "zero")) if m))
    if stretch_report is not None:
        stretch_report.update(input=os.path.abspath(args.input), seconds=n / args.sr, flags=vars(args))
        with open(args.stretch_report, "w") as f:
            json.dump(stretch_report, f, indent=1)
        print("Stretch report (consistency): " + "; ".join("{} spectral convergence {:.4f}, LSD {:.2f} dB".format(
            p, m["spectral_convergence"], m["lsd_db"]) for p, m in stretch_report["metrics"].items()))
        if "mid_metrics" in stretch_report:
            print("Stretch report (consistency of the channel mean): " + "; ".join("{} spectral convergence {:.4f}".format(
                p, m["spectral_convergence"]) for p, m in stretch_report["mid_metrics"].items()))


if __name__ == "__main__":
    main()
