#!/usr/bin/env python3
"""Formant preservation (phasegen.ops.formant_shift, phasegen.track formant_semitones / pitch_shift(formants="keep")) measured in ONE
process over alternating rounds, on the track of tools/lock_bench.py (3-minute stereo at n_fft 2048 / hop 512):

  * pg_formant_shift at the defaults (order 64, hold 16, 2 iterations) on the track's log-magnitude planes, read in place from the
    polar tensor, `out` only, as the pipeline calls it: microseconds, the floating-point operations of the 1 + iters passes (two GEMMs
    each, 2 x 2 bins order per frame and pass), the algorithmic bytes (one plane read, one written) and the rates they come to;
  * the whole ``pitch_shift(+4 semitones, phase="vocoder_locked")`` with and without formants="keep";
  * the quality table through the real chain (STFT, correction, locked vocoder, ISTFT, resampler): the harmonic-amplitude error of a
    shifted vowel against the input's true envelope (tests/_formant_ref.py: played_error_db) over order {32, 64} x hold {0, 8, 16} x
    iters {0, 2}, for shifts of +4 and -4 semitones at two pitches, beside the uncorrected figure.

HIP events around every repetition; every time is the median over the rounds with min..max.  Prints markdown (DESIGN.md section 4.18
holds a copy); --out writes it to a file as well."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from vocoder_bench import STATS, fmt, make_audio, time_ms  # noqa: E402  (puts the package and tests/ on the path)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import _formant_ref as fref  # noqa: E402
from phasegen import ops, track  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=1024, help="C (bins): 1024 = the reference's 2048-point FFT")
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--overlap_frames", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=180.0)
    ap.add_argument("--sr", type=int, default=16000)
    ap.add_argument("--semitones", type=float, default=4.0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", help="also write the markdown to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("formant_bench: needs the GPU (nothing here can be measured on a CPU)")
    if args.rounds < 5:
        sys.exit("formant_bench: at least 5 rounds")
    bins, hop, frames, ov, n_ch = args.width, args.width // 2, args.frames, args.overlap_frames, 2
    n_fft, stretch = 2 * bins, 2.0 ** (args.semitones / 12.0)
    order, hold, iters, eps = min(track.FORMANT_ORDER, bins), track.FORMANT_HOLD, track.FORMANT_ITERS, track.FORMANT_EPS
    audio = make_audio(args.seconds, args.sr, n_ch)
    a_len = audio.shape[1]
    pl = track.spectral_plan(a_len, frames, hop, ov, stretch)

    begin = torch.arange(n_ch, dtype=torch.int64, device="cuda") * a_len
    pol = ops.stft_crops(audio.reshape(-1), begin, begin + a_len, pl.n_src, n_fft, hop, polar=True, stats=STATS)
    out = torch.empty(n_ch, bins, pl.F_src, device="cuda")
    kw = dict(n_fft=n_fft, hop_length=hop, frames=frames, overlap_frames=ov, stats=STATS, phase="vocoder_locked")
    runs = {"kernel": lambda: ops.formant_shift(pol[:, 0], stretch, order, hold, iters, eps, out=out),
            "hold only": lambda: ops.formant_envelope(pol[:, 0], 1, hold, 0, out=out),
            "pitch": lambda: track.pitch_shift(None, audio, args.semitones, **kw),
            "pitch+keep": lambda: track.pitch_shift(None, audio, args.semitones, formants="keep", **kw)}
    inner = {"kernel": 10, "hold only": 10, "pitch": 3, "pitch+keep": 3}
    for fn in runs.values():                                              # warm-up: workspaces, allocator, tables
        fn()
        fn()
    times = {k: [] for k in runs}
    for r in range(args.rounds):
        for name in runs:
            times[name].append(time_ms(runs[name], inner=inner[name]))
        print(f"# round {r}: " + ", ".join(f"{k} {v[-1]:.3f} ms" for k, v in times.items()), flush=True)

    # quality through the real chain, the constants of phasegen.track set for each row
    saved = (track.FORMANT_ORDER, track.FORMANT_HOLD, track.FORMANT_ITERS)
    q = dict(n_fft=2048, hop_length=512, frames=32, overlap_frames=8, phase="vocoder_locked")
    tones = [(f0, st) for f0 in (180.0, 260.0) for st in (4.0, -4.0)]
    waves = {f0: fref.vowel_audio(f0, 2.0) for f0 in (180.0, 260.0)}
    played = lambda y, f0, st: fref.played_error_db(y.cpu().numpy(), f0 * 2.0 ** (st / 12.0))
    plain = [played(track.pitch_shift(None, waves[f0], st, **q), f0, st) for f0, st in tones]
    table = []
    try:
        for o in (32, 64):
            for h in (0, 8, 16):
                for it in (0, 2):
                    track.FORMANT_ORDER, track.FORMANT_HOLD, track.FORMANT_ITERS = o, h, it
                    table.append((o, h, it, [played(track.pitch_shift(None, waves[f0], st, formants="keep", **q), f0, st) for f0, st in tones]))
    finally:
        track.FORMANT_ORDER, track.FORMANT_HOLD, track.FORMANT_ITERS = saved

    cells = n_ch * bins * pl.F_src
    flops = (1 + iters) * 2 * 2.0 * bins * order * n_ch * pl.F_src
    nbytes = 8.0 * cells
    med = lambda k: float(np.median(times[k])) * 1e-3
    lines = [f"{args.seconds:g} s, {n_ch} channels at {args.sr} Hz, n_fft {n_fft}, hop {hop}, {args.semitones:+g} semitones: F_src {pl.F_src}, "
             f"{cells / 1e6:.1f} M cells; {torch.cuda.get_device_name(0)}; {args.rounds} rounds, median (min..max)", "",
             "| kernel | floating-point operations | algorithmic bytes | us | TFLOP/s | TB/s |", "|---|---|---|---|---|---|",
             f"| `pg_formant_shift` order {order}, hold {hold}, {iters} iterations, out only | {flops / 1e9:.2f} G | {nbytes / 1e6:.1f} MB | "
             f"{fmt(times['kernel'], 1e3, 1)} | {flops / med('kernel') / 1e12:.1f} | {nbytes / med('kernel') / 1e12:.2f} |",
             f"| ... order 1, no iteration, env only: the tile traffic and the peak hold | | {nbytes / 1e6:.1f} MB | {fmt(times['hold only'], 1e3, 1)} | | "
             f"{nbytes / med('hold only') / 1e12:.2f} |", "",
             "| whole call, phase=\"vocoder_locked\" | ms |", "|---|---|",
             f"| `pitch_shift(..., {args.semitones:+g})` | {fmt(times['pitch'], 1.0, 3)} |",
             f"| ... with `formants=\"keep\"` | {fmt(times['pitch+keep'], 1.0, 3)} |",
             f"| difference | {fmt([b - a for a, b in zip(times['pitch'], times['pitch+keep'])], 1.0, 3)} |", "",
             "harmonic-amplitude error (dB) of a 2 s vowel after `pitch_shift`, against the input's true envelope, 2048 / 512:", "",
             "| order | hold | iters | " + " | ".join(f"{f0:g} Hz {st:+g} st" for f0, st in tones) + " | mean |", "|---|---|---|" + "---|" * (len(tones) + 1),
             "| uncorrected | | | " + " | ".join(f"{v:.2f}" for v in plain) + f" | {np.mean(plain):.2f} |"]
    lines += [f"| {o} | {h} | {it} | " + " | ".join(f"{v:.2f}" for v in vals) + f" | {np.mean(vals):.2f} |" for o, h, it, vals in table]
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
