#!/usr/bin/env python3
"""The phase vocoder (phasegen.track, phase="vocoder") measured in ONE process over alternating rounds:

  * pg_phase_vocoder alone on one synthetic 3-minute stereo track at n_fft 2048 / hop 512 stretched by 1.5, against the bytes it
    moves: the angle and the log-magnitude plane read once, the output plane written once.
  * the whole ``reconstruct_track(join="spectral", stretch=1.5)`` at phase="vocoder" beside phase="zero" (neither needs weights):
    the difference is what the vocoder's phase costs end to end.
  * the floor table: spectrogram consistency (``track.evaluate_stretch``: spectral convergence and log-spectral distance between the
    imposed magnitudes and the spectrogram of the result) of the synthetic melody of tests/_vocoder_ref.py at stretch 1.5 with the
    track's own moments, for reset_below in {0, 0.01, 0.05, 0.2} and for phase="zero".  ``track.VOCODER_RESET_BELOW`` is the floor
    with the smallest spectral convergence here.

HIP events around every repetition; every figure is the median over the rounds with min..max.  Prints markdown (DESIGN.md section
4.11 holds a copy); --out writes it to a file as well."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "unet-phasegen_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import _vocoder_ref  # noqa: E402
from phasegen import ops, track  # noqa: E402

STATS = (0.0, 3.0)
FLOORS = (0.0, 0.01, 0.05, 0.2)


def time_ms(fn, inner=1):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def make_audio(seconds, sr, n_ch, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    n = int(seconds * sr)
    t = torch.arange(n, device="cuda", dtype=torch.float64)
    tones = 0.3 * torch.sin(2 * np.pi * 440.0 / sr * t) + 0.2 * torch.sin(2 * np.pi * 1730.0 / sr * t + 0.5)
    return (0.1 * torch.randn(n_ch, n, device="cuda", generator=g) + tones.float()[None]).contiguous()


def fmt(vals, scale=1.0, prec=3):
    return f"{statistics.median(vals) * scale:.{prec}f} ({min(vals) * scale:.{prec}f}..{max(vals) * scale:.{prec}f})"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=1024, help="C (bins): 1024 = the reference's 2048-point FFT")
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--overlap_frames", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=180.0)
    ap.add_argument("--channels", type=int, default=2)
    ap.add_argument("--sr", type=int, default=16000)
    ap.add_argument("--stretch", type=float, default=1.5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", help="also write the markdown to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("vocoder_bench: needs the GPU (nothing here can be measured on a CPU)")
    if args.rounds < 5:
        sys.exit("vocoder_bench: at least 5 rounds")
    bins, hop, frames, ov, n_ch, stretch = args.width, args.width // 2, args.frames, args.overlap_frames, args.channels, args.stretch
    n_fft = 2 * bins
    audio = make_audio(args.seconds, args.sr, n_ch)
    a_len = audio.shape[1]
    pl = track.spectral_plan(a_len, frames, hop, ov, stretch)
    kw = dict(n_fft=n_fft, hop_length=hop, frames=frames, overlap_frames=ov, stats=STATS, sr=args.sr, normalize=False, join="spectral", stretch=stretch)

    # the kernel alone, on the planes the pipeline hands it
    begin = torch.arange(n_ch, dtype=torch.int64, device="cuda") * a_len
    pol = ops.stft_crops(audio.reshape(-1), begin, begin + a_len, pl.n_src, n_fft, hop, polar=True, stats=STATS)
    out = torch.empty(n_ch, bins, pl.F_out, device="cuda")
    pv_bytes = 4 * (2 * n_ch * bins * pl.F_src + out.numel())
    runs = {"kernel": lambda: ops.phase_vocoder(pol[:, 1], pl.F_out, 1.0 / stretch, logmag=pol[:, 0], reset_below=track.VOCODER_RESET_BELOW, out=out),
            "vocoder": lambda: track.reconstruct_track(None, audio, phase="vocoder", **kw),
            "zero": lambda: track.reconstruct_track(None, audio, phase="zero", **kw)}
    for fn in runs.values():                                              # warm-up: workspaces, allocator
        fn()
        fn()
    times = {k: [] for k in runs}
    for r in range(args.rounds):
        times["kernel"].append(time_ms(runs["kernel"], inner=10))
        for name in ("vocoder", "zero"):
            times[name].append(time_ms(runs[name]))
        print(f"# round {r}: " + ", ".join(f"{k} {v[-1]:.3f} ms" for k, v in times.items()), flush=True)

    # the floor table on the melody, the track's own moments
    melody = _vocoder_ref.melody()
    table = []
    for floor in FLOORS:
        rep = track.evaluate_stretch(None, melody, 1.5, phases=("vocoder", "zero") if not table else ("vocoder",), reset_below=floor)
        if not table:
            zero = rep["metrics"]["zero"]
        table.append((floor, rep["metrics"]["vocoder"]))
    best = min(table, key=lambda fm: fm[1]["spectral_convergence"])[0]

    lines = [f"{args.seconds:g} s, {n_ch} channels at {args.sr} Hz, n_fft {n_fft}, hop {hop}, stretch {stretch:g}: F_src {pl.F_src}, F_out {pl.F_out}, "
             f"{n_ch * bins} rows; {torch.cuda.get_device_name(0)}; {args.rounds} rounds, median (min..max)", "",
             "| kernel | bytes moved | us | TB/s |", "|---|---|---|---|",
             f"| `pg_phase_vocoder` (angle and log-magnitude in, phase out) | {pv_bytes / 1e6:.1f} MB | {fmt(times['kernel'], 1e3, 1)} | "
             f"{fmt([pv_bytes / t / 1e9 for t in times['kernel']])} |", "",
             f"| `reconstruct_track(join=\"spectral\", stretch={stretch:g})`, no model | ms |", "|---|---|",
             f"| phase=\"vocoder\" | {fmt(times['vocoder'], 1.0, 2)} |", f"| phase=\"zero\" | {fmt(times['zero'], 1.0, 2)} |", "",
             "| melody (6 s, 16 kHz) at stretch 1.5, own moments | spectral convergence | LSD dB |", "|---|---|---|"]
    lines += [f"| vocoder, reset_below {floor:g} | {m['spectral_convergence']:.4f} | {m['lsd_db']:.3f} |" for floor, m in table]
    lines += [f"| zero phase | {zero['spectral_convergence']:.4f} | {zero['lsd_db']:.3f} |", "",
              f"smallest spectral convergence at reset_below {best:g}; track.VOCODER_RESET_BELOW is {track.VOCODER_RESET_BELOW:g}"]
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
